"""CPU: the guard-band checker of tests/guard_bands.py sees what it must see, on CPU tensors.

A clean buffer passes; one byte planted in the front band, in the back band and in the row padding is reported at its
offset relative to the view and on its side; an offset view reports relative to itself; item padding is watched; and the
inputs of ``surrounded_in`` hold the array where it belongs and the poison everywhere else."""
import numpy as np
import pytest
import torch

import guard_bands as G

CPU = torch.device("cpu")


def _plant(check, byte_offset_from_view):
    """Flip one byte at an offset relative to the view's first element."""
    i = check.layout.start + byte_offset_from_view
    check.raw[i] = int(check.raw[i]) ^ 0x5A


def test_clean_buffer_passes_and_layout_is_as_documented():
    view, check = G.banded_out(torch, CPU, (2, 5, 7), np.float32, pitch_extra=3, item_extra=11)
    check()
    assert tuple(view.shape) == (2, 5, 7) and view.stride() == (5 * 10 + 11, 10, 1)
    assert view.row_stride == 40 and view.item_stride == 4 * (50 + 11)
    lay = check.layout
    assert lay.band == 4096 and lay.start == 4096 and lay.total >= lay.end + lay.band
    # the logical elements hold the pattern too (a NaN with its payload), and writing all of them leaves the rest alone
    assert np.array_equal(view.contiguous().numpy().view(np.uint32), np.full((2, 5, 7), G.PATTERN, np.uint32))
    view.copy_(torch.arange(70, dtype=torch.float32).reshape(2, 5, 7))
    check()
    assert np.array_equal(view.numpy(), np.arange(70, dtype=np.float32).reshape(2, 5, 7))


def test_band_is_two_rows_plus_256_for_wide_rows():
    _, check = G.banded_out(torch, CPU, (1, 2, 3000, 2), np.float32, row_dims=2)
    want = 2 * 24000 + 256          # then rounded up to a multiple of 256 B, which keeps the view's start aligned
    assert want <= check.layout.band == G.band_bytes(24000) < want + 256 and check.layout.band % 256 == 0
    assert G.band_bytes(1) == 4096


@pytest.mark.parametrize("where,offset,side", [
    ("front", -1, "front band"), ("front_far", -4096, "front band"),
    ("back", 4 * (4 * 10 + 7), "back band"),            # the byte after the last logical element (row 4, column 6)
    ("pitch", 4 * 7, "padding inside the view"),        # the first padding byte of row 0
    ("pitch_last", 4 * (3 * 10 + 9) + 3, "padding inside the view")])
def test_one_planted_byte_is_reported_at_its_offset(where, offset, side):
    view, check = G.banded_out(torch, CPU, (5, 7), np.float32, pitch_extra=3)
    view.fill_(1.0)
    check()
    _plant(check, offset)
    with pytest.raises(AssertionError) as e:
        check()
    msg = str(e.value)
    assert f"first at byte offset {offset} relative to the view ({side}" in msg and msg.startswith("1 byte(s)")


def test_logical_bytes_are_not_guarded():
    view, check = G.banded_out(torch, CPU, (5, 7), np.uint8, pitch_extra=3)
    _plant(check, 10 * 4 + 6)     # row 4, column 6: the last logical byte
    check()


def test_offset_view_reports_relative_to_itself():
    view, check = G.banded_out(torch, CPU, (3, 4), np.int16, pitch_extra=2, offset_elems=3)
    assert check.layout.start == 4096 + 6 and view.data_ptr() == check.raw.data_ptr() + 4096 + 6
    check()
    check.raw[4096 + 5] = 0          # the byte in front of the offset view
    with pytest.raises(AssertionError, match=r"first at byte offset -1 relative to the view \(front band"):
        check()
    view2, check2 = G.banded_out(torch, CPU, (3, 4), np.int16, pitch_extra=2, offset_elems=3)
    _plant(check2, 2 * (2 * 6 + 4))  # one element past the end of the last row
    with pytest.raises(AssertionError, match=r"first at byte offset 32 relative to the view \(back band"):
        check2()


def test_item_padding_is_guarded_and_counts_are_reported():
    view, check = G.banded_out(torch, CPU, (2, 3, 4, 2), np.float32, row_dims=2, item_extra=5)
    assert view.stride() == (29, 8, 2, 1)
    _plant(check, 4 * 24)
    _plant(check, 4 * 28 + 3)
    with pytest.raises(AssertionError, match=r"^2 byte\(s\).*first at byte offset 96 relative to the view \(padding"):
        check()


@pytest.mark.parametrize("dtype,poison", [(np.uint8, 0xFF), (np.uint16, 0x8000), (np.int16, -0x8000),
                                          (np.float32, np.nan), (np.float32, -1e30)])
def test_surrounded_in_places_the_array_in_poison(dtype, poison):
    arr = (np.arange(2 * 3 * 5).reshape(2, 3, 5) % 100 + 1).astype(dtype)
    t = G.surrounded_in(torch, CPU, arr, poison, pitch_extra=4, item_extra=6, offset_elems=1)
    it = arr.dtype.itemsize
    assert t.row_stride == 9 * it and t.item_stride == (27 + 6) * it
    assert np.array_equal(t.contiguous().numpy().view(dtype), arr)
    whole = t._base.numpy().view(dtype) if t._base is not None else None
    assert whole is not None
    start = 4096 // it + 1
    inside = np.zeros(whole.size, bool)
    for i in range(2):
        for y in range(3):
            o = start + i * 33 + y * 9
            inside[o:o + 5] = True
    rest = whole[~inside]
    assert rest.size >= 2 * 4096 // it
    assert np.isnan(rest).all() if isinstance(poison, float) and np.isnan(poison) else (rest == dtype(poison)).all()


def test_banded_items_share_one_allocation_and_name_the_item():
    views, check = G.banded_items(torch, CPU, [(2, 3, 2), (4, 5, 2), (1, 1, 2)], np.float32, pitch_extra=6, row_dims=2)
    check()
    assert [tuple(v.shape) for v in views] == [(2, 3, 2), (4, 5, 2), (1, 1, 2)]
    assert views[1].row_stride == 4 * 16 and all((v.data_ptr() - check.raw.data_ptr()) % 256 == 0 for v in views)
    lays = check.layouts
    assert all(b.start - a.end >= 4096 for a, b in zip(lays, lays[1:])) and len(check.raw) >= lays[-1].end + 4096
    for v in views:
        v.fill_(2.0)
    check()
    _plant(check, lays[1].start - lays[0].start + 4 * 10)       # item 1: the first padding byte of its row 0
    with pytest.raises(AssertionError, match=r"first at byte offset 40 relative to the view of item 1 \(padding"):
        check()
    views, check = G.banded_items(torch, CPU, [(2, 3), (4, 5)], np.uint8)
    _plant(check, check.layouts[1].start - check.layouts[0].start - 1)
    with pytest.raises(AssertionError, match=r"first at byte offset -1 relative to the view of item 1 \(front band"):
        check()
