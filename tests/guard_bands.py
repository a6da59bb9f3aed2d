"""Guard bands for tests of device entries: outputs that sit inside a larger allocation the test owns, inputs whose
surroundings hold a chosen poison.

An entry writes no byte outside the logical elements of its outputs and its results do not depend on memory outside the
logical elements of its inputs (include/nsof.h, "Layout rule").  A comparison with a reference sees neither violation
when the output tensor is exactly as large as the result and the input is dense or zero padded: a store past the end
lands in somebody else's allocation, a load outside the frame reads something harmless.  Here

* ``banded_out`` hands out a view of the wanted shape in the middle of ONE allocation filled with a 32-bit pattern
  (written through an integer view, so the NaN it spells as a float keeps its payload).  Row padding, padding between
  the items of a stack and a band of ``max(4096 B, two rows + 256 B)`` before and after the view all hold the pattern;
  ``check()`` asserts that they still do, byte for byte, and names the first dirty byte relative to the view.
* ``surrounded_in`` uploads an array with the same kind of band, row padding and item padding around it, all holding
  ``poison``: a result that changes with the poison was computed from memory outside the frame.

Nothing is ever placed flush against the end of an allocation and nothing relies on a fault: an overrun shows as changed
band bytes.  Works on CPU tensors as well (tests/test_guard_bands_cpu.py proves the checker there).

Layout of both: ``shape = lead + (rows,) + row``, where the last ``row_dims`` dimensions are one contiguous row
(``row_dims=2`` for an interleaved flow row ``(w, 2)``).  ``pitch_extra`` elements follow every row, ``item_extra``
elements follow every item (an item = one index of the dimension before ``rows``; needs ``len(lead) >= 1``), and the
view starts ``offset_elems`` elements past the 256-byte aligned end of the front band.
"""
import numpy as np

PATTERN = 0x7FE5B3C9          # as float32: a quiet NaN with a payload; all four bytes differ and none is 0x00 / 0xFF
_PATTERN_BYTES = np.frombuffer(np.uint32(PATTERN).tobytes(), np.uint8)
MIN_BAND = 4096


def _prod(t):
    n = 1
    for v in t:
        n *= int(v)
    return n


def band_bytes(row_bytes):
    """max(4096 B, two rows + 256 B), rounded up to 256 B so that the view's aligned start stays 256-byte aligned."""
    return (max(MIN_BAND, 2 * int(row_bytes) + 256) + 255) // 256 * 256


class _Layout:
    """Element strides and byte extents of a view of `shape` with padded rows and items inside a banded allocation."""

    def __init__(self, shape, itemsize, row_dims, pitch_extra, item_extra, offset_elems, origin=0):
        shape = tuple(int(s) for s in shape)
        assert 1 <= row_dims < len(shape), "shape needs a rows dimension in front of the row"
        assert pitch_extra >= 0 and item_extra >= 0 and offset_elems >= 0
        self.shape, self.itemsize = shape, itemsize
        row, rows, lead = shape[-row_dims:], shape[-row_dims - 1], shape[:-row_dims - 1]
        assert item_extra == 0 or lead, "item_extra needs a stack of items"
        self.row_elems = _prod(row)
        self.pitch = self.row_elems + pitch_extra                 # elements from one row to the next
        self.item = rows * self.pitch + item_extra                # elements from one item to the next
        strides = []
        s = 1
        for d in reversed(row):
            strides.append(s)
            s *= d
        strides.append(self.pitch)
        s = self.item
        for d in reversed(lead):
            strides.append(s)
            s *= d
        self.strides = tuple(reversed(strides))                   # in elements
        self.span = 1 + sum((d - 1) * st for d, st in zip(shape, self.strides)) if _prod(shape) else 0
        self.band = band_bytes(self.row_elems * itemsize)
        assert origin % 256 == 0
        self.origin = origin                                      # where this view's front band starts
        self.start = origin + self.band + offset_elems * itemsize   # byte offset of the view in the allocation
        self.end = self.start + self.span * itemsize              # first byte after the view's last logical element
        self.total = (self.end + self.band + 7) // 8 * 8          # an allocation that ends with this view's back band

    def mark_logical(self, mask):
        """Sets mask (one bool per byte of the allocation) at the bytes of the view's logical elements."""
        it = self.itemsize
        elems = np.lib.stride_tricks.as_strided(mask[self.start:], self.shape + (it,),
                                                tuple(s * it for s in self.strides) + (1,))
        elems[...] = True


def _torch_dtype(torch, dtype):
    if isinstance(dtype, torch.dtype):
        return dtype
    return {"uint8": torch.uint8, "int8": torch.int8, "int16": torch.int16, "int32": torch.int32, "int64": torch.int64,
            "float32": torch.float32, "float64": torch.float64,
            "uint16": torch.int16}[np.dtype(dtype).name]   # (16-bit payloads travel as int16: same bytes)


def _sync(torch, dev):
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()


def _tag(view, lay):
    """The byte strides an entry is given, as attributes of the view."""
    view.row_stride = lay.pitch * lay.itemsize
    view.item_stride = lay.item * lay.itemsize


def _banded(torch, dev, lays, tdt):
    """The views of `lays` (laid out one after the other) in one pattern-filled allocation, and its checker."""
    total = lays[-1].total
    itemsize = lays[0].itemsize
    raw = torch.empty(total, dtype=torch.uint8, device=dev)
    raw.view(torch.int32).fill_(int(np.uint32(PATTERN).astype(np.int32)))
    views = []
    mask = np.zeros(total, bool)
    for lay in lays:
        assert lay.start % itemsize == 0
        view = raw.view(tdt).as_strided(lay.shape, lay.strides, lay.start // itemsize)
        _tag(view, lay)
        lay.mark_logical(mask)
        views.append(view)
    _sync(torch, dev)
    want = np.tile(_PATTERN_BYTES, total // 4)

    def check():
        _sync(torch, dev)
        got = raw.cpu().numpy()
        dirty = (got != want) & ~mask
        if dirty.any():
            first = int(np.flatnonzero(dirty)[0])
            k = max(i for i, lay in enumerate(lays) if lay.origin <= first)
            lay = lays[k]
            side = ("front band" if first < lay.start else "back band" if first >= lay.end else "padding inside the view")
            raise AssertionError(
                f"{int(dirty.sum())} byte(s) outside the logical elements were written: first at byte offset "
                f"{first - lay.start} relative to the view{f' of item {k}' if len(lays) > 1 else ''} ({side}; the view spans "
                f"{lay.end - lay.start} bytes, row pitch {lay.pitch * itemsize} B, item pitch {lay.item * itemsize} B): "
                f"0x{int(got[first]):02x} where the pattern has 0x{int(want[first]):02x}")

    check.raw, check.layouts, check.layout = raw, lays, lays[0]
    return views, check


def banded_out(torch, dev, shape, dtype, *, pitch_extra=0, offset_elems=0, item_extra=0, row_dims=1):
    """-> (view, check).  `view`: a tensor of `shape` / `dtype` on `dev` inside one larger allocation (see the module
    doc); its logical elements hold the pattern too, so an element the entry never wrote shows in the comparison with
    the reference.  `check()` synchronises and asserts that every byte outside the logical elements still holds the
    pattern."""
    tdt = _torch_dtype(torch, dtype)
    itemsize = torch.empty((), dtype=tdt).element_size()
    views, check = _banded(torch, dev, [_Layout(shape, itemsize, row_dims, pitch_extra, item_extra, offset_elems)], tdt)
    return views[0], check


def banded_items(torch, dev, shapes, dtype, *, pitch_extra=0, offset_elems=0, row_dims=1):
    """-> (views, check): one view per shape, one after the other in ONE allocation, each with its own padded rows and a
    band between neighbours (the outputs of a work list whose items differ in shape).  `check()` names the item."""
    tdt = _torch_dtype(torch, dtype)
    itemsize = torch.empty((), dtype=tdt).element_size()
    lays, origin = [], 0
    for shape in shapes:
        lays.append(_Layout(shape, itemsize, row_dims, pitch_extra, 0, offset_elems, origin))
        origin = (lays[-1].end + 255) // 256 * 256
    return _banded(torch, dev, lays, tdt)


def surrounded_in(torch, dev, array, poison, *, pitch_extra=0, item_extra=0, offset_elems=0, row_dims=1):
    """-> a tensor view on `dev` holding `array` (its shape, rows padded by `pitch_extra`, items by `item_extra`
    elements, starting `offset_elems` elements past an aligned address) whose band, row padding and item padding all
    hold `poison`, a scalar of the array's dtype.  uint16 arrays come back as int16 tensors (the same bytes)."""
    array = np.asarray(array)
    lay = _Layout(array.shape, array.dtype.itemsize, row_dims, pitch_extra, item_extra, offset_elems)
    assert lay.total % array.dtype.itemsize == 0 and lay.start % array.dtype.itemsize == 0
    host = np.full(lay.total // array.dtype.itemsize, poison, array.dtype)
    np.lib.stride_tricks.as_strided(host[lay.start // array.dtype.itemsize:], array.shape,
                                    tuple(s * array.dtype.itemsize for s in lay.strides))[...] = array
    tdt = _torch_dtype(torch, array.dtype)
    npview = host.view(np.int16) if array.dtype == np.uint16 else host
    buf = torch.from_numpy(npview).to(dev)
    if buf.data_ptr() == npview.__array_interface__["data"][0]:
        buf = buf.clone()   # a CPU tensor must own its bytes
    view = buf.view(tdt).as_strided(lay.shape, lay.strides, lay.start // array.dtype.itemsize)
    _tag(view, lay)
    _sync(torch, dev)
    return view

