"""CPU: the float work-list entries are exported and bound as declared, and the host list refuses what the Python layer
checks before any device work (non-finite values, dtypes that differ within a pair, depths cv2 refuses)."""
import threading

import numpy as np
import pytest

from nsof.errors import NsofValueError

F32_LIST_ENTRIES = ("nsof_farneback_f32_batch", "nsof_farneback_f32_batch_desc_dev", "nsof_farneback_f32_roi_sequence_dev")


def test_float_worklist_entries_are_exported_and_bound(nsof_lib):
    import ctypes as C
    from nsof import _lib
    lib = _lib.load()
    for name in F32_LIST_ENTRIES:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    # the same argument lists as the 8-bit twins (nsof_pair_desc_f32 has nsof_pair_desc's layout)
    for name in F32_LIST_ENTRIES:
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_f32_", "_u8_")], name
    assert C.sizeof(_lib.PairDesc) == 56
    import nsof
    assert callable(nsof.farneback_pairs_f32_dev) and callable(nsof.farneback_roi_sequence_f32_dev)


class _HostOnlyContext:
    """What a float host list touches before the native call: the context's lock and its conversion buffer (a plain
    array here).  Anything else -- the library, the native context -- fails the test."""

    def __init__(self):
        self.lock = threading.RLock()
        self._nsof_f32_stage = np.empty(1 << 16, np.uint8)

    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name}) before the input was refused")


@pytest.mark.parametrize("case", ["nan", "inf", "f64_overflow", "u16_with_nan_f32", "mixed_pair", "bool", "three_channel"])
def test_host_list_refusals_before_device_work(nsof_lib, case):
    from nsof.farneback import PARAMS_A, farneback_pairs
    a = np.full((16, 24), 3, np.float32)
    b = a.copy()
    other = (np.zeros((8, 8), np.uint16), np.zeros((8, 8), np.uint16))
    if case == "nan":
        b[3, 4] = np.nan
    elif case == "inf":
        a, b = a.astype(np.float64), b.astype(np.float64)
        a[0, 0] = -np.inf
    elif case == "f64_overflow":   # finite in float64, inf after the conversion to float32
        a, b = a.astype(np.float64), b.astype(np.float64)
        b[1, 1] = 1e39
    elif case == "u16_with_nan_f32":   # a NaN in the LAST pair of a list
        a[0, 5] = np.nan
        other = (np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8))
    elif case == "mixed_pair":
        b = b.astype(np.uint16)
    elif case == "bool":
        a, b = a.astype(bool), b.astype(bool)
    elif case == "three_channel":
        a, b = np.zeros((16, 24, 3), np.uint16), np.zeros((16, 24, 3), np.uint16)
    with pytest.raises(NsofValueError):
        farneback_pairs([other, (a, b)], PARAMS_A, ctx=_HostOnlyContext())


def test_host_conversion_buffer_is_bounded(nsof_lib, monkeypatch):
    """Frames beyond the page-locked buffer's cap are converted into ordinary arrays; values are astype(np.float32)."""
    from nsof import farneback as F
    ctx = _HostOnlyContext()
    stage = ctx._nsof_f32_stage
    monkeypatch.setattr(F, "_F32_STAGE_CAP", stage.nbytes)
    rng = np.random.default_rng(3)
    pairs = [(rng.integers(0, 65536, (40, 60)).astype(np.uint16), rng.integers(0, 65536, (40, 60)).astype(np.uint16))
             for _ in range(12)]   # 12 * 2 * 9600 B > 64 KiB
    out = F._f32_host_frames(pairs, ctx)
    assert ctx._nsof_f32_stage is stage   # not grown past the cap
    lo, hi = stage.ctypes.data, stage.ctypes.data + stage.nbytes
    inside = [lo <= a.ctypes.data < hi for pq in out for a in pq]
    assert any(inside) and not all(inside)
    for (a, b), (fa, fb) in zip(pairs, out):
        assert fa.dtype == np.float32 and np.array_equal(fa, a.astype(np.float32)) and np.array_equal(fb, b.astype(np.float32))
