"""CPU: the host side of the mapped frame-driven path -- ``variability_maps(trials=)``, the plane helper's rejections, the
NumPy gate statistics on a hand-written case, the new symbols, and ``simulate_frames_dev(param_maps=)`` refusing a host
array before any device call.  None of it needs a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["nsof_accum_frames_f64_maps_dev", "nsof_accum_frames_f64_maps", "nsof_gate_stats_dev"]


def test_new_entries_are_declared_exported_and_bound(nsof_lib):
    from nsof import _lib
    header = open(os.path.join(ROOT, "include", "nsof.h")).read()
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.nsof_abi_version() == 3 and re.search(r"#define NSOF_ABI_VERSION 3\b", header)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_variability_trials_are_the_seeds_in_turn(nsof_lib, dtype):
    from nsof.accumulator import variability_maps
    sig = dict(koff=0.1, Ron=0.1, wini=0.5, voff=0.3)
    p = dict(nsof_lib.PARAMS, koff=40.0)
    got = variability_maps(5, 7, sig, p, seed=11, trials=4, dtype=dtype)
    assert set(got) == set(sig)
    for t in range(4):
        one = variability_maps(5, 7, sig, p, seed=11 + t, dtype=dtype)
        for k in sig:
            assert got[k].shape == (4, 5, 7) and got[k].dtype == dtype
            assert np.array_equal(got[k][t], one[k]), (k, t)
    assert not np.array_equal(got["koff"][0], got["koff"][1])            # the trials differ
    # without trials= nothing changed: 2-D float32 planes
    assert variability_maps(5, 7, sig, p, seed=11)["koff"].shape == (5, 7)
    assert variability_maps(5, 7, sig, p, seed=11)["koff"].dtype == np.float32
    # float64 planes are the unrounded values: a spread of 0 is the nominal value itself (51.03 is no float32)
    z = variability_maps(2, 3, dict(koff=0.0), None, trials=2, dtype=np.float64)["koff"]
    assert (z == 51.03).all() and float(np.float32(51.03)) != 51.03
    for bad in (0, -1, 2.0, True):
        with pytest.raises(nsof_lib.error):
            variability_maps(2, 2, sig, trials=bad)


def test_plane_helper(nsof_lib):
    from nsof import _lib
    from nsof.accumulator import _PARAM_KEYS, frame_param_maps_arg
    assert frame_param_maps_arg(None) == (1, [])
    assert frame_param_maps_arg({}) == (1, [])
    a32 = np.full((3, 4), 0.25, np.float32)
    a64 = np.arange(24, dtype=np.float64).reshape(2, 3, 4) + 1
    trials, maps = frame_param_maps_arg(dict(Ron=a64, son=a32), (3, 4))
    assert trials == 2 and [k for k, _ in maps] == ["son", "Ron"]           # the library's key order
    assert [k for k in _PARAM_KEYS if k in ("son", "Ron")] == ["son", "Ron"]
    son, ron = maps[0][1], maps[1][1]
    assert son.dtype == ron.dtype == np.float64 and son.flags.c_contiguous and ron.flags.c_contiguous
    assert son.shape == (1, 3, 4) and ron.shape == (2, 3, 4)               # shared by the trials / one per trial
    assert np.array_equal(son[0], a32.astype(np.float64)) and np.array_equal(ron, a64)
    assert frame_param_maps_arg(dict(son=a32))[0] == 1                      # every plane 2-D: one trial
    assert frame_param_maps_arg(dict(son=a32[None]))[1][0][1].shape == (1, 3, 4)

    def refused(maps, shape=(3, 4)):
        with pytest.raises(nsof_lib.error) as e:
            frame_param_maps_arg(maps, shape)
        assert isinstance(e.value, ValueError)
        return e.value
    assert "won" in str(refused(dict(won=a32)))                              # not a device parameter
    assert "dt" in str(refused(dict(dt=a32)))
    refused([("son", a32)])                                                  # not a mapping
    assert refused(dict(son=np.zeros((4, 3)))).status == _lib.NSOF_ESHAPE    # transposed
    assert refused(dict(son=np.zeros(12))).status == _lib.NSOF_ESHAPE        # 1-D
    assert refused(dict(son=np.zeros((1, 2, 3, 4)))).status == _lib.NSOF_ESHAPE
    assert refused(dict(son=np.zeros((0, 3, 4)))).status == _lib.NSOF_ESHAPE
    assert refused(dict(son=np.zeros((2, 3, 5)))).status == _lib.NSOF_ESHAPE
    e = refused(dict(son=np.zeros((2, 3, 4)), Ron=np.ones((3, 3, 4))))       # differing trial counts
    assert e.status == _lib.NSOF_ESHAPE and "2" in str(e) and "3" in str(e)
    refused(dict(son=[["a", "b"]]), None)
    for bad in (np.nan, np.inf, -np.inf):
        b = a64.copy()
        b[1, 2, 3] = bad
        msg = str(refused(dict(Ron=b)))
        assert "Ron" in msg and "trial 1" in msg and "row 2" in msg and "column 3" in msg


def test_numpy_gate_stats_hand_case(nsof_lib):
    from nsof import gating
    # gray(I) = uint8(clip(-3366 / log10(I) - 306, 0, 255)): 1e-6 A -> 255, 7e-7 A -> 240 (below 245), 1e-7 A -> 174
    assert list(gating.current_to_gray(np.array([1e-6, 7e-7, 1e-7]))) == [255, 240, 174]
    on, off = 1e-6, 7e-7
    nominal = np.array([[[on, off], [off, off]]])                          # F = 1, 2 x 2
    current = np.array([[[[on, off], [off, off]]],                        # trial 0: the nominal map
                        [[[off, on], [off, off]]],                        # trial 1: two cells differ
                        [[[on, on], [on, on]]]])                          # trial 2: three cells differ
    counts, flips = gating.gate_stats(current, nominal, 245)
    assert counts.dtype == np.int32 and flips.dtype == np.int32
    assert counts.tolist() == [[[2, 2], [1, 1]]]
    assert flips.tolist() == [[0], [2], [3]]
    with pytest.raises(ValueError):
        gating.gate_stats(current, nominal[0], 245)


def test_device_entry_refuses_a_host_array_first(nsof_lib):
    """No context is passed and none may be made: the refusal comes before any device call."""
    from nsof import _lib
    maps = dict(koff=np.full((4, 4), 50.0))
    with pytest.raises(nsof_lib.error) as e:
        nsof_lib.simulate_frames_dev(np.zeros((3, 4, 4)), param_maps=maps)
    assert isinstance(e.value, ValueError) and e.value.status == _lib.NSOF_EINVAL
    # the host entry's helper refuses before a context exists as well
    with pytest.raises(nsof_lib.error) as e:
        nsof_lib.simulate_frames(np.zeros((3, 4, 4)), param_maps=dict(koff=np.zeros((5, 4))))
    assert e.value.status == _lib.NSOF_ESHAPE
