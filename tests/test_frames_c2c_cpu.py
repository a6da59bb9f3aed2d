"""CPU: the host side of the frame-driven run's cycle-to-cycle write noise and pair-index origin
(``nsof_accum_frames_f64_c2c*``, ``simulate_frames*(trials=, c2c=, first_pair=)``, ``gating_variability_dev(c2c=)``) -- the new
symbols, the refusals that come before any context exists, the restatement's self-checks, and the conditions on the inputs
of tests/test_frames_c2c_gpu.py without which a test there could pass vacuously.  No GPU is touched."""
import os
import re

import numpy as np
import pytest

import accum_c2c_ref as N  # noqa: N812
import accum_params_ref as R  # noqa: N812
import frames_c2c_ref as Z  # noqa: N812
from test_accum_c2c_cpu import BAD_C2C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nsof_accum_frames_f64_c2c_dev", "nsof_accum_frames_f64_c2c")


def test_new_symbols_are_declared_exported_and_bound(nsof_lib):
    from nsof import _lib
    header = open(os.path.join(ROOT, "include", "nsof.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.nsof_abi_version() == 3 and re.search(r"#define NSOF_ABI_VERSION 3\b", header)
    # the existing entries keep their signatures: the new ones are those lists plus the pointer and the pair index
    for new, old in zip(NEW, ("nsof_accum_frames_f64_maps_dev", "nsof_accum_frames_f64_maps")):
        assert _lib.SIGNATURES[new][1][:-2] == _lib.SIGNATURES[old][1]
        assert _lib.SIGNATURES[new][1][-1] is _lib.C.c_int64


@pytest.fixture
def no_device(monkeypatch, nsof_lib):
    """Any attempt to make a context or to call the library fails the test."""
    from nsof import accumulator as A  # noqa: N812
    from nsof import context

    def refused(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(A, "default_context", refused)
    monkeypatch.setattr(context, "default_context", refused)
    monkeypatch.setattr(A._lib, "load", refused)
    return nsof_lib


def test_refusals_come_before_any_context(no_device):
    from nsof import _lib
    nsof = no_device
    imgs = np.full((3, 2, 4), 0.5)
    for bad, match in BAD_C2C:
        with pytest.raises(nsof.error, match=match) as e:
            nsof.simulate_frames(imgs, c2c=bad)
        assert isinstance(e.value, ValueError), bad
    for bad in (0, True, 2.5):                                              # trials
        with pytest.raises(nsof.error, match="trials"):
            nsof.simulate_frames(imgs, trials=bad, c2c=dict(sigma=0.1))
    for t_planes in (2, 1):                                                 # a [T'][H][W] plane with T' != T
        with pytest.raises(nsof.error, match=f"{t_planes} trials.*3") as e:
            nsof.simulate_frames(imgs, param_maps=dict(von=np.full((t_planes, 2, 4), 0.1)), trials=3)
        assert e.value.status == _lib.NSOF_ESHAPE
    for bad in (-1, 1.5):                                                   # first_pair
        with pytest.raises(nsof.error, match="first_pair"):
            nsof.simulate_frames(imgs, first_pair=bad)
    with pytest.raises(nsof.error, match="65536") as e:                     # noise with more trials than the counter word holds
        nsof.simulate_frames(imgs, trials=65536, c2c=dict(sigma=0.1))
    assert e.value.status == _lib.NSOF_EUNSUPPORTED
    # the order: c2c, then trials, then first_pair, then the shapes
    with pytest.raises(nsof.error, match="sigma"):
        nsof.simulate_frames(imgs[0], trials=0, c2c=dict(sigma=-1.0), first_pair=-1)
    with pytest.raises(nsof.error, match="trials"):
        nsof.simulate_frames(imgs[0], trials=0, first_pair=-1)
    with pytest.raises(nsof.error, match="first_pair"):
        nsof.simulate_frames(imgs[0], first_pair=-1)
    with pytest.raises(nsof.error, match="sigma"):                          # the study refuses a bad c2c before its frames are read
        nsof.gating_variability_dev(None, nsof.GatingConfig(MEMSIZE=16, THRES=240), {}, 2, c2c=dict(sigma=-0.1))


@pytest.mark.parametrize("p", Z.CLASSES, ids=["alpha", "wide", "default"])
def test_without_noise_the_restatement_is_accum_params_ref(p):
    imgs = Z.frames((4, 4))
    for th in Z.THRESHOLDS:
        w, res = R.simulate_frames(imgs, Z.DT, Z.N_SUB, th[0], th[1], p=p)
        for noise in (None, dict(sigma=0.0, seed=9)):
            out = Z.simulate(imgs, 2, p, None, noise, th=th)
            for t in range(2):
                assert np.array_equal(out["w"][-1][t], w) and np.array_equal(out["res"][:, t], res)
            assert (out["u"] == 1).all()


def test_the_library_variate_is_the_restatement_over_the_gpu_ranges(nsof_lib):
    """Trials 0..4, the cells of the 13 x 24 grid, pairs 0..4 -- and pairs from 2 on, as the resumed runs draw them."""
    seeds = {Z.NOISE["seed"], Z.CLAMP_NOISE["seed"], Z.ON_ONLY["seed"]}
    for seed in seeds:
        for t in range(5):
            want = N.xi(seed, 0, t, np.arange(312)[:, None], np.arange(5)[None])
            got = np.stack([nsof_lib.c2c_noise(seed, 0, t, i, 0, 5) for i in range(312)])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (seed, t)
            assert np.array_equal(nsof_lib.c2c_noise(seed, 0, t, 311, 2, 3), want[311, 2:])


@pytest.mark.parametrize("grid", [(4, 4), (13, 24)])
def test_a_resumed_restatement_is_the_one_shot_run(grid):
    imgs, planes, one = Z.pow_free_case(grid)
    head = Z.simulate(imgs[:3], 3, Z.POW_FREE, planes, Z.NOISE)
    tail = Z.simulate(imgs[2:], 3, Z.POW_FREE, planes, Z.NOISE, first_pair=2, w0=head["w"][-1])
    assert np.array_equal(head["w"], one["w"][:2]) and np.array_equal(tail["w"], one["w"][2:])
    assert np.array_equal(tail["res"][1:], one["res"][3:])
    # ... and the origin matters: the same tail drawn from pair 0 is another run
    again = Z.simulate(imgs[2:], 3, Z.POW_FREE, planes, Z.NOISE, first_pair=0, w0=head["w"][-1])
    assert not np.array_equal(again["w"], tail["w"])


def _both_branches_in_every_trial(out):
    return all(out["off"][:, t].any() and out["on"][:, t].any() for t in range(out["off"].shape[1]))


def test_preconditions_of_the_gpu_cases():
    # the main cases: both branches occur in every trial, and the noise moves the result
    for grid in Z.GRIDS:
        imgs, planes, out = Z.pow_free_case(grid)
        assert _both_branches_in_every_trial(out), grid
        wf = out["w"][-1]
        inside = ((wf > 0) & (wf < 1)).mean()
        print(f"pow-free {grid}: {inside:.2f} of the final states strictly inside (0, 1)")
        assert inside >= 0.5, grid                       # the pow-free case: at least half of the final states are not clipped
        quiet = Z.simulate(imgs, 3, Z.POW_FREE, planes, None)
        assert not np.array_equal(quiet["w"][-1], wf)
        if wf[0].size > 1:
            assert not np.array_equal(wf[0], wf[1])      # the trials differ
    for grid, n_sub in Z.CLASS_CASES[:2]:
        _, _, noisy, quiet = Z.class_case(grid, n_sub)
        assert _both_branches_in_every_trial(noisy), grid
        assert not np.array_equal(noisy["w"][-1], quiet["w"][-1])
    # the clamp case: cells with u < 0 and cells with u > 0 both occur; the former stay at wini, the latter move
    _, c = Z.clamp_case()
    u, w = c["u"][0], c["w"][0]
    assert (u < 0).sum() > 100 and (u > 0).sum() > 100 and (c["off"][0] | c["on"][0]).all()
    assert (w[u < 0] == R.DEFAULT["wini"]).all() and (w[u > 0] != R.DEFAULT["wini"]).all()
    # the directional cases: cells of both branches and of the dead zone occur, an on-branch cell has xi != 0, no state is
    # clipped -- so a noisy cell differs from the noiseless run and no other does
    for which in ("on", "off"):
        _, _, noisy, quiet = Z.direction_case(which)
        on, off, x = noisy["on"][0], noisy["off"][0], noisy["xi"][0]
        assert on.sum() > 50 and off.sum() > 50 and (~(on | off)).sum() > 50
        assert (on & (x != 0)).any() and (off & (x != 0)).any()
        assert ((quiet["w"][0] > 0) & (quiet["w"][0] < 1)).all()
        sel = (on if which == "on" else off) & (x != 0)
        assert (noisy["w"][0][sel] != quiet["w"][0][sel]).all() and np.array_equal(noisy["w"][0][~sel], quiet["w"][0][~sel])
