"""CPU: the flow-ensemble entry is declared, exported and bound; the Python entries refuse bad arguments before a context
exists; the NumPy restatement the GPU tests compare against (tests/flow_ensemble_ref.py) agrees with the plain
definitions and with itself when the trials are chunked; and the GPU case list keeps its coverage of the kernel's tiles
and load forms, recomputed from the tile constants of csrc/flow_ensemble.hip."""
import os
import re

import numpy as np
import pytest

import flow_ensemble_ref as R
from conftest import ROOT


def test_symbol_is_declared_exported_and_bound(nsof_lib):
    from nsof import _lib, pipeline
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsof.h")).read(), flags=re.S)
    decl = re.search(r"int\s+nsof_flow_ensemble_dev\s*\(([^;]*)\)\s*;", header)
    assert decl, "nsof_flow_ensemble_dev is not declared in include/nsof.h"
    res, args = _lib.SIGNATURES["nsof_flow_ensemble_dev"]
    assert len(args) == len(decl.group(1).split(",")) == 20
    lib = _lib.load()
    assert hasattr(lib, "nsof_flow_ensemble_dev") and lib.nsof_abi_version() == 3
    assert re.search(r"#define\s+NSOF_ABI_VERSION\s+3\b", header)
    for name in ("flow_ensemble_dev", "flow_ensemble_summary", "events_flow_variability_dev"):
        assert callable(getattr(nsof_lib, name))
    assert pipeline.events_flow_variability_dev is nsof_lib.events_flow_variability_dev


def _events():
    from nsof import synth
    return synth.make_events(1, width=32, height=24, n_background=50, duration_us=70_000, box=(4, 4))


@pytest.fixture()
def no_context(nsof_lib, monkeypatch):
    """Any attempt to create or fetch a context fails the test."""
    from nsof import context

    def boom(*a, **k):
        raise AssertionError("a context was asked for before the arguments were refused")
    monkeypatch.setattr(context, "default_context", boom)
    monkeypatch.setattr(context.Context, "__init__", boom)


def test_flow_ensemble_dev_refuses_before_a_context(nsof_lib, no_context):
    import torch
    err = nsof_lib.errors.NsofValueError
    with pytest.raises(err, match="CUDA tensor"):
        nsof_lib.flow_ensemble_dev(np.zeros((2, 1, 4, 4, 2), np.float32))
    with pytest.raises(err, match="CUDA tensor"):
        nsof_lib.flow_ensemble_dev(torch.zeros((2, 1, 4, 4, 2)))
    with pytest.raises(err, match="n_trials"):
        nsof_lib.flow_ensemble_summary(dict(n_trials=1, sum=torch.zeros(1, 2, 2, 2), sq=torch.zeros(1, 2, 2, 3),
                                            epe2_max=torch.zeros(1, 2, 2)))


@pytest.mark.parametrize("kw, match", [
    (dict(rel_sigma=dict(nosuch=0.1)), "per-pixel parameter"),
    (dict(trials=0), "trials"),
    (dict(trials=2.5), "trials"),
    (dict(c2c=dict(sigma=-1.0)), "c2c"),
    (dict(c2c=[0.1]), "c2c"),
    (dict(active_v=[-6.0, -5.0]), "active_v"),
    (dict(silent_v=(0.0, 0.1)), "silent_v"),
    (dict(tau=-1.0), "tau"),
    (dict(tau=float("nan")), "tau"),
    (dict(tau="1"), "tau"),
    (dict(trial_chunk=0), "trial_chunk"),
    (dict(trial_chunk=1.5), "trial_chunk"),
])
def test_events_flow_variability_dev_refuses_before_a_context(nsof_lib, no_context, kw, match):
    x, y, p, t = _events()
    args = dict(rel_sigma=dict(koff=0.1), trials=2)
    args.update(kw)
    with pytest.raises(nsof_lib.errors.NsofValueError, match=match):
        nsof_lib.events_flow_variability_dev(x, y, p, t, (24, 32), **args)


def test_refusals_come_in_events_variability_devs_order(nsof_lib, no_context):
    """The maps, then c2c, then active_v, then silent_v: with every argument bad, the first one is named."""
    x, y, p, t = _events()
    bad = dict(rel_sigma=dict(nosuch=0.1), trials=2, c2c=dict(sigma=-1.0), active_v=[1, 2], silent_v=[1, 2], tau=-1.0)
    for fixed, match in ((dict(), "per-pixel parameter"), (dict(rel_sigma={}), "c2c"), (dict(c2c=None), "active_v"),
                         (dict(active_v=-6.0), "silent_v"), (dict(silent_v=0.0), "tau")):
        bad.update(fixed)
        with pytest.raises(nsof_lib.errors.NsofValueError, match=match):
            nsof_lib.events_flow_variability_dev(x, y, p, t, (24, 32), **bad)


def test_restatement_matches_the_plain_definitions(nsof_lib):
    """sum, sq and epe2_max of the restatement against np.mean, np.cov and np.max over the trial axis -- and through
    nsof.flow_ensemble_summary, which is plain torch and runs on host tensors as well.  Bounds: 7 trials of |values| <= 40
    (flow and reference in +-20), so the mean carries at most ~7 roundings of 2^-53 * 40 < 1e-13; the covariance is a
    difference of sums of squares up to 7 * 1600, rounded to 2^-53 * 11200 ~ 1.3e-12 each, divided by 6: < 1e-11."""
    import torch
    flows, ref = R.make_flows((7, 2, 5, 6), 11)
    res = R.fold(flows, ref, tau=15.0)
    f64 = flows.astype(np.float64)
    d = f64 - ref.astype(np.float64)
    e2 = d[..., 0] ** 2 + d[..., 1] ** 2
    assert np.array_equal(res["epe2_max"], e2.max(axis=0))
    assert np.array_equal(res["outliers"], (e2 > 225.0).sum(axis=(2, 3))) and not res["nonfinite"].any() and res["n_trials"] == 7
    np.testing.assert_allclose(res["aee"], np.sqrt(e2).mean(axis=(2, 3)), rtol=1e-13)
    summary = nsof_lib.flow_ensemble_summary({k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in res.items()},
                                             torch.from_numpy(ref))
    np.testing.assert_allclose(summary["mean"].numpy(), f64.mean(axis=0), rtol=0, atol=1e-13)
    cov = np.empty((2, 5, 6, 2, 2))
    for idx in np.ndindex(2, 5, 6):
        cov[idx] = np.cov(f64[(slice(None),) + idx].T)
    np.testing.assert_allclose(summary["cov"].numpy(), cov, rtol=0, atol=1e-11)
    np.testing.assert_allclose(summary["epe_rms"].numpy(), np.sqrt(e2.mean(axis=0)), rtol=1e-14)
    assert np.array_equal(summary["epe_max"].numpy(), np.sqrt(e2.max(axis=0)))
    # the zero reference: the raw moments
    raw = R.fold(flows)
    np.testing.assert_allclose(raw["sum"] / 7, f64.mean(axis=0), rtol=0, atol=1e-13)


@pytest.mark.parametrize("cuts", [(2,), (1, 2, 3, 4), (4,)])
def test_restatement_chunked_equals_one_shot(nsof_lib, cuts):
    """... and so do the maps nsof.flow_ensemble_summary forms from the two."""
    import torch
    flows, ref = R.make_flows((5, 2, 7, 9), 3)
    whole = R.fold(flows, ref, tau=12.0)
    state, per_trial = None, []
    for a, b in zip((0,) + cuts, cuts + (5,)):
        state = R.fold(flows[a:b], ref, tau=12.0, state=state)
        per_trial.append(state)
    assert state["n_trials"] == 5
    for k in ("sum", "sq", "epe2_max"):
        assert np.array_equal(state[k], whole[k]), k
    for k in ("aee", "outliers", "nonfinite"):
        assert np.array_equal(np.concatenate([r[k] for r in per_trial]), whole[k]), k
    maps = [nsof_lib.flow_ensemble_summary({k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in r.items()},
                                           torch.from_numpy(ref)) for r in (state, whole)]
    for k in ("mean", "cov", "epe_rms", "epe_max"):
        assert torch.equal(maps[0][k], maps[1][k]), k


def test_kernel_cases_keep_their_coverage():
    """What the GPU cases give, recomputed from the kernel's tile constants: an edit of the case list or of the tiles that
    loses one of these fails here, without a GPU."""
    bx, by, px, inflight = (R.tile_constant(k) for k in ("FE_BX", "FE_BY", "FE_PX", "FE_INFLIGHT"))
    assert bx == 64 * px and px in (1, 2), "a wave covers FE_BX pixels of a row, one or two per lane"
    cases = R.kernel_cases()
    assert cases[:2] == [(1, 1, 1, 1), (5, 2, 19, 37)]
    g = {c: R.geometry(c) for c in cases}
    assert g[(1, 1, 1, 1)][:2] == (1, 1), "one workgroup"
    assert any(v[0] >= 3 and v[1] >= 3 and v[2] == 1 and v[3] == 1 for v in g.values()), \
        "three workgroups in x and in y, the last tiles one pixel wide and one row high"
    assert any(v[4] for v in g.values()) and any(not v[4] and c[3] > 1 for c, v in g.items()), "rows with and without a lone last pixel"
    assert any(v[3] != by for v in g.values()) and any(v[2] not in (1, bx) for v in g.values()), "row and lane tails"
    assert any(c[0] > inflight and c[0] % inflight for c in cases), "a full batch of trials and a tail"
    assert any(0 < c[0] < inflight for c in cases), "fewer trials than a batch"
    assert any(c[1] > 1 for c in cases), "more than one field"
    forms = {R.load_form(c, padded) for c in cases for padded in (False, True)}
    assert forms == {"px", "pair", "pair_odd"}, forms
    # the padded layouts stay legal: even strides that hold their rows
    for c in cases:
        rs, fs, ts = R.strides(c, True)
        assert rs % 2 == 0 and rs > 2 * c[3] and fs > c[2] * rs - 1 and ts > c[1] * fs - 1 and fs % 2 == 0 and ts % 2 == 0
