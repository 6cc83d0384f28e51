"""The shared test scaffolding (support.py, golden_io.py, gpu_support.py's gate): the state
builders against the literal code they replaced, bit for bit, and the assertion helpers on
inputs that must pass and that must fail."""
import importlib
import os
import sys

import numpy as np
import pytest

import support
from golden_io import (GOLDEN, MGP_DATASETS, MGP_NAMES, fixture_names, load_ref, oracle_replay,
                       sweep_state)
from support import (assert_replay_matches, batch_start_state, host_tool, pad, prior_box, rel,
                     start_state)


@pytest.fixture(scope="module")
def refs():
    return [load_ref("beta_fixed"), load_ref("simclean_beta_fixed")]     # n = 130, n = 119


def _literal(ref, C, x, width=None):
    """The expression the test modules wrote out before start_state"""
    s0 = sweep_state(ref, 0)
    w = (lambda a: a) if width is None else (lambda a: _literal_pad(a, width))
    return dict(x=x, b=np.tile(s0["b"], (C, 1)), z=np.tile(w(s0["z"]), (C, 1)),
                alpha=np.tile(w(s0["alpha"]), (C, 1)), pout=np.tile(w(s0["pout"]), (C, 1)),
                theta=np.full(C, s0["theta"]), nu=np.full(C, s0["nu"]))


def _literal_pad(a, width):
    out = np.zeros(a.shape[:-1] + (width,))
    out[..., :a.shape[-1]] = a
    return out


def _same(got, want):
    assert list(got) == list(want) == ["x", "b", "z", "alpha", "pout", "theta", "nu"]
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("C", [1, 7])
def test_start_state_x_choices(refs, C):
    for ref in refs:
        lo = np.array([p.pmin for p in ref["pta"].params])
        hi = np.array([p.pmax for p in ref["pta"].params])
        _same(start_state(ref, C), _literal(ref, C, np.tile(ref["xs"], (C, 1))))
        _same(start_state(ref, C, "chain0"), _literal(ref, C, np.tile(ref["chain"][0], (C, 1))))
        for seed in (5, [5, 1]):
            x = np.random.default_rng(seed).uniform(lo, hi, size=(C, len(lo)))
            _same(start_state(ref, C, seed), _literal(ref, C, x))
        lo2, hi2 = prior_box(ref["pta"])
        assert lo2.tobytes() == lo.tobytes() and hi2.tobytes() == hi.tobytes()
    if C == 1:      # the one-chain form the replays wrote: arrays[None], np.array([scalar])
        ref, s0 = refs[0], sweep_state(refs[0], 0)
        _same(start_state(ref, 1), dict(
            x=ref["xs"][None], b=s0["b"][None], z=s0["z"][None], alpha=s0["alpha"][None],
            pout=s0["pout"][None], theta=np.array([s0["theta"]]), nu=np.array([s0["nu"]])))


def test_start_state_padded_width(refs):
    ref = refs[1]
    assert ref["pta"].n == 119
    x = np.tile(ref["xs"], (3, 1))
    got = start_state(ref, 3, width=130)
    _same(got, _literal(ref, 3, x, 130))
    assert got["z"].shape == (3, 130) and np.all(got["alpha"][:, 119:] == 0.0)
    assert pad(np.ones((2, 3)), 5).tolist() == [[1, 1, 1, 0, 0]] * 2


def test_batch_start_state(refs):
    per, width = 4, 130
    assert [r["pta"].n for r in refs] == [130, 119]
    parts = []
    for d, ref in enumerate(refs):        # the accumulator tests' per-dataset seeding
        lo = np.array([p.pmin for p in ref["pta"].params])
        hi = np.array([p.pmax for p in ref["pta"].params])
        x = np.random.default_rng([5, d]).uniform(lo, hi, size=(per, len(lo)))
        parts.append(_literal(ref, per, x, width))
    want = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    _same(batch_start_state(refs, per, width, x=lambda d: [5, d]), want)
    parts = [_literal(r, per, np.tile(r["xs"], (per, 1)), width) for r in refs]
    want = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    _same(batch_start_state(refs, per, width), want)


def test_rel():
    inf = np.inf
    with np.errstate(all="raise"):
        r = rel([inf, -inf, inf, -inf, 3.0, 0.0, -2.0], [inf, -inf, -inf, inf, 2.0, 0.0, -4.0])
    assert r.tolist() == [0.0, 0.0, inf, inf, 0.5, 0.0, 0.5]
    assert rel(1e-300, 0.0) == 1.0          # the denominator's floor


def test_assert_replay_matches_passes_and_raises(refs):
    ref = refs[0]
    want = oracle_replay(ref, 3)
    assert_replay_matches({k: v.copy() for k, v in want.items()}, want, ref)

    def broken(key, change):
        got = {k: v.copy() for k, v in want.items()}
        change(got[key])
        return got

    def flip(z):
        z[1, 5] = 1.0 - z[1, 5]

    def one_ulp(x):
        x[2, 0] = np.nextafter(x[2, 0], np.inf)

    def scale(alpha):
        alpha[1, 7] *= 1.0 + 1e-9

    for key, change in (("z", flip), ("x", one_ulp), ("alpha", scale)):
        with pytest.raises(AssertionError):
            assert_replay_matches(broken(key, change), want, ref, key)


def test_load_ref_finds_both_families():
    names = fixture_names()
    assert names and not any(n.split("_")[0] in MGP_DATASETS for n in names)
    for name in names:
        ref = load_ref(name)
        assert ref["chain"].shape[0] == int(ref["niter"]) and ref["pta"].n == ref["zchain"].shape[1]
    assert len(MGP_NAMES) == 2 * len(MGP_DATASETS)
    for name in MGP_NAMES:
        ref = load_ref(name)
        ncols, nec, _ = MGP_DATASETS[name.split("_")[0]]
        stored = np.load(os.path.join(GOLDEN, f"mgp_{name.split('_')[0]}_dataset.npz"))["names"]
        assert ref["pta"].param_names == [str(v) for v in stored]
        assert tuple(q.ncol for q in ref["pta"].procs) == ncols and ref["pta"].n_ecorr == nec


def test_gpu_support_import_is_the_gate():
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a device is present: the import does not skip")
    except ImportError:
        pass
    sys.modules.pop("gpu_support", None)
    with pytest.raises(pytest.skip.Exception):
        importlib.import_module("gpu_support")


def test_host_tool_builds_once(tmp_path_factory, monkeypatch):
    first = host_tool(tmp_path_factory, "philox_kat", flags=("-O2",))

    def no_rebuild(*a, **kw):
        raise AssertionError("host_tool rebuilt a program it had")
    monkeypatch.setattr(support.subprocess, "run", no_rebuild)
    assert host_tool(tmp_path_factory, "philox_kat", flags=("-O2",)) == first
