"""Posterior sums kept on the device (gst_set_accum, include/gst.h): while accumulators are
set, every sweep adds the state at its start -- the values a record of that sweep holds --
into caller-owned running sums, one owner per element, in sweep order.  A sum must therefore
be BITWISE the sequential sum of the recorded chains (b_sq to one rounding per term: the
kernel may fuse v * v into the addition), on every kernel variant, whatever record_every is,
and accumulating must change nothing else."""
import numpy as np
import pytest

from gpu_support import accum_run, accum_sampler, ncu, upload_tape
from gibbs_student_t_amd import Gibbs
from gibbs_student_t_amd.native import ACCUM_KEYS, pack_tape
from gibbs_student_t_amd.post import PosteriorSums
from golden_io import load_ref, sweep_state
from support import check_accum_sums

pytestmark = pytest.mark.gpu

REC_KEYS = ("b", "z", "alpha", "pout")


def _run(*args, **kw):
    """gpu_support.accum_run as the tuple (records, sums, final state, each chain's n)"""
    out = accum_run(*args, **kw)
    return out["rec"], out["sums"], out["state"], out["n_of"]


# each case: the smallest shape that reaches one code path
CASES = {
    "one_wave_n130": dict(names=["beta_fixed"], path="persistent", waves=1),   # 3 slots, last 2 lanes
    "pair": dict(names=["beta_fixed"], path="persistent", waves=2),
    "student_t": dict(names=["t_fixed"], path="persistent"),
    "vvh17": dict(names=["vvh17_fixed"], path="persistent"),
    "gen_n72": dict(names=["ecb_beta_fixed"], path="persistent"),
    "wide_n910": dict(names=["wide_beta_fixed"], path="persistent"),
    "large": dict(names=["beta_fixed"], path="large"),
    "large_epochs_first": dict(names=["mb_beta_fixed"], path="large"),
    # n = 130 next to n = 119: the per-TOA row stride is the batch's largest n
    "batch_ragged": dict(names=["beta_fixed", "simclean_beta_fixed"], path="auto"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_sums_equal_recorded_chains(case):
    """8 chains, 24 sweeps in three launches of 8, sums from sweep0 + 5 on (inside the first
    launch): every sum is the sequential sum of records 5..23, count == 19."""
    cfg = CASES[case]
    per = 8 // len(cfg["names"])
    rec, sums, state, n_of = _run(cfg["names"], per, 3, 8, path=cfg["path"],
                                  waves=cfg.get("waves"))
    if case == "batch_ragged":
        assert n_of.min() < n_of.max() == rec["z"].shape[2]
    check_accum_sums(rec, sums, n_of, 5)
    assert np.all(sums["count"] == 19)


@pytest.mark.parametrize("path", ["persistent", "large"])
def test_tape_mode_accumulates_too(path):
    """Parity launches (injected variates: the persistent kernel's tape instances) keep the
    sums like any other sampling launch"""
    ref = load_ref("beta_fixed")
    S, C, burn = int(ref["niter"]), 5, 2
    ns, _, _ = accum_sampler(["beta_fixed"], C, path)
    n_of = np.full(C, ref["pta"].n)
    ns.set_state(x=np.tile(ref["xs"], (C, 1)))
    rows = pack_tape(ref["tape"], np.arange(S), ns.n, ns.m, ns.stride)
    tape = upload_tape(ns, np.tile(rows, (C, 1, 1)))
    acc = ns.alloc_accum()
    ns.set_accum(acc, from_sweep=burn)
    rec = ns.alloc_records(S, REC_KEYS)
    ns.sweep(S, records=rec, tape=tape)
    sums = {k: v.cpu().numpy() for k, v in acc.items()}
    recs = {k: v.cpu().numpy() for k, v in rec.items()}
    ns.close()
    check_accum_sums(recs, sums, n_of, burn)
    assert np.all(sums["count"] == S - burn) and S - burn >= 3


@pytest.mark.parametrize("path,waves", [("persistent", 1), ("persistent", 2), ("large", None)])
def test_accumulating_changes_nothing_else(path, waves):
    """Same seed with and without accumulators: records and final state bitwise equal; the
    accumulating run under GST_DEBUG_POISON gives the sums of an unpoisoned one."""
    kw = dict(path=path, waves=waves)
    rec0, _, st0, _ = _run(["beta_fixed"], 8, 3, 8, accum=None, **kw)
    rec1, sums1, st1, _ = _run(["beta_fixed"], 8, 3, 8, poison=True, **kw)
    _, sums2, _, _ = _run(["beta_fixed"], 8, 3, 8, **kw)
    for k in REC_KEYS:
        np.testing.assert_array_equal(rec0[k], rec1[k], err_msg=f"rec {k}")
    for k in st0:
        np.testing.assert_array_equal(st0[k], st1[k], err_msg=f"state {k}")
    for k in ACCUM_KEYS:
        np.testing.assert_array_equal(sums1[k], sums2[k], err_msg=k)


@pytest.mark.parametrize("path", ["persistent", "large"])
def test_thinned_run_has_the_same_sums(path):
    """The sums count every sweep whatever record_every is"""
    _, full, _, _ = _run(["beta_fixed"], 8, 3, 8, path=path)
    _, thin, _, _ = _run(["beta_fixed"], 8, 3, 8, path=path, every=4)
    for k in ACCUM_KEYS:
        np.testing.assert_array_equal(thin[k], full[k], err_msg=k)
    assert np.all(thin["count"] == 19)


def test_two_chains_per_simd():
    """More chains than SIMDs: the two-chains-per-SIMD instance"""
    C = 4 * ncu() + 16
    rec, sums, _, n_of = _run(["beta_fixed"], C, 1, 6, path="persistent", burn=2)
    check_accum_sums(rec, sums, n_of, 2)
    assert np.all(sums["count"] == 4)


@pytest.mark.parametrize("path", ["persistent", "large"])
def test_null_subsets(path):
    """Any accumulator may be unset, count included"""
    rec, sums, _, n_of = _run(["beta_fixed"], 8, 3, 8, path=path, accum=("pout_sum",),
                              rec_keys=("pout",))
    assert set(sums) == {"pout_sum"}
    check_accum_sums(rec, sums, n_of, 5, keys=("pout_sum",))


def test_gibbs_record_subset_and_post():
    ref = load_ref("beta_fixed")
    s0 = sweep_state(ref, 0)

    def make():
        g = Gibbs(ref["pta"], **ref["kw"], nchains=4, seed=21)
        g._b, g._z, g._alpha, g._pout = s0["b"], s0["z"], s0["alpha"], s0["pout"]
        g._theta, g.tdf = s0["theta"], s0["nu"]
        return g

    g = make()
    g.sample(ref["xs"], niter=40, record=("x", "theta", "nu"), accumulate=True, burn=10)
    assert g.zchain is None and g.alphachain is None and g.poutchain is None
    assert g.bchain is None
    assert g.chain.shape == (4, 40, len(ref["xs"])) and g.thetachain.shape == (4, 40)
    assert isinstance(g.post, PosteriorSums) and np.all(g.post.count == 30)
    full = make()
    full.sample(ref["xs"], niter=40)
    np.testing.assert_array_equal(full.chain, g.chain)
    np.testing.assert_allclose(g.post.z_mean(pool=False), full.zchain[:, 10:].mean(axis=1),
                               rtol=1e-13, atol=0.0)
    # the notebook's rule on the recorded run (all chains' sweeps pooled)
    zc = full.zchain[:, 10:].reshape(-1, full.zchain.shape[-1])
    np.testing.assert_array_equal(g.post.outliers(), np.flatnonzero(zc.mean(axis=0) > 0.9))
    # the stage methods never accumulate; a sample() without accumulate leaves no new sums
    post, z_sum = g.post, g.post.z_sum.copy()
    x = g.chain[:, -1]
    g.update_theta(x)
    g.sample(x, niter=4)
    assert g.post is post and np.array_equal(post.z_sum, z_sum) and np.all(post.count == 30)
    assert g.zchain is not None
    g.close()
    full.close()
