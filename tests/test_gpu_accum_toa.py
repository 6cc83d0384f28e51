"""Per-TOA exceedance counts and residual sums kept on the device (gst_set_accum_toa,
include/gst.h): while gst_set_accum is set, every counted sweep adds, per TOA, 1 where
pout_t > thr[k] (strict) and y_t, y_t^2 of y = r - T b for the start-of-sweep b.

pout is a record, so a count must be BITWISE the count over the recorded chain.  y is not a
record: it is compared with the long-double r - T @ b_rec[i] to the fp64 rounding of an
m-term dot product in any order plus the N additions of the sum,

    |resid_sum_t - sum_i y_it|  <=  2 (m + 2 + N) eps  sum_i A_it,   A_it = |r_t| + sum_j |T_tj b_ij|

and resid_sq to the same relative bound of its own terms: an error d <= (m + 2) eps A in y
moves y^2 by 2 |y| d + d^2 <= 2 (m + 2) eps A^2 (to first order, |y| <= A), the square and the
N additions add (N + 1) eps A^2 at most:

    |resid_sq_t - sum_i y_it^2|  <=  2 (m + 2 + N) eps  sum_i A_it^2.

Neither bound is a measured number.  The new sums must change nothing else."""
import ctypes as ct
import functools

import numpy as np
import pytest

from gpu_support import SENTINEL, accum_alloc, accum_run, accum_sampler, ncu, upload_tape
from gibbs_student_t_amd import Gibbs, _abi, run_sims
from gibbs_student_t_amd.native import ACCUM_KEYS, ACCUM_TOA_KEYS, pack_tape
from gibbs_student_t_amd.post import PosteriorSums
from golden_io import load_ref, sweep_state
from support import check_accum_sums

pytestmark = pytest.mark.gpu

REC_KEYS = ("b", "z", "alpha", "pout")
THR = (0.1, 0.5, 0.9)
EPS = np.finfo(np.float64).eps
ALL_KEYS = ACCUM_KEYS + ACCUM_TOA_KEYS
_run = functools.partial(accum_run, accum=ALL_KEYS, thr=THR)


def _check_counts(out, burn, thr=THR, nondegenerate=True):
    """pout_gt[k] is bitwise the count of rec_pout > thr[k] over the records from ``burn`` on;
    entries t >= n keep the sentinel"""
    pout, gt = out["rec"]["pout"], out["sums"]["pout_gt"]
    nrec = pout.shape[1]
    assert gt.shape == (len(thr),) + pout.shape[::2]
    inside = False
    for k, t in enumerate(thr):
        want = np.zeros_like(pout[:, 0])
        for i in range(burn, nrec):
            want = want + (pout[:, i] > t)
        for c, n in enumerate(out["n_of"]):
            np.testing.assert_array_equal(gt[k, c, :n], want[c, :n], err_msg=f"thr {t} chain {c}")
            assert np.all(gt[k, c, n:] == SENTINEL), f"pout_gt[{k}]: chain {c} wrote t >= n"
            inside = inside or bool(np.any((want[c, :n] > 0) & (want[c, :n] < nrec - burn)))
    if nondegenerate:
        # not a vacuous comparison of all-0 / all-N planes
        assert inside, "no TOA with 0 < count < N at any threshold"


def _check_resid(out, burn, keys=("resid_sum", "resid_sq")):
    """resid_sum / resid_sq against long-double sums of r - T @ b_rec[i], to the bounds of the
    module docstring; each figure is printed before it is asserted"""
    b = out["rec"]["b"]
    nrec = b.shape[1]
    N = nrec - burn
    for c, d in enumerate(out["ds_of"]):
        pta = out["refs"][d]["pta"]
        T = np.asarray(pta.get_basis()[0], dtype=np.float64)
        r = np.asarray(pta.get_residuals()[0], dtype=np.float64)
        n, m = T.shape
        bc = b[c, burn:]                                           # [N, m]
        y = r.astype(np.longdouble)[None, :] - bc.astype(np.longdouble) @ T.T.astype(np.longdouble)
        A = np.abs(r)[None, :] + np.abs(bc) @ np.abs(T).T          # [N, n]
        rel = 2.0 * (m + 2 + N) * EPS
        for key, want, bound in (("resid_sum", y.sum(axis=0), rel * A.sum(axis=0)),
                                 ("resid_sq", (y * y).sum(axis=0), rel * (A * A).sum(axis=0))):
            if key not in keys:
                continue
            got = out["sums"][key][c]
            err = np.abs(got[:n].astype(np.longdouble) - want).astype(np.float64)
            if c == 0:
                print(f"{key}: chain 0 worst error / bound = {float(np.max(err / bound)):.3g}")
            assert np.all(err <= bound), f"{key} chain {c}: worst error / bound " \
                                         f"{float(np.max(err / bound)):.3g}"
            assert np.all(got[n:] == SENTINEL), f"{key}: chain {c} wrote t >= n"
            assert np.any(want != 0)


def _check_old_sums(out, burn):
    check_accum_sums(out["rec"], out["sums"], out["n_of"], burn,
                     ("z_sum", "pout_sum", "alpha_sum", "b_sum", "count"))


# each case: the smallest shape that reaches one code path (tests/test_gpu_accum.py)
CASES = {
    "one_wave_n130": dict(names=["beta_fixed"], path="persistent", waves=1),
    "pair": dict(names=["beta_fixed"], path="persistent", waves=2),
    "vvh17": dict(names=["vvh17_fixed"], path="persistent"),
    "gen_n72": dict(names=["ecb_beta_fixed"], path="persistent"),
    "wide_n910": dict(names=["wide_beta_fixed"], path="persistent"),
    "large": dict(names=["beta_fixed"], path="large"),
    "large_epochs_first": dict(names=["mb_beta_fixed"], path="large"),
    "batch_ragged": dict(names=["beta_fixed", "simclean_beta_fixed"], path="auto"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_counts_and_residual_sums_equal_recorded_chains(case):
    """8 chains, 24 sweeps in three launches of 8, sums from sweep0 + 5 on (inside the first
    launch): counts of records 5..23 bitwise, residual sums to their rounding bound, and the
    old sums as ever beside them."""
    cfg = CASES[case]
    per = 8 // len(cfg["names"])
    out = _run(cfg["names"], per, 3, 8, path=cfg["path"], waves=cfg.get("waves"))
    if case == "batch_ragged":
        assert out["n_of"].min() < out["n_of"].max() == out["rec"]["z"].shape[2]
    _check_counts(out, 5)
    _check_resid(out, 5)
    _check_old_sums(out, 5)
    assert np.all(out["sums"]["count"] == 19)


def test_all_zero_counts():
    """The Student-t model's pout never exceeds 0.1: every plane stays zero"""
    out = _run(["t_fixed"], 8, 3, 8, path="persistent")
    _check_counts(out, 5, nondegenerate=False)
    n = out["n_of"][0]
    assert np.all(out["sums"]["pout_gt"][:, :, :n] == 0.0)
    _check_resid(out, 5)


@pytest.mark.parametrize("path", ["persistent", "large"])
def test_tape_mode(path):
    """Parity launches (injected variates: the persistent kernel's tape instances)"""
    ref = load_ref("beta_fixed")
    S, C, burn = int(ref["niter"]), 5, 2
    ns, refs, ds_of = accum_sampler(["beta_fixed"], C, path)
    n_of = np.full(C, ref["pta"].n)
    ns.set_state(x=np.tile(ref["xs"], (C, 1)))
    rows = pack_tape(ref["tape"], np.arange(S), ns.n, ns.m, ns.stride)
    tape = upload_tape(ns, np.tile(rows, (C, 1, 1)))
    acc = accum_alloc(ns, n_of, ALL_KEYS, THR)
    ns.set_accum(acc, from_sweep=burn, pout_thresholds=THR)
    rec = ns.alloc_records(S, REC_KEYS)
    ns.sweep(S, records=rec, tape=tape)
    out = dict(rec={k: v.cpu().numpy() for k, v in rec.items()},
               sums={k: v.cpu().numpy() for k, v in acc.items()}, refs=refs, ds_of=ds_of,
               n_of=n_of)
    ns.close()
    _check_counts(out, burn)
    _check_resid(out, burn)
    _check_old_sums(out, burn)
    assert S - burn >= 3


def test_two_chains_per_simd():
    """More chains than SIMDs: the two-chains-per-SIMD instance"""
    C = 4 * ncu() + 16
    out = _run(["beta_fixed"], C, 1, 6, path="persistent", burn=2)
    _check_counts(out, 2)
    # (the residual check on the first and last 8 chains: the host reference is long double)
    for sl in (slice(0, 8), slice(C - 8, C)):
        sub = dict(out, rec={k: v[sl] for k, v in out["rec"].items()},
                   sums={k: (v[:, sl] if k == "pout_gt" else v[sl]) for k, v in out["sums"].items()},
                   ds_of=out["ds_of"][sl], n_of=out["n_of"][sl])
        _check_resid(sub, 2)
    assert np.all(out["sums"]["count"] == 4)


@pytest.mark.parametrize("path,waves", [("persistent", 1), ("persistent", 2), ("large", None)])
def test_new_sums_change_nothing_else(path, waves):
    """Same seed with the old sums only and with the new ones beside them: records, final
    state and all six old sums bitwise equal; under GST_DEBUG_POISON the new sums are those of
    an unpoisoned run."""
    kw = dict(path=path, waves=waves)
    old = _run(["beta_fixed"], 8, 3, 8, accum=ACCUM_KEYS, **kw)
    new = _run(["beta_fixed"], 8, 3, 8, **kw)
    poi = _run(["beta_fixed"], 8, 3, 8, poison=True, **kw)
    for k in REC_KEYS:
        np.testing.assert_array_equal(old["rec"][k], new["rec"][k], err_msg=f"rec {k}")
    for k in old["state"]:
        np.testing.assert_array_equal(old["state"][k], new["state"][k], err_msg=f"state {k}")
    for k in ACCUM_KEYS:
        np.testing.assert_array_equal(old["sums"][k], new["sums"][k], err_msg=k)
    for k in ACCUM_TOA_KEYS:
        np.testing.assert_array_equal(poi["sums"][k], new["sums"][k], err_msg=k)


@pytest.mark.parametrize("path", ["persistent", "large"])
def test_thinned_run_has_the_same_new_sums(path):
    """The new sums count every sweep whatever record_every is"""
    full = _run(["beta_fixed"], 8, 3, 8, path=path)
    thin = _run(["beta_fixed"], 8, 3, 8, path=path, every=4)
    for k in ACCUM_TOA_KEYS:
        np.testing.assert_array_equal(thin["sums"][k], full["sums"][k], err_msg=k)
    assert np.all(thin["sums"]["count"] == 19)


@pytest.mark.parametrize("path", ["persistent", "large"])
def test_null_subsets(path):
    """Any of the new pointers may be unset: only pout_gt with K = 1, only resid_sum, K = 4"""
    out = _run(["beta_fixed"], 8, 3, 8, path=path, accum=("pout_gt",), thr=(0.5,),
               rec_keys=("pout",))
    assert set(out["sums"]) == {"pout_gt"}
    _check_counts(out, 5, thr=(0.5,))
    out = _run(["beta_fixed"], 8, 3, 8, path=path, accum=("resid_sum", "count"), thr=None,
               rec_keys=("b",))
    _check_resid(out, 5, keys=("resid_sum",))
    assert np.all(out["sums"]["count"] == 19)
    thr4 = (0.1, 0.5, 0.9, 0.99)
    out = _run(["beta_fixed"], 8, 3, 8, path=path, accum=("pout_gt", "resid_sq"), thr=thr4,
               rec_keys=("pout", "b"))
    _check_counts(out, 5, thr=thr4)
    _check_resid(out, 5, keys=("resid_sq",))


@pytest.mark.parametrize("path", ["persistent", "large"])
def test_without_set_accum_nothing_is_written(path):
    """gst_set_accum_toa alone keeps nothing: the sums exist only while gst_set_accum is set"""
    out = _run(["beta_fixed"], 8, 1, 8, path=path, accum=ACCUM_TOA_KEYS, with_accum=False,
               burn=0)
    n = out["n_of"][0]
    for k in ACCUM_TOA_KEYS:
        assert np.all(out["sums"][k][..., :n] == 0.0), k
        assert np.all(out["sums"][k][..., n:] == SENTINEL), k


def test_bad_thresholds_are_refused():
    ns, _, _ = accum_sampler(["beta_fixed"], 2)
    for thr in ((0.5, 0.5), (0.9, 0.1), (0.0,), (1.0,), (float("nan"),)):
        a = _abi.AccumToa(len(thr), (ct.c_double * 4)(*thr), None, None, None)
        assert ns.lib.gst_set_accum_toa(ns.ctx, ct.byref(a)) != 0
        assert "threshold" in _abi.last_error(ns.lib)
    a = _abi.AccumToa(5, (ct.c_double * 4)(0.1, 0.2, 0.3, 0.4), None, None, None)
    assert ns.lib.gst_set_accum_toa(ns.ctx, ct.byref(a)) != 0
    with pytest.raises(ValueError):
        ns.alloc_accum(("pout_gt",), pout_thresholds=(0.1, 0.2, 0.3, 0.4, 0.5))
    ns.close()


def test_gibbs_median_rule_and_signal_band():
    """3 chains x 31 counted sweeps (93 is odd: no tie): the median rule of the device counts
    is that of a fully recorded run with the same seed, the band that of T @ bchain."""
    ref = load_ref("beta_fixed")
    s0 = sweep_state(ref, 0)
    burn, N = 9, 31

    def make():
        g = Gibbs(ref["pta"], **ref["kw"], nchains=3, seed=21)
        g._b, g._z, g._alpha, g._pout = s0["b"], s0["z"], s0["alpha"], s0["pout"]
        g._theta, g.tdf = s0["theta"], s0["nu"]
        return g

    g = make()
    g.sample(ref["xs"], niter=burn + N, record=("x",), accumulate=True, burn=burn,
             pout_thresholds=(0.2, 0.5), signal_band=True)
    full = make()
    full.sample(ref["xs"], niter=burn + N)
    np.testing.assert_array_equal(full.chain, g.chain)
    assert np.all(g.post.count == N)
    n = full.poutchain.shape[-1]
    pc = full.poutchain[:, burn:].reshape(-1, n)
    for thr in (0.2, 0.5):
        got, amb = g.post.pout_median_gt(thr)
        assert not amb.any()
        np.testing.assert_array_equal(g.post.outliers(thr, rule="median"),
                                      np.flatnonzero(np.median(pc, axis=0) > thr))
    np.testing.assert_array_equal(g.post.outliers(), np.flatnonzero(
        full.zchain[:, burn:].reshape(-1, n).mean(axis=0) > 0.9))
    # the band: Var[T b] = E y^2 - (E y)^2 of y = r - T b.  With the module docstring's bounds
    # e1 on sum y and e2 on sum y^2 over the Nt = 93 pooled sweeps, the variance moves by at
    # most e2 / Nt + (2 |mean y| e1 + e1^2 / Nt) / Nt, plus the few roundings of forming it
    T = np.asarray(ref["pta"].get_basis()[0], dtype=np.float64)
    r = np.asarray(ref["pta"].get_residuals()[0], dtype=np.float64)
    m = T.shape[1]
    bc = full.bchain[:, burn:].reshape(-1, full.bchain.shape[-1])[:, :m]
    Nt = bc.shape[0]
    tb = bc.astype(np.longdouble) @ T.T.astype(np.longdouble)
    y = r.astype(np.longdouble) - tb
    A = np.abs(r)[None, :] + np.abs(bc) @ np.abs(T).T
    rel = 2.0 * (m + 2 + N) * EPS
    e1, e2 = rel * A.sum(axis=0), rel * (A * A).sum(axis=0)
    ybar = np.abs(y.mean(axis=0)).astype(np.float64)
    ey2 = (y * y).mean(axis=0).astype(np.float64)
    dvar = e2 / Nt + (2 * ybar * e1 + e1 * e1 / Nt) / Nt + 8 * EPS * ey2
    var_ref = ((tb * tb).mean(axis=0) - tb.mean(axis=0) ** 2).astype(np.float64)
    err = np.abs(g.post.signal_sd() ** 2 - var_ref)
    print(f"signal variance: worst error / bound = {float(np.max(err / dvar)):.3g}")
    assert np.all(err <= dvar)
    assert np.all(g.post.signal_sd() > 0)
    np.testing.assert_allclose(g.post.signal_mean_toa(r), g.post.signal_mean(T)[:n],
                               atol=float(np.max(e1)) / Nt * 2, rtol=0)
    with pytest.raises(ValueError, match="accumulate"):
        g.sample(g.chain[:, -1], niter=2, pout_thresholds=(0.5,))
    g.close()
    full.close()


def test_study_post_files(tmp_path):
    """One theta, two models, 2 chains, 40 sweeps with --post: each entry's post.npz holds the
    sums of that entry's chain files"""
    run_sims.main(["--thetas", "0.1", "--models", "beta", "vvh17", "--chains", "2", "--niter",
                   "40", "--burn", "10", "--chunk", "16", "--outdir", str(tmp_path),
                   "--generator", "host", "--seed", "7", "--post", "--pout-thresholds", "0.2",
                   "0.9", "--signal-band"])
    entries = run_sims.build_grid((0.1,), 1, ("beta", "vvh17"), 7, generator="host")
    assert len(entries) == 4
    for e in entries:
        d = e.outdir(str(tmp_path))
        post = PosteriorSums.load(d + "/post.npz")
        ch = {f: np.load(f"{d}/{f}.npy") for f in ("bchain", "zchain", "poutchain", "alphachain")}
        n = e.pta.n
        assert ch["poutchain"].shape == (2, 30, n) and np.all(post.count == 30)
        assert post.pout_gt.shape == (2, 2, n) and post.resid_sum.shape == (2, n)
        for key, f in (("z_sum", "zchain"), ("pout_sum", "poutchain"), ("alpha_sum", "alphachain"),
                       ("b_sum", "bchain")):
            want = np.zeros_like(ch[f][:, 0])
            for i in range(30):
                want = want + ch[f][:, i]
            np.testing.assert_array_equal(getattr(post, key), want, err_msg=key)
        for k, t in enumerate((0.2, 0.9)):
            np.testing.assert_array_equal(post.pout_gt[k], (ch["poutchain"] > t).sum(axis=1))
        T = np.asarray(e.pta.get_basis()[0], dtype=np.float64)
        r = np.asarray(e.pta.get_residuals()[0], dtype=np.float64)
        m = T.shape[1]
        for c in range(2):
            bc = ch["bchain"][c]
            y = r.astype(np.longdouble) - bc.astype(np.longdouble) @ T.T.astype(np.longdouble)
            A = np.abs(r)[None, :] + np.abs(bc) @ np.abs(T).T
            rel = 2.0 * (m + 2 + 30) * EPS
            assert np.all(np.abs(post.resid_sum[c] - y.sum(axis=0)) <= rel * A.sum(axis=0))
            assert np.all(np.abs(post.resid_sq[c] - (y * y).sum(axis=0))
                          <= rel * (A * A).sum(axis=0))
