"""Models with several power-law processes (red noise + DM (+ chromatic)): the kernel variants
agree with one another, the persistent kernel's launch-boundary invariants hold on its general
instances with a process boundary inside the Fourier block (dmg: column 14 of 24; dme: column
10 of 20, then 24 ECORR columns), a large-path chain does not depend on its batch partners,
the Philox-mode hyper MH block follows the tape the numpy mirror writes over every process's
parameters, and the public ``Gibbs`` class runs such a model with a checkpoint round trip."""
import numpy as np
import pytest

from gpu_support import (builds, launch_records, open_sampler, single_sweep_differences, torch,
                         upload_tape)
from gibbs_student_t_amd import _abi, data
from gibbs_student_t_amd.model import PTA
from gibbs_student_t_amd.native import STATE_KEYS as KEYS, pack_tape
from gibbs_student_t_amd.sampler import Gibbs
from oracle import philox_variates as pv
from oracle.gibbs_oracle import Oracle, OutlierModel
from support import RTOL, cached_ref, prior_box, rel, start_state, states_at

pytestmark = pytest.mark.gpu


# ---- kernel variants --------------------------------------------------------------------------
@pytest.mark.parametrize("ds,variants", [
    ("dmx", ({}, dict(epochs_lds=True), dict(large_hyper=True))),
    ("dmw", ({}, dict(large_hyper=True)))])
def test_kernel_variants_agree(ds, variants):
    """dmx on lg_hyper_ecr, lg_hyper<2> (GST_DEBUG_EPOCHS_LDS) and lg_hyper<0>
    (GST_DEBUG_LARGE_HYPER), dmw on lg_hyper_reg<16> and lg_hyper<0>: the hyper likelihood at
    every recorded point within 1e-10 of one another, and the 12-sweep replay of the
    reference's tape makes the same MH decisions (x, z, nu bit for bit)."""
    ref = cached_ref(f"{ds}_beta_prior")
    tape = ref["tape"]
    S = int(ref["niter"])
    idx = np.repeat(np.arange(S), 11)
    st, ss = states_at(ref, idx)
    xs = tape["hyper_lnl_x"].reshape(S * 11, -1)
    rows = pack_tape(tape, np.arange(S), ref["pta"].n, ref["pta"].m,
                     _abi.TAPE_DELTA + ref["pta"].m + 2 + 2 * ref["pta"].n)
    lnl, recs = [], []
    for dbg in variants:
        ns = open_sampler(ref, S * 11, "large", **dbg)
        ns.set_state(x=xs, theta=np.array([s["theta"] for s in ss]),
                     nu=np.array([s["nu"] for s in ss]), **st)
        lnl.append(ns.eval_lnlike()[1])
        ns.close()
        ns = open_sampler(ref, 1, "large", **dbg)
        assert ns.stride == rows.shape[1]
        ns.set_state(**start_state(ref, 1))
        rec = ns.alloc_records(S, keys=("x", "z", "nu"))
        ns.sweep(S, records=rec, tape=upload_tape(ns, rows[None]))
        recs.append({k: v.cpu().numpy() for k, v in rec.items()})
        ns.close()
    assert np.isfinite(lnl[0]).sum() > 100
    for k in range(1, len(variants)):
        r = rel(lnl[k], lnl[0])
        assert np.all(r <= RTOL), (variants[k], r.max())
        for key in ("x", "z", "nu"):
            np.testing.assert_array_equal(recs[k][key], recs[0][key], err_msg=f"{variants[k]} {key}")
    assert np.ptp(recs[0]["x"][0], axis=0).astype(bool).sum() >= 4   # both processes moved


# ---- launch boundaries of the persistent kernel -----------------------------------------------
S_INV = 24


def _launch(ref, C, waves, init, S, seed, sweep0, poison=False):
    ns = open_sampler(ref, C, "persistent", waves, poison=poison)
    ns.set_state(**init)
    return launch_records(ns, S, seed=seed, sweep0=sweep0)


@pytest.fixture(scope="module")
def long_runs():
    """One launch of S_INV sweeps per (dataset, build), shared by the tests below."""
    cache = {}

    def get(ds, build):
        if (ds, build) not in cache:
            ref = cached_ref(f"{ds}_beta_fixed")
            C, waves = builds()[build]
            init = start_state(ref, C, 21)
            cache[ds, build] = (init,) + _launch(ref, C, waves, init, S_INV, 11, 5)
        return cache[ds, build]
    return get


@pytest.mark.parametrize("ds", ["dmg", "dme"])
@pytest.mark.parametrize("build", ["occ1", "pair", "occ2"])
def test_one_launch_equals_single_sweep_launches(ds, build, long_runs):
    ref = cached_ref(f"{ds}_beta_fixed")
    C, waves = builds()[build]
    init, rec, long_state = long_runs(ds, build)
    ns = open_sampler(ref, C, "persistent", waves)
    ns.set_state(**init)
    bad = single_sweep_differences(ns, rec, long_state, S_INV, 11, 5)
    assert not bad, f"{build}: first difference (sweep, array) {bad[:4]}"
    x = rec["x"].cpu().numpy()
    moved = (np.ptp(x, axis=1) > 0).any(axis=0)
    assert all(moved[q.idx_log10_A] and moved[q.idx_gamma] for q in ref["pta"].procs)
    assert np.all((long_state["status"].cpu().numpy() & _abi.STATUS_ERRORS) == 0)


@pytest.mark.parametrize("ds", ["dmg", "dme"])
@pytest.mark.parametrize("build", ["occ1", "pair", "occ2"])
def test_poisoned_lds_and_scratch_change_nothing(ds, build, long_runs):
    ref = cached_ref(f"{ds}_beta_fixed")
    C, waves = builds()[build]
    init, rec, state = long_runs(ds, build)
    rec_p, state_p = _launch(ref, C, waves, init, S_INV, 11, 5, poison=True)
    for k in KEYS:
        assert torch.equal(rec[k], rec_p[k]), f"{build}: record {k} differs under poisoning"
    for k in KEYS + ("status",):
        assert torch.equal(state[k], state_p[k]), f"{build}: final {k} differs under poisoning"


@pytest.mark.parametrize("ds", ["dmg", "dme"])
def test_builds_agree(ds, long_runs):
    """Two waves per chain equal one wave, and the two-chains-per-SIMD build equals the
    one-chain build on the chains they share (Philox keyed by chain, the same starts)."""
    init1, rec1, st1 = long_runs(ds, "occ1")
    init2, rec2, st2 = long_runs(ds, "pair")
    init3, rec3, st3 = long_runs(ds, "occ2")
    C = rec1["x"].shape[0]
    np.testing.assert_array_equal(init1["x"], init3["x"][:C])
    for k in KEYS:
        assert torch.equal(rec1[k], rec2[k]), f"two waves: record {k}"
        assert torch.equal(rec1[k], rec3[k][:C]), f"two chains per SIMD: record {k}"
    for k in KEYS + ("status",):
        assert torch.equal(st1[k], st2[k]), f"two waves: final {k}"
        assert torch.equal(st1[k], st3[k][:C]), f"two chains per SIMD: final {k}"


def test_large_path_chain_is_independent_of_its_batch():
    """A dmw chain (lg_hyper_reg<16>: the process boundary at column 60, inside the first 64
    lanes) run alone is bitwise the chain it is among 40."""
    ref = cached_ref("dmw_beta_fixed")
    C, S, who = 40, 6, 23
    init = start_state(ref, C, 31)
    ns = open_sampler(ref, C, "large")
    ns.set_state(**init)
    rec = ns.alloc_records(S)
    ns.sweep(S, records=rec, seed=5, sweep0=2)
    many = {k: v.cpu().numpy()[who] for k, v in rec.items()}
    fin = ns.get_state()
    ns.close()
    ns = open_sampler(ref, 1, "large")
    ns.set_state(**{k: v[who:who + 1] for k, v in init.items()})
    rec = ns.alloc_records(S)
    ns.sweep(S, records=rec, seed=5, sweep0=2, chain0=who)
    one = {k: v.cpu().numpy()[0] for k, v in rec.items()}
    fin1 = ns.get_state()
    ns.close()
    for k in KEYS:
        np.testing.assert_array_equal(one[k], many[k], err_msg=k)
        np.testing.assert_array_equal(fin1[k][0], fin[k][who], err_msg=f"final {k}")
    assert np.ptp(many["x"], axis=0).astype(bool).sum() >= 3


# ---- Philox mode against the mirror's tape ------------------------------------------------------
@pytest.mark.parametrize("ds,path", [("dmg", "persistent"), ("dmx", "large")])
def test_hyper_mh_follows_the_mirror(ds, path):
    """The white and hyper MH blocks in Philox mode against the same launch in tape mode on the
    tape oracle/philox_variates.py writes, with 4 (dmg) and 6 (dmx) hyper indices: the same
    parameters move at every sweep and x agrees within 1e-12 of the prior range.  A wrong
    index table (a process's log10_A / gamma taken for another's) shows here."""
    ref = cached_ref(f"{ds}_beta_fixed")
    pta = ref["pta"]
    orc = Oracle(pta, OutlierModel(**ref["kw"]))
    assert len(orc.hind) == (4 if ds == "dmg" else 6)
    C, S, seed, sweep0, chain0 = 16, 6, 2**40 + 77, 1000, 300
    mask = _abi.STAGE_WHITE | _abi.STAGE_HYPER
    out = []
    for mode in ("philox", "tape"):
        ns = open_sampler(ref, C, path, 1 if path == "persistent" else None)
        ns.set_state(**start_state(ref, C))
        rec = ns.alloc_records(S, keys=("x",))
        if mode == "philox":
            ns.sweep(S, records=rec, mask=mask, seed=seed, sweep0=sweep0, chain0=chain0)
        else:
            tape = np.zeros((C, S, ns.stride))
            tape[:, :, :120] = pv.mh_tape(seed, chain0 + np.arange(C), sweep0 + np.arange(S),
                                          orc.wind, orc.hind)
            ns.sweep(S, records=rec, mask=mask, tape=upload_tape(ns, tape))
        fin = ns.get_state()
        assert np.all((fin["status"] & _abi.STATUS_ERRORS) == 0)
        out.append(np.concatenate([rec["x"].cpu().numpy(), fin["x"][:, None]], axis=1))
        ns.close()
    gx, wx = out
    moved = np.diff(gx, axis=1) != 0
    np.testing.assert_array_equal(moved, np.diff(wx, axis=1) != 0)
    for q in pta.procs:       # every process's parameters moved somewhere
        assert moved[..., q.idx_log10_A].any() and moved[..., q.idx_gamma].any(), q.name
    rng_ = np.array([p.pmax - p.pmin for p in pta.params])
    err = (np.abs(gx - wx) / rng_).max()
    print(ds, path, "moves", int(moved.sum()), "max |dx| / range", err)
    assert err <= 1e-12, err


# ---- the public class -----------------------------------------------------------------------------
def test_gibbs_class_with_a_dm_process(tmp_path):
    """Gibbs(PTA(psr, dm_gp=...), model="mixture", nchains=64).sample(..., accumulate=True) on
    dmg's pulsar, built through the public constructors: clean status, x inside the prior box,
    finite posterior sums, and a checkpoint round trip that continues the chains bitwise."""
    psr = data.multiband(60, 3, seed=1644, band_mhz=np.linspace(1150.0, 1850.0, 3),
                         dm=(-13.3, 2.8, 5))
    pta = PTA(psr, components=7, dm_gp=dict(components=5))
    assert [q.ncol for q in pta.procs] == [14, 10] and len(pta.params) == 5
    kw = dict(model="mixture", nchains=64, seed=99, chunk=16)
    lo, hi = prior_box(pta)
    x0 = np.random.default_rng(3).uniform(lo, hi, size=(64, 5))
    N, M = 30, 20
    g = Gibbs(pta, **kw)
    assert g._native.path == "persistent" and g._native.procs.nproc == 2
    xa = g.sample(x0, niter=N + M, accumulate=True)
    assert np.all((g._native.get_state()["status"] & _abi.STATUS_ERRORS) == 0)
    assert np.all((g.chain >= lo) & (g.chain <= hi)) and np.all((xa >= lo) & (xa <= hi))
    assert all(np.ptp(g.chain[..., j]) > 0 for j in range(5))
    post = g.post
    assert int(np.min(post.count)) == N + M
    for k in ("z_sum", "pout_sum", "alpha_sum", "b_sum", "b_sq"):
        assert np.all(np.isfinite(getattr(post, k))), k
    full = {k: getattr(g, k).copy() for k in ("chain", "bchain", "zchain", "alphachain",
                                               "poutchain", "thetachain", "dfchain")}
    g.close()
    h = Gibbs(pta, **kw)
    h.sample(x0, niter=N)
    h.save_checkpoint(tmp_path / "ck.npz")
    h.close()
    r = Gibbs(pta, **dict(kw, seed=1))          # the key comes from the file
    x = r.load_checkpoint(tmp_path / "ck.npz")
    xb = r.sample(x, niter=M)
    for k, v in full.items():
        np.testing.assert_array_equal(getattr(r, k), v[:, N:], err_msg=k)
    np.testing.assert_array_equal(xb, xa)
    r.close()
