"""Models with several power-law processes (red noise + DM (+ chromatic)): the kernel variants
agree with one another, the persistent kernel's launch-boundary invariants hold on its general
instances with a process boundary inside the Fourier block (dmg: column 14 of 24; dme: column
10 of 20, then 24 ECORR columns), a large-path chain does not depend on its batch partners,
the Philox-mode hyper MH block follows the tape the numpy mirror writes over every process's
parameters, and the public ``Gibbs`` class runs such a model with a checkpoint round trip."""
import numpy as np
import pytest

from golden_io import sweep_state
import mgp_io

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("needs a HIP device", allow_module_level=True)

from gibbs_student_t_amd import _abi  # noqa: E402
from gibbs_student_t_amd.native import NativeSampler, pack_tape  # noqa: E402
from gibbs_student_t_amd.sampler import Gibbs  # noqa: E402
from oracle import philox_variates as pv  # noqa: E402
from oracle.gibbs_oracle import Oracle, OutlierModel  # noqa: E402
from test_gpu_parity import _rel, _states  # noqa: E402
from test_gpu_waves import KEYS, _init  # noqa: E402

RTOL = 1e-10


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = mgp_io.load_ref(name)
        return cache[name]
    return get


def _native(ref, C, path, **debug):
    ns = NativeSampler(ref["pta"], ref["kw"], 0, path=path)
    assert ns.path == path
    ns.set_debug(**debug)
    ns.alloc(C)
    return ns


# ---- kernel variants --------------------------------------------------------------------------
@pytest.mark.parametrize("ds,variants", [
    ("dmx", ({}, dict(epochs_lds=True), dict(large_hyper=True))),
    ("dmw", ({}, dict(large_hyper=True)))])
def test_kernel_variants_agree(ds, variants, refs):
    """dmx on lg_hyper_ecr, lg_hyper<2> (GST_DEBUG_EPOCHS_LDS) and lg_hyper<0>
    (GST_DEBUG_LARGE_HYPER), dmw on lg_hyper_reg<16> and lg_hyper<0>: the hyper likelihood at
    every recorded point within 1e-10 of one another, and the 12-sweep replay of the
    reference's tape makes the same MH decisions (x, z, nu bit for bit)."""
    ref = refs(f"{ds}_beta_prior")
    tape = ref["tape"]
    S = int(ref["niter"])
    idx = np.repeat(np.arange(S), 11)
    st, ss = _states(ref, idx)
    xs = tape["hyper_lnl_x"].reshape(S * 11, -1)
    s0 = sweep_state(ref, 0)
    rows = pack_tape(tape, np.arange(S), ref["pta"].n, ref["pta"].m,
                     _abi.TAPE_DELTA + ref["pta"].m + 2 + 2 * ref["pta"].n)
    lnl, recs = [], []
    for dbg in variants:
        ns = _native(ref, S * 11, "large", **dbg)
        ns.set_state(x=xs, theta=np.array([s["theta"] for s in ss]),
                     nu=np.array([s["nu"] for s in ss]), **st)
        lnl.append(ns.eval_lnlike()[1])
        ns.close()
        ns = _native(ref, 1, "large", **dbg)
        assert ns.stride == rows.shape[1]
        ns.set_state(x=ref["xs"][None], b=s0["b"][None], z=s0["z"][None],
                     alpha=s0["alpha"][None], pout=s0["pout"][None],
                     theta=np.array([s0["theta"]]), nu=np.array([s0["nu"]]))
        rec = ns.alloc_records(S, keys=("x", "z", "nu"))
        ns.sweep(S, records=rec, tape=torch.as_tensor(rows[None]).to(ns.tdev).contiguous())
        recs.append({k: v.cpu().numpy() for k, v in rec.items()})
        ns.close()
    assert np.isfinite(lnl[0]).sum() > 100
    for k in range(1, len(variants)):
        r = _rel(lnl[k], lnl[0])
        assert np.all(r <= RTOL), (variants[k], r.max())
        for key in ("x", "z", "nu"):
            np.testing.assert_array_equal(recs[k][key], recs[0][key], err_msg=f"{variants[k]} {key}")
    assert np.ptp(recs[0]["x"][0], axis=0).astype(bool).sum() >= 4   # both processes moved


# ---- launch boundaries of the persistent kernel -----------------------------------------------
def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _builds():
    # one chain per SIMD, two waves per chain, two chains per SIMD (C > 4 x CUs)
    return {"occ1": (96, 1), "pair": (96, 2), "occ2": (4 * _ncu() + 64, 1)}


S_INV = 24


def _launch(ref, C, waves, init, S, seed, sweep0, poison=False):
    ns = _native(ref, C, "persistent", poison=poison)
    ns.set_waves(waves)
    ns.set_state(**init)
    rec = ns.alloc_records(S)
    ns.sweep(S, records=rec, seed=seed, sweep0=sweep0)
    state = {k: v.clone() for k, v in ns.state.items()}
    ns.close()
    return rec, state


@pytest.fixture(scope="module")
def long_runs(refs):
    """One launch of S_INV sweeps per (dataset, build), shared by the tests below."""
    cache = {}

    def get(ds, build):
        if (ds, build) not in cache:
            ref = refs(f"{ds}_beta_fixed")
            C, waves = _builds()[build]
            init = _init(ref, C, 21)
            cache[ds, build] = (init,) + _launch(ref, C, waves, init, S_INV, 11, 5)
        return cache[ds, build]
    return get


@pytest.mark.parametrize("ds", ["dmg", "dme"])
@pytest.mark.parametrize("build", ["occ1", "pair", "occ2"])
def test_one_launch_equals_single_sweep_launches(ds, build, refs, long_runs):
    ref = refs(f"{ds}_beta_fixed")
    C, waves = _builds()[build]
    init, rec, long_state = long_runs(ds, build)
    ns = _native(ref, C, "persistent")
    ns.set_waves(waves)
    ns.set_state(**init)
    bad = []
    for s in range(S_INV):
        for k in KEYS:        # the state entering sweep s is record s of the long launch
            if not torch.equal(ns.state[k], rec[k][:, s]):
                bad.append((s, k))
        if bad:
            break
        ns.sweep(1, seed=11, sweep0=5 + s)
    if not bad:
        for k in KEYS + ("status",):
            if not torch.equal(ns.state[k], long_state[k]):
                bad.append((S_INV, k))
    ns.close()
    assert not bad, f"{build}: first difference (sweep, array) {bad[:4]}"
    x = rec["x"].cpu().numpy()
    moved = (np.ptp(x, axis=1) > 0).any(axis=0)
    assert all(moved[q.idx_log10_A] and moved[q.idx_gamma] for q in ref["pta"].procs)
    assert np.all((long_state["status"].cpu().numpy() & _abi.STATUS_ERRORS) == 0)


@pytest.mark.parametrize("ds", ["dmg", "dme"])
@pytest.mark.parametrize("build", ["occ1", "pair", "occ2"])
def test_poisoned_lds_and_scratch_change_nothing(ds, build, refs, long_runs):
    ref = refs(f"{ds}_beta_fixed")
    C, waves = _builds()[build]
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


def test_large_path_chain_is_independent_of_its_batch(refs):
    """A dmw chain (lg_hyper_reg<16>: the process boundary at column 60, inside the first 64
    lanes) run alone is bitwise the chain it is among 40."""
    ref = refs("dmw_beta_fixed")
    C, S, who = 40, 6, 23
    init = _init(ref, C, 31)
    ns = _native(ref, C, "large")
    ns.set_state(**init)
    rec = ns.alloc_records(S)
    ns.sweep(S, records=rec, seed=5, sweep0=2)
    many = {k: v.cpu().numpy()[who] for k, v in rec.items()}
    fin = ns.get_state()
    ns.close()
    ns = _native(ref, 1, "large")
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
def test_hyper_mh_follows_the_mirror(ds, path, refs):
    """The white and hyper MH blocks in Philox mode against the same launch in tape mode on the
    tape oracle/philox_variates.py writes, with 4 (dmg) and 6 (dmx) hyper indices: the same
    parameters move at every sweep and x agrees within 1e-12 of the prior range.  A wrong
    index table (a process's log10_A / gamma taken for another's) shows here."""
    ref = refs(f"{ds}_beta_fixed")
    pta = ref["pta"]
    orc = Oracle(pta, OutlierModel(**ref["kw"]))
    assert len(orc.hind) == (4 if ds == "dmg" else 6)
    C, S, seed, sweep0, chain0 = 16, 6, 2**40 + 77, 1000, 300
    mask = _abi.STAGE_WHITE | _abi.STAGE_HYPER
    s0 = sweep_state(ref, 0)
    tile = lambda v: np.tile(np.asarray(v, dtype=np.float64), (C, 1))  # noqa: E731
    out = []
    for mode in ("philox", "tape"):
        ns = _native(ref, C, path)
        if path == "persistent":
            ns.set_waves(1)
        ns.set_state(x=tile(ref["xs"]), b=tile(s0["b"]), z=tile(s0["z"]), alpha=tile(s0["alpha"]),
                     pout=tile(s0["pout"]), theta=np.full(C, s0["theta"]), nu=np.full(C, s0["nu"]))
        rec = ns.alloc_records(S, keys=("x",))
        if mode == "philox":
            ns.sweep(S, records=rec, mask=mask, seed=seed, sweep0=sweep0, chain0=chain0)
        else:
            tape = np.zeros((C, S, ns.stride))
            tape[:, :, :120] = pv.mh_tape(seed, chain0 + np.arange(C), sweep0 + np.arange(S),
                                          orc.wind, orc.hind)
            ns.sweep(S, records=rec, mask=mask,
                     tape=torch.as_tensor(tape).to(ns.tdev).contiguous())
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
    from gibbs_student_t_amd import data
    from gibbs_student_t_amd.model import PTA
    psr = data.multiband(60, 3, seed=1644, band_mhz=np.linspace(1150.0, 1850.0, 3),
                         dm=(-13.3, 2.8, 5))
    pta = PTA(psr, components=7, dm_gp=dict(components=5))
    assert [q.ncol for q in pta.procs] == [14, 10] and len(pta.params) == 5
    kw = dict(model="mixture", nchains=64, seed=99, chunk=16)
    lo = np.array([p.pmin for p in pta.params])
    hi = np.array([p.pmax for p in pta.params])
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
