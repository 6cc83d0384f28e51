"""DM and chromatic power-law processes beside the red noise (PTA(dm_gp=, chrom_gp=),
gst_model_set_procs) on the GPU against the reference's recorded runs
(tests/golden/mgp_ref_*.npz, tools/gen_golden.py multi_gp): the kernel each dataset runs on,
both likelihoods at every point the reference evaluated, the MH blocks and the b draw from
every recorded start, and the 12-sweep replay against the oracle.  Tolerances are
test_gpu_parity's: continuous outputs <= 1e-10 relative, discrete draws exact."""
import ctypes as ct
import functools
import subprocess

import numpy as np
import pytest

from gpu_support import open_sampler, replay, upload_tape
from gibbs_student_t_amd import _abi
from gibbs_student_t_amd.native import NativeSampler, model_desc, pack_tape
from golden_io import MGP_DATASETS, MGP_NAMES, load_ref, oracle_replay
from support import (RTOL, assert_b_within_reference_error, assert_lnl_within_reference_error,
                     assert_replay_matches, cached_ref, chain_state, host_tool, rel,
                     start_state, states_at)

pytestmark = pytest.mark.gpu

# the large path's hyper kernel of each dataset (tools/plan_dump.cpp names), by debug flags
LARGE_KERNEL = {
    ("dmw", ""): "hyper_reg<16>", ("dmw", "large_hyper"): "hyper<0>",
    ("dm3", ""): "hyper<0>",
    ("dmx", ""): "hyper_ecr<8,62>", ("dmx", "epochs_lds"): "hyper<2>",
    ("dmx", "large_hyper"): "hyper<0>",
}
DEBUG_BITS = {"large_hyper": _abi.DEBUG_LARGE_HYPER, "epochs_lds": _abi.DEBUG_EPOCHS_LDS}
# every path that takes the model: (path, debug flag)
RUNS = {"dmg": [("persistent", ""), ("large", "")], "dme": [("persistent", ""), ("large", "")],
        "dmw": [("large", ""), ("large", "large_hyper")], "dm3": [("large", "")],
        "dmx": [("large", ""), ("large", "epochs_lds"), ("large", "large_hyper")]}
CASES = [(name, path, dbg) for name in MGP_NAMES for path, dbg in RUNS[name.split("_")[0]]]
IDS = [f"{n}-{p}{'-' + d if d else ''}" for n, p, d in CASES]


def _native(ref, C, path="auto", dbg=""):
    return open_sampler(ref, C, path, **({dbg: True} if dbg else {}))


@pytest.fixture(scope="module")
def plan_bin(tmp_path_factory):
    return host_tool(tmp_path_factory, "plan_dump", required=True)


def planned_hyper_kernel(plan_bin, pta, dbg):
    """The hyper kernel the large path's planner launches for this model."""
    r16 = lambda a: (a + 15) // 16 * 16  # noqa: E731
    nf, ntm, nec = pta.nfourier, pta.ntm, pta.n_ecorr
    ntm_pad = r16(max(ntm, 1))
    raug = ntm_pad + nf + nec
    disjoint = int(np.all((pta.T[:, nf + ntm:] != 0).sum(axis=1) <= 1))
    spec = ",".join(str(v) for v in (64 * ((pta.n + 63) // 64), r16(raug + 1), nf, nec, ntm,
                                     ntm_pad, raug, disjoint, 0))
    out = subprocess.run([plan_bin, "large", "64", str(_abi.STAGE_ALL), str(DEBUG_BITS.get(dbg, 0)),
                          "0", "1", spec], capture_output=True, text=True,
                         check=True).stdout.splitlines()
    names = [ln.split()[1] for ln in out if ln.split()[2] == "HYPER"]
    return " ".join(sorted(set(names), key=names.index))


@pytest.mark.parametrize("ds", list(MGP_DATASETS))
def test_path_of_each_dataset(ds, plan_bin):
    """dmg and dme (P = 5 and 8, 24 and 44 hyper columns) run on the persistent kernel's
    general instances, the others on the large path: dmw (100 columns) on lg_hyper_reg<16>, dm3
    (130) on lg_hyper<0>, dmx (40 Fourier + 60 ECORR) epochs first on lg_hyper_ecr."""
    ref = cached_ref(f"{ds}_beta_fixed")
    pta = ref["pta"]
    ncols, nec, path = MGP_DATASETS[ds]
    assert tuple(q.ncol for q in pta.procs) == ncols and pta.n_ecorr == nec
    assert len(pta.params) <= (8 if path == "persistent" else 16)
    ns = NativeSampler(pta, ref["kw"], 0)
    assert ns.path == path and ns.procs.nproc == len(ncols)
    ns.close()
    if path == "large":
        for (d, dbg), kernel in LARGE_KERNEL.items():
            if d == ds:
                assert planned_hyper_kernel(plan_bin, pta, dbg) == kernel, (ds, dbg)


@pytest.mark.parametrize("name,path,dbg", CASES, ids=IDS)
def test_lnlikelihoods(name, path, dbg):
    """get_lnlikelihood_white / get_lnlikelihood at every point the reference evaluated, on
    every kernel that takes the model.  The long-double value arbitrates where the reference's
    own fp64 value is inexact (test_gpu_parity.test_lnlikelihoods' rule), on at most a tenth of
    the points: the fixtures were chosen so (tools/mgp_conditioning.py)."""
    ref = cached_ref(name)
    tape = ref["tape"]
    S = int(ref["niter"])
    for which, K in (("white", 21), ("hyper", 11)):
        idx = np.repeat(np.arange(S), K)
        st, ss = states_at(ref, idx)
        xs = tape[f"{which}_lnl_x"].reshape(S * K, -1)
        want = tape[f"{which}_lnl"].reshape(-1)
        ns = _native(ref, S * K, path, dbg)
        ns.set_state(x=xs, theta=np.array([s["theta"] for s in ss]),
                     nu=np.array([s["nu"] for s in ss]), **st)
        w, h = ns.eval_lnlike()
        ns.close()
        got = w if which == "white" else h
        r = rel(got, want)
        print(f"{name} {path} {dbg} {which}: max rel {np.nanmax(r):.3e}")
        bad = np.flatnonzero(r > RTOL)
        assert len(bad) <= 0.1 * len(want), f"{which}: {len(bad)} of {len(want)} points arbitrated"
        for k in bad:
            assert which == "hyper", f"white lnL mismatch {r[k]:.3e} at {k}"
            assert_lnl_within_reference_error(ref["pta"], chain_state(ss[k]), xs[k], got[k],
                                              want[k], f"{which}[{k}]")


@pytest.mark.parametrize("name,path,dbg", CASES, ids=IDS)
def test_mh_blocks_and_b_draw(name, path, dbg):
    """White MH + Gram + hyper MH + b draw, each sweep from the reference's recorded start: x
    bit-exact (the same MH decisions over every process's parameters), b within 1e-9 of the
    Cholesky mean plus the recorded draw term."""
    ref = cached_ref(name)
    S = int(ref["niter"])
    idx = np.arange(S)
    st, ss = states_at(ref, idx)
    ns = _native(ref, S, path, dbg)
    ns.set_state(x=ref["chain"][:S], theta=np.array([s["theta"] for s in ss]),
                 nu=np.array([s["nu"] for s in ss]), **st)
    rows = pack_tape(ref["tape"], idx, ns.n, ns.m, ns.stride)
    ns.sweep(1, mask=_abi.STAGE_WHITE | _abi.STAGE_HYPER | _abi.STAGE_B,
             tape=upload_tape(ns, rows[:, None, :]))
    out = ns.get_state()
    ns.close()
    assert np.all((out["status"] & _abi.STATUS_ERRORS) == 0)
    np.testing.assert_array_equal(out["x"][:S - 1], ref["chain"][1:S])
    t = ref["tape"]
    drew = ~np.isnan(t["b_cond"])
    assert drew.any()
    want = t["b_mean_chol"] + t["b_delta"]
    for i in np.flatnonzero(drew):
        assert not out["status"][i] & _abi.STATUS_FLOOR
        err = np.linalg.norm(out["b"][i] - want[i]) / np.linalg.norm(want[i])
        if err > 1e-9:
            x_h = ref["chain"][i + 1] if i + 1 < S else out["x"][i]
            assert_b_within_reference_error(
                ref["pta"], chain_state(ss[i]), x_h, out["b"][i], t["b_mean_chol"][i],
                t["b_delta"][i], f"sweep {i}: b err {err:.3e} (cond {t['b_cond'][i]:.2e})")
    for i in np.flatnonzero(~drew):
        np.testing.assert_array_equal(out["b"][i], ref["bchain"][i])


@pytest.fixture(scope="module")
def replays():
    return functools.lru_cache(maxsize=None)(lambda name: oracle_replay(cached_ref(name)))


@pytest.mark.parametrize("name,path,dbg", CASES, ids=IDS)
def test_full_chain_replay_vs_oracle(name, path, dbg, replays):
    """The recorded sweeps on the reference's tape against the oracle replaying the same tape
    with the Cholesky-mean b draw: discrete records exact, continuous ones <= 1e-10."""
    ref = cached_ref(name)
    S = int(ref["niter"])
    ns = _native(ref, 1, path, dbg)
    ns.set_state(**start_state(ref, 1))
    got = replay(ns, ref, S)
    ns.close()
    assert_replay_matches(got, replays(name), ref, name)


@pytest.mark.parametrize("name", ["beta_fixed", "ecb_beta_fixed", "mb_beta_fixed"])
def test_one_process_is_the_legacy_entry(name):
    """gst_model_set_procs with nproc = 1 gives bitwise the chains of gst_model_set_batch on a
    classic, a GEN and a large-path model: 20 Philox sweeps of 8 chains."""
    ref = load_ref(name)
    outs = []
    for procs in (False, True):
        ns = NativeSampler(ref["pta"], ref["kw"], 0)
        assert ns.procs.nproc == 1
        if procs:
            desc, keep = model_desc(ref["pta"], ref["kw"])
            arr = (_abi.ModelDesc * 1)(desc)
            _abi.check(ns.lib, ns.lib.gst_model_set_procs(ns.ctx, arr, ct.byref(keep["procs"]), 1),
                       "gst_model_set_procs")
        ns.alloc(8)
        ns.set_state(**start_state(ref, 8))
        rec = ns.alloc_records(20)
        ns.sweep(20, records=rec, seed=77)
        outs.append(({k: v.cpu().numpy() for k, v in rec.items()}, ns.get_state(), ns.path))
        ns.close()
    assert outs[0][2] == outs[1][2]
    assert len(np.unique(outs[0][0]["x"][:, -1], axis=0)) > 1     # the chains moved apart
    for k in outs[0][0]:
        np.testing.assert_array_equal(outs[0][0][k], outs[1][0][k], err_msg=k)
    for k in outs[0][1]:
        np.testing.assert_array_equal(outs[0][1][k], outs[1][1][k], err_msg=k)
