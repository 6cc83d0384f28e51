"""The block second moment of b kept on the device (gst_set_accum_block, include/gst.h): while
gst_set_accum is set, every counted sweep adds b_i b_j of its start-of-sweep b -- the b a
record of that sweep holds -- into the packed lower triangle of a chosen column range, one
owner per element, in sweep order.  A sum is therefore the sequential sum of the recorded
products to one rounding per term and addition, on every kernel variant, whatever
record_every is, and keeping it changes nothing else."""
import ctypes as ct

import numpy as np
import pytest

from block_support import assert_waveform, mgp_model
from gpu_block_support import (BLOCK_KEYS, REC_KEYS, block_alloc, cached_block_run,
                               check_block_sums)
from gpu_support import ACCUM_SEED, accum_sampler, builds, upload_tape
from gibbs_student_t_amd import Gibbs, _abi, run_sims
from gibbs_student_t_amd.native import ACCUM_KEYS, model_desc, pack_tape
from gibbs_student_t_amd.post import PosteriorSums
from golden_io import load_ref, sweep_state

pytestmark = pytest.mark.gpu

# one case per code path: (fixture, path, waves, block)
CASES = {
    "one_wave_whole_b": ("beta_fixed", "persistent", 1, (0, 74)),     # ncol > 64, into the TM
    "pair": ("beta_fixed", "persistent", 2, (0, 60)),
    "gen_dm_gp": ("dmg_beta_fixed", "persistent", None, (14, 10)),    # col0 != 0
    "gen_ecorr": ("dme_beta_fixed", "persistent", None, (10, 10)),
    "wide_boundary": ("wide_beta_fixed", "persistent", None, (59, 2)),  # Fourier | timing model
    "large_100": ("dmw_beta_fixed", "large", None, (0, 100)),
    "large_dm_gp": ("dmw_beta_fixed", "large", None, (60, 40)),
    "large_epochs_first": ("dmx_beta_fixed", "large", None, (20, 20)),  # reference column order
    "large_130": ("dm3_beta_fixed", "large", None, (0, 130)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_sums_equal_recorded_chains(case):
    """8 chains, 24 sweeps in three launches of 8, sums from sweep0 + 5 on: every element of the
    block is the sum over records 5..23 of b_i b_j, N = 19"""
    name, path, waves, block = CASES[case]
    out = cached_block_run(name, 8, block, path, waves)
    assert out["path"] == path and block[0] + block[1] <= out["m"]
    assert out["rec"]["b"].shape[:2] == (8, 24)
    check_block_sums(out["rec"]["b"], out["sums"]["b_outer"], block, 5, case)
    assert np.all(out["sums"]["count"] == 19)


def test_two_chains_per_simd():
    """More chains than SIMDs (the two-chains-per-SIMD instance), the smallest block"""
    C, waves = builds()["occ2"]
    out = cached_block_run("beta_fixed", C, (0, 1), "persistent", waves)
    check_block_sums(out["rec"]["b"], out["sums"]["b_outer"], (0, 1), 5, "occ2")
    assert out["sums"]["b_outer"].shape == (C, 1) and np.all(out["sums"]["count"] == 19)


@pytest.mark.parametrize("path,waves,block", [("persistent", 1, (0, 74)),
                                              ("persistent", 2, (0, 60)), ("large", None, (0, 74))])
def test_block_changes_nothing_else(path, waves, block):
    """With and without the block: records, final state and every other sum bitwise equal"""
    a = cached_block_run("beta_fixed", 8, block, path, waves)
    b = cached_block_run("beta_fixed", 8, None, path, waves)
    for k in REC_KEYS:
        np.testing.assert_array_equal(a["rec"][k], b["rec"][k], err_msg=f"rec {k}")
    for k in b["state"]:
        np.testing.assert_array_equal(a["state"][k], b["state"][k], err_msg=f"state {k}")
    for k in ACCUM_KEYS:
        np.testing.assert_array_equal(a["sums"][k], b["sums"][k], err_msg=k)
    if path == "large":
        check_block_sums(a["rec"]["b"], a["sums"]["b_outer"], block, 5, "large beta_fixed")


@pytest.mark.parametrize("path,block", [("persistent", (0, 74)), ("large", (0, 74))])
def test_thinned_run_has_the_same_block_sums(path, block):
    """The block counts every sweep whatever record_every is"""
    waves = 1 if path == "persistent" else None
    full = cached_block_run("beta_fixed", 8, block, path, waves)
    thin = cached_block_run("beta_fixed", 8, block, path, waves, 4)
    assert thin["rec"]["b"].shape[1] == 6
    np.testing.assert_array_equal(thin["sums"]["b_outer"], full["sums"]["b_outer"])
    assert np.all(thin["sums"]["count"] == 19)


@pytest.mark.parametrize("path", ["persistent", "large"])
def test_tape_mode_accumulates_the_block_too(path):
    """Parity launches (injected variates: the persistent kernel's tape instances)"""
    ref = load_ref("beta_fixed")
    S, C, burn, block = int(ref["niter"]), 5, 2, (30, 44)
    ns, _, _ = accum_sampler(["beta_fixed"], C, path)
    ns.set_state(x=np.tile(ref["xs"], (C, 1)))
    rows = pack_tape(ref["tape"], np.arange(S), ns.n, ns.m, ns.stride)
    tape = upload_tape(ns, np.tile(rows, (C, 1, 1)))
    acc = ns.alloc_accum(BLOCK_KEYS, b_block=block)
    ns.set_accum(acc, from_sweep=burn, b_block=block)
    rec = ns.alloc_records(S, ("b",))
    ns.sweep(S, records=rec, tape=tape)
    bb, b = acc["b_outer"].cpu().numpy(), rec["b"].cpu().numpy()
    count = acc["count"].cpu().numpy()
    ns.close()
    check_block_sums(b, bb, block, burn, f"tape {path}")
    assert np.all(count == S - burn) and S - burn >= 3


@pytest.mark.parametrize("path", ["persistent", "large"])
def test_block_without_accum_and_switching_off(path):
    """A block without gst_set_accum writes nothing; after gst_set_accum_block(NULL) the buffer
    no longer changes while the other sums go on"""
    block = (3, 66)
    ns, refs, _ = accum_sampler(["beta_fixed"], 8, path)
    n_of = np.full(8, refs[0]["pta"].n)
    acc = block_alloc(ns, n_of, block)
    ns.set_accum_block(acc, block)
    ns.sweep(4, seed=ACCUM_SEED, sweep0=0)
    assert not acc["b_outer"].any().item() and not acc["count"].any().item()
    ns.set_accum(acc, from_sweep=0, b_block=block)
    ns.sweep(4, seed=ACCUM_SEED, sweep0=4)
    bb1, bs1 = acc["b_outer"].clone(), acc["b_sum"].clone()
    assert bb1.any().item() and np.all(acc["count"].cpu().numpy() == 4)
    ns.set_accum_block(None)
    ns.sweep(4, seed=ACCUM_SEED, sweep0=8)
    assert np.all(acc["count"].cpu().numpy() == 8)
    assert (acc["b_outer"] == bb1).all().item()
    assert not (acc["b_sum"] == bs1).all().item()
    # clear_accum switches the block off with the rest
    ns.set_accum(acc, from_sweep=0, b_block=block)
    ns.clear_accum()
    ns.sweep(2, seed=ACCUM_SEED, sweep0=12)
    assert (acc["b_outer"] == bb1).all().item() and np.all(acc["count"].cpu().numpy() == 8)
    ns.close()


def test_validation():
    """Every bad descriptor returns < 0 with a message and leaves the sampler usable; a block
    needs a model, and a later gst_model_set* switches it off"""
    ref = load_ref("beta_fixed")
    ns, _, _ = accum_sampler(["beta_fixed"], 8, "persistent")
    lib, m = ns.lib, ns.m
    acc = ns.alloc_accum(BLOCK_KEYS, b_block=(0, m))
    ptr = ct.c_void_p(acc["b_outer"].data_ptr())
    ns.set_accum(acc, from_sweep=0, b_block=(0, m))
    for col0, ncol, word in ((-1, 4, "col0"), (0, 0, "ncol"), (0, -3, "ncol"),
                             (0, _abi.BLOCK_MAX + 1, "ncol"), (m - 3, 4, "col0 + ncol"),
                             (m, 1, "col0 + ncol"), (2 ** 31 - 1, 2, "col0 + ncol")):
        blk = _abi.AccumBlock(col0, ncol, ptr)
        assert lib.gst_set_accum_block(ns.ctx, ct.byref(blk)) < 0, (col0, ncol)
        msg = _abi.last_error(lib)
        assert "gst_set_accum_block" in msg and word in msg, msg
    with pytest.raises(ValueError):
        ns.set_accum_block(acc, (0, m + 1))
    with pytest.raises(ValueError, match="b_block"):
        ns.set_accum(acc, from_sweep=0)
    with pytest.raises(ValueError, match="b_outer needs b_block"):
        ns.alloc_accum(("b_outer",))
    # the failed calls left the block as it was: the sampler runs and the whole-b block adds
    ns.sweep(3, seed=ACCUM_SEED, sweep0=0)
    assert np.all(acc["count"].cpu().numpy() == 3) and acc["b_outer"].any().item()
    # a later gst_model_set switches the block off (its columns were checked against the old m)
    bb = acc["b_outer"].clone()
    desc, keep = model_desc(ref["pta"], ref["kw"])
    _abi.check(lib, lib.gst_model_set(ns.ctx, ct.byref(desc)), "gst_model_set")
    ns.sweep(3, seed=ACCUM_SEED, sweep0=3)
    assert np.all(acc["count"].cpu().numpy() == 6) and (acc["b_outer"] == bb).all().item()
    del keep
    ns.close()
    # before any model
    ctx = ct.c_void_p()
    _abi.check(lib, lib.gst_ctx_create(0, ct.byref(ctx)), "gst_ctx_create")
    blk = _abi.AccumBlock(0, 1, ptr)
    assert lib.gst_set_accum_block(ctx, ct.byref(blk)) < 0
    assert "no model" in _abi.last_error(lib)
    assert lib.gst_set_accum_block(ctx, None) == 0        # switching off needs none
    _abi.check(lib, lib.gst_ctx_destroy(ctx), "gst_ctx_destroy")


def test_gibbs_b_cov_arguments():
    ref = load_ref("beta_fixed")
    g = Gibbs(ref["pta"], **ref["kw"], nchains=2, seed=3)
    with pytest.raises(ValueError, match="accumulate=True"):
        g.sample(ref["xs"], niter=2, b_cov="red")
    with pytest.raises(ValueError, match="unknown process"):
        g.sample(ref["xs"], niter=2, accumulate=True, b_cov="dm_gp")
    with pytest.raises(ValueError, match="columns must lie"):
        g.sample(ref["xs"], niter=2, accumulate=True, b_cov=(70, 5))
    g.sample(ref["xs"], niter=3, accumulate=True, b_cov="all")
    assert g.post.b_block == (0, 74) and g.post.b_outer.shape == (2, 74 * 75 // 2)
    g.close()


def test_process_waveform_end_to_end():
    """Gibbs.sample(b_cov="dm_gp") on the dmg model: the DM waveform's mean and band at the TOAs
    equal those of B @ bchain[..., 14:24] over chains x sweeps 10..59, and on a dense grid and in
    DM units they come from the same sums"""
    pta, _ = mgp_model("dmg")
    ref = load_ref("dmg_beta_fixed")
    np.testing.assert_array_equal(pta.T[:, :24], ref["pta"].T[:, :24])
    s0 = sweep_state(ref, 0)
    g = Gibbs(pta, **ref["kw"], nchains=8, seed=77)
    g._b, g._z, g._alpha, g._pout = s0["b"], s0["z"], s0["alpha"], s0["pout"]
    g._theta, g.tdf = s0["theta"], s0["nu"]
    g.sample(ref["xs"], niter=60, accumulate=True, burn=10, b_cov="dm_gp", record=("b",))
    post, bchain = g.post, g.bchain
    g.close()
    assert isinstance(post, PosteriorSums) and post.b_block == (14, 10)
    assert np.all(post.count == 50) and bchain.shape == (8, 60, pta.m)
    B = pta.process_basis("dm_gp")
    np.testing.assert_array_equal(B, pta.T[:, 14:24])
    samples = bchain[:, 10:, 14:24]
    mean, sd = post.process_waveform(pta, "dm_gp")
    assert mean.shape == sd.shape == (pta.n,) and np.all(sd > 0)
    assert_waveform(mean, sd, B, samples.reshape(-1, 10), "dm_gp pooled")
    mean_c, sd_c = post.process_waveform(pta, "dm_gp", pool=False)
    for c in (0, 7):
        assert_waveform(mean_c[c], sd_c[c], B, samples[c], f"dm_gp chain {c}")
    # a dense grid beyond the TOAs, in DM units
    t = np.linspace(pta.psr.toas.min() - 0.05 * pta.Tspan, pta.psr.toas.max() + 0.05 * pta.Tspan,
                    101)
    Bg = pta.process_basis("dm_gp", toas=t, scaled=False) * (2.41e-4 * 1400.0 ** 2)
    mg, sg = post.process_waveform(pta, "dm_gp", toas=t, units="dm")
    assert_waveform(mg, sg, Bg, samples.reshape(-1, 10), "dm_gp grid, DM units")
    with pytest.raises(ValueError, match="block kept"):
        post.process_waveform(pta, "red")


def test_run_sims_writes_the_block(tmp_path):
    """run_sims --post --b-cov red: each entry's post.npz holds its chains' block, equal to the
    sums over its written bchain"""
    run_sims.main(["--thetas", "0.1", "--models", "beta", "--chains", "2", "--niter", "40",
                   "--burn", "10", "--chunk", "16", "--outdir", str(tmp_path), "--generator",
                   "host", "--seed", "7", "--post", "--b-cov", "red"])
    entries = run_sims.build_grid((0.1,), 1, ("beta",), 7, generator="host")
    assert len(entries) == 2
    for e in entries:
        d = e.outdir(str(tmp_path))
        post = PosteriorSums.load(d + "/post.npz")
        bchain = np.load(f"{d}/bchain.npy")
        lo, hi = e.pta.process_columns("red")
        assert post.b_block == (lo, hi - lo) and np.all(post.count == 30)
        assert bchain.shape[:2] == (2, 30)
        check_block_sums(bchain, post.b_outer, post.b_block, 0, "run_sims")
