"""Philox-mode conditional draws against their exact laws, one kernel at a time.

The single-stage tests start C chains from one fixed state and run S sweeps in Philox mode
with a single-stage mask.  No stage changes its own inputs (Sigma and d do not depend on b; z
depends on b, alpha, theta, x; ...), so every chain-sweep is one independent draw of the same
law, N = C S in all: records 1..S-1 (the state before sweep k) plus the final state.  The
statistics and their bounds are draw_laws.py's; test_draw_laws_cpu.py shows that the oracle's
own fp64 draws pass them at these states and sizes.  The combined-mask tests (theta, z, alpha
and nu in one launch, the fused pass of a full sweep) hold each chain-sweep to the law at its
own inputs; the MH test compares with tape mode on the tape a numpy mirror of Philox writes.
The b cases assert which kernel drew: the path, the persistent kernel's shape rule (csrc/gst.hip
shape_for) or the large path's planner (csrc/gst_plan.h through tools/plan_dump.cpp) together
with the launch counters.

The observed statistics of an MI355X run are in profiles/draw_laws.json.
"""
import json
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.stats

import draw_laws as dl
from gpu_support import upload_tape
from gibbs_student_t_amd import _abi
from gibbs_student_t_amd._abi import STATUS_ERRORS, STATUS_FLOOR
from gibbs_student_t_amd.native import NativeSampler
from oracle import philox_variates as pv
from oracle.gibbs_oracle import DF_GRID, Oracle, OutlierModel
from support import host_tool

pytestmark = pytest.mark.gpu

DEBUG_BITS = {"large_hyper": _abi.DEBUG_LARGE_HYPER, "epochs_lds": _abi.DEBUG_EPOCHS_LDS}
# seeds and counter offsets are constants: (seed, sweep0, chain0) by case parity
SEEDS = ((0x5EED0001, 0, 0), (0x9E3779B97F4A7C15, 1_000_003, 3_000_000_019))
OBSERVED = os.environ.get("GST_DRAW_LAWS_JSON")      # write the observed statistics here


def observe(test, case, stats):
    if OBSERVED:
        try:
            with open(OBSERVED) as f:
                book = json.load(f)
        except (OSError, ValueError):
            book = {}
        cases = book.setdefault("cases", {}).setdefault(test, {})
        cases[case] = {k: (float(v) if isinstance(v, (float, np.floating)) else v)
                       for k, v in stats.items()}
        # per test: the smallest p-value, the largest z-score and the largest correlation
        pick = lambda pre, f: f([v for s in cases.values() for k, v in s.items()  # noqa: E731
                                 if k.startswith(pre)] or [None])
        book.setdefault("summary", {})[test] = {
            "min_p": pick("p_", min), "max_z": pick("z_", max), "max_corr": pick("corr_", max)}
        with open(OBSERVED, "w") as f:
            json.dump(book, f, indent=1, sort_keys=True)


def launch(pta, kw, st, x, path, mask, C, S, seed, sweep0=0, chain0=0, debug=None,
           keys=("b",), timing=False, tape=None):
    """C chains from (st, x), S sweeps of ``mask``: ({key: draws [C, S, ...]}, status [C],
    kernel launch counts).  One wave per chain on the persistent path."""
    ns = NativeSampler(pta, kw, 0, path=path)
    assert ns.path == path
    ns.set_debug(**(debug or {}))
    if path == "persistent":
        ns.set_waves(1)
    ns.alloc(C)
    tile = lambda v: np.tile(np.asarray(v, dtype=np.float64), (C, 1))  # noqa: E731
    ns.set_state(x=tile(x), b=tile(st.b), z=tile(st.z), alpha=tile(st.alpha), pout=tile(st.pout),
                 theta=np.full(C, st.theta), nu=np.full(C, float(st.nu)))
    if timing:
        ns.set_timing(True)
    rec = ns.alloc_records(S, keys=keys)
    tp = None if tape is None else upload_tape(ns, tape)
    ns.sweep(S, records=rec, mask=mask, seed=seed, sweep0=sweep0, chain0=chain0, tape=tp)
    fin = ns.get_state()
    counts = {k: v[1] for k, v in ns.kernel_times().items()} if timing else {}
    out = {k: np.concatenate([rec[k].cpu().numpy()[:, 1:], fin[k][:, None]], axis=1) for k in keys}
    ns.close()
    return out, fin["status"], counts


# ---- which kernel ran ----------------------------------------------------------------------
def persistent_shape(pta):
    """The register-resident shape of csrc/gst.hip shape_for for this model, as "MT m K0 k"
    or "GEN MT m K0 k" (general white noise: the ECORR columns join the hyper block)."""
    gen = int(getattr(pta, "nbackend", 1)) > 1 or int(getattr(pta, "n_ecorr", 0)) > 0
    nf = pta.nfourier + (int(getattr(pta, "n_ecorr", 0)) if gen else 0)
    table = ((8, 2, 62), (10, 2, 76)) if gen else ((8, 2, 56), (10, 2, 76), (10, 3, 76))
    for MT, K0, RA in table:
        if 8 * K0 >= max(pta.ntm, 1) and RA - 8 * K0 >= nf:
            return ("GEN " if gen else "") + f"MT {MT} K0 {K0}"
    return None


PERSISTENT_SHAPES = {"MT 10": "MT 10 K0 2", "MT 8": "MT 8 K0 2", "K0 3": "MT 10 K0 3",
                     "GEN": "GEN MT 8 K0 2"}


@pytest.fixture(scope="module")
def plan_bin(tmp_path_factory):
    return host_tool(tmp_path_factory, "plan_dump", required=True)


def planned_b_kernels(plan_bin, pta, mask, debug):
    """The hyper / lg_btm kernels the planner launches for this model (the integers of
    gst_model_set_batch's large-path packing), e.g. "hyper_reg<8> btm"."""
    r16 = lambda a: (a + 15) // 16 * 16  # noqa: E731
    nf, ntm, nec = pta.nfourier, pta.ntm, int(getattr(pta, "n_ecorr", 0))
    ntm_pad = r16(max(ntm, 1))
    raug = ntm_pad + nf + nec
    T = pta.get_basis()[0]
    disjoint = int(np.all((T[:, nf + ntm:] != 0).sum(axis=1) <= 1))
    spec = ",".join(str(v) for v in (64 * ((pta.n + 63) // 64), r16(raug + 1), nf, nec, ntm,
                                     ntm_pad, raug, disjoint, 0))
    dbg = sum(DEBUG_BITS[k] for k, v in debug.items() if v)
    out = subprocess.run([plan_bin, "large", "64", str(mask), str(dbg), "0", "1", spec],
                         capture_output=True, text=True, check=True).stdout.splitlines()
    names = [ln.split()[1] for ln in out if ln.split()[2] in ("HYPER", "BTM")]
    return " ".join(sorted(set(names), key=names.index))


# ---- b ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whiteners():
    cache = {}

    def get(name):
        if name not in cache:
            pta, kw, st, x = dl.b_case(name)
            orc = Oracle(pta, OutlierModel(**kw))
            Sigma, d = orc.sigma_matrix(st, x)
            assert st.z.sum() >= 1 and orc.floor_shift(Sigma) == 0.0
            cache[name] = (pta, kw, st, x, dl.Whitener(Sigma, d))
        return cache[name]
    return get


@pytest.mark.parametrize("i", range(len(dl.B_CASES)),
                         ids=[f"{c[0]}-{c[1]}-" + re.sub("[^a-z0-9]+", "_", c[3].lower()).strip("_")
                              for c in dl.B_CASES])
def test_b_draw_law(i, whiteners, plan_bin):
    """b | rest ~ N(Sigma^-1 d, Sigma^-1) from each kernel's own back substitution of Philox
    normals: the whitened draws L^T (b - mu) are iid N(0, 1)."""
    name, path, debug, kernel = dl.B_CASES[i]
    pta, kw, st, x, white = whiteners(name)
    mask = _abi.STAGE_B | _abi.STAGE_B_FORCE
    if path == "persistent":
        assert persistent_shape(pta) == PERSISTENT_SHAPES[kernel]
    else:
        assert planned_b_kernels(plan_bin, pta, mask, debug) == kernel
    C, S = dl.C_B, dl.b_sweeps(pta.m)
    seed, sweep0, chain0 = SEEDS[i % 2]
    out, status, counts = launch(pta, kw, st, x, path, mask, C, S, seed, sweep0, chain0, debug,
                                 timing=path == "large")
    if path == "large":     # the planned kernels are the launched ones
        assert counts["hyper"] > 0 and (counts["btm"] > 0) == ("btm" in kernel), counts
    assert np.all((status & STATUS_ERRORS) == 0) and np.all((status & STATUS_FLOOR) == 0)
    b = out["b"].reshape(C * S, pta.m)
    assert np.all(np.isfinite(b))
    stats = dl.b_draw_stats(white(b))
    print(name, path, kernel, stats)
    observe("b", f"{name}/{path}/{kernel}", stats)
    dl.assert_b_draw(stats, (name, path, kernel))


# ---- theta ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", dl.THETA_K)
@pytest.mark.parametrize("name,path", dl.THETA_CASES)
def test_theta_draw_law(name, path, k):
    """theta ~ Beta(k + a_prior, n - k + b_prior) (gibbs.py:185-198) with k flagged TOAs."""
    pta, kw, st, x = dl.fixture_case(name)
    st.z = dl.flag_first(pta.n, k)
    C, S = dl.THETA_CS
    seed, sweep0, chain0 = SEEDS[(k > 0) ^ (path == "large")]
    out, status, _ = launch(pta, kw, st, x, path, _abi.STAGE_THETA, C, S, seed, sweep0, chain0,
                            keys=("theta",))
    assert np.all((status & STATUS_ERRORS) == 0)
    stats = dl.beta_stats(out["theta"], *dl.theta_shapes(pta, kw, k))
    print(name, path, k, stats)
    observe("theta", f"{name}/{path}/k{k}", stats)
    dl.assert_beta(stats, (name, path, k))


# ---- z ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path", dl.Z_CASES)
def test_z_draw_law(name, path):
    """z_i ~ Bernoulli(q_i) (gibbs.py:201-226), independent over TOAs, chains and sweeps."""
    pta, kw, st, x = dl.z_case(name)
    orc = Oracle(pta, OutlierModel(**kw))
    q = orc.outlier_prob(st, x)
    assert ((q > 0.02) & (q < 0.98)).mean() >= 0.5
    C, S = dl.Z_CS
    seed, sweep0, chain0 = SEEDS[path == "large"]
    out, status, _ = launch(pta, kw, st, x, path, _abi.STAGE_Z, C, S, seed, sweep0, chain0,
                            keys=("z", "pout"))
    assert np.all((status & STATUS_ERRORS) == 0)
    assert np.abs(out["pout"] - q).max() <= 1e-10
    z = out["z"]
    assert np.all((z == 0.0) | (z == 1.0))
    stats = dl.bernoulli_stats(z, np.minimum(q, 1.0))
    print(name, path, stats)
    observe("z", f"{name}/{path}", stats)
    dl.assert_bernoulli(stats, (name, path))


# ---- alpha ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu", dl.ALPHA_NU)
@pytest.mark.parametrize("name,path", dl.ALPHA_CASES)
def test_alpha_draw_law(name, path, nu):
    """alpha_i = rate_i / Gamma((z_i + nu) / 2) (gibbs.py:229-242); nu = 1: shape 1/2 on the
    unflagged TOAs, gamma_mt's a < 1 boost."""
    pta, kw, st, x = dl.fixture_case(name)
    st.nu = nu
    assert 1 <= st.z.sum() < pta.n
    rate, shape = dl.alpha_law(Oracle(pta, OutlierModel(**kw)), st, x)
    C, S = dl.ALPHA_CS
    seed, sweep0, chain0 = SEEDS[(nu > 1) ^ (path == "large")]
    out, status, _ = launch(pta, kw, st, x, path, _abi.STAGE_ALPHA, C, S, seed, sweep0, chain0,
                            keys=("alpha",))
    assert np.all((status & STATUS_ERRORS) == 0)
    stats = dl.pit_stats(dl.alpha_pit(out["alpha"], rate, shape))
    print(name, path, nu, stats)
    observe("alpha", f"{name}/{path}/nu{nu:g}", stats)
    dl.assert_pit(stats, (name, path, nu))


@pytest.mark.parametrize("name,path", dl.ALPHA_CASES)
def test_alpha_unchanged_without_outliers(name, path):
    """gibbs.py:234: with no flagged TOA alpha keeps its values, bitwise."""
    pta, kw, st, x = dl.fixture_case(name)
    st.z = np.zeros(pta.n)
    out, status, _ = launch(pta, kw, st, x, path, _abi.STAGE_ALPHA, 16, 3, 11, keys=("alpha",))
    assert np.all((status & STATUS_ERRORS) == 0)
    np.testing.assert_array_equal(out["alpha"], np.broadcast_to(st.alpha, out["alpha"].shape))


# ---- nu -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("persistent", "large"))
@pytest.mark.parametrize("name", dl.NU_FIXTURES)
def test_nu_draw_law(name, path):
    """nu on the grid 1..30 with Oracle.draw_nu's probabilities (gibbs.py:244-259)."""
    pta, kw, st, x, p = dl.nu_case(name)
    C, S = dl.NU_CS
    assert dl.big_cells(p, C * S) >= 4
    seed, sweep0, chain0 = SEEDS[path == "large"]
    out, status, _ = launch(pta, kw, st, x, path, _abi.STAGE_DF, C, S, seed, sweep0, chain0,
                            keys=("nu",))
    assert np.all((status & STATUS_ERRORS) == 0)
    pval, cells = dl.categorical_chi2(out["nu"], DF_GRID, p)
    print(name, path, pval, cells)
    observe("nu", f"{name}/{path}", {"p_chi2": pval, "cells": cells})
    assert cells >= 4 and pval > dl.P_MIN, (name, path, pval, cells)


# ---- theta, z, alpha, nu in one launch (the fused pass of a full sweep) --------------------------
def combined_toa_stats(pta, kw, st, x, path, C, S):
    """theta, z, alpha and nu in one launch (a full sweep's fused pass over the TOAs): each
    chain-sweep's draws against the laws at its own inputs (theta from the previous z, z from
    the new theta and the previous alpha, alpha from the new z and the previous nu, nu from the
    new alpha), z and alpha pooled over the TOAs, nu through a randomised PIT."""
    from oracle.gibbs_oracle import ChainState
    mask = _abi.STAGE_THETA | _abi.STAGE_Z | _abi.STAGE_ALPHA | _abi.STAGE_DF
    seed, sweep0, chain0 = SEEDS[1]
    keys = ("z", "alpha", "pout", "theta", "nu")
    out, status, _ = launch(pta, kw, st, x, path, mask, C, S, seed, sweep0, chain0, keys=keys)
    assert np.all((status & STATUS_ERRORS) == 0)
    first = {"z": st.z, "alpha": st.alpha, "pout": st.pout, "theta": st.theta, "nu": float(st.nu)}
    h = {k: np.concatenate([np.broadcast_to(first[k], out[k][:, :1].shape), out[k]], axis=1)
         for k in keys}
    orc = Oracle(pta, OutlierModel(**kw))
    u_theta, z_z, u_alpha, u_nu = [], [], [], []
    urng = np.random.default_rng(23)
    for c in range(C):
        for s in range(S):
            zs = h["z"][c, s].sum()
            th = h["theta"][c, s + 1]
            u_theta.append(scipy.stats.beta.cdf(th, *dl.theta_shapes(pta, kw, zs)))
            cur = ChainState(b=st.b, z=h["z"][c, s], alpha=h["alpha"][c, s], pout=st.pout,
                             theta=th, nu=h["nu"][c, s])
            with np.errstate(invalid="ignore", divide="ignore"):   # 0 / 0 -> q = 1 (gibbs.py:224)
                q = orc.outlier_prob(cur, x)
            assert np.abs(h["pout"][c, s + 1] - q).max() <= 1e-10
            z1 = h["z"][c, s + 1]
            z_z.append((z1 - q).sum() / np.sqrt((q * (1 - q)).sum()))
            cur.z = z1
            assert z1.sum() >= 1
            rate, shape = dl.alpha_law(orc, cur, x)
            a1 = h["alpha"][c, s + 1]
            u_alpha.append(dl.alpha_pit(a1, rate, shape))
            cur.alpha = a1
            ll = np.array([orc.df_logdensity(cur, v) for v in DF_GRID])
            p = np.exp(ll - ll.max())
            p /= p.sum()
            k = int(h["nu"][c, s + 1]) - 1
            assert p[k] > 1e-9, (c, s, k, p[k])
            u_nu.append(p[:k].sum() + urng.random() * p[k])      # exactly U(0, 1) under the law
    return {"p_theta": float(dl.ks_uniform(np.array(u_theta))[0]),
            "z_pooled": float(np.abs(z_z).max()),
            "p_alpha": float(dl.ks_uniform(np.concatenate(u_alpha))[0]),
            "p_nu": float(dl.ks_uniform(np.array(u_nu))[0])}


def assert_combined(stats, label):
    print(label, stats)
    observe("toa_fused", label, stats)
    assert min(stats["p_theta"], stats["p_alpha"], stats["p_nu"]) > dl.P_MIN, (label, stats)
    assert stats["z_pooled"] <= dl.Z_MAX, (label, stats)


@pytest.mark.parametrize("path", ("persistent", "large"))
def test_toa_stages_in_one_launch(path):
    """beta_fixed at the z test's state (lg_toa<256>'s fused pass; the persistent kernel)."""
    pta, kw, st, x = dl.z_case("beta_fixed")
    assert_combined(combined_toa_stats(pta, kw, st, x, path, 64, 8), f"beta_fixed/{path}")


def test_toa_stages_on_the_1024_thread_class(plan_bin):
    """lg_toa<1024> (toa class 1): n just above 32768 TOAs, several TOAs per thread."""
    from gibbs_student_t_amd import data
    from gibbs_student_t_amd.model import PTA
    from gibbs_student_t_amd.run_sims import MODELS
    from oracle.gibbs_oracle import ChainState
    n = 32768 + 40
    pta = PTA(data.scaled_synthetic(n=n, components=10, ntm=8, seed=3), components=10)
    kw = dict(MODELS["beta"])
    assert (pta.n, pta.nfourier, pta.ntm) == (n, 20, 8)
    spec = f"{64 * ((n + 63) // 64)},48,20,0,8,16,36,1,0"      # mp 48, ntm_pad 16, raug 36
    mask = _abi.STAGE_THETA | _abi.STAGE_Z | _abi.STAGE_ALPHA | _abi.STAGE_DF
    plan = subprocess.run([plan_bin, "large", "16", str(mask), "0", "0", "1", spec],
                          capture_output=True, text=True, check=True).stdout
    assert "toa<1024>" in plan and "toa<256>" not in plan
    rng = np.random.default_rng(17)
    z0 = (rng.random(n) < 0.1).astype(np.float64)
    st = ChainState(b=np.zeros(pta.m), z=z0, alpha=np.where(z0 > 0, 4.0, 1.0) * (1 + rng.random(n)),
                    pout=np.zeros(n), theta=0.1, nu=4.0)
    x = np.array([0.5 * (p.pmin + p.pmax) for p in pta.params])
    assert_combined(combined_toa_stats(pta, kw, st, x, "large", 16, 4), "scaled_synthetic_32808")


# ---- MH variates --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ("persistent", "large"))
@pytest.mark.parametrize("name", ("beta_fixed", "ecb_beta_fixed"))
def test_mh_variates_match_the_mirror(name, path):
    """The white and hyper Metropolis blocks in Philox mode with (seed, sweep0, chain0) against
    the same launch in tape mode on the tape the numpy mirror writes (oracle/philox_variates.py:
    the counter layout, the index map, the scale uniform, the cosine Box-Muller normal and the
    acceptance uniform): the same parameters move at every sweep, x within 1e-12 of the prior
    range (the host's libm against the device's polynomial cos / log in the normal)."""
    pta, kw, st, x = dl.fixture_case(name)
    orc = Oracle(pta, OutlierModel(**kw))
    C, S = 16, 6
    seed, sweep0, chain0 = SEEDS[1]
    mask = _abi.STAGE_WHITE | _abi.STAGE_HYPER
    got, status, _ = launch(pta, kw, st, x, path, mask, C, S, seed, sweep0, chain0, keys=("x",))
    assert np.all((status & STATUS_ERRORS) == 0)
    probe = NativeSampler(pta, kw, 0, path=path)
    stride = probe.stride
    probe.close()
    tape = np.zeros((C, S, stride))
    tape[:, :, :120] = pv.mh_tape(seed, chain0 + np.arange(C), sweep0 + np.arange(S),
                                  orc.wind, orc.hind)
    want, status, _ = launch(pta, kw, st, x, path, mask, C, S, 0, keys=("x",), tape=tape)
    assert np.all((status & STATUS_ERRORS) == 0)
    gx = np.concatenate([np.broadcast_to(x, (C, 1, len(x))), got["x"]], axis=1)
    wx = np.concatenate([np.broadcast_to(x, (C, 1, len(x))), want["x"]], axis=1)
    moved = np.diff(gx, axis=1) != 0
    assert moved.any(axis=(0, 1)).sum() >= 2          # the test sees moves of several parameters
    np.testing.assert_array_equal(moved, np.diff(wx, axis=1) != 0)
    rng_ = np.array([p.pmax - p.pmin for p in pta.params])
    err = (np.abs(gx - wx) / rng_).max()
    print(name, path, "moves", int(moved.sum()), "max |dx| / range", err)
    observe("mh", f"{name}/{path}", {"moves": int(moved.sum()), "max_dx_over_range": float(err)})
    assert err <= 1e-12, err
