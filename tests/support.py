"""What the test modules share and a CPU can run: numpy and the oracle, no torch.  A test module
imports this (and gpu_support.py for launches), never another test module."""
from __future__ import annotations

import functools
import os
import shutil
import socket
import subprocess

import numpy as np
import pytest
import scipy.linalg as sl

from gibbs_student_t_amd import data
from gibbs_student_t_amd.model import PTA
from gibbs_student_t_amd.native import ACCUM_KEYS
from golden_io import GOLDEN, load_ref, sweep_state
from oracle.gibbs_oracle import (ChainState, Oracle, OutlierModel, b_mean_extended,
                                 lnlike_marginal_extended)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10            # continuous outputs, relative (fp64)
PATHS = ("persistent", "large")
SAME_START_P = 1e-4     # ~60 tests per dataset (time points x series): family-wise ~0.6%
MIXTURE_KW = dict(model="mixture", vary_df=True, theta_prior="beta")

# Philox4x32-10 known answers (Salmon et al. SC'11, Random123 kat_vectors): counter, key, output
KAT = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000",
     "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


cached_ref = functools.lru_cache(maxsize=None)(load_ref)   # shared fixtures: never written to


def rel(a, b):
    """|a - b| / |b| elementwise: 0 where both are the same infinity, inf where they are
    opposite ones."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    inf = np.isinf(a) & np.isinf(b)
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    return np.where(inf, np.where(np.sign(a) == np.sign(b), 0.0, np.inf), d)


def pad(a, width):
    """Per-TOA arrays [..., n] zero-padded to a batch's row stride"""
    out = np.zeros(a.shape[:-1] + (width,))
    out[..., :a.shape[-1]] = a
    return out


def prior_box(pta):
    return (np.array([p.pmin for p in pta.params]), np.array([p.pmax for p in pta.params]))


def chain_state(s):
    """The oracle's ChainState of a golden_io.sweep_state dict (no copies)"""
    return ChainState(b=s["b"], z=s["z"], alpha=s["alpha"], pout=s["pout"], theta=s["theta"],
                      nu=s["nu"])


def states_at(ref, idx):
    """The reference's states at the start of sweeps ``idx``: the stacked per-chain arrays
    and the sweep_state dicts themselves (theta, nu)."""
    ss = [sweep_state(ref, i) for i in idx]
    return {k: np.stack([s[k] for s in ss]) for k in ("b", "z", "alpha", "pout")}, ss


def start_state(ref, C, x="xs", width=None):
    """The fixture's sweep-0 state tiled over C chains, in set_state's order.  ``x``: "xs" (the
    recorded start), "chain0" (``chain[0]``), or a seed for ``np.random.default_rng``, taken as
    given, for a uniform draw over the prior box.  ``width``: the row stride to pad the per-TOA
    arrays to."""
    s0 = sweep_state(ref, 0)
    if isinstance(x, str):
        xv = np.tile(ref["xs"] if x == "xs" else ref["chain"][0], (C, 1))
    else:
        lo, hi = prior_box(ref["pta"])
        xv = np.random.default_rng(x).uniform(lo, hi, size=(C, len(lo)))
    w = (lambda a: a) if width is None else (lambda a: pad(a, width))
    return dict(x=xv, b=np.tile(s0["b"], (C, 1)), z=np.tile(w(s0["z"]), (C, 1)),
                alpha=np.tile(w(s0["alpha"]), (C, 1)), pout=np.tile(w(s0["pout"]), (C, 1)),
                theta=np.full(C, s0["theta"]), nu=np.full(C, s0["nu"]))


def batch_start_state(refs, per, width, x="xs"):
    """start_state of ``per`` chains for each fixture of a batch, padded to the batch's n and
    concatenated; ``x`` as in start_state, or a function of the dataset index giving it."""
    parts = [start_state(r, per, x(d) if callable(x) else x, width) for d, r in enumerate(refs)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def j1713_epochs():
    """J1713+0747's TOAs [s], timing-model design matrix and raw data (gibbs_student_t_amd.data)"""
    raw = data.load_j1713_raw()
    mjd = raw["mjd_int"].astype(np.float64) + raw["mjd_frac"]
    return mjd * data.DAY_SEC, data.design_matrix(mjd, raw["par"], raw["fit"]), raw


def narrowed_prior_model(kind, wA, wg):
    """The hyper-step tests' model with log10_A / gamma priors of half-widths wA / wg around
    the start x0 (and log10_ecorr priors of half-width wA in the general model)."""
    A0, g0 = -14.0, 4.33
    pri = dict(log10_A=(A0 - wA, A0 + wA), gamma=(g0 - wg, g0 + wg))
    if kind == "classic":
        pta = PTA(data.scaled_synthetic(n=100, components=10, ntm=8, seed=3), components=10,
                  **pri)
    else:
        d = np.load(os.path.join(GOLDEN, "ecb_dataset.npz"), allow_pickle=False)
        pta = PTA.from_arrays(str(d["names"][0]).split("_")[0], d["residuals"], d["toaerrs"],
                              d["T"], d["Ffreqs"], int(d["components"]), float(d["tm_weight"]),
                              efac=(0.2, 10.0) if int(d["efac_varied"]) else 1.0,
                              backends=d["backends"], selection=str(d["selection"]),
                              n_ecorr=int(d["n_ecorr"]), ecorr_backend=d["ecorr_backend"],
                              log10_ecorr=(-6.6 - wA, -6.6 + wA), **pri)
    x0 = []
    for p in pta.params:
        nm = p.name
        x0.append(g0 if "gamma" in nm else A0 if "log10_A" in nm else 1.0 if "efac" in nm
                  else -6.6 if "ecorr" in nm else -6.8)
    return pta, np.array(x0)


# ---- the long-double arbiter ---------------------------------------------------------------------
def assert_lnl_within_reference_error(pta, st, x, got, want, label):
    """A marginal likelihood that misses the reference's fp64 value by more than RTOL
    (ill-conditioned Sigma: that value is itself inexact): the GPU error against the
    long-double value must be within twice the reference's own, or within 1e-10 of the
    magnitude of the cancelling terms (log|N|, r^T N^-1 r, d^T Sigma^-1 d, log|Sigma|,
    log|phi|)."""
    ext, scale = lnlike_marginal_extended(pta, st, x, with_scale=True)
    assert abs(got - ext) <= max(2 * abs(want - ext), RTOL * scale), \
        f"{label}: gpu {got!r} ref {want!r} extended {ext!r} scale {scale:.3e}"


def assert_b_within_reference_error(pta, st, x, b_gpu, mean_chol, delta, label):
    """cond(Sigma) so large that fp64 Cholesky means (LAPACK's and ours) both carry ~cond*eps
    error: the long-double mean arbitrates, allowing twice the reference's own error."""
    mext = b_mean_extended(pta, st, x)
    e_gpu = np.linalg.norm(b_gpu - (mext + delta))
    e_ref = np.linalg.norm(mean_chol - mext)
    assert e_gpu <= 2 * e_ref + 1e-12 * np.linalg.norm(mext), \
        f"{label}, vs extended {e_gpu:.3e} > 2 x ref {e_ref:.3e}"


def assert_floor_draw_within_reference_error(b_gpu, t, i, Sigma, d, f):
    """A b draw at the SVD noise floor against the reference's OWN b (``b_ref``, its SVD draw
    u (u^T d / s) + U S^-1/2 xi, gibbs.py:166-180) on the same sweep: the GPU b must be no
    further from it than the exact draw (cho_solve(Sigma, d) + the same draw term) is, or the
    shift f I must lie within the reference's own SVD error -- the perturbation
    ||U S U^T - Sigma||_2 that LAPACK's SVD itself makes of Sigma on this sweep (long-double
    reconstruction of the recomputed SVD, which must be bitwise the fixture's)."""
    b_ref = t["b_ref"][i]
    e_gpu = np.linalg.norm(b_gpu - b_ref)
    e_exact = np.linalg.norm(t["b_mean_chol"][i] + t["b_delta"][i] - b_ref)
    if e_gpu <= e_exact:
        return
    u, sv, _ = sl.svd(Sigma)
    np.testing.assert_array_equal(u @ ((u.T @ d) / sv), t["b_mean_svd"][i])
    ld = np.longdouble
    E = (u.astype(ld) * sv.astype(ld)) @ u.T.astype(ld) - Sigma.astype(ld)
    e_svd = np.linalg.norm(E.astype(np.float64), 2)
    assert f <= e_svd, (f"sweep {i}: floor b {e_gpu:.3e} from the reference's b (exact draw "
                        f"{e_exact:.3e}) and f {f:.3e} > the SVD's own error {e_svd:.3e}")


def assert_replay_matches(got, want, ref, label=""):
    """Discrete records exact; b normwise per sweep, alpha / pout elementwise <= RTOL.

    Where the two fp64 Cholesky means (LAPACK's in the oracle, the kernel's) differ by more
    than RTOL -- cond(Sigma) ~ 1e8 leaves both ~1e-10 from the exact mean -- the long-double
    mean arbitrates, as in test_mh_blocks_and_b_draw: the GPU b must then be at least as
    close to it as the oracle's (within twice its error)."""
    n = want["z"].shape[-1]
    for k in ("x", "z", "nu", "theta"):
        g = got[k][..., :n] if k == "z" else got[k]
        np.testing.assert_array_equal(g, want[k], err_msg=f"{label} {k}")
    eb = np.linalg.norm(got["b"] - want["b"], axis=1) / np.maximum(
        np.linalg.norm(want["b"], axis=1), 1e-300)
    delta = ref["tape"]["b_delta"]
    orc = Oracle(ref["pta"], OutlierModel(**ref["kw"]))
    for k in np.flatnonzero(eb > RTOL):
        assert k >= 1, f"{label} b differs at the start state"
        # b recorded at sweep k was drawn in sweep k-1 at that sweep's (z, alpha) and x_k
        st = ChainState(b=want["b"][k - 1], z=want["z"][k - 1], alpha=want["alpha"][k - 1],
                        pout=want["pout"][k - 1], theta=float(want["theta"][k - 1]),
                        nu=float(want["nu"][k - 1]))
        orc.cache = None
        f = orc.floor_shift(orc.sigma_matrix(st, want["x"][k])[0])   # the draw's floor shift
        exact = b_mean_extended(ref["pta"], st, want["x"][k], shift=f) + delta[k - 1]
        e_gpu = np.linalg.norm(got["b"][k] - exact)
        e_orc = np.linalg.norm(want["b"][k] - exact)
        assert e_gpu <= 2 * e_orc + 1e-13 * np.linalg.norm(exact), \
            f"{label} b sweep {k}: rel {eb[k]:.3e}, |gpu - exact| {e_gpu:.3e} > " \
            f"2 |oracle - exact| {e_orc:.3e}"
    for k in ("alpha", "pout"):
        r = rel(got[k][..., :n], want[k])
        assert np.all(r <= RTOL), f"{label} {k}: max rel {r.max():.3e}"


def check_accum_sums(rec, sums, n_of, burn, keys=ACCUM_KEYS,
                     per_toa=("z_sum", "pout_sum", "alpha_sum"), sentinel=-7.25):
    """Posterior sums against a sequential host sum of the records from record ``burn`` on;
    per-TOA entries t >= n of a chain must keep the sentinel they were allocated with."""
    nrec = rec["b"].shape[1] if "b" in rec else rec["pout"].shape[1]
    for key, rk in (("z_sum", "z"), ("pout_sum", "pout"), ("alpha_sum", "alpha"),
                    ("b_sum", "b")):
        if key not in keys:
            continue
        want = np.zeros_like(rec[rk][:, 0])
        for i in range(burn, nrec):        # sequential, as the kernel adds (np.sum is pairwise)
            want = want + rec[rk][:, i]
        if key in per_toa:
            for c, n in enumerate(n_of):
                np.testing.assert_array_equal(sums[key][c, :n], want[c, :n], err_msg=f"{key} {c}")
                assert np.all(sums[key][c, n:] == sentinel), f"{key}: chain {c} wrote t >= n"
        else:
            np.testing.assert_array_equal(sums[key], want, err_msg=key)
    if "b_sq" in keys:
        want = np.zeros_like(rec["b"][:, 0])
        for i in range(burn, nrec):
            want = want + rec["b"][:, i] * rec["b"][:, i]
        # non-negative terms, fused or unfused multiply-add: one rounding per term
        np.testing.assert_allclose(sums["b_sq"], want, rtol=1e-14, atol=0.0)
    if "count" in keys:
        np.testing.assert_array_equal(sums["count"], nrec - burn)


# ---- the host packer's small dataset (tools/pack_dump.cpp) -----------------------------------------
PACK_DIMS = (70, 4, 3, 18, 2, 8)         # N, NF, NTM, NEC, NB, P
# (MT, ntm_pad, raug): the large path (mp = 48) and the GEN shape (8, 2, 62) (mp = 64)
PACKINGS = {"large": (0, 16, 38), "gen": (8, 16, 62)}


def pack_dataset(variant):
    """classes: <= 8 (sigma, backend) classes; sigmas: 9 distinct sigmas; overlap: one TOA in
    two epochs"""
    N, NF, NTM, NEC, NB, P = PACK_DIMS
    rng = np.random.default_rng(11)
    T = np.zeros((N, NF + NTM + NEC))
    T[:, :NF + NTM] = rng.standard_normal((N, NF + NTM))
    # 18 epochs of 1..5 TOAs (51 TOAs), scattered; the other 19 TOAs are in no epoch
    sizes = [1 + e % 5 for e in range(NEC)]
    toas = rng.permutation(N)[:sum(sizes)]
    start = np.concatenate([[0], np.cumsum(sizes)])
    for e in range(NEC):
        T[toas[start[e]:start[e + 1]], NF + NTM + e] = 0.5 + rng.random(sizes[e])
    if variant == "overlap":
        T[toas[0], NF + NTM + 7] = 0.25      # epoch 0's TOA also in epoch 7
    backend = rng.integers(0, NB, N).astype(np.int32)
    nsig = 9 if variant == "sigmas" else 3
    toaerrs = (1e-7 * (1 + np.arange(nsig)))[rng.integers(0, nsig, N)]
    if variant == "sigmas":
        toaerrs[:9] = 1e-7 * (1 + np.arange(9))
    return dict(T=T, residuals=1e-6 * rng.standard_normal(N), toaerrs=toaerrs,
                ffreqs=np.repeat(np.array([1.0, 2.0]) / 3e8, 2), pmin=-np.arange(1.0, P + 1),
                pmax=np.arange(2.0, P + 2) / 3, df_A=rng.random(30), df_B=rng.random(30),
                backend=backend, ecorr_backend=rng.integers(0, NB, NEC).astype(np.int32),
                ecorr_idx=np.array([4, 5], np.int32), efac_idx=np.array([0, 1], np.int32),
                equad_idx=np.array([2, 3], np.int32), hyper_idx=np.array([4, 5, 6, 7], np.int32),
                white_idx=np.array([0, 1, 2, 3], np.int32))


def run_packer(pack_bin, tmp_path, d, MT, ntm_pad, raug, disjoint, procs=None):
    """pack_dump on the descriptor file of ``d`` (with the gst_model_procs arrays ``procs`` =
    (nproc, ncol, idx_log10_A, idx_gamma) appended, if given): its named output arrays."""
    N, NF, NTM, NEC, NB, P = PACK_DIMS
    head = np.array([N, NF + NTM + NEC, NF, NTM, NEC, NB, P, 4, 4, ntm_pad, raug, MT, disjoint,
                     6, 7, 0 if procs is None else procs[0]], np.int32)
    src, dst = tmp_path / "desc.bin", tmp_path / "packed.bin"
    with open(src, "wb") as f:
        f.write(head.tobytes())
        for k in ("T", "residuals", "toaerrs", "ffreqs", "pmin", "pmax", "df_A", "df_B"):
            f.write(np.ascontiguousarray(d[k], np.float64).tobytes())
        for k in ("backend", "ecorr_backend", "ecorr_idx", "efac_idx", "equad_idx", "hyper_idx",
                  "white_idx"):
            f.write(np.ascontiguousarray(d[k], np.int32).tobytes())
        if procs is not None:
            f.write(np.array(procs[1] + procs[2] + procs[3], np.int32).tobytes())
    subprocess.run([pack_bin, str(src), str(dst)], check=True)
    out, raw, pos = {}, dst.read_bytes(), 0
    while pos < len(raw):
        end = raw.index(b"\n", pos)
        name, dtype, count = raw[pos:end].decode().split()
        size = int(count) * int(dtype[1])
        out[name] = np.frombuffer(raw[end + 1:end + 1 + size], dtype="<" + dtype)
        pos = end + 1 + size
    return out


# ---- processes and host programs ----------------------------------------------------------------
def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_TOOLS = {}


def host_tool(tmp_path_factory, name, flags=("-O1",), required=False):
    """``tools/<name>.cpp`` built with g++ once per session; returns the program's path.
    Without g++ a CPU test skips; a GPU test that needs the planner passes ``required``."""
    key = (name,) + tuple(flags)
    if key not in _TOOLS:
        if shutil.which("g++") is None:
            assert not required, f"this check needs g++ (tools/{name}.cpp)"
            pytest.skip("no g++")
        out = tmp_path_factory.mktemp(name) / name
        subprocess.run(["g++", *flags, "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I",
                        os.path.join(ROOT, "gibbs_student_t_amd", "csrc"),
                        os.path.join(ROOT, "tools", f"{name}.cpp"), "-o", str(out)], check=True)
        _TOOLS[key] = str(out)
    return _TOOLS[key]
