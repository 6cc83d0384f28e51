"""What the tests of the block second moment of b (gst_set_accum_block, post.PosteriorSums
b_outer) share and a CPU can run: the packing, the long-double references and the derived
tolerances.  Sits on golden_io.py; gpu_block_support.py adds the launches on gpu_support.py."""
from __future__ import annotations

import os

import numpy as np

from gibbs_student_t_amd.model import PTA, PulsarData
from golden_io import GOLDEN

EPS = 2.0 ** -52
LD = np.longdouble


def tri_index(K):
    """(i, j) of every packed element e = i (i + 1) / 2 + j, i >= j, in order"""
    i, j = np.tril_indices(K)
    assert np.array_equal(i * (i + 1) // 2 + j, np.arange(K * (K + 1) // 2))
    return i, j


def packed_outer_sums(b, block, first=0):
    """Sequential fp64 sums, as the kernels add them, of b_i b_j over the records first.. of
    ``b`` [C, N, m] for the packed lower triangle of ``block`` = (col0, ncol): [C, K (K + 1) / 2]"""
    col0, K = block
    i, j = tri_index(K)
    out = np.zeros((b.shape[0], len(i)))
    for s in range(first, b.shape[1]):
        v = b[:, s, col0:col0 + K]
        out = out + v[:, i] * v[:, j]
    return out


def packed_outer_reference(b, block, first=0):
    """(want, bound) of the block sums of the records first.. of ``b`` [C, N, m]: the
    long-double sum of b_i b_j and (N + 2) 2^-52 sum_s |b_si b_sj| -- N additions and one
    product rounding per term, fused or not -- per packed element"""
    col0, K = block
    i, j = tri_index(K)
    v = b[:, first:, col0:col0 + K].astype(LD)
    prod = v[:, :, i] * v[:, :, j]
    N = prod.shape[1]
    return prod.sum(axis=1), (N + 2) * EPS * np.abs(prod).sum(axis=1)


def waveform_reference(B, bs):
    """Mean, population variance and the derived tolerance of the variance of ``B @ b`` over the
    samples ``bs`` [N, K] in long double.  Tolerance of row t:
    (N + K + 4) 2^-52 sum_ij |B_ti B_tj| (sum_s |b_si b_sj| / N + |mu_i mu_j|): the rounding
    of N additions per element of the second moment plus a K-term quadratic form."""
    B, bs = np.asarray(B).astype(LD), np.asarray(bs).astype(LD)
    N, K = bs.shape
    w = bs @ B.T                                   # [N, T]
    mean = w.sum(axis=0) / N
    var = ((w - mean) ** 2).sum(axis=0) / N       # np.cov(..., bias=True)'s diagonal
    mu = bs.sum(axis=0) / N
    S = np.abs(bs[:, :, None] * bs[:, None, :]).sum(axis=0) / N + np.abs(mu[:, None] * mu[None, :])
    aB = np.abs(B)
    tol = (N + K + 4) * EPS * np.einsum("ti,ij,tj->t", aB, S, aB)
    return mean, var, tol


def assert_waveform(got_mean, got_sd, B, bs, label=""):
    """``PosteriorSums.waveform``'s (mean, sd) against waveform_reference: the variance within
    its tolerance, the mean within the same rounding of a K-term dot product of N-term sums"""
    mean, var, tol = waveform_reference(B, bs)
    N, K = np.asarray(bs).shape
    aB, amu = np.abs(np.asarray(B)).astype(LD), np.abs(np.asarray(bs)).astype(LD).sum(axis=0) / N
    tol_mean = (N + K + 4) * EPS * (aB @ amu)
    got_mean, got_var = np.asarray(got_mean).astype(LD), np.asarray(got_sd).astype(LD) ** 2
    em, ev = np.abs(got_mean - mean), np.abs(got_var - var)
    print(f"{label}: mean err / tol {float(np.max(em / tol_mean)):.3g}, "
          f"var err / tol {float(np.max(ev / tol)):.3g}")
    assert np.all(em <= tol_mean), f"{label} mean: worst {float(np.max(em / tol_mean)):.3g} x tol"
    assert np.all(ev <= tol), \
        f"{label} variance: worst {float(np.max(ev / tol)):.3g} x tol"


def mgp_model(ds="dmg", **gps):
    """The multi-process dataset ``ds`` of tests/golden rebuilt from its pulsar arrays (epochs,
    radio frequencies, design matrix) instead of from its stored basis, so that the model knows
    its epochs and span: (pta, the stored dataset)."""
    d = np.load(os.path.join(GOLDEN, f"mgp_{ds}_dataset.npz"), allow_pickle=False)
    comps = dict(zip((str(v) for v in d["proc_names"]), (int(v) for v in d["proc_components"])))
    psr = PulsarData(name=str(d["names"][0]).split("_")[0], toas=d["toas"],
                     residuals=d["residuals"], toaerrs=d["toaerrs"], Mmat=d["Mmat"],
                     freqs=d["freqs"])
    kw = {k: dict(components=comps[k]) for k in ("dm_gp", "chrom_gp") if k in comps}
    kw.update(gps)
    return PTA(psr, components=int(d["components"]), tm_weight=float(d["tm_weight"]), **kw), d
