"""The hyper MH's likelihood statistics as chol_stats_diag (csrc/gst_chol.hpp) forms them, emulated
in numpy fp64 and held against a long-double elimination of the same system.

The kernel eliminates the augmented system [[Sigma, d], [d^T, r^T N^-1 r]] right-looking on raw
columns (a_ij -= (a_ik / a_kk) a_jk; the a_kk are the pivots), timing-model columns first.  From
the Fourier block's elimination it takes
  * log|Sigma| as a product of the pivots' mantissas and a sum of their exponents, each residue
    class k % 8 multiplied on its own (one diagonal lane each), then the eight classes combined;
  * d^T Sigma^-1 d from the augmented row's own diagonal element (the "corner"): its value before
    the Fourier block's elimination minus its value after it, since every step subtracts
    a_{R,k}^2 / a_kk from it.
The form it replaces gathered every pivot and augmented-row entry and summed a_{R,k}^2 / a_kk
(the "summed form").  Both are emulated here; the corner form's lnL must be within twice the summed
form's own error against the long-double value, or within 1e-12 of the magnitude of the
cancelling terms (two decimal orders inside the suite's RTOL yardstick; the emulation reaches
4e-14 of it at worst).
"""
import warnings

import numpy as np
import pytest

from gibbs_student_t_amd.run_sims import MODELS
from golden_io import load_dataset
from oracle.gibbs_oracle import (ChainState, Oracle, OutlierModel, lnlike_marginal_extended)
from support import MIXTURE_KW, cached_ref, prior_box, states_at

C = 64
BOUND = 1e-12


def _mant_exp(values):
    """prod(values) as (mantissa product, exponent sum), multiplied in the order given"""
    mm, ee = 1.0, 0
    for a in values:
        m, e = np.frexp(a)
        mm *= m
        ee += int(e)
    return mm, ee


def _emulate(orc, st, x):
    """(lnL corner form, lnL summed form) of the fp64 raw-column elimination, or None where a
    pivot is not positive."""
    orc.cache = None
    pm = orc._pmap(x)
    N = orc.noise(st, x)
    Sigma, d = orc.sigma_matrix(st, x)
    logdet_phi = orc.pta.get_phiinv(pm, logdet=True)[0][1]
    order = orc.internal_order()
    m = len(order)
    ntm = int(orc.pta.U.shape[1])
    rNr = np.sum(orc.r ** 2 / N)
    A = np.empty((m + 1, m + 1))
    A[:m, :m] = Sigma[np.ix_(order, order)]
    A[m, :m] = A[:m, m] = d[order]
    A[m, m] = rNr
    piv, z = np.empty(m), np.empty(m)
    corner_tm = None
    for k in range(m):
        if k == ntm:
            corner_tm = A[m, m]          # S0's corner: what the Fourier block starts from
        piv[k] = A[k, k]
        if not piv[k] > 0.0:
            return None
        z[k] = A[m, k]
        col = A[k + 1:, k].copy()
        A[k + 1:, k + 1:] -= np.outer(col * (1.0 / piv[k]), col)
    # the timing-model columns: the gathered form in both (chol_stats, once per sweep)
    quad_tm = np.sum(z[:ntm] ** 2 / piv[:ntm])
    mt, et = _mant_exp(piv[:ntm])
    # Fourier block, summed form: pivots in column order
    ms, es = _mant_exp(piv[ntm:])
    quad_sum = np.sum(z[ntm:] ** 2 / piv[ntm:])
    # Fourier block, diagonal lanes: a class k % 8 at a time, then across the classes
    md, ed = 1.0, 0
    for q in range(8):
        mq, eq = _mant_exp(piv[ntm:][q::8])
        md *= mq
        ed += eq
    quad_corner = corner_tm - A[m, m]
    logdetN = np.sum(np.log(N))

    def lnl(mant, expo, quad):
        ld_sigma = np.log(mt * mant) + (et + expo) * np.log(2.0)
        return -0.5 * (logdetN + rNr) + 0.5 * ((quad_tm + quad) - ld_sigma - logdet_phi)
    return lnl(md, ed, quad_corner), lnl(ms, es, quad_sum)


def _reference_points():
    """The 64 points of tests/test_gpu_hyper_stats.py::test_eval_lnlike_j1713"""
    ref = cached_ref("beta_fixed")
    st, ss = states_at(ref, np.arange(C) // 11)
    x = ref["tape"]["hyper_lnl_x"].reshape(-1, len(ref["xs"]))[:C]
    return ref["pta"], ref["kw"], [
        (ChainState(b=st["b"][c], z=st["z"][c], alpha=st["alpha"][c], pout=st["pout"][c],
                    theta=ss[c]["theta"], nu=ss[c]["nu"]), x[c]) for c in range(C)]


def _prior_box_states():
    """Hyper parameters anywhere in their prior box, a tenth of the TOAs flagged at alpha 5"""
    ref = cached_ref("beta_fixed")
    pta = ref["pta"]
    orc = Oracle(pta, OutlierModel(**MIXTURE_KW))
    rng = np.random.default_rng(41)
    lo, hi = prior_box(pta)
    hyp = np.zeros(len(lo), bool)
    hyp[orc.hind] = True
    x = np.where(hyp[None], rng.uniform(lo, hi, size=(C, len(lo))), ref["xs"][None])
    z = (rng.uniform(size=(C, pta.n)) < 0.1).astype(np.float64)
    return pta, MIXTURE_KW, [
        (ChainState(b=np.zeros(pta.m), z=z[c], alpha=np.where(z[c] > 0, 5.0, 1.0),
                    pout=np.zeros(pta.n), theta=0.05, nu=4.0), x[c]) for c in range(C)]


def _vvh17_starts():
    """The all-outlier start of the vvh17 model: z = 1, alpha = 1e10, x over the prior box"""
    pta = load_dataset()
    lo, hi = prior_box(pta)
    x = np.random.default_rng(3).uniform(lo, hi, size=(C, len(lo)))
    return pta, MODELS["vvh17"], [
        (ChainState(b=np.zeros(pta.m), z=np.ones(pta.n), alpha=np.full(pta.n, 1e10),
                    pout=np.zeros(pta.n), theta=0.01, nu=4.0), x[c]) for c in range(C)]


@pytest.mark.parametrize("case", ["reference_points", "prior_box", "vvh17_start"])
def test_corner_form_within_reference_error(case):
    pta, kw, states = {"reference_points": _reference_points, "prior_box": _prior_box_states,
                       "vvh17_start": _vvh17_starts}[case]()
    orc = Oracle(pta, OutlierModel(**kw))
    worst = (0.0, 0.0, 0.0)
    for c, (st, x) in enumerate(states):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = _emulate(orc, st, x)
            ext, scale = lnlike_marginal_extended(pta, st, x, with_scale=True)
        assert got is not None and np.isfinite(ext), (case, c)
        corner, summed = got
        e_corner, e_sum = abs(corner - ext), abs(summed - ext)
        worst = max(worst, (e_corner / scale, e_corner, e_sum))
        assert e_corner <= max(2 * e_sum, BOUND * scale), \
            f"{case}[{c}]: corner {corner!r} summed {summed!r} extended {ext!r} scale {scale:.3e}"
    print(f"{case}: worst corner-form error {worst[1]:.3e} = {worst[0]:.2e} of the scale "
          f"(summed form there {worst[2]:.3e})")
