"""Posterior sums kept on the device (include/gst.h gst_accum) and what a run ends in.

The reference workflow ends in a few averages of the chains: the outlier flags
``np.flatnonzero(zchain.mean(axis=0) > 0.9)``, the means of ``poutchain`` and ``alphachain``
and the signal ``T @ bchain`` (gibbs_likelihood.ipynb).  ``PosteriorSums`` holds the sums
those averages need -- per chain, so that chains, successive ``Gibbs.sample`` calls and
ranks merge by addition -- without any per-TOA chain array.

Two of the notebook's products are no mean (include/gst.h gst_accum_toa): its outlier rule
``np.median(poutchain, axis=0) > tau``, which the per-TOA counts of the sweeps with
``pout_t > tau`` decide exactly, and the band of the signal ``np.dot(Tmat, bchain[ind, :])``
at every TOA, which the sums of ``y = r - T b`` and ``y^2`` give (r is constant:
``E[T b] = r - E[y]``, ``Var[T b] = Var[y]``).

All arrays are host numpy arrays with a leading chain axis: ``count`` [C] (int64),
``z_sum`` / ``pout_sum`` / ``alpha_sum`` [C, n], ``b_sum`` / ``b_sq`` [C, m],
``resid_sum`` / ``resid_sq`` [C, n]; ``pout_gt`` is [K, C, n], one plane per threshold of
``pout_thr`` [K]; a sum that was not kept is ``None``.

The spread of one process's waveform ``T_p b_p`` needs the covariance of b inside the process
(include/gst.h gst_accum_block): ``b_outer`` [C, K (K + 1) / 2] is the packed lower triangle
of the sum of ``b b^T`` over the columns ``b_block = (col0, K)`` of b, element (i, j), i >= j,
at ``i (i + 1) / 2 + j``.  With ``b_sum`` and ``count`` it gives ``b_cov`` and, for any design
matrix B over the block's columns, mean and standard deviation of ``B @ b`` (``waveform``,
``process_waveform``).
"""
from __future__ import annotations

import numpy as np

SUM_KEYS = ("z_sum", "pout_sum", "alpha_sum", "b_sum", "b_sq")
# the sums of gst_accum_toa: after SUM_KEYS wherever the sums are listed in order, so that
# a PosteriorSums without them looks (pooled vector, files) as it always did
TOA_KEYS = ("pout_gt", "resid_sum", "resid_sq")
# the sum of gst_accum_block: after every other key, for the same reason
BLOCK_KEYS = ("b_outer",)
ALL_KEYS = SUM_KEYS + TOA_KEYS + BLOCK_KEYS


class PosteriorSums:
    def __init__(self, count, z_sum=None, pout_sum=None, alpha_sum=None, b_sum=None, b_sq=None,
                 pout_thr=None, pout_gt=None, resid_sum=None, resid_sq=None, b_outer=None,
                 b_block=None):
        self.count = np.atleast_1d(np.asarray(count, dtype=np.int64))
        C = self.count.shape[0]
        for key, v in zip(SUM_KEYS + TOA_KEYS[1:] + BLOCK_KEYS,
                          (z_sum, pout_sum, alpha_sum, b_sum, b_sq, resid_sum, resid_sq, b_outer)):
            if v is not None:
                v = np.asarray(v, dtype=np.float64)
                if v.ndim != 2 or v.shape[0] != C:
                    raise ValueError(f"{key}: need [C = {C}, ...], got {v.shape}")
            setattr(self, key, v)
        if (pout_gt is None) != (pout_thr is None):
            raise ValueError("pout_gt and pout_thr go together")
        if pout_gt is not None:
            pout_thr = np.atleast_1d(np.asarray(pout_thr, dtype=np.float64))
            pout_gt = np.asarray(pout_gt, dtype=np.float64)
            if pout_gt.ndim != 3 or pout_gt.shape[:2] != (pout_thr.shape[0], C):
                raise ValueError(f"pout_gt: need [K = {pout_thr.shape[0]}, C = {C}, n], "
                                 f"got {pout_gt.shape}")
        self.pout_thr, self.pout_gt = pout_thr, pout_gt
        if (b_outer is None) != (b_block is None):
            raise ValueError("b_outer and b_block go together")
        if b_block is not None:
            b_block = tuple(int(v) for v in np.asarray(b_block).reshape(-1))
            if len(b_block) != 2 or b_block[0] < 0 or b_block[1] < 1:
                raise ValueError(f"b_block: need (col0, ncol), got {b_block}")
            K = b_block[1]
            if self.b_outer.shape[1] != K * (K + 1) // 2:
                raise ValueError(f"b_outer: need [C = {C}, {K * (K + 1) // 2}] for a block of "
                                 f"{K} columns, got {self.b_outer.shape}")
        self.b_block = b_block

    @classmethod
    def from_device(cls, acc: dict, pout_thresholds=None, b_block=None):
        """From ``NativeSampler.alloc_accum`` tensors (synchronises the device);
        ``pout_thresholds``: the thresholds of ``acc["pout_gt"]``'s planes; ``b_block``: the
        ``(col0, ncol)`` of ``acc["b_outer"]``."""
        host = {k: v.detach().cpu().numpy() for k, v in acc.items()}
        if "count" not in host:
            raise ValueError("the accumulators need 'count'")
        if "pout_gt" in host:
            host["pout_thr"] = pout_thresholds
        if "b_outer" in host:
            host["b_block"] = b_block
        return cls(**host)

    @property
    def nchains(self):
        return self.count.shape[0]

    # ---- means ---------------------------------------------------------------------
    def _get(self, key):
        v = getattr(self, key)
        if v is None:
            raise ValueError(f"{key} was not accumulated")
        return v

    def _mean(self, key, pool):
        s = self._get(key)
        if pool:
            return s.sum(axis=0) / self.count.sum()
        return s / self.count[:, None]

    def z_mean(self, pool=True):
        """Outlier probability of each TOA, mean of z_t: [n], or [C, n] per chain."""
        return self._mean("z_sum", pool)

    def pout_mean(self, pool=True):
        return self._mean("pout_sum", pool)

    def alpha_mean(self, pool=True):
        return self._mean("alpha_sum", pool)

    def b_mean(self, pool=True):
        return self._mean("b_sum", pool)

    def b_var(self, pool=True):
        """Variance of each b_j over the counted sweeps (population form, E b^2 - (E b)^2;
        pooled: over all chains' sweeps together)."""
        m = self._mean("b_sum", pool)
        return np.maximum(self._mean("b_sq", pool) - m * m, 0.0)

    def z_mean_se(self):
        """Monte-Carlo standard error of the pooled z_mean from the spread of the chains:
        standard deviation of the per-chain means / sqrt(C) (needs C >= 2)."""
        if self.nchains < 2:
            raise ValueError("z_mean_se needs at least two chains")
        return self.z_mean(pool=False).std(axis=0, ddof=1) / np.sqrt(self.nchains)

    def outliers(self, threshold=0.9, rule="mean"):
        """Indices of the outlier TOAs.  ``rule="mean"``: mean z above ``threshold``, the
        notebook's ``np.flatnonzero(zchain.mean(axis=0) > 0.9)``.  ``rule="median"``: its
        ``np.flatnonzero(np.median(poutchain, axis=0) > threshold)`` over all chains' sweeps,
        from the exceedance counts (``threshold`` must be one of ``pout_thr``); a TOA that the
        counts cannot decide (``pout_median_gt``) is an error, never a guess."""
        if rule == "mean":
            return np.flatnonzero(self.z_mean() > threshold)
        if rule != "median":
            raise ValueError("rule must be 'mean' or 'median'")
        gt, amb = self.pout_median_gt(threshold)
        if amb.any():
            raise ValueError(f"median rule undecided at TOAs {np.flatnonzero(amb).tolist()}: "
                             "exactly half of an even number of sweeps exceed the threshold "
                             "(see pout_median_gt)")
        return np.flatnonzero(gt)

    def signal_mean(self, T):
        """Posterior mean of the signal T b (the mean of ``T @ bchain`` over the sweeps)."""
        return np.asarray(T, dtype=np.float64) @ self.b_mean()

    # ---- exceedance counts: the median rule ------------------------------------------
    def _plane(self, thr):
        gt = self._get("pout_gt")
        k = np.flatnonzero(self.pout_thr == float(thr))
        if k.size == 0:
            raise ValueError(f"threshold {thr!r} was not kept; kept: {self.pout_thr.tolist()}")
        return gt[k[0]]

    def pout_exceed_frac(self, thr, pool=True):
        """Fraction of the counted sweeps with ``pout_t > thr`` (strict): [n], or [C, n] per
        chain.  ``thr`` must be one of the kept thresholds ``pout_thr``."""
        g = self._plane(thr)
        if pool:
            return g.sum(axis=0) / self.count.sum()
        return g / self.count[:, None]

    def pout_median_gt(self, thr):
        """``(decision, ambiguous)``, two boolean [n] arrays: whether the median of pout_t
        over all chains' counted sweeps exceeds ``thr``, exactly as
        ``np.median(poutchain, axis=0) > thr`` decides it.  With N sweeps and k of them above
        ``thr`` the median is above for 2 k > N and not above for 2 k < N; for 2 k == N (even
        N) the median is the mean of a value above and a value not above ``thr``, which
        counts cannot place: those TOAs are marked ``ambiguous`` (their decision is False)."""
        k = np.rint(self._plane(thr).sum(axis=0)).astype(np.int64)
        N = int(self.count.sum())
        return 2 * k > N, 2 * k == N

    # ---- residual sums: the signal at every TOA --------------------------------------
    def signal_mean_toa(self, r):
        """Posterior mean of the signal T b at every TOA, ``r - E[y]`` with ``r`` the
        residuals the model was built from: the centre of the notebook's waveform figure."""
        return np.asarray(r, dtype=np.float64) - self._mean("resid_sum", True)

    def signal_sd(self, pool=True):
        """Standard deviation of the signal T b at every TOA over the counted sweeps
        (population form; Var[T b] = Var[y] = E y^2 - (E y)^2): [n], or [C, n] per chain."""
        m = self._mean("resid_sum", pool)
        return np.sqrt(np.maximum(self._mean("resid_sq", pool) - m * m, 0.0))

    # ---- block second moment: covariance of b, waveforms with bands -------------------
    def _block_moments(self, pool):
        """(mu [.., K], M [.., K, K]) of the block: mean of b and of b b^T over the counted
        sweeps, pooled over all chains' sweeps or per chain (leading axis C)."""
        bo = self._get("b_outer")
        col0, K = self.b_block
        bs = self._get("b_sum")[:, col0:col0 + K]
        if pool:
            N = self.count.sum()
            tri, mu = bo.sum(axis=0) / N, bs.sum(axis=0) / N
        else:
            tri, mu = bo / self.count[:, None], bs / self.count[:, None]
        i, j = np.tril_indices(K)      # row-major lower triangle: e = i (i + 1) / 2 + j
        M = np.zeros(tri.shape[:-1] + (K, K))
        M[..., i, j] = tri
        M[..., j, i] = tri
        return mu, M

    def b_cov(self, pool=True):
        """Covariance of the block's coefficients over the counted sweeps (population form,
        E b b^T - E b E b^T): [K, K] pooled over all chains' sweeps, or [C, K, K] per chain."""
        mu, M = self._block_moments(pool)
        return M - mu[..., :, None] * mu[..., None, :]

    def waveform(self, B, cols=None, pool=True):
        """``(mean, sd)`` of ``B @ b[cols]`` over the counted sweeps: ``B`` [T, k] is a design
        matrix over the block's columns ``cols`` (a slice relative to the block's first
        column; default: the whole block); sd = sqrt(max(diag(B Cov B^T), 0)), population
        form.  [T] each, or [C, T] per chain."""
        B = np.asarray(B, dtype=np.float64)
        mu, M = self._block_moments(pool)
        cov = M - mu[..., :, None] * mu[..., None, :]
        if cols is not None:
            if not isinstance(cols, slice) or cols.step not in (None, 1):
                raise ValueError("cols: a contiguous slice inside the block")
            mu, cov = mu[..., cols], cov[..., cols, cols]
        if B.ndim != 2 or B.shape[1] != mu.shape[-1]:
            raise ValueError(f"B: need [T, {mu.shape[-1]}], got {B.shape}")
        mean = mu @ B.T
        var = np.einsum("ti,...ij,tj->...t", B, cov, B)
        return mean, np.sqrt(np.maximum(var, 0.0))

    def process_waveform(self, pta, name, toas=None, freqs=None, units="s", pool=True):
        """``(mean, sd)`` of the waveform of the process ``name`` ("red", "dm_gp", "chrom_gp")
        of ``pta`` (model.PTA) at the epochs ``toas`` and radio frequencies ``freqs`` (default:
        the model's own), from ``PTA.process_basis``; the block must cover the process.
        ``units="s"``: the delay in seconds as it enters the residuals; ``units="dm"``: the
        process without its (1400 / nu)^chi weight times 2.41e-4 * 1400^2, i.e. DM in
        pc cm^-3 for ``dm_gp`` (see ``PTA.process_basis`` on parity)."""
        if units not in ("s", "dm"):
            raise ValueError('units must be "s" or "dm"')
        self._get("b_outer")
        lo, hi = pta.process_columns(name)
        col0, K = self.b_block
        if lo < col0 or hi > col0 + K:
            raise ValueError(f"process {name!r} owns columns [{lo}, {hi}), the block kept "
                             f"[{col0}, {col0 + K})")
        B = pta.process_basis(name, toas=toas, freqs=freqs, scaled=units == "s")
        if units == "dm":
            from .model import DM_K
            B = B * (DM_K * 1400.0 ** 2)
        return self.waveform(B, cols=slice(lo - col0, hi - col0), pool=pool)

    # ---- merging -------------------------------------------------------------------
    def _same_kept(self, other):
        if self.b_block != other.b_block:
            raise ValueError(f"b blocks differ: {self.b_block} and {other.b_block}")
        for key in ALL_KEYS:
            if (getattr(self, key) is None) != (getattr(other, key) is None):
                raise ValueError(f"{key} is kept by one operand only")
        if self.pout_gt is not None and not np.array_equal(self.pout_thr, other.pout_thr):
            raise ValueError(f"pout thresholds differ: {self.pout_thr.tolist()} and "
                             f"{other.pout_thr.tolist()}")

    def __add__(self, other):
        """Sums of the same chains over more sweeps (successive ``sample`` calls)."""
        if not isinstance(other, PosteriorSums):
            return NotImplemented
        if other.count.shape != self.count.shape:
            raise ValueError(f"chain counts differ: {self.nchains} and {other.nchains}; "
                             "use concat() for other chains")
        self._same_kept(other)
        kw = {key: None if getattr(self, key) is None else getattr(self, key) + getattr(other, key)
              for key in ALL_KEYS}
        return PosteriorSums(self.count + other.count, pout_thr=self.pout_thr,
                             b_block=self.b_block, **kw)

    def concat(self, other):
        """Sums of other chains of the same model (another rank's shard) appended."""
        self._same_kept(other)
        kw = {}
        for key in ALL_KEYS:
            a, b = getattr(self, key), getattr(other, key)
            kw[key] = None if a is None else np.concatenate([a, b], axis=a.ndim - 2)
        return PosteriorSums(np.concatenate([self.count, other.count]), pout_thr=self.pout_thr,
                             b_block=self.b_block, **kw)

    def select(self, chains, n=None):
        """The sums of the chains ``chains`` (indices or a slice), per-TOA arrays cut to their
        first ``n`` entries (a batch's dataset with fewer TOAs than the batch's stride)."""
        kw = {}
        for key in ALL_KEYS:
            v = getattr(self, key)
            if v is not None:
                v = v[..., chains, :]
                if n is not None and key not in ("b_sum", "b_sq", "b_outer"):
                    v = v[..., :n]
            kw[key] = v
        return PosteriorSums(self.count[chains], pout_thr=self.pout_thr, b_block=self.b_block,
                             **kw)

    # ---- pooled form (what ranks exchange) -------------------------------------------
    def pooled(self):
        """The sums over this object's chains as one pseudo-chain ``PosteriorSums`` (C = 1):
        every pooled mean is unchanged, and pooled sums of several ranks merge with ``+``."""
        kw = {}
        for k in ALL_KEYS:
            v = getattr(self, k)
            kw[k] = None if v is None else v.sum(axis=v.ndim - 2, keepdims=True)
        return PosteriorSums([self.count.sum()], pout_thr=self.pout_thr, b_block=self.b_block,
                             **kw)

    def pooled_vector(self):
        """``pooled()`` as one flat float64 vector [total count | the kept sums in SUM_KEYS
        order | pout_gt plane by plane, resid_sum, resid_sq, b_outer where kept]: what
        ``dist.reduce_summary`` adds over the ranks (counts stay exact below 2^53)."""
        p = self.pooled()
        parts = [p.count.astype(np.float64)]
        parts += [getattr(p, k)[0] for k in SUM_KEYS if getattr(p, k) is not None]
        if p.pout_gt is not None:
            parts.append(p.pout_gt.reshape(-1))
        parts += [getattr(p, k)[0] for k in TOA_KEYS[1:] + BLOCK_KEYS
                  if getattr(p, k) is not None]
        return np.concatenate(parts)

    def from_pooled_vector(self, vec):
        """A reduced ``pooled_vector()`` back as a C = 1 ``PosteriorSums`` with this object's
        kept sums, thresholds, block and sizes."""
        vec = np.asarray(vec, dtype=np.float64)
        kw, o = {}, 1
        for k in ALL_KEYS:
            v = getattr(self, k)
            if v is None:
                continue
            w = v.shape[-1]
            if k == "pout_gt":
                K = v.shape[0]
                kw[k] = vec[o:o + K * w].reshape(K, 1, w)
                o += K * w
            else:
                kw[k] = vec[None, o:o + w]
                o += w
        if o != vec.shape[0]:
            raise ValueError(f"vector of {vec.shape[0]} entries, expected {o}")
        return PosteriorSums([int(round(vec[0]))], pout_thr=self.pout_thr,
                             b_block=self.b_block, **kw)

    # ---- files ---------------------------------------------------------------------
    def save(self, path):
        """A plain .npz (no pickles) of the arrays that were kept."""
        arrays = {k: getattr(self, k) for k in SUM_KEYS + TOA_KEYS
                  if getattr(self, k) is not None}
        if self.pout_gt is not None:
            arrays["pout_thr"] = self.pout_thr
        if self.b_outer is not None:
            arrays["b_outer"] = self.b_outer
            arrays["b_block"] = np.asarray(self.b_block, dtype=np.int64)
        np.savez(path, count=self.count, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as f:
            return cls(**{k: f[k] for k in f.files})
