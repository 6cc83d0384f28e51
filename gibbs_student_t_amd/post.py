"""Posterior sums kept on the device (include/gst.h gst_accum) and what a run ends in.

The reference workflow ends in a few averages of the chains: the outlier flags
``np.flatnonzero(zchain.mean(axis=0) > 0.9)``, the means of ``poutchain`` and ``alphachain``
and the signal ``T @ bchain`` (gibbs_likelihood.ipynb).  ``PosteriorSums`` holds the sums
those averages need -- per chain, so that chains, successive ``Gibbs.sample`` calls and
ranks merge by addition -- without any per-TOA chain array.

All arrays are host numpy arrays with a leading chain axis: ``count`` [C] (int64),
``z_sum`` / ``pout_sum`` / ``alpha_sum`` [C, n], ``b_sum`` / ``b_sq`` [C, m]; a sum that
was not kept is ``None``.
"""
from __future__ import annotations

import numpy as np

SUM_KEYS = ("z_sum", "pout_sum", "alpha_sum", "b_sum", "b_sq")


class PosteriorSums:
    def __init__(self, count, z_sum=None, pout_sum=None, alpha_sum=None, b_sum=None, b_sq=None):
        self.count = np.atleast_1d(np.asarray(count, dtype=np.int64))
        C = self.count.shape[0]
        for key, v in zip(SUM_KEYS, (z_sum, pout_sum, alpha_sum, b_sum, b_sq)):
            if v is not None:
                v = np.asarray(v, dtype=np.float64)
                if v.ndim != 2 or v.shape[0] != C:
                    raise ValueError(f"{key}: need [C = {C}, ...], got {v.shape}")
            setattr(self, key, v)

    @classmethod
    def from_device(cls, acc: dict):
        """From ``NativeSampler.alloc_accum`` tensors (synchronises the device)."""
        host = {k: v.detach().cpu().numpy() for k, v in acc.items()}
        if "count" not in host:
            raise ValueError("the accumulators need 'count'")
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

    def outliers(self, threshold=0.9):
        """Indices of the TOAs with mean z above ``threshold``: the notebook's
        ``np.flatnonzero(zchain.mean(axis=0) > 0.9)``."""
        return np.flatnonzero(self.z_mean() > threshold)

    def signal_mean(self, T):
        """Posterior mean of the signal T b (the mean of ``T @ bchain`` over the sweeps)."""
        return np.asarray(T, dtype=np.float64) @ self.b_mean()

    # ---- merging -------------------------------------------------------------------
    def __add__(self, other):
        """Sums of the same chains over more sweeps (successive ``sample`` calls)."""
        if not isinstance(other, PosteriorSums):
            return NotImplemented
        if other.count.shape != self.count.shape:
            raise ValueError(f"chain counts differ: {self.nchains} and {other.nchains}; "
                             "use concat() for other chains")
        kw = {}
        for key in SUM_KEYS:
            a, b = getattr(self, key), getattr(other, key)
            if (a is None) != (b is None):
                raise ValueError(f"{key} is kept by one operand only")
            kw[key] = None if a is None else a + b
        return PosteriorSums(self.count + other.count, **kw)

    def concat(self, other):
        """Sums of other chains of the same model (another rank's shard) appended."""
        kw = {}
        for key in SUM_KEYS:
            a, b = getattr(self, key), getattr(other, key)
            if (a is None) != (b is None):
                raise ValueError(f"{key} is kept by one operand only")
            kw[key] = None if a is None else np.concatenate([a, b])
        return PosteriorSums(np.concatenate([self.count, other.count]), **kw)

    # ---- pooled form (what ranks exchange) -------------------------------------------
    def pooled(self):
        """The sums over this object's chains as one pseudo-chain ``PosteriorSums`` (C = 1):
        every pooled mean is unchanged, and pooled sums of several ranks merge with ``+``."""
        kw = {k: None if getattr(self, k) is None else getattr(self, k).sum(axis=0, keepdims=True)
              for k in SUM_KEYS}
        return PosteriorSums([self.count.sum()], **kw)

    def pooled_vector(self):
        """``pooled()`` as one flat float64 vector [total count | the kept sums in SUM_KEYS
        order]: what ``dist.reduce_summary`` adds over the ranks (counts stay exact below
        2^53)."""
        p = self.pooled()
        parts = [p.count.astype(np.float64)]
        parts += [getattr(p, k)[0] for k in SUM_KEYS if getattr(p, k) is not None]
        return np.concatenate(parts)

    def from_pooled_vector(self, vec):
        """A reduced ``pooled_vector()`` back as a C = 1 ``PosteriorSums`` with this object's
        kept sums and sizes."""
        vec = np.asarray(vec, dtype=np.float64)
        kw, o = {}, 1
        for k in SUM_KEYS:
            if getattr(self, k) is not None:
                w = getattr(self, k).shape[1]
                kw[k] = vec[None, o:o + w]
                o += w
        if o != vec.shape[0]:
            raise ValueError(f"vector of {vec.shape[0]} entries, expected {o}")
        return PosteriorSums([int(round(vec[0]))], **kw)

    # ---- files ---------------------------------------------------------------------
    def save(self, path):
        """A plain .npz (no pickles) of the arrays that were kept."""
        arrays = {k: getattr(self, k) for k in SUM_KEYS if getattr(self, k) is not None}
        np.savez(path, count=self.count, **arrays)

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as f:
            return cls(**{k: f[k] for k in f.files})
