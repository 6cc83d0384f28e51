"""Device-side chain state and launches over the C ABI (libgst.so).

PyTorch-ROCm owns every chain buffer (``torch.empty(..., device='cuda')``); the library
receives raw ``data_ptr()`` values and the current HIP stream.  Nothing here computes a
sweep on the CPU: a missing library or device raises.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _abi
from .model import df_tables, hyper_white_indices

MODEL_CODES = {"gaussian": _abi.GST_MODEL_GAUSSIAN, "t": _abi.GST_MODEL_T,
               "mixture": _abi.GST_MODEL_MIXTURE, "vvh17": _abi.GST_MODEL_VVH17}
STATE_KEYS = ("x", "b", "z", "alpha", "pout", "theta", "nu")
# gst_accum's buffers, in the struct's order
ACCUM_KEYS = ("z_sum", "pout_sum", "alpha_sum", "b_sum", "b_sq", "count")
# gst_accum_toa's buffers, in the struct's order (allocated on request)
ACCUM_TOA_KEYS = ("pout_gt", "resid_sum", "resid_sq")
# gst_accum_block's buffer (allocated on request, with b_block=(col0, ncol))
ACCUM_BLOCK_KEY = "b_outer"


def check_block(b_block, m):
    """``(col0, ncol)`` as two ints: col0 >= 0, 1 <= ncol <= GST_BLOCK_MAX, col0 + ncol <= m."""
    try:
        col0, ncol = (int(v) for v in b_block)
    except (TypeError, ValueError):
        raise ValueError(f"b_block: need (col0, ncol), got {b_block!r}") from None
    if col0 < 0 or ncol < 1 or col0 + ncol > m:
        raise ValueError(f"b_block {(col0, ncol)}: columns must lie in [0, {m})")
    if ncol > _abi.BLOCK_MAX:
        raise ValueError(f"b_block {(col0, ncol)}: at most GST_BLOCK_MAX = {_abi.BLOCK_MAX} "
                         "columns")
    return col0, ncol


def _check_thresholds(thr):
    """pout thresholds as a tuple of floats: at most 4, strictly increasing, each in (0, 1)."""
    thr = () if thr is None else tuple(float(v) for v in np.atleast_1d(thr))
    if len(thr) > 4 or any(not 0.0 < v < 1.0 for v in thr) or \
            any(b <= a for a, b in zip(thr, thr[1:])):
        raise ValueError("pout_thresholds: at most 4 strictly increasing values in (0, 1)")
    return thr


def _torch():
    import torch
    return torch


def model_desc(pta, cfg: dict):
    """Build the gst_model_desc for a ``model.PTA`` and Gibbs kwargs (gibbs.py:9-11).

    Returns ``(desc, keepalive)``; keep ``keepalive`` referenced while ``desc`` is used.
    ``keepalive["procs"]`` is the ``gst_model_procs`` of the model's Fourier block (``pta.procs``:
    red | dm | chrom; one process for a pta without the attribute), which ``gst_model_set_procs``
    takes beside the descriptors when there is more than one.
    """
    names = [p.name for p in pta.params]
    P = len(names)
    hind, wind = hyper_white_indices(names)
    procs = list(getattr(pta, "procs", ()))

    def role(suffix):
        # the red noise's pair by exact name: dm_gp_log10_A sorts before log10_A
        if procs and suffix in ("log10_A", "gamma"):
            return procs[0].idx_log10_A if suffix == "log10_A" else procs[0].idx_gamma
        for i, nm in enumerate(names):
            if nm.endswith("_" + suffix):
                return i
        return -1

    r = np.ascontiguousarray(pta.get_residuals()[0], dtype=np.float64)
    T = np.ascontiguousarray(pta.get_basis()[0], dtype=np.float64)
    n, m = T.shape
    A, B = df_tables(n)
    keep = {
        "T": T, "r": r,
        "err": np.ascontiguousarray(pta._toaerrs, dtype=np.float64),
        "ff": np.ascontiguousarray(pta.Ffreqs, dtype=np.float64),
        "pmin": np.array([p.pmin for p in pta.params], dtype=np.float64),
        "pmax": np.array([p.pmax for p in pta.params], dtype=np.float64),
        "hind": np.ascontiguousarray(hind, dtype=np.int32),
        "wind": np.ascontiguousarray(wind, dtype=np.int32),
        "A": np.ascontiguousarray(A, dtype=np.float64),
        "B": np.ascontiguousarray(B, dtype=np.float64),
    }
    # general white noise (ABI 3): per-backend parameters and ECORR basis columns
    nb = int(getattr(pta, "nbackend", 1))
    n_ec = int(getattr(pta, "n_ecorr", 0))
    if nb > 1 or n_ec:
        keep.update(
            bk=np.ascontiguousarray(pta.bidx, dtype=np.int32),
            efi=np.ascontiguousarray(pta.backend_param_indices("efac"), dtype=np.int32),
            eqi=np.ascontiguousarray(pta.backend_param_indices("log10_equad"), dtype=np.int32),
            eci=np.ascontiguousarray(pta.backend_param_indices("log10_ecorr"), dtype=np.int32),
            ecb=np.ascontiguousarray(pta.ecorr_backend, dtype=np.int32))
    dp = lambda a: a.ctypes.data_as(_abi._D)  # noqa: E731
    ip = lambda a: a.ctypes.data_as(_abi._I)  # noqa: E731
    model = cfg.get("model", "gaussian")
    if model not in MODEL_CODES:
        raise ValueError(f"unknown model {model!r}")
    if model == "vvh17" and cfg.get("pspin") is None:
        raise ValueError("model='vvh17' needs pspin")
    desc = _abi.ModelDesc(
        n=n, m=m, nfourier=pta.nfourier, ntm=pta.ntm, nparams=P,
        T=dp(keep["T"]), residuals=dp(keep["r"]), toaerrs=dp(keep["err"]),
        ffreqs=dp(keep["ff"]), tm_weight=float(pta.tm_weight),
        idx_efac=role("efac"), idx_equad=role("log10_equad"), idx_log10_A=role("log10_A"),
        idx_gamma=role("gamma"),
        efac_const=float(pta.efac_const if pta.efac_const is not None else 1.0),
        pmin=dp(keep["pmin"]), pmax=dp(keep["pmax"]),
        hyper_idx=ip(keep["hind"]), n_hyper=len(hind),
        white_idx=ip(keep["wind"]), n_white=len(wind),
        model=MODEL_CODES[model], vary_df=int(bool(cfg.get("vary_df", True))),
        vary_alpha=int(bool(cfg.get("vary_alpha", True))),
        theta_prior_beta=int(cfg.get("theta_prior", "beta") == "beta"),
        mprior=float(cfg.get("m", 0.01)),
        pspin=float(cfg.get("pspin") or 0.0),
        df_A=dp(keep["A"]), df_B=dp(keep["B"]),
    )
    if nb > 1 or n_ec:
        desc.nbackend = nb
        desc.backend = ip(keep["bk"])
        desc.efac_idx = ip(keep["efi"])
        desc.equad_idx = ip(keep["eqi"])
        desc.ecorr_idx = ip(keep["eci"])
        desc.n_ecorr = n_ec
        desc.ecorr_backend = ip(keep["ecb"]) if n_ec else None
    if len(procs) > _abi.NPROC_MAX:
        raise ValueError(f"at most {_abi.NPROC_MAX} power-law processes")
    pr = _abi.ModelProcs(nproc=max(len(procs), 1))
    pr.ncol[0], pr.idx_log10_A[0], pr.idx_gamma[0] = pta.nfourier, desc.idx_log10_A, desc.idx_gamma
    for j, q in enumerate(procs):
        pr.ncol[j], pr.idx_log10_A[j], pr.idx_gamma[j] = q.ncol, q.idx_log10_A, q.idx_gamma
    keep["procs"] = pr
    return desc, keep


class NativeSampler:
    """One HIP context + model + a batch of C chains resident on one GPU.

    ``pta``/``cfg`` may be lists: a batch of datasets (e.g. the run_sims.py grid of
    simulated pulsars x outlier models) sharing the basis shape and parameter set; each
    chain then names its dataset through ``alloc(C, dataset=...)``.  Per-TOA state and
    record arrays are laid out with row stride ``self.n`` = the largest n of the batch.
    """

    def __init__(self, pta, cfg: dict, device: int = 0, path: str = "auto"):
        torch = _torch()
        self.lib = _abi.load()
        if not torch.cuda.is_available():
            raise _abi.GstNativeError("no HIP device visible: the sampler runs only on GPU")
        self.device = int(device)
        self.tdev = torch.device("cuda", self.device)
        ptas = list(pta) if isinstance(pta, (list, tuple)) else [pta]
        cfgs = list(cfg) if isinstance(cfg, (list, tuple)) else [cfg] * len(ptas)
        if len(cfgs) != len(ptas):
            raise ValueError("one cfg per dataset (or a single shared cfg)")
        ctx = ct.c_void_p()
        _abi.check(self.lib, self.lib.gst_ctx_create(self.device, ct.byref(ctx)),
                   "gst_ctx_create")
        self.ctx = ctx
        if path not in _abi.PATHS:
            raise ValueError(f"path must be one of {sorted(_abi.PATHS)}")
        _abi.check(self.lib, self.lib.gst_set_path(self.ctx, _abi.PATHS[path]), "gst_set_path")
        self.ptas, self.cfgs = ptas, [dict(c) for c in cfgs]
        self.pta, self.cfg = ptas[0], self.cfgs[0]
        descs, self._keep = [], []
        for p_, c_ in zip(ptas, cfgs):
            d, k = model_desc(p_, c_)
            descs.append(d)
            self._keep.append(k)
        arr = (_abi.ModelDesc * len(descs))(*descs)
        # several power-law processes (DM, chromatic): one layout shared by the batch
        layouts = [tuple(bytes(k["procs"])) for k in self._keep]
        if any(v != layouts[0] for v in layouts):
            raise ValueError("the datasets of a batch must share the power-law processes")
        self.procs = self._keep[0]["procs"]
        if self.procs.nproc > 1:
            if not hasattr(self.lib, "gst_model_set_procs"):
                raise _abi.GstNativeError("this libgst.so lacks gst_model_set_procs; rebuild")
            _abi.check(self.lib, self.lib.gst_model_set_procs(self.ctx, arr, ct.byref(self.procs),
                                                              len(descs)), "gst_model_set_procs")
        else:
            _abi.check(self.lib, self.lib.gst_model_set_batch(self.ctx, arr, len(descs)),
                       "gst_model_set_batch")
        nd, nmax, stride = ct.c_int(), ct.c_int(), ct.c_int()
        _abi.check(self.lib, self.lib.gst_model_info(self.ctx, ct.byref(nd), ct.byref(nmax),
                                                     ct.byref(stride)), "gst_model_info")
        self.ndatasets = nd.value
        pth = ct.c_int()
        _abi.check(self.lib, self.lib.gst_get_path(self.ctx, ct.byref(pth)), "gst_get_path")
        self.path = {v: k for k, v in _abi.PATHS.items()}[pth.value]
        self.n_of = [int(p_.T.shape[0]) for p_ in ptas]
        self.n, self.m = nmax.value, int(ptas[0].T.shape[1])
        self.P = len(ptas[0].params)
        self.stride = stride.value
        self.C = 0
        self.state = None
        self.dataset = None
        self._accum = None
        self._accum_toa = None
        self._accum_block = None

    def set_waves(self, waves="auto"):
        """Waves per chain of the persistent path's sampling launches (gst_set_waves):
        "auto" (two when C <= 2 x CUs), 1 or 2.  The draws are bitwise the same."""
        code = {"auto": 0, 1: 1, 2: 2}[waves]
        _abi.check(self.lib, self.lib.gst_set_waves(self.ctx, code), "gst_set_waves")

    def set_debug(self, poison: bool = False, large_gram: bool = False,
                  large_hyper: bool = False, exact_bdraw: bool = False,
                  mfma_gram: bool = False, epochs_lds: bool = False):
        """gst_set_debug: GST_DEBUG_POISON overwrites every chain's LDS and parked scratch
        with NaN at each sweep start (a check that no sweep reads stale state);
        GST_DEBUG_LARGE_GRAM / _HYPER force the large path's generic Gram / hyper kernels
        (tests compare them with the mid-size kernels); GST_DEBUG_EXACT_BDRAW draws b from
        Sigma exactly also beyond fp64 resolution (no SVD noise floor, include/gst.h);
        GST_DEBUG_MFMA_GRAM keeps the persistent kernel's Gram on the MFMA path (no low-rank
        Gram); GST_DEBUG_EPOCHS_LDS runs ECORR-epochs-first chains on the 256-thread lg_hyper<2>
        instead of the one-wave lg_hyper_ecr."""
        flags = ((_abi.DEBUG_POISON if poison else 0) | (_abi.DEBUG_LARGE_GRAM if large_gram else 0)
                 | (_abi.DEBUG_LARGE_HYPER if large_hyper else 0)
                 | (_abi.DEBUG_EXACT_BDRAW if exact_bdraw else 0)
                 | (_abi.DEBUG_MFMA_GRAM if mfma_gram else 0)
                 | (_abi.DEBUG_EPOCHS_LDS if epochs_lds else 0))
        _abi.check(self.lib, self.lib.gst_set_debug(self.ctx, flags), "gst_set_debug")

    # ---- state ---------------------------------------------------------------------
    def alloc(self, C: int, dataset=None):
        """Allocate C chains; ``dataset[c]`` is chain c's dataset index (default all 0)."""
        torch = _torch()
        f64 = dict(dtype=torch.float64, device=self.tdev)
        self.C = int(C)
        ds = np.zeros(C, dtype=np.int32) if dataset is None else \
            np.asarray(dataset, dtype=np.int32).reshape(C)
        if ds.size and (ds.min() < 0 or ds.max() >= self.ndatasets):
            raise ValueError(f"dataset indices must lie in [0, {self.ndatasets})")
        if dataset is None and self.ndatasets > 1:
            raise ValueError("several datasets: pass dataset= to alloc")
        if self.path == "large" and self.ndatasets > 1:
            # the large path stages one dataset's T per 16-chain group (Gram, T b)
            groups = [ds[i:i + 16] for i in range(0, C, 16)]
            if any(np.any(grp != grp[0]) for grp in groups):
                raise ValueError("large path with several datasets: every aligned group of "
                                 "16 chains must share one dataset")
        self.dataset_host = ds
        self.dataset = torch.as_tensor(ds).to(self.tdev)
        self.state = {
            "x": torch.zeros((C, self.P), **f64), "b": torch.zeros((C, self.m), **f64),
            "z": torch.zeros((C, self.n), **f64), "alpha": torch.ones((C, self.n), **f64),
            "pout": torch.zeros((C, self.n), **f64), "theta": torch.zeros(C, **f64),
            "nu": torch.zeros(C, **f64),
            "status": torch.zeros(C, dtype=torch.int32, device=self.tdev),
        }
        return self.state

    def set_state(self, **arrays):
        torch = _torch()
        for k, v in arrays.items():
            if v is None:
                continue
            t = self.state[k]
            src = torch.from_numpy(np.array(v, dtype=np.float64)).reshape(t.shape)
            t.copy_(src.to(self.tdev))

    def get_state(self):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.state.items()}

    def _state_struct(self):
        s = self.state
        return _abi.State(*(ct.c_void_p(s[k].data_ptr()) for k in STATE_KEYS),
                          ct.c_void_p(s["status"].data_ptr()),
                          ct.c_void_p(self.dataset.data_ptr()))

    def alloc_records(self, nrec: int, keys=STATE_KEYS):
        torch = _torch()
        f64 = dict(dtype=torch.float64, device=self.tdev)
        shapes = {"x": (self.P,), "b": (self.m,), "z": (self.n,), "alpha": (self.n,),
                  "pout": (self.n,), "theta": (), "nu": ()}
        return {k: torch.empty((self.C, nrec) + shapes[k], **f64) for k in keys}

    # ---- posterior sums (gst_set_accum, gst_set_accum_toa) ---------------------------
    def _accum_shapes(self, nthr=None, b_block=None):
        sh = {"z_sum": (self.C, self.n), "pout_sum": (self.C, self.n),
              "alpha_sum": (self.C, self.n), "b_sum": (self.C, self.m),
              "b_sq": (self.C, self.m), "count": (self.C,),
              "resid_sum": (self.C, self.n), "resid_sq": (self.C, self.n)}
        if nthr:
            sh["pout_gt"] = (int(nthr), self.C, self.n)
        if b_block is not None:
            K = check_block(b_block, self.m)[1]
            sh[ACCUM_BLOCK_KEY] = (self.C, K * (K + 1) // 2)
        return sh

    def alloc_accum(self, keys=ACCUM_KEYS, pout_thresholds=None, b_block=None):
        """Zeroed device tensors for the posterior sums: ``z_sum`` / ``pout_sum`` /
        ``alpha_sum`` [C, n], ``b_sum`` / ``b_sq`` [C, m] (float64) and ``count`` [C]
        (int64); on request ``pout_gt`` [K, C, n] (K = len(pout_thresholds)) and
        ``resid_sum`` / ``resid_sq`` [C, n], and with ``b_block=(col0, ncol)`` the key
        ``b_outer`` [C, ncol (ncol + 1) / 2]: the packed lower triangle of sum b b^T over
        the columns [col0, col0 + ncol) of b.  Pass the dict (or a subset of it) to
        ``set_accum``."""
        torch = _torch()
        thr = _check_thresholds(pout_thresholds)
        shapes = self._accum_shapes(len(thr), b_block)
        unknown = [k for k in keys if k not in shapes]
        if unknown:
            if unknown == ["pout_gt"]:
                raise ValueError("pout_gt needs pout_thresholds")
            if unknown == [ACCUM_BLOCK_KEY]:
                raise ValueError("b_outer needs b_block=(col0, ncol)")
            raise ValueError(f"unknown accumulator(s) {unknown}; choose from "
                             f"{ACCUM_KEYS + ACCUM_TOA_KEYS + (ACCUM_BLOCK_KEY,)}")
        return {k: torch.zeros(shapes[k], device=self.tdev,
                               dtype=torch.int64 if k == "count" else torch.float64)
                for k in keys}

    def _check_accum(self, acc, thr, b_block=None):
        torch = _torch()
        shapes = self._accum_shapes(len(thr), b_block)
        for k, t in acc.items():
            want = torch.int64 if k == "count" else torch.float64
            if k not in shapes or t.dtype != want or not t.is_contiguous() \
                    or t.device != self.tdev or tuple(t.shape) != shapes[k]:
                raise ValueError(f"accumulator {k!r}: need a contiguous {want} tensor of shape "
                                 f"{shapes.get(k)} on {self.tdev} (alloc_accum)")

    def set_accum_toa(self, acc, pout_thresholds=None):
        """gst_set_accum_toa alone: the ``pout_gt`` / ``resid_sum`` / ``resid_sq`` tensors of
        ``acc`` (None or none of them: off).  They are added to only while ``set_accum`` is
        set, from its ``from_sweep`` on."""
        thr = _check_thresholds(pout_thresholds)
        toa = {k: acc[k] for k in ACCUM_TOA_KEYS if acc and k in acc}
        if not hasattr(self.lib, "gst_set_accum_toa"):
            if toa:
                raise _abi.GstNativeError("this libgst.so lacks gst_set_accum_toa; rebuild")
            return
        if "pout_gt" in toa and not thr:
            raise ValueError("pout_gt needs pout_thresholds")
        self._check_accum(toa, thr)
        if not toa:
            _abi.check(self.lib, self.lib.gst_set_accum_toa(self.ctx, None), "gst_set_accum_toa")
            self._accum_toa = None
            return
        ptr = lambda k: ct.c_void_p(toa[k].data_ptr()) if k in toa else None  # noqa: E731
        K = len(thr) if "pout_gt" in toa else 0
        a = _abi.AccumToa(K, (ct.c_double * 4)(*thr[:K]), *(ptr(k) for k in ACCUM_TOA_KEYS))
        _abi.check(self.lib, self.lib.gst_set_accum_toa(self.ctx, ct.byref(a)),
                   "gst_set_accum_toa")
        self._accum_toa = toa

    def set_accum_block(self, acc, b_block=None):
        """gst_set_accum_block alone: the ``b_outer`` tensor of ``acc`` over the columns
        ``b_block = (col0, ncol)`` (None or no such key: off).  It is added to only while
        ``set_accum`` is set, from its ``from_sweep`` on."""
        bo = acc.get(ACCUM_BLOCK_KEY) if acc else None
        if not hasattr(self.lib, "gst_set_accum_block"):
            if bo is not None:
                raise _abi.GstNativeError("this libgst.so lacks gst_set_accum_block; rebuild")
            return
        if bo is None:
            _abi.check(self.lib, self.lib.gst_set_accum_block(self.ctx, None),
                       "gst_set_accum_block")
            self._accum_block = None
            return
        if b_block is None:
            raise ValueError("b_outer needs b_block=(col0, ncol)")
        col0, ncol = check_block(b_block, self.m)
        self._check_accum({ACCUM_BLOCK_KEY: bo}, (), (col0, ncol))
        a = _abi.AccumBlock(col0, ncol, ct.c_void_p(bo.data_ptr()))
        _abi.check(self.lib, self.lib.gst_set_accum_block(self.ctx, ct.byref(a)),
                   "gst_set_accum_block")
        self._accum_block = bo

    def set_accum(self, acc: dict, from_sweep: int = 0, pout_thresholds=None, b_block=None):
        """Every later ``sweep`` adds the state at the start of each of its sweeps with global
        index ``sweep0 + i >= from_sweep`` into ``acc`` (tensors from ``alloc_accum``; missing
        keys are skipped), whatever ``record_every`` is, until ``clear_accum``.  With
        ``pout_gt`` in ``acc``, plane k counts the sweeps with ``pout > pout_thresholds[k]``
        (up to 4 strictly increasing values in (0, 1)); with ``b_outer`` in ``acc``,
        ``b_block = (col0, ncol)`` names its columns.  The sampler keeps ``acc`` referenced
        while it is set."""
        thr = _check_thresholds(pout_thresholds)
        if ACCUM_BLOCK_KEY in acc and b_block is None:
            raise ValueError("b_outer needs b_block=(col0, ncol)")
        self._check_accum(acc, thr, b_block if ACCUM_BLOCK_KEY in acc else None)
        self.set_accum_toa(acc, thr)
        self.set_accum_block(acc, b_block)
        ptr = lambda k: ct.c_void_p(acc[k].data_ptr()) if k in acc else None  # noqa: E731
        a = _abi.Accum(*(ptr(k) for k in ACCUM_KEYS), int(from_sweep))
        _abi.check(self.lib, self.lib.gst_set_accum(self.ctx, ct.byref(a)), "gst_set_accum")
        self._accum = acc

    def clear_accum(self):
        """Stop accumulating (launches already queued on the stream still add)."""
        _abi.check(self.lib, self.lib.gst_set_accum(self.ctx, None), "gst_set_accum")
        if hasattr(self.lib, "gst_set_accum_toa"):
            _abi.check(self.lib, self.lib.gst_set_accum_toa(self.ctx, None), "gst_set_accum_toa")
        if hasattr(self.lib, "gst_set_accum_block"):
            _abi.check(self.lib, self.lib.gst_set_accum_block(self.ctx, None),
                       "gst_set_accum_block")
        self._accum = None
        self._accum_toa = None
        self._accum_block = None

    # ---- launches ------------------------------------------------------------------
    def stream_ptr(self):
        torch = _torch()
        return ct.c_void_p(torch.cuda.current_stream(self.tdev).cuda_stream)

    def sweep(self, nsweeps: int, *, records=None, record_every: int = 1,
              mask: int = _abi.STAGE_ALL, seed: int = 0, sweep0: int = 0, chain0: int = 0,
              tape=None):
        """Launch ``nsweeps`` sweeps of all C chains.  ``records`` is a dict from
        ``alloc_records`` (or None); ``tape`` a device float64 tensor [C, nsweeps, stride]."""
        st = self._state_struct()
        rec = None
        if records is not None:
            nrec = next(iter(records.values())).shape[1]
            ptr = lambda k: ct.c_void_p(records[k].data_ptr()) if k in records else None  # noqa
            rec = _abi.Records(*(ptr(k) for k in STATE_KEYS), nrec)
        tp = None
        if tape is not None:
            if tuple(tape.shape) != (self.C, nsweeps, self.stride):
                raise ValueError(f"tape shape {tuple(tape.shape)} != "
                                 f"{(self.C, nsweeps, self.stride)}")
            tp = _abi.Tape(ct.c_void_p(tape.data_ptr()), self.stride)
        rc = self.lib.gst_sweep(self.ctx, ct.byref(st), ct.byref(rec) if rec else None,
                                ct.byref(tp) if tp else None, self.C, int(nsweeps),
                                int(sweep0), int(record_every if rec else 0), int(mask),
                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain0), self.stream_ptr())
        _abi.check(self.lib, rc, "gst_sweep")

    def eval_lnlike(self):
        torch = _torch()
        ow = torch.empty(self.C, dtype=torch.float64, device=self.tdev)
        oh = torch.empty(self.C, dtype=torch.float64, device=self.tdev)
        st = self._state_struct()
        rc = self.lib.gst_eval_lnlike(self.ctx, ct.byref(st), self.C,
                                      ct.c_void_p(ow.data_ptr()), ct.c_void_p(oh.data_ptr()),
                                      self.stream_ptr())
        _abi.check(self.lib, rc, "gst_eval_lnlike")
        return ow.cpu().numpy(), oh.cpu().numpy()

    def synchronize(self):
        _abi.check(self.lib, self.lib.gst_sync(self.ctx, self.stream_ptr()), "gst_sync")

    def last_kernel_ms(self):
        ms = ct.c_double()
        _abi.check(self.lib, self.lib.gst_last_sweep_ms(self.ctx, ct.byref(ms)),
                   "gst_last_sweep_ms")
        return ms.value

    def set_timing(self, on: bool = True):
        """Per-kernel HIP-event timing of the large path (kernel_times())."""
        _abi.check(self.lib, self.lib.gst_set_timing(self.ctx, int(bool(on))), "gst_set_timing")

    def kernel_times(self):
        """{kind: (total ms, launches)} for the last launch with timing enabled."""
        k = len(_abi.KERNEL_KINDS)
        ms = (ct.c_double * k)()
        nl = (ct.c_int * k)()
        _abi.check(self.lib, self.lib.gst_kernel_times(self.ctx, ms, nl, k), "gst_kernel_times")
        return {name: (ms[i], nl[i]) for i, name in enumerate(_abi.KERNEL_KINDS)}

    def gram_counts(self, reset: bool = True):
        """Grams computed since the last reset, by path (include/gst.h gst_gram_counts):
        {"low_rank": persistent low-rank (VALU), "mfma": persistent fp64 MFMA,
        "large_mfma": large path fp64 MFMA} in chain-Grams; synchronises the device."""
        v = (ct.c_longlong * 3)()
        _abi.check(self.lib, self.lib.gst_gram_counts(self.ctx, v, int(bool(reset))),
                   "gst_gram_counts")
        return {"low_rank": int(v[0]), "mfma": int(v[1]), "large_mfma": int(v[2])}

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.gst_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


def pack_tape(ref_tape: dict, sweeps, n: int, m: int, stride: int, nst: int | None = None):
    """Golden-fixture tape (tools/gen_golden.py fields) -> [len(sweeps), stride] rows.

    ``nst`` is the per-TOA row stride of the launch (the batch's largest n; default n)."""
    nst = n if nst is None else int(nst)
    rows = np.zeros((len(sweeps), stride))
    for k, i in enumerate(sweeps):
        row = rows[k]
        for stage, off, ns in (("white", _abi.TAPE_WHITE, 20), ("hyper", _abi.TAPE_HYPER, 10)):
            e = np.stack([ref_tape[f"{stage}_u"][i], ref_tape[f"{stage}_idx"][i].astype(float),
                          ref_tape[f"{stage}_xi"][i], ref_tape[f"{stage}_acc"][i]], axis=1)
            row[off:off + 4 * ns] = e.reshape(-1)
        o = _abi.TAPE_DELTA
        row[o:o + m] = np.nan_to_num(ref_tape["b_delta"][i])
        row[o + m] = ref_tape["beta"][i]
        row[o + m + 1:o + m + 1 + n] = ref_tape["z_u"][i]
        row[o + m + 1 + nst:o + m + 1 + nst + n] = ref_tape["gamma"][i]
        row[o + m + 1 + 2 * nst] = ref_tape["df_u"][i]
    return rows


def debug_variates(kind: str, a: float, n: int, b: float = 1.0, seed: int = 1, call: int = 0,
                   device: int = 0):
    """The kernel's own samplers (include/gst.h gst_debug_variates) -> float64 device tensor:
    kind "gamma" (gamma_mt), "beta" (the theta stage's two-gamma Beta), "gamma_slots" (the
    alpha stage's gamma_mt_slots<4>; n a multiple of 256)."""
    torch = _torch()
    lib = _abi.load()
    k = {"gamma": 0, "beta": 1, "gamma_slots": 2}[kind]
    out = torch.empty(int(n), dtype=torch.float64, device=f"cuda:{device}")
    with torch.cuda.device(device):
        st = torch.cuda.current_stream().cuda_stream
        rc = lib.gst_debug_variates(k, float(a), float(b), int(n), int(seed), int(call),
                                    ct.c_void_p(out.data_ptr()), ct.c_void_p(st))
    _abi.check(lib, rc, "gst_debug_variates")
    return out
