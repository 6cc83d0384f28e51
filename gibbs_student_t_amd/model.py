"""Structured single-pulsar noise model: the "pta" object `Gibbs` consumes.

The reference sampler (`/root/reference/gibbs.py`) talks to an enterprise ``PTA``
through five duck-typed calls:

* ``get_residuals()[0]``                       (gibbs.py:29)
* ``get_basis(params)[0]``                     (gibbs.py:35,158,210,236,269,301)
* ``get_ndiag(params)[0]``                     (gibbs.py:154,209,235,268,297)
* ``get_phiinv(params, logdet=...)[0]``        (gibbs.py:155,298)
* ``params`` (objects with ``.name``, ``.get_logpdf``, ``.sample``)  (gibbs.py:56,339;
  run_sims.py:111)

enterprise is not installed here (no network) and is not vendored by the reference, so
this module restates the *specific* model `run_sims.py:57-83` builds:

* white noise ``N0 = efac^2 * sigma^2 + 10^(2*log10_equad)``  (MeasurementNoise + EquadNoise,
  run_sims.py:57-62); efac is ``Constant(1.0)`` there, ``Uniform(0.2, 10)`` in the notebook.
* red noise: Fourier GP, ``components`` sin/cos pairs on ``f_k = k / Tspan``, power-law
  spectrum with ``log10_A ~ U(-18,-12)``, ``gamma ~ U(1,7)`` (run_sims.py:65-66).
* timing model: ``BasisGP`` on the SVD basis ``U`` of the design matrix with prior weight
  ``1e40`` (run_sims.py:22-29,69-71).

and, as the notebook's J1643-1224 model uses them (gibbs_likelihood.ipynb cell 2), the
general white-noise options the reference sampler handles through its index sets
(gibbs.py:64-77: any ``ecorr`` parameter is a hyper parameter, any ``efac``/``equad`` a white
one):

* ``selection="backend"``: one efac / log10_equad (/ log10_ecorr) per backend
  (enterprise ``selections.by_backend``), parameters named ``{psr}_{backend}_efac`` etc.;
  ``"none"`` (``no_selection``): one set named ``{psr}_efac`` etc.
* ``log10_ecorr=(pmin, pmax)``: ECORR as a basis GP (enterprise ``EcorrBasisModel``): one
  column per observing epoch with at least two TOAs (``quantization_matrix``), per backend
  under ``selection="backend"``, prior variance ``10^(2 log10_ecorr)``.

The enterprise formulas (Fourier design matrix, power law, ``phiinv``/``logdet`` from a
diagonal ``phi``) are restated from their published form; parity against enterprise
itself is **unpinned** (no fixture of it exists in the reference).  Everything else in the
build -- the CPU oracle, the golden generator and the HIP path -- consumes this one model,
so the sampler parity is exact with respect to it.

* ``dm_gp=dict(components=, log10_A=(lo, hi), gamma=(lo, hi))`` / ``chrom_gp=...``:
  dispersion-measure variations and a scattering-like chromatic process, each a second
  power-law Fourier GP whose basis is scaled by ``(1400 MHz / nu)^2`` resp. ``^4``
  (enterprise ``createfourierdesignmatrix_dm`` / ``_chromatic`` with ``utils.powerlaw``),
  parameters ``{psr}_dm_gp_log10_A``, ``{psr}_dm_gp_gamma``, ``{psr}_chrom_gp_...``.  The
  reference sampler takes every ``log10_A`` / ``gamma`` parameter as a hyper parameter
  (gibbs.py:64-69) and asks the pta for ``phi``, so it runs such a model unchanged.

Column order of the basis ``T`` is ``[Fourier (red | dm | chrom) | timing model | ECORR]`` as
in enterprise's signal-collection order ``ef + eq + rn (+ dm) + tm (+ ec)`` (run_sims.py:74,
gibbs_likelihood.ipynb cell 2); ``Ffreqs`` is each process's ``repeat(f, 2)`` in turn and
``pta.procs`` describes the layout.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

# enterprise.constants: yr = 365.25 * 86400 s, fyr = 1 / yr
YR_SEC = 365.25 * 86400.0
FYR = 1.0 / YR_SEC
DAY_SEC = 86400.0


class Constant:
    """A fixed parameter (enterprise ``parameter.Constant``); never sampled."""

    def __init__(self, value: float):
        self.value = float(value)


class Uniform:
    """Uniform prior parameter (enterprise ``parameter.Uniform``).

    ``get_logpdf`` is ``scipy.stats.uniform(pmin, pmax - pmin).logpdf``: ``-log(pmax-pmin)``
    on the closed interval, ``-inf`` outside (called at gibbs.py:339).
    """

    def __init__(self, name: str, pmin: float, pmax: float):
        self.name = name
        self.pmin = float(pmin)
        self.pmax = float(pmax)
        self.logpdf_in = -np.log(self.pmax - self.pmin)

    def get_logpdf(self, value):
        value = float(value)
        if self.pmin <= value <= self.pmax:
            return self.logpdf_in
        return -np.inf

    def sample(self):
        # run_sims.py:111 draws the initial point from the priors
        return np.random.uniform(self.pmin, self.pmax)

    def __repr__(self):
        return f"{self.name}:Uniform(pmin={self.pmin}, pmax={self.pmax})"


def fourier_basis(toas: np.ndarray, nmodes: int, Tspan: float | None = None):
    """Red-noise Fourier design matrix (enterprise ``createfourierdesignmatrix_red``).

    Columns alternate sin/cos of ``2 pi f_k t`` with ``f_k = k / Tspan``, k = 1..nmodes.
    Returns ``(F, Ffreqs)`` with ``Ffreqs = repeat(f, 2)``.
    """
    T = Tspan if Tspan is not None else toas.max() - toas.min()
    f = np.linspace(1.0 / T, nmodes / T, nmodes)
    F = np.zeros((len(toas), 2 * nmodes))
    arg = 2.0 * np.pi * toas[:, None] * f[None, :]
    F[:, ::2] = np.sin(arg)
    F[:, 1::2] = np.cos(arg)
    return F, np.repeat(f, 2)


# Power-law processes of the Fourier block beside the achromatic red noise, in basis order:
# (PTA keyword, chromatic index chi).  Process p's basis is the red-noise Fourier basis scaled
# TOA by TOA with (FREF_MHZ / nu_t)^chi (enterprise ``createfourierdesignmatrix_dm`` for
# chi = 2, ``createfourierdesignmatrix_chromatic`` with idx = 4), its parameters are named
# ``<psr>_<keyword>_log10_A`` / ``<psr>_<keyword>_gamma``.
CHROMATIC_GPS = (("dm_gp", 2), ("chrom_gp", 4))
FREF_MHZ = 1400.0
# enterprise.constants.DM_K: a delay of dt seconds at radio frequency nu (MHz) is a dispersion
# measure of DM_K * nu^2 * dt pc cm^-3
DM_K = 2.41e-4


@dataclass(frozen=True)
class Process:
    """One power-law process of the Fourier block: its columns of ``T`` (``col0`` ..
    ``col0 + ncol``), chromatic index and the indices of its two parameters in ``params``."""

    name: str          # "red", "dm_gp", "chrom_gp"
    chi: int
    components: int
    col0: int
    ncol: int
    idx_log10_A: int
    idx_gamma: int


def chromatic_basis(toas, freqs, nmodes: int, chi: int, Tspan: float | None = None):
    """Fourier design matrix of a chromatic process: ``fourier_basis`` with every row scaled by
    ``(1400 MHz / nu_t)^chi``.  Returns ``(F, Ffreqs)``; the ladder is the process's own."""
    F, ff = fourier_basis(toas, nmodes, Tspan)
    return F * ((FREF_MHZ / np.asarray(freqs, dtype=np.float64)) ** chi)[:, None], ff


def powerlaw(f: np.ndarray, log10_A: float, gamma: float, components: int = 2):
    """Power-law prior variances (enterprise ``utils.powerlaw``).

    ``phi_k = A^2 / 12 / pi^2 * fyr^(gamma-3) * f_k^(-gamma) * df_k``.  The left-to-right
    evaluation order is part of the contract the HIP kernel reproduces.
    """
    df = np.diff(np.concatenate((np.array([0.0]), f[::components])))
    return ((10 ** log10_A) ** 2 / 12.0 / np.pi ** 2 * FYR ** (gamma - 3)
            * f ** (-gamma) * np.repeat(df, components))


def quantization_matrix(toas: np.ndarray, dt: float = 1.0, nmin: int = 2):
    """Epoch basis of ECORR (enterprise ``utils.create_quantization_matrix``): TOAs sorted
    by time, a new epoch whenever a TOA is ``dt`` seconds or more after the epoch's first
    TOA; epochs with fewer than ``nmin`` TOAs get no column.  Returns ``U`` (n x epochs,
    one 1 per row of a TOA in a kept epoch)."""
    toas = np.asarray(toas, dtype=np.float64)
    isort = np.argsort(toas, kind="stable")
    buckets = [[isort[0]]] if len(toas) else []
    ref = toas[isort[0]] if len(toas) else 0.0
    for i in isort[1:]:
        if toas[i] - ref < dt:
            buckets[-1].append(i)
        else:
            buckets.append([i])
            ref = toas[i]
    buckets = [b for b in buckets if len(b) >= nmin]
    U = np.zeros((len(toas), len(buckets)))
    for e, b in enumerate(buckets):
        U[b, e] = 1.0
    return U


def svd_tm_basis(Mmat: np.ndarray):
    """Timing-model basis: left singular vectors of the design matrix (run_sims.py:22-25)."""
    u, s, _ = np.linalg.svd(Mmat, full_matrices=False)
    return u, np.ones_like(s)


@dataclass
class PulsarData:
    """What the sampler needs from a pulsar (enterprise ``Pulsar`` subset)."""

    name: str
    toas: np.ndarray        # seconds
    residuals: np.ndarray   # seconds
    toaerrs: np.ndarray     # seconds
    Mmat: np.ndarray        # timing-model design matrix (n x ntm)
    freqs: np.ndarray | None = None
    meta: dict = field(default_factory=dict)
    backends: np.ndarray | None = None   # backend label of each TOA (tim-file flag -be/-f)

    @property
    def n(self):
        return len(self.toas)


class PTA:
    """Single-pulsar model with the enterprise ``PTA`` protocol used by ``Gibbs``.

    Parameters mirror run_sims.py:57-71.  ``efac`` may be a float (constant, run_sims)
    or a ``(pmin, pmax)`` tuple (varied, as in the notebook).
    """

    def __init__(self, psr: PulsarData, components: int = 30, efac=1.0,
                 log10_equad=(-10.0, -5.0), log10_A=(-18.0, -12.0), gamma=(1.0, 7.0),
                 tm_weight: float = 1e40, Tspan: float | None = None, *,
                 selection: str = "none", log10_ecorr=None, ecorr_dt: float = 1.0,
                 dm_gp=None, chrom_gp=None):
        self.psr = psr
        self.components = int(components)
        self._r = np.asarray(psr.residuals, dtype=np.float64)
        self._toaerrs = np.asarray(psr.toaerrs, dtype=np.float64)
        toas = np.asarray(psr.toas, dtype=np.float64)
        # the ladder's span, remembered for process_basis at other epochs
        self.Tspan = float(Tspan) if Tspan is not None else float(toas.max() - toas.min())
        self.F, self.Ffreqs = fourier_basis(toas, self.components, Tspan)
        # dispersion-measure / chromatic power laws: dict(components=, log10_A=(lo, hi),
        # gamma=(lo, hi)); their columns follow the red noise's, T = [red | dm | chrom | ...]
        self._gps = self._gp_specs(dm_gp=dm_gp, chrom_gp=chrom_gp)
        for kw, chi, spec in self._gps:
            if psr.freqs is None:
                raise ValueError(f"{kw} needs psr.freqs (the TOAs' radio frequencies, MHz)")
            Fp, ffp = chromatic_basis(toas, psr.freqs, spec["components"], chi, Tspan)
            self.F = np.hstack([self.F, Fp])
            self.Ffreqs = np.concatenate([self.Ffreqs, ffp])
        U, w = svd_tm_basis(np.asarray(psr.Mmat, dtype=np.float64))
        self.U = U
        self.tm_phi = w * tm_weight          # tm_prior (run_sims.py:27-29)
        self.tm_weight = float(tm_weight)
        self._set_backends(psr.backends, selection)
        cols, self.ecorr_backend = [], np.zeros(0, dtype=np.int64)
        if log10_ecorr is not None:
            # one quantization per backend (enterprise applies the basis per selection mask)
            eb = []
            for b in range(len(self.backend_names)):
                mask = self.bidx == b
                Ub = quantization_matrix(toas[mask], ecorr_dt)
                full = np.zeros((len(toas), Ub.shape[1]))
                full[mask] = Ub
                cols.append(full)
                eb += [b] * Ub.shape[1]
            self.ecorr_backend = np.array(eb, dtype=np.int64)
        self.Uec = np.hstack(cols) if cols else np.zeros((len(toas), 0))
        self.T = np.hstack([self.F, self.U, self.Uec])
        self._build_params(efac, log10_equad, log10_A, gamma, log10_ecorr)

    # --- white-noise structure ----------------------------------------------------------
    def _set_backends(self, backends, selection):
        if selection not in ("none", "backend"):
            raise ValueError("selection must be 'none' or 'backend'")
        n = len(self._r)
        self.selection = selection
        if selection == "backend":
            if backends is None:
                raise ValueError("selection='backend' needs psr.backends")
            labels = np.asarray(backends).astype(str)
            self.backend_names = sorted(set(labels.tolist()))
            self.bidx = np.array([self.backend_names.index(v) for v in labels], dtype=np.int64)
        else:
            self.backend_names = [""]
            self.bidx = np.zeros(n, dtype=np.int64)

    @staticmethod
    def _gp_specs(**gps):
        """[(keyword, chi, dict(components, log10_A, gamma))] of the given chromatic processes,
        in basis order, with the red noise's default priors filled in."""
        out = []
        for kw, chi in CHROMATIC_GPS:
            spec = gps.get(kw)
            if spec is None:
                continue
            unknown = set(spec) - {"components", "log10_A", "gamma"}
            if unknown or "components" not in spec or int(spec["components"]) < 1:
                raise ValueError(f"{kw}: dict(components=, log10_A=(lo, hi), gamma=(lo, hi))")
            out.append((kw, chi, dict(components=int(spec["components"]),
                                      log10_A=tuple(spec.get("log10_A", (-18.0, -12.0))),
                                      gamma=tuple(spec.get("gamma", (1.0, 7.0))))))
        return out

    def _pname(self, b, what):
        be = self.backend_names[b]
        return f"{self.psr.name}_{be}_{what}" if be else f"{self.psr.name}_{what}"

    def _build_params(self, efac, log10_equad, log10_A, gamma, log10_ecorr):
        nm = self.psr.name
        plist = []
        nb = len(self.backend_names)
        if isinstance(efac, (tuple, list)):
            plist += [Uniform(self._pname(b, "efac"), *efac) for b in range(nb)]
            self.efac_const = None
        else:
            self.efac_const = float(efac)
        plist += [Uniform(self._pname(b, "log10_equad"), *log10_equad) for b in range(nb)]
        if log10_ecorr is not None:
            plist += [Uniform(self._pname(b, "log10_ecorr"), *log10_ecorr) for b in range(nb)]
        plist.append(Uniform(f"{nm}_log10_A", *log10_A))
        plist.append(Uniform(f"{nm}_gamma", *gamma))
        for kw, _, spec in self._gps:
            plist.append(Uniform(f"{nm}_{kw}_log10_A", *spec["log10_A"]))
            plist.append(Uniform(f"{nm}_{kw}_gamma", *spec["gamma"]))
        # enterprise returns params sorted by name
        self._params = sorted(plist, key=lambda p: p.name)
        self.has_ecorr = log10_ecorr is not None
        # the layout of the Fourier block, process by process
        names = [p.name for p in self._params]
        self.procs, col0 = [], 0
        for kw, chi, nc in [("red", 0, self.components)] + \
                [(kw, chi, spec["components"]) for kw, chi, spec in self._gps]:
            pre = f"{nm}_" if kw == "red" else f"{nm}_{kw}_"
            self.procs.append(Process(kw, chi, nc, col0, 2 * nc, names.index(pre + "log10_A"),
                                      names.index(pre + "gamma")))
            col0 += 2 * nc

    @classmethod
    def from_arrays(cls, name, residuals, toaerrs, T, Ffreqs, components, tm_weight=1e40,
                    efac=1.0, **priors):
        """Rebuild a model from stored arrays (golden fixtures) without re-deriving T.
        ``components`` counts the red noise's; ``dm_gp`` / ``chrom_gp`` (keywords, as in the
        constructor) say how the rest of the Fourier block of ``T`` / ``Ffreqs`` splits."""
        obj = cls.__new__(cls)
        obj.psr = PulsarData(name=str(name), toas=np.zeros(len(residuals)),
                             residuals=np.asarray(residuals), toaerrs=np.asarray(toaerrs),
                             Mmat=np.zeros((len(residuals), 0)))
        obj.components = int(components)
        obj.Tspan = None                     # no epochs: process_basis raises
        obj._r = np.asarray(residuals, dtype=np.float64)
        obj._toaerrs = np.asarray(toaerrs, dtype=np.float64)
        # the Fourier block: [red | dm | chrom], Ffreqs each process's ladder in turn
        obj._gps = cls._gp_specs(dm_gp=priors.pop("dm_gp", None),
                                 chrom_gp=priors.pop("chrom_gp", None))
        nf = 2 * (obj.components + sum(spec["components"] for _, _, spec in obj._gps))
        T = np.asarray(T, dtype=np.float64)
        obj.F, obj.Ffreqs = T[:, :nf], np.asarray(Ffreqs, dtype=np.float64)
        obj.U = T[:, nf:]
        obj.tm_weight = float(tm_weight)
        n_ec = int(priors.pop("n_ecorr", 0))
        ntm = T.shape[1] - nf - n_ec
        obj.U = T[:, nf:nf + ntm]
        obj.Uec = T[:, nf + ntm:]
        obj.tm_phi = np.ones(obj.U.shape[1]) * obj.tm_weight
        obj.T = T
        obj.psr.backends = priors.pop("backends", None)
        obj._set_backends(obj.psr.backends, priors.pop("selection", "none"))
        eb = priors.pop("ecorr_backend", None)
        obj.ecorr_backend = (np.zeros(0, dtype=np.int64) if eb is None
                             else np.asarray(eb, dtype=np.int64))
        obj._build_params(efac, priors.get("log10_equad", (-10., -5.)),
                          priors.get("log10_A", (-18., -12.)), priors.get("gamma", (1., 7.)),
                          priors.get("log10_ecorr"))
        return obj

    # --- the protocol ---------------------------------------------------------------
    @property
    def params(self):
        return list(self._params)

    @property
    def param_names(self):
        return [p.name for p in self._params]

    def get_residuals(self):
        return [self._r]

    def get_basis(self, params=None):
        return [self.T]

    def _value(self, params, suffix):
        return params[f"{self.psr.name}_{suffix}"]

    def get_ndiag(self, params):
        if len(self.backend_names) == 1:
            efac = (self.efac_const if self.efac_const is not None
                    else params[self._pname(0, "efac")])
            eq = params[self._pname(0, "log10_equad")]
            return [efac ** 2 * self._toaerrs ** 2 + 10 ** (2 * eq) * np.ones(len(self._r))]
        nb = len(self.backend_names)
        efac = np.array([self.efac_const if self.efac_const is not None
                         else params[self._pname(b, "efac")] for b in range(nb)])[self.bidx]
        eq = np.array([params[self._pname(b, "log10_equad")] for b in range(nb)])[self.bidx]
        return [efac ** 2 * self._toaerrs ** 2 + 10 ** (2 * eq)]

    def get_phi(self, params):
        pl = powerlaw(self.Ffreqs[:2 * self.components], self._value(params, "log10_A"),
                      self._value(params, "gamma"), components=2)
        parts = [pl]
        for pr in self.procs[1:]:   # each over its own ladder: df restarts at f_1 - 0
            parts.append(powerlaw(self.Ffreqs[pr.col0:pr.col0 + pr.ncol],
                                  self._value(params, f"{pr.name}_log10_A"),
                                  self._value(params, f"{pr.name}_gamma"), components=2))
        parts.append(self.tm_phi)
        if self.n_ecorr:
            ec = np.array([params[self._pname(b, "log10_ecorr")]
                           for b in range(len(self.backend_names))])
            parts.append(10 ** (2 * ec[self.ecorr_backend]))
        return [np.concatenate(parts)]

    def get_phiinv(self, params, logdet=False):
        phi = self.get_phi(params)[0]
        if logdet:
            return [(1.0 / phi, np.sum(np.log(phi)))]
        return [1.0 / phi]

    # --- convenience for the native path --------------------------------------------
    @property
    def n(self):
        return self.T.shape[0]

    @property
    def m(self):
        return self.T.shape[1]

    @property
    def nfourier(self):
        return self.F.shape[1]

    @property
    def ntm(self):
        return self.U.shape[1]

    @property
    def n_ecorr(self):
        return self.Uec.shape[1]

    @property
    def nbackend(self):
        return len(self.backend_names)

    def backend_param_indices(self, what):
        """Index into ``params`` of each backend's ``what`` parameter (-1: none / constant)."""
        names = self.param_names
        return np.array([names.index(self._pname(b, what)) if self._pname(b, what) in names
                         else -1 for b in range(len(self.backend_names))], dtype=np.int64)

    def param_index(self, suffix):
        """Index of the parameter ``<psr>_<suffix>``, else of the first whose name ends in
        ``_<suffix>`` (per-backend names) and is not another process's (``dm_gp_log10_A``
        sorts before ``log10_A``)."""
        names = self.param_names
        exact = f"{self.psr.name}_{suffix}"
        if exact in names:
            return names.index(exact)
        for i, nm in enumerate(names):
            if nm.endswith("_" + suffix) and \
                    not any(nm.endswith(f"_{kw}_{suffix}") for kw, _ in CHROMATIC_GPS):
                return i
        return -1

    def process_columns(self, name):
        """``(lo, hi)``: the columns [lo, hi) of ``T`` (and of b) that the process ``name``
        ("red", "dm_gp", "chrom_gp") owns."""
        for pr in self.procs:
            if pr.name == name:
                return pr.col0, pr.col0 + pr.ncol
        raise ValueError(f"unknown process {name!r}; this model has "
                         f"{[pr.name for pr in self.procs]}")

    def process_basis(self, name, toas=None, freqs=None, scaled=True):
        """Fourier basis of the process ``name`` ("red", "dm_gp", "chrom_gp") at the epochs
        ``toas`` (seconds) and radio frequencies ``freqs`` (MHz), on the model's own ladder
        f_k = k / Tspan: [len(toas), 2 * components], the design matrix of the process's
        waveform on any grid, between and beyond the TOAs.  Defaults: the model's TOAs and
        their frequencies, where the result is bitwise the process's columns of ``T``.
        ``scaled=False`` leaves out the ``(1400 MHz / nu)^chi`` weight of a chromatic process
        (``freqs`` is then not needed): the delay at 1400 MHz, which times
        ``DM_K * 1400^2`` (enterprise's ``DM_K = 2.41e-4``) is DM(t) in pc cm^-3 for
        ``dm_gp``.  Like the rest of this module the formulas are restated from enterprise's
        published form; parity against enterprise itself is **unpinned**.
        A model rebuilt by ``from_arrays`` has neither epochs nor a span and raises."""
        self.process_columns(name)           # an unknown process raises
        pr = next(p_ for p_ in self.procs if p_.name == name)
        if getattr(self, "Tspan", None) is None:
            raise ValueError("process_basis: this model was rebuilt from arrays and has no "
                             "epochs or span; build it from the pulsar (PTA(psr, ...))")
        own = toas is None
        toas = np.asarray(self.psr.toas if own else toas, dtype=np.float64)
        F, _ = fourier_basis(toas, pr.components, self.Tspan)
        if not scaled or pr.chi == 0:
            return F
        if freqs is None:
            if not own:
                raise ValueError(f"process_basis: {name} at other epochs needs freqs (MHz)")
            freqs = self.psr.freqs
        freqs = np.broadcast_to(np.asarray(freqs, dtype=np.float64), toas.shape)
        return F * ((FREF_MHZ / freqs) ** pr.chi)[:, None]

    def sample_params(self):
        return np.array([p.sample() for p in self._params]).flatten()


def df_tables(n: int):
    """Constant parts of the dof log-density (gibbs.py:331-335) for nu = 1..30.

    ``ll(nu) = -(nu/2)*S + A[nu] - B[nu]`` with ``A = n*(nu/2)*log(nu/2)`` and
    ``B = n*gammaln(nu/2)``; evaluated on the host exactly as the reference does so the
    device only adds ``-(nu/2)*S``.
    """
    import scipy.special
    dfs = np.arange(1, 31)
    A = np.array([n * (df / 2) * np.log(df / 2) for df in dfs])
    B = np.array([n * scipy.special.gammaln(df / 2) for df in dfs])
    return A, B


def hyper_white_indices(names):
    """Parameter index sets (gibbs.py:64-77): hyper = ecorr/log10_A/gamma, white = efac/equad."""
    hind = [i for i, nm in enumerate(names)
            if "ecorr" in nm or "log10_A" in nm or "gamma" in nm]
    wind = [i for i, nm in enumerate(names) if "efac" in nm or "equad" in nm]
    return np.array(hind, dtype=np.int64), np.array(wind, dtype=np.int64)


def mh_constants():
    """Jump-scale mixture of the MH proposals (gibbs.py:93-94,126-127)."""
    return np.array([0.1, 0.15, 0.5, 0.15, 0.1]), np.array([0.1, 0.5, 1.0, 3.0, 10.0])


__all__ = ["Constant", "Uniform", "PulsarData", "PTA", "Process", "fourier_basis",
           "chromatic_basis", "powerlaw", "CHROMATIC_GPS", "FREF_MHZ", "DM_K",
           "svd_tm_basis", "quantization_matrix", "df_tables", "hyper_white_indices", "mh_constants",
           "FYR", "YR_SEC", "DAY_SEC"]
