"""DM and chromatic power-law processes beside the red noise, on the CPU: the model
(``PTA(dm_gp=, chrom_gp=)``), ``data.multiband``'s new arguments, the host packer's per-process
spectrum pieces, the ctypes struct against the header, the binding's descriptor, and the
unchanged oracle reproducing every new reference fixture bit for bit."""
import ctypes as ct
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from gibbs_student_t_amd import _abi, data, model
from golden_io import (CHAIN_KEYS, GOLDEN, MGP_DATASETS, MGP_NAMES, fixture_names, load_dataset,
                       load_ref)
from support import PACKINGS, PACK_DIMS, host_tool, pack_dataset, run_packer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = np.linspace(1150.0, 1850.0, 3)


@pytest.fixture(scope="module")
def psr():
    return data.multiband(20, 3, seed=5, band_mhz=BAND, dm=(-13.3, 2.8, 4))


# ---- the model -----------------------------------------------------------------------------
def test_layout_names_and_sort_order(psr):
    pta = model.PTA(psr, components=6, dm_gp=dict(components=4),
                    chrom_gp=dict(components=3, log10_A=(-17.0, -13.0), gamma=(0.5, 6.0)))
    assert pta.param_names == ["MB_chrom_gp_gamma", "MB_chrom_gp_log10_A", "MB_dm_gp_gamma",
                               "MB_dm_gp_log10_A", "MB_gamma", "MB_log10_A", "MB_log10_equad"]
    assert pta.param_names == sorted(pta.param_names)
    assert [(q.name, q.chi, q.col0, q.ncol, q.idx_log10_A, q.idx_gamma) for q in pta.procs] == \
        [("red", 0, 0, 12, 5, 4), ("dm_gp", 2, 12, 8, 3, 2), ("chrom_gp", 4, 20, 6, 1, 0)]
    assert pta.nfourier == 26 and pta.components == 6
    assert pta.T.shape == (60, 26 + pta.ntm)
    p = {q.name: q for q in pta.params}
    assert (p["MB_chrom_gp_log10_A"].pmin, p["MB_chrom_gp_gamma"].pmax) == (-17.0, 6.0)
    assert (p["MB_dm_gp_log10_A"].pmin, p["MB_dm_gp_gamma"].pmax) == (-18.0, 7.0)
    # every log10_A / gamma is a hyper parameter (gibbs.py:64-69)
    hind, wind = model.hyper_white_indices(pta.param_names)
    assert hind.tolist() == [0, 1, 2, 3, 4, 5] and wind.tolist() == [6]
    # basis: each process the red-noise Fourier basis on its own ladder, scaled per TOA
    F, ff = model.fourier_basis(psr.toas, 6)
    np.testing.assert_array_equal(pta.T[:, :12], F)
    for q in pta.procs[1:]:
        Fq, fq = model.fourier_basis(psr.toas, q.components)
        w = (1400.0 / psr.freqs) ** q.chi
        np.testing.assert_array_equal(pta.T[:, q.col0:q.col0 + q.ncol], Fq * w[:, None])
        np.testing.assert_array_equal(pta.Ffreqs[q.col0:q.col0 + q.ncol], fq)
    np.testing.assert_array_equal(pta.Ffreqs[:12], ff)
    assert len(np.unique(w)) == 3 and w.max() > 1.0 > w.min()


def test_get_phi_against_the_formula(psr):
    pta = model.PTA(psr, components=6, dm_gp=dict(components=4), chrom_gp=dict(components=3))
    vals = dict(chrom_gp_gamma=2.2, chrom_gp_log10_A=-14.6, dm_gp_gamma=2.8, dm_gp_log10_A=-13.3,
                gamma=4.33, log10_A=-14.0, log10_equad=-7.0)
    x = {f"MB_{k}": v for k, v in vals.items()}
    phi = pta.get_phi(x)[0]
    Tspan = psr.toas.max() - psr.toas.min()
    want = []
    for pre, nc in (("", 6), ("dm_gp_", 4), ("chrom_gp_", 3)):
        f = np.repeat(np.arange(1, nc + 1) / Tspan, 2)
        A, g = 10.0 ** vals[pre + "log10_A"], vals[pre + "gamma"]
        # df from the process's own ladder: every pair's df is 1 / Tspan, the first f_1 - 0
        want.append(A ** 2 / (12 * np.pi ** 2) * model.FYR ** (g - 3) * f ** -g / Tspan)
    np.testing.assert_allclose(phi[:26], np.concatenate(want), rtol=1e-12)
    assert np.all(phi[26:] == 1e40)
    phiinv, ld = pta.get_phiinv(x, logdet=True)[0]
    # log|phi| = sum_p (nf_p lc_p - gamma_p sum log f + sum log df) + timing model
    tot = pta.ntm * np.log(1e40)
    for q in pta.procs:
        pre = "" if q.name == "red" else q.name + "_"
        f = pta.Ffreqs[q.col0:q.col0 + q.ncol]
        lc = 2 * vals[pre + "log10_A"] * np.log(10) - np.log(12 * np.pi ** 2) + \
            (vals[pre + "gamma"] - 3) * np.log(model.FYR)
        tot += q.ncol * lc - vals[pre + "gamma"] * np.log(f).sum() - q.ncol * np.log(Tspan)
    assert np.isclose(ld, tot, rtol=1e-13)


def test_exact_name_lookup(psr):
    from gibbs_student_t_amd.native import model_desc
    pta = model.PTA(psr, components=6, dm_gp=dict(components=4))
    names = pta.param_names
    assert names.index("MB_dm_gp_log10_A") < names.index("MB_log10_A")
    assert pta.param_index("log10_A") == names.index("MB_log10_A")
    assert pta.param_index("gamma") == names.index("MB_gamma")
    assert pta.param_index("dm_gp_gamma") == 0 and pta.param_index("nothing") == -1
    desc, keep = model_desc(pta, dict(model="mixture"))
    assert (desc.idx_log10_A, desc.idx_gamma) == (3, 2) and desc.nfourier == 20
    pr = keep["procs"]
    assert pr.nproc == 2 and list(pr.ncol) == [12, 8, 0]
    assert list(pr.idx_log10_A)[:2] == [3, 1] and list(pr.idx_gamma)[:2] == [2, 0]
    # per-backend names still resolve to the first backend's
    ptb = model.PTA(psr, components=6, efac=(0.2, 10.0), selection="backend",
                    dm_gp=dict(components=4))
    assert ptb.param_names[ptb.param_index("efac")] == "MB_ASP_efac"
    assert ptb.param_names[ptb.param_index("log10_A")] == "MB_log10_A"


def test_dm_gp_needs_freqs_and_a_valid_spec(psr):
    with pytest.raises(ValueError, match="freqs"):
        model.PTA(data.multiband(20, 3, seed=5), dm_gp=dict(components=4))
    with pytest.raises(ValueError, match="dm_gp"):
        model.PTA(psr, dm_gp=dict(components=4, index=2))
    with pytest.raises(ValueError, match="band_mhz"):
        data.multiband(20, 3, dm=(-13.3, 2.8, 4))


@pytest.mark.parametrize("ds", ["j1713", "mb", "ecb", "mid"])
def test_defaults_are_todays_object(ds):
    """Without dm_gp / chrom_gp: one process over the whole Fourier block, T, Ffreqs, the
    parameters and phi bit for bit what the stored datasets hold."""
    pta = load_dataset(dataset=ds)
    d = np.load(os.path.join(GOLDEN, f"{ds}_dataset.npz"))
    # (golden_io names every single-backend pulsar J1713+0747)
    assert [n.split("_", 1)[1] for n in pta.param_names] == \
        [str(v).split("_", 1)[1] for v in d["names"]]
    assert len(pta.procs) == 1 and pta.nfourier == 2 * pta.components == 2 * int(d["components"])
    q = pta.procs[0]
    assert (q.name, q.col0, q.ncol) == ("red", 0, pta.nfourier)
    assert pta.param_names[q.idx_log10_A].endswith("_log10_A")
    assert q.idx_log10_A == pta.param_index("log10_A") and q.idx_gamma == pta.param_index("gamma")
    np.testing.assert_array_equal(pta.T, d["T"])
    x = dict(zip(pta.param_names, [0.5 * (p.pmin + p.pmax) for p in pta.params]))
    phi = pta.get_phi(x)[0]
    pl = model.powerlaw(d["Ffreqs"], x[pta.param_names[q.idx_log10_A]],
                        x[pta.param_names[q.idx_gamma]])
    np.testing.assert_array_equal(phi[:pta.nfourier], pl)


def test_constructor_defaults_bitwise():
    """PTA without dm_gp / chrom_gp: T is today's [Fourier | SVD timing model | ECORR] of the
    same functions, bit for bit, and ecb's stored dataset to rounding (its SVD and sines were
    computed on another machine)."""
    raw = data.multiband(24, 3, seed=2443)
    a = model.PTA(raw, components=10, efac=(0.2, 10.0), selection="backend",
                  log10_ecorr=(-8.5, -5.0))
    F, ff = model.fourier_basis(raw.toas, 10)
    U = model.svd_tm_basis(raw.Mmat)[0]
    np.testing.assert_array_equal(a.T[:, :34], np.hstack([F, U]))
    np.testing.assert_array_equal(a.Ffreqs, ff)
    assert a.nfourier == 20 and a.m == 34 + a.n_ecorr and raw.freqs is None
    d = np.load(os.path.join(GOLDEN, "ecb_dataset.npz"))
    assert a.param_names == [str(v) for v in d["names"]]
    np.testing.assert_array_equal(a.T[:, 34:], d["T"][:, 34:])
    np.testing.assert_allclose(a.T[:, :20], d["T"][:, :20], rtol=0, atol=1e-12)
    np.testing.assert_allclose(a.Ffreqs, d["Ffreqs"], rtol=1e-15)


# ---- data.multiband ------------------------------------------------------------------------
def test_multiband_new_arguments():
    """band_mhz / dm None: today's arrays (the mb and mid datasets' stored residuals); band_mhz
    alone changes nothing but freqs; dm adds a nu^-2 realisation from a generator of its own."""
    for ds, kw in (("mb", {}), ("mid", dict(nepochs=130, nsub=3, seed=390))):
        d = np.load(os.path.join(GOLDEN, f"{ds}_dataset.npz"))
        a = data.multiband(**kw)
        # the generator's stream is undisturbed: the error bars (its first draws) bit for bit,
        # the residuals (every later draw, then a projection) to the rounding of a projection
        # computed on another machine
        np.testing.assert_array_equal(a.toaerrs, d["toaerrs"])
        np.testing.assert_allclose(a.residuals, d["residuals"], rtol=0,
                                   atol=1e-9 * np.abs(d["residuals"]).max())
        assert a.freqs is None
    a = data.multiband(20, 3, seed=5)
    b = data.multiband(20, 3, seed=5, band_mhz=BAND)
    c = data.multiband(20, 3, seed=5, band_mhz=BAND, dm=(-13.3, 2.8, 4))
    np.testing.assert_array_equal(a.residuals, b.residuals)
    np.testing.assert_array_equal(b.freqs, np.tile(BAND, 20))
    for k in ("toas", "toaerrs"):
        np.testing.assert_array_equal(getattr(a, k), getattr(c, k))
    np.testing.assert_array_equal(a.meta["z_true"], c.meta["z_true"])
    # the difference is the projected nu^-2 realisation: in the span of the DM basis + the
    # timing model, and larger in the low band
    diff = c.residuals - a.residuals
    Fd, _ = model.chromatic_basis(c.toas, c.freqs, 4, 2)
    U = np.linalg.svd(c.Mmat, full_matrices=False)[0]
    B = np.hstack([Fd, U])
    res = diff - B @ np.linalg.lstsq(B, diff, rcond=None)[0]
    assert np.linalg.norm(res) < 1e-8 * np.linalg.norm(diff) and np.linalg.norm(diff) > 0


# ---- the packer ----------------------------------------------------------------------------
PACK_KEYS = ("Tmf", "Tcol", "resid", "sig2", "ref2int", "cidx", "csig2", "ccount", "Trow", "Gcls",
             "Tx", "Xe", "ekl", "eblk", "bk", "ecb", "cls_b", "ec_count", "lp_sum", "ints",
             "lfreq", "ldf", "sums")


def _pack(pack_bin, tmp_path, d, procs, packing="large"):
    MT, ntm_pad, raug = PACKINGS[packing]
    return run_packer(pack_bin, tmp_path, d, MT, ntm_pad, raug, 1, procs)


@pytest.fixture(scope="module")
def pack_bin(tmp_path_factory):
    return host_tool(tmp_path_factory, "pack_dump")


@pytest.mark.parametrize("packing", ["large", "gen"])
def test_pack_one_process_is_todays_packed_model(pack_bin, tmp_path, packing):
    d = pack_dataset("classes")
    legacy = _pack(pack_bin, tmp_path, d, None, packing)
    one = _pack(pack_bin, tmp_path, d, (1, [PACK_DIMS[1], 0, 0], [6, 0, 0], [7, 0, 0]), packing)
    assert set(legacy) == set(one)
    for k in legacy:
        assert legacy[k].tobytes() == one[k].tobytes(), k
    assert set(PACK_KEYS) <= set(legacy)
    assert one["nproc"][0] == 1 and one["pcol"].tolist() == [0, PACK_DIMS[1], PACK_DIMS[1], PACK_DIMS[1]]
    assert one["pidxA"].tolist() == [6, 6, 6] and one["pidxG"].tolist() == [7, 7, 7]
    # one process: its sums are the block's, the values today's loop gives
    f = d["ffreqs"]
    assert one["psum_lfreq"][0] == one["sums"][0] and one["psum_ldf"][0] == one["sums"][1]
    np.testing.assert_array_equal(one["lfreq"], np.log(f))
    np.testing.assert_array_equal(one["ldf"], np.log(np.repeat([f[0], f[2] - f[0]], 2)))
    assert not one["psum_lfreq"][1:].any() and not one["psum_ldf"][1:].any()


def test_pack_log_df_restarts_at_a_process_boundary(pack_bin, tmp_path):
    """Two processes of one pair each over the 4 Fourier columns, both ladders starting at f_1:
    the legacy packer forms log(f_1 - f_1) at the boundary; with the layout df restarts."""
    d = pack_dataset("classes")
    f1 = 1.0 / 3e8
    d["ffreqs"] = np.repeat([f1, f1], 2)
    with np.errstate(divide="ignore"):
        legacy = _pack(pack_bin, tmp_path, d, None)
    assert np.isneginf(legacy["ldf"][2])
    two = _pack(pack_bin, tmp_path, d, (2, [2, 2, 0], [6, 4, 0], [7, 5, 0]))
    np.testing.assert_array_equal(two["ldf"], np.full(4, np.log(f1)))
    np.testing.assert_array_equal(two["lfreq"], np.full(4, np.log(f1)))
    assert two["nproc"][0] == 2 and two["pcol"].tolist() == [0, 2, 4, 4]
    assert two["pidxA"].tolist() == [6, 4, 6] and two["pidxG"].tolist() == [7, 5, 7]
    assert two["idx_red"].tolist() == [6, 7]
    s = np.log(f1) + np.log(f1)
    assert two["psum_lfreq"].tolist() == [s, s, 0.0] and two["psum_ldf"].tolist() == [s, s, 0.0]
    # everything that does not look at what a Fourier column means is unchanged
    for k in PACK_KEYS:
        if k not in ("lfreq", "ldf", "sums"):
            assert two[k].tobytes() == legacy[k].tobytes(), k
    # a first pair that is not the lowest frequency of the block still has df = f - 0
    d["ffreqs"] = np.array([2 * f1, 2 * f1, f1, f1])
    two = _pack(pack_bin, tmp_path, d, (2, [2, 2, 0], [6, 4, 0], [7, 5, 0]))
    np.testing.assert_array_equal(two["ldf"], np.log([2 * f1, 2 * f1, f1, f1]))


# ---- the ABI ------------------------------------------------------------------------------
PROG = r"""
#include <stddef.h>
#include <stdio.h>
#include "gst.h"
int main(void) {
  printf("%d %d %zu", GST_ABI_VERSION, GST_NPROC_MAX, sizeof(gst_model_procs));
  printf(" %zu %zu %zu %zu %zu %zu\n", offsetof(gst_model_procs, nproc),
         offsetof(gst_model_procs, ncol), sizeof(((gst_model_procs*)0)->ncol),
         offsetof(gst_model_procs, idx_log10_A), offsetof(gst_model_procs, idx_gamma),
         sizeof(gst_model_desc));
  return 0;
}
"""


def test_model_procs_struct_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(PROG)
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    Pr = _abi.ModelProcs
    assert [f for f, _ in Pr._fields_] == ["nproc", "ncol", "idx_log10_A", "idx_gamma"]
    assert got == [_abi.ABI_VERSION, _abi.NPROC_MAX, ct.sizeof(Pr), Pr.nproc.offset,
                   Pr.ncol.offset, Pr.ncol.size, Pr.idx_log10_A.offset, Pr.idx_gamma.offset,
                   ct.sizeof(_abi.ModelDesc)]
    # additive: the version stays 7 and callers find the entry point by symbol lookup
    assert _abi.ABI_VERSION == 7 and "gst_model_set_procs" in _abi.EXPORTS
    assert "gst_model_set_procs" in _abi.OPTIONAL


# ---- the fixtures and the oracle --------------------------------------------------------------
@pytest.mark.parametrize("ds", list(MGP_DATASETS))
def test_fixture_layout(ds):
    pta = load_dataset(dataset=ds)
    ncols, nec, path = MGP_DATASETS[ds]
    assert tuple(q.ncol for q in pta.procs) == ncols and pta.n_ecorr == nec
    assert [q.name for q in pta.procs] == ["red", "dm_gp", "chrom_gp"][:len(ncols)]
    assert pta.nfourier == sum(ncols) and pta.m == sum(ncols) + pta.ntm + nec
    if path == "persistent":      # the GEN instances' limits: 8 parameters, 46 hyper columns
        assert len(pta.params) <= 8 and sum(ncols) + nec <= 46 and pta.ntm <= 16
    else:
        assert sum(ncols) + nec > 60
    for kind in ("fixed", "prior"):
        fn = os.path.join(GOLDEN, f"mgp_ref_{ds}_beta_{kind}.npz")
        assert os.path.getsize(fn) <= 392975       # ref_wide_beta_fixed.npz, today's largest
    assert not any(n.startswith(("dm", "mgp")) for n in fixture_names())


@pytest.mark.parametrize("name", MGP_NAMES)
def test_legacy_stream_reproduces_reference_bit_exact(name):
    """The unchanged oracle on the reference's RNG stream: identical chains, and the recorded
    sweep count (12; dm3: 6) from the injected values and from a prior draw."""
    from oracle.gibbs_oracle import Oracle, OutlierModel
    ref = load_ref(name)
    assert int(ref["niter"]) == (6 if name.startswith("dm3") else 12)
    assert int(ref["prior_draw"]) == int(name.endswith("prior"))
    orc = Oracle(ref["pta"], OutlierModel(**ref["kw"]))
    np.random.seed(int(ref["seed"]))
    xs = ref["pta"].sample_params() if int(ref["prior_draw"]) else ref["xs"]
    np.testing.assert_array_equal(xs, ref["xs"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, st, x = orc.run(xs, int(ref["niter"]))
    for k in CHAIN_KEYS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    np.testing.assert_array_equal(st.b, ref["final_b"])
    np.testing.assert_array_equal(st.alpha, ref["final_alpha"])
    # every process's parameters moved in the recorded run
    moved = np.ptp(ref["chain"], axis=0) > 0
    for q in ref["pta"].procs:
        assert moved[q.idx_log10_A] or moved[q.idx_gamma], q.name
