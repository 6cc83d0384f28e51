"""The shared draw laws (csrc/gst_draws.h) on the host, against the CPU oracles.

tools/draws_dump.cpp includes only gst_draws.h and philox.hpp and is built with g++: that it
builds at all shows the laws' header is free of HIP.  It evaluates the laws at the inputs written
here; the results are compared with oracle/philox_variates.py (uniforms, MH variates) and
with the power law as the reference's model evaluates it.  Discrete results must be equal;
real-valued ones agree to a relative error (host libm and numpy differ in the last ulp of
exp / log / cos).  The z, alpha, theta and nu laws are not covered here: they are not in
gst_draws.h (each kernel keeps its copy; tests/test_gpu_draw_laws.py pins them per kernel).
"""
import subprocess

import numpy as np
import pytest

from oracle import philox_variates as pv
from support import host_tool

SEED = 0x5EED0123456789AB
C, S = 3, 4                     # chains x sweeps of MH variates (x 30 steps)
WIND, HIND = [2, 0, 5], [1, 3, 4, 6, 7]
CDF = [0.1, 0.25, 0.75, 0.9, 1.0]        # hypothetical jump-scale mixture (5 classes)
SIZE = [0.01, 0.2, 1.0, 3.0, 10.0]
NH, NF = 12, 30
FYR = 1.0 / (365.25 * 86400.0)
# Largest relative errors measured on the CPU against the oracles (x86-64, g++ -O1, glibc libm
# vs numpy / scipy); each bound below is 4x the measured value.
MEASURED = {
    "normal": 6.172e-14,   # relative: the cosine's absolute ~1e-16 near its zeros
    "log_u": 1.323e-16, "pow10": 2.932e-15, "lc": 2.798e-16, "phi_inv": 2.613e-14,
    "phi_inv_ecorr": 6.076e-15, "logdet_phi": 6.111e-16,
}


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


@pytest.fixture(scope="module")
def laws(tmp_path_factory):
    exe = host_tool(tmp_path_factory, "draws_dump",
                    flags=("-O1", "-ffp-contract=off", "-Wno-unknown-pragmas"))
    d = tmp_path_factory.mktemp("draws")
    rng = np.random.RandomState(20240611)
    inp = {}
    f = np.repeat(np.arange(1, NF // 2 + 1) / (10.0 * 365.25 * 86400.0), 2)
    inp["f"], inp["df"] = f, np.full(NF, f[0])
    inp["pl"] = np.stack([rng.uniform(-18, -11, NH), rng.uniform(0, 7, NH),
                          rng.uniform(-8.5, -5, NH)], axis=1)
    inp["fsh"] = 0.0
    head = [SEED & 0xFFFFFFFF, SEED >> 32, C, S, len(WIND), len(HIND), 0.05 * len(WIND),
            0.05 * len(HIND), NH, NF]
    pad = lambda v: list(v) + [0] * (8 - len(v))  # noqa: E731
    blob = np.concatenate([np.asarray(v, float).ravel() for v in (
        head, pad(WIND), pad(HIND), CDF, SIZE,
        [np.log(12.0) + 2.0 * np.log(np.pi), np.log(FYR), inp["fsh"]], np.log(f),
        np.log(inp["df"]), inp["pl"])])
    src, dst = d / "in.bin", d / "out.bin"
    blob.tofile(src)
    subprocess.run([str(exe), str(src), str(dst)], check=True)
    out, raw, pos = {}, dst.read_bytes(), 0
    while pos < len(raw):
        end = raw.index(b"\n", pos)
        name, _, cnt = raw[pos:end].decode().split()
        out[name] = np.frombuffer(raw, "<f8", int(cnt), end + 1)
        pos = end + 1 + 8 * int(cnt)
    return inp, out


def check(name, got, want):
    err = rel(got, want)
    print(f"{name}: max relative error {err:.3e} (bound {4 * MEASURED[name]:.1e})")
    assert err <= 4 * MEASURED[name], name


def test_mh_variates(laws):
    _, out = laws
    ch, sw = np.arange(C)[:, None, None], np.arange(S)[None, :, None]
    u = out["mh_u"].reshape(C, S, 30, 3)
    xi = out["mh_xi"].reshape(C, S, 30)
    v = out["mh_out"].reshape(C, S, 30, 4)
    # a tape row made of the same variates gives the same entries (log u from the tape's u)
    assert np.array_equal(out["mh_tape"].reshape(C, S, 30, 4), v)
    for tag, lo, nsteps, ind, sig in ((pv.TAG_WHITE, 0, 20, WIND, 0.05 * len(WIND)),
                                      (pv.TAG_HYPER, 20, 10, HIND, 0.05 * len(HIND))):
        step = np.arange(nsteps)[None, None, :]
        us, ua = pv.uniform2(SEED, ch, sw, tag | (3 * step))
        uidx, _ = pv.uniform2(SEED, ch, sw, tag | (3 * step + 2))
        sl = slice(lo, lo + nsteps)
        # the uniforms and the chosen parameter: equal
        assert np.array_equal(u[:, :, sl, 0], us) and np.array_equal(u[:, :, sl, 1], ua)
        assert np.array_equal(u[:, :, sl, 2], uidx)
        assert np.array_equal(v[:, :, sl, 0], np.asarray(ind)[pv.choice_index(uidx, len(ind))])
        # the jump given the normal, with the oracle's scale class, as numpy evaluates it (no
        # contraction): equal -- and so the scale class (the five sizes differ)
        k = pv.scale_class(us, CDF)
        assert len(np.unique(k)) == 5
        assert np.array_equal(v[:, :, sl, 1], (xi[:, :, sl] * sig) * np.asarray(SIZE)[k])
        check("normal", xi[:, :, sl], pv.normal_from(SEED, ch, sw, tag | (3 * step + 1)))
        check("log_u", v[:, :, sl, 2], np.log(ua))
        check("pow10", v[:, :, sl, 3], 10.0 ** (2.0 * v[:, :, sl, 1]))


def test_prior_side(laws):
    inp, out = laws
    lA, g, lec = inp["pl"].T
    f, df = inp["f"], inp["df"]
    # enterprise's power law, evaluated left to right (model.powerlaw)
    phi = ((10.0 ** lA[:, None]) ** 2 / 12.0 / np.pi ** 2 * FYR ** (g[:, None] - 3.0)
           * f[None, :] ** (-g[:, None]) * df[None, :])
    check("lc", out["lc"], np.log(phi[:, 0]) + g * np.log(f[0]) - np.log(df[0]))
    check("phi_inv", out["phi_inv"].reshape(NH, NF), 1.0 / phi)
    check("phi_inv_ecorr", out["phi_inv_ecorr"], 1.0 / 10.0 ** (2.0 * lec))
    ld = np.sum(np.log(phi), axis=1) + 3.0 * np.log(10.0 ** (2.0 * lec))
    check("logdet_phi", out["logdet_phi"], ld)
    # lnL's sum, the kernels' order: equal (draws_dump passes lA, g, lec, lc, log|phi| as terms)
    want = -0.5 * (lA + g) + 0.5 * (lec - out["lc"] - out["logdet_phi"])
    assert np.array_equal(out["marginal_ll"], want)
