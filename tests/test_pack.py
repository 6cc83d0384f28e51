"""The host packer (csrc/gst_pack.h) on a CPU: a small general-white-noise dataset packed by
tools/pack_dump.cpp as the large path and as a persistent GEN shape does, compared exactly
with a numpy restatement of the layouts documented on DevModel (csrc/gst_model.h)."""
import math

import numpy as np
import pytest

from support import PACKINGS, PACK_DIMS, host_tool, pack_dataset as dataset, run_packer

N, NF, NTM, NEC, NB, P = PACK_DIMS
M = NF + NTM + NEC
NPAD, NKS = 128, 18                      # 70 TOAs: two 64-TOA slots, 18 k-steps of 4


@pytest.fixture(scope="module")
def pack_bin(tmp_path_factory):
    return host_tool(tmp_path_factory, "pack_dump")


def mfma_tiles(A):
    """[n][16 NT] -> [npad / 4][NT][64]: lane l of tile X at k-step ks holds TOA 4 ks + l / 16,
    column 16 X + l % 16"""
    NT = A.shape[1] // 16
    Ap = np.zeros((NPAD, 16 * NT))
    Ap[:N] = A
    return Ap.reshape(NPAD // 4, 4, NT, 16).transpose(0, 2, 1, 3).reshape(-1)


def expected(d, MT, ntm_pad, raug):
    T, r = d["T"], d["residuals"]
    mp = (raug + 1 + 15) // 16 * 16
    ref2int = np.concatenate([ntm_pad + np.arange(NF), np.arange(NTM), ntm_pad + NF + np.arange(NEC)])
    A = np.zeros((N, mp))                  # augmented rows, internal column order
    A[:, ref2int] = T
    A[:, raug] = r
    e = dict(ref2int=ref2int, Tmf=mfma_tiles(A))
    e["Tcol"] = np.zeros((M, NPAD))
    e["Tcol"][:, :N] = T.T
    # noise classes in order of first appearance, (sigma^2, backend) pairs
    sig2 = d["toaerrs"] * d["toaerrs"]
    classes, cidx = [], np.full(NPAD, -1)
    for t in range(N):
        key = (sig2[t], int(d["backend"][t]))
        if key not in classes:
            classes.append(key)
        cidx[t] = classes.index(key)
    ncls = len(classes) if len(classes) <= 8 else 0
    e["ncls"] = ncls
    e["cidx"] = cidx if ncls else np.zeros(0)
    e["csig2"] = np.array([c[0] for c in classes]) if ncls else np.zeros(0)
    e["ccount"] = np.bincount(cidx[:N], minlength=len(classes)).astype(float) if ncls else np.zeros(0)
    e["cls_b"] = np.array([c[1] for c in classes[:ncls]] + [0] * (8 - ncls))
    e["Trow"] = e["Gcls"] = np.zeros(0)
    if MT and ncls:
        W = 8 * MT
        i = np.arange(W)
        trow = np.zeros((NPAD, W))
        trow[:N, (i % 8) * MT + i // 8] = A[:, :W]          # [t][i % 8][i / 8]
        e["Trow"] = trow
        acc = np.zeros((ncls, W, W), np.longdouble)
        for t in range(N):                                 # TOA order, 80-bit accumulation
            row = A[t, :W].astype(np.longdouble)
            acc[cidx[t]] += np.outer(row, row)
        g = np.zeros((ncls, MT * (MT + 1) // 2, 64))
        lane = np.arange(64)
        for rr in range(MT):
            for s in range(rr + 1):                        # slot SL(r, s), lane 8 p + q
                g[:, rr * (rr + 1) // 2 + s] = acc[:, 8 * rr + lane // 8, 8 * s + lane % 8]
        e["Gcls"] = g
    ec = T[:, NF + NTM:]
    disjoint = bool(np.all((ec != 0).sum(axis=1) <= 1))
    e["disjoint"] = disjoint
    e["gx_nt"] = e["nkse"] = e["neblk"] = 0
    e["Tx"] = e["Xe"] = e["ekl"] = e["eblk"] = np.zeros(0)
    if MT == 0 and disjoint:
        Q = ntm_pad + NF                                   # X = [TM | pad | Fourier], r, ones
        NX = (Q + 2 + 15) // 16
        Xc = np.zeros((N, 16 * NX))
        Xc[:, :Q] = A[:, :Q]
        Xc[:, Q] = r
        e["Tx"] = mfma_tiles(Xc)
        ent, eblk = [], []
        for b in range((NEC + 15) // 16):                  # 16 epochs per block, whole k-steps
            eblk.append(len(ent) // 4)
            for ep in range(16 * b, min(NEC, 16 * b + 16)):
                ent += [(t, ep - 16 * b, ec[t, ep]) for t in np.flatnonzero(ec[:, ep])]
            ent += [(-1, -1, 0.0)] * (-len(ent) % 4)
        eblk.append(len(ent) // 4)
        nkse = max(16, (eblk[-1] + 15) // 16 * 16)
        ent += [(-1, -1, 0.0)] * (4 * nkse - len(ent))
        xe = np.zeros((nkse, NX, 4, 16))
        for p, (t, _, u) in enumerate(ent):
            if t >= 0:
                row = u * Xc[t]
                row[Q + 1] = u * u
                xe[p // 4, :, p % 4, :] = row.reshape(NX, 16)
        e.update(Xe=xe, ekl=np.array([(t, ep) for t, ep, _ in ent]), eblk=np.array(eblk),
                 gx_nt=NX, nkse=nkse, neblk=len(eblk) - 1)
    lp = 0.0
    for j in range(P):                                     # Python sum() order
        lp += -math.log(d["pmax"][j] - d["pmin"][j])   # libm's log, as the packer's
    e["lp_sum"] = lp
    e["ec_count"] = np.bincount(d["ecorr_backend"], minlength=8).astype(float)
    return e, mp


@pytest.mark.parametrize("packing", ["large", "gen"])
@pytest.mark.parametrize("variant", ["classes", "sigmas", "overlap"])
def test_pack(pack_bin, tmp_path, variant, packing):
    MT, ntm_pad, raug = PACKINGS[packing]
    d = dataset(variant)
    want, mp = expected(d, MT, ntm_pad, raug)
    got = run_packer(pack_bin, tmp_path, d, MT, ntm_pad, raug, int(want["disjoint"]))
    ints = dict(zip(("nks", "npad", "mp", "gx_nt", "nkse", "neblk", "ncls", "ec_disjoint", "n", "m",
                     "nf", "ntm", "ntm_pad", "raug", "nslot_toa", "nec", "nb"), got["ints"]))
    assert ints == dict(nks=NKS, npad=NPAD, mp=mp, gx_nt=want["gx_nt"], nkse=want["nkse"],
                        neblk=want["neblk"], ncls=want["ncls"], ec_disjoint=int(want["disjoint"]),
                        n=N, m=M, nf=NF, ntm=NTM, ntm_pad=ntm_pad, raug=raug, nslot_toa=2, nec=NEC,
                        nb=NB)
    # what the variants are for
    assert want["disjoint"] == (variant != "overlap")
    assert (want["ncls"] == 0) == (variant == "sigmas") and want["ncls"] <= 8
    if packing == "large":
        assert (ints["gx_nt"], ints["neblk"]) == ((2, 2) if want["disjoint"] else (0, 0))
        if want["disjoint"]:       # 18 epochs: two 16-epoch blocks, both end in -1 padding
            ekl = got["ekl"].reshape(-1, 2)
            assert all(ekl[4 * got["eblk"][b + 1] - 1, 0] == -1 for b in range(2))
    for k in ("Tmf", "Tcol", "ref2int", "cidx", "csig2", "ccount", "cls_b", "Trow", "Tx", "Xe",
              "ekl", "eblk", "lp_sum", "ec_count"):
        w = np.asarray(want[k]).reshape(-1)
        assert got[k].shape == w.shape and np.array_equal(got[k], w), k
    if np.finfo(np.longdouble).nmant == 63:    # the packer accumulates in x87 80-bit
        assert np.array_equal(got["Gcls"], want["Gcls"].reshape(-1))
    else:
        assert got["Gcls"].shape == want["Gcls"].reshape(-1).shape
    # the padding past the 70 TOAs is zero
    assert not got["Tmf"].reshape(NPAD // 4, -1, 4, 16)[NKS:].any()
    assert not got["Tmf"].reshape(NPAD // 4, -1, 4, 16)[NKS - 1, :, 2:].any()
