"""The launch planner (csrc/gst_plan.h) on a CPU: which kernels a large-path call launches, in
which order and shape, the LDS layouts' totals and the persistent kernel's launch shape.  The
expected lists are written by hand from the class rules at the head of gst_plan.h (white /
toa / hyper classes, ec_reg_mt, gram_ec_of); tools/plan_dump.cpp prints the planner's."""
import subprocess

import pytest

from support import host_tool

ALL = 0x7F
GRAM_ONLY = 0x100                      # GST_STAGE_GRAM
D_GRAM, D_HYPER, D_EXACT, D_EPOCHS = 2, 4, 8, 32   # GST_DEBUG_LARGE_GRAM, ...
GRAM_LDS = (2 * 16 * 8 * 64 + 2 * 8 * 64) * 8


@pytest.fixture(scope="module")
def plan_bin(tmp_path_factory):
    return host_tool(tmp_path_factory, "plan_dump")


def r16(a):
    return (a + 15) // 16 * 16


def ds(npad, nf, nec=0, ntm=3, disjoint=1, gx_nt=0):
    """The integers of a large-path dataset as gst_model_set_batch packs them."""
    ntm_pad = r16(max(ntm, 1))
    raug = ntm_pad + nf + nec
    return dict(npad=npad, mp=r16(raug + 1), nf=nf, nec=nec, ntm=ntm, ntm_pad=ntm_pad, raug=raug,
                disjoint=disjoint, gx_nt=gx_nt)


def run(plan_bin, *args):
    return subprocess.run([plan_bin] + [str(a) for a in args], capture_output=True, text=True,
                          check=True).stdout.strip().splitlines()


def large(plan_bin, dsets, C=64, mask=ALL, debug=0, eval_only=0, rec_on=0):
    specs = [",".join(str(d[k]) for k in ("npad", "mp", "nf", "nec", "ntm", "ntm_pad", "raug",
                                          "disjoint", "gx_nt")) for d in dsets]
    rows = []
    for line in run(plan_bin, "large", C, mask, debug, eval_only, rec_on, *specs):
        if line.startswith("error:"):
            return line
        f = line.split()
        rows.append(dict(list=f[0], kernel=f[1], kind=f[2], gx=int(f[3]), gy=int(f[4]),
                         block=int(f[5]), lds=int(f[6]), kclass=int(f[7]), floor=int(f[8]),
                         ev=int(f[9]), record=int(f[10])))
    return rows


def names(rows):
    """'list:kernel', with '*' on floor-pass launches"""
    return [f"{r['list'][0]}:{r['kernel']}{'*' if r['floor'] else ''}" for r in rows]


def full_sweep(white, gram, hyper, toa):
    """A full sweep of a batch that needs the timing-model kernels"""
    return ["p:tb", f"s:{white}", f"s:{gram}", "s:tmelim", f"s:{hyper}", "s:tmelim*",
            f"s:{hyper}*", "s:btm", "s:tb", f"s:{toa}"]


def ec_sweep(white, gram, hyper, toa):
    """... of a batch of epochs-first (class 2) datasets: no lg_tmelim, no lg_btm"""
    return ["p:tb", f"s:{white}", f"s:{gram}", f"s:{hyper}", f"s:{hyper}*", "s:tb", f"s:{toa}"]


# hyper blocks without ECORR: <= 62 columns lg_hyper_reg<8>, <= 126 lg_hyper_reg<16>, <= 138
# lg_hyper<0>, past that lg_hyper<1>.  mp = 16 + nf + 1 rounded up to 16: at most 6 tiles
# take lg_gram_small<tiles>
@pytest.mark.parametrize("nf,gram,hyper", [
    (62, "gram_small<5>", "hyper_reg<8>"), (63, "gram_small<5>", "hyper_reg<16>"),
    (126, "gram", "hyper_reg<16>"), (127, "gram", "hyper<0>"), (138, "gram", "hyper<0>"),
    (139, "gram", "hyper<1>")])
def test_hyper_kernel_by_columns(plan_bin, nf, gram, hyper):
    rows = large(plan_bin, [ds(128, nf)])
    assert names(rows) == full_sweep("white<64>", gram, hyper, "toa<256>")


# disjoint-ECORR models (nf, nec, ntm, gx_nt = tiles of ntm_pad + nf + 2 columns, debug)
MB = dict(nf=20, nec=60, ntm=3, gx_nt=3)       # 80 columns, 60 epochs >= 24 rows of X: class 2
@pytest.mark.parametrize("model,debug,gram,hyper", [
    (MB, 0, "gram_ec<3>", "hyper_ecr<6,46>"),                                    # nf <= 30
    (dict(nf=40, nec=80, ntm=3, gx_nt=4), 0, "gram_ec<4>", "hyper_ecr<8,62>"),   # nf <= 46
    (dict(nf=20, nec=60, ntm=20, gx_nt=4), 0, "gram_ec<4>", "hyper<2>"),         # ntm > 16
    (dict(nf=20, nec=200, ntm=3, gx_nt=3), 0, "gram_ec<3>", "hyper<2>"),         # > 192 epochs
    (MB, D_EPOCHS, "gram_ec<3>", "hyper<2>")])
def test_hyper_kernel_epochs_first(plan_bin, model, debug, gram, hyper):
    rows = large(plan_bin, [ds(128, **model)], debug=debug)
    assert names(rows) == ec_sweep("white<64>", gram, hyper, "toa<256>")
    assert not any(r["kernel"] in ("tmelim", "btm") for r in rows)


def test_hyper_kernel_other_ecorr(plan_bin):
    # X has 3 + 80 + 1 = 84 > 76 rows: not epochs first; 180 columns: lg_hyper<1>
    rows = large(plan_bin, [ds(128, nf=80, nec=100)])
    assert names(rows) == full_sweep("white<64>", "gram", "hyper<1>", "toa<256>")
    # a TOA in two epochs: the 80-column block goes to lg_hyper_reg<16>, mp = 112: 7 tiles
    rows = large(plan_bin, [ds(128, nf=20, nec=60, disjoint=0)])
    assert names(rows) == full_sweep("white<64>", "gram", "hyper_reg<16>", "toa<256>")


@pytest.mark.parametrize("npad,white,toa", [
    (8192, "white<64>", "toa<256>"), (8256, "white<256>", "toa<256>"),
    (32768, "white<256>", "toa<256>"), (32832, "white<1024>", "toa<1024>")])
def test_white_and_toa_classes(plan_bin, npad, white, toa):
    rows = large(plan_bin, [ds(npad, 62)])
    assert names(rows) == full_sweep(white, "gram_small<5>", "hyper_reg<8>", toa)
    w = next(r for r in rows if r["kernel"] == white)
    t = next(r for r in rows if r["kernel"] == toa)
    assert (w["kclass"], t["kclass"]) == ({"white<64>": 0, "white<256>": 1, "white<1024>": 2}[white],
                                          {"toa<256>": 0, "toa<1024>": 1}[toa])
    assert (w["gx"], w["block"]) == (64, int(white[6:-1]))
    assert (t["gx"], t["block"]) == (64, int(toa[4:-1]))
    tb = rows[0]
    assert (tb["gx"], tb["gy"], tb["block"]) == (npad // 64, 1, 256)


def test_batch_of_two_white_classes(plan_bin):
    rows = large(plan_bin, [ds(8192, 62), ds(8256, 62)], C=300)
    assert names(rows) == ["p:tb", "s:white<64>", "s:white<256>", "s:gram_small<5>", "s:tmelim",
                           "s:hyper_reg<8>", "s:tmelim*", "s:hyper_reg<8>*", "s:btm", "s:tb",
                           "s:toa<256>"]
    # lg_tb: the batch's largest npad in 64-TOA tiles x 256 chains per workgroup
    assert (rows[0]["gx"], rows[0]["gy"]) == (8256 // 64, 2)


def test_gram_kernels(plan_bin):
    # forced dense: the super-tile Gram instead of lg_gram_small / lg_gram_ec
    rows = large(plan_bin, [ds(128, 62)], debug=D_GRAM)
    assert names(rows) == full_sweep("white<64>", "gram", "hyper_reg<8>", "toa<256>")
    rows = large(plan_bin, [ds(128, **MB)], debug=D_GRAM)
    assert names(rows) == ec_sweep("white<64>", "gram", "hyper_ecr<6,46>", "toa<256>")
    # shapes, C = 100: lg_gram_small 4 chains, lg_gram_ec 2 chains per 256-thread workgroup;
    # lg_gram 8 chains per 512-thread workgroup and lower 64x64 super-tile (mp = 112: 2 rows
    # of super-tiles, 3 of them)
    g = large(plan_bin, [ds(128, 62)], C=100)[2]
    assert (g["kernel"], g["kind"], g["gx"], g["block"], g["lds"]) == ("gram_small<5>", "GRAM", 25, 256, 0)
    g = large(plan_bin, [ds(128, **MB)], C=100)[2]
    assert (g["kernel"], g["gx"], g["block"], g["lds"]) == ("gram_ec<3>", 50, 256, 0)
    g = large(plan_bin, [ds(128, **MB)], C=100, debug=D_GRAM)[2]
    assert (g["kernel"], g["gx"], g["block"], g["lds"]) == ("gram", 3 * 13, 512, GRAM_LDS)
    # both Grams in one call: one timing event pair around the two launches
    rows = large(plan_bin, [ds(128, **MB), ds(128, **dict(MB, gx_nt=0))])
    assert names(rows)[1:4] == ["s:white<64>", "s:gram_ec<3>", "s:gram"]
    assert [r["ev"] for r in rows] == [3, 3, 1, 2] + [3] * (len(rows) - 4)


def test_hyper_launch_shapes(plan_bin):
    """chains per workgroup: reg<8> 4, reg<16> 2, ecr<6,46> 4, ecr<8,62> 2; lg_hyper one chain
    per 256-thread workgroup with its layout's LDS"""
    def hyper(model, **kw):
        return next(r for r in large(plan_bin, [ds(128, **model)], C=101, **kw)
                    if r["kind"] == "HYPER")
    for model, kernel, gx, block in [
            (dict(nf=62), "hyper_reg<8>", 26, 256), (dict(nf=63), "hyper_reg<16>", 51, 128),
            (MB, "hyper_ecr<6,46>", 26, 256),
            (dict(nf=40, nec=80, gx_nt=4), "hyper_ecr<8,62>", 51, 128)]:
        h = hyper(model)
        assert (h["kernel"], h["gx"], h["gy"], h["block"], h["lds"]) == (kernel, gx, 1, block, 0)
    h = hyper(dict(nf=138))          # S [139][140], phi^-1 [138], two vectors of 139
    assert (h["kernel"], h["gx"], h["block"], h["lds"]) == ("hyper<0>", 101, 256,
                                                            8 * (139 * 140 + 138 + 2 * 139))


def test_debug_large_hyper(plan_bin):
    # every dataset on the generic kernels: class 0 up to 138 columns, the timing-model
    # kernels and the dense Gram with it
    rows = large(plan_bin, [ds(128, 62)], debug=D_HYPER)
    assert names(rows) == full_sweep("white<64>", "gram_small<5>", "hyper<0>", "toa<256>")
    rows = large(plan_bin, [ds(128, **MB)], debug=D_HYPER)
    assert names(rows) == full_sweep("white<64>", "gram", "hyper<0>", "toa<256>")
    # past 138 columns lg_hyper<1>; 1120 columns: its panel [1152][17] alone is 153 KiB
    rows = large(plan_bin, [ds(128, nf=20, nec=200, gx_nt=3)], debug=D_HYPER)
    assert names(rows) == full_sweep("white<64>", "gram", "hyper<1>", "toa<256>")
    out = large(plan_bin, [ds(128, nf=20, nec=1100, gx_nt=3)], debug=D_HYPER)
    assert out == ("error: gst: GST_DEBUG_LARGE_HYPER: this model's red-noise / ECORR block is "
                   "too large for the blocked elimination's LDS panel (lg_hyper<1>)")
    assert isinstance(large(plan_bin, [ds(128, nf=20, nec=1100, gx_nt=3)]), list)


def test_masks_and_flags(plan_bin):
    d = [ds(128, 62)]
    assert names(large(plan_bin, d, debug=D_EXACT)) == [
        "p:tb", "s:white<64>", "s:gram_small<5>", "s:tmelim", "s:hyper_reg<8>", "s:btm", "s:tb",
        "s:toa<256>"]
    assert names(large(plan_bin, d, mask=GRAM_ONLY)) == [
        "p:tb", "s:white<64>", "s:gram_small<5>", "s:tmelim"]
    assert names(large(plan_bin, d, mask=ALL & ~4)) == [
        "p:tb", "s:white<64>", "s:gram_small<5>", "s:tmelim", "s:hyper_reg<8>", "s:toa<256>"]
    assert names(large(plan_bin, d, mask=1)) == ["p:tb", "s:white<64>"]
    assert names(large(plan_bin, d, mask=0, eval_only=1)) == [
        "p:tb", "s:white<64>", "s:gram_small<5>", "s:tmelim", "s:hyper_reg<8>"]
    rows = large(plan_bin, d, rec_on=1)
    assert names(rows) == ["p:tb", "s:record"] + full_sweep("white<64>", "gram_small<5>",
                                                            "hyper_reg<8>", "toa<256>")[1:]
    assert [r["record"] for r in rows] == [0, 1] + [0] * 9
    assert [r["kind"] for r in rows] == ["TB", "RECORD", "WHITE", "GRAM", "TMELIM", "HYPER",
                                         "TMELIM", "HYPER", "BTM", "TB", "TOA"]


# (nf, nec, ntm): three models of each hyper class
@pytest.mark.parametrize("nf,nec,ntm", [(127, 0, 3), (100, 38, 12), (60, 70, 30),
                                        (139, 0, 3), (80, 100, 3), (100, 300, 40),
                                        (20, 200, 3), (30, 400, 20), (40, 150, 35)])
def test_layout_totals(plan_bin, nf, nec, ntm):
    """each layout's bytes against the closed forms gst_model_set_batch used to carry"""
    d = ds(128, nf, nec, ntm)
    mp, ms, qx = d["mp"], nf + nec + 1, ntm + nf + 1
    want = [mp * 17 * 8, (3 * d["ntm_pad"] + d["raug"]) * 8,
            (ms * (ms + 1) + nf + nec + 2 * ms) * 8,
            (mp * 17 + 16 + nf + nec + 2 * ms) * 8,
            (2 * qx * (qx + 1) + nf + nec + 4 * mp + nec + 2 * 32 * r16(qx) + 2 * 32) * 8]
    got = run(plan_bin, "lds", nf, nec, ntm, mp, d["ntm_pad"], d["raug"])[0].split()
    assert [int(v) for v in got] == want
    # ... and the planner's launches carry them
    rows = large(plan_bin, [d])
    lds = {r["kernel"]: r["lds"] for r in rows}
    for kernel, w in zip(("tmelim", "btm", "hyper<0>", "hyper<1>", "hyper<2>"), want):
        assert lds.get(kernel, w) == w


# ncu = 256, shape MT = 8, NS = 4, K0 = 2 (15 timing-model factor slots of 64 doubles), full
# mask: (C, waves) -> wpb, pair, occ2, use_prog, grid, block, tmfac bytes / (15 * 64 * 8)
PERSIST = {
    (256, 0): (1, 1, 0, 0, 256, 128, 512), (256, 1): (1, 0, 0, 0, 256, 64, 256),
    (256, 2): (1, 1, 0, 0, 256, 128, 512),
    (257, 0): (2, 1, 0, 0, 257, 128, 514), (257, 1): (2, 0, 0, 0, 129, 128, 257),
    (257, 2): (2, 1, 0, 0, 257, 128, 514),
    (512, 0): (2, 1, 0, 0, 512, 128, 1024), (512, 1): (2, 0, 0, 0, 256, 128, 512),
    (512, 2): (2, 1, 0, 0, 512, 128, 1024),
    (513, 0): (4, 0, 0, 0, 129, 256, 513), (513, 1): (4, 0, 0, 0, 129, 256, 513),
    (513, 2): (4, 1, 0, 0, 513, 128, 1026),
    (1024, 0): (4, 0, 0, 0, 256, 256, 1024), (1024, 1): (4, 0, 0, 0, 256, 256, 1024),
    (1024, 2): (4, 1, 0, 0, 1024, 128, 2048),
    (1025, 0): (4, 0, 1, 1, 257, 256, 1025), (1025, 1): (4, 0, 1, 1, 257, 256, 1025),
    (1025, 2): (4, 1, 1, 0, 1025, 128, 2050),
}


@pytest.mark.parametrize("C", [256, 257, 512, 513, 1024, 1025])
def test_persistent_plan(plan_bin, C):
    def plan(waves, tape=0, eval_only=0, mask=ALL, NS=4):
        return tuple(int(v) for v in run(plan_bin, "persist", 256, C, tape, eval_only, mask, waves,
                                         NS, 8, 2)[0].split())
    for waves in (0, 1, 2):
        w = PERSIST[(C, waves)]
        assert plan(waves) == w[:6] + (w[6] * 15 * 64 * 8,)
        # tape mode: four chains per workgroup, one wave per chain, no progress counter
        assert plan(waves, tape=1) == (4, 0, int(C > 1024), 0, (C + 3) // 4, 256, C * 15 * 64 * 8)
        # eval_only and GST_STAGE_GRAM launches run one wave per chain
        assert plan(waves, eval_only=1)[1] == 0 and plan(waves, mask=ALL | GRAM_ONLY)[1] == 0
    # no progress counter without the red-noise block; no two-chains-per-SIMD build past NS 8
    assert plan(1, mask=ALL & ~2)[3] == 0
    assert plan(1, NS=12)[2] == 0
