"""The launch planner with the posterior sums on (plan_large's acc_on, csrc/gst_plan.h): the
sweep list gains lg_accum directly after lg_record's place, one workgroup per chain, and
nothing else changes; without it the lists are the planner's usual ones."""
import subprocess

import pytest

from support import host_tool

ALL = 0x7F


@pytest.fixture(scope="module")
def plan_bin(tmp_path_factory):
    return host_tool(tmp_path_factory, "plan_dump")


def r16(a):
    return (a + 15) // 16 * 16


def spec(npad, nf, nec=0, ntm=3, gx_nt=0):
    ntm_pad = r16(max(ntm, 1))
    raug = ntm_pad + nf + nec
    return f"{npad},{r16(raug + 1)},{nf},{nec},{ntm},{ntm_pad},{raug},1,{gx_nt}"


def plan(plan_bin, mode, specs, C=100, mask=ALL, rec_on=0, eval_only=0):
    out = subprocess.run([plan_bin, mode, str(C), str(mask), "0", str(eval_only), str(rec_on)]
                         + specs, capture_output=True, text=True, check=True).stdout
    return [line.split() for line in out.strip().splitlines()]


# a classic dataset, an epochs-first one (no lg_tmelim / lg_btm), a batch of two white classes
BATCHES = [[spec(128, 62)], [spec(128, 20, 60, gx_nt=3)], [spec(8192, 62), spec(8256, 62)]]


@pytest.mark.parametrize("specs", BATCHES)
@pytest.mark.parametrize("rec_on", [0, 1])
@pytest.mark.parametrize("mask", [ALL, 1, ALL & ~4])
def test_accum_follows_the_record_position(plan_bin, specs, rec_on, mask):
    base = plan(plan_bin, "large", specs, rec_on=rec_on, mask=mask)
    acc = plan(plan_bin, "large_acc", specs, rec_on=rec_on, mask=mask)
    # prologue lg_tb, then lg_record when records are on: lg_accum directly after it
    at = 1 + rec_on
    assert acc[:at] == base[:at] and acc[at + 1:] == base[at:]
    assert base[at - 1][1] == ("record" if rec_on else "tb")
    # sweep list, kernel, kind, gx = C, gy, block, no LDS, no class, no floor pass, both
    # timing events, not tied to record_every
    assert acc[at] == ["sweep", "accum", "ACCUM", "100", "1", "256", "0", "-1", "0", "3", "0"]
    assert not any(r[1] == "accum" for r in base)


def test_gx_is_the_chain_count(plan_bin):
    for C in (1, 16, 1040):
        row = plan(plan_bin, "large_acc", BATCHES[0], C=C)[1]
        assert row[1] == "accum" and int(row[3]) == C
