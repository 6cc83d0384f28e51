"""gst_set_accum_toa is additive to ABI 7: the ctypes AccumToa struct has the layout of
gst_accum_toa in include/gst.h, as the system C compiler lays it out; the version stays 7
and callers find the entry point by symbol lookup."""
import ctypes as ct
import os
import shutil
import subprocess

import pytest

from gibbs_student_t_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROG = r"""
#include <stddef.h>
#include <stdio.h>
#include "gst.h"
int main(void) {
  printf("%d %zu", GST_ABI_VERSION, sizeof(gst_accum_toa));
  printf(" %zu %zu %zu %zu %zu %zu\n", offsetof(gst_accum_toa, nthr),
         offsetof(gst_accum_toa, thr), sizeof(((gst_accum_toa*)0)->thr),
         offsetof(gst_accum_toa, pout_gt), offsetof(gst_accum_toa, resid_sum),
         offsetof(gst_accum_toa, resid_sq));
  return 0;
}
"""


def test_accum_toa_struct_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(PROG)
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    fields = ("nthr", "thr", "pout_gt", "resid_sum", "resid_sq")
    assert [f for f, _ in _abi.AccumToa._fields_] == list(fields)
    A = _abi.AccumToa
    assert got == [_abi.ABI_VERSION, ct.sizeof(A), A.nthr.offset, A.thr.offset, A.thr.size,
                   A.pout_gt.offset, A.resid_sum.offset, A.resid_sq.offset]
    assert A.thr.size == 4 * ct.sizeof(ct.c_double)


def test_additive_to_abi_7():
    assert _abi.ABI_VERSION == 7
    assert "gst_set_accum_toa" in _abi.EXPORTS
    # older builds may lack it: found by symbol lookup, not by a version bump
    assert "gst_set_accum_toa" in _abi.OPTIONAL
