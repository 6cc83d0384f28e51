"""ABI 7: the ctypes Accum struct has the layout of gst_accum in include/gst.h, as the
system C compiler lays it out."""
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
  printf("%d %zu", GST_ABI_VERSION, sizeof(gst_accum));
  printf(" %zu %zu %zu %zu %zu %zu %zu\n", offsetof(gst_accum, z_sum),
         offsetof(gst_accum, pout_sum), offsetof(gst_accum, alpha_sum),
         offsetof(gst_accum, b_sum), offsetof(gst_accum, b_sq), offsetof(gst_accum, count),
         offsetof(gst_accum, from_sweep));
  return 0;
}
"""


def test_accum_struct_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(PROG)
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    fields = ("z_sum", "pout_sum", "alpha_sum", "b_sum", "b_sq", "count", "from_sweep")
    assert [f for f, _ in _abi.Accum._fields_] == list(fields)
    assert got == [_abi.ABI_VERSION, ct.sizeof(_abi.Accum)] + \
        [getattr(_abi.Accum, f).offset for f in fields]
    assert _abi.ABI_VERSION == 7 and "gst_set_accum" in _abi.EXPORTS
    assert _abi.KERNEL_KINDS[8] == "accum"
