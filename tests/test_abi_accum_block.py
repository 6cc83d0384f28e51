"""gst_set_accum_block is additive to ABI 7: the ctypes AccumBlock struct has the layout of
gst_accum_block in include/gst.h, as the system C compiler lays it out (the header compiles as
bare C); the version stays 7 and callers find the entry point by symbol lookup."""
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
  printf("%d %d %zu", GST_ABI_VERSION, GST_BLOCK_MAX, sizeof(gst_accum_block));
  printf(" %zu %zu %zu\n", offsetof(gst_accum_block, col0), offsetof(gst_accum_block, ncol),
         offsetof(gst_accum_block, bb));
  return 0;
}
"""


def test_accum_block_struct_layout(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(PROG)
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert [f for f, _ in _abi.AccumBlock._fields_] == ["col0", "ncol", "bb"]
    A = _abi.AccumBlock
    assert got == [_abi.ABI_VERSION, _abi.BLOCK_MAX, ct.sizeof(A), A.col0.offset, A.ncol.offset,
                   A.bb.offset]
    assert _abi.BLOCK_MAX == 256


def test_additive_to_abi_7():
    assert _abi.ABI_VERSION == 7
    assert "gst_set_accum_block" in _abi.EXPORTS
    # older builds may lack it: found by symbol lookup, not by a version bump
    assert "gst_set_accum_block" in _abi.OPTIONAL
    # the neighbouring structs keep their layout
    assert [f for f, _ in _abi.Accum._fields_] == ["z_sum", "pout_sum", "alpha_sum", "b_sum",
                                                   "b_sq", "count", "from_sweep"]
    assert [f for f, _ in _abi.AccumToa._fields_] == ["nthr", "thr", "pout_gt", "resid_sum",
                                                      "resid_sq"]


@pytest.mark.skipif(not os.path.exists(_abi.LIB_PATH), reason="libgst.so not built")
def test_symbol_is_exported():
    lib = _abi.load()
    assert lib.gst_version() == 7
    assert hasattr(lib, "gst_set_accum_block")
    assert lib.gst_set_accum_block.restype is ct.c_int
    # a null context is an error with a message, not a crash
    assert lib.gst_set_accum_block(None, None) < 0
    assert "gst_set_accum_block" in _abi.last_error(lib)
