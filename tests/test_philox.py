"""The on-device RNG is standard Philox4x32-10: known-answer vectors (Salmon et al. SC'11,
Random123 kat_vectors) through the same header the kernel includes."""
import subprocess

import pytest

from support import KAT, host_tool


@pytest.fixture(scope="module")
def kat_bin(tmp_path_factory):
    return host_tool(tmp_path_factory, "philox_kat", flags=("-O2",))


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(kat_bin, ctr, key, want):
    out = subprocess.run([kat_bin] + ctr.split() + key.split(), capture_output=True,
                         text=True, check=True).stdout.strip()
    assert out == want
