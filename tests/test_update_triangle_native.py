"""The wave -> block deal of the triangle update kernel (gpk_tri_map.h) covers its 44 blocks exactly once (no GPU).

tests/native/tri_map_main.cpp is compiled here with the system C++ compiler -- plain -std=c++17, no HIP include path,
so a HIP header in gpk_tri_map.h fails the build -- and checks the table update_tri_kernel unrolls over: each of the
36 blocks on or below the diagonal of a 128 x 128 tile and each of the 8 blocks of the y row's 16-row block has exactly
one owner, no wave has more than 6 blocks, and no pair of waves that share a SIMD (w, w + 4) has more than 11.
"""
import os
import shutil
import subprocess

import pytest

from gaussianprocessfundamentals_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "native", "tri_map_main.cpp")


def test_every_block_has_one_owner_and_the_simds_are_level(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    exe = str(tmp_path / "tri_map_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I" + _build.CSRC, MAIN, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout
    assert res.stdout.split() == ["ok", "44", "6", "11"]
