"""The chain planner is host-only code, and the library runs that very code (no GPU).

tests/native/chain_plan_main.cpp, gpk_tune.cpp and gpk_chain_plan.cpp are compiled here with the system C++ compiler
-- plain -std=c++17, no HIP include path, so a HIP header in either unit fails the build -- and the program's digest
of every plan (1 .. 33 diagonal blocks, grids of 1 .. 256 workgroups; plain, identity-augmented and f32 plans; the
knobs at their defaults) must equal the digest of the list libgpk.so's gpk_chain_plan_ex returns for the same shape.
"""
import os
import shutil
import subprocess
import zlib

import pytest

from gaussianprocessfundamentals_amd import _build, _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "native", "chain_plan_main.cpp")
NB = 128
BLOCKS = (1, 2, 3, 5, 9, 17, 33)
GRIDS = (1, 7, 64, 256)
KINDS = ("plain", "eye", "f32")


def test_standalone_planner_matches_the_library(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    _build.build()
    exe = str(tmp_path / "chain_plan_main")
    units = [MAIN] + [os.path.join(_build.CSRC, s) for s in ("gpk_tune.cpp", "gpk_chain_plan.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + _build.CSRC] + units + ["-o", exe], check=True)
    # (the program inherits this process's environment, so a GPK_* override reaches both planners alike)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {tuple(ln.split()[:3]): tuple(ln.split()[3:]) for ln in out.splitlines()}
    assert len(got) == len(KINDS) * len(BLOCKS) * len(GRIDS)
    bad = {}
    for kind in KINDS:
        for nblk in BLOCKS:
            for grid in GRIDS:
                n_pad = nblk * NB
                t = nat.chain_plan(n_pad, 2 * n_pad if kind == "eye" else n_pad, grid, eye=kind == "eye",
                                   f32=kind == "f32")
                exp = (str(len(t)), "%08x" % zlib.crc32(t.tobytes()))
                if got[(kind, str(nblk), str(grid))] != exp:
                    bad[(kind, nblk, grid)] = (got[(kind, str(nblk), str(grid))], exp)
    assert not bad, bad
