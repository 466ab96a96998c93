"""The launch path's schedule is host-only code, and the library runs that very code (no GPU).

tests/native/launch_plan_main.cpp, gpk_tune.cpp and gpk_launch_plan.cpp are compiled here with the system C++ compiler
-- plain -std=c++17, no HIP include path, so a HIP header in either unit fails the build -- and the program's digest
of every plan (1 .. 65 diagonal blocks -- 65 crosses la_min_blocks --, m = 0 and 77, batches of 1 and 32 -- both sides of
rl_max_tiles, upd_t128_min and trsm_t128_min --; plain, identity-augmented and f32; with and without the fused K build;
the knobs at their defaults) must equal the digest of the steps libgpk.so's gpk_launch_plan returns for the same shape.
"""
import os
import shutil
import subprocess
import zlib

import pytest

from gaussianprocessfundamentals_amd import _build, _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "native", "launch_plan_main.cpp")
NB = 128
BLOCKS = (1, 2, 3, 5, 9, 17, 65)


def cases():
    for kind in ("plain", "eye", "f32"):
        for nblk in BLOCKS:
            for m in (0, 77):
                for batch in (1, 32):
                    for kbuild in (0, 1):
                        if (kind == "eye" and m) or (kbuild and (kind != "plain" or m)):
                            continue
                        yield kind, nblk, m, batch, kbuild


def test_standalone_schedule_matches_the_library(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no system C++ compiler")
    _build.build()
    exe = str(tmp_path / "launch_plan_main")
    units = [MAIN] + [os.path.join(_build.CSRC, s) for s in ("gpk_tune.cpp", "gpk_launch_plan.cpp")]
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + _build.CSRC] + units + ["-o", exe], check=True)
    # (the program inherits this process's environment, so a GPK_* override reaches both alike)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {tuple(ln.split()[:5]): tuple(ln.split()[5:]) for ln in out.splitlines()}
    want = list(cases())
    assert len(got) == len(want) == 7 * (4 + 2 + 2 + 4)
    bad = {}
    for kind, nblk, m, batch, kbuild in want:
        n = nblk * NB
        lay = nat.plan(nat.GPK_F32 if kind == "f32" else nat.GPK_F64, batch, n, n if kind == "eye" else m, 1)
        t = nat.launch_plan(lay, eye=kind == "eye", counters=True, kbuild=bool(kbuild))
        exp = (str(len(t)), "%08x" % zlib.crc32(t.tobytes()))
        key = (kind, str(nblk), str(m), str(batch), str(kbuild))
        if got[key] != exp:
            bad[key] = (got[key], exp)
    assert not bad, bad
