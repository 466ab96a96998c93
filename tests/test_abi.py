"""The C-ABI library loads and exports every function include/gpk.h declares (no GPU needed);
gpk_plan (host-only) sizes the augmented layout."""
import ctypes
import os
import re

import pytest

from gaussianprocessfundamentals_amd import _build, _native

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpk.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gpk_[a-z0-9_]+)\s*\(", src)))


def table_knobs():
    """(gpk_tune key, environment name) of every row of the knob table (GPK_KNOBS, csrc/gpk_tune.h): K(field, default)
    or, where the names do not follow the rule, KN(field, default, "key", "ENVIRONMENT_NAME")."""
    src = open(os.path.join(_build.CSRC, "gpk_tune.h")).read()
    src = src[src.index("#define GPK_KNOBS("):src.index("namespace gpk")]
    rows = [(f, "GPK_" + f.upper()) for f in re.findall(r"^\s*K\((\w+), -?\d+\)", src, flags=re.M)]
    rows += re.findall(r'^\s*KN\(\w+, -?\d+, "(\w+)", "(\w+)"\)', src, flags=re.M)
    return rows


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _native.load_library()


def test_every_declared_symbol_is_exported(lib):
    decl = declared_functions()
    assert len(decl) >= 10
    missing = [f for f in decl if not hasattr(lib, f)]
    assert not missing, missing
    assert sorted(_native.EXPORTS) == decl


def test_abi_version(lib):
    assert lib.gpk_abi_version() == _native.GPK_ABI_VERSION


@pytest.mark.parametrize("n,m,batch", [(1, 0, 1), (128, 0, 1), (129, 0, 2), (8192, 0, 1), (4096, 512, 1), (300, 77, 3)])
def test_plan_layout(lib, n, m, batch):
    lay = _native.plan(_native.GPK_F64, batch, n, m, 2)
    nb = lay.nb
    assert lay.n_pad % nb == 0 and lay.n_pad >= n and lay.n_pad - n < nb
    assert lay.y_row == lay.n_pad + m
    assert lay.p % nb == 0 and lay.p > lay.y_row
    assert lay.ld >= lay.p
    assert lay.w_bytes == batch * lay.p * lay.ld * 8
    assert lay.inv_bytes == batch * (lay.n_pad // nb) * nb * nb * 8


def test_plan_rejects_bad_arguments(lib):
    lay = _native.GpkLayout()
    assert lib.gpk_plan(7, 1, 10, 0, 1, ctypes.byref(lay)) < 0
    assert lib.gpk_plan(0, 0, 10, 0, 1, ctypes.byref(lay)) < 0
    assert lib.gpk_plan(0, 1, 0, 0, 1, ctypes.byref(lay)) < 0
    assert lib.gpk_plan(0, 1, 10, 0, 17, ctypes.byref(lay)) < 0
    assert b"invalid argument" in lib.gpk_last_error()


def test_struct_sizes_match_header(lib):
    # gpk_node: 4 x int32; gpk_kdesc: 4 x int32 + 16 nodes; gpk_layout: 2 x int32 + 10 x int64 + 2 size_t
    assert ctypes.sizeof(_native.GpkNode) == 16
    assert ctypes.sizeof(_native.GpkKdesc) == 16 + 16 * 16
    assert ctypes.sizeof(_native.GpkLayout) == 8 + 10 * 8 + 2 * 8
    # one step of gpk_launch_plan: GPK_LAUNCH_STEP_WORDS 8-byte words, the int64 fields and the two doubles
    words = int(re.search(r"#define GPK_LAUNCH_STEP_WORDS (\d+)", open(HEADER).read()).group(1))
    assert words == _native.LAUNCH_STEP_WORDS == len(_native.LAUNCH_STEP_FIELDS) + 2
    steps = _native.launch_plan(_native.plan(_native.GPK_F64, 1, 300, 77, 2))
    assert steps.dtype.itemsize == 8 * words and steps.dtype.names[-2:] == ("flops", "bytes")
    assert len(steps) > 0 and set(steps["kind"]) <= set(range(len(_native.LAUNCH_KINDS)))


def test_product_fails_loudly_without_gpu(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_native.NativeUnavailable):
        _native.lib()


def test_tune_keys_and_scheduling_defaults(lib):
    """Every knob include/gpk.h documents is accepted (host-only call), the defaults are the measured
    policy (auto look-ahead from 64 blocks, fused panel solve with the look-ahead off, up to 256
    workgroups), and an unknown key is rejected."""
    src = re.sub(r"\s+", " ", open(HEADER).read())
    doc = src[src.index("Scheduling knobs"):src.index("int gpk_tune(")]
    keys = sorted(set(re.findall(r'"([a-z0-9_]+)"', doc)))
    assert {"lookahead", "la_min_blocks", "fuse_trsm", "fuse_trsm_max", "panel_stream", "group"} <= set(keys)
    for k in keys:
        old = _native.tune(k, 0)
        assert _native.tune(k, old) == 0
    import subprocess
    import sys
    # defaults in a fresh process (environment overrides cleared)
    env = {k: v for k, v in os.environ.items() if not k.startswith("GPK_")}
    code = ("from gaussianprocessfundamentals_amd import _native as n\n"
            "print([n.tune(k, 0) for k in ('lookahead', 'la_min_blocks', 'fuse_trsm', 'fuse_trsm_max', "
            "'panel_stream')])")  # returns the default each knob held
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True,
                         cwd=os.path.dirname(HEADER) + "/..")
    assert out.stdout.strip().splitlines()[-1] == "[2, 64, 1, 256, 0]"
    with pytest.raises(Exception):
        _native.tune("no_such_knob", 1)


def test_thread_tune_is_per_thread(lib):
    """gpk_tune_thread pins a knob for the calling thread only (host-only calls): another thread still sees
    the global value, and leaving the context restores the thread's previous state."""
    import ctypes
    import threading

    def probe():
        ov, os_ = ctypes.c_int64(0), ctypes.c_int32(0)
        _native.check(lib.gpk_tune_thread(b"chain", 123, 1, ctypes.byref(ov), ctypes.byref(os_)), "probe")
        _native.check(lib.gpk_tune_thread(b"chain", ov.value, os_.value, None, None), "probe")  # restore
        return int(ov.value), int(os_.value)

    glob = _native.tune("chain", 1)
    _native.tune("chain", glob)
    with _native.thread_tune(chain=0, lookahead=0):
        assert probe() == (0, 1)        # this thread: overridden
        seen = []
        t = threading.Thread(target=lambda: seen.append(probe()))
        t.start()
        t.join()
        assert seen == [(glob, 0)]      # another thread: the global value, no override
        with _native.thread_tune(chain=2):
            assert probe() == (2, 1)
        assert probe() == (0, 1)        # nested context restored
    assert probe() == (glob, 0)
    assert _native.chain_stats()["launches"] == 0
    with pytest.raises(Exception):
        with _native.thread_tune(no_such_knob=1):
            pass


def test_knob_defaults_land_in_their_fields(lib):
    """Every knob reads back its default -- restated here, not read from the table (gpk_tune.h), so a row that
    lands in another field or loses its value shows."""
    import os
    expect = {"chain": 1, "chain_max_p": 12416, "chain_grid": 0, "chain_timeout_ms": 1000, "chain_group": 0,
              "chain_max_batch": 8, "chain_batch_max_rows": 17500, "chain_uq": 1, "group": 8, "lookahead": 2,
              "fuse_kbuild": 1, "diag_version": 2, "chain_group_corner": 16, "chain_corner_tail": 8,
              "chain_group_la": 2, "asm_f32_fast": 1, "chain_group_eye": 8, "chain_xcd": 0, "chain_xcd_seats": 16,
              "asm_f32_chunk": 4, "chain_f32": 1, "chain_group_near": 2, "chain_u128": 2, "chain_near_la": 1, "chain_s128": 2,
              # the other 24
              "upd_t128_min": 512, "trsm_t128_min": 256, "diag_debug": 0, "la_min_blocks": 64, "fuse_trsm": 1,
              "fuse_trsm_max": 256, "reserve_cus": 32, "group_first": 8, "upd_band": 0, "skip_zero_rows": 1,
              "syevj_abs_tol_e3": 0, "ingroup": 0, "rl_max_tiles": 256, "band_skip": 1, "group_eye": 4,
              "asm_generic": 0, "panel_stream": 0, "trd_split_m": 1024, "chain_eye": 1,
              "chain_max_p_eye": 16640, "asm_feat": 1, "chain_min_p": 768, "chain_min_p_eye": 3072, "cp_skip": 1}
    assert len(expect) == 49 and sorted(expect) == sorted(k for k, _ in table_knobs())
    for k, v in expect.items():
        if os.environ.get("GPK_" + k.upper()):
            continue
        old = _native.tune(k, v)
        assert old == v, (k, old)


def test_environment_names_regular_and_irregular(lib):
    """The environment initialises the knobs under "GPK_" + the key in upper case, and under the name its row
    states where that differs (diag_dbg: "diag_debug", GPK_DIAG_DEBUG): both read back in a fresh process."""
    import subprocess
    import sys
    assert dict(table_knobs())["chain_group"] == "GPK_CHAIN_GROUP"
    assert dict(table_knobs())["diag_debug"] == "GPK_DIAG_DEBUG"
    env = {k: v for k, v in os.environ.items() if not k.startswith("GPK_")}
    env.update(GPK_CHAIN_GROUP="3", GPK_DIAG_DEBUG="5")
    code = ("from gaussianprocessfundamentals_amd import _native as n\n"
            "print([n.tune(k, 0) for k in ('chain_group', 'diag_debug', 'chain_group_eye')])")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True,
                         cwd=os.path.dirname(HEADER) + "/..")
    assert out.stdout.strip().splitlines()[-1] == "[3, 5, 8]"


def test_every_table_key_is_accepted_and_documented(lib):
    """The table's keys are exactly the keys gpk.h documents, bar "chain_force_timeout" (no Tune field: the entry
    point's own), and gpk_tune and gpk_tune_thread accept every one of them."""
    src = re.sub(r"\s+", " ", open(HEADER).read())
    doc = src[src.index("Scheduling knobs"):src.index("int gpk_tune(")]
    documented = set(re.findall(r'"([a-z0-9_]+)"', doc))
    keys = [k for k, _ in table_knobs()]
    assert len(keys) == len(set(keys)) == 49
    assert documented - set(keys) == {"chain_force_timeout"}
    assert set(keys) - documented == set()
    for k in keys:
        old = _native.tune(k, 0)
        assert _native.tune(k, old) == 0
        with _native.thread_tune(**{k: 1}):
            pass
