"""Host side of the predictor's joint covariance (no GPU): the library's three new entries and their argument checks,
which return before any device work, the workspace query, the symmetric-mode misuse cases and the refusals of the
Python layers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from gaussianprocessfundamentals_amd import _build, _native, engine
from gaussianprocessfundamentals_amd.Statistics.Predictor import PosteriorPredictor

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpk.h")
NAMES = ("gpk_predict_vt_workspace_bytes", "gpk_predict_vt", "gpk_predict_cov")
FAKE = ctypes.c_void_p(0x1000)    # non-NULL pointers that are never dereferenced: every call below fails before that
FAKE2 = ctypes.c_void_p(0x2000)


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _native.load_library()


def _kd(dim=1):
    kd = _native.GpkKdesc()
    kd.n_nodes, kd.n_hyp, kd.dim, kd.n_ard = 1, 1, dim, 0
    kd.nodes[0].op, kd.nodes[0].hyp_offset, kd.nodes[0].ard_slot, kd.nodes[0].flags = _native.OP_SE, 0, -1, 0
    return kd


def _plan(lib, n, m, dtype=_native.GPK_F64, batch=1, d=1):
    lay = _native.GpkLayout()
    assert lib.gpk_plan(dtype, batch, n, m, d, ctypes.byref(lay)) == 0
    return lay


# ------------------------------------------------------------------------------------------------ the library
def test_library_has_the_entries(lib):
    assert _native.PREDICT_COV_ENTRIES == NAMES
    assert _native.PREDICT_ENTRIES == ("gpk_predict_workspace_bytes", "gpk_predict")   # (unchanged)
    assert all(n in _native.EXPORTS for n in NAMES)
    assert all(hasattr(lib, n) for n in NAMES)
    assert _native.predict_cov_supported(lib)
    _native.require_predict_cov(lib)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
    assert lib.gpk_abi_version() == 7 and _native.GPK_ABI_VERSION == 7


def test_an_older_library_reads_as_unsupported():
    class Old:                      # has the predictor of before, not the covariance entries
        gpk_predict = None
        gpk_predict_workspace_bytes = None
    assert _native.predict_supported(Old())
    assert not _native.predict_cov_supported(Old())
    with pytest.raises(_native.NativeUnavailable, match="gpk_predict_cov"):
        _native.require_predict_cov(Old())

    class Half(Old):                # all three are needed
        gpk_predict_vt = None
        gpk_predict_vt_workspace_bytes = None
    assert not _native.predict_cov_supported(Half())


def test_workspace_bytes(lib):
    kd = _kd()
    ws = lib.gpk_predict_vt_workspace_bytes
    assert ws(ctypes.byref(kd), ctypes.byref(_plan(lib, 200, 200, _native.GPK_F32)), 64) == 0
    assert ws(ctypes.byref(kd), ctypes.byref(_plan(lib, 200, 64)), 64) == 0         # m != n
    assert ws(ctypes.byref(kd), ctypes.byref(_plan(lib, 200, 0)), 64) == 0
    assert ws(ctypes.byref(_kd(2)), ctypes.byref(_plan(lib, 200, 200)), 64) == 0    # program of another dimension
    assert ws(None, ctypes.byref(_plan(lib, 200, 200)), 64) == 0
    assert ws(ctypes.byref(kd), None, 64) == 0
    lay = _plan(lib, 200, 200)
    assert lay.n_pad >= 200
    for rows in (0, -1, 65535 * 64 + 1):
        assert ws(ctypes.byref(kd), ctypes.byref(lay), rows) == 0
        assert lib.gpk_predict_workspace_bytes(ctypes.byref(kd), ctypes.byref(lay), rows) == 0   # the same conditions
    for rows in (1, 2, 63, 64, 65, 200, 4096, 100000, 65535 * 64):
        assert ws(ctypes.byref(kd), ctypes.byref(lay), rows) == 8 * rows * lay.n_pad              # the documented count


# ------------------------------------------------------------------------------------------- gpk_predict_vt
@pytest.mark.parametrize("what,code,word", [
    ("W", -5, "W"), ("Xs", -7, "Xs"), ("m0", -8, "m"), ("m-", -8, "m"), ("Vt", -9, "Vt"), ("ldv", -10, "ldv"),
    ("member-", -6, "member"), ("member+", -6, "member"), ("work", -11, "work"), ("short", -11, "work"),
    ("hyp", -3, "hyp_dev"), ("X", -4, "X"), ("kd", -1, "kernel descriptor"), ("f32", -2, "fp64 only"),
    ("m!=n", -2, "m = n"), ("lay", -2, "layout"),
])
def test_vt_bad_arguments_return_before_any_device_work(lib, what, code, word):
    kd = _kd(2) if what == "kd" else _kd()
    lay = _plan(lib, 200, 64 if what == "m!=n" else 200, _native.GPK_F32 if what == "f32" else _native.GPK_F64, batch=3)
    need = lib.gpk_predict_vt_workspace_bytes(ctypes.byref(_kd()), ctypes.byref(_plan(lib, 200, 200)), 64)
    a = dict(hyp=FAKE, X=FAKE, W=FAKE, member=1, Xs=FAKE, m=500, Vt=FAKE, ldv=200, work=FAKE, bytes=need)
    if what in ("W", "Xs", "work", "hyp", "X", "Vt"):
        a[what] = None
    elif what == "m0":
        a["m"] = 0
    elif what == "m-":
        a["m"] = -4
    elif what == "ldv":
        a["ldv"] = 199            # one short of n
    elif what == "member-":
        a["member"] = -1
    elif what == "member+":
        a["member"] = 3
    elif what == "short":
        a["bytes"] = need - 8     # one double short of a tile of 64 rows
    got = lib.gpk_predict_vt(ctypes.byref(kd), None if what == "lay" else ctypes.byref(lay), a["hyp"], a["X"], a["W"],
                             a["member"], a["Xs"], a["m"], a["Vt"], a["ldv"], a["work"], a["bytes"], None)
    assert got == code
    assert word in lib.gpk_last_error().decode()


def test_vt_fewer_points_than_a_tile_need_only_their_own_rows(lib):
    kd, lay = _kd(), _plan(lib, 200, 200)
    ws = lib.gpk_predict_vt_workspace_bytes
    five, tile = ws(ctypes.byref(kd), ctypes.byref(lay), 5), ws(ctypes.byref(kd), ctypes.byref(lay), 64)
    assert 0 < five < tile
    got = lib.gpk_predict_vt(ctypes.byref(kd), ctypes.byref(lay), FAKE, FAKE, FAKE, 0, FAKE, 5, FAKE, 200, FAKE,
                             five - 8, None)
    assert got == -11


# ------------------------------------------------------------------------------------------ gpk_predict_cov
def _cov_args(**over):
    a = dict(kd=_kd(), d=1, hyp=FAKE, Xa=FAKE, ma=100, Va=FAKE, lda=256, Xb=FAKE2, mb=70, Vb=FAKE2, ldb=200, n=200,
             C=FAKE, ldc=70, symmetric=0)
    a.update(over)
    return a


def _cov(lib, a):
    return lib.gpk_predict_cov(ctypes.byref(a["kd"]) if a["kd"] is not None else None, a["d"], a["hyp"], a["Xa"],
                               a["ma"], a["Va"], a["lda"], a["Xb"], a["mb"], a["Vb"], a["ldb"], a["n"], a["C"],
                               a["ldc"], a["symmetric"], None)


@pytest.mark.parametrize("over,code", [
    (dict(kd=None), -1), (dict(kd=_kd(2)), -1), (dict(d=0), -2), (dict(d=17), -2), (dict(hyp=None), -3),
    (dict(Xa=None), -4), (dict(ma=0), -5), (dict(ma=-3), -5), (dict(ma=65535 * 64 + 1), -5), (dict(Va=None), -6),
    (dict(lda=199), -7), (dict(Xb=None), -8), (dict(mb=0), -9), (dict(mb=65535 * 64 + 1, ldc=65535 * 64 + 1), -9),
    (dict(Vb=None), -10), (dict(ldb=199), -11), (dict(n=0), -12), (dict(n=-1), -12), (dict(C=None), -13),
    (dict(ldc=69), -14), (dict(symmetric=2), -15), (dict(symmetric=-1), -15),
])
def test_cov_bad_arguments_return_before_any_device_work(lib, over, code):
    assert _cov(lib, _cov_args(**over)) == code
    assert "invalid argument" in lib.gpk_last_error().decode()


@pytest.mark.parametrize("over,code", [
    (dict(Xb=FAKE2), -8),            # other points
    (dict(mb=99, ldc=100), -9),      # another count
    (dict(Vb=FAKE2), -10),           # other rows of V'
    (dict(ldb=257), -11),            # the same rows under another stride
    (dict(ma=5793 * 64, mb=5793 * 64, ldc=5793 * 64), -5),   # more lower tiles than one launch enumerates
])
def test_cov_symmetric_mode_takes_one_set_of_points_only(lib, over, code):
    sym = dict(Xa=FAKE, Xb=FAKE, Va=FAKE, Vb=FAKE, ma=100, mb=100, lda=256, ldb=256, ldc=100, symmetric=1)
    sym.update(over)
    assert _cov(lib, _cov_args(**sym)) == code
    assert "symmetric" in lib.gpk_last_error().decode()


# ------------------------------------------------------------------------------------------------- refusals
def _bare_predictor(d=1):
    p = PosteriorPredictor.__new__(PosteriorPredictor)   # (no device: the refusals come before anything needs one)
    p.d = d
    return p


def test_include_noise_with_other_points_refuses():
    with pytest.raises(ValueError, match="include_noise .* not with x_other"):
        _bare_predictor().covariance(np.zeros((3, 1)), np.zeros((2, 1)), include_noise=True)


@pytest.mark.parametrize("shape", [(4, 2), (3,), (2, 3), (3, 2, 1)])
def test_a_wrong_z_shape_refuses(shape):
    with pytest.raises(ValueError, match=r"z must be \[3, 2\]"):
        _bare_predictor().sample(np.zeros((3, 1)), 2, z=torch.zeros(shape, dtype=torch.float64))
    with pytest.raises(ValueError, match="n_draws"):
        _bare_predictor().sample(np.zeros((3, 1)), 0)


def _bare_factorization(lib, code):
    f = engine.InverseFactorization.__new__(engine.InverseFactorization)   # (no device)
    f.code, f.L, f.done, f._loo_operands, f.batch = code, lib, False, None, 1
    return f


def test_run_not_called_refuses(lib):
    f = _bare_factorization(lib, _native.GPK_F64)
    with pytest.raises(RuntimeError, match=r"run\(\.\.\.\) first"):
        f.predict_vt(torch.zeros(3, 1))
    with pytest.raises(RuntimeError, match=r"run\(\.\.\.\) first"):
        f.predict_cov(torch.zeros(3, 1))


def test_fp32_refuses(lib):
    f = _bare_factorization(lib, _native.GPK_F32)
    with pytest.raises(NotImplementedError, match="prediction is fp64 only"):
        f.predict_vt(torch.zeros(3, 1))
    with pytest.raises(NotImplementedError, match="prediction is fp64 only"):
        f.predict_cov(torch.zeros(3, 1), torch.zeros(2, 1))


def test_an_older_library_refuses_by_name():
    class Old:
        gpk_predict = None
    f = _bare_factorization(Old(), _native.GPK_F64)
    with pytest.raises(_native.NativeUnavailable, match="gpk_predict_vt"):
        f.predict_vt(torch.zeros(3, 1))
