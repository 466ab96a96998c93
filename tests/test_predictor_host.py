"""Host side of the fitted predictor (no GPU): the library's two new entries and their argument checks, which return
before any device work, the workspace query, and the refusals of the Python layers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gaussianprocessfundamentals_amd.global_parameters as gp
from gaussianprocessfundamentals_amd import _build, _native, engine
from gaussianprocessfundamentals_amd.DataHandling.DataInput import BatchDataInput, DataInput
from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops
from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
from gaussianprocessfundamentals_amd.Optimizer import Fitter as fit
from gaussianprocessfundamentals_amd.Optimizer.FitterType import FitterType
from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import (BlockwiseGaussianProcess, GaussianProcess,
                                                                        PartitionedGaussianProcess)
from gaussianprocessfundamentals_amd.Statistics.Predictor import PosteriorPredictor

NONE, CHOL = mht.MatrixApproximations.NONE, mht.NumericalMatrixHandlingType.CHOLESKY_BASED
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gpk.h")
NAMES = ("gpk_predict_workspace_bytes", "gpk_predict")
FAKE = ctypes.c_void_p(0x1000)   # a non-NULL pointer that is never dereferenced: every call below fails before that


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
    assert _native.PREDICT_ENTRIES == NAMES
    assert all(n in _native.EXPORTS for n in NAMES)
    assert _native.predict_supported(lib)
    _native.require_predict(lib)
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), n
    assert lib.gpk_abi_version() == 7 and _native.GPK_ABI_VERSION == 7


def test_an_older_library_reads_as_unsupported():
    class Old:
        gpk_predict = None
    assert not _native.predict_supported(Old())
    with pytest.raises(_native.NativeUnavailable, match="gpk_predict"):
        _native.require_predict(Old())


def test_workspace_bytes(lib):
    kd = _kd()
    ws = lib.gpk_predict_workspace_bytes
    assert ws(ctypes.byref(kd), ctypes.byref(_plan(lib, 200, 200, _native.GPK_F32)), 64) == 0
    assert ws(ctypes.byref(kd), ctypes.byref(_plan(lib, 200, 64)), 64) == 0         # m != n
    assert ws(ctypes.byref(kd), ctypes.byref(_plan(lib, 200, 0)), 64) == 0
    assert ws(ctypes.byref(_kd(2)), ctypes.byref(_plan(lib, 200, 200)), 64) == 0    # program of another dimension
    lay = _plan(lib, 200, 200)
    assert ws(ctypes.byref(kd), ctypes.byref(lay), 0) == 0
    prev = 0
    for rows in (1, 2, 63, 64, 65, 200, 4096, 100000):
        b = ws(ctypes.byref(kd), ctypes.byref(lay), rows)
        assert b == 8 * rows * (lay.n_pad + 1 + (200 + 63) // 64)                   # the documented count
        assert b > 0 and b >= prev
        prev = b


@pytest.mark.parametrize("what,code,word", [
    ("W", -5, "W"), ("Xs", -7, "Xs"), ("m0", -8, "m"), ("m-", -8, "m"), ("outputs", -9, "mu and var"),
    ("member-", -6, "member"), ("member+", -6, "member"), ("work", -11, "work"), ("short", -11, "work"),
    ("hyp", -3, "hyp_dev"), ("X", -4, "X"), ("kd", -1, "kernel descriptor"), ("f32", -2, "fp64 only"),
    ("m!=n", -2, "m = n"),
])
def test_bad_arguments_return_before_any_device_work(lib, what, code, word):
    kd = _kd(2) if what == "kd" else _kd()
    lay = _plan(lib, 200, 64 if what == "m!=n" else 200, _native.GPK_F32 if what == "f32" else _native.GPK_F64, batch=3)
    need = lib.gpk_predict_workspace_bytes(ctypes.byref(_kd()), ctypes.byref(_plan(lib, 200, 200)), 64)
    a = dict(hyp=FAKE, X=FAKE, W=FAKE, member=1, Xs=FAKE, m=500, mu=FAKE, var=FAKE, work=FAKE, bytes=need)
    if what in ("W", "Xs", "work", "hyp", "X"):
        a[what] = None
    elif what == "m0":
        a["m"] = 0
    elif what == "m-":
        a["m"] = -4
    elif what == "outputs":
        a["mu"] = a["var"] = None
    elif what == "member-":
        a["member"] = -1
    elif what == "member+":
        a["member"] = 3
    elif what == "short":
        a["bytes"] = need - 8     # one double short of a tile of 64 rows
    got = lib.gpk_predict(ctypes.byref(kd), ctypes.byref(lay), a["hyp"], a["X"], a["W"], a["member"], a["Xs"], a["m"],
                          a["mu"], a["var"], a["work"], a["bytes"], None)
    assert got == code
    assert word in lib.gpk_last_error().decode()


def test_fewer_points_than_a_tile_need_only_their_own_rows(lib):
    """m = 5: the workspace of 5 rows is enough to pass the size check (the call then fails on the next thing wrong --
    here nothing is, so it is not made: the sizes alone are compared)."""
    kd, lay = _kd(), _plan(lib, 200, 200)
    ws = lib.gpk_predict_workspace_bytes
    five, tile = ws(ctypes.byref(kd), ctypes.byref(lay), 5), ws(ctypes.byref(kd), ctypes.byref(lay), 64)
    assert 0 < five < tile
    got = lib.gpk_predict(ctypes.byref(kd), ctypes.byref(lay), FAKE, FAKE, FAKE, 0, FAKE, 5, FAKE, None, FAKE,
                          five - 8, None)
    assert got == -11


# ------------------------------------------------------------------------------------------------- refusals
def _problem(n=24):
    x = np.linspace(0.0, 1.0, n).reshape(-1, 1)
    di = DataInput(x, np.sin(6 * x), x, np.sin(6 * x))
    di.set_mean_function(ZeroMeanFunction(1))
    return di, GaussianProcess(bk.SquaredExponentialKernel(1), ZeroMeanFunction(1))


def _batch_input():
    x = np.linspace(0, 1, 16).reshape(2, 8, 1)
    return BatchDataInput(x, np.sin(x), None, None, test_ratio=0)


def _make(cls, di, g, metric):
    return cls(di, g, metric, FitterType.GRADIENT, False, NONE, CHOL)


@pytest.mark.parametrize("cls", [BlockwiseGaussianProcess, PartitionedGaussianProcess])
def test_segmented_gps_refuse(cls):
    kids = [bk.SquaredExponentialKernel(1), bk.SquaredExponentialKernel(1)]
    # (the constructors read the operator's child_nodes only)
    g = cls(ops.ChangePointOperator(1, kids, [torch.tensor(0.5, dtype=torch.float64)]), ZeroMeanFunction(1))
    with pytest.raises(NotImplementedError, match="%s.get_predictor: segmented" % cls.__name__):
        g.get_predictor()


def test_batch_data_input_refuses():
    _, g = _problem()
    g.set_data_input(_batch_input())
    with pytest.raises(NotImplementedError, match="GaussianProcess.get_predictor: BatchDataInput"):
        g.get_predictor()
    with pytest.raises(NotImplementedError, match="PosteriorPredictor: BatchDataInput"):
        PosteriorPredictor(g.kernel, [torch.tensor(0.3)], 0.05, ZeroMeanFunction(1), None, _batch_input())


def test_a_gp_without_data_asks_for_it():
    _, g = _problem()
    with pytest.raises(RuntimeError, match="set_data_input"):
        g.get_predictor()


@pytest.mark.parametrize("name", ["DeviceKfoldLbfgsFitter", "DeviceKfoldMseLbfgsFitter"])
def test_kfold_fitters_refuse(name):
    di, g = _problem()
    f = _make(getattr(fit, name), [di, di], g, MetricType.MSE if "Mse" in name else MetricType.LL)
    with pytest.raises(NotImplementedError, match="%s.predictor: .*no single training set" % name):
        f.predictor()


@pytest.mark.parametrize("name", ["DeviceLbfgsFitter", "DeviceMseLbfgsFitter", "DeviceLooLbfgsFitter"])
def test_the_fitters_ask_for_a_fit_first(name):
    di, g = _problem()
    f = _make(getattr(fit, name), di, g, MetricType.MSE if "Mse" in name else MetricType.LL)
    with pytest.raises(RuntimeError, match="%s.predictor: fit\\(\\) first" % name):
        f.predictor()


def test_fp32_refuses():
    f = engine.InverseFactorization.__new__(engine.InverseFactorization)   # (no device: only the dtype is looked at)
    f.code = _native.GPK_F32
    with pytest.raises(NotImplementedError, match="prediction is fp64 only"):
        f.predict(torch.zeros(3, 1))
