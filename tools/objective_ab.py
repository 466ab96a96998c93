"""A/B of the fit objectives' results between two checkouts (needs the MI355X): every result array as a SHA-256.

    python tools/objective_ab.py dump <out.json>        (in each checkout, with its own libgpk.so)
    python tools/objective_ab.py compare <a.json> <b.json>

dump: seeded inputs through the five evaluators of sweep (-LML, k-fold -LML, MSE, k-fold MSE, LOO with both losses;
1 and 3 candidates, plain and settle=True) and through the metric-level entries on the same engine classes
(LogLikelihood and MeanSquaredError get_metric_and_gradient, LeaveOneOut value / gradient / predictions with both
losses, CrossValidation's fold metrics for LL and MSE, the blockwise -LML gradient).  Sizes 70, 257 and 1024; kernels
SE, ADD(SE, PER) and a change point over two SE children; gpk_tune chain 0 (launch path) and 2 (persistent launch
where the batch allows it).  compare: every case of either dump must be in both with equal digests; prints the case
count and the verdict, exit status 1 on any difference.
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (70, 257, 1024)
HYPS = {"SE": [0.3], "ADD": [0.3, 0.9, 0.5], "CP": [0.45, 0.2, 0.4]}
NOISE = 0.05


def _digests(obj):
    """One SHA-256 per array of a nested result (tensors, floats, lists; None as an empty array)."""
    import numpy as np
    import torch
    if isinstance(obj, torch.Tensor):
        return [hashlib.sha256(np.ascontiguousarray(obj.detach().cpu().numpy()).tobytes()).hexdigest()]
    if isinstance(obj, (list, tuple)):
        return [d for o in obj for d in _digests(o)]
    return [hashlib.sha256(np.asarray([] if obj is None else obj, dtype=np.float64).tobytes()).hexdigest()]


def dump(path):
    import numpy as np
    import torch

    import gaussianprocessfundamentals_amd.global_parameters as gp
    gp.init(0)
    from gaussianprocessfundamentals_amd import _native as nat
    from gaussianprocessfundamentals_amd import engine, sweep
    from gaussianprocessfundamentals_amd.DataHandling.DataInput import BlockwiseDataInput, DataInput
    from gaussianprocessfundamentals_amd.KernelBasics import BaseKernels as bk
    from gaussianprocessfundamentals_amd.KernelBasics import Operators as ops
    from gaussianprocessfundamentals_amd.MeanFunctionBasics.BaseMeanFunctions import ZeroMeanFunction
    from gaussianprocessfundamentals_amd.Metrics import CrossValidation as cv
    from gaussianprocessfundamentals_amd.Metrics import MatrixHandlingTypes as mht
    from gaussianprocessfundamentals_amd.Metrics.Auxiliary import get_metric_by_type
    from gaussianprocessfundamentals_amd.Metrics.LeaveOneOut import LeaveOneOut
    from gaussianprocessfundamentals_amd.Metrics.Metrics import MetricType
    from gaussianprocessfundamentals_amd.Statistics.GaussianProcess import BlockwiseGaussianProcess, GaussianProcess

    dev = engine.device()
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)  # noqa: E731
    S = lambda v: torch.tensor(v, dtype=torch.float64)  # noqa: E731

    def kernel(name):
        se, per = bk.SquaredExponentialKernel, bk.PeriodicKernel
        if name == "SE":
            return se(1)
        if name == "ADD":
            return ops.AdditionOperator(1, [se(1), per(1)])
        return ops.ChangePointOperator(1, [se(1), se(1)], [S(0.45)])

    def points(n, seed):
        rng = np.random.default_rng(seed)
        x = np.sort(rng.uniform(0.0, 1.0, (n, 1)), axis=0)
        return x, np.sin(7.0 * x[:, 0]) + np.where(x[:, 0] < 0.45, 0.0, 0.5) + 0.1 * rng.standard_normal(n)

    def process(k, x, y, xs, ys):
        di = DataInput(x, y.reshape(-1, 1), xs, ys.reshape(-1, 1))
        di.set_mean_function(ZeroMeanFunction(1))
        g = GaussianProcess(k, ZeroMeanFunction(1))
        g.set_data_input(di)
        return g, di

    res = {}
    for chain in (0, 2):
        old = nat.tune("chain", chain)
        for n in SIZES:
            m = max(5, n // 8)
            x, y = points(n, n)
            xs, ys = points(m, n + 1)
            folds = [points(n - f, 10 * n + f) + points(m - f, 20 * n + f) for f in range(2)]
            for name, hyp in HYPS.items():
                key = "chain=%d n=%d %s " % (chain, n, name)
                k = kernel(name)
                dfolds = [tuple(T(a) for a in fold) for fold in folds]
                evaluators = {
                    "nlml": sweep.native_batched_value_and_gradient(k, T(x), T(y)),
                    "kfold_nlml": sweep.native_kfold_value_and_gradient(k, [f[:2] for f in dfolds]),
                    "mse": sweep.native_batched_mse_value_and_gradient(k, T(x), T(y), T(xs), T(ys)),
                    "kfold_mse": sweep.native_kfold_mse_value_and_gradient(k, dfolds),
                    "loo_lpd": sweep.native_batched_loo_value_and_gradient(k, T(x), T(y), nat.LOO_LPD),
                    "loo_mse": sweep.native_batched_loo_value_and_gradient(k, T(x), T(y), nat.LOO_MSE),
                }
                for B in (1, 3):
                    cands = T([[h + 0.03 * b for h in hyp] + [NOISE + 0.01 * b] for b in range(B)])
                    for what, ev in evaluators.items():
                        for settle in (False, True):
                            res[key + "%s B=%d settle=%d" % (what, B, settle)] = _digests(ev(cands, settle=settle))
                g, di = process(k, x, y, xs, ys)
                hl, nz = [S(h) for h in hyp], S(NOISE)
                for mt in (MetricType.LL, MetricType.MSE):
                    res[key + "metric %s" % mt.name] = _digests(get_metric_by_type(mt, g).get_metric_and_gradient(hl, nz))
                    loo = LeaveOneOut(di, g.covariance_matrix, loss=mt)
                    res[key + "LeaveOneOut %s" % mt.name] = _digests(
                        [loo.get_metric(hl, nz), loo.get_metric_and_gradient(hl, nz), loo.get_predictions(hl, nz)])
                    np.random.seed(7)
                    split = cv.get_data_inputs(di, 0.2)
                    cross = cv.CrossValidation(g, di, mht.MatrixApproximations.NONE,
                                               mht.NumericalMatrixHandlingType.CHOLESKY_BASED, metric_type=mt)
                    res[key + "CrossValidation %s" % mt.name] = _digests(cross.batched_fold_metrics(split, hl, nz))
            # the blockwise -LML gradient: three segments with their own programs, one ragged batch
            cps = [S(0.25), S(0.6)]
            children = [bk.SquaredExponentialKernel(1), bk.MaternKernel5_2(1), bk.PeriodicKernel(1)]
            bdi = BlockwiseDataInput(x, y.reshape(-1, 1), xs, ys.reshape(-1, 1), cps)
            bdi.set_mean_function(ZeroMeanFunction(1))
            bg = BlockwiseGaussianProcess(ops.ChangePointOperator(1, children, cps), ZeroMeanFunction(1))
            bg.set_data_input(bdi)
            metric = get_metric_by_type(MetricType.blockwise_LL, bg)
            res["chain=%d n=%d blockwise_LL" % (chain, n)] = _digests(
                metric.get_metric_and_gradient([S(v) for v in (0.08, 0.3, 0.9, 0.45)], nz))
        nat.tune("chain", old)
    torch.cuda.synchronize()
    with open(path, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print("wrote %s: %d cases, %d arrays" % (path, len(res), sum(len(v) for v in res.values())))


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = sorted(set(A) ^ set(B)) + sorted(k for k in set(A) & set(B) if A[k] != B[k])
    print("%s: %d cases (%d arrays); %s: %d cases (%d arrays); %d differ: %s" % (
        a, len(A), sum(len(v) for v in A.values()), b, len(B), sum(len(v) for v in B.values()), len(bad),
        "DIFFERENT" if bad else "every array equal bit for bit"))
    for k in bad[:50]:
        print("  DIFFERS", k)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        sys.exit(dump(sys.argv[2]))
    sys.exit("usage: objective_ab.py dump <out.json> | objective_ab.py compare <a.json> <b.json>")
