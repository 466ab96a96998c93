"""Split the update launches of the last look-ahead-off step of a rocprofv3 trace into the group
(bulk, K = 128 G) launches and the in-group launches, with their achieved TF/s.

usage: python tools/update_split.py bench_out/prof/run_kernel_trace.csv N BATCH [G] [INGROUP] [depth]
G / INGROUP: gpk_tune "group" / "ingroup" of the traced run (default: the library's, environment included).
The sequence of update launches, their depths and their flops are the library's own schedule for the shape
(nat.launch_plan with the look-ahead off), so every in-group mode and the fused K build are covered; the steps are
labelled by their role: thin, half, or group (a group's trailing update).  "depth" adds a per-depth table.
"""
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussianprocessfundamentals_amd import _native as nat  # noqa: E402


def sequence(n, batch, knobs):
    """(label, depth, flops of the whole batch) of every update launch, in issue order"""
    lay = nat.plan(nat.GPK_F64, batch, n, 0, 1)
    with nat.thread_tune(lookahead=0, **knobs):
        steps = nat.launch_plan(lay)
    label = {"thin": "thin", "half": "half"}
    return [(label.get(nat.LAUNCH_ROLES[int(s["role"])], "group"), int(s["kdepth"]), float(s["flops"]))
            for s in steps if nat.LAUNCH_KINDS[int(s["kind"])] == "update"]


def main():
    path, n, batch = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    knobs = {}
    if len(sys.argv) > 4:
        knobs["group"] = int(sys.argv[4])
    if len(sys.argv) > 5:
        knobs["ingroup"] = int(sys.argv[5])
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"])
                  for r in csv.DictReader(open(path)))
    starts = [i for i, r in enumerate(rows) if "assemble_kernel" in r[2]]
    step = rows[starts[-1]:]
    seq = sequence(n, batch, knobs)
    # one span per update step: a group / half step may be two kernels (gpk_tune "upd_tri": gemm_kernel on the strictly
    # lower tiles, then update_tri_kernel on the diagonal tiles; gemm_kernel is absent when no strictly lower tile is
    # left) -- its span is the sum of the two durations
    kern = [(s, e, "update_tri_kernel" in k) for s, e, k in step
            if "gemm_kernel<double, 0" in k or "gemm_kernel<float, 0" in k or "update_tri_kernel" in k]
    upd, i = [], 0
    while i < len(kern):
        s, e, tri = kern[i]
        i += 1
        if not tri and i < len(kern) and kern[i][2] and len(upd) < len(seq) and seq[len(upd)][0] != "thin":
            e = e + (kern[i][1] - kern[i][0])
            i += 1
        upd.append((s, e))
    if len(seq) != len(upd):
        print("launch count mismatch: trace %d, plan %d (other knobs than the traced run's?)" % (len(upd), len(seq)))
    tot = {}
    bydepth = {}
    for (s, e), (kind, depth, fl) in zip(upd, seq):
        t = tot.setdefault(kind, [0.0, 0.0, 0])
        t[0] += (e - s) * 1e-9
        t[1] += fl
        t[2] += 1
        if kind != "group":
            b = bydepth.setdefault((kind, depth), [0.0, 0.0, 0])
            b[0] += (e - s) * 1e-9
            b[1] += fl
            b[2] += 1
    for kind, (sec, fl, cnt) in tot.items():
        print("%-5s %3d launches  %.3f ms  %.1f TF/s" % (kind, cnt, sec * 1e3, fl / max(sec, 1e-12) / 1e12))
    big = [(e - s, fl) for (s, e), (kind, _, fl) in zip(upd, seq) if kind == "group"]
    for dt, fl in big[:4] + big[-3:]:
        print("   group launch %.1f us  %.1f TF/s" % (dt / 1e3, fl / max(dt * 1e-9, 1e-12) / 1e12))
    if "depth" in sys.argv[6:]:
        for (kind, depth), (sec, fl, cnt) in sorted(bydepth.items()):
            print("   %-4s depth %4d: %2d launches, avg %6.1f us, %.1f TF/s"
                  % (kind, depth, cnt, sec / cnt * 1e6, fl / sec / 1e12))


if __name__ == "__main__":
    main()
