"""A/B of the chain planner (gpk_chain_plan_ex; host only, no GPU) between two builds of libgpk.so, selected with GPK_LIB.

    GPK_LIB=<library> python tools/plan_ab.py dump <out.json>
    python tools/plan_ab.py compare <a.json> <b.json>

dump: for every case the task count and the SHA-256 of the task words (int32, four per task, in claim order) -- the
lists themselves run to gigabytes.  Cases: 1-5, 8, 9, 16, 17, 32, 33, 47, 48, 63, 64, 79, 80 and 96 diagonal blocks;
the y row 0, 5, 127 and 129 rows past n_pad (identity-augmented plans: n = n_pad and n_pad - 127 rows past it); grids
of 1, 2, 7, 64, 96, 256 and 304 workgroups; plain, identity-augmented and f32 plans; the knobs at their defaults and
every planner knob swept alone (SWEEPS; the three that only identity-augmented plans read on those plans only), set
with gpk_tune.  compare: every case of either dump must be in both with equal count and digest (equal words); prints
the case count and the verdict, exit status 1 on any difference.
"""
import hashlib
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NB = 128
BLOCKS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 47, 48, 63, 64, 79, 80, 96)
Y_PAST = (0, 5, 127, 129)
GRIDS = (1, 2, 7, 64, 96, 256, 304)
EYE_ONLY = ("chain_group_eye", "chain_group_corner", "chain_corner_tail")
SWEEPS = (
    (None, (None,)),  # the defaults
    ("chain_group", (0, 1, 2, 4, 8, 16)),
    ("chain_group_eye", (0, 1, 4, 8, 16)),
    ("chain_group_corner", (1, 4, 8, 16)),
    ("chain_corner_tail", (0, 4, 8, 16)),
    ("chain_group_la", (1, 2, 3)),
    ("chain_group_near", (1, 2, 4)),
    ("chain_near_la", (1, 2, 3)),
    ("chain_uq", (0, 1, 2)),
    ("chain_u128", (0, 1, 2)),
    ("chain_s128", (0, 1, 2)),
)


def shapes(kinds):
    for kind in kinds:
        for nblk in BLOCKS:
            n_pad = nblk * NB
            for past in ((n_pad, n_pad - 127) if kind == "eye" else Y_PAST):
                for grid in GRIDS:
                    yield kind, n_pad, n_pad + past, grid


def _setting(job):
    """One knob setting in a process of its own (the knobs are process-wide): {case: [ntasks, sha256]}."""
    knob, value = job
    from gaussianprocessfundamentals_amd import _native as nat
    old = nat.tune(knob, value) if knob else None
    out = {}
    for kind, n_pad, y_row, grid in shapes(("eye",) if knob in EYE_ONLY else ("plain", "eye", "f32")):
        t = nat.chain_plan(n_pad, y_row, grid, eye=kind == "eye", f32=kind == "f32")
        out["%s=%s %s n_pad=%d y_row=%d grid=%d" % (knob, value, kind, n_pad, y_row, grid)] = [
            len(t), hashlib.sha256(t.tobytes()).hexdigest()]
    if knob:
        nat.tune(knob, old)
    return out


def dump(path):
    jobs = [(knob, v) for knob, values in SWEEPS for v in values]
    res = {}
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for part in ex.map(_setting, jobs):
            res.update(part)
    with open(path, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
    print("wrote %s: %d plans, %d tasks, %d knob settings, library %s" % (
        path, len(res), sum(v[0] for v in res.values()), len(jobs), os.environ.get("GPK_LIB", "(in-tree)")))


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = sorted(set(A) ^ set(B)) + sorted(k for k in set(A) & set(B) if A[k] != B[k])
    print("%d plans (%d tasks), %d differ: %s" % (len(A), sum(v[0] for v in A.values()), len(bad),
                                                  "DIFFERENT" if bad else "every list equal word for word"))
    for k in bad[:50]:
        print("  DIFFERS", k, A.get(k), B.get(k))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    dump(sys.argv[2])
