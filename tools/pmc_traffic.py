"""Per-launch HBM traffic of the trailing-update kernels from a tools/pmc_pass.sh run.

usage: python tools/pmc_traffic.py KEY [pmc_dir] [out.json]

HBM bytes of one dispatch = 2 x FETCH_SIZE + WRITE_SIZE (both in KiB; FETCH_SIZE doubled per
the gfx950 correction of MI355X_MICROARCH.md: it tallies 128-B requests at 64 B), averaged over
every update-class dispatch (gemm_kernel<T, 0, ...>, both tile shapes).  Stores the figure
under KEY (e.g. metric_b8) in profiles/pmc_traffic.json, where bench.py picks it up for
roofline.traffic.  Run the PMC pass with GPK_LOOKAHEAD=0 so that its update launches are the
ones of bench.py's roofline post-pass.
"""
import collections
import csv
import glob
import json
import re
import sys

key = sys.argv[1]
root = sys.argv[2] if len(sys.argv) > 2 else "bench_out/pmc"
out = sys.argv[3] if len(sys.argv) > 3 else "profiles/pmc_traffic.json"

per = collections.defaultdict(dict)   # dispatch id -> counter -> value
for f in sorted(glob.glob(root + "/p*/run_counter_collection.csv")):
    for r in csv.DictReader(open(f)):
        if not re.search(r"gemm_kernel<\w+, 0,", r["Kernel_Name"]):
            continue
        d = per[(f, r["Dispatch_Id"])]
        d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
fetch = [d["FETCH_SIZE"] for d in per.values() if "FETCH_SIZE" in d]
write = [d["WRITE_SIZE"] for d in per.values() if "WRITE_SIZE" in d]
if not fetch or not write:
    sys.exit("no FETCH_SIZE / WRITE_SIZE samples of the update kernels under " + root)
bpl = (2.0 * sum(fetch) / len(fetch) + sum(write) / len(write)) * 1024.0
try:
    db = json.load(open(out))
except (OSError, ValueError):
    db = {}
db[key] = {"hbm_bytes_per_launch": round(bpl), "dispatches": len(fetch),
           "source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (tools/pmc_pass.sh, GPK_LOOKAHEAD=0), "
                     "2 x FETCH + WRITE averaged over the update dispatches"}
json.dump(db, open(out, "w"), indent=1, sort_keys=True)
print(key, db[key])
