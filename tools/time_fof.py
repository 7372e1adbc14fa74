"""nbody_fof_compute against the k = 6 tree kNN compute on the same state, in ONE process (boxes of the pool differ by several
percent: only an interleaved comparison in one session says anything).  Times are HIP events recorded on the context's own stream
around `reps` back-to-back calls, the two computes alternated, median of the rounds.
    python tools/time_fof.py [--quick]
Per configuration — N = 65 536, 262 144 and 10^6; 3D galaxy and plummer; float and double — the linking length is b = 1, 2 and 4
times the MEDIAN nearest-neighbour distance of the system, taken from DeviceSystem.knn(1, "tree"); the line gives the friends-of-
friends compute, the k = 6 tree kNN compute (the yardstick: the two share the structure's build), their ratio, the number of groups
and the largest group.  --quick runs N = 125 000 only.
A compute's split over its kernels comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats --output-format csv
-- python tools/time_fof.py --quick, a run of its own): the launches of a compute are separate kernels there, and
    python tools/time_fof.py --summarize KERNEL_TRACE.csv
prints, per configuration of the quick run, the median duration of every stage over the traced computes (no GPU needed)."""
import csv
import os
import re
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402


def timed(stream, fn, reps):
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def medians(forms, stream, reps, rounds):
    for f in forms:
        f()
    torch.cuda.synchronize()
    ms = [[] for _ in forms]
    for _ in range(rounds):
        for q, f in enumerate(forms):
            ms[q].append(timed(stream, f, reps))
    return [statistics.median(v) for v in ms]


STAGES = ("init", "structure", "structure sort", "link", "flatten + labels", "summary", "catalogue sort", "catalogue compaction",
          "catalogue sums")
COMPUTES_PER_CONFIG = 1 + 5 * 5  # the warm-up call, then 5 rounds of 5


def stage_of(name):
    for text, stage in (("fof_init", "init"), ("fof_link", "link"), ("fof_flatten", "flatten + labels"), ("fof_labels", "flatten + labels"),
                        ("fof_summary", "summary"), ("fof_cat_sum", "catalogue sums"), ("fof_cat", "catalogue compaction"),
                        ("pair_pack", "structure"), ("nntree_bounds", "structure"), ("nntree_keys", "structure"),
                        ("nntree_gather", "structure"), ("nntree_upper", "structure")):
        if text in name:
            return stage
    return "sort" if re.search(r"sort|splitter|radix", name) else None


def summarize(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    computes, cur = [], None
    for r in rows:  # a friends-of-friends compute runs from its init kernel to its catalogue sums
        name, stage = r["Kernel_Name"], stage_of(r["Kernel_Name"])
        if stage == "init":
            cur = {"type": None, "us": {}}
        if cur is None or stage is None:
            continue
        if stage == "sort":
            stage = "catalogue sort" if "link" in cur["us"] else "structure sort"
        if stage == "link":
            cur["type"] = "f64" if "double" in name else "f32"
        cur["us"][stage] = cur["us"].get(stage, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
        if stage == "catalogue sums":
            computes.append(cur)
            cur = None
    print(f"{len(computes)} friends-of-friends computes traced; median us per stage, kernels only")
    at = 0
    for model in ("galaxy", "plummer"):
        for tname in ("f32", "f64"):
            for mult in (1, 2, 4):
                group = computes[at:at + COMPUTES_PER_CONFIG]
                at += COMPUTES_PER_CONFIG
                assert len(group) == COMPUTES_PER_CONFIG and all(c["type"] == tname for c in group), (model, tname, mult)
                med = {k: statistics.median(c["us"].get(k, 0.0) for c in group) for k in STAGES}
                total = sum(med.values())
                print(f"  {tname} {model:8s} b={mult}x: " + ", ".join(f"{k} {med[k]:.1f}" for k in STAGES)
                      + f"; sum {total:.1f} (link {100 * med['link'] / total:.0f} %)")


def main():
    if "--summarize" in sys.argv:
        return summarize(sys.argv[sys.argv.index("--summarize") + 1])
    quick = "--quick" in sys.argv
    nb = load_package()
    sizes = (125000,) if quick else (65536, 262144, 1000000)
    print("friends-of-friends vs the k = 6 tree kNN, 3D (ms per compute; ratio = fof / knn; b in units of the median nearest-neighbour distance)")
    for n in sizes:
        for model in ("galaxy", "plummer"):
            for tname, dtype in (("f32", nb.F32), ("f64", nb.F64)):
                dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, model, n))
                _, d2 = dev.knn(1, "tree")
                nnd = float(np.median(np.sqrt(d2[:, 0].astype(np.float64))))
                for mult in (1, 2, 4):
                    b = mult * nnd
                    f, k = medians((lambda: dev.fof_compute(b, 20), lambda: dev.knn_compute(6, "tree")), dev.stream, 5, 5)
                    groups, _, largest, _ = dev.fof_handle(20).summary(dev.stream)
                    print(f"  {tname} N={n:<8d} {model:8s} b={mult} x {nnd:.4e}  fof {f:8.3f}   knn6 {k:8.3f}   ratio {f / k:6.3f}   "
                          f"groups {groups:<8d} largest {largest}", flush=True)
                dev.close()


if __name__ == "__main__":
    main()
