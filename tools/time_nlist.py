"""nbody_nlist_compute against the k = 6 tree kNN compute and a friends-of-friends compute at b = r on the same state, in ONE process
(boxes of the pool differ by several percent: only an interleaved comparison in one session says anything).  Times are HIP events
recorded on the context's own stream around `reps` back-to-back calls, the computes alternated, median of the rounds.
    python tools/time_nlist.py [--quick]
Per configuration — N = 65 536, 262 144 and 10^6; 3D galaxy and plummer; float and double — the radius is chosen for about 16, 64 and
256 neighbours a body: r16 is the MEDIAN distance to the 16th neighbour, from DeviceSystem.knn(16, "tree"), and the other two are
r16 4^(1/3) and r16 16^(1/3) (the count of a uniform neighbourhood grows with r^3).  What a radius really gives is on the line: the
mean and the largest count of that compute, and its status (2: a body has more than 4096 neighbours, so no list was made and the
time is that of the counts alone plus two launches that return at once).  The handle's capacity is the total of a counts-only compute.
The line gives the whole compute with lists, the counts-only compute (capacity 0), the k = 6 tree kNN compute and the
friends-of-friends compute (all four build the same structure), and the ratio lists / knn6.  --quick runs N = 262 144 only.
A compute's split over its kernels comes from a kernel trace of `--trace-run` (N = 262 144, neighbour-list computes only):
    rocprofv3 --kernel-trace --stats --output-format csv -- python tools/time_nlist.py --trace-run     (a run of its own)
    python tools/time_nlist.py --summarize KERNEL_TRACE.csv                                             (no GPU needed)
prints, per configuration, the median duration of every stage over the traced computes."""
import csv
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TARGETS = (16, 64, 256)
TRACE_N = 262144
TRACE_COMPUTES = 6  # per configuration of --trace-run, with lists


def timed(stream, fn, reps):
    import torch
    s = torch.cuda.ExternalStream(stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def medians(forms, stream, reps, rounds):
    import torch
    for f in forms:
        f()
    torch.cuda.synchronize()
    ms = [[] for _ in forms]
    for _ in range(rounds):
        for q, f in enumerate(forms):
            ms[q].append(timed(stream, f, reps))
    return [statistics.median(v) for v in ms]


def radii_for(dev):
    """The radii for about 16, 64 and 256 neighbours a body (see the head of the file)."""
    _, d2 = dev.knn(16, "tree")
    r16 = float(np.median(np.sqrt(d2[:, 15].astype(np.float64))))
    return [r16 * (t / 16.0) ** (1.0 / 3.0) for t in TARGETS]


def configurations(nb, sizes):
    for n in sizes:
        for model in ("galaxy", "plummer"):
            for tname, dtype in (("f32", nb.F32), ("f64", nb.F64)):
                dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, model, n))
                for target, r in zip(TARGETS, radii_for(dev)):
                    dev.nlist_compute(r, 0)
                    total = int(dev.nlist_handle(0).summary(dev.stream)[0])
                    yield n, model, tname, dev, target, r, total
                    if total in dev._nlist and total != 0:
                        dev._nlist.pop(total).close()  # one list-holding handle at a time
                dev.close()


STAGES = ("structure", "structure sort", "count walk", "scan", "fill walk", "ordering")


def stage_of(name):
    for text, stage in (("nlist_count", "count walk"), ("nlist_fill", "fill walk"), ("nlist_order", "ordering"), ("nlist_strip", "scan"),
                        ("nlist_scan", "scan"), ("nlist_offsets", "scan"), ("pair_pack", "structure"), ("nntree_bounds", "structure"),
                        ("nntree_keys", "structure"), ("nntree_gather", "structure"), ("nntree_upper", "structure"), ("nntree_walk", "other"),
                        ("nntree_finish", "other"), ("knn_", "other")):
        if text in name:
            return stage
    return "structure sort" if re.search(r"sort|splitter|radix", name) else None


def summarize(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    computes, cur = [], None
    for r in rows:  # a compute runs from the structure's pack kernel to its last kernel; the radius search's kNN computes are dropped
        name, stage = r["Kernel_Name"], stage_of(r["Kernel_Name"])
        if stage is None:
            continue
        if "pair_pack" in name:
            if cur is not None and "fill walk" in cur["us"] and not cur["other"]:
                computes.append(cur)
            cur = {"type": "f64" if "double" in name else "f32", "us": {}, "other": False}
        if cur is None:
            continue
        if stage == "other":
            cur["other"] = True
            continue
        cur["us"][stage] = cur["us"].get(stage, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0
    if cur is not None and "fill walk" in cur["us"] and not cur["other"]:
        computes.append(cur)
    print(f"{len(computes)} neighbour-list computes with lists traced at N = {TRACE_N}; median us per stage, kernels only")
    at = 0
    for model in ("galaxy", "plummer"):
        for tname in ("f32", "f64"):
            for target in TARGETS:
                group = computes[at:at + TRACE_COMPUTES]
                at += TRACE_COMPUTES
                assert len(group) == TRACE_COMPUTES and all(c["type"] == tname for c in group), (model, tname, target, len(group))
                med = {k: statistics.median(c["us"].get(k, 0.0) for c in group) for k in STAGES}
                total = sum(med.values())
                print(f"  {tname} {model:8s} ~{target:<3d} neighbours: " + ", ".join(f"{k} {med[k]:.1f}" for k in STAGES)
                      + f"; sum {total:.1f} (walks {100 * (med['count walk'] + med['fill walk']) / total:.0f} %, ordering {100 * med['ordering'] / total:.0f} %)")


def main():
    if "--summarize" in sys.argv:
        return summarize(sys.argv[sys.argv.index("--summarize") + 1])
    from conftest import load_package
    nb = load_package()
    if "--trace-run" in sys.argv:
        for n, model, tname, dev, target, r, total in configurations(nb, (TRACE_N,)):
            for _ in range(TRACE_COMPUTES):
                dev.nlist_compute(r, total)
            dev.sync()
        return None
    sizes = (TRACE_N,) if "--quick" in sys.argv else (65536, 262144, 1000000)
    print("fixed-radius neighbour lists vs the k = 6 tree kNN and friends-of-friends at b = r, 3D (ms per compute; ratio = lists / knn6)")
    for n, model, tname, dev, target, r, total in configurations(nb, sizes):
        forms = (lambda: dev.nlist_compute(r, total), lambda: dev.nlist_compute(r, 0), lambda: dev.knn_compute(6, "tree"), lambda: dev.fof_compute(r, 20))
        full, counts, knn, fof = medians(forms, dev.stream, 5, 5)
        _, most, _, status = (int(v) for v in dev.nlist_handle(total).summary(dev.stream))
        print(f"  {tname} N={n:<8d} {model:8s} ~{target:<3d} r={r:.4e}  lists {full:8.3f}   counts {counts:8.3f}   knn6 {knn:8.3f}   fof {fof:8.3f}   "
              f"ratio {full / knn:6.3f}   mean {total / n:7.1f} max {most:<6d} status {status}", flush=True)
    return None


if __name__ == "__main__":
    main()
