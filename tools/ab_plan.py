"""A/B of a host-only refactor between the parent's library (libnbody_hip_var_parent.so) and this tree's, alternately in one session:
parent / new / parent / new / parent / new, one child process per run.  Stops at the first child that fails.
    python tools/ab_plan.py bvh [--out FILE]        (profiles/bvh_plan/bench_parent_new.txt)
    python tools/ab_plan.py octree [--out FILE]     (profiles/octree_plan/ab_parent_new.txt)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
CASES = {"bvh": (("f64 1e4", 1, 10000, 200), ("f64 1e5", 1, 100000, 50), ("f64 1e6", 1, 1000000, 10), ("f32 1e6", 0, 1000000, 10)),
         "octree": (("f64 1e3", 1, 1000, 200), ("f64 1e5", 1, 100000, 50), ("f64 1e6", 1, 1000000, 10), ("f32 1e6", 0, 1000000, 10))}
TITLE = {"bvh": "BVH traversal", "octree": "Octree phases"}
NOTE = {"bvh": "auto traversal, theta 0.5, galaxy 3D.",
        "octree": "auto build and walk, theta 0.5, galaxy 3D; enqueue only: bounds + insert + multipoles + force, before the sync."}


def best_of(dev, fn, reps, rounds=5):
    """(ms per call with the device's work, ms per call of the host's enqueue alone), the best of `rounds`"""
    best, host = 1e9, 1e9
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        t1 = time.perf_counter()
        dev.sync()
        best = min(best, (time.perf_counter() - t0) / reps * 1e3)
        host = min(host, (t1 - t0) / reps * 1e3)
    return best, host


def recorded(nb, dev, body, reps):
    g = nb.StepGraph(dev, body)
    for _ in range(10):
        g.launch()
    dev.sync()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(max(reps, 20)):
            g.launch()
        dev.sync()
        best = min(best, (time.perf_counter() - t0) / max(reps, 20) * 1e3)
    g.close()
    return best


def child_bvh(nb, out):
    for label, dtype, n, reps in CASES["bvh"]:
        dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, "galaxy", n))
        st, t = dev.state(), dev.bvh
        t.bounding_box(st, dev.stream); t.hilbert_sort(st, dev.stream); t.build_tree(st, dev.stream)
        for _ in range(5):
            t.compute_force(st, 0.5, dev.stream)
        dev.sync()
        best, host = best_of(dev, lambda: t.compute_force(st, 0.5, dev.stream), reps)
        out[label + " eager traversal, ms"] = best
        if n == 10000:
            out[label + " eager traversal, enqueue only, ms"] = host
        out[label + " recorded bvh step, ms"] = recorded(nb, dev, lambda: (dev.bvh_force(0.5), dev.accelerate_step()), reps)
        dev.close()


def child_octree(nb, out):
    for label, dtype, n, reps in CASES["octree"]:
        dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, "galaxy", n))
        st, t = dev.state(), dev.octree
        phases = (("bounds", lambda: t.compute_bounds(st, dev.stream)), ("insert", lambda: t.insert(st, dev.stream)),
                  ("multipoles", lambda: t.compute_tree(dev.stream)), ("force", lambda: t.compute_force(st, 0.5, dev.stream)))
        for _ in range(3):
            for _, fn in phases:
                fn()
        dev.sync()
        for name, fn in phases:
            out[f"{label} eager {name}, ms"] = best_of(dev, fn, reps)[0]
        out[label + " eager four phases, enqueue only, ms"] = best_of(dev, lambda: [fn() for _, fn in phases], reps)[1]
        out[label + " recorded octree step, ms"] = recorded(nb, dev, lambda: (dev.octree_force(0.5), dev.accelerate_step()), reps)
        dev.close()
    best = 1e9
    for _ in range(50):  # 21 allocations and frees: the least of many, the runtime's allocator is noisy
        t0 = time.perf_counter()
        nb.Octree(nb.F64, 3, 1000000).close()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    out["f64 1e6 create + destroy of a handle, ms"] = best


if len(sys.argv) == 4 and sys.argv[1] == "--child":
    from conftest import load_package
    nb = load_package()
    nb.LIB_PATH, nb._lib = sys.argv[3], None
    out = {}
    {"bvh": child_bvh, "octree": child_octree}[sys.argv[2]](nb, out)
    print(json.dumps(out))
    sys.exit(0)

if len(sys.argv) < 2 or sys.argv[1] not in CASES:
    sys.exit(__doc__)
what = sys.argv[1]
libs = ["libnbody_hip_var_parent.so", "libnbody_hip.so"]
res = {l: [] for l in libs}
for rnd in range(3):
    for lib in libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", what, os.path.join(ROOT, "stdpar-nbody_amd", lib)],
                           capture_output=True, text=True, timeout=280)
        if r.returncode:
            print(lib, "FAILED with status", r.returncode, r.stderr[-1500:])
            sys.exit(1)
        res[lib].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("round", rnd, lib, "done", flush=True)
lines = [TITLE[what] + ", parent's library against this tree's, one session on one MI355X, runs alternated parent / new x 3 (ms; the",
         "three rounds of each).  " + NOTE[what] + "  The kernels are identical, so the yardstick is the parent's",
         "own spread: `inside` = every round of the new library lies in [parent min - spread, parent max + spread], spread = parent max - min.",
         "", "%-46s%30s%30s  %s" % ("", "parent", "new", "verdict")]
bad = 0
for k in res[libs[0]][0]:
    p = [r[k] for r in res[libs[0]]]
    q = [r[k] for r in res[libs[1]]]
    spread = max(p) - min(p)
    ok = min(p) - spread <= min(q) and max(q) <= max(p) + spread
    bad += not ok
    lines.append("%-46s%30s%30s  %s" % (k, " / ".join("%.4f" % v for v in p), " / ".join("%.4f" % v for v in q), "inside" if ok else "OUTSIDE"))
text = "\n".join(lines) + "\n"
if len(sys.argv) == 4 and sys.argv[2] == "--out":
    open(sys.argv[3], "w").write(text)
print(text)
