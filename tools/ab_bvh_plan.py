"""A/B of the BVH traversal between the parent's library (libnbody_hip_var_parent.so) and this tree's, alternately in one session:
parent / new / parent / new / parent / new, one child process per run.  Stops at the first child that fails.
    python tools/ab_bvh_plan.py [--out FILE]        (profiles/bvh_plan/bench_parent_new.txt)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
CASES = (("f64 1e4", 1, 10000, 200), ("f64 1e5", 1, 100000, 50), ("f64 1e6", 1, 1000000, 10), ("f32 1e6", 0, 1000000, 10))


def child(lib):
    from conftest import load_package
    nb = load_package()
    nb.LIB_PATH, nb._lib = lib, None
    out = {}
    for label, dtype, n, reps in CASES:
        dev = nb.DeviceSystem.from_host(nb.build_model(dtype, 3, "galaxy", n))
        st, t = dev.state(), dev.bvh
        t.bounding_box(st, dev.stream); t.hilbert_sort(st, dev.stream); t.build_tree(st, dev.stream)
        for _ in range(5):
            t.compute_force(st, 0.5, dev.stream)
        dev.sync()
        best, host = 1e9, 1e9
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(reps):
                t.compute_force(st, 0.5, dev.stream)
            t1 = time.perf_counter()
            dev.sync()
            best = min(best, (time.perf_counter() - t0) / reps * 1e3)
            host = min(host, (t1 - t0) / reps * 1e3)
        out[label + " eager traversal, ms"] = best
        if n == 10000:
            out[label + " eager traversal, enqueue only, ms"] = host
        g = nb.StepGraph(dev, lambda: (dev.bvh_force(0.5), dev.accelerate_step()))
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
        out[label + " recorded bvh step, ms"] = best
        g.close(); dev.close()
    print(json.dumps(out))


if len(sys.argv) == 3 and sys.argv[1] == "--child":
    child(sys.argv[2])
    sys.exit(0)

libs = ["libnbody_hip_var_parent.so", "libnbody_hip.so"]
res = {l: [] for l in libs}
for rnd in range(3):
    for lib in libs:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.join(ROOT, "stdpar-nbody_amd", lib)],
                           capture_output=True, text=True, timeout=280)
        if r.returncode:
            print(lib, "FAILED with status", r.returncode, r.stderr[-1500:])
            sys.exit(1)
        res[lib].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print("round", rnd, lib, "done", flush=True)
lines = ["BVH traversal, parent's library against this tree's, one session on one MI355X, runs alternated parent / new x 3 (ms; the",
         "three rounds of each).  auto traversal, theta 0.5, galaxy 3D.  The kernels are identical, so the yardstick is the parent's",
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
if len(sys.argv) == 3 and sys.argv[1] == "--out":
    open(sys.argv[2], "w").write(text)
print(text)
