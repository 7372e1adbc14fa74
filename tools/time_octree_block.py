"""Block time steps of the octree leapfrog (nbody_octree_block_*), timed in ONE process per table (boxes of the pool differ by several
percent: only an interleaved comparison in one session says anything).
    python tools/time_octree_block.py [--quick] [a] [b] [c]      the three tables below (default: all), profiler off
    python tools/time_octree_block.py --trace N                   the block steps of table (b) for N bodies, nothing timed: run it as
        rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/time_octree_block.py --trace N
    python tools/time_octree_block.py --summarize DIR             the split of a block step into its phases from that trace
(a) a block step with every body active (max_level = 0) against the fixed octree step (clear, bounds, insert, multipoles, softened walk,
    accelerate_step), 3D galaxy, eps = 0.05, theta = 0.5: N = 10^5 and 10^6 in double and float.  HIP events around `reps` calls, the
    two forms alternated, median and min .. max of the rounds.  The build and the walk are the same launches, so the difference is
    the schedule, the two active lists, the predictor and the 8-byte read-back against K3.
(b) time per block step against n_act in {1, 64, 1024, 16 384, N}, N = 10^5 and 10^6 in double: HIP events around every single call and
    the host clock around call + synchronise.  The active sets are made by construction: n_act tracers of negligible mass are put
    at distance ~ eps around the heaviest body (eps a twentieth of the distance of its nearest neighbour), where the softened pull is at its largest; dt
    is 0.8 of the largest step that keeps every other body at level 0, and the tracers' criterion then puts them `levels` (>= 1, at most 4)
    deeper: all but one block step of an interval have exactly the tracers active, the last one all N.  A row is printed only if
    every timed step had the n_act it was built for.  The split into schedule / predict / build / walk list / walk / kick comes from
    a kernel trace of the same steps (--trace, --summarize).
(c) a whole run: galaxy, N = 10^6, float, theta = 0.5, eps = 0.05, to t = 16 dt of the model: block steps (eta 0.8 .. 0.05,
    max_level = 8, dt_max = 16 dt) against fixed steps of dt_max / 2^s: wall time, block steps, body steps, |dE / E| from octree_energies."""
import collections
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

EPS, THETA, ETA = 0.05, 0.5, 0.02


def events(stream):
    import torch
    s = torch.cuda.ExternalStream(stream)
    return s, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)


def timed(stream, fn, reps):
    s, e0, e1 = events(stream)
    e0.record(s)
    for _ in range(reps):
        fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def spread(v):
    return f"{statistics.median(v):9.3f} ms ({min(v):.3f} .. {max(v):.3f})"


# ---- (a) -----------------------------------------------------------------------------------------------------------------------------
def table_a(nb, quick):
    print("(a) every body active: nbody_octree_block_step with max_level = 0 against the fixed octree step (softened walk + K3); "
          "median (min .. max) of the rounds")
    for tname, dtype in (("f64", nb.F64), ("f32", nb.F32)):
        for n in (100000, 1000000):
            n = n // 8 if quick else n
            hs = nb.build_model(dtype, 3, "galaxy", n)
            fixed, block = nb.DeviceSystem.from_host(hs), nb.DeviceSystem.from_host(hs)
            block.octree_block_start(THETA, EPS, ETA, 0)

            def fixed_step():
                fixed.octree_force(THETA, softening=EPS)
                fixed.accelerate_step()

            forms = ((fixed, fixed_step), (block, lambda: block.octree_block_step(THETA, EPS, ETA)))
            for d, f in forms:
                f()
                d.sync()
            reps, rounds = 10, 7
            ms = [[], []]
            for _ in range(rounds):
                for k, (d, f) in enumerate(forms):
                    ms[k].append(timed(d.stream, f, reps))
            fixed.octree.info(fixed.stream)
            block.octree.info(block.stream)
            ratio = statistics.median(ms[1]) / statistics.median(ms[0])
            print(f"{tname} 3D galaxy N={hs.n:<8d} fixed step {spread(ms[0])}   block step {spread(ms[1])}   ratio {ratio:.4f}", flush=True)
            fixed.close()
            block.close()


# ---- (b) -----------------------------------------------------------------------------------------------------------------------------
def nrm(q):
    return np.sqrt((q * q).sum(-1))


def tracer_case(nb, n, k):
    """The galaxy with its last k bodies made tracers (1e-12 of the lightest mass) in a shell of 0.8 .. 1.2 eps around the
    heaviest body; returns (hs, eps, levels)."""
    hs = nb.build_model(nb.F64, 3, "galaxy", n)
    n = hs.n
    heavy = int(np.argmax(hs.m[: n - k]))
    d = nrm(hs.x[: n - k] - hs.x[heavy])
    d[heavy] = np.inf
    eps = float(d.min() / 20)
    rng = np.random.default_rng(7)
    u = rng.normal(0, 1, (k, 3))
    tr = np.arange(n - k, n)
    hs.m[tr] = hs.m[: n - k].min() * 1e-12  # not 0: a cell of tracers alone needs a centre of mass
    hs.x[tr] = hs.x[heavy] + eps * rng.uniform(0.8, 1.2, (k, 1)) * u / nrm(u)[:, None]
    hs.v[tr] = hs.v[heavy]
    dev = nb.DeviceSystem.from_host(hs)
    dev.octree_force(THETA, softening=eps)
    a = nrm(dev.download().a)
    dev.close()
    kk = 2 * ETA * eps
    hs.dt = float(0.8 * np.sqrt(kk / a[: n - k].max()))  # every other body stays at level 0, with a margin for the steps to come
    want = float(np.sqrt(kk / a[tr].min()))
    levels = 0
    while levels < 4 and hs.dt / 2 ** (levels + 1) >= want * 1.2:  # a margin: the tracers must stay at the deepest level
        levels += 1
    return hs, eps, levels


def table_b(nb, quick, trace_n=None):
    if trace_n is None:
        print("(b) time per block step against n_act (double, 3D galaxy, theta = 0.5): HIP events around one call | host clock around "
              "call + sync; medians")
    for n in ((100000, 1000000) if trace_n is None else (trace_n,)):
        n = n // 8 if quick else n
        all_active = []
        for k in (k for k in (1, 64, 1024, 16384) if k <= n // 4):
            hs, eps, levels = tracer_case(nb, n, k)
            if levels < 1:
                print(f"N={n:<8d} n_act={k:<8d} the tracers do not reach a deeper level than the rest: row void")
                continue
            dev = nb.DeviceSystem.from_host(hs)
            dev.octree_block_start(THETA, eps, ETA, levels)
            dev.sync()
            s, e0, e1 = events(dev.stream)
            ev, wall, ok, seen = [], [], True, set()
            for interval in range(1 if trace_n else 4):
                for step in range(1 << 20):  # until the interval is complete
                    t0 = time.perf_counter()
                    e0.record(s)
                    n_act, tau = dev.octree_block_step(THETA, eps, ETA)
                    e1.record(s)
                    e1.synchronize()
                    w = (time.perf_counter() - t0) * 1e3
                    last = tau == 1 << levels
                    ok = ok and n_act == (hs.n if last else k)
                    seen.add(n_act)
                    if last:
                        all_active.append((e0.elapsed_time(e1), w))
                        break
                    if interval or step:  # the very first step loads the code objects
                        ev.append(e0.elapsed_time(e1))
                        wall.append(w)
            try:
                dev.octree.info(dev.stream)
            except nb.NbodyError as e:
                ok = False
                print(f"N={n:<8d} n_act={k:<8d} {e}")
            dev.close()
            if trace_n is None:
                print(f"N={n:<8d} n_act={k:<8d} {statistics.median(ev) * 1e3:10.1f} us | {statistics.median(wall) * 1e3:10.1f} us   "
                      f"(max_level {levels}, {len(ev)} steps)" + ("" if ok else f"   (NOT the active sets it was built for, but {sorted(seen)[:6]}: row void)"), flush=True)
        if trace_n is None and all_active:
            print(f"N={n:<8d} n_act={n:<8d} {statistics.median(q[0] for q in all_active) * 1e3:10.1f} us | "
                  f"{statistics.median(q[1] for q in all_active) * 1e3:10.1f} us", flush=True)


PHASES = (("schedule", ("block_sched_min_kernel",)), ("predict", ("otb_predict_kernel",)), ("walk", ("ot_force_softened_kernel",)),
          ("kick", ("otb_kick_kernel",)),
          ("lists", ("block_sched_count_kernel", "block_sched_scan_kernel", "block_sched_compact_kernel")))


def summarize(d):
    """Per class of block step (the grid of its walk), per phase: median of the summed kernel times, and the median span of the step.
    `lists`: both active lists (six launches); `build`: everything between the predictor and the walk list that is not one of ours
    (bounds, keys, radix sort, cells, multipoles)."""
    f = sorted(glob.glob(d + "/**/*kernel_trace.csv", recursive=True))[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    name = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "").replace("nbody::", "").split("<")[0]
    steps, cur = [], None
    for r in rows:
        nm = name(r)
        if nm == "block_sched_min_kernel":
            cur = []
        if cur is not None:
            cur.append(r)
            if nm == "otb_kick_kernel":
                steps.append(cur)
                cur = None
    classes = collections.defaultdict(list)
    for s in steps:
        walk = [r for r in s if name(r) == "ot_force_softened_kernel"]
        if len(walk) == 1:
            wg = int(walk[0].get("Workgroup_Size_X", 64) or 64)
            classes[int(walk[0]["Grid_Size_X"]) // wg].append(s)
    for blocks, ss in sorted(classes.items()):
        tot = collections.defaultdict(list)
        for s in ss:
            acc = collections.defaultdict(float)
            for r in s:
                nm, dur = name(r), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
                key = next((p for p, pre in PHASES if nm.startswith(pre)), "build")
                acc[key] += dur
            for key in ("schedule", "lists", "predict", "build", "walk", "kick"):
                tot[key].append(acc[key])
            tot["launches"].append(len(s))
            tot["span"].append((int(s[-1]["End_Timestamp"]) - int(s[0]["Start_Timestamp"])) / 1e3)
        med = {k: statistics.median(v) for k, v in tot.items()}
        busy = sum(med[k] for k in ("schedule", "lists", "predict", "build", "walk", "kick"))
        print(f"walk grid {blocks} waves (n_act <= {blocks * 8}): {len(ss)} block steps, {int(med['launches'])} launches each; kernel us: "
              + "  ".join(f"{k} {med[k]:.1f}" for k in ("schedule", "lists", "predict", "build", "walk", "kick"))
              + f"  | busy {busy:.1f}, first launch .. kick {med['span']:.1f} us (device clock)")


# ---- (c) -----------------------------------------------------------------------------------------------------------------------------
def table_c(nb, quick):
    n = 1000000 // (8 if quick else 1)
    base = nb.build_model(nb.F32, 3, "galaxy", n)
    nint, L, span = 1, 8, 16
    print(f"(c) galaxy N={base.n} float, theta = {THETA}, eps = {EPS}, to t = {span} dt of the model (dt = {base.dt:g}); wall time (host "
          f"clock, synchronised), |dE / E| from octree_energies at theta = {THETA}")

    def system(dt):
        hs = nb.build_model(nb.F32, 3, "galaxy", n)
        hs.dt = dt
        return hs

    def energy(dev):
        k, p = dev.octree_energies(THETA, softening=EPS)
        return float(k) + float(p)

    for eta in (0.8, 0.4, 0.2, 0.05):
        dev = nb.DeviceSystem.from_host(system(base.dt * span))
        e0 = energy(dev)
        dev.octree_block_start(THETA, EPS, eta, L)
        dev.sync()
        t0 = time.perf_counter()
        bs, bod = 0, 0
        for _ in range(nint):
            s, b = dev.octree_block_advance(THETA, EPS, eta)
            bs, bod = bs + s, bod + b
        dev.sync()
        w = time.perf_counter() - t0
        dev.octree.info(dev.stream)
        lev, _ = dev.octree_block_levels()
        de = abs((energy(dev) - e0) / e0)
        dev.close()
        print(f"  block steps eta={eta}: {w * 1e3:10.1f} ms  {bs} block steps, {bod} body steps ({bod / base.n:.2f} N)  |dE/E| {de:.3g}  "
              f"levels {np.bincount(lev, minlength=L + 1).tolist()}", flush=True)
    for sub in (0, 2, 4, 6):
        dev = nb.DeviceSystem.from_host(system(base.dt * span / 2 ** sub))
        e0 = energy(dev)
        dev.sync()
        t0 = time.perf_counter()
        for _ in range(nint << sub):
            dev.octree_force(THETA, softening=EPS)
            dev.accelerate_step()
        dev.sync()
        w = time.perf_counter() - t0
        dev.octree.info(dev.stream)
        de = abs((energy(dev) - e0) / e0)
        dev.close()
        print(f"  fixed step dt_max/2^{sub}:  {w * 1e3:10.1f} ms  {nint << sub} steps ({nint << sub} N evaluations)  |dE/E| {de:.3g}", flush=True)


def main():
    args = sys.argv[1:]
    if "--summarize" in args:
        return summarize(args[args.index("--summarize") + 1])
    nb = load_package()
    quick = "--quick" in args
    if "--trace" in args:
        return table_b(nb, quick, int(args[args.index("--trace") + 1]))
    which = [a for a in args if a in ("a", "b", "c")] or ["a", "b", "c"]
    for w in which:
        {"a": table_a, "b": table_b, "c": table_c}[w](nb, quick)


if __name__ == "__main__":
    main()
