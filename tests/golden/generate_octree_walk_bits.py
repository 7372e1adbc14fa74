#!/usr/bin/env python3
"""The bits of the six compiler-scheduled octree walks (ot_force_kernel, ot_force_softened_kernel, ot_force_quadrupole_kernel,
ot_potential_kernel, ot_potential_softened_kernel, ot_potential_quadrupole_kernel) as sha256 hashes:
tests/golden/octree_walk_bits.json, compared with == by tests/test_gpu_octree_walk_bits.py.  A body's walk result depends on nothing
but the tree and that body, and the tree's build is not what the fixture guards, so the fixture holds a restructuring of the walk to
the same tests, accepted terms, order of the 2^D partial sums, indices and bounds.  It was written once, on an MI355X, from the code
as it stood while the walk was the text csrc/ot_walk_body.inc pasted into six kernels, and is not regenerated from later code: a
mismatch is a bug in the code (a changed operation, contraction, summation order, index or bound), never a reason to run this script
again.

Inputs are seeded NumPy draws (no library of the project is involved): seed 6000 + n, m uniform in [0.5, 1.5) / n, x normal, all
rounded to the type, c = 1; at n = 1025 and 4097 one body is then moved to 2^-30 (float: 2^-12) beside another, which puts the near
branches of ot_accumulate and ot_potential_term on a recorded path.  Sizes, each in {double, float} x {3D, 2D} and at theta 0 (every
cell opened, every term a leaf) and 0.5: 1 (the root is a body, the loop is never entered), 2 (the root opened once: one sibling
group), 17 (more bodies than a wave holds, invalid lanes in the last block), 1000 and 1025 (either side of kSmallN = 1024: the
one-block build and the general one), 4097; at 4097 also the shard window first = 1000, count = 2000 (the owned list, body - first);
in double 3D also the 60-level chain of tests/test_gpu_octree.py::_deep_chain at theta 0 (cells below the key depth, ~120 pending
cells, the stack not full).  Every case runs all six walks on one tree (walk form 1, so the plain force is the compiler-scheduled
kernel too; eps = 2^-4 for the softened ones), each once with the counters off and once with them on, into buffers filled with a
sentinel beforehand.  run_case gives per walk W: "W" and "W+count" (a or phi of the two COUNT instantiations) and "W+counters" (the
counters' rows of the window).  nbody_octree_info is asked after every walk and no case may raise a flag.  In every recorded case the
two COUNT instantiations gave the same a / phi and the six walks the same counters (compact() fails otherwise), so the file holds
seven hashes per case, one line each: one per walk and "counters"; expand() gives back the eighteen that run_case is compared with.

    python tests/golden/generate_octree_walk_bits.py        (needs the GPU)
"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "octree_walk_bits.json")

SIZES = [1, 2, 17, 1000, 1025, 4097]
CLOSE_PAIR_SIZES = (1025, 4097)
WINDOW_N, WINDOW = 4097, (1000, 2000)
CHAIN_LEVELS = 60
THETAS = (0.0, 0.5)
EPS, C_GRAV = 2.0 ** -4, 1.0
TYPES = [(dtype, dim) for dtype in (1, 0) for dim in (3, 2)]
WALKS = ("force", "force_softened", "force_quadrupole", "potential", "potential_softened", "potential_quadrupole")
# (dtype, dim, n, theta, first, count); n = 0: the chain
CASES = ([(dtype, dim, n, theta, 0, n) for n in SIZES for theta in THETAS for dtype, dim in TYPES] +
         [(dtype, dim, WINDOW_N, theta) + WINDOW for theta in THETAS for dtype, dim in TYPES] +
         [(1, 3, 0, 0.0, 0, 0)])


def case_key(dtype, dim, n, theta, first, count):
    what = f"n{n}" if n else f"chain{CHAIN_LEVELS}"
    return f"{'f64' if dtype == 1 else 'f32'}-{dim}d-{what}-theta{theta}" + (f"-first{first}-count{count}" if n and count != n else "")


def load_package():
    if "stdpar_nbody_amd" in sys.modules:
        return sys.modules["stdpar_nbody_amd"]
    spec = importlib.util.spec_from_file_location("stdpar_nbody_amd", os.path.join(ROOT, "stdpar-nbody_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["stdpar_nbody_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def deep_chain(nb, levels):
    """tests/test_gpu_octree.py::_deep_chain restated: the root cube [-8, 8]^3 and a chain of cells [0, 16 / 2^k]^3, k = 1..levels,
    each with two octants that hold a pair of bodies and the low octant continuing the chain."""
    pts = [(-7.0, -7.0, -7.0), (7.0, 7.0, 7.0)]
    for k in range(1, levels + 1):
        s = 16.0 / 2.0 ** k
        pts += [(0.75 * s, 0.25 * s, 0.25 * s), (0.80 * s, 0.20 * s, 0.20 * s),
                (0.25 * s, 0.75 * s, 0.25 * s), (0.20 * s, 0.80 * s, 0.20 * s)]
    s = 16.0 / 2.0 ** levels
    pts.append((0.1 * s, 0.1 * s, 0.1 * s))
    hs = nb.HostSystem(nb.F64, 3, len(pts))
    hs.x[:] = np.array(pts)
    hs.m[:] = 1.0
    hs.c, hs.dt = C_GRAV, 2.0 ** -7
    return hs


def system(nb, dtype, dim, n):
    if n == 0:
        return deep_chain(nb, CHAIN_LEVELS)
    t = np.float32 if dtype == 0 else np.float64
    rng = np.random.default_rng(6000 + n)
    hs = nb.HostSystem(dtype, dim, n)
    hs.m[:] = (rng.uniform(0.5, 1.5, n) / n).astype(t)
    x = rng.normal(0, 1, (n, 3)).astype(t)[:, :dim]
    if n in CLOSE_PAIR_SIZES:
        i, j = rng.choice(n, 2, replace=False)
        x[j] = x[i]
        x[j, 0] = x[i, 0] + t(2.0 ** -30 if dtype == 1 else 2.0 ** -12)
        assert x[j, 0] != x[i, 0]
    hs.x[:] = x
    hs.dt, hs.c = 2.0 ** -7, C_GRAV
    return hs


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_case(nb, dtype, dim, n, theta, first, count):
    """Everything recorded for one case: a dict of hashes."""
    import torch
    hs = system(nb, dtype, dim, n)
    count = count if n else hs.n
    dev = nb.DeviceSystem.from_host(hs)
    try:
        tt = torch.float32 if dtype == 0 else torch.float64
        where = f"cuda:{dev.device}"
        a, phi = torch.empty((count, dim), dtype=tt, device=where), torch.empty(count, dtype=tt, device=where)
        st, tree = dev.state(first, count), dev.octree
        st.a = a.data_ptr()
        tree.set_walk(1)
        tree.clear(dev.stream)
        tree.compute_bounds(dev.state(), dev.stream)
        tree.insert(dev.state(), dev.stream)
        tree.compute_tree(dev.stream)
        tree.compute_quadrupoles(dev.stream)
        walks = {
            "force": lambda: tree.compute_force(st, theta, dev.stream),
            "force_softened": lambda: tree.compute_softened_force(st, theta, EPS, dev.stream),
            "force_quadrupole": lambda: tree.compute_quadrupole_force(st, theta, dev.stream),
            "potential": lambda: tree.compute_potential(st, theta, phi.data_ptr(), dev.stream),
            "potential_softened": lambda: tree.compute_softened_potential(st, theta, EPS, phi.data_ptr(), dev.stream),
            "potential_quadrupole": lambda: tree.compute_quadrupole_potential(st, theta, phi.data_ptr(), dev.stream),
        }
        out = {}
        for counters in (False, True):
            tree.enable_counters(counters)
            for name in WALKS:
                res = a if name.startswith("force") else phi
                res.fill_(-7.25)
                torch.cuda.synchronize()
                walks[name]()
                dev.sync()
                tree.info(dev.stream)  # raises if the walk set a flag
                out[name + ("+count" if counters else "")] = sha(res.cpu().numpy())
                if counters:
                    out[name + "+counters"] = sha(tree.read_counters(dev.stream)[first:first + count])
        return out
    finally:
        dev.close()


def compact(full):
    """run_case's eighteen hashes as the seven the file holds."""
    assert all(full[w] == full[w + "+count"] for w in WALKS), "the two COUNT instantiations differ"
    assert len({full[w + "+counters"] for w in WALKS}) == 1, "the walks' counters differ"
    return {**{w: full[w] for w in WALKS}, "counters": full[WALKS[0] + "+counters"]}


def expand(rec):
    """The file's seven hashes as the eighteen run_case gives."""
    return {**{w: rec[w] for w in WALKS}, **{w + "+count": rec[w] for w in WALKS}, **{w + "+counters": rec["counters"] for w in WALKS}}


def write(out, path):
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(out[k], sort_keys=True)}" for k in sorted(out)) + "\n}\n")


def main():
    nb = load_package()
    out = {}
    for c in CASES:
        out[case_key(*c)] = compact(run_case(nb, *c))
        print(case_key(*c), flush=True)
    write(out, sys.argv[1] if len(sys.argv) > 1 else OUT)
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()
