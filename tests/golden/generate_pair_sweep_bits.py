#!/usr/bin/env python3
"""The bits of the two all-pairs diagnostics, nbody_neighbours_* and nbody_knn_*, as sha256 hashes: tests/golden/pair_sweep_bits.json,
compared with == by tests/test_gpu_pair_sweep_bits.py.  Both promise results that are a function of the input and of sz alone (a fixed
rounding order of the potential, an exact tie rule of the selections); the fixture holds a restructuring of them to that promise.  It
was written once, on an MI355X, from the code as it stood before the two files shared csrc/pair_sweep.hpp, and is not regenerated from
later code: a mismatch is a bug in the code (a changed operation, contraction, merge order or index bound), never a reason to run
this script again.

Inputs are seeded NumPy draws (no library of the project is involved): seed 4000 + n, m uniform in [0.5, 1.5) / n, x normal, all
rounded to the type; then, where n allows, min(n // 4, 9) bodies moved onto the integer lattice {0, 1, 2}^2 (x {0} in 3D; many exactly
equal d2: the tie rule), min(n // 8, 4) bodies moved exactly onto another body and one more onto the first of those pairs (a triple;
d2 = 0, and for the potential the m / eps term).  c = 1, eps = 2^-4.
Sizes: the smallest that reach every branch of the shared sweep — 1 (no neighbour), 2, 65 (a block whose own targets are not in slice
0; one slice that is both own and padded), 257 (two tiles, two chunks), 5889 (several tiles per chunk), 65537 (two targets per lane
in neighbours, the last tile padded) — each in {double, float} x {3D, 2D}; for neighbours also 65535 and 65536, either side of the
switch to two targets per lane; for kNN k = 6 at every size and k in {1, 4, 16} at 257 and 5889 (the three list capacities, k equal
to the capacity, and k = 1 with its NaN summary).  Recorded per case:
    nb     phi, nn, nnd2 and the closest-pair record (i, j as uint32, d2 of T);
    knn    idx, d2, rho and the summary (x_dc, r_c, rho_c of T) as raw bytes: a NaN hashes like anything else.

    python tests/golden/generate_pair_sweep_bits.py        (needs the GPU)
"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pair_sweep_bits.json")

SIZES = [1, 2, 65, 257, 5889, 65537]
NB_SIZES = SIZES + [65535, 65536]
K_ALL, K_MORE, K_MORE_SIZES = 6, (1, 4, 16), (257, 5889)
EPS, C_GRAV = 2.0 ** -4, 1.0
TYPES = [(dtype, dim) for dtype in (1, 0) for dim in (3, 2)]
# (kind, dtype, dim, n, k); k = 0 for neighbours
CASES = ([("nb", dtype, dim, n, 0) for n in sorted(NB_SIZES) for dtype, dim in TYPES] +
         [("knn", dtype, dim, n, K_ALL) for n in SIZES for dtype, dim in TYPES] +
         [("knn", dtype, dim, n, k) for n in K_MORE_SIZES for k in K_MORE for dtype, dim in TYPES])


def case_key(kind, dtype, dim, n, k):
    return f"{kind}-{'f64' if dtype == 1 else 'f32'}-{dim}d-n{n}" + (f"-k{k}" if kind == "knn" else "")


def load_package():
    if "stdpar_nbody_amd" in sys.modules:
        return sys.modules["stdpar_nbody_amd"]
    spec = importlib.util.spec_from_file_location("stdpar_nbody_amd", os.path.join(ROOT, "stdpar-nbody_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["stdpar_nbody_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def system(nb, dtype, dim, n):
    t = np.float32 if dtype == 0 else np.float64
    rng = np.random.default_rng(4000 + n)
    hs = nb.HostSystem(dtype, dim, n)
    hs.m[:] = (rng.uniform(0.5, 1.5, n) / n).astype(t)
    x = rng.normal(0, 1, (n, 3)).astype(t)[:, :dim]
    nlat, ndup = min(n // 4, 9), min(n // 8, 4)
    moved = rng.choice(n, nlat + 2 * ndup + (1 if ndup else 0), replace=False)  # distinct bodies, in no index order
    lat, src, dst = moved[:nlat], moved[nlat:nlat + ndup], moved[nlat + ndup:]
    j = np.arange(nlat)
    x[lat] = np.stack([j % 3, j // 3, 0 * j], axis=1)[:, :dim].astype(t)
    x[dst[:ndup]] = x[src]
    if ndup:
        x[dst[ndup]] = x[src[0]]
    hs.x[:] = x
    hs.dt, hs.c = 2.0 ** -7, C_GRAV
    return hs


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_case(nb, kind, dtype, dim, n, k):
    """Everything recorded for one case: a dict of hashes."""
    dev = nb.DeviceSystem.from_host(system(nb, dtype, dim, n))
    try:
        if kind == "nb":
            h = dev.neighbours_handle
            h.compute(dev.state(), EPS, dev.stream)
            i, j, d2 = h.closest_pair(dev.stream)
            return {"phi": sha(h.read(0, dev.stream)), "nn": sha(h.read(1, dev.stream)), "nnd2": sha(h.read(2, dev.stream)),
                    "closest": sha(np.array([i, j], np.uint32), d2)}
        h = dev.knn_handle(k)
        h.compute(dev.state(), dev.stream)
        xc, rc, rhoc = h.density_centre(dev.stream)
        return {"idx": sha(h.read(0, dev.stream)), "d2": sha(h.read(1, dev.stream)), "rho": sha(h.read(2, dev.stream)),
                "summary": sha(xc, rc, rhoc)}
    finally:
        dev.close()


def main():
    nb = load_package()
    out = {}
    for c in CASES:
        out[case_key(*c)] = run_case(nb, *c)
        print(case_key(*c), flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()
