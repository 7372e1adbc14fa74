#!/usr/bin/env python3
"""The bits of the direct-sum Hermite integrators (orders 4 and 6, and the block time steps of order 4) as sha256 hashes:
tests/golden/hermite_bits.json, compared with == by tests/test_gpu_hermite_bits.py.  These kernels promise a rounding order that is a
function of sz alone; the fixture holds a restructuring of them to that promise.  It was written once, on an MI355X, from the code as
it stood before the two orders were folded onto one tiled pair-sum skeleton, and is not regenerated from later code: a mismatch is a
bug in the code (floating-point contraction, an operand order in the hand-off), never a reason to run this script again.

Inputs are closed-form and exactly representable in float and double (no random numbers, no library can change them):
    x[i][k] = ((i 2654435761 + k 40503 + 12345) mod 2^20) / 2^20 - 1/2
    v[i][k] = (((i 2246822519 + k 25171 + 54321) mod 2^20) / 2^20 - 1/2) / 4
    m[i]    = (8 + i mod 7) / (8 n), rounded to the type;        c = 1, dt = 2^-7, eps = 2^-4.
Sizes: the smallest on either side of every regime of the launch plan (one tile | two tiles, and for order 6 two chunks | a ragged tile
| several tiles per chunk with a ragged last chunk | two chunks of 128 tiles | two targets per lane with a ragged tile), each in
{double, float} x {3D, 2D}.  Recorded per case:
    h4     x, v, a, the jerk and the predicted x, v after the start and after 3 steps;
    h6     x, v, a and the six nbody_hermite6_read arrays after the start and after 3 steps;
    block  (n <= 5889, eta = 0.02, max_level = 6) x, v, a, the jerk, the levels and tau after block_start and after two block_advance,
           with the (block steps, body steps) each advance returned.

    python tests/golden/generate_hermite_bits.py        (needs the GPU)
"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hermite_bits.json")

SIZES = [2, 257, 1000, 5889, 65473, 65537]
BLOCK_SIZES = [257, 1000, 5889]
EPS, DT, C_GRAV = 2.0 ** -4, 2.0 ** -7, 1.0
ETA, MAX_LEVEL, NSTEPS, NADVANCE = 0.02, 6, 3, 2
CASES = [(dtype, dim, n) for n in SIZES for dtype in (1, 0) for dim in (3, 2)]


def case_key(dtype, dim, n):
    return f"{'f64' if dtype == 1 else 'f32'}-{dim}d-n{n}"


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
    i = np.arange(n, dtype=np.uint64)[:, None]
    k = np.arange(dim, dtype=np.uint64)[None, :]
    frac = lambda mi, mk, add: ((i * np.uint64(mi) + k * np.uint64(mk) + np.uint64(add)) % np.uint64(1 << 20)).astype(np.float64) / 2.0 ** 20 - 0.5
    hs = nb.HostSystem(dtype, dim, n)
    x, v = frac(2654435761, 40503, 12345), frac(2246822519, 25171, 54321) * 0.25
    hs.x[:], hs.v[:] = x.astype(t), v.astype(t)
    assert np.array_equal(hs.x.astype(np.float64), x) and np.array_equal(hs.v.astype(np.float64), v)  # exactly representable
    hs.m[:] = ((8 + np.arange(n) % 7) / (8.0 * n)).astype(t)
    hs.dt, hs.c = DT, C_GRAV
    return hs


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def hashes(names, arrays):
    arrays = list(arrays)
    assert len(names) == len(arrays)
    return {name: sha(a) for name, a in zip(names, arrays)}


def xva(dev):
    out = dev.download()
    return [out.x, out.v, out.a]


def run_case(nb, dtype, dim, n):
    """Everything recorded for one (dtype, dim, n): a dict of hashes and integers."""
    hs = system(nb, dtype, dim, n)
    rec = {}

    names4 = ("x", "v", "a", "jerk", "xp", "vp")
    snap4 = lambda dev: hashes(names4, xva(dev) + [dev.hermite.read(w, dev.stream) for w in range(3)])
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite_start(EPS)
    rec["h4"] = {"start": snap4(dev)}
    for _ in range(NSTEPS):
        dev.hermite_step(EPS)
    rec["h4"]["steps"] = snap4(dev)
    dev.close()

    names6 = ("x", "v", "a", "jerk", "snap", "crackle", "xp", "vp", "ap")
    snap6 = lambda dev: hashes(names6, xva(dev) + [dev.hermite6_read(w) for w in range(6)])
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite6_start(EPS)
    rec["h6"] = {"start": snap6(dev)}
    for _ in range(NSTEPS):
        dev.hermite6_step(EPS)
    rec["h6"]["steps"] = snap6(dev)
    dev.close()

    if n in BLOCK_SIZES:
        namesb = ("x", "v", "a", "jerk", "levels", "tau")
        snapb = lambda dev: hashes(namesb, xva(dev) + [dev.hermite_jerk()] + list(dev.hermite_block_levels()))
        dev = nb.DeviceSystem.from_host(hs)
        dev.hermite_block_start(EPS, ETA, MAX_LEVEL)
        rec["block"] = {"start": snapb(dev)}
        counts = [[int(c) for c in dev.hermite_block_advance(EPS, ETA)] for _ in range(NADVANCE)]
        rec["block"]["advance"] = snapb(dev)
        rec["block"]["counts"] = counts
        dev.close()
    return rec


def main():
    nb = load_package()
    out = {}
    for dtype, dim, n in CASES:
        out[case_key(dtype, dim, n)] = run_case(nb, dtype, dim, n)
        print(case_key(dtype, dim, n), out[case_key(dtype, dim, n)].get("block", {}).get("counts", ""), flush=True)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", len(out), "cases")


if __name__ == "__main__":
    main()
