"""SHA-256 of the whole state of a run of block time steps, step by step, for the three integrators that take them: what two builds
of the library must agree on bit for bit when a change is not meant to move a result.  It uses the Python binding alone.
    python tools/block_state_digest.py > digest.txt          (then: diff the output of two builds)
Cases: fourth-order Hermite (f32, f64) x (2D, 3D), sixth-order Hermite f64 x (2D, 3D), octree leapfrog (theta = 0.5) (f32, f64) x
(2D, 3D), each at N = 257 (one schedule strip) and 4097 (two strips, a nonzero offset into the second), and one f64 3D case of each
integrator at N = 65537 (seventeen strips, two targets per lane).  Galaxy workload, eps = 0.05, max_level = 6, the eta of
tests/test_gpu_*_block.py, and dt_max a power of two that spreads the bodies over the levels (the galaxy's bodies ask the Hermite
criterion for steps of 40 .. 400 and the octree's for 2 .. 10: dt_max = 1024 and 64 put them on levels 1 .. 5 and 1 .. 6; with every
body on level 0 the schedule would have nothing to do).  After the start and after every one of 24 block steps one line
    case  step  n_act  tau_next  sha256(x, v, a, levels, tau, the active list, then the jerk / snap / crackle where the integrator has them)
and one line per case over all of its steps, with the number of bodies on each level at the end."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_package  # noqa: E402

EPS, LEVELS, STEPS, THETA = 0.05, 6, 24, 0.5
DT_MAX = {"hermite4": 1024.0, "hermite6": 1024.0, "octree": 64.0}
ETA = {"hermite4": (0.3, 0.4), "hermite6": (0.3, 0.4), "octree": (0.05, 0.05)}  # (start, step)


def cases(nb):
    for n in (257, 4097):
        for kind, dtypes in (("hermite4", (nb.F32, nb.F64)), ("hermite6", (nb.F64,)), ("octree", (nb.F32, nb.F64))):
            for dtype in dtypes:
                for dim in (2, 3):
                    yield kind, dtype, dim, n
    for kind in ("hermite4", "hermite6", "octree"):
        yield kind, nb.F64, 3, 65537


def run(nb, kind, dtype, dim, n):
    hs = nb.build_model(dtype, dim, "galaxy", n)
    hs.dt = DT_MAX[kind]
    dev = nb.DeviceSystem.from_host(hs)
    eta_start, eta = ETA[kind]
    if kind == "hermite4":
        dev.hermite_block_start(EPS, eta_start, LEVELS)
        step, levels, active = (lambda: dev.hermite_block_step(EPS, eta)), dev.hermite_block_levels, dev.hermite_block_active
        extra = lambda: [dev.hermite_jerk()]
    elif kind == "hermite6":
        dev.hermite6_block_start(EPS, eta_start, LEVELS)
        step, levels, active = (lambda: dev.hermite6_block_step(EPS, eta)), dev.hermite6_block_levels, dev.hermite6_block_active
        extra = lambda: [dev.hermite6_read(w) for w in (0, 1, 2)]
    else:
        dev.octree_block_start(THETA, EPS, eta_start, LEVELS)
        step, levels, active = (lambda: dev.octree_block_step(THETA, EPS, eta)), dev.octree_block_levels, dev.octree_block_active
        extra = lambda: []
    name = f"{kind} {'f32' if dtype == nb.F32 else 'f64'} {dim}D N={n}"
    whole = hashlib.sha256()
    n_act = tau_next = 0
    for k in range(STEPS + 1):
        if k:
            n_act, tau_next = step()
        out = dev.download()
        lev, tau = levels()
        parts = [out.x, out.v, out.a, lev, tau] + ([active(n_act)] if k else []) + extra()
        h = hashlib.sha256()
        for p in parts:
            h.update(p.tobytes())
        whole.update(h.digest())
        print(f"{name:28s} step {k:2d}  n_act {n_act:6d}  tau_next {tau_next:3d}  {h.hexdigest()}")
    print(f"{name:28s} all {STEPS} steps, levels {np.bincount(lev, minlength=LEVELS + 1).tolist()}  {whole.hexdigest()}", flush=True)
    dev.close()


def main():
    nb = load_package()
    for case in cases(nb):
        run(nb, *case)


if __name__ == "__main__":
    main()
