"""CPU: the host plan of the octree (csrc/octree_plan.hpp) — tools/octree_plan_check.cpp, compiled for the host alone, sweeps the
plan's invariants over the sizes (grids, every buffer against the indices its launches produce), pins the multipole routes, the
one-block thresholds, the capacity floor and the ISA walk's reach at both sides of each boundary, and walks the truth table of the
phase flags.  No device is opened."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_plan_invariants_pinned_routes_and_phases(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = tmp_path / "octree_plan_check"
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "--offload-host-only", "-I", os.path.join(ROOT, "stdpar-nbody_amd", "csrc"), "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "octree_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (r.stdout, r.stderr)
