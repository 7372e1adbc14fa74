"""CPU: octree quadrupole moments (additive under ABI 2.4) — the three entry points are declared, exported and bound; their argument
errors need no GPU; the CLI refuses --quadrupole where it does not apply before a device is opened; the new kernels are in the code
object and pass the static checks."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

QUAD_SYMBOLS = ("nbody_octree_compute_quadrupoles", "nbody_octree_compute_quadrupole_force", "nbody_octree_read_root_quadrupole")
QUAD_KERNELS = ("ot_quadrupole_level_kernel", "ot_quadrupole_ranks_level_kernel", "ot_quadrupole_deep_kernel",
                "ot_force_quadrupole_kernel")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CLI = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location(name + "_quadrupole", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_quadrupole_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    L = nb.lib()
    for sym in QUAD_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", text), f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
    assert L.nbody_abi_version() == 2004
    for meth in ("compute_quadrupoles", "compute_quadrupole_force", "read_root_quadrupole"):
        assert callable(getattr(nb.Octree, meth))


def _state(nb, dtype=1, dim=3, n=16):
    st = nb.nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = dtype, dim, n, 0, n
    st.m = st.x = st.v = st.a = st.ao = 0x1000  # never dereferenced: every case below is refused before the device is touched
    return st


def test_quadrupole_argument_errors_do_not_need_a_gpu(nb):
    L = nb.lib()
    out = (ctypes.c_double * 6)()
    assert L.nbody_octree_compute_quadrupoles(None, None) == 1
    assert b"NULL" in L.nbody_last_error()
    st = _state(nb)
    assert L.nbody_octree_compute_quadrupole_force(None, ctypes.byref(st), ctypes.c_double(0.5), None) == 1
    assert b"nbody_octree is NULL" in L.nbody_last_error()
    assert L.nbody_octree_read_root_quadrupole(None, out, None) == 1
    assert b"NULL" in L.nbody_last_error()
    # the state is checked before the tree: each case below reports its own check, not the NULL tree
    assert L.nbody_octree_compute_quadrupole_force(None, None, ctypes.c_double(0.5), None) == 1
    assert b"nbody_state is NULL" in L.nbody_last_error()
    st = _state(nb, dim=4)
    assert L.nbody_octree_compute_quadrupole_force(None, ctypes.byref(st), ctypes.c_double(0.5), None) == 1
    assert b"bad dim" in L.nbody_last_error()
    st = _state(nb, dtype=7)
    assert L.nbody_octree_compute_quadrupole_force(None, ctypes.byref(st), ctypes.c_double(0.5), None) == 1
    assert b"bad dtype" in L.nbody_last_error()


def test_octree_force_refuses_softening_with_quadrupole(nb):
    class Dev:  # octree_force refuses the combination before it touches the system
        pass

    with pytest.raises(ValueError, match="quadrupole"):
        nb.DeviceSystem.octree_force(Dev(), 0.5, softening=0.1, quadrupole=True)


@pytest.mark.parametrize("args, words", [
    (["--algorithm", "bvh", "--quadrupole"], ("octree",)),
    (["--quadrupole", "--algorithm", "all-pairs"], ("octree",)),
    (["--quadrupole", "--algorithm", "all-pairs-collapsed"], ("octree",)),
    (["--quadrupole", "--softening", "0.1"], ("--quadrupole", "--softening")),
    (["--algorithm", "octree", "--softening", "0.1", "--quadrupole"], ("--quadrupole", "--softening")),
])
def test_cli_refuses_quadrupole_before_opening_a_device(args, words):
    assert os.path.exists(CLI)
    r = subprocess.run([CLI, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0, args
    for w in words:
        assert w in r.stderr, (args, r.stderr)
    assert "Starting simulation" not in r.stdout


def test_cli_help_does_not_mention_quadrupole():
    help_text = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "Help:" in help_text and "quadrupole" not in help_text


def test_quadrupole_kernels_are_in_the_code_object(nb):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    mod = _tool("compare_kernel_isa")
    names = mod.kernels(nb.LIB_PATH)
    demangled = _tool("kernel_resources").demangle(sorted(names))
    for kern in QUAD_KERNELS:
        found = [n for n in demangled if f"nbody::{kern}<" in n]
        # 2 dtypes x 2 dims, and the walk once with and once without counters
        assert len(found) == (8 if kern == "ot_force_quadrupole_kernel" else 4), (kern, found)


def test_quadrupole_kernels_have_no_isa_hazards(nb):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    mod = _tool("check_isa_hazards")
    total, lanes, problems = mod.check(nb.LIB_PATH)
    assert not problems, "\n".join(problems[:10])
    mod = _tool("check_smem_pipeline")
    loads, problems = mod.check(nb.LIB_PATH)
    assert not problems, "\n".join(problems[:10])


def test_quadrupole_walk_keeps_the_lds_of_the_monopole_walk(nb):
    """The quadrupole walk adds registers, not LDS: its per-body stack is the monopole walk's."""
    mod = _tool("kernel_resources")
    ks = mod.kernels(nb.LIB_PATH)
    names = mod.demangle([k["symbol"].replace(".kd", "") for k in ks])
    lds = {}
    for k, n in zip(ks, names):
        m = re.search(r"nbody::(ot_force_quadrupole_kernel|ot_force_kernel)<(\w+), (\d), (\w+)>", n)
        if m:
            lds[m.group(1, 2, 3, 4)] = int(k.get("group_segment_fixed_size", -1))
    quad = {key[1:]: v for key, v in lds.items() if key[0] == "ot_force_quadrupole_kernel"}
    base = {key[1:]: v for key, v in lds.items() if key[0] == "ot_force_kernel"}
    assert len(quad) == 8 and set(quad) == set(base), (sorted(quad), sorted(base))
    assert all(quad[k] == base[k] for k in quad), (quad, base)
