"""CPU: octree potentials and energies (additive under ABI 2.4) — the four entry points are declared, exported and bound; their argument
errors need no GPU; the CLI refuses --tree-energy where it does not apply before a device is opened; the new walks are in the code
object, pass the static checks and keep the force walk's LDS."""
import ctypes
import importlib.util
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

POT_SYMBOLS = ("nbody_octree_compute_potential", "nbody_octree_compute_softened_potential",
               "nbody_octree_compute_quadrupole_potential", "nbody_octree_calc_energies")
POT_KERNELS = ("ot_potential_kernel", "ot_potential_softened_kernel", "ot_potential_quadrupole_kernel")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CLI = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location(name + "_tree_energy", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_tree_energy_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    L = nb.lib()
    for sym in POT_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", text), f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
        assert getattr(L, sym).argtypes, f"{sym} has no argtypes"
    assert L.nbody_abi_version() == 2004
    for meth in ("compute_potential", "compute_softened_potential", "compute_quadrupole_potential", "calc_energies"):
        assert callable(getattr(nb.Octree, meth))
    for meth in ("octree_potential", "octree_energies"):
        assert callable(getattr(nb.DeviceSystem, meth))


def _state(nb, dtype=1, dim=3, n=16):
    st = nb.nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = dtype, dim, n, 0, n
    st.m = st.x = st.v = st.a = st.ao = 0x1000  # never dereferenced: every case below is refused before the device is touched
    return st


def _err(L):
    return L.nbody_last_error()


def test_potential_argument_errors_do_not_need_a_gpu(nb):
    L = nb.lib()
    st = _state(nb)
    phi = ctypes.c_void_p(0x2000)
    calls = (lambda t, s, p: L.nbody_octree_compute_potential(t, s, 0.5, p, None),
             lambda t, s, p: L.nbody_octree_compute_softened_potential(t, s, 0.5, 0.05, p, None),
             lambda t, s, p: L.nbody_octree_compute_quadrupole_potential(t, s, 0.5, p, None))
    for call in calls:
        assert call(None, ctypes.byref(st), phi) == 1
        assert b"nbody_octree is NULL" in _err(L)
        # the state and phi are checked before the tree
        assert call(None, None, phi) == 1
        assert b"nbody_state is NULL" in _err(L)
        assert call(None, ctypes.byref(_state(nb, dim=4)), phi) == 1
        assert b"bad dim" in _err(L)
        assert call(None, ctypes.byref(_state(nb, dtype=7)), phi) == 1
        assert b"bad dtype" in _err(L)
        assert call(None, ctypes.byref(st), None) == 1
        assert b"phi is NULL" in _err(L)
    for eps in (0.0, -1.0, float("inf"), float("nan"), 1e-200):
        assert L.nbody_octree_compute_softened_potential(None, ctypes.byref(st), 0.5, eps, phi, None) == 1
        assert b"softening length" in _err(L), eps
    assert L.nbody_octree_compute_softened_potential(None, ctypes.byref(_state(nb, dtype=0)), 0.5, 1e-20, phi, None) == 1
    assert b"softening length" in _err(L)  # e2 below float's bound


def test_calc_energies_argument_errors_do_not_need_a_gpu(nb):
    L = nb.lib()
    ke, pe = ctypes.c_double(), ctypes.c_double()
    st = _state(nb)

    def call(t=None, s=ctypes.byref(st), theta=0.5, eps=0.0, quad=0, k=ctypes.byref(ke), p=ctypes.byref(pe)):
        return L.nbody_octree_calc_energies(t, s, theta, eps, quad, k, p, None)

    assert call() == 1
    assert b"nbody_octree is NULL" in _err(L)
    assert call(s=None) == 1
    assert b"nbody_state is NULL" in _err(L)
    assert call(k=None) == 1 and b"NULL output" in _err(L)
    assert call(p=None) == 1 and b"NULL output" in _err(L)
    for eps in (-1.0, float("inf"), float("nan")):
        assert call(eps=eps) == 1
        assert b"eps" in _err(L), eps
    assert call(eps=1e-200) == 1 and b"softening length" in _err(L)
    assert call(eps=0.05, quad=1) == 1
    assert b"cannot be combined" in _err(L)
    shard = _state(nb)
    shard.first, shard.count = 4, 8
    assert call(s=ctypes.byref(shard)) == 1
    assert b"whole system" in _err(L)


def test_octree_energies_refuses_softening_with_quadrupole(nb):
    class Dev:  # refused before the system is touched
        pass

    with pytest.raises(ValueError, match="quadrupole"):
        nb.DeviceSystem.octree_energies(Dev(), 0.5, softening=0.1, quadrupole=True)
    with pytest.raises(ValueError, match="quadrupole"):
        nb.DeviceSystem.octree_potential(Dev(), 0.5, softening=0.1, quadrupole=True)


@pytest.mark.parametrize("args, words", [
    (["--algorithm", "bvh", "--tree-energy", "--save", "energy"], ("--tree-energy", "octree")),
    (["--tree-energy", "--algorithm", "all-pairs", "--save", "all"], ("--tree-energy", "octree")),
    (["--tree-energy", "--algorithm", "all-pairs-collapsed", "--save", "energy"], ("--tree-energy", "octree")),
    (["--tree-energy"], ("--tree-energy", "--save")),
    (["--tree-energy", "--save", "pos"], ("--tree-energy", "--save")),
    (["--algorithm", "octree", "--save", "none", "--tree-energy"], ("--tree-energy", "--save")),
])
def test_cli_refuses_tree_energy_before_opening_a_device(args, words):
    assert os.path.exists(CLI)
    r = subprocess.run([CLI, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0, args
    for w in words:
        assert w in r.stderr, (args, r.stderr)
    assert "Starting simulation" not in r.stdout


def test_cli_help_does_not_mention_tree_energy():
    help_text = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "Help:" in help_text and "tree-energy" not in help_text


def test_potential_kernels_are_in_the_code_object(nb):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    mod = _tool("compare_kernel_isa")
    demangled = _tool("kernel_resources").demangle(sorted(mod.kernels(nb.LIB_PATH)))
    total = 0
    for kern in POT_KERNELS:
        found = [n for n in demangled if f"nbody::{kern}<" in n]
        assert len(found) == 8, (kern, found)  # 2 dtypes x 2 dims x counters on / off
        total += len(found)
    assert total == 24


def test_potential_kernels_have_no_isa_hazards(nb):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    mod = _tool("check_isa_hazards")
    total, lanes, problems = mod.check(nb.LIB_PATH)
    assert not problems, "\n".join(problems[:10])
    mod = _tool("check_smem_pipeline")
    loads, problems = mod.check(nb.LIB_PATH)
    assert not problems, "\n".join(problems[:10])


def test_potential_walks_keep_the_lds_of_the_force_walk(nb):
    """The potential walks keep one scalar instead of acc[dim]: the per-body stack in LDS is the force walk's."""
    mod = _tool("kernel_resources")
    ks = mod.kernels(nb.LIB_PATH)
    names = mod.demangle([k["symbol"].replace(".kd", "") for k in ks])
    lds = {}
    for k, n in zip(ks, names):
        m = re.search(r"nbody::(ot_potential_kernel|ot_potential_softened_kernel|ot_potential_quadrupole_kernel|ot_force_kernel)"
                      r"<(\w+), (\d), (\w+)>", n)
        if m:
            lds[m.group(1, 2, 3, 4)] = int(k.get("group_segment_fixed_size", -1))
    base = {key[1:]: v for key, v in lds.items() if key[0] == "ot_force_kernel"}
    assert len(base) == 8
    for kern in POT_KERNELS:
        pot = {key[1:]: v for key, v in lds.items() if key[0] == kern}
        assert set(pot) == set(base), (kern, sorted(pot))
        assert all(pot[k] == base[k] for k in pot), (kern, pot, base)
