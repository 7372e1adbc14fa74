"""CPU: Plummer softening (ABI 2.4) — the three entry points are declared, exported and bound; their argument errors need no GPU;
the softened kernels in the built code object pass the same static checks as their unsoftened twins."""
import ctypes
import importlib.util
import os
import re
import sys

import pytest

from conftest import ROOT

SOFT_SYMBOLS = ("nbody_all_pairs_softened_force", "nbody_calc_energies_softened", "nbody_octree_compute_softened_force")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location(name + "_softening", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_softened_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    L = nb.lib()
    for sym in SOFT_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", text), f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
    assert L.nbody_abi_version() == 2004


def _state(nb, dtype=1, dim=3, n=16):
    st = nb.nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = dtype, dim, n, 0, n
    st.m = st.x = st.v = st.a = st.ao = 0x1000  # never dereferenced: every case below is refused before the device is touched
    return st


# eps values refused in both precisions; plus one whose square underflows each precision (or leaves y^3 = e2^-3/2 infinite)
BAD_EPS = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]
UNDERFLOW = {0: 1e-20, 1: 1e-160}


@pytest.mark.parametrize("dtype", [0, 1])
def test_softened_argument_errors_do_not_need_a_gpu(nb, dtype):
    L = nb.lib()
    k, p = (ctypes.c_double * 1)(), (ctypes.c_double * 1)()
    for eps in BAD_EPS + [UNDERFLOW[dtype]]:
        st = _state(nb, dtype)
        assert L.nbody_all_pairs_softened_force(ctypes.byref(st), ctypes.c_double(eps), None) == 1, eps
        assert b"softening" in L.nbody_last_error(), L.nbody_last_error()
        assert L.nbody_calc_energies_softened(ctypes.byref(st), ctypes.c_double(eps), k, p, None) == 1, eps
        assert b"softening" in L.nbody_last_error()
    # a null state, dim 4, a null tree
    assert L.nbody_all_pairs_softened_force(None, ctypes.c_double(0.1), None) == 1
    assert b"NULL" in L.nbody_last_error()
    assert L.nbody_calc_energies_softened(None, ctypes.c_double(0.1), k, p, None) == 1
    st = _state(nb, dtype, dim=4)
    assert L.nbody_all_pairs_softened_force(ctypes.byref(st), ctypes.c_double(0.1), None) == 1
    assert b"dim" in L.nbody_last_error()
    assert L.nbody_calc_energies_softened(ctypes.byref(st), ctypes.c_double(0.1), k, p, None) == 1
    assert b"dim" in L.nbody_last_error()
    st = _state(nb, dtype)
    assert L.nbody_octree_compute_softened_force(None, ctypes.byref(st), ctypes.c_double(0.5), ctypes.c_double(0.1), None) == 1
    assert b"NULL" in L.nbody_last_error()


def test_softened_k1_passes_the_handoff_checks(nb):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    mod = _tool("check_k1_handoff")
    mod.KERNEL = "all_pairs_softened_sgpr_kernel"
    facts, problems = mod.check(nb.LIB_PATH)
    assert len(facts) >= 1, "no instantiation of all_pairs_softened_sgpr_kernel in the code object"
    assert not problems, "\n".join(problems[:10])
    assert all(p == 2 and loads >= 2 and stores == 2 * loads and swaps == 1 for p, loads, stores, swaps in facts.values()), facts
    tried, missed = mod.self_test(nb.LIB_PATH)
    assert tried >= 10 * len(facts) and missed == 0, f"{missed} of {tried} mutations went unreported"


def test_softened_kernels_keep_their_smem_pipeline(nb):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    mod = _tool("check_smem_pipeline")
    mod.HAND_WRITTEN = tuple(mod.HAND_WRITTEN) + ("all_pairs_softened_sgpr_kernel",)
    funcs = mod.functions(mod.disassemble(nb.LIB_PATH))
    soft = {n: c for n, c in funcs.items() if ("all_pairs_softened_sgpr_kernel" in n or "softened_potential_sgpr_kernel" in n) and c}
    assert len(soft) >= 2, sorted(soft)
    loads, problems = 0, []
    for name, code in soft.items():
        n, p = mod.check_function(name, code)
        loads += n
        problems += p
    assert loads >= 2 * len(soft), loads
    assert not problems, "\n".join(problems[:10])
    loads, problems = mod.check(nb.LIB_PATH)
    assert not problems, "\n".join(problems[:10])


def test_softened_kernels_have_no_isa_hazards(nb):
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    mod = _tool("check_isa_hazards")
    total, lanes, problems = mod.check(nb.LIB_PATH)
    assert not problems, "\n".join(problems[:10])


def test_softened_k1_runs_at_the_waves_of_its_twin(nb):
    """Same occupancy as the unsoftened scalar-stream K1 of the same (T, D, R, JS): the softened pair adds no register pressure."""
    mod = _tool("kernel_resources")
    ks = mod.kernels(nb.LIB_PATH)
    names = mod.demangle([k["symbol"].replace(".kd", "") for k in ks])

    def waves(k):
        v, a = int(k.get("vgpr_count", 0)), int(k.get("agpr_count", 0))
        tot = (v + a + 7) // 8 * 8
        by_v = min(8, 512 // tot) if tot else 8
        sg = int(k.get("sgpr_count", 0))
        return min(by_v, min(8, 800 // ((sg + 15) // 16 * 16 + 16)))

    soft, base = {}, {}
    for k, n in zip(ks, names):
        m = re.search(r"nbody::(all_pairs_softened_sgpr_kernel|all_pairs_force_sgpr_kernel)<(\w+), (\d), (\d), (\d)(, 0)?>", n)
        if not m:
            continue
        key = m.group(2, 3, 4, 5)
        (soft if m.group(1) == "all_pairs_softened_sgpr_kernel" else base)[key] = waves(k)
    assert len(soft) == 32 and set(soft) <= set(base), (len(soft), sorted(soft))
    worse = {k: (soft[k], base[k]) for k in soft if soft[k] < base[k]}
    assert not worse, worse


def test_existing_kernels_unchanged_by_the_softened_forms(nb):
    """The compare tool itself: a library compared with itself is identical kernel for kernel."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    mod = _tool("compare_kernel_isa")
    common, differ, gone, added = mod.compare(nb.LIB_PATH, nb.LIB_PATH)
    assert len(common) > 200 and not differ and not gone and not added


def test_cli_refuses_bad_softening_before_opening_a_device(nb):
    import subprocess
    cli = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")
    assert os.path.exists(cli)
    for args, word in ((["--softening", "-1"], "softening"), (["--softening", "nan"], "softening"), (["--softening", "x"], "softening"),
                       (["--softening", "0.1", "--algorithm", "bvh"], "octree"),
                       (["--algorithm", "all-pairs-collapsed", "--softening", "0.1"], "all-pairs")):
        r = subprocess.run([cli, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0, args
        assert word in r.stderr, (args, r.stderr)
        assert "Starting simulation" not in r.stdout
    help_text = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "softening" not in help_text
