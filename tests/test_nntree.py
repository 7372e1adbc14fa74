"""CPU: the tree-pruned exact kNN (NBODY_KNN_TREE of nbody_knn_*, csrc/nntree.inc) — the two new entry points are declared, exported
and bound and the ABI version is unchanged; the argument errors of nbody_knn_create_method come in the header's order without a GPU;
the CLI refuses --density-tree without --save-density before a device is opened; and in the built code object every nntree_* kernel
is free of scratch, the walk is free of divides, reciprocals and roots and exists per (type, dimension, list capacity).
What the method computes is held to the all-pairs method bit for bit in tests/test_gpu_nntree.py, and its rules to brute force in
tests/test_nntree_model.py."""
import ctypes
import importlib.util
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("nbody_knn_create_method", "nbody_knn_method")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CLI = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")


def test_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nbody_[a-z_0-9]+)\s*\(", text))
    L = nb.lib()
    for sym in SYMBOLS:
        assert sym in declared, f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
        assert getattr(L, sym).argtypes is not None, f"{sym} has no argtypes"
    assert L.nbody_abi_version() == 2004  # additive: the version stays
    assert re.search(r"#define\s+NBODY_KNN_ALL_PAIRS\s+0\b", text) and re.search(r"#define\s+NBODY_KNN_TREE\s+1\b", text)
    assert nb.Knn.METHODS == {"all-pairs": 0, "tree": 1}
    assert isinstance(nb.Knn.method, property)
    import inspect
    assert inspect.signature(nb.Knn.__init__).parameters["method"].default == "all-pairs"
    for name in ("knn_handle", "knn", "knn_compute", "local_density", "density_centre"):
        assert inspect.signature(getattr(nb.DeviceSystem, name)).parameters["method"].default == "all-pairs", name
    with pytest.raises(ValueError):
        nb.Knn(1, 3, 16, 6, method="octree")  # refused before the library is asked


def test_create_method_argument_errors_come_in_order_and_need_no_gpu(nb):
    L = nb.lib()
    err = lambda: L.nbody_last_error()
    f = L.nbody_knn_create_method
    h = ctypes.c_void_p()
    # out NULL, dtype, dim, n, k, method — each earlier error wins over every later one
    assert f(None, 7, 4, 0, 0, 9, 0) == 1 and b"out is NULL" in err()
    assert f(ctypes.byref(h), 7, 4, 0, 0, 9, 0) == 1 and b"dtype" in err()
    assert f(ctypes.byref(h), 1, 4, 0, 0, 9, 0) == 1 and b"dim" in err()
    assert f(ctypes.byref(h), 1, 3, 0, 0, 9, 0) == 1 and b"2^28" in err()
    assert f(ctypes.byref(h), 0, 2, (1 << 28) + 1, 0, 9, 0) == 1 and b"2^28" in err()
    for k in (0, -1, 17, 1 << 20):
        for method in (0, 1, 9):
            assert f(ctypes.byref(h), 1, 3, 16, k, method, 0) == 1, (k, method)
            assert b"1 <= k <= 16" in err(), err()
    for method in (-1, 2, 9, 1 << 20):
        for dtype, dim in ((1, 3), (0, 2)):
            assert f(ctypes.byref(h), dtype, dim, 16, 6, method, 0) == 1, method
            assert b"method" in err() and b"k <=" not in err(), err()
    assert not h.value
    # nbody_knn_method of NULL: -1 and a message
    assert L.nbody_knn_method(None) == -1
    assert b"nbody_knn is NULL" in err()


REFUSALS = [
    (["--density-tree"], "--density-tree needs --save-density K."),
    (["--algorithm", "octree", "--density-tree", "--save", "pos"], "--density-tree needs --save-density K."),
    (["--density-tree", "--algorithm", "bvh", "--precision", "double"], "--density-tree needs --save-density K."),
    (["--density-tree", "--save-density", "1"], "--save-density needs a neighbour count K in 2 .. 16."),
    (["--save-density", "6", "--density-tree", "--gpus", "1"], "--save-density runs on one GPU: it cannot be combined with --gpus."),
]


@pytest.mark.parametrize("args,line", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_cli_refuses_before_opening_a_device(args, line, tmp_path):
    assert os.path.exists(CLI)
    r = subprocess.run([CLI, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode != 0, args
    assert line in r.stderr.splitlines(), (args, r.stderr)
    assert "HIP" not in r.stderr and "hip" not in r.stderr, r.stderr
    assert "Starting simulation" not in r.stdout
    assert not os.path.exists(tmp_path / "density.bin")


def test_cli_help_does_not_mention_the_flag():
    got = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert got == open(os.path.join(ROOT, "tests", "golden", "help_d3.txt"), "rb").read()
    assert b"density" not in got


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name + "_nntree", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_nntree_kernels_do_not_spill_and_the_walk_has_no_divide_or_root(nb):
    """Every nntree_*_kernel: private segment 0, no scratch_ instruction; none has `knn_` in its name (the all-pairs kernels are
    counted by that prefix).  The walk has no LDS either — its lists are registers —, no v_div_*, v_rcp, v_rsq or v_sqrt, and exists
    for (float, double) x (2, 3) x capacity (4, 8, 16); the finish likewise; bounds, keys, gather and upper exist per (type, dimension)."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    kr = _load_tool("kernel_resources")
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    seen = {"bounds": set(), "keys": set(), "gather": set(), "upper": set(), "walk": set(), "finish": set()}
    for k, n in zip(ks, names):
        if "nntree_" not in n:
            continue
        assert "knn_" not in n, n
        m = re.search(r"nbody::nntree_(\w+)_kernel<(float|double), (\d+)(?:, (\d+))?>", n)
        assert m and m.group(1) in seen, f"an nntree kernel with an unexpected name: {n}"
        assert int(k.get("private_segment_fixed_size", 0)) == 0, (n, k)
        if m.group(1) == "walk":
            assert int(k.get("group_segment_fixed_size", 0)) == 0, (n, k)
        seen[m.group(1)].add((m.group(2),) + tuple(int(g) for g in m.groups()[2:] if g is not None))
    types = ("float", "double")
    for stage in ("walk", "finish"):
        assert seen[stage] == {(t, d, c) for t in types for d in (2, 3) for c in (4, 8, 16)}, (stage, sorted(seen[stage]))
    for stage in ("bounds", "keys", "gather", "upper"):
        assert seen[stage] == {(t, d) for t in types for d in (2, 3)}, (stage, sorted(seen[stage]))
    sm = _load_tool("check_smem_pipeline")
    funcs = {n: c for n, c in sm.functions(sm.disassemble(nb.LIB_PATH)).items() if re.search(r"nntree_\w+_kernel", n) and c}
    assert len(funcs) == 12 + 12 + 4 * 4, sorted(funcs)
    for name, code in funcs.items():
        text = "\n".join(ins for _, ins, _ in code)
        assert "scratch_" not in text, name
        if "nntree_walk" not in name:
            continue
        assert "v_div_" not in text, name
        assert not re.findall(r"\bv_(rsq|rcp|sqrt)_", text), name
        assert "s_load_dword" in text, name  # boxes and records come through the scalar cache: wave-uniform addresses
