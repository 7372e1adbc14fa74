"""CPU: all-pairs k nearest neighbours, local densities and the density centre (nbody_knn_*) — the six entry points are declared,
exported and bound; their argument errors come in the header's order without a GPU; the CLI's --save-density refusals come before a
device is opened and --help is still the reference's text; the new kernels in the built code object do not spill, and only the finish
and summary kernels divide or take a root.
(A handle made for another dtype, dim or n needs a handle, which needs a device: tests/test_gpu_knn.py covers it.)"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("nbody_knn_create", "nbody_knn_create_on", "nbody_knn_destroy", "nbody_knn_compute", "nbody_knn_read",
           "nbody_knn_density_centre")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CLI = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")


def test_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nbody_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(nb.ABI_SYMBOLS)
    L = nb.lib()
    for sym in SYMBOLS:
        assert sym in declared, f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
        assert getattr(L, sym).argtypes is not None, f"{sym} has no argtypes"
    assert L.nbody_abi_version() == 2004  # additive: the version stays
    assert re.search(r"#define\s+NBODY_KNN_MAX\s+16\b", text)
    assert hasattr(nb, "Knn")
    for name in ("compute", "read", "density_centre", "close"):
        assert callable(getattr(nb.Knn, name))
    for name in ("knn", "knn_compute", "local_density", "density_centre"):
        assert callable(getattr(nb.DeviceSystem, name))


def _state(nb, dtype=1, dim=3, n=16, first=0, arrays=True):
    st = nb.nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = dtype, dim, n, first, n - first
    st.m = st.x = 0x1000  # never dereferenced: every case below is refused before the device is touched
    if arrays:
        st.v = st.a = st.ao = 0x1000
    return st


@pytest.mark.parametrize("dtype", [0, 1])
def test_compute_argument_errors_come_in_order_and_need_no_gpu(nb, dtype):
    L = nb.lib()
    f = L.nbody_knn_compute
    err = lambda: L.nbody_last_error()
    # validation order: the state (dtype, dim, window, tuning), the whole-system rule, then the handle — so every case here is reached
    # with h = NULL, and each earlier error wins over every later one
    assert f(None, None, None) == 1
    assert b"nbody_state is NULL" in err()
    bad = _state(nb, dtype)
    bad.dtype = 7
    assert f(None, ctypes.byref(bad), None) == 1 and b"dtype" in err()
    assert f(None, ctypes.byref(_state(nb, dtype, dim=4, first=1)), None) == 1
    assert b"dim" in err()
    over = _state(nb, dtype)
    over.count = 17
    assert f(None, ctypes.byref(over), None) == 1 and b"exceeds" in err()
    tun = _state(nb, dtype, first=1)
    tun.tuning = 0xdeadbeef
    assert f(None, ctypes.byref(tun), None) == 1 and b"tuning" in err()
    assert f(None, ctypes.byref(_state(nb, dtype, first=1)), None) == 1  # a shard window
    assert b"whole system" in err() and b"nbody_knn_compute" in err()
    assert f(None, ctypes.byref(_state(nb, dtype)), None) == 1
    assert b"nbody_knn is NULL" in err()
    # v, a and ao are not read: NULL there changes nothing (the handle is what is missing)
    assert f(None, ctypes.byref(_state(nb, dtype, arrays=False)), None) == 1
    assert b"nbody_knn is NULL" in err()
    nom = _state(nb, dtype)
    nom.m = None
    assert f(None, ctypes.byref(nom), None) == 1 and b"NULL array" in err()
    # 2D too
    assert f(None, ctypes.byref(_state(nb, dtype, dim=2)), None) == 1
    assert b"nbody_knn is NULL" in err()


def test_read_density_centre_create_and_destroy_argument_errors(nb):
    L = nb.lib()
    err = lambda: L.nbody_last_error()
    buf = (ctypes.c_double * 4)()
    for what in (-1, 3, 7):
        assert L.nbody_knn_read(None, what, buf, 32, None) == 1
        assert b"what" in err()
    assert L.nbody_knn_read(None, 0, buf, 0, None) == 1
    assert b"bytes" in err()
    assert L.nbody_knn_read(None, 1, buf, 32, None) == 1
    assert b"nbody_knn is NULL" in err()
    buf[0] = 5.0
    assert L.nbody_knn_density_centre(None, buf, buf, buf, None) == 1
    assert b"nbody_knn is NULL" in err()
    assert buf[0] == 5.0
    L.nbody_knn_destroy(None)  # no-op
    # create: out NULL, dtype, dim, n, k — each earlier error wins over every later one
    h = ctypes.c_void_p()
    assert L.nbody_knn_create(None, 7, 4, 0, 0) == 1 and b"out is NULL" in err()
    assert L.nbody_knn_create(ctypes.byref(h), 7, 4, 0, 0) == 1 and b"dtype" in err()
    assert L.nbody_knn_create(ctypes.byref(h), 1, 4, 0, 0) == 1 and b"dim" in err()
    assert L.nbody_knn_create(ctypes.byref(h), 1, 3, 0, 0) == 1 and b"2^28" in err()
    assert L.nbody_knn_create_on(ctypes.byref(h), 1, 3, (1 << 28) + 1, 0, 0) == 1 and b"2^28" in err()
    for k in (0, -1, 17, 1 << 20):
        assert L.nbody_knn_create(ctypes.byref(h), 1, 3, 16, k) == 1, k
        assert b"1 <= k <= 16" in err(), err()
        assert L.nbody_knn_create_on(ctypes.byref(h), 0, 2, 16, k, 0) == 1, k
        assert b"1 <= k <= 16" in err(), err()
    assert not h.value


REFUSALS = [
    (["--algorithm", "all-pairs", "--save-density"], "--save-density needs a neighbour count K in 2 .. 16."),
    (["--save-density", "six"], "--save-density needs a neighbour count K in 2 .. 16."),
    (["--save-density", "6.5"], "--save-density needs a neighbour count K in 2 .. 16."),
    (["--save-density", "--save", "pos"], "--save-density needs a neighbour count K in 2 .. 16."),
    (["--save-density", "1"], "--save-density needs a neighbour count K in 2 .. 16."),
    (["--save-density", "17", "--algorithm", "bvh"], "--save-density needs a neighbour count K in 2 .. 16."),
    (["--save-density", "-6"], "--save-density needs a neighbour count K in 2 .. 16."),
    (["--algorithm", "all-pairs", "--save-density", "6", "--gpus", "1"],
     "--save-density runs on one GPU: it cannot be combined with --gpus."),
    (["--save-density", "16", "--gpus", "2", "--save", "pos"], "--save-density runs on one GPU: it cannot be combined with --gpus."),
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


def test_cli_help_is_still_the_reference_text():
    got = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert got == open(os.path.join(ROOT, "tests", "golden", "help_d3.txt"), "rb").read()
    assert b"density" not in got


def _load_tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + "_knn", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_knn_kernels_do_not_spill_and_the_sweep_has_no_transcendental(nb):
    """Every knn_*_kernel and the pack kernel (csrc/pair_sweep.hpp's, shared with neighbours): private segment 0 and no scratch_
    instruction; the sweep exists per (dtype, dim, list capacity) and has no v_rsq, v_rcp, v_sqrt or v_div_*: only finish and summary
    may divide or take a root (pack has none either)."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    kr = _load_tool("kernel_resources")
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    seen = {"pack": set(), "sweep": set(), "finish": set(), "summary": set()}
    for k, n in zip(ks, names):
        assert not re.search(r"neighbours_\w*knn|knn_\w*neighbours", n)
        m = re.search(r"nbody::(?:knn|pair)_(\w+)_kernel<(float|double)(?:, (\d+))?(?:, (\d+))?>", n)
        if not m:
            assert "knn_" not in n, f"a knn kernel with an unexpected name: {n}"
            continue
        assert m.group(1) in seen, n
        assert int(k.get("private_segment_fixed_size", 0)) == 0, (n, k)
        seen[m.group(1)].add((m.group(2),) + tuple(int(g) for g in m.groups()[2:] if g is not None))
    types = ("float", "double")
    assert seen["sweep"] == {(t, d, c) for t in types for d in (2, 3) for c in (4, 8, 16)}, sorted(seen["sweep"])
    assert seen["finish"] == {(t, d, c) for t in types for d in (2, 3) for c in (4, 8, 16)}, sorted(seen["finish"])
    assert seen["pack"] == {(t, d) for t in types for d in (2, 3)}, sorted(seen["pack"])
    assert seen["summary"] == {(t, d) for t in types for d in (2, 3)}, sorted(seen["summary"])
    sm = _load_tool("check_smem_pipeline")
    funcs = {n: c for n, c in sm.functions(sm.disassemble(nb.LIB_PATH)).items() if re.search(r"(knn_\w+|pair_pack)_kernel", n) and c}
    assert len(funcs) == 12 + 12 + 4 + 4, sorted(funcs)
    for name, code in funcs.items():
        text = "\n".join(ins for _, ins, _ in code)
        assert "scratch_" not in text, name
        if "finish" in name or "summary" in name:
            continue
        assert "v_div_" not in text, name
        assert not re.findall(r"\bv_(rsq|rcp|sqrt)_", text), name
