"""CPU: all-pairs per-body potentials, nearest neighbours and the closest pair (nbody_neighbours_*) — the six entry points are declared,
exported and bound; their argument errors come in the header's order without a GPU; the CLI's --save-neighbours refusals come before a
device is opened and --help is still the reference's text; the new kernels in the built code object neither spill nor divide.
(A handle made for another dtype, dim or n needs a handle, which needs a device: tests/test_gpu_neighbours.py covers it.)"""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("nbody_neighbours_create", "nbody_neighbours_create_on", "nbody_neighbours_destroy", "nbody_neighbours_compute",
           "nbody_neighbours_read", "nbody_neighbours_closest_pair")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CLI = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")

# the eps values tests/test_softening.py refuses (restated: that file is not a module of helpers)
BAD_EPS = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]
UNDERFLOW = {0: 1e-20, 1: 1e-160}


def test_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(nbody_[a-z_0-9]+)\s*\(", text)))
    assert declared == sorted(nb.ABI_SYMBOLS)
    L = nb.lib()
    for sym in SYMBOLS:
        assert sym in declared, f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
    assert L.nbody_abi_version() == 2004  # additive: the version stays
    for name in ("Neighbours",):
        assert hasattr(nb, name)
    for name in ("neighbours", "closest_pair"):
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
    f = L.nbody_neighbours_compute
    err = lambda: L.nbody_last_error()
    # validation order: the state (dtype, dim, window, tuning), the whole-system rule, eps, then the handle — so every case here is
    # reached with h = NULL, and each earlier error wins over every later one
    assert f(None, None, 0.0, None) == 1
    assert b"nbody_state is NULL" in err()
    bad = _state(nb, dtype)
    bad.dtype = 7
    assert f(None, ctypes.byref(bad), 0.0, None) == 1 and b"dtype" in err()
    assert f(None, ctypes.byref(_state(nb, dtype, dim=4, first=1)), 0.0, None) == 1
    assert b"dim" in err()
    over = _state(nb, dtype)
    over.count = 17
    assert f(None, ctypes.byref(over), 0.0, None) == 1 and b"exceeds" in err()
    tun = _state(nb, dtype, first=1)
    tun.tuning = 0xdeadbeef
    assert f(None, ctypes.byref(tun), 0.0, None) == 1 and b"tuning" in err()
    assert f(None, ctypes.byref(_state(nb, dtype, first=1)), 0.0, None) == 1  # a shard window, with a bad eps behind it
    assert b"whole system" in err() and b"nbody_neighbours_compute" in err()
    for eps in BAD_EPS + [UNDERFLOW[dtype]]:
        assert f(None, ctypes.byref(_state(nb, dtype)), eps, None) == 1, eps
        assert b"softening" in err(), (eps, err())
    assert f(None, ctypes.byref(_state(nb, dtype)), 0.1, None) == 1
    assert b"nbody_neighbours is NULL" in err() and b"softening" not in err()
    # v, a and ao are not read: NULL there changes nothing (the handle is what is missing)
    assert f(None, ctypes.byref(_state(nb, dtype, arrays=False)), 0.1, None) == 1
    assert b"nbody_neighbours is NULL" in err()
    nom = _state(nb, dtype)
    nom.m = None
    assert f(None, ctypes.byref(nom), 0.1, None) == 1 and b"NULL array" in err()
    # 2D too
    assert f(None, ctypes.byref(_state(nb, dtype, dim=2)), 0.0, None) == 1
    assert b"softening" in err()


def test_read_closest_pair_create_and_destroy_argument_errors(nb):
    L = nb.lib()
    err = lambda: L.nbody_last_error()
    buf = (ctypes.c_double * 4)()
    for what in (-1, 3, 7):
        assert L.nbody_neighbours_read(None, what, buf, 32, None) == 1
        assert b"what" in err()
    assert L.nbody_neighbours_read(None, 0, buf, 0, None) == 1
    assert b"bytes" in err()
    assert L.nbody_neighbours_read(None, 1, buf, 32, None) == 1
    assert b"nbody_neighbours is NULL" in err()
    i, j = ctypes.c_uint32(5), ctypes.c_uint32(6)
    assert L.nbody_neighbours_closest_pair(None, ctypes.byref(i), ctypes.byref(j), buf, None) == 1
    assert b"nbody_neighbours is NULL" in err()
    assert (i.value, j.value) == (5, 6)
    L.nbody_neighbours_destroy(None)  # no-op
    h = ctypes.c_void_p()
    assert L.nbody_neighbours_create(None, 1, 3, 16) == 1 and b"NULL" in err()
    assert L.nbody_neighbours_create(ctypes.byref(h), 1, 4, 16) == 1 and b"dim" in err()
    assert L.nbody_neighbours_create(ctypes.byref(h), 7, 3, 16) == 1 and b"dtype" in err()
    assert L.nbody_neighbours_create(ctypes.byref(h), 1, 3, 0) == 1
    assert L.nbody_neighbours_create_on(ctypes.byref(h), 1, 3, (1 << 28) + 1, 0) == 1
    assert not h.value


REFUSALS = [
    (["--algorithm", "all-pairs", "--save-neighbours"], "--save-neighbours needs --softening EPS with EPS > 0."),
    (["--algorithm", "all-pairs", "--save-neighbours", "--softening", "0"], "--save-neighbours needs --softening EPS with EPS > 0."),
    (["--save-neighbours"], "--save-neighbours needs --softening EPS with EPS > 0."),  # default: octree
    (["--algorithm", "bvh", "--save-neighbours"], "--save-neighbours needs --softening EPS with EPS > 0."),
    (["--algorithm", "all-pairs", "--save-neighbours", "--softening", "0.05", "--gpus", "1"],
     "--save-neighbours runs on one GPU: it cannot be combined with --gpus."),
    (["--algorithm", "all-pairs", "--save-neighbours", "--softening", "0.05", "--gpus", "2", "--save", "pos"],
     "--save-neighbours runs on one GPU: it cannot be combined with --gpus."),
]


@pytest.mark.parametrize("args,line", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_cli_refuses_before_opening_a_device(args, line, tmp_path):
    assert os.path.exists(CLI)
    r = subprocess.run([CLI, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode != 0, args
    assert line in r.stderr.splitlines(), (args, r.stderr)
    assert "HIP" not in r.stderr and "hip" not in r.stderr, r.stderr
    assert "Starting simulation" not in r.stdout
    assert not os.path.exists(tmp_path / "neighbours.bin")


def test_cli_help_is_still_the_reference_text():
    got = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert got == open(os.path.join(ROOT, "tests", "golden", "help_d3.txt"), "rb").read()
    assert b"neighbours" not in got


def _disassembly(nb):
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_smem_pipeline_neighbours", os.path.join(ROOT, "tools", "check_smem_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.functions(mod.disassemble(nb.LIB_PATH))


def test_neighbours_kernels_neither_spill_nor_divide(nb):
    """Every kernel of a compute (the pack kernel is csrc/pair_sweep.hpp's, shared with kNN): private segment 0, no scratch_
    instruction, no v_div_*; the sweep exists per (dtype, dim, targets per lane) and its only transcendental is the reciprocal square
    root (no v_rcp, no v_sqrt); the other kernels have none."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources_neighbours", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    sweeps, others = set(), set()
    for k, n in zip(ks, names):
        m = re.search(r"nbody::(?:pair|neighbours)_(pack|sweep|finish|closest)_kernel<(float|double)(?:, (\d))?(?:, (\d))?>", n)
        if not m:
            continue
        assert int(k.get("private_segment_fixed_size", 0)) == 0, (n, k)
        if m.group(1) == "sweep":
            sweeps.add((m.group(2), int(m.group(3)), int(m.group(4))))
        else:
            others.add((m.group(1), m.group(2)))
    assert sweeps == {(t, d, r) for t in ("float", "double") for d in (2, 3) for r in (1, 2)}, sorted(sweeps)
    assert others == {(k, t) for k in ("pack", "finish", "closest") for t in ("float", "double")}, sorted(others)
    funcs = {n: c for n, c in _disassembly(nb).items() if re.search(r"(pair|neighbours)_(pack|sweep|finish|closest)_kernel", n) and c}
    assert len(funcs) == 8 + 4 + 2 + 2, sorted(funcs)
    for name, code in funcs.items():
        text = "\n".join(ins for _, ins, _ in code)
        assert "scratch_" not in text, name
        assert "v_div_" not in text, name
        trans = re.findall(r"\bv_(rsq|rcp|sqrt)_f(32|64)", text)
        if "sweep" in name:
            assert "v_rsq_f64" in text or "v_rsq_f32" in text, name
            assert all(t == "rsq" for t, _ in trans), name
        else:
            assert not trans, name
