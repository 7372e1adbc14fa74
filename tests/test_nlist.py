"""CPU: exact fixed-radius neighbour lists (nbody_nlist_*, csrc/nlist.inc) — the seven entry points are declared, exported and bound
and the ABI version is unchanged; the argument errors of create, set_radii, compute, read and summary come in the header's order
without a GPU; the CLI refuses the stated combinations of --save-lists / --lists-capacity before a device is opened and --help does
not mention them; in the built code object every nlist_*_kernel is free of scratch and of atomics, the two walk kernels of divides,
reciprocals and roots and of LDS, and no signature contains `knn_`, `nntree_` or `fof_`; and the launch plan (csrc/nlist_plan.hpp)
holds its invariants in a program of its own under the address and undefined-behaviour sanitizers (tests/nlist_plan_main.cpp).
What the feature computes is held to brute force in tests/test_gpu_nlist.py, and its rules in tests/test_nlist_model.py."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("nbody_nlist_create", "nbody_nlist_create_on", "nbody_nlist_destroy", "nbody_nlist_set_radii", "nbody_nlist_compute",
           "nbody_nlist_read", "nbody_nlist_summary")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CLI = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")


def test_symbols_declared_exported_and_bound(nb):
    header = open(os.path.join(ROOT, "include", "nbody_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(nbody_[a-z_0-9]+)\s*\(", text))
    L = nb.lib()
    for sym in SYMBOLS:
        assert sym in declared, f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
        assert getattr(L, sym).argtypes is not None, f"{sym} has no argtypes"
    assert L.nbody_abi_version() == 2004  # additive: the version stays
    assert re.search(r"#define NBODY_NLIST_MAX_PER_BODY 4096\b", text) and nb.NeighbourLists.MAX_PER_BODY == 4096
    assert re.search(r"#define NBODY_NLIST_OVER_CAPACITY 1u", text) and re.search(r"#define NBODY_NLIST_OVER_PER_BODY 2u", text)
    assert (nb.NeighbourLists.OVER_CAPACITY, nb.NeighbourLists.OVER_PER_BODY) == (1, 2)
    for name in ("set_radii", "clear_radii", "compute", "summary", "read", "lists"):
        assert callable(getattr(nb.NeighbourLists, name))
    assert inspect.signature(nb.NeighbourLists.set_radii).parameters["squared"].default is False
    for name in ("nlist_handle", "nlist_compute", "radius_counts", "radius_neighbours"):
        assert callable(getattr(nb.DeviceSystem, name))
    for name in ("radius_counts", "radius_neighbours"):
        p = inspect.signature(getattr(nb.DeviceSystem, name)).parameters
        assert p["r"].default is None and p["radii"].default is None and p["squared"].default is False
    assert inspect.signature(nb.DeviceSystem.radius_neighbours).parameters["capacity"].default is None


def test_create_argument_errors_come_in_order_and_need_no_gpu(nb):
    L = nb.lib()
    err = lambda: L.nbody_last_error()
    h = ctypes.c_void_p()
    over = (1 << 32) + 1
    for f, tail in ((L.nbody_nlist_create_on, (0,)), (L.nbody_nlist_create, ())):
        # out NULL, dtype, dim, n, capacity — each earlier error wins over every later one
        assert f(None, 7, 4, 0, over, *tail) == 1 and b"out is NULL" in err()
        assert f(ctypes.byref(h), 7, 4, 0, over, *tail) == 1 and b"dtype" in err()
        assert f(ctypes.byref(h), 1, 4, 0, over, *tail) == 1 and b"dim" in err()
        assert f(ctypes.byref(h), 1, 3, 0, over, *tail) == 1 and b"2^28" in err()
        assert f(ctypes.byref(h), 0, 2, (1 << 28) + 1, over, *tail) == 1 and b"2^28" in err()
        for n in (1, 16, 1 << 28):
            assert f(ctypes.byref(h), 1, 3, n, over, *tail) == 1, n
            assert b"capacity" in err() and b"2^32" in err() and b"2^28" not in err(), err()
        assert not h.value
    L.nbody_nlist_destroy(None)  # a no-op


def test_set_radii_compute_read_and_summary_argument_errors_need_no_gpu(nb):
    """Everything that is decided before the handle is looked at or a device is touched."""
    L = nb.lib()
    err = lambda: L.nbody_last_error()
    assert L.nbody_nlist_compute(None, None, 0.1, None) == 1 and b"nbody_state is NULL" in err()
    m = (ctypes.c_double * 12)()
    st = nb.nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = 1, 3, 4, 0, 4
    st.m = st.x = ctypes.cast(m, ctypes.c_void_p).value  # never dereferenced: every call below is refused before the device
    assert L.nbody_nlist_compute(None, ctypes.byref(st), float("nan"), None) == 1 and b"nbody_nlist is NULL" in err()  # h before r
    st.count = 2
    assert L.nbody_nlist_compute(None, ctypes.byref(st), 0.1, None) == 1 and b"whole system" in err()
    st.count, st.dim = 4, 5
    assert L.nbody_nlist_compute(None, ctypes.byref(st), 0.1, None) == 1 and b"dim" in err()
    buf = (ctypes.c_uint64 * 4)()
    for what in (-1, 3, 100):
        assert L.nbody_nlist_read(None, what, buf, 16, None) == 1 and b"what must be" in err()
    for what in range(3):
        assert L.nbody_nlist_read(None, what, buf, 16, None) == 1 and b"nbody_nlist is NULL" in err()
    assert L.nbody_nlist_summary(None, buf, None) == 1 and b"nbody_nlist is NULL" in err()
    assert L.nbody_nlist_summary(None, None, None) == 1 and b"nbody_nlist is NULL" in err()
    for values, nbytes in ((buf, 32), (None, 0), (None, 8)):
        assert L.nbody_nlist_set_radii(None, values, nbytes, 0, None) == 1 and b"nbody_nlist is NULL" in err()


REFUSALS = [
    (["--lists-capacity", "5"], "--lists-capacity needs --save-lists R."),
    (["--algorithm", "octree", "--lists-capacity", "5", "--save", "pos"], "--lists-capacity needs --save-lists R."),
    (["--save-lists", "-0.5"], "--save-lists needs a radius R, finite and >= 0."),
    (["--save-lists", "inf"], "--save-lists needs a radius R, finite and >= 0."),
    (["--save-lists", "nan"], "--save-lists needs a radius R, finite and >= 0."),
    (["--save-lists", "0.1x"], "--save-lists needs a radius R, finite and >= 0."),
    (["--save-lists"], "--save-lists needs a radius R, finite and >= 0."),
    (["--save-lists", "0.1", "--lists-capacity", "-1"], "--lists-capacity needs an entry count C in 0 .. 2^32."),
    (["--save-lists", "0.1", "--lists-capacity", "4294967297"], "--lists-capacity needs an entry count C in 0 .. 2^32."),
    (["--save-lists", "0.1", "--lists-capacity", "12k"], "--lists-capacity needs an entry count C in 0 .. 2^32."),
    (["--save-lists", "0.1", "--lists-capacity"], "--lists-capacity needs an entry count C in 0 .. 2^32."),
    (["--save-lists", "0.1", "--gpus", "1"], "--save-lists runs on one GPU: it cannot be combined with --gpus."),
    (["--gpus", "2", "--save-lists", "0.1", "--lists-capacity", "64", "--algorithm", "octree"],
     "--save-lists runs on one GPU: it cannot be combined with --gpus."),
]


@pytest.mark.parametrize("args,line", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_cli_refuses_before_opening_a_device(args, line, tmp_path):
    assert os.path.exists(CLI)
    r = subprocess.run([CLI, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode != 0, args
    assert line in r.stderr.splitlines(), (args, r.stderr)
    assert "HIP" not in r.stderr and "hip" not in r.stderr, r.stderr
    assert "Starting simulation" not in r.stdout
    assert not os.path.exists(tmp_path / "lists.bin")


def test_cli_help_does_not_mention_the_flags():
    got = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert got == open(os.path.join(ROOT, "tests", "golden", "help_d3.txt"), "rb").read()
    assert b"lists" not in got


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name + "_nlist", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PER_TYPE_AND_DIM = ("count", "fill")                  # <T, D>: the two instantiations of the one walk
PLAIN = ("strip", "scan", "offsets", "order")         # integers only


def test_nlist_kernels_do_not_spill_have_no_atomics_and_the_walks_no_divide_or_root(nb):
    """Every nlist_*_kernel: private segment 0, no scratch_ instruction, no atomic of any kind (so no floating-point one); none has
    `nntree_`, `knn_` or `fof_` in its demangled signature (those kernels are counted by substring).  The two walk kernels have no LDS
    either, no v_div_*, v_rcp, v_rsq or v_sqrt, read boxes and records through scalar loads and exist for (float, double) x (2, 3)."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    kr = _load_tool("kernel_resources")
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    seen = {s: set() for s in PER_TYPE_AND_DIM + PLAIN}
    for k, n in zip(ks, names):
        if "nlist_" not in n:
            continue
        assert "knn_" not in n and "nntree_" not in n and "fof_" not in n, n  # the whole demangled signature: parameter types count too
        m = re.search(r"nbody::nlist_(\w+)_kernel(?:<(float|double), (\d+)>)?", n)
        assert m and m.group(1) in seen, f"an nlist kernel with an unexpected name: {n}"
        assert int(k.get("private_segment_fixed_size", 0)) == 0, (n, k)
        if m.group(1) in PER_TYPE_AND_DIM:
            assert int(k.get("group_segment_fixed_size", 0)) == 0, (n, k)
        if m.group(1) == "order":
            assert int(k.get("group_segment_fixed_size", 0)) == 4 * nb.NeighbourLists.MAX_PER_BODY, (n, k)  # the staged segment: 16 KB
        seen[m.group(1)].add(tuple(g if i == 0 else int(g) for i, g in enumerate(m.groups()[1:]) if g is not None))
    types = ("float", "double")
    for stage in PER_TYPE_AND_DIM:
        assert seen[stage] == {(t, d) for t in types for d in (2, 3)}, (stage, sorted(seen[stage]))
    for stage in PLAIN:
        assert seen[stage] == {()}, (stage, sorted(seen[stage]))
    sm = _load_tool("check_smem_pipeline")
    funcs = {n: c for n, c in sm.functions(sm.disassemble(nb.LIB_PATH)).items() if re.search(r"nlist_\w+_kernel", n) and c}
    assert len(funcs) == 4 * len(PER_TYPE_AND_DIM) + len(PLAIN), sorted(funcs)
    for name, code in funcs.items():
        text = "\n".join(ins for _, ins, _ in code)
        assert "scratch_" not in text, name
        assert "atomic" not in text, name  # none at all: nothing here needs one
        if "nlist_count" not in name and "nlist_fill" not in name:
            continue
        assert "v_div_" not in text, name
        assert not re.findall(r"\bv_(rsq|rcp|sqrt)_", text), name
        assert "ds_" not in text and "s_barrier" not in text, name  # every wave on its own
        assert "s_load_dword" in text, name  # boxes and records come through the scalar cache: wave-uniform addresses
        # ... all of them: the only vector loads of any width are the lane's own record (position, index: at most three
        # instructions), its radius and, in the fill, its two offsets
        assert len(re.findall(r"\bglobal_load_\w+", text)) <= (4 if "nlist_count" in name else 6), name


def test_plan_header_stands_alone():
    """What lets a host compiler build it: the standard library, nothing of the project's and nothing of HIP's."""
    text = open(os.path.join(ROOT, "stdpar-nbody_amd", "csrc", "nlist_plan.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstdint>"], includes


def test_plan_invariants_under_host_sanitizers(tmp_path):
    """tests/nlist_plan_main.cpp: n around every boundary and n = 2^28 — every body covered exactly once by the strips, the walks and
    the ordering, every strip by the scan, the strip sums and the total within 64 bits, nothing 32-bit overflows.  A stand-alone
    program built with the host compiler and the sanitizers; no GPU and nothing loaded into this process."""
    src = os.path.join(ROOT, "tests", "nlist_plan_main.cpp")
    exe = str(tmp_path / "nlist_plan_main")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-I", os.path.join(ROOT, "stdpar-nbody_amd", "csrc"), src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.rstrip().endswith("nlist_plan ok")
