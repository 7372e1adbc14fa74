"""CPU: friends-of-friends groups (nbody_fof_*, csrc/fof.inc) — the six entry points are declared, exported and bound and the ABI
version is unchanged; the argument errors of create, compute, read and summary come in the header's order without a GPU; the CLI
refuses the stated combinations of --save-groups / --groups-min before a device is opened and --help does not mention them; in the
built code object every fof_*_kernel is free of scratch and of floating-point atomics and the link kernel of divides, reciprocals and
roots; and the union-find the link kernel runs (csrc/fof_union.hpp) gives the sequential partition on 8 host threads under the
address, undefined-behaviour and thread sanitizers (tests/fof_union_main.cpp, a program of its own).
What the feature computes is held to brute force in tests/test_gpu_fof.py, and its rules in tests/test_fof_model.py."""
import ctypes
import importlib.util
import inspect
import os
import platform
import re
import shutil
import subprocess
import tempfile

import pytest

from conftest import ROOT

SYMBOLS = ("nbody_fof_create", "nbody_fof_create_on", "nbody_fof_destroy", "nbody_fof_compute", "nbody_fof_read", "nbody_fof_summary")
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
    for name in ("compute", "read", "summary", "catalogue"):
        assert callable(getattr(nb.Fof, name))
    assert inspect.signature(nb.Fof.__init__).parameters["min_members"].default == 1
    assert inspect.signature(nb.DeviceSystem.fof_handle).parameters["min_members"].default == 1
    assert inspect.signature(nb.DeviceSystem.fof).parameters["min_members"].default == 1
    assert inspect.signature(nb.DeviceSystem.fof_groups).parameters["min_members"].default == 20


def test_create_argument_errors_come_in_order_and_need_no_gpu(nb):
    L = nb.lib()
    err = lambda: L.nbody_last_error()
    h = ctypes.c_void_p()
    for f, tail in ((L.nbody_fof_create_on, (0,)), (L.nbody_fof_create, ())):
        # out NULL, dtype, dim, n, min_members — each earlier error wins over every later one
        assert f(None, 7, 4, 0, 0, *tail) == 1 and b"out is NULL" in err()
        assert f(ctypes.byref(h), 7, 4, 0, 0, *tail) == 1 and b"dtype" in err()
        assert f(ctypes.byref(h), 1, 4, 0, 0, *tail) == 1 and b"dim" in err()
        assert f(ctypes.byref(h), 1, 3, 0, 0, *tail) == 1 and b"2^28" in err()
        assert f(ctypes.byref(h), 0, 2, (1 << 28) + 1, 0, *tail) == 1 and b"2^28" in err()
        for n, mm in ((16, 0), (16, 17), (1, 2), (1 << 28, (1 << 28) + 1)):
            assert f(ctypes.byref(h), 1, 3, n, mm, *tail) == 1, (n, mm)
            assert b"min_members" in err() and b"2^28" not in err(), err()
        assert not h.value
    L.nbody_fof_destroy(None)  # a no-op


def test_compute_read_and_summary_argument_errors_need_no_gpu(nb):
    """Everything that is decided before the handle is looked at or a device is touched."""
    L = nb.lib()
    err = lambda: L.nbody_last_error()
    assert L.nbody_fof_compute(None, None, 0.1, None) == 1 and b"nbody_state is NULL" in err()
    m = (ctypes.c_double * 12)()
    st = nb.nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = 1, 3, 4, 0, 4
    st.m = st.x = ctypes.cast(m, ctypes.c_void_p).value  # never dereferenced: every call below is refused before the device
    assert L.nbody_fof_compute(None, ctypes.byref(st), float("nan"), None) == 1 and b"nbody_fof is NULL" in err()  # h before b
    st.count = 2
    assert L.nbody_fof_compute(None, ctypes.byref(st), 0.1, None) == 1 and b"whole system" in err()
    buf = (ctypes.c_uint32 * 4)()
    for what in (-1, 6, 100):
        assert L.nbody_fof_read(None, what, buf, 16, None) == 1 and b"what must be" in err()
    for what in range(6):
        assert L.nbody_fof_read(None, what, buf, 16, None) == 1 and b"nbody_fof is NULL" in err()
    assert L.nbody_fof_summary(None, buf, None) == 1 and b"nbody_fof is NULL" in err()


REFUSALS = [
    (["--groups-min", "5"], "--groups-min needs --save-groups B."),
    (["--algorithm", "octree", "--groups-min", "5", "--save", "pos"], "--groups-min needs --save-groups B."),
    (["--save-groups", "-0.5"], "--save-groups needs a linking length B, finite and >= 0."),
    (["--save-groups", "inf"], "--save-groups needs a linking length B, finite and >= 0."),
    (["--save-groups", "nan"], "--save-groups needs a linking length B, finite and >= 0."),
    (["--save-groups", "0.1x"], "--save-groups needs a linking length B, finite and >= 0."),
    (["--save-groups"], "--save-groups needs a linking length B, finite and >= 0."),
    (["--save-groups", "0.1", "--groups-min", "0"], "--groups-min needs a member count M >= 1."),
    (["--save-groups", "0.1", "--groups-min", "65"], "--groups-min M must not exceed the number of bodies (M = 65)."),
    (["--save-groups", "0.1", "--gpus", "1"], "--save-groups runs on one GPU: it cannot be combined with --gpus."),
    (["--gpus", "2", "--save-groups", "0.1", "--groups-min", "2", "--algorithm", "octree"],
     "--save-groups runs on one GPU: it cannot be combined with --gpus."),
]


@pytest.mark.parametrize("args,line", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_cli_refuses_before_opening_a_device(args, line, tmp_path):
    assert os.path.exists(CLI)
    r = subprocess.run([CLI, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60, cwd=tmp_path)
    assert r.returncode != 0, args
    assert line in r.stderr.splitlines(), (args, r.stderr)
    assert "HIP" not in r.stderr and "hip" not in r.stderr, r.stderr
    assert "Starting simulation" not in r.stdout
    assert not os.path.exists(tmp_path / "groups.bin")


def test_cli_help_does_not_mention_the_flags():
    got = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert got == open(os.path.join(ROOT, "tests", "golden", "help_d3.txt"), "rb").read()
    assert b"groups" not in got


def _load_tool(name):
    spec = importlib.util.spec_from_file_location(name + "_fof", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PER_TYPE_AND_DIM = ("link", "cat_sum")  # <T, D>
PER_TYPE = ("flatten", "labels")        # <T>: they read the sorted record, nothing of the dimension
PLAIN = ("init", "summary", "cat_count", "cat_scan", "cat_scatter")  # integers only


def test_fof_kernels_do_not_spill_have_no_float_atomics_and_the_link_has_no_divide_or_root(nb):
    """Every fof_*_kernel: private segment 0, no scratch_ instruction, no floating-point atomic; none has `nntree_` or `knn_` in its
    name (those kernels are counted by prefix).  The link kernel has no LDS either, no v_div_*, v_rcp, v_rsq or v_sqrt, reads boxes
    and records through scalar loads and exists for (float, double) x (2, 3), as the catalogue's sum does."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    kr = _load_tool("kernel_resources")
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    seen = {s: set() for s in PER_TYPE_AND_DIM + PER_TYPE + PLAIN}
    for k, n in zip(ks, names):
        if "fof_" not in n:
            continue
        assert "knn_" not in n and "nntree_" not in n, n  # the whole demangled signature: parameter types count too
        m = re.search(r"nbody::fof_(\w+)_kernel(?:<(float|double)(?:, (\d+))?>)?", n)
        assert m and m.group(1) in seen, f"a fof kernel with an unexpected name: {n}"
        assert int(k.get("private_segment_fixed_size", 0)) == 0, (n, k)
        if m.group(1) == "link":
            assert int(k.get("group_segment_fixed_size", 0)) == 0, (n, k)
        seen[m.group(1)].add(tuple(g if i == 0 else int(g) for i, g in enumerate(m.groups()[1:]) if g is not None))
    types = ("float", "double")
    for stage in PER_TYPE_AND_DIM:
        assert seen[stage] == {(t, d) for t in types for d in (2, 3)}, (stage, sorted(seen[stage]))
    for stage in PER_TYPE:
        assert seen[stage] == {(t,) for t in types}, (stage, sorted(seen[stage]))
    for stage in PLAIN:
        assert seen[stage] == {()}, (stage, sorted(seen[stage]))
    sm = _load_tool("check_smem_pipeline")
    funcs = {n: c for n, c in sm.functions(sm.disassemble(nb.LIB_PATH)).items() if re.search(r"fof_\w+_kernel", n) and c}
    assert len(funcs) == 4 * len(PER_TYPE_AND_DIM) + 2 * len(PER_TYPE) + len(PLAIN), sorted(funcs)
    for name, code in funcs.items():
        text = "\n".join(ins for _, ins, _ in code)
        assert "scratch_" not in text, name
        assert not re.findall(r"atomic_(?:pk_)?(?:add|min|max)_(?:f|bf)\d+", text), name  # integers only
        if "fof_link" not in name:
            continue
        assert "v_div_" not in text, name
        assert not re.findall(r"\bv_(rsq|rcp|sqrt)_", text), name
        assert "s_load_dword" in text, name  # boxes and records come through the scalar cache: wave-uniform addresses
        # ... all of them: the only vector loads wider than a dword are the lane's own position (at most two instructions)
        assert len(re.findall(r"\bglobal_load_dwordx[234]\b", text)) <= 2, name
        assert "global_atomic_cmpswap" in text, name  # the hook


def _build(src, exe, san, extra=()):
    return subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", f"-fsanitize={san}", *extra, src, "-o", exe],
                          capture_output=True, text=True)


def _thread_sanitizer_launcher():
    """Decided ONCE, when this file is collected, with a program that does nothing: how a -fsanitize=thread binary is started here.
    [] — directly; [setarch, machine, -R] — the runtime cannot lay out its shadow memory under this kernel's address-space
    randomisation ("unexpected memory mapping" before main), so every thread-sanitizer child gets randomisation switched off for
    itself, a personality flag of that one process; None — the toolchain has no usable runtime (no compiler, no libtsan, or it
    starts neither way): the thread case is then not part of this file, and TSAN_NOTE says so."""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "probe.cpp"), os.path.join(d, "probe")
        open(src, "w").write("int main() { return 0; }\n")
        try:
            if _build(src, exe, "thread").returncode != 0:
                return None
            if subprocess.run([exe], capture_output=True, timeout=60).returncode == 0:
                return []
            setarch = shutil.which("setarch")
            if setarch and subprocess.run([setarch, platform.machine(), "-R", exe], capture_output=True, timeout=60).returncode == 0:
                return [setarch, platform.machine(), "-R"]
        except (OSError, subprocess.TimeoutExpired):
            pass
    return None


TSAN_LAUNCHER = _thread_sanitizer_launcher()
TSAN_NOTE = ("the thread-sanitizer build runs" + (" directly" if TSAN_LAUNCHER == [] else " with address-space randomisation off for the child")
             if TSAN_LAUNCHER is not None else "this toolchain has no thread-sanitizer runtime that starts here: the thread build is not run")
SANITIZERS = [("address,undefined", ["-fno-sanitize-recover=all"], [])] + ([("thread", [], TSAN_LAUNCHER)] if TSAN_LAUNCHER is not None else [])


@pytest.mark.parametrize("san,extra,launcher", SANITIZERS, ids=[s for s, _, _ in SANITIZERS])
def test_union_find_on_host_threads_under_sanitizers(san, extra, launcher, tmp_path):
    """csrc/fof_union.hpp with std::atomic, 8 threads, random edge lists, chains and stars, against a sequential union-find: a
    stand-alone program built with the host compiler and the sanitizer, no GPU and nothing loaded into this process.  Whether and
    how the thread-sanitizer build can be started is settled at collection (TSAN_LAUNCHER); a run that fails here is a failure."""
    print(TSAN_NOTE)
    src = os.path.join(ROOT, "tests", "fof_union_main.cpp")
    exe = str(tmp_path / "fof_union_main")
    cc = _build(src, exe, san, extra)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run(launcher + [exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "fof_union ok" in run.stdout


def test_union_header_stands_alone():
    """What lets a host compiler build it: the standard library, nothing of the project's and nothing of HIP's."""
    text = open(os.path.join(ROOT, "stdpar-nbody_amd", "csrc", "fof_union.hpp")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<cstdint>"], includes
