"""CPU: the sixth-order Hermite integrator (nbody_hermite6_*) — the six entry points are declared, exported and bound; their argument
errors and the CLI's --hermite-order refusals need no GPU; the force + jerk + snap kernels in the built code object neither spill nor
divide, and their only transcendental is the reciprocal square root."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HERMITE6_SYMBOLS = ("nbody_hermite6_create", "nbody_hermite6_create_on", "nbody_hermite6_destroy", "nbody_hermite6_start",
                    "nbody_hermite6_step", "nbody_hermite6_read")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CLI = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")

# the eps values tests/test_softening.py refuses (restated: that file is not a module of helpers)
BAD_EPS = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]
UNDERFLOW = {0: 1e-20, 1: 1e-160}


def test_hermite6_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    L = nb.lib()
    for sym in HERMITE6_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", text), f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
    assert L.nbody_abi_version() == 2004
    assert all(hasattr(nb.DeviceSystem, k) for k in ("hermite6_start", "hermite6_step", "hermite6_read")) and hasattr(nb, "Hermite6")


def _state(nb, dtype=1, dim=3, n=16, first=0):
    st = nb.nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = dtype, dim, n, first, n - first
    st.m = st.x = st.v = st.a = st.ao = 0x1000  # never dereferenced: every case below is refused before the device is touched
    return st


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("entry", ["nbody_hermite6_start", "nbody_hermite6_step"])
def test_hermite6_argument_errors_do_not_need_a_gpu(nb, dtype, entry):
    """The fourth-order entries' errors, in their order: the state, then eps, then the handle — every case is reached with h = NULL."""
    L = nb.lib()
    f = getattr(L, entry)
    err = lambda: L.nbody_last_error()
    assert f(None, None, 0.1, None) == 1
    assert b"NULL" in err()
    assert f(None, ctypes.byref(_state(nb, 7)), 0.1, None) == 1
    assert b"dtype" in err()
    assert f(None, ctypes.byref(_state(nb, dtype, dim=4)), 0.1, None) == 1
    assert b"dim" in err()
    assert f(None, ctypes.byref(_state(nb, dtype, first=1)), 0.1, None) == 1
    assert b"whole system" in err()
    st = _state(nb, dtype)
    st.tuning = 0xdeadbeef
    assert f(None, ctypes.byref(st), 0.1, None) == 1
    assert b"tuning" in err()
    for eps in BAD_EPS + [UNDERFLOW[dtype]]:
        assert f(None, ctypes.byref(_state(nb, dtype)), eps, None) == 1, eps
        assert b"softening" in err(), (eps, err())
    assert f(None, ctypes.byref(_state(nb, dtype)), 0.1, None) == 1
    assert b"nbody_hermite6 is NULL" in err() and b"softening" not in err()
    # 2D too
    assert f(None, ctypes.byref(_state(nb, dtype, dim=2)), 0.0, None) == 1
    assert b"softening" in err()


def test_hermite6_create_read_and_destroy_errors(nb):
    L = nb.lib()
    buf = (ctypes.c_double * 4)()
    for what in range(6):
        assert L.nbody_hermite6_read(None, what, buf, 32, None) == 1
        assert b"NULL" in L.nbody_last_error()
    L.nbody_hermite6_destroy(None)  # no-op
    h = ctypes.c_void_p()
    assert L.nbody_hermite6_create(None, 1, 3, 16) == 1 and b"NULL" in L.nbody_last_error()
    assert L.nbody_hermite6_create(ctypes.byref(h), 1, 4, 16) == 1 and b"dim" in L.nbody_last_error()
    assert L.nbody_hermite6_create(ctypes.byref(h), 7, 3, 16) == 1 and b"dtype" in L.nbody_last_error()
    assert L.nbody_hermite6_create(ctypes.byref(h), 1, 3, 0) == 1
    assert L.nbody_hermite6_create_on(ctypes.byref(h), 1, 4, 16, 0) == 1 and b"dim" in L.nbody_last_error()
    assert L.nbody_hermite6_create_on(ctypes.byref(h), 1, 3, 0, 0) == 1
    assert not h.value


SIXTH = ["--hermite-order", "6"]
REFUSALS = [
    # the flag's own
    (["--algorithm", "all-pairs", "--softening", "0.05"] + SIXTH, "--hermite-order needs --integrator hermite."),
    (["--algorithm", "all-pairs", "--softening", "0.05", "--hermite-order", "4"], "--hermite-order needs --integrator hermite."),
    (["--algorithm", "all-pairs", "--softening", "0.05", "--integrator", "leapfrog"] + SIXTH, "--hermite-order needs --integrator hermite."),
    (["--algorithm", "all-pairs", "--softening", "0.05", "--integrator", "hermite", "--hermite-order", "5"],
     '--hermite-order needs 4 or 6, got "5".'),
    (["--algorithm", "all-pairs", "--softening", "0.05", "--integrator", "hermite", "--hermite-order", "six"],
     '--hermite-order needs 4 or 6, got "six".'),
    (["--algorithm", "all-pairs", "--softening", "0.05", "--integrator", "hermite", "--hermite-eta", "0.02"] + SIXTH,
     "--hermite-order 6 takes a fixed step: it cannot be combined with --hermite-eta."),
    # what --integrator hermite refuses, unchanged with --hermite-order 6
    (["--algorithm", "all-pairs", "--integrator", "hermite"] + SIXTH, "--integrator hermite needs --softening EPS with EPS > 0."),
    (["--algorithm", "all-pairs", "--integrator", "hermite", "--softening", "0"] + SIXTH,
     "--integrator hermite needs --softening EPS with EPS > 0."),
    (["--algorithm", "octree", "--integrator", "hermite", "--softening", "0.05"] + SIXTH,
     "--integrator hermite is supported by --algorithm all-pairs only."),
    (["--algorithm", "bvh", "--integrator", "hermite", "--softening", "0.05"] + SIXTH,
     "--integrator hermite is supported by --algorithm all-pairs only."),
    (["--algorithm", "all-pairs-collapsed", "--integrator", "hermite", "--softening", "0.05"] + SIXTH,
     "--integrator hermite is supported by --algorithm all-pairs only."),
    (["--integrator", "hermite", "--softening", "0.05"] + SIXTH, "--integrator hermite is supported by --algorithm all-pairs only."),
    (["--algorithm", "all-pairs", "--integrator", "hermite", "--softening", "0.05", "--gpus", "1"] + SIXTH,
     "--integrator hermite runs on one GPU: it cannot be combined with --gpus."),
    (["--algorithm", "all-pairs", "--integrator", "hermite", "--softening", "0.05", "--hermite-levels", "4"] + SIXTH,
     "--hermite-levels needs --hermite-eta ETA."),
    (["--algorithm", "all-pairs", "--integrator", "rk4"] + SIXTH, 'Unknown integrator: "rk4".'),
]


@pytest.mark.parametrize("args,line", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_cli_refuses_before_opening_a_device(args, line):
    assert os.path.exists(CLI)
    r = subprocess.run([CLI, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0, args
    assert line in r.stderr.splitlines(), (args, r.stderr)
    assert "HIP" not in r.stderr and "hip" not in r.stderr, r.stderr
    assert "Starting simulation" not in r.stdout
    if "rk4" in args:
        assert "Options are: leapfrog (default), hermite." in r.stderr


def test_cli_help_is_still_the_reference_text():
    got = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert got == open(os.path.join(ROOT, "tests", "golden", "help_d3.txt"), "rb").read()
    assert b"hermite" not in got


def _disassembly(nb):
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_smem_pipeline_hermite6", os.path.join(ROOT, "tools", "check_smem_pipeline.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.functions(mod.disassemble(nb.LIB_PATH))


def test_pair_kernels_neither_spill_nor_divide(nb):
    """One force + jerk + snap kernel at least per (dtype, dim); private segment size 0, no scratch_ instruction, no v_div_*, and every
    transcendental is a v_rsq."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_resources_hermite6", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    seen = {}
    for k, n in zip(ks, names):
        m = re.search(r"nbody::hermite6_pair_kernel<(float|double), (\d), (\d)>", n)
        if m:
            seen.setdefault((m.group(1), int(m.group(2))), []).append(k)
            assert int(k.get("private_segment_fixed_size", 0)) == 0, (n, k)
    assert set(seen) == {(t, d) for t in ("float", "double") for d in (2, 3)}, sorted(seen)
    funcs = {n: c for n, c in _disassembly(nb).items() if "hermite6_pair_kernel" in n and c}
    assert len(funcs) >= 4, sorted(funcs)
    for name, code in funcs.items():
        text = "\n".join(ins for _, ins, _ in code)
        assert "scratch_" not in text, name
        assert "v_div_" not in text, name
        assert "v_rsq_f64" in text or "v_rsq_f32" in text, name
        trans = re.findall(r"\bv_(rsq|rcp|sqrt|exp|log|sin|cos)(?:_[a-z]+)?_f(?:16|32|64)", text)
        assert trans and all(t == "rsq" for t in trans), (name, trans)
    # the earlier selection by substring (tests/test_hermite.py) still sees the fourth-order kernels alone
    assert not any("hermite_force_jerk_kernel" in n for n in funcs)
