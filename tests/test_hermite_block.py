"""CPU: block time steps of the Hermite integrator (nbody_hermite_block_*) — the four entry points are declared, exported and bound;
their argument errors come in the documented order and the CLI's --hermite-eta / --hermite-levels refusals need no GPU; the force +
jerk kernel of the active set is in the built code object for float/double x 2D/3D and neither spills nor divides."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

BLOCK_SYMBOLS = ("nbody_hermite_block_start", "nbody_hermite_block_step", "nbody_hermite_block_advance", "nbody_hermite_block_read")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CLI = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")

BAD_EPS = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]
BAD_ETA = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]
ETA_UNDERFLOW = {0: [1e-60], 1: []}  # > 0 as a double but 0 as a float: eta must be > 0 as T too


def test_block_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    L = nb.lib()
    for sym in BLOCK_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", text), f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
    assert L.nbody_abi_version() == 2004
    for name in ("block_start", "block_step", "block_advance", "block_read"):
        assert callable(getattr(nb.Hermite, name))
    for name in ("hermite_block_start", "hermite_block_step", "hermite_block_advance", "hermite_block_levels"):
        assert callable(getattr(nb.DeviceSystem, name))


def _state(nb, dtype=1, dim=3, n=16, first=0, dt=0.0625):
    st = nb.nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = dtype, dim, n, first, n - first
    st.dt, st.c = dt, 1.0
    st.m = st.x = st.v = st.a = st.ao = 0x1000  # never dereferenced: every case below is refused before the device is touched
    return st


def _calls(L):
    """The three calls as f(h, state, eps, eta, max_level): step and advance have no max_level."""
    na, tau = ctypes.c_uint32(), ctypes.c_uint32()
    bs, bod = ctypes.c_uint64(), ctypes.c_uint64()
    return {
        "start": lambda h, s, eps, eta, lv=12: L.nbody_hermite_block_start(h, s, eps, eta, lv, None),
        "step": lambda h, s, eps, eta, lv=12: L.nbody_hermite_block_step(h, s, eps, eta, None, ctypes.byref(na), ctypes.byref(tau)),
        "advance": lambda h, s, eps, eta, lv=12: L.nbody_hermite_block_advance(h, s, eps, eta, None, ctypes.byref(bs), ctypes.byref(bod)),
    }


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("entry", ["start", "step", "advance"])
def test_block_argument_errors_in_the_documented_order(nb, dtype, entry):
    """State, eps, eta, max_level, then the handle: every case is reached with h = NULL and a state that is never dereferenced."""
    L = nb.lib()
    f = _calls(L)[entry]
    err = lambda: L.nbody_last_error()
    ok = lambda **kw: ctypes.byref(_state(nb, dtype, **kw))
    assert f(None, None, 0.1, 0.02) == 1
    assert b"NULL" in err() and b"nbody_state" in err()
    assert f(None, ok(dim=4), 0.1, 0.02) == 1
    assert b"dim" in err()
    assert f(None, ok(first=1), 0.1, 0.02) == 1
    assert b"whole system" in err()
    # eps before eta: a bad eta does not hide a bad eps
    for eps in BAD_EPS:
        assert f(None, ok(), eps, float("nan")) == 1, eps
        assert b"softening" in err(), (eps, err())
    # eta before max_level and the handle
    for eta in BAD_ETA + ETA_UNDERFLOW[dtype]:
        assert f(None, ok(), 0.1, eta, 99) == 1, eta
        assert b"eta" in err() and b"softening" not in err() and b"max_level" not in err(), (eta, err())
    assert (b"eta_start" in err()) == (entry == "start")
    if entry == "start":  # max_level before the handle
        for lv in (-1, -2, 21, 1 << 20):
            assert f(None, ok(), 0.1, 0.02, lv) == 1, lv
            assert b"max_level" in err() and b"NULL" not in err(), (lv, err())
        for lv in (0, 20):
            assert f(None, ok(), 0.1, 0.02, lv) == 1
            assert b"nbody_hermite is NULL" in err()
    assert f(None, ok(), 0.1, 0.02) == 1
    assert b"nbody_hermite is NULL" in err()
    assert f(None, ok(dim=2), 0.1, 0.0) == 1
    assert b"eta" in err()


def test_block_read_takes_null(nb):
    L = nb.lib()
    buf = (ctypes.c_int32 * 4)()
    assert L.nbody_hermite_block_read(None, 0, buf, 16, None) == 1
    assert b"NULL" in L.nbody_last_error()


HERMITE = ["--algorithm", "all-pairs", "--integrator", "hermite", "--softening", "0.002"]
REFUSALS = [
    (["--algorithm", "all-pairs", "--softening", "0.002", "--hermite-eta", "0.02"], "--hermite-eta needs --integrator hermite."),
    (["--algorithm", "all-pairs", "--integrator", "leapfrog", "--softening", "0.002", "--hermite-eta", "0.02"],
     "--hermite-eta needs --integrator hermite."),
    (HERMITE + ["--hermite-eta", "0"], '--hermite-eta needs a finite accuracy parameter > 0, got "0".'),
    (HERMITE + ["--hermite-eta", "-1"], '--hermite-eta needs a finite accuracy parameter > 0, got "-1".'),
    (HERMITE + ["--hermite-eta", "nan"], '--hermite-eta needs a finite accuracy parameter > 0, got "nan".'),
    (HERMITE + ["--hermite-eta", "inf"], '--hermite-eta needs a finite accuracy parameter > 0, got "inf".'),
    (HERMITE + ["--hermite-eta", "0.02x"], '--hermite-eta needs a finite accuracy parameter > 0, got "0.02x".'),
    (HERMITE + ["--hermite-eta", "0.02", "--hermite-levels", "21"], '--hermite-levels needs a level count in 0 .. 20, got "21".'),
    (HERMITE + ["--hermite-eta", "0.02", "--hermite-levels", "-1"], '--hermite-levels needs a level count in 0 .. 20, got "-1".'),
    (HERMITE + ["--hermite-levels", "8"], "--hermite-levels needs --hermite-eta ETA."),
    (["--algorithm", "octree", "--integrator", "hermite", "--softening", "0.002", "--hermite-eta", "0.02"],
     "--integrator hermite is supported by --algorithm all-pairs only."),
    (HERMITE + ["--hermite-eta", "0.02", "--gpus", "1"], "--integrator hermite runs on one GPU: it cannot be combined with --gpus."),
]


@pytest.mark.parametrize("args,line", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_cli_refuses_before_opening_a_device(args, line):
    assert os.path.exists(CLI)
    r = subprocess.run([CLI, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0, args
    assert line in r.stderr.splitlines(), (args, r.stderr)
    assert "HIP" not in r.stderr and "hip" not in r.stderr, r.stderr
    assert "Starting simulation" not in r.stdout


def test_cli_help_and_integrator_choices_are_unchanged():
    got = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert got == open(os.path.join(ROOT, "tests", "golden", "help_d3.txt"), "rb").read()
    assert b"hermite" not in got
    r = subprocess.run([CLI, "--integrator", "block"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Options are: leapfrog (default), hermite." in r.stderr


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + "_hermite_block", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_active_set_kernels_neither_spill_nor_divide(nb):
    """hermite_block_active_kernel for float/double x 2D/3D, one and two targets per lane; private segment 0, no scratch_ instruction, no
    v_div_*, one reciprocal square root per pair and no other transcendental; its name must not select it into the fixed-step test."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    kr = _tool("kernel_resources")
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    seen = {}
    for k, n in zip(ks, names):
        m = re.search(r"nbody::hermite_block_active_kernel<(float|double), (\d), (\d)>", n)
        if m:
            seen.setdefault((m.group(1), int(m.group(2))), []).append(int(m.group(3)))
            assert int(k.get("private_segment_fixed_size", 0)) == 0, (n, k)
            assert "hermite_force_jerk_kernel" not in n
    assert set(seen) == {(t, d) for t in ("float", "double") for d in (2, 3)}, sorted(seen)
    assert all(sorted(r) == [1, 2] for r in seen.values()), seen
    sp = _tool("check_smem_pipeline")
    funcs = {n: c for n, c in sp.functions(sp.disassemble(nb.LIB_PATH)).items() if "hermite_block_active_kernel" in n and c}
    assert len(funcs) >= 8, sorted(funcs)
    for name, code in funcs.items():
        text = "\n".join(ins for _, ins, _ in code)
        assert "scratch_" not in text, name
        assert "v_div_" not in text, name
        assert "v_rsq_f64" in text or "v_rsq_f32" in text, name
        assert len(re.findall(r"\bv_(rsq|rcp|sqrt)_f(32|64)", text)) == len(re.findall(r"\bv_rsq_f(32|64)", text)), name
        assert "atomic" not in text, name


def test_schedule_kernels_take_no_order_dependent_atomic(nb):
    """The only atomic of the schedule is the integer minimum of tau_next (a minimum does not depend on the order it is taken in); the
    compaction, the scan and the corrector have none."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    sp = _tool("check_smem_pipeline")
    funcs = {n: c for n, c in sp.functions(sp.disassemble(nb.LIB_PATH)).items() if re.search(r"block_sched_|hermite_block_", n) and c}
    assert any("block_sched_compact_kernel" in n for n in funcs) and any("hermite_block_correct_kernel" in n for n in funcs), sorted(funcs)
    for name, code in funcs.items():
        atomics = [ins for _, ins, _ in code if "atomic" in ins]
        if "block_sched_min_kernel" in name:
            assert atomics and all("atomic_umin" in a for a in atomics), (name, atomics)
        else:
            assert not atomics, (name, atomics)
