"""CPU: block time steps of the sixth-order Hermite integrator (nbody_hermite6_block_*) — the four entry points are declared, exported
and bound; their argument errors come in the documented order, the float refusal in its place before eps; the step criterion's
formulas recover the derivatives of a quintic; the NumPy model of the scheme (tests/hermite6_block_model.py) with max_level = 0 is the
fixed step; the launch shape of the active set's kernel with every body active is the fixed step's; the force + jerk + snap kernel of
the active set is in the built code object for double x 2D/3D and neither spills nor divides.
The CLI's refusal of --hermite-order 6 --hermite-eta stands as tests/test_hermite6.py pins it and is not repeated here."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import hermite6_block_model as M

BLOCK_SYMBOLS = ("nbody_hermite6_block_start", "nbody_hermite6_block_step", "nbody_hermite6_block_advance", "nbody_hermite6_block_read")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"

BAD_EPS = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]
BAD_ETA = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]


def test_block_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    L = nb.lib()
    for sym in BLOCK_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", text), f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
    assert L.nbody_abi_version() == 2004
    for name in ("block_start", "block_step", "block_advance", "block_read"):
        assert callable(getattr(nb.Hermite6, name))
    for name in ("hermite6_block_start", "hermite6_block_step", "hermite6_block_advance", "hermite6_block_levels", "hermite6_block_active"):
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
        "start": lambda h, s, eps, eta, lv=12: L.nbody_hermite6_block_start(h, s, eps, eta, lv, None),
        "step": lambda h, s, eps, eta, lv=12: L.nbody_hermite6_block_step(h, s, eps, eta, None, ctypes.byref(na), ctypes.byref(tau)),
        "advance": lambda h, s, eps, eta, lv=12: L.nbody_hermite6_block_advance(h, s, eps, eta, None, ctypes.byref(bs), ctypes.byref(bod)),
    }


@pytest.mark.parametrize("entry", ["start", "step", "advance"])
def test_block_argument_errors_in_the_documented_order(nb, entry):
    """The state, the whole system, the dtype, eps, eta, max_level, then the handle: every case is reached with h = NULL and a state
    that is never dereferenced."""
    L = nb.lib()
    f = _calls(L)[entry]
    err = lambda: L.nbody_last_error()
    ok = lambda dtype=1, **kw: ctypes.byref(_state(nb, dtype, **kw))
    assert f(None, None, 0.1, 0.3) == 1
    assert b"NULL" in err() and b"nbody_state" in err()
    assert f(None, ok(7), 0.1, 0.3) == 1
    assert b"dtype" in err() and b"fifth" not in err()
    assert f(None, ok(dim=4), 0.1, 0.3) == 1
    assert b"dim" in err()
    st = _state(nb)
    st.tuning = 0xdeadbeef
    assert f(None, ctypes.byref(st), 0.1, 0.3) == 1
    assert b"tuning" in err()
    for dtype in (0, 1):  # the whole system before the dtype
        assert f(None, ok(dtype, first=1), float("nan"), float("nan")) == 1
        assert b"whole system" in err()
    # float: refused after the whole-system rule and before eps, whatever else is wrong
    for dim in (2, 3):
        for eps in [0.1] + BAD_EPS:
            assert f(None, ok(0, dim=dim), eps, float("nan"), 99) == 1
            assert b"NBODY_F64" in err() and b"fifth difference" in err() and b"float" in err() and b"rounding" in err(), err()
            assert b"softening" not in err() and b"eta" not in err().replace(b"nbody_hermite", b"")
    # eps before eta: a bad eta does not hide a bad eps
    for eps in BAD_EPS + [1e-160]:
        assert f(None, ok(), eps, float("nan")) == 1, eps
        assert b"softening" in err(), (eps, err())
    # eta before max_level and the handle
    for eta in BAD_ETA:
        assert f(None, ok(), 0.1, eta, 99) == 1, eta
        assert b"eta" in err() and b"softening" not in err() and b"max_level" not in err(), (eta, err())
    assert (b"eta_start" in err()) == (entry == "start")
    if entry == "start":  # max_level before the handle
        for lv in (-1, -2, 21, 1 << 20):
            assert f(None, ok(), 0.1, 0.3, lv) == 1, lv
            assert b"max_level" in err() and b"NULL" not in err(), (lv, err())
        for lv in (0, 20):
            assert f(None, ok(), 0.1, 0.3, lv) == 1
            assert b"nbody_hermite6 is NULL" in err()
    assert f(None, ok(), 0.1, 0.3) == 1
    assert b"nbody_hermite6 is NULL" in err()
    assert f(None, ok(dim=2), 0.1, 0.0) == 1
    assert b"eta" in err()


def test_block_read_takes_null(nb):
    L = nb.lib()
    buf = (ctypes.c_int32 * 4)()
    assert L.nbody_hermite6_block_read(None, 0, buf, 16, None) == 1
    assert b"NULL" in L.nbody_last_error()


def test_derivs_recover_a_quintic():
    """a3, a4, a5 at h from (a, a', a'') at 0 and at h of random quintics with coefficients of size 1, against NumPy's own derivatives:
    within 1e-9 (of 1, or of the derivative where that is larger).  The formulas are differences: a5 comes out of terms of size
    720 / h^5, so in float64 its rounding is about 720 x 2^-53 / h^5 — 8e-11 at the smallest h here, 0.25."""
    rng = np.random.default_rng(1)
    for h in (0.25, 0.37, 1.0):
        for _ in range(20):
            p = np.polynomial.Polynomial(rng.normal(size=6))
            f = lambda k, t: p.deriv(k)(t) if k else p(t)
            got = M.derivs(f(0, 0.0), f(1, 0.0), f(2, 0.0), f(0, h), f(1, h), f(2, h), h)
            for k, g in zip((3, 4, 5), got):
                ref = f(k, h)
                assert abs(g - ref) <= 1e-9 * max(1.0, abs(ref)), (h, k, g, ref)


def _fixed_step(m, S, h, c, e2):
    """One nbody_hermite6_step of include/nbody_hip.h, written out on its own."""
    x, v, a0, j0, s0, k0 = S
    xp = x + h * v + h ** 2 / 2 * a0 + h ** 3 / 6 * j0 + h ** 4 / 24 * s0 + h ** 5 / 120 * k0
    vp = v + h * a0 + h ** 2 / 2 * j0 + h ** 3 / 6 * s0 + h ** 4 / 24 * k0
    ap = a0 + h * j0 + h ** 2 / 2 * s0 + h ** 3 / 6 * k0
    a1, j1, s1 = M.ref_force_jerk_snap(m, xp, vp, ap, c, e2, np.float64)
    v1 = v + h / 2 * (a0 + a1) + h ** 2 / 10 * (j0 - j1) + h ** 3 / 120 * (s0 + s1)
    x1 = x + h / 2 * (v + v1) + h ** 2 / 10 * (a0 - a1) + h ** 3 / 120 * (j0 + j1)
    k1 = (60 * (a1 - a0) - h * (24 * j0 + 36 * j1) + h ** 2 * (9 * s1 - 3 * s0)) / h ** 3
    return [x1, v1, a1, j1, s1, k1]


@pytest.mark.parametrize("dim,n", [(3, 200), (2, 65)])
def test_model_with_max_level_0_is_the_fixed_step(dim, n):
    """Three block steps of the model with max_level = 0: every body active at every step, tau_next = 1, the levels stay 0, and the
    state is that of three fixed steps (the same expressions: 1e-13 of the largest value of each array)."""
    T, dt, c, eps = np.float64, 0.01, 1.0, 0.05
    e2 = T(eps) * T(eps)
    m, x, v = M.random_arrays(dim, n, seed=n)
    S, lev = M.ref_start(m, x, v, c, e2, 0.3, dt, 0, T)
    assert not lev.any() and not S[5].any()
    F = [q.copy() for q in S]
    tau = np.zeros(n, np.int64)
    for _ in range(3):
        r = M.ref_block_step(T, m, S, lev, tau, dt, 0, c, e2, 0.4, ft=T)
        assert r["nxt"] == 1 and np.array_equal(r["act"], np.arange(n))
        M.apply_step(S, lev, tau, r, 0)
        assert not lev.any() and not tau.any()
        F = _fixed_step(m, F, T(dt), c, e2)
    for got, ref in zip(S, F):
        assert M.maxrel(got, ref) <= 1e-13


def test_launch_shape_with_every_body_active_is_the_fixed_steps(tmp_path):
    """tools/hermite_block_plan_check.cpp, compiled for the host alone: hermite_block_plan_for(sz, sz, 2) == hermite_plan_for(sz, 2) for
    sz in 1 .. 200 000, and the partial sums of any active set fit hermite_block_part_slots(sz, 2) (and the same for the fourth order,
    with 1 in place of 2)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    exe = tmp_path / "hermite_block_plan_check"
    subprocess.check_call([hipcc, "-std=c++17", "-O1", "--offload-host-only", "-I", os.path.join(ROOT, "stdpar-nbody_amd", "csrc"), "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "hermite_block_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), (r.stdout, r.stderr)


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + "_hermite6_block", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_active_set_kernels_neither_spill_nor_divide(nb):
    """hermite6_block_active_kernel<double, {2, 3}, {1, 2}> and no float one; private segment 0, no scratch_ instruction, no v_div_*,
    and every transcendental is a v_rsq (the checks tests/test_hermite6.py makes of the fixed step's pair kernels)."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    kr = _tool("kernel_resources")
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    seen = {}
    for k, n in zip(ks, names):
        m = re.search(r"nbody::hermite6_block_active_kernel<(float|double), (\d), (\d)>", n)
        if m:
            seen.setdefault((m.group(1), int(m.group(2))), []).append(int(m.group(3)))
            assert int(k.get("private_segment_fixed_size", 0)) == 0, (n, k)
    assert set(seen) == {("double", 2), ("double", 3)}, sorted(seen)
    assert all(sorted(r) == [1, 2] for r in seen.values()), seen
    sp = _tool("check_smem_pipeline")
    funcs = {n: c for n, c in sp.functions(sp.disassemble(nb.LIB_PATH)).items() if "hermite6_block_active_kernel" in n and c}
    assert len(funcs) >= 4, sorted(funcs)
    for name, code in funcs.items():
        text = "\n".join(ins for _, ins, _ in code)
        assert "scratch_" not in text, name
        assert "v_div_" not in text, name
        assert "v_rsq_f64" in text, name
        trans = re.findall(r"\bv_(rsq|rcp|sqrt|exp|log|sin|cos)(?:_[a-z]+)?_f(?:16|32|64)", text)
        assert trans and all(t == "rsq" for t in trans), (name, trans)
        assert "atomic" not in text, name
        assert "hermite6_pair_kernel" not in name  # the fixed step's test selects by that substring


def test_schedule_kernels_take_no_order_dependent_atomic(nb):
    """The only atomic of block_sched_* / hermite6_block_* / hermite_block_{init,reduce}_kernel is the unsigned minimum of tau_next
    (every code object's copy of the shared ones: tests/test_block_schedule.py)."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    sp = _tool("check_smem_pipeline")
    funcs = {n: c for n, c in sp.functions(sp.disassemble(nb.LIB_PATH)).items() if re.search(r"block_sched_|hermite6_block_|hermite_block_(init|reduce)_", n) and c}
    for kernel in ("block_sched_min_kernel", "block_sched_count_kernel", "block_sched_scan_kernel", "block_sched_compact_kernel",
                   "hermite_block_init_kernel", "hermite6_block_predict_kernel", "hermite_block_reduce_kernel",
                   "hermite6_block_correct_kernel"):
        assert any(kernel in n for n in funcs), (kernel, sorted(funcs))
    for name, code in funcs.items():
        atomics = [ins for _, ins, _ in code if "atomic" in ins]
        if "block_sched_min_kernel" in name:
            assert atomics and all("atomic_umin" in a for a in atomics), (name, atomics)
        else:
            assert not atomics, (name, atomics)
