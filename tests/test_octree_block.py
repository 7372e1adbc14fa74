"""CPU: block time steps of the octree leapfrog (nbody_octree_block_*) — the entry points are declared, exported and bound; their
argument errors come in the documented order with no device present; the CLI's --block-eta / --block-levels refusals need no GPU and
--help is unchanged; the level rule of the scheme, restated here in NumPy, on hand-worked cases; the new kernels are in the built
code object and neither the predictor nor the kick spills."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = ("nbody_octree_block_create", "nbody_octree_block_create_on", "nbody_octree_block_destroy", "nbody_octree_block_start",
           "nbody_octree_block_step", "nbody_octree_block_advance", "nbody_octree_block_read")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
CLI = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")

BAD_EPS = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]
BAD_ETA = [0.0, -1.0, float("nan"), float("inf"), -float("inf")]
ETA_UNDERFLOW = {0: [1e-60], 1: []}  # > 0 as a double but 0 as a float: eta must be > 0 as T too


def test_symbols_declared_exported_and_bound(nb):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nbody_hip.h")).read(), flags=re.S)
    L = nb.lib()
    for sym in SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", text), f"{sym} is not declared in nbody_hip.h"
        assert hasattr(L, sym), f"libnbody_hip.so does not export {sym}"
        assert sym in nb.ABI_SYMBOLS
    assert L.nbody_abi_version() == 2004
    for name in ("start", "step", "advance", "read"):
        assert callable(getattr(nb.OctreeBlock, name))
    for name in ("octree_block_start", "octree_block_step", "octree_block_advance", "octree_block_levels", "octree_block_active",
                 "octree_block_predicted"):
        assert callable(getattr(nb.DeviceSystem, name))


def _state(nb, dtype=1, dim=3, n=16, first=0, dt=0.0625):
    st = nb.nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = dtype, dim, n, first, n - first
    st.dt, st.c = dt, 1.0
    st.m = st.x = st.v = st.a = st.ao = 0x1000  # never dereferenced: every case below is refused before the device is touched
    return st


def _calls(L):
    """The three calls as f(h, tree, state, eps, eta, max_level): step and advance have no max_level."""
    na, tau = ctypes.c_uint32(), ctypes.c_uint32()
    bs, bod = ctypes.c_uint64(), ctypes.c_uint64()
    return {
        "start": lambda h, t, s, eps, eta, lv=12: L.nbody_octree_block_start(h, t, s, 0.5, eps, eta, lv, None),
        "step": lambda h, t, s, eps, eta, lv=12: L.nbody_octree_block_step(h, t, s, 0.5, eps, eta, None, ctypes.byref(na), ctypes.byref(tau)),
        "advance": lambda h, t, s, eps, eta, lv=12: L.nbody_octree_block_advance(h, t, s, 0.5, eps, eta, None, ctypes.byref(bs),
                                                                                ctypes.byref(bod)),
    }


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("entry", ["start", "step", "advance"])
def test_argument_errors_in_the_documented_order(nb, dtype, entry):
    """State, eps, eta, max_level, then the handles: every case is reached with h = NULL, tree = NULL and a state that is never
    dereferenced, so none of them needs a device."""
    L = nb.lib()
    f = _calls(L)[entry]
    err = lambda: L.nbody_last_error()
    ok = lambda **kw: ctypes.byref(_state(nb, dtype, **kw))
    assert f(None, None, None, 0.1, 0.02) == 1
    assert b"NULL" in err() and b"nbody_state" in err()
    assert f(None, None, ok(dim=4), 0.1, 0.02) == 1
    assert b"dim" in err()
    assert f(None, None, ok(first=1), 0.1, 0.02) == 1
    assert b"whole system" in err()
    # eps before eta: a bad eta does not hide a bad eps
    for eps in BAD_EPS:
        assert f(None, None, ok(), eps, float("nan")) == 1, eps
        assert b"softening" in err(), (eps, err())
    # eta before max_level and the handles
    for eta in BAD_ETA + ETA_UNDERFLOW[dtype]:
        assert f(None, None, ok(), 0.1, eta, 99) == 1, eta
        assert b"eta" in err() and b"softening" not in err() and b"max_level" not in err(), (eta, err())
    if entry == "start":  # max_level before the handles
        for lv in (-1, -2, 21, 1 << 20):
            assert f(None, None, ok(), 0.1, 0.02, lv) == 1, lv
            assert b"max_level" in err() and b"NULL" not in err(), (lv, err())
        for lv in (0, 20):
            assert f(None, None, ok(), 0.1, 0.02, lv) == 1
            assert b"nbody_octree_block is NULL" in err()
    # the handles before s->dt: a bad dt does not hide a NULL handle
    assert f(None, None, ok(dt=0.0), 0.1, 0.02) == 1
    assert b"nbody_octree_block is NULL" in err()
    assert f(None, None, ok(dim=2), 0.1, 0.0) == 1
    assert b"eta" in err()


def test_read_and_create_take_bad_arguments(nb):
    L = nb.lib()
    buf = (ctypes.c_int32 * 4)()
    assert L.nbody_octree_block_read(None, 0, buf, 16, None) == 1
    assert b"NULL" in L.nbody_last_error()
    h = ctypes.c_void_p()
    assert L.nbody_octree_block_create(ctypes.byref(h), 7, 3, ctypes.c_uint32(16)) == 1 and not h
    assert L.nbody_octree_block_create(ctypes.byref(h), 1, 4, ctypes.c_uint32(16)) == 1 and not h
    assert L.nbody_octree_block_create(ctypes.byref(h), 1, 3, ctypes.c_uint32(0)) == 1 and not h
    assert L.nbody_octree_block_create(None, 1, 3, ctypes.c_uint32(16)) == 1
    L.nbody_octree_block_destroy(None)


BLOCK = ["--softening", "0.05", "--block-eta", "0.02"]
REFUSALS = [
    (["--algorithm", "all-pairs"] + BLOCK, "--block-eta is supported by --algorithm octree only."),
    (["--algorithm", "bvh", "--block-eta", "0.02"], "--block-eta is supported by --algorithm octree only."),
    (["--block-eta", "0.02"], "--block-eta needs --softening EPS with EPS > 0."),
    (["--softening", "0", "--block-eta", "0.02"], "--block-eta needs --softening EPS with EPS > 0."),
    (BLOCK + ["--quadrupole"], "--block-eta takes the softened monopole walk: it cannot be combined with --quadrupole."),
    (BLOCK + ["--integrator", "hermite"], "--block-eta steps the octree leapfrog: it cannot be combined with --integrator hermite."),
    (BLOCK + ["--gpus", "1"], "--block-eta runs on one GPU: it cannot be combined with --gpus."),
    (["--softening", "0.05", "--block-levels", "8"], "--block-levels needs --block-eta ETA."),
    (["--softening", "0.05", "--block-eta", "0"], '--block-eta needs a finite accuracy parameter > 0, got "0".'),
    (["--softening", "0.05", "--block-eta", "-1"], '--block-eta needs a finite accuracy parameter > 0, got "-1".'),
    (["--softening", "0.05", "--block-eta", "nan"], '--block-eta needs a finite accuracy parameter > 0, got "nan".'),
    (["--softening", "0.05", "--block-eta", "inf"], '--block-eta needs a finite accuracy parameter > 0, got "inf".'),
    (["--softening", "0.05", "--block-eta", "0.02x"], '--block-eta needs a finite accuracy parameter > 0, got "0.02x".'),
    (BLOCK + ["--block-levels", "21"], '--block-levels needs a level count in 0 .. 20, got "21".'),
    (BLOCK + ["--block-levels", "-1"], '--block-levels needs a level count in 0 .. 20, got "-1".'),
]


@pytest.mark.parametrize("args,line", REFUSALS, ids=[" ".join(a) for a, _ in REFUSALS])
def test_cli_refuses_before_opening_a_device(args, line):
    assert os.path.exists(CLI)
    r = subprocess.run([CLI, "-n", "64", "-s", "1"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0, args
    assert line in r.stderr.splitlines(), (args, r.stderr)
    assert "HIP" not in r.stderr and "hip" not in r.stderr, r.stderr
    assert "Starting simulation" not in r.stdout


def test_cli_help_is_unchanged_and_hermite_stays_all_pairs_only():
    got = subprocess.run([CLI, "--help"], capture_output=True, timeout=60).stdout
    assert got == open(os.path.join(ROOT, "tests", "golden", "help_d3.txt"), "rb").read()
    assert b"block" not in got
    r = subprocess.run([CLI, "--algorithm", "octree", "--integrator", "hermite", "--softening", "0.05"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--integrator hermite is supported by --algorithm all-pairs only." in r.stderr.splitlines()


# ---- the level rule, restated -------------------------------------------------------------------------------------------------------
def want_of(a_norm, eta, eps):
    with np.errstate(divide="ignore"):
        return np.sqrt(2 * eta * eps / np.asarray(a_norm, np.float64))  # |a| = 0: inf, no limit


def start_level(want, dtmax, L):
    """The smallest level l with dtmax 2^-l <= want, clamped to [0, L]."""
    l = 0
    while l < L and dtmax * 2.0 ** -l > want:
        l += 1
    return l


def new_level(want, l, dtmax, L, tau_next):
    """The rule of a block step for a body of level l that is due at tau_next (in ticks of dtmax / 2^L)."""
    step = 1 << (L - l)
    h = dtmax * 2.0 ** -l
    if want < h:  # the smallest level deeper than l whose step is <= want, at most L
        nl = l + 1
        while nl < L and dtmax * 2.0 ** -nl > want:
            nl += 1
        return min(nl, L)
    if want >= 2 * h and l > 0 and tau_next % (2 * step) == 0:
        return l - 1
    return l


def test_level_rule_on_hand_worked_cases():
    # want = sqrt(2 eta eps / |a|): eta = 0.02, eps = 0.05 -> 2 eta eps = 0.002; |a| = 0.002 -> 1; 0.128 -> 0.125; 0 -> no limit
    assert want_of(0.002, 0.02, 0.05) == pytest.approx(1.0)
    assert want_of(0.128, 0.02, 0.05) == pytest.approx(0.125)
    assert np.isinf(want_of(0.0, 0.02, 0.05))
    # start, dtmax = 1, L = 4: steps 1, 1/2, 1/4, 1/8, 1/16
    assert [start_level(w, 1.0, 4) for w in (np.inf, 2.0, 1.0, 0.99, 0.5, 0.3, 0.25, 0.1, 0.0625, 0.01)] == [0, 0, 0, 1, 1, 2, 2, 4, 4, 4]
    assert start_level(0.001, 1.0, 0) == 0
    # a step, dtmax = 1, L = 4 (16 ticks).  A body of level 2 (h = 1/4, 4 ticks):
    assert new_level(0.3, 2, 1.0, 4, 4) == 2        # h <= want < 2 h: stays
    assert new_level(0.25, 2, 1.0, 4, 4) == 2       # want == h is not "< h"
    assert new_level(0.2, 2, 1.0, 4, 4) == 3        # 1/8 <= 0.2: one level deeper
    assert new_level(0.1, 2, 1.0, 4, 4) == 4        # 1/8 > 0.1, 1/16 <= 0.1: two levels deeper
    assert new_level(0.001, 2, 1.0, 4, 4) == 4      # at most L
    assert new_level(0.5, 2, 1.0, 4, 4) == 2        # want >= 2 h, but tick 4 is not on the grid of level 1 (8 ticks)
    assert new_level(0.5, 2, 1.0, 4, 8) == 1        # ... tick 8 is
    assert new_level(100.0, 2, 1.0, 4, 16) == 1     # one doubling at most, however large want is
    assert new_level(np.inf, 2, 1.0, 4, 16) == 1    # no limit: the same
    assert new_level(np.inf, 2, 1.0, 4, 12) == 2
    assert new_level(0.49, 2, 1.0, 4, 8) == 2       # want < 2 h
    # level 0 never goes coarser, level L never deeper
    assert new_level(100.0, 0, 1.0, 4, 16) == 0
    assert new_level(0.5, 0, 1.0, 4, 16) == 1
    assert new_level(0.01, 4, 1.0, 4, 3) == 4
    assert new_level(0.125, 4, 1.0, 4, 3) == 4      # 2 h, tick 3 is odd
    assert new_level(0.125, 4, 1.0, 4, 6) == 3
    assert new_level(0.5, 0, 1.0, 0, 1) == 0        # L = 0: one level


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name + "_octree_block", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_new_kernels_are_built_and_do_not_spill(nb):
    """The predictor, the kick and the start-level kernel for float/double x 2D/3D and the four schedule kernels are in the code object;
    none uses scratch; the only atomic is the integer minimum of tau_next (a minimum does not depend on the order it is taken in)."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    kr = _tool("kernel_resources")
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    seen = {}
    for k, n in zip(ks, names):
        m = re.search(r"nbody::((?:otb|block_sched)_\w+_kernel)(?:<(float|double), (\d)>)?", n)
        if m:
            seen.setdefault(m.group(1), set()).add((m.group(2), m.group(3)))
            assert int(k.get("private_segment_fixed_size", 0)) == 0, (n, k)
    td = {(t, d) for t in ("float", "double") for d in ("2", "3")}
    assert {k: v for k, v in seen.items() if k in ("otb_predict_kernel", "otb_kick_kernel", "otb_init_kernel")} == {
        "otb_predict_kernel": td, "otb_kick_kernel": td, "otb_init_kernel": td}, seen
    for name in ("block_sched_min_kernel", "block_sched_count_kernel", "block_sched_scan_kernel", "block_sched_compact_kernel"):
        assert name in seen, sorted(seen)
    sp = _tool("check_smem_pipeline")
    funcs = {n: c for n, c in sp.functions(sp.disassemble(nb.LIB_PATH)).items() if ("otb_" in n or "block_sched_" in n) and c}
    assert len(funcs) >= 16, sorted(funcs)
    for name, code in funcs.items():
        text = "\n".join(ins for _, ins, _ in code)
        assert "scratch_" not in text, name
        atomics = [ins for _, ins, _ in code if "atomic" in ins]
        if "block_sched_min_kernel" in name:
            assert atomics and all("atomic_umin" in a for a in atomics), (name, atomics)
        else:
            assert not atomics, (name, atomics)
