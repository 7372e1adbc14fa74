"""GPU: block (individual) time steps of the sixth-order Hermite integrator (nbody_hermite6_block_*, double only) against the NumPy
restatement of the scheme in tests/hermite6_block_model.py: np.longdouble for single block steps and single evaluations, float64 for
runs.  The shapes are those of tests/test_gpu_hermite_block.py.

Launch-shape boundaries of hermite_block_plan_for(sz, n_act, 2) (csrc/hermite_block_plan.hpp) crossed below.  Over n_act: the block of 64
targets (63 / 64 / 65), two targets per lane from 65536 active bodies on (max_level = 0 at 65 537 bodies), and the cut of the source
tiles over grid.y: ceil(2048 / blocks) chunks, at least two, at most one per tile of 256 sources — at N = 20 000 (79 tiles) 1 .. 365
active bodies take 79 chunks of one tile (more than 64: the reduce kernel), all 20 000 take 7 chunks of 12 tiles, the fixed step's
plan.  Over N with every body active (max_level = 0): one tile (200), one tile per chunk (300, 1000), several tiles per chunk
(40 000), two targets per lane (65 537).  The schedule's strips of 4096 bodies: 4097 is two strips, 65 537 seventeen.

The two bounds the scheme's own conditioning sets, measured on the CPU with the model (float64 replay of a block step against the
longdouble replay, the cases and seeds of test_one_block_step_against_numpy_longdouble, the state before the step made by the
float64 model):
  crackle   largest distance (maxrel) 2.38e-10 (N = 65 537, 3D; 1.14e-10 at N = 2 in 2D, 1.3e-12 .. 7.3e-11 elsewhere): the crackle
            is 60 (a1 - a0) / h^3 - ..., a third difference.  CRACKLE_TOL = 8 x that.
  want      largest relative difference 5.54e-9 (N = 2, 2D, want / h = 4.7; <= 1.7e-9 elsewhere, 1.6e-9 and 1.2e-9 at N = 65 537), no
            level different in any of the ten cases, want / h between 0.15 and 4.7.  LEVEL_EXCUSE = 10 x that.

Per-body bounds in ulps against a wide reference, c != 1 and the ends of the softening range are in tests/test_gpu_hermite_wide.py."""
import ctypes

import numpy as np
import pytest

import hermite6_block_model as M
from hermite6_block_model import LD, TOL, maxrel

pytestmark = pytest.mark.gpu

CRACKLE_TOL = 8 * 2.38e-10
LEVEL_EXCUSE = 10 * 5.54e-9


def e2_of(eps):
    return np.float64(np.float64(eps) * np.float64(eps))


def host_system(nb, m, x, v, dt, c=1.0, dtype=1):
    t = np.float32 if dtype == 0 else np.float64
    hs = nb.HostSystem(dtype, x.shape[1], len(m))
    hs.m[:], hs.x[:], hs.v[:] = m.astype(t), x.astype(t), v.astype(t)
    hs.dt, hs.c = dt, c
    return hs


def random_system(nb, dim, n, seed, dt=0.01):
    return host_system(nb, *M.random_arrays(dim, n, seed), dt)


def binary_cluster(nb, n=512, seed=2024, eps=0.002, sep=0.004, dt=1.0 / 16, dtype=1):
    return host_system(nb, *M.binary_arrays(n, seed, eps, sep), dt, dtype=dtype)


def snapshot(dev):
    """(x, v, a, jerk, snap, crackle), levels and tau as they are on the device."""
    out = dev.download()
    lev, tau = dev.hermite6_block_levels()
    return (out.x.copy(), out.v.copy(), out.a.copy()) + tuple(dev.hermite6_read(w) for w in range(3)), lev, tau


# ---- 1. one block step against NumPy longdouble ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [3, 2])
def test_one_block_step_against_numpy_longdouble(nb, dim):
    """N in {2, 65, 257, 4097, 65537}, seeds 300 + N, eps = 0.05, dt_max = 0.5, max_level = 6, eta_start = 0.3, eta = 0.4.  Three block
    steps bring the bodies to different tau; the fourth is downloaded before and after and replayed in longdouble.  tau_next and the
    active list must be equal; x, v, a, the jerk and the snap of the active bodies (of 256 of them, evenly spread over the list, where
    more are active) within TOL, the crackle within CRACKLE_TOL; every inactive body bitwise untouched in x, v, a, jerk, snap,
    crackle, level and tau; the new levels equal except where longdouble `want` is within LEVEL_EXCUSE of a decision boundary, at most
    1 % of the evaluated bodies.
    Measured on an MI355X (worst over the ten cases): x 7.1e-17, v 1.1e-16, a 4.6e-15, jerk 4.2e-15, snap 3.6e-15, crackle 5.4e-11
    (N = 2, 2D; 3.4e-13 .. 2.6e-11 elsewhere), no level different from longdouble's, want / h between 0.15 and 4.7."""
    T, eps, L, eta_start, eta = np.float64, 0.05, 6, 0.3, 0.4
    e2 = e2_of(eps)
    for n in (2, 65, 257, 4097, 65537):
        hs = random_system(nb, dim, n, seed=300 + n, dt=0.5)
        dev = nb.DeviceSystem.from_host(hs)
        dev.hermite6_block_start(eps, eta_start, L)
        for _ in range(3):
            dev.hermite6_block_step(eps, eta)
        S0, lev0, tau0 = snapshot(dev)
        n_act, nxt = dev.hermite6_block_step(eps, eta)
        act = dev.hermite6_block_active(n_act)
        S1, lev1, tau1 = snapshot(dev)
        dev.close()

        rn, ract, _ = M.schedule(lev0, tau0, L)
        assert nxt == rn and n_act == len(ract) and np.array_equal(act, ract), (n, nxt, rn, n_act, len(ract))
        subset = None if n_act <= 256 else np.unique(np.linspace(0, n_act - 1, 256).astype(np.int64))
        r = M.ref_block_step(T, hs.m, S0, lev0, tau0, hs.dt, L, hs.c, e2, eta, subset=subset)
        t = ract[r["sel"]]
        worst = {k: maxrel(got[t], r[k]) for k, got in zip("xvajsk", S1)}
        inactive = np.ones(n, bool)
        inactive[ract] = False
        for got, old in zip(S1 + (lev1, tau1), S0 + (lev0, tau0)):
            assert np.array_equal(got[inactive], old[inactive]), n
        assert np.array_equal(tau1[ract], np.full(n_act, 0 if nxt == 1 << L else nxt, np.uint32))
        differ = lev1[t] != r["lev"]
        excused = differ & M.near_boundary(r["want"], r["h"], T(hs.dt), L, LEVEL_EXCUSE)
        ratio = r["want"] / r["h"]
        print(f"dim={dim} n={n}: tau_next={nxt} n_act={n_act} levels {np.bincount(lev0, minlength=L + 1).tolist()} "
              + " ".join(f"{k} {w:.3g}" for k, w in worst.items())
              + f" want/h {float(ratio.min()):.3g}..{float(ratio.max()):.3g} levels differ {differ.sum()} excused {excused.sum()} of {len(t)}")
        assert all(worst[k] <= TOL[1] for k in "xvajs"), (n, worst)
        assert worst["k"] <= CRACKLE_TOL, (n, worst)
        assert not (differ & ~excused).any(), (n, lev1[t][differ], r["lev"][differ], r["want"][differ], r["h"][differ])
        assert excused.sum() <= 0.01 * len(t), (n, excused.sum(), len(t))


# ---- 2. active sets in every launch regime -----------------------------------------------------------------------------------------
def test_active_sets_in_every_launch_regime(nb):
    """N = 20 000, one interval of 256 ticks (graded_arrays, eta = eta_start = 0.1): the active sets must include one of at most 64
    bodies, one of 65 .. 2047 (79 chunks of one tile: the reduce kernel) and all N (7 chunks of 12 tiles, added by the corrector).  At
    the first step of each size a, the jerk and the snap of the active bodies (of 256 of them when all are active) against a longdouble
    evaluation at the predicted state the library reports (nbody_hermite6_read 3, 4, 5), within TOL."""
    m, x, v, dt, eps, L = M.graded_arrays(eta=0.1)
    eta = 0.1
    hs = host_system(nb, m, x, v, dt)
    e2 = e2_of(eps)
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite6_block_start(eps, eta, L)
    lev, _ = dev.hermite6_block_levels()
    print("start levels", np.bincount(lev, minlength=L + 1).tolist())
    seen, sizes, nxt = {}, [], 0
    while nxt != 1 << L:
        lev0, tau0 = dev.hermite6_block_levels()
        n_act, nxt = dev.hermite6_block_step(eps, eta)
        sizes.append(n_act)
        rn, ract, _ = M.schedule(lev0, tau0, L)
        assert (nxt, n_act) == (rn, len(ract)), (nxt, rn, n_act, len(ract))
        if n_act in seen:
            continue
        act = dev.hermite6_block_active(n_act)
        assert np.array_equal(act, ract)
        xp, vp, ap = (dev.hermite6_read(w) for w in (3, 4, 5))
        got = (dev.download().a, dev.hermite6_read(0), dev.hermite6_read(1))
        t = act if n_act <= 512 else act[np.unique(np.linspace(0, n_act - 1, 256).astype(np.int64))]
        ref = M.ref_force_jerk_snap(hs.m, xp, vp, ap, hs.c, e2, targets=t)
        seen[n_act] = tuple(maxrel(g[t], r) for g, r in zip(got, ref))
        print(f"tau_next={nxt} n_act={n_act}: a {seen[n_act][0]:.3g} jerk {seen[n_act][1]:.3g} snap {seen[n_act][2]:.3g}")
        assert max(seen[n_act]) <= TOL[1], (n_act, seen[n_act])
    dev.close()
    print("sizes of the active sets:", sorted(set(sizes)))
    assert any(s <= 64 for s in sizes) and any(65 <= s <= 2047 for s in sizes) and hs.n in sizes, sorted(set(sizes))


# ---- 3. max_level = 0 is the fixed step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,n", [(3, 200), (3, 1000), (2, 300), (3, 40000), (3, 65537)])
def test_max_level_0_is_the_fixed_step(nb, dim, n):
    """max_level = 0: one advance is one block step with every body active.  After block_start, one advance and one block step, against
    nbody_hermite6_start and two nbody_hermite6_step at the same dt: a, the jerk and the snap bitwise equal (the same kernel body, the
    same plan, the same chunk order), x and v within TOL, the crackle within 1e-14 of 60 max|a1 - a0| / h^3, the size of the terms it
    is the difference of.  Prints whether everything was bitwise."""
    eps = 0.05
    hs = random_system(nb, dim, n, seed=n)
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite6_block_start(eps, 0.3, 0)
    assert dev.hermite6_block_advance(eps, 0.4) == (1, n)
    assert dev.hermite6_block_step(eps, 0.4) == (n, 1)
    got, lev, tau = snapshot(dev)
    dev.close()
    assert not lev.any() and not tau.any()
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite6_start(eps)
    dev.hermite6_step(eps)
    a0 = dev.download().a.copy()
    dev.hermite6_step(eps)
    out = dev.download()
    ref = (out.x, out.v, out.a) + tuple(dev.hermite6_read(w) for w in range(3))
    dev.close()
    bitwise = [np.array_equal(g, r) for g, r in zip(got, ref)]
    kscale = 60 * np.abs(ref[2] - a0).max() / hs.dt ** 3
    kerr = np.abs(got[5] - ref[5]).max()
    print(f"dim={dim} n={n}: x {maxrel(got[0], ref[0]):.3g} v {maxrel(got[1], ref[1]):.3g} crackle {kerr / kscale:.3g} of 60|a1-a0|/h^3; "
          f"bitwise x v a j s k {bitwise}, all {all(bitwise)}")
    assert bitwise[2] and bitwise[3] and bitwise[4], bitwise
    assert maxrel(got[0], ref[0]) <= TOL[1] and maxrel(got[1], ref[1]) <= TOL[1]
    assert kerr <= 1e-14 * kscale, (kerr, kscale)


# ---- 4. invariants over three intervals --------------------------------------------------------------------------------------------
def test_invariants_over_advances(nb):
    """N = 1000 cluster with a binary, max_level = 8, three intervals stepped one block step at a time: tau_i stays a multiple of the
    body's step, levels stay in [0, L], tau_next strictly increases, all tau_i = 0 after each interval.  The same run through
    block_advance gives the same counts (body_steps = the sum of the n_active) and the same bits."""
    eps, L, eta, eta_start = 0.01, 8, 0.3, 0.01
    hs = binary_cluster(nb, n=1000, eps=eps, sep=0.02)
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite6_block_start(eps, eta_start, L)
    counts = []
    for _ in range(3):
        last, bs, bod = 0, 0, 0
        while last != 1 << L:
            n_act, nxt = dev.hermite6_block_step(eps, eta)
            assert nxt > last and 1 <= n_act <= hs.n
            last, bs, bod = nxt, bs + 1, bod + n_act
            lev, tau = dev.hermite6_block_levels()
            assert lev.min() >= 0 and lev.max() <= L
            step = np.int64(1) << (L - lev.astype(np.int64))
            assert (tau.astype(np.int64) % step == 0).all()
            assert (tau.astype(np.int64) <= nxt % (1 << L)).all()
        assert n_act == hs.n and not tau.any()
        counts.append((bs, bod))
    stepped, _, _ = snapshot(dev)
    dev.close()
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite6_block_start(eps, eta_start, L)
    advanced = [dev.hermite6_block_advance(eps, eta) for _ in range(3)]
    out, lev, tau = snapshot(dev)
    dev.close()
    print(f"(block steps, body steps) per interval {counts}")
    assert advanced == counts and not tau.any()
    assert all(np.array_equal(g, r) for g, r in zip(out, stepped))
    assert counts[0][0] > 1 and counts[0][1] < counts[0][0] * hs.n  # it is a block scheme: not every body at every step


# ---- 5. the point of the feature ---------------------------------------------------------------------------------------------------
def gpu_block_run(nb, hs, eps, eta, eta_start, L, nint, order):
    """`nint` advances of the sixth-order (order 6) or fourth-order (4) block steps: block steps, body steps, |dE / E| (in float64 from
    the uploaded and the downloaded state, as the model's is), the final levels."""
    e2 = e2_of(eps)
    e0 = M.ref_energy(hs.m, hs.x, hs.v, hs.c, e2)
    dev = nb.DeviceSystem.from_host(hs)
    start, advance, levels = ((dev.hermite6_block_start, dev.hermite6_block_advance, dev.hermite6_block_levels) if order == 6 else
                              (dev.hermite_block_start, dev.hermite_block_advance, dev.hermite_block_levels))
    start(eps, eta_start, L)
    bs = bod = 0
    for _ in range(nint):
        s, b = advance(eps, eta)
        bs, bod = bs + s, bod + b
    out = dev.download()
    lev, _ = levels()
    dev.close()
    return bs, bod, abs((M.ref_energy(hs.m, out.x, out.v, hs.c, e2) - e0) / e0), lev


def test_binary_in_a_cluster(nb):
    """N = 512, eps = 0.002, bodies 0 and 1 a circular binary of separation 0.004 (period 0.025), to t = 0.5 with dt_max = 1/16,
    max_level = 12, eta_start = 0.01, eta = 0.3.  Against the float64 model run (583 block steps, 14 827 body steps, |dE / E| 7.0e-9,
    no body deeper than level 6): block steps and body steps within 2 %, |dE / E| at most 4 x the model's.  And against the GPU's own
    fourth-order block run of the same system with eta = 0.02 (1115 block steps, 16 755 body steps, 8.3e-8): a smaller |dE / E| from no
    more body steps."""
    eps, L, eta, eta_start, nint = 0.002, 12, 0.3, 0.01, 8
    hs = binary_cluster(nb)
    e2 = e2_of(eps)
    e0 = M.ref_energy(hs.m, hs.x, hs.v, hs.c, e2)
    x, v, nbs, nbod, deepest = M.ref_block_run(np.float64, hs.m, hs.x, hs.v, hs.dt, L, hs.c, e2, eta, eta_start, nint)
    de_np = abs((M.ref_energy(hs.m, x, v, hs.c, e2) - e0) / e0)
    bs, bod, de_gpu, lev = gpu_block_run(nb, hs, eps, eta, eta_start, L, nint, 6)
    bs4, bod4, de4, _ = gpu_block_run(nb, hs, eps, 0.02, eta_start, L, nint, 4)
    print(f"numpy:       {nbs} block steps, {nbod} body steps ({nbod / hs.n:.1f} N), dE/E {de_np:.3g}, deepest level {deepest}")
    print(f"gpu order 6: {bs} block steps, {bod} body steps ({bod / hs.n:.1f} N), dE/E {de_gpu:.3g}; final levels {np.bincount(lev).tolist()}")
    print(f"gpu order 4: {bs4} block steps, {bod4} body steps ({bod4 / hs.n:.1f} N), dE/E {de4:.3g}")
    assert abs(bs - nbs) <= 0.02 * nbs and abs(bod - nbod) <= 0.02 * nbod, (bs, nbs, bod, nbod)
    assert de_gpu <= 4 * de_np, (de_gpu, de_np)
    assert de_gpu < de4 and bod <= bod4, (de_gpu, de4, bod, bod4)


# ---- 6. repeatability --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 5000])
def test_bitwise_repeatable(nb, n):
    """Two runs of 4 advances from the same upload give the same x, v, a, jerk, snap, crackle and levels bit for bit; so does a run whose
    handle is destroyed after two advances and made again (block_start then restarts the levels from the state on the device, in all
    runs alike)."""
    eps, L, eta, eta_start = 0.01, 10, 0.3, 0.01
    hs = binary_cluster(nb, n=n, eps=eps, sep=0.02)

    def run(remake):
        dev = nb.DeviceSystem.from_host(hs)
        dev.hermite6_block_start(eps, eta_start, L)
        counts = [dev.hermite6_block_advance(eps, eta) for _ in range(2)]
        if remake:
            dev._hermite6.close()
            dev._hermite6 = None
        dev.hermite6_block_start(eps, eta_start, L)
        counts += [dev.hermite6_block_advance(eps, eta) for _ in range(2)]
        S, lev, _ = snapshot(dev)
        dev.close()
        return S, lev, counts

    a, b, c = run(False), run(False), run(True)
    print(f"n={n}: {a[2]}")
    for other in (b, c):
        assert other[2] == a[2]
        assert all(np.array_equal(g, r) for g, r in zip(other[0], a[0])) and np.array_equal(other[1], a[1])


# ---- 7. call sequence --------------------------------------------------------------------------------------------------------------
def test_call_sequence_and_capture(nb):
    """block_step / block_advance / block_read before block_start, and after a later nbody_hermite6_start: NBODY_ERR_STATE.  Under
    capture block_start, block_step, block_advance and block_read return NBODY_ERR_STATE and leave the capture usable: it goes on to
    record a fixed step that replays.  A float handle with a float state is refused at block_start with NBODY_ERR_ARG."""
    L = nb.lib()
    hs = random_system(nb, 3, 300, seed=1)
    dev = nb.DeviceSystem.from_host(hs)
    st, stream = dev.state(), ctypes.c_void_p(dev.stream)
    h = nb.Hermite6(1, 3, 300, dev.device)
    na, tau = ctypes.c_uint32(), ctypes.c_uint32()
    bs, bod = ctypes.c_uint64(), ctypes.c_uint64()
    buf = np.zeros(300, np.int32)
    step = lambda: L.nbody_hermite6_block_step(h.h, ctypes.byref(st), 0.05, 0.4, stream, ctypes.byref(na), ctypes.byref(tau))
    advance = lambda: L.nbody_hermite6_block_advance(h.h, ctypes.byref(st), 0.05, 0.4, stream, ctypes.byref(bs), ctypes.byref(bod))
    start = lambda: L.nbody_hermite6_block_start(h.h, ctypes.byref(st), 0.05, 0.3, 6, stream)
    read = lambda: L.nbody_hermite6_block_read(h.h, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, stream)
    assert (step(), advance(), read()) == (3, 3, 3)
    h.start(st, 0.05, dev.stream)
    assert (step(), advance(), read()) == (3, 3, 3)  # nbody_hermite6_start starts a fixed-step run, not a block run
    other = nb.Hermite6(1, 3, 301, dev.device)
    assert L.nbody_hermite6_block_start(other.h, ctypes.byref(st), 0.05, 0.3, 6, stream) == 1
    other.close()
    assert start() == 0 and step() == 0 and na.value >= 1 and read() == 0
    assert L.nbody_hermite6_block_read(h.h, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes - 4, stream) == 1
    assert L.nbody_hermite6_block_read(h.h, 3, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, stream) == 1
    st2 = dev.state()
    st2.dt = st.dt / 2  # another dt than block_start's
    assert L.nbody_hermite6_block_step(h.h, ctypes.byref(st2), 0.05, 0.4, stream, None, None) == 1
    assert advance() == 0 and bs.value >= 1  # completes the interval: synchronous again, a fixed step may follow
    h.step(st, 0.05, dev.stream)
    h.start(st, 0.05, dev.stream)
    assert (step(), advance(), read()) == (3, 3, 3)  # a later nbody_hermite6_start ends the block run
    assert start() == 0
    assert L.nbody_graph_begin(stream) == 0
    try:
        rcs = (start(), step(), advance(), read())
        h.step(st, 0.05, dev.stream)
    finally:
        g = ctypes.c_void_p()
        rc_end = L.nbody_graph_end(stream, ctypes.byref(g))
    assert rcs == (3, 3, 3, 3) and rc_end == 0
    before = dev.download().x.copy()
    assert L.nbody_graph_launch(g, stream) == 0
    dev.sync()
    assert not np.array_equal(dev.download().x, before)
    L.nbody_graph_destroy(g)
    assert start() == 0 and advance() == 0  # and block steps work again after the capture
    h.close()
    dev.close()
    # float: refused with NBODY_ERR_ARG before anything is allocated or launched
    m, x, v = M.random_arrays(3, 300, 1)
    fdev = nb.DeviceSystem.from_host(host_system(nb, m, x, v, 0.01, dtype=0))
    fst = fdev.state()
    fh = nb.Hermite6(0, 3, 300, fdev.device)
    assert L.nbody_hermite6_block_start(fh.h, ctypes.byref(fst), 0.05, 0.3, 6, ctypes.c_void_p(fdev.stream)) == 1
    assert b"NBODY_F64" in L.nbody_last_error()
    assert L.nbody_hermite6_block_step(fh.h, ctypes.byref(fst), 0.05, 0.4, ctypes.c_void_p(fdev.stream), None, None) == 1
    fh.start(fst, 0.05, fdev.stream)  # the fixed step is there in float
    fh.step(fst, 0.05, fdev.stream)
    fdev.sync()
    fh.close()
    fdev.close()
