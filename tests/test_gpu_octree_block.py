"""GPU: block (individual) time steps of the octree leapfrog (nbody_octree_block_*) against a NumPy restatement of the scheme of
include/nbody_hip.h written here (the reference has one shared step, so there are no fixtures).

The force of a block step is pinned with no tolerance: the predicted positions are uploaded into a second DeviceSystem and the public
octree_force(theta, softening=eps) on it must give the active rows bit for bit.  Everything around the force is one or two operations
per body and is held to bounds that follow from the number formats:
  predictor   xp = fma(h, fma(h/2, a, v), x) with h = T(tau_next - tau_i) * T(tick) a number of T by definition: against longdouble
              the error is at most the inner and the outer FMA's rounding; the bound is THREE roundings, 3 u (|x| + |h v| + |h^2/2 a|)
              per coordinate, u = eps(T) / 2 (a third covers h where T(dtau) * tick is not exact);
  kick        v = fma(h/2, a0 + a1, v0): the sum's and the FMA's rounding; bound 3 u (|v0| + |h/2| (|a0| + |a1|)) per coordinate;
  levels      want = sqrt(k / sqrt(|a1|^2)), k = T(2) T(eta) T(eps).  Its relative error in T against longdouble, measured on the CPU
              over 4e6 random accelerations spanning five decades (NumPy in T against NumPy longdouble): 2.43e-16 in float64, 1.27e-7
              in float32.  A level may differ from the longdouble one only where want lies within 4 x that (LEVEL_EXCUSE: 9.7e-16,
              5.1e-7) of a decision boundary (h, 2 h, a step dt_max 2^-l), and for at most 1 % of the active bodies.
N in {2, 65, 257, 4097, 65537}: the schedule's strips of 4096 positions (4097: two strips, 65537: seventeen) and the walk's bodies per
wave (8 in 3D, 16 in 2D: 65 and 257 end a wave after one body) are crossed.

The figures an MI355X gave are in the tests' docstrings, on the lines marked `measured`."""
import ctypes
import os
import struct
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

LD = np.longdouble
LEVEL_EXCUSE = {1: 4 * 2.43e-16, 0: 4 * 1.27e-7}
SIZES = [2, 65, 257, 4097, 65537]


def npt(dtype):
    return np.float32 if dtype == 0 else np.float64


def unit_roundoff(dtype):
    return LD(np.finfo(npt(dtype)).eps) / 2


def nrm(a):
    return np.sqrt((a * a).sum(-1))


def k_of(T, eta, eps):
    return T(T(2) * T(eta) * T(eps))


def want_of(a, k, ft):
    """sqrt(k / |a|) in `ft`, k a number of T; |a| = 0: no limit."""
    an = nrm(np.asarray(a, ft))
    with np.errstate(divide="ignore"):
        return np.where(an > 0, np.sqrt(ft(k) / np.where(an > 0, an, 1)), ft(np.inf))


def level_for(want, dtmax, L):
    """The smallest level l with dtmax 2^-l <= want, clamped to [0, L] (the steps are exact scalings of dtmax)."""
    steps = dtmax * (want.dtype.type(2) ** -np.arange(L + 1))
    return np.minimum((steps[None, :] > np.asarray(want)[:, None]).sum(1), L).astype(np.int64)


def schedule(lev, tau, L):
    step = np.int64(1) << (L - lev.astype(np.int64))
    due = tau.astype(np.int64) + step
    nxt = int(due.min())
    return nxt, np.nonzero(due == nxt)[0], step


def new_levels(want, l, h, dtmax, L, nxt, step):
    """The rule of a block step for the active bodies: levels l, steps h (time) and `step` (ticks), due at nxt."""
    down = want < h
    deeper = np.minimum(np.maximum(l + 1, level_for(want, dtmax, L)), L)
    up = (~down) & (want >= 2 * h) & (l > 0) & (nxt % (2 * step) == 0)
    return np.where(down, deeper, np.where(up, l - 1, l))


def near_boundary(want, h, dtmax, L, tol):
    """want within a relative tol of h, 2 h or one of the steps dtmax 2^-l."""
    ft = want.dtype.type
    b = np.concatenate([np.stack([h, 2 * h], 1), np.broadcast_to(ft(dtmax) * ft(2) ** -np.arange(L + 1), (len(h), L + 1))], 1)
    return (np.abs(want[:, None] - b) <= ft(tol) * b).any(1)


def step_sizes(T, dt, L, nxt, tau):
    """tick and h_i = T(tau_next - tau_i) * T(tick), numbers of T."""
    tick = T(T(dt) * T(2.0 ** -L))
    return tick, np.asarray(nxt - tau.astype(np.int64), T) * tick


def soft_force(m, x, c, e2, ft, targets=None):
    """a_i = c sum_j m_j d / (|d|^2 + e2)^(3/2), d = x_j - x_i, in `ft`, for the targets only (direct sum)."""
    m, x = np.asarray(m, ft), np.asarray(x, ft)
    idx = np.arange(len(m)) if targets is None else np.asarray(targets)
    a = np.zeros((len(idx), x.shape[1]), ft)
    step = max(1, min(256, (1 << 21) // len(m)))
    for s in range(0, len(idx), step):
        t = idx[s:s + step]
        d = x[None, :, :] - x[t][:, None, :]
        q = (d * d).sum(-1) + ft(e2)
        a[s:s + step] = ((m[None, :] / (q * np.sqrt(q)))[:, :, None] * d).sum(1)
    return ft(c) * a


def random_system(nb, dtype, dim, n, seed, c=1.0, dt=0.5, core=False):
    """A Gaussian cluster; core: every body's radius scaled by 10^U(-1.5, 0.5), a dense centre whose accelerations span two decades, so
    that the levels of one system spread over five or six values."""
    rng = np.random.default_rng(seed)
    t = npt(dtype)
    hs = nb.HostSystem(dtype, dim, n)
    hs.m[:] = rng.uniform(0.5, 1.5, n).astype(t) / n
    hs.x[:] = (rng.normal(0, 1, (n, dim)) * (10.0 ** rng.uniform(-1.5, 0.5, (n, 1)) if core else 1.0)).astype(t)
    hs.v[:] = rng.normal(0, 0.3, (n, dim)).astype(t)
    hs.dt, hs.c = dt, c
    return hs


def binary_cluster(nb, dtype, n=512, seed=2024, eps=0.002, sep=0.004, dt=1.0 / 16):
    """tests/test_gpu_hermite_block.py's: a Gaussian cluster (sigma_x = 1, sigma_v = 0.3, m = 1 / N, c = 1) with bodies 0 and 1 made a
    circular binary of separation `sep` (circular in the softened potential)."""
    rng = np.random.default_rng(seed)
    m = np.full(n, 1.0 / n)
    x, v = rng.normal(0, 1, (n, 3)), rng.normal(0, 0.3, (n, 3))
    vc = np.sqrt((m[0] + m[1]) / sep) * (sep * sep / (sep * sep + eps * eps)) ** 0.75
    x[1] = x[0] + [sep, 0, 0]
    v[1] = v[0] + [0, vc, 0]
    t = npt(dtype)
    hs = nb.HostSystem(dtype, 3, n)
    hs.m[:], hs.x[:], hs.v[:] = m.astype(t), x.astype(t), v.astype(t)
    hs.dt, hs.c = dt, 1.0
    return hs


def snapshot(dev):
    """x, v, a, levels and tau as they are on the device."""
    out = dev.download()
    lev, tau = dev.octree_block_levels()
    return out, lev, tau


def public_force(nb, hs, x, theta, eps):
    """The public octree_force(theta, softening=eps) of a second DeviceSystem whose positions are x: its accelerations."""
    h2 = nb.HostSystem(hs.dtype, hs.dim, hs.n)
    h2.m[:], h2.x[:], h2.v[:], h2.dt, h2.c = hs.m, x, hs.v, hs.dt, hs.c
    d2 = nb.DeviceSystem.from_host(h2)
    d2.octree_force(theta, softening=eps)
    d2.octree.info(d2.stream)
    a = d2.download().a.copy()
    d2.close()
    return a


# ---- 1 .. 5: the fourth block step, taken apart -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [0.5, 0.0])
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_one_block_step_taken_apart(nb, dtype, dim, theta):
    """N in SIZES (clusters with a dense core: levels 0 .. 5), eps = 0.05, dt_max = 0.5, max_level = 6, eta = 0.05.  Three block steps bring the bodies to different tau; the fourth is
    downloaded before and after.  Schedule: tau_next, n_active and the active list equal NumPy's exactly.  Predictor, kick: against
    longdouble under the derived bounds of the module docstring.  Force: the active rows equal the public softened octree force on xp
    bit for bit.  x of the active bodies is xp bitwise, tau is tau_next (0 at the end of the interval), every inactive body's x, v, a,
    level and tau are bitwise untouched.  Levels: NumPy longdouble's from the downloaded a1, excuses as in the module docstring.
    measured on an MI355X: predictor at most 0.60 (double) / 0.59 (float) of its bound and the kick 0.66 / 0.66 over the 40 cases; no
    force row, no inactive body and no level differs in any case (0 excused), and the NumPy-in-T levels equal longdouble's too.  The
    fourth step is at tick 8 of 64 (tick 7 for N = 4097 in 2D) with 50 of 65, 201 of 257, 3131 of 4097 and 50 113 of 65 537 bodies
    active in 3D, 54, 213, 163 and 54 445 in 2D (theta = 0: 50 103; 54, 214, 132, 54 537); N = 2: both bodies."""
    eps, L, eta = 0.05, 6, 0.05
    T, u = npt(dtype), unit_roundoff(dtype)
    for n in SIZES:
        hs = random_system(nb, dtype, dim, n, seed=100 + n, core=True)
        dev = nb.DeviceSystem.from_host(hs)
        dev.octree_block_start(theta, eps, eta, L)
        for _ in range(3):
            dev.octree_block_step(theta, eps, eta)
        b, lev0, tau0 = snapshot(dev)
        n_act, nxt = dev.octree_block_step(theta, eps, eta)
        dev.octree.info(dev.stream)
        act = dev.octree_block_active(n_act)
        xp = dev.octree_block_predicted()
        a, lev1, tau1 = snapshot(dev)
        dev.close()
        # 1. schedule
        r_nxt, r_act, step = schedule(lev0, tau0, L)
        assert (nxt, n_act) == (r_nxt, len(r_act)) and np.array_equal(act, r_act), (n, nxt, r_nxt, n_act, len(r_act))
        # 2. predictor
        tick, h = step_sizes(T, hs.dt, L, nxt, tau0)
        hl = h.astype(LD)[:, None]
        x0, v0, a0 = (np.asarray(q, LD) for q in (b.x, b.v, b.a))
        ref_xp = x0 + hl * v0 + hl * hl / LD(2) * a0
        bound = 3 * u * (np.abs(x0) + np.abs(hl * v0) + np.abs(hl * hl / LD(2) * a0))
        err = np.abs(xp.astype(LD) - ref_xp)
        worst_p = float((err / np.maximum(bound, LD(1e-4900))).max())
        assert (err <= bound).all(), (n, worst_p)
        # 3. force, bitwise
        a1 = public_force(nb, hs, xp, theta, eps)
        assert np.array_equal(a.a[act], a1[act]), (n, np.nonzero((a.a[act] != a1[act]).any(1))[0][:8])
        # 4. kick
        ha = hl[act]
        ref_v = v0[act] + ha / LD(2) * (a0[act] + a1[act].astype(LD))
        bound = 3 * u * (np.abs(v0[act]) + np.abs(ha / LD(2)) * (np.abs(a0[act]) + np.abs(a1[act].astype(LD))))
        err = np.abs(a.v[act].astype(LD) - ref_v)
        worst_k = float((err / np.maximum(bound, LD(1e-4900))).max())
        assert (err <= bound).all(), (n, worst_k)
        assert np.array_equal(a.x[act], xp[act])
        assert (tau1[act] == (0 if nxt == 1 << L else nxt)).all()
        off = np.ones(n, bool)
        off[act] = False
        for name, before, after in (("x", b.x, a.x), ("v", b.v, a.v), ("a", b.a, a.a), ("lev", lev0, lev1), ("tau", tau0, tau1)):
            assert np.array_equal(before[off], after[off]), (n, name)
        # 5. levels
        k = k_of(T, eta, eps)
        hh, l = h[act], lev0[act].astype(np.int64)
        want = want_of(a1[act], k, LD)
        ref_lev = new_levels(want, l, hh.astype(LD), LD(T(hs.dt)), L, nxt, step[act])
        bad = lev1[act] != ref_lev
        excused = bad & near_boundary(want, hh.astype(LD), T(hs.dt), L, LEVEL_EXCUSE[dtype])
        t_lev = new_levels(want_of(a1[act], k, T), l, hh, T(hs.dt), L, nxt, step[act])  # the NumPy-in-T replay against longdouble
        assert n_act < n or n == 2, "the fourth step of this case leaves nobody inactive: nothing is shown about inactive bodies"
        print(f"dtype={dtype} dim={dim} theta={theta} n={n}: tau_next {nxt} n_active {n_act}, predictor {worst_p:.3g} kick {worst_k:.3g} "
              f"of their bounds, levels differing {int(bad.sum())} (excused {int(excused.sum())}), numpy-in-T differing "
              f"{int((t_lev != ref_lev).sum())}; new levels {np.bincount(lev1, minlength=L + 1).tolist()}")
        assert (t_lev != ref_lev).sum() <= 0.01 * n_act, "the case itself sits on decision boundaries: choose another seed"
        assert not (bad & ~excused).any(), (n, np.nonzero(bad & ~excused)[0][:8])
        assert excused.sum() <= 0.01 * n_act, (n, int(excused.sum()), n_act)


# ---- 6. max_level = 0 -----------------------------------------------------------------------------------------------------------------------
def fma_exact(T, a, b, c):
    """fl_T(a * b + c) element by element, with one rounding (rational arithmetic; float(Fraction) rounds correctly)."""
    out = np.empty(a.shape, T)
    fa, fb, fc, fo = a.ravel(), np.broadcast_to(b, a.shape).ravel(), c.ravel(), out.ravel()
    for i in range(fa.size):
        fo[i] = T(float(Fraction(float(fa[i])) * Fraction(float(fb[i])) + Fraction(float(fc[i]))))
    return out


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_max_level_0_is_predictor_public_force_kick(nb, dtype, dim):
    """max_level = 0: every body is active in every block step (n_active = N, tau_next = 1), and the step equals, bit for bit, the
    composition made here: the predictor xp = fma(h, fma(h/2, a, v), x) evaluated with exactly rounded FMAs in rational arithmetic, the
    public octree_force(theta, softening=eps) on xp, and the kick v = fma(h/2, a0 + a1, v0), x = xp, a = a1.  (A float FMA emulated
    through a correctly rounded double can round twice; that would show as a one-ulp difference in a single coordinate, not seen.)
    measured on an MI355X: bitwise equal in all 20 cases (4 x 5 sizes)."""
    theta, eps, eta = 0.5, 0.05, 0.05
    T = npt(dtype)
    for n in SIZES:
        hs = random_system(nb, dtype, dim, n, seed=200 + n, dt=0.125)
        dev = nb.DeviceSystem.from_host(hs)
        dev.octree_block_start(theta, eps, eta, 0)
        b, lev, tau = snapshot(dev)
        assert np.array_equal(b.a, public_force(nb, hs, hs.x, theta, eps))  # start: the public force of all bodies
        assert (lev == 0).all() and (tau == 0).all()
        n_act, nxt = dev.octree_block_step(theta, eps, eta)
        assert (n_act, nxt) == (n, 1)
        assert np.array_equal(dev.octree_block_active(n), np.arange(n))
        xp = dev.octree_block_predicted()
        a, lev, tau = snapshot(dev)
        dev.close()
        h = T(T(1) * T(hs.dt))
        hh = T(h * T(0.5))
        ref_xp = fma_exact(T, np.full_like(b.x, h), fma_exact(T, np.full_like(b.x, hh), b.a, b.v), b.x)
        assert np.array_equal(xp, ref_xp), (n, int((xp != ref_xp).sum()))
        a1 = public_force(nb, hs, ref_xp, theta, eps)
        ref_v = fma_exact(T, np.full_like(b.x, hh), (b.a + a1).astype(T), b.v)
        assert np.array_equal(a.a, a1) and np.array_equal(a.x, ref_xp), n
        assert np.array_equal(a.v, ref_v), (n, int((a.v != ref_v).sum()))
        assert (lev == 0).all() and (tau == 0).all()
        print(f"dtype={dtype} dim={dim} n={n}: bitwise equal")


# ---- 7. two runs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,dim,n", [(1, 3, 4097), (0, 3, 4097), (1, 2, 257), (0, 2, 65537)])
def test_two_runs_give_the_same_bits(nb, dtype, dim, n):
    """Two runs of one interval from the same upload: identical x, v, a, levels, block and body step counts.
    measured on an MI355X: identical; (block steps, body steps) = (58, 97 959) / (58, 97 959) / (61, 7 213) / (60, 1 844 968)."""
    theta, eps, eta, L = 0.5, 0.05, 0.05, 6
    hs = random_system(nb, dtype, dim, n, seed=300 + n, core=True)

    def run():
        dev = nb.DeviceSystem.from_host(hs)
        dev.octree_block_start(theta, eps, eta, L)
        counts = dev.octree_block_advance(theta, eps, eta)
        dev.octree.info(dev.stream)
        out, lev, tau = snapshot(dev)
        dev.close()
        return out, lev, tau, counts

    a, b = run(), run()
    print(f"dtype={dtype} dim={dim} n={n}: (block steps, body steps) = {a[3]}")
    assert a[3] == b[3] and a[3][0] >= 1 and a[3][1] >= n
    assert (a[2] == 0).all()
    for name in ("x", "v", "a"):
        assert np.array_equal(getattr(a[0], name), getattr(b[0], name)), name
    assert np.array_equal(a[1], b[1])


# ---- 8. the point of the feature ----------------------------------------------------------------------------------------------------------
STEP_COUNT_MEASURED = (0, 0)  # |GPU - NumPy| in (block steps, body steps), measured once on an MI355X; the bound is twice that


def ref_block_run(m, x, v, dt, L, c, e2, k, nint):
    """`nint` intervals of dt with block steps in float64, the force by direct sums: x, v, block steps, body steps."""
    T = np.float64
    m, x, v = np.asarray(m, T), np.asarray(x, T).copy(), np.asarray(v, T).copy()
    a = soft_force(m, x, c, e2, T)
    lev = level_for(want_of(a, k, T), T(dt), L)
    bsteps = bodysteps = 0
    for _ in range(nint):
        tau = np.zeros(len(m), np.int64)
        while True:
            nxt, act, step = schedule(lev, tau, L)
            _, h = step_sizes(T, dt, L, nxt, tau)
            xp = x + h[:, None] * v + h[:, None] * h[:, None] / 2 * a
            a1 = soft_force(m, xp, c, e2, T, targets=act)
            ha = h[act]
            v[act] += ha[:, None] / 2 * (a[act] + a1)
            x[act], a[act] = xp[act], a1
            lev[act] = new_levels(want_of(a1, k, T), lev[act], ha, T(dt), L, nxt, step[act])
            tau[act] = nxt
            bsteps += 1
            bodysteps += len(act)
            if nxt == 1 << L:
                assert len(act) == len(m)
                break
    return x, v, bsteps, bodysteps


def test_binary_in_a_cluster_holds_the_energy(nb):
    """binary_cluster, N = 512 double, eps = 0.002, bodies 0 and 1 a circular binary of separation 0.004 (period 0.025); theta = 0, so the
    force is conservative to rounding.  To t = 0.5 in 8 intervals of dt_max = 1/16 with max_level = 12 and eta = 0.02; |dE / E| is the
    largest over the 8 synchronous times, from calc_energies(softening=eps).  The comparison is the fixed-step octree leapfrog
    (octree_force(0, softening=eps) + accelerate_step) on the same GPU over the same time with at least as many force evaluations as
    the block run's body steps: ceil(body steps / N) steps, rounded up to a multiple of 8, sampled at the same 8 times.  The block run's
    |dE / E| must be smaller.  Block and body steps against the float64 NumPy model of the run (direct sums): within twice the
    difference measured once (STEP_COUNT_MEASURED).
    measured on an MI355X: GPU 1024 block steps, 19 386 body steps (37.9 N), final levels [0, 8, 474, 28, 0, 0, 0, 2] (the binary at
    level 7); the NumPy model the same counts (difference 0 block steps, 0 body steps, so the bound is equality); max |dE / E| 7.62e-5
    against the fixed step's 5.56e-2 with 40 steps (20 480 evaluations): the fixed step's is 729 x the block steps'."""
    theta, eps, L, eta, nint = 0.0, 0.002, 12, 0.02, 8
    hs = binary_cluster(nb, 1)
    T = np.float64
    e2 = T(T(eps) * T(eps))
    _, _, nbs, nbod = ref_block_run(hs.m, hs.x, hs.v, hs.dt, L, hs.c, e2, k_of(T, eta, eps), nint)

    def drift(e, e0):
        return abs((float(e[0]) + float(e[1]) - e0) / e0)

    dev = nb.DeviceSystem.from_host(hs)
    k0, p0 = dev.calc_energies(softening=eps)
    e0 = float(k0) + float(p0)
    dev.octree_block_start(theta, eps, eta, L)
    bs = bod = 0
    de_block = 0.0
    for _ in range(nint):
        s, b = dev.octree_block_advance(theta, eps, eta)
        bs, bod = bs + s, bod + b
        de_block = max(de_block, drift(dev.calc_energies(softening=eps), e0))
    dev.octree.info(dev.stream)
    lev, _ = dev.octree_block_levels()
    dev.close()
    nfixed = -(-(-(-bod // hs.n)) // nint) * nint  # ceil(body steps / N), up to a multiple of nint
    fx = binary_cluster(nb, 1, dt=hs.dt * nint / nfixed)
    dev = nb.DeviceSystem.from_host(fx)
    de_fixed = 0.0
    for i in range(nfixed):
        dev.octree_force(theta, softening=eps)
        dev.accelerate_step()
        if (i + 1) % (nfixed // nint) == 0:
            de_fixed = max(de_fixed, drift(dev.calc_energies(softening=eps), e0))
    dev.octree.info(dev.stream)
    dev.close()
    print(f"numpy: {nbs} block steps, {nbod} body steps ({nbod / hs.n:.1f} N)")
    print(f"gpu:   {bs} block steps, {bod} body steps ({bod / hs.n:.1f} N), max dE/E {de_block:.3g}; final levels {np.bincount(lev).tolist()}")
    print(f"difference to numpy: {abs(bs - nbs)} block steps, {abs(bod - nbod)} body steps (measured once: {STEP_COUNT_MEASURED})")
    print(f"gpu fixed step, {nfixed} steps ({nfixed * hs.n} evaluations): max dE/E {de_fixed:.3g} ({de_fixed / de_block:.3g} x the block steps')")
    assert nfixed * hs.n >= bod
    assert de_block < de_fixed, (de_block, de_fixed)
    assert abs(bs - nbs) <= 2 * STEP_COUNT_MEASURED[0] and abs(bod - nbod) <= 2 * STEP_COUNT_MEASURED[1], (bs, nbs, bod, nbod)


# ---- 9. CLI ------------------------------------------------------------------------------------------------------------------------------
def read_energies(path):
    raw = open(path, "rb").read()
    steps, tsz = struct.unpack("<2I", raw[:8])
    return steps, np.frombuffer(raw[8:], dtype=np.float32 if tsz == 4 else np.float64).reshape(-1, 2)


@pytest.mark.parametrize("tree_energy", [False, True])
def test_cli_block_steps_run_and_save(nb, tree_energy):
    """-n 4096 --workload galaxy --softening 0.05 --block-eta 0.02 -s 4 --save energy (with and without --tree-energy): without
    --csv-detailed the run completes and saves the first frame; with it, the octree CSV line is printed, the time goes to the force
    column, and energy.bin holds the 5 frames of the existing layout, all finite.  The drift is recorded beside the same run without
    --block-eta, not asserted.
    measured on an MI355X: max |dE / E| over the 4 saved steps 3.22e-7 with --block-eta 0.02 (the same with --block-levels 4) against
    4.02e-5 without it (exact sum); 3.08e-6 against 4.35e-5 with --tree-energy."""
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")
    base = ["-n", "4096", "--workload", "galaxy", "--softening", "0.05", "-s", "4", "--save", "energy"] + (["--tree-energy"] if tree_energy else [])
    block = ["--block-eta", "0.02"]
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run([exe] + base + block, cwd=d, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "Done simulation" in r.stdout, (r.stdout, r.stderr)
        steps, en = read_energies(os.path.join(d, "energy.bin"))
        assert steps == 4 and en.shape == (1, 2) and np.isfinite(en).all()
        drift = {}
        for name, extra in (("block", block), ("block L=4", block + ["--block-levels", "4"]), ("fixed", [])):
            r = subprocess.run([exe] + base + extra + ["--csv-detailed"], cwd=d, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, (name, r.stderr)
            lines = r.stdout.splitlines()
            assert lines[0].startswith("algorithm,dim,precision,nsteps,nbodies,total [s],force [s],accel [s],clear [s]"), lines
            row = lines[-1].split(",")
            assert row[:5] == ["octree", "3", "32", "4", "4096"] and len(row) == 13, row
            if extra:
                assert [float(c) for c in row[7:]] == [0.0] * 6, row  # the advance's time is the force column's
            steps, en = read_energies(os.path.join(d, "energy.bin"))
            assert steps == 4 and en.shape == (5, 2) and np.isfinite(en).all(), (name, en)
            e = en.astype(np.float64).sum(1)
            drift[name] = np.abs((e - e[0]) / e[0]).max()
    print(f"tree_energy={tree_energy}: max |dE / E| over the 4 saved steps:", {k: f"{v:.3g}" for k, v in drift.items()})


# ---- 10. errors ----------------------------------------------------------------------------------------------------------------------------
def test_call_sequence_walk_form_and_capture(nb):
    """step / advance / read before start: NBODY_ERR_STATE.  After nbody_octree_set_walk(t, 2), start returns NBODY_ERR_ARG with the
    softened walk's message.  A step inside a capture returns NBODY_ERR_STATE (so do start, advance and read) and the capture still
    ends cleanly: it goes on to record a fixed step that replays; block steps work again afterwards."""
    L = nb.lib()
    n = 300
    hs = random_system(nb, 1, 3, n, seed=1)
    dev = nb.DeviceSystem.from_host(hs)
    st, stream = dev.state(), ctypes.c_void_p(dev.stream)
    t, h = dev.octree, nb.OctreeBlock(1, 3, n, dev.device)
    na, tau = ctypes.c_uint32(), ctypes.c_uint32()
    bs, bod = ctypes.c_uint64(), ctypes.c_uint64()
    buf = np.zeros(n, np.int32)
    sref = ctypes.byref(st)
    step = lambda: L.nbody_octree_block_step(h.h, t.h, sref, 0.5, 0.05, 0.05, stream, ctypes.byref(na), ctypes.byref(tau))
    advance = lambda: L.nbody_octree_block_advance(h.h, t.h, sref, 0.5, 0.05, 0.05, stream, ctypes.byref(bs), ctypes.byref(bod))
    start = lambda: L.nbody_octree_block_start(h.h, t.h, sref, 0.5, 0.05, 0.05, 6, stream)
    read = lambda what=0, nbytes=buf.nbytes: L.nbody_octree_block_read(h.h, what, buf.ctypes.data_as(ctypes.c_void_p), nbytes, stream)
    assert (step(), advance(), read()) == (3, 3, 3)
    t.set_walk(2)
    assert start() == 1 and b"softened walk" in L.nbody_last_error() and b"nbody_octree_set_walk" in L.nbody_last_error()
    assert (step(), read()) == (1, 3)  # still not started
    t.set_walk(0)
    other = nb.OctreeBlock(1, 3, n + 1, dev.device)
    assert L.nbody_octree_block_start(other.h, t.h, sref, 0.5, 0.05, 0.05, 6, stream) == 1
    other.close()
    assert start() == 0 and read() == 0 and read(1) == 0
    assert read(2, 0) == 3 and b"block_step" in L.nbody_last_error()  # the active list and xp exist after a block step
    assert step() == 0 and 1 <= na.value <= n and 1 <= tau.value <= 64
    assert read(0, buf.nbytes - 4) == 1 and read(4) == 1 and read(2, 4 * na.value) == 0
    st2 = dev.state()
    st2.dt = st.dt / 2  # another dt than start's
    assert L.nbody_octree_block_step(h.h, t.h, ctypes.byref(st2), 0.5, 0.05, 0.05, stream, None, None) == 1
    assert advance() == 0 and bs.value >= 1 and bod.value >= n
    t.set_walk(2)
    assert step() == 1 and b"softened walk" in L.nbody_last_error()
    t.set_walk(0)
    assert L.nbody_graph_begin(stream) == 0
    try:
        rcs = (start(), step(), advance(), read())
        dev.octree_force(0.5, softening=0.05)
        dev.accelerate_step()
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
    dev.octree.info(dev.stream)
    h.close()
    dev.close()
