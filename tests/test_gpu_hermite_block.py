"""GPU: block (individual) time steps of the Hermite integrator (nbody_hermite_block_*) against a NumPy restatement of the scheme of
include/nbody_hip.h written here (the reference has no Hermite, so there are no fixtures): np.longdouble for single block steps and
single evaluations, float64 / float32 for runs.

Launch-shape boundaries of hermite_block_plan_for(sz, n_act, 1) (csrc/hermite_block_plan.hpp) crossed below.  Over n_act: the block of 64
targets (63 / 64 / 65: one block, then two), two targets per lane from 65536 active bodies on (max_level = 0 at 65 536 and 70 001
bodies, all active), and the cut of the
source tiles over grid.y, which is ceil(2048 / blocks) chunks capped at one chunk per tile of 256 sources: at N = 20 000 (79 tiles)
n_act = 1 .. 64 gives 79 chunks of one tile, 65 (2 blocks) still 79, 365 (6 blocks) 79, 20 000 (313 blocks) 7 chunks of 12 tiles — the
plan of the fixed step; at N = 65 537 (257 tiles) a small active set takes 257 chunks.  Over N: one tile / two tiles (257), N = 2
(one tile, one chunk, n_act 1 or 2).  The schedule's strips of 4096 bodies: 4097 is two strips, 65 537 seventeen.

Measured on an MI355X (max|got - ref| / max|ref|, worst over the cases): one block step x 6.0e-17, v 1.5e-16, a 3.6e-15, jerk
2.3e-15 in double and 3.8e-8, 4.6e-8, 1.9e-6, 1.9e-6 in float, no level different from NumPy's in any case; the graded active sets a
3.4e-16, jerk 4.1e-16; max_level = 0 bitwise equal to nbody_hermite_step in all four cases; the binary in a cluster 1115 block steps,
16 755 body steps, |dE / E| 8.34e-8 — NumPy's to the printed digits — against the fixed step's 2.15e-2 (2.6e5 x), final x within 3.0e-14 of NumPy's; in float 339 block steps / 14 499
body steps against float64's 334 / 14 496, |dE / E| 3.4e-8 under a bound of 4 x 6.75e-8, the trajectory at 0.86 x its yardstick
(9.7e-7); CLI max |dE / E| over 8 steps 1.2e-6 with --hermite-eta 0.02 against 0.49 without.

Per-body bounds in ulps against a wide reference, c != 1 and the ends of the softening range are in tests/test_gpu_hermite_wide.py."""
import ctypes
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

TOL = {1: 1e-12, 0: 2e-5}  # tests/test_gpu_hermite.py's bound for a summed force (and the jerk) against NumPy longdouble
LEVEL_EXCUSE = {1: 1e-9, 0: 1e-4}  # a level may differ from NumPy's where longdouble `want` is this close to a decision boundary
LD = np.longdouble


def maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def npt(dtype):
    return np.float32 if dtype == 0 else np.float64


def e2_of(dtype, eps):
    t = npt(dtype)
    return t(t(eps) * t(eps))


def nrm(a):
    return np.sqrt((a * a).sum(-1))


def ref_force_jerk(m, x, v, c, e2, dt=LD, targets=None, reverse=False):
    """a_i = c sum_j m_j d q^(-3/2), j_i = c sum_j m_j (u - 3 (d.u)/q d) q^(-3/2); d = x_j - x_i, u = v_j - v_i, q = |d|^2 + e2, in `dt`,
    for the targets only.  reverse: sources summed in reversed order."""
    m, x, v = np.asarray(m, dt), np.asarray(x, dt), np.asarray(v, dt)
    ms, xs, vs = (m[::-1], x[::-1], v[::-1]) if reverse else (m, x, v)
    idx = np.arange(len(m)) if targets is None else np.asarray(targets)
    a, j = np.zeros((len(idx), x.shape[1]), dt), np.zeros((len(idx), x.shape[1]), dt)
    step = max(1, min(256, (1 << 21) // len(m)))
    for s in range(0, len(idx), step):
        t = idx[s:s + step]
        d = xs[None, :, :] - x[t][:, None, :]
        u = vs[None, :, :] - v[t][:, None, :]
        q = (d * d).sum(-1) + dt(e2)
        du = (d * u).sum(-1)
        w = ms[None, :] / (q * np.sqrt(q))
        a[s:s + step] = (w[:, :, None] * d).sum(1)
        j[s:s + step] = (w[:, :, None] * (u - (dt(3) * du / q)[:, :, None] * d)).sum(1)
    return dt(c) * a, dt(c) * j


def level_for(want, dtmax, L):
    """The smallest level l with dtmax 2^-l <= want, clamped to [0, L] (the steps are exact scalings of dtmax)."""
    steps = dtmax * (want.dtype.type(2) ** -np.arange(L + 1))
    return np.minimum((steps[None, :] > np.asarray(want)[:, None]).sum(1), L).astype(np.int64)


def start_levels(a, j, eta_start, dtmax, L, ft):
    an, jn = nrm(np.asarray(a, ft)), nrm(np.asarray(j, ft))
    want = np.where(jn > 0, ft(eta_start) * an / np.where(jn > 0, jn, 1), ft(np.inf))
    return level_for(want, ft(dtmax), L), want


def schedule(lev, tau, L):
    step = np.int64(1) << (L - lev.astype(np.int64))
    due = tau.astype(np.int64) + step
    nxt = int(due.min())
    return nxt, np.nonzero(due == nxt)[0], step


def ref_block_step(T, m, x, v, a, j, lev, tau, dt, L, c, e2, eta, ft=LD, subset=None, reverse=False):
    """One block step of the scheme from the state as downloaded, in `ft`.  dt, the tick and h_i = T(tau_next - tau_i) * T(tick) are
    numbers of T, as the scheme has them.  subset: positions in the active list to evaluate (None: all).  Returns tau_next, the active
    list, the evaluated positions `sel` in it, x1, v1, a1, j1, the new levels, `want` and h of those."""
    nxt, act, step = schedule(lev, tau, L)
    dtT = T(dt)
    tick = T(dtT * T(2.0 ** -L))
    h = (np.asarray(nxt - tau.astype(np.int64), T) * tick).astype(ft)[:, None]
    x, v, a, j = (np.asarray(q, ft) for q in (x, v, a, j))
    xp = x + h * v + h * h / ft(2) * a + h * h * h / ft(6) * j
    vp = v + h * a + h * h / ft(2) * j
    sel = np.arange(len(act)) if subset is None else np.asarray(subset)
    t = act[sel]
    a1, j1 = ref_force_jerk(m, xp, vp, c, e2, ft, targets=t, reverse=reverse)
    ha, a0, j0, v0 = h[t], a[t], j[t], v[t]
    v1 = v0 + ha / ft(2) * (a0 + a1) + ha * ha / ft(12) * (j0 - j1)
    x1 = x[t] + ha / ft(2) * (v0 + v1) + ha * ha / ft(12) * (a0 - a1)
    a3 = (ft(12) * (a0 - a1) + ft(6) * ha * (j0 + j1)) / (ha * ha * ha)
    a2 = (ft(-6) * (a0 - a1) - ha * (ft(4) * j0 + ft(2) * j1)) / (ha * ha) + ha * a3
    num = nrm(a1) * nrm(a2) + nrm(j1) ** 2
    den = nrm(j1) * nrm(a3) + nrm(a2) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(den > 0, np.sqrt(ft(eta) * num / np.where(den > 0, den, 1)), ft(np.inf))
    hh, l = ha[:, 0], lev[t].astype(np.int64)
    down = want < hh
    deeper = np.minimum(np.maximum(l + 1, level_for(want, ft(dtT), L)), L)
    up = (~down) & (want >= 2 * hh) & (l > 0) & (nxt % (2 * step[t]) == 0)
    newl = np.where(down, deeper, np.where(up, l - 1, l))
    return dict(nxt=nxt, act=act, sel=sel, x=x1, v=v1, a=a1, j=j1, lev=newl, want=want, h=hh)


def near_boundary(want, h, dt, L, tol):
    """want within a relative tol of h, 2 h or one of the steps dt 2^-l."""
    ft = want.dtype.type
    b = np.concatenate([np.stack([h, 2 * h], 1), np.broadcast_to(ft(dt) * ft(2) ** -np.arange(L + 1), (len(h), L + 1))], 1)
    return (np.abs(want[:, None] - b) <= ft(tol) * b).any(1)


def ref_block_run(T, m, x, v, dt, L, c, e2, eta, eta_start, nint, reverse=False):
    """`nint` intervals of dt with block steps, all in T (float64 or float32): x, v, block steps, body steps."""
    m, x, v = np.asarray(m, T), np.asarray(x, T).copy(), np.asarray(v, T).copy()
    a, j = ref_force_jerk(m, x, v, c, e2, T, reverse=reverse)
    lev, _ = start_levels(a, j, eta_start, T(dt), L, T)
    bsteps = bodysteps = 0
    for _ in range(nint):
        tau = np.zeros(len(m), np.int64)
        while True:
            r = ref_block_step(T, m, x, v, a, j, lev, tau, dt, L, c, e2, eta, ft=T, reverse=reverse)
            t = r["act"]
            x[t], v[t], a[t], j[t], lev[t], tau[t] = r["x"], r["v"], r["a"], r["j"], r["lev"], r["nxt"]
            bsteps += 1
            bodysteps += len(t)
            if r["nxt"] == 1 << L:
                assert len(t) == len(m)
                break
    return x, v, bsteps, bodysteps


def ref_energy(m, x, v, c, e2):
    m, x, v = np.asarray(m, np.float64), np.asarray(x, np.float64), np.asarray(v, np.float64)
    d = x[None] - x[:, None]
    inv = 1 / np.sqrt((d * d).sum(-1) + np.float64(e2))
    np.fill_diagonal(inv, 0)
    return 0.5 * (m * (v * v).sum(-1)).sum() - 0.5 * c * (m[:, None] * m[None, :] * inv).sum()


def random_system(nb, dtype, dim, n, seed, c=1.0, dt=0.01):
    rng = np.random.default_rng(seed)
    t = npt(dtype)
    hs = nb.HostSystem(dtype, dim, n)
    hs.m[:] = rng.uniform(0.5, 1.5, n).astype(t) / n
    hs.x[:] = rng.normal(0, 1, (n, dim)).astype(t)
    hs.v[:] = rng.normal(0, 0.3, (n, dim)).astype(t)
    hs.dt, hs.c = dt, c
    return hs


def binary_cluster(nb, dtype, n=512, seed=2024, eps=0.002, sep=0.004, dt=1.0 / 16):
    """The Gaussian cluster of tests/test_gpu_hermite.py (sigma_x = 1, sigma_v = 0.3, m = 1 / N, c = 1) with bodies 0 and 1 made a
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
    """x, v, a, the jerk, levels and tau as they are on the device."""
    out = dev.download()
    lev, tau = dev.hermite_block_levels()
    return out, dev.hermite_jerk(), lev, tau


# ---- 1. one block step against NumPy longdouble ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_one_block_step_against_numpy_longdouble(nb, dtype, dim):
    """N in {2, 65, 257, 4097, 65537}, eps = 0.05, dt_max = 0.5, max_level = 6, eta_start = 0.3, eta = 0.4.  Three block steps bring
    the bodies to different tau; the fourth is downloaded before and after and replayed.  tau_next and the active list must be equal; x,
    v, a and the jerk of the active bodies (of 256 of them, evenly spread over the list, where more are active) within TOL; every inactive
    body bitwise untouched; the new levels equal except where longdouble `want` is within LEVEL_EXCUSE of a decision boundary, at most
    1 % of the active bodies.
    Why steps this long: `want` takes a3 h^3 = 12 (a0 - a1) + 6 h (j0 + j1), a third difference of size (h / t)^3 |a| for a body whose
    force changes on the time scale t, from force sums that carry ~1e-6 |a| of rounding in float.  For `want` to come out the same to
    the 1e-4 the level check excuses, h / t must be ~0.5, which eta = 0.4 asks for; with eta = 0.01 (h / t ~ 0.05) a float32 NumPy
    replay already differs from the longdouble one in `want` by 1e-2 and in 8 of 98 levels.  Checked on the CPU for these seeds up to
    N = 4097: the float64 replay differs from the longdouble one in no level (`want` within 1.5e-11), the float32 replay in none
    (`want` within 4e-3 at worst; its relative error summed over the evaluated bodies of a case, which is about the number of levels
    one expects to differ without being excused, is 0.016 at most)."""
    T, eps, L, eta_start, eta = npt(dtype), 0.05, 6, 0.3, 0.4
    e2 = e2_of(dtype, eps)
    for n in (2, 65, 257, 4097, 65537):
        hs = random_system(nb, dtype, dim, n, seed=300 + n, dt=0.5)
        dev = nb.DeviceSystem.from_host(hs)
        dev.hermite_block_start(eps, eta_start, L)
        for _ in range(3):
            dev.hermite_block_step(eps, eta)
        before, j0, lev0, tau0 = snapshot(dev)
        n_act, nxt = dev.hermite_block_step(eps, eta)
        act = dev.hermite_block_active(n_act)
        after, j1, lev1, tau1 = snapshot(dev)
        dev.close()

        rn, ract, _ = schedule(lev0, tau0, L)
        assert nxt == rn and n_act == len(ract) and np.array_equal(act, ract), (n, nxt, rn, n_act, len(ract))
        subset = None if n_act <= 256 else np.unique(np.linspace(0, n_act - 1, 256).astype(np.int64))
        r = ref_block_step(T, hs.m, before.x, before.v, before.a, j0, lev0, tau0, hs.dt, L, hs.c, e2, eta, subset=subset)
        t = ract[r["sel"]]
        worst = {k: maxrel(got[t], r[k]) for k, got in (("x", after.x), ("v", after.v), ("a", after.a), ("j", j1))}
        inactive = np.ones(n, bool)
        inactive[ract] = False
        for got, old in ((after.x, before.x), (after.v, before.v), (after.a, before.a), (j1, j0), (lev1, lev0), (tau1, tau0)):
            assert np.array_equal(got[inactive], old[inactive]), n
        assert np.array_equal(tau1[ract], np.full(n_act, 0 if nxt == 1 << L else nxt, np.uint32))
        differ = lev1[t] != r["lev"]
        excused = differ & near_boundary(r["want"], r["h"], T(hs.dt), L, LEVEL_EXCUSE[dtype])
        print(f"dtype={dtype} dim={dim} n={n}: tau_next={nxt} n_act={n_act} levels {np.bincount(lev0, minlength=L + 1).tolist()} "
              + " ".join(f"{k} {w:.3g}" for k, w in worst.items()) + f" levels differ {differ.sum()} excused {excused.sum()} of {len(t)}")
        assert all(w <= TOL[dtype] for w in worst.values()), (n, worst)
        assert not (differ & ~excused).any(), (n, lev1[t][differ], r["lev"][differ], r["want"][differ], r["h"][differ])
        assert excused.sum() <= 0.01 * len(t), (n, excused.sum(), len(t))


# ---- 2. active sets of every size ----------------------------------------------------------------------------------------------------
def graded_system(nb, dtype, n=20000, seed=7, L=8, eta_start=0.1):
    """A Gaussian cluster of n bodies whose own steps are all dt = 2^-12 (level 0), and 365 near-massless satellites (10^-10 of a cluster
    body's mass) on circular orbits around 365 cluster bodies, the orbits sized so that the satellite's eta_start |a| / |j| = eta_start /
    omega is sqrt(2) x the step of its level: 1 satellite at level 8, 1 at 7, 61 at 6, 1 at 5, 1 at 4, 300 at 3.  With eta = eta_start^2 the
    criterion of the step gives the same sqrt(eta) / omega on a circular orbit, so the levels stay.  One interval of 256 ticks then has
    active sets of 1 (odd ticks), 2, 63, 64, 65, 365 and, at the end, n bodies.  The satellites sit at random body indices."""
    rng = np.random.default_rng(seed)
    dt, eps = 2.0 ** -12, 5e-6
    m = np.full(n, 1.0 / n)
    x, v = rng.normal(0, 1, (n, 3)), rng.normal(0, 0.3, (n, 3))
    counts = {8: 1, 7: 1, 6: 61, 5: 1, 4: 1, 3: 300}
    pick = rng.choice(n, 2 * sum(counts.values()), replace=False)
    sats, hosts = pick[:len(pick) // 2], pick[len(pick) // 2:]
    k = 0
    for l, cnt in counts.items():
        omega = eta_start / (np.sqrt(2.0) * dt * 2.0 ** -l)
        r2 = (m[0] / omega ** 2) ** (2.0 / 3.0) - eps * eps  # omega^2 = M / (s^2 + eps^2)^(3/2)
        assert r2 > (2 * eps) ** 2
        for _ in range(cnt):
            s, hst = sats[k], hosts[k]
            e1 = rng.normal(0, 1, 3)
            e1 /= np.linalg.norm(e1)
            e2v = np.cross(e1, rng.normal(0, 1, 3))
            e2v /= np.linalg.norm(e2v)
            m[s] = 1e-10 / n
            x[s] = x[hst] + np.sqrt(r2) * e1
            v[s] = v[hst] + omega * np.sqrt(r2) * e2v
            k += 1
    t = npt(dtype)
    hs = nb.HostSystem(dtype, 3, n)
    hs.m[:], hs.x[:], hs.v[:] = m.astype(t), x.astype(t), v.astype(t)
    hs.dt, hs.c = dt, 1.0
    return hs, eps, L, eta_start, eta_start ** 2


def test_active_sets_of_every_size(nb):
    """N = 20 000 in double, one interval of 256 block steps (graded_system): active sets of 1, 2, 63, 64, 65, 365 and 20 000 bodies must
    all occur; at the first step of each size a and the jerk of the active bodies (of 256 of them when all are active) against a
    longdouble force + jerk at the predicted state the library reports (nbody_hermite_read 1, 2), within TOL.  The launch shapes:
    79 chunks of one tile for 1 .. 365 active bodies (1, 1, 1, 1, 2 and 6 blocks), 7 chunks of 12 tiles for all 20 000 (313 blocks)."""
    hs, eps, L, eta_start, eta = graded_system(nb, 1)
    e2 = e2_of(1, eps)
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite_block_start(eps, eta_start, L)
    lev, _ = dev.hermite_block_levels()
    print("start levels", np.bincount(lev, minlength=L + 1).tolist())
    seen, sizes, nxt = {}, [], 0
    while nxt != 1 << L:
        lev0, tau0 = dev.hermite_block_levels()
        n_act, nxt = dev.hermite_block_step(eps, eta)
        sizes.append(n_act)
        rn, ract, _ = schedule(lev0, tau0, L)
        assert (nxt, n_act) == (rn, len(ract)), (nxt, rn, n_act, len(ract))
        if n_act in seen:
            continue
        act = dev.hermite_block_active(n_act)
        assert np.array_equal(act, ract)
        xp, vp = dev.hermite.read(1, dev.stream), dev.hermite.read(2, dev.stream)
        a, j = dev.download().a, dev.hermite_jerk()
        t = act if n_act <= 512 else act[np.unique(np.linspace(0, n_act - 1, 256).astype(np.int64))]
        ra, rj = ref_force_jerk(hs.m, xp, vp, hs.c, e2, targets=t)
        seen[n_act] = (maxrel(a[t], ra), maxrel(j[t], rj))
        print(f"tau_next={nxt} n_act={n_act}: a {seen[n_act][0]:.3g} jerk {seen[n_act][1]:.3g}")
        assert seen[n_act][0] <= TOL[1] and seen[n_act][1] <= TOL[1], (n_act, seen[n_act])
    dev.close()
    print("sizes of the active sets:", sorted(set(sizes)))
    assert {1, 2, 63, 64, 65, 365, hs.n} <= set(sizes), sorted(set(sizes))


# ---- 3. invariants over an advance -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [1, 0])
def test_invariants_over_advances(nb, dtype):
    """N = 1000 cluster with a binary, max_level = 8, three intervals stepped one block step at a time: tau_i stays a multiple of the
    body's step, levels stay in [0, L], tau_next strictly increases, all tau_i = 0 after each interval.  The same run through
    block_advance gives the same counts (body_steps = the sum of the n_active) and the same bits."""
    eps, L, eta = 0.01, 8, 0.02
    hs = binary_cluster(nb, dtype, n=1000, eps=eps, sep=0.02)
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite_block_start(eps, 0.01, L)
    counts = []
    for _ in range(3):
        last, bs, bod = 0, 0, 0
        while last != 1 << L:
            n_act, nxt = dev.hermite_block_step(eps, eta)
            assert nxt > last and 1 <= n_act <= hs.n
            last, bs, bod = nxt, bs + 1, bod + n_act
            lev, tau = dev.hermite_block_levels()
            assert lev.min() >= 0 and lev.max() <= L
            step = np.int64(1) << (L - lev.astype(np.int64))
            assert (tau.astype(np.int64) % step == 0).all()
            assert (tau.astype(np.int64) <= nxt % (1 << L)).all()
        assert n_act == hs.n and not tau.any()
        counts.append((bs, bod))
    stepped = dev.download()
    dev.close()
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite_block_start(eps, 0.01, L)
    advanced = [dev.hermite_block_advance(eps, eta) for _ in range(3)]
    out = dev.download()
    lev, tau = dev.hermite_block_levels()
    dev.close()
    print(f"dtype={dtype}: (block steps, body steps) per interval {counts}")
    assert advanced == counts and not tau.any()
    assert np.array_equal(out.x, stepped.x) and np.array_equal(out.v, stepped.v)
    assert counts[0][0] > 1 and counts[0][1] < counts[0][0] * hs.n  # it is a block scheme: not every body at every step


@pytest.mark.parametrize("dtype,dim,n", [(1, 3, 1000), (0, 3, 1000), (1, 2, 300), (0, 3, 65536), (1, 3, 70001)])
def test_max_level_0_is_the_fixed_step(nb, dtype, dim, n):
    """max_level = 0: one advance is one block step with every body active, and x, v, a, the jerk agree with nbody_hermite_step at the
    same dt within TOL (they came out bitwise equal on an MI355X in every case: the same arithmetic in the same launch shape)."""
    eps = 0.05
    hs = random_system(nb, dtype, dim, n, seed=n)
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite_block_start(eps, 0.01, 0)
    assert dev.hermite_block_advance(eps, 0.02) == (1, n)
    assert dev.hermite_block_step(eps, 0.02) == (n, 1)
    got, gj = dev.download(), dev.hermite_jerk()
    lev, tau = dev.hermite_block_levels()
    dev.close()
    assert not lev.any() and not tau.any()
    dev = nb.DeviceSystem.from_host(hs)
    dev.hermite_start(eps)
    dev.hermite_step(eps)
    dev.hermite_step(eps)
    ref, rj = dev.download(), dev.hermite_jerk()
    dev.close()
    worst = max(maxrel(got.x, ref.x), maxrel(got.v, ref.v), maxrel(got.a, ref.a), maxrel(gj, rj))
    print(f"dtype={dtype} dim={dim} n={n}: {worst:.3g} bitwise {np.array_equal(got.x, ref.x) and np.array_equal(got.v, ref.v)}")
    assert worst <= TOL[dtype]


# ---- 4. the point of the feature ---------------------------------------------------------------------------------------------------------
def gpu_block_run(nb, hs, eps, eta, eta_start, L, nint):
    dev = nb.DeviceSystem.from_host(hs)
    k0, p0 = dev.calc_energies(softening=eps)
    dev.hermite_block_start(eps, eta_start, L)
    bs = bod = 0
    for _ in range(nint):
        s, b = dev.hermite_block_advance(eps, eta)
        bs, bod = bs + s, bod + b
    k1, p1 = dev.calc_energies(softening=eps)
    out = dev.download()
    lev, _ = dev.hermite_block_levels()
    dev.close()
    return out, bs, bod, abs((float(k1) + float(p1) - float(k0) - float(p0)) / (float(k0) + float(p0))), lev


def test_binary_in_a_cluster(nb):
    """N = 512 double, eps = 0.002, bodies 0 and 1 a circular binary of separation 0.004 (period 0.025), to t = 0.5 with dt_max = 1/16,
    max_level = 12, eta_start = 0.01, eta = 0.02.  Against the float64 NumPy block run: block steps and body steps within 2 %, |dE / E| at
    most 4 x NumPy's, and at most 1/1000 of the GPU's fixed step with 128 steps over the same time.
    NumPy: 1115 block steps, 16 755 body steps, |dE / E| 8.3e-8 (fixed step: 2.2e-2)."""
    eps, L, eta, eta_start, nint = 0.002, 12, 0.02, 0.01, 8
    hs = binary_cluster(nb, 1)
    e2 = e2_of(1, eps)
    e0 = ref_energy(hs.m, hs.x, hs.v, hs.c, e2)
    x, v, nbs, nbod = ref_block_run(np.float64, hs.m, hs.x, hs.v, hs.dt, L, hs.c, e2, eta, eta_start, nint)
    de_np = abs((ref_energy(hs.m, x, v, hs.c, e2) - e0) / e0)
    out, bs, bod, de_gpu, lev = gpu_block_run(nb, hs, eps, eta, eta_start, L, nint)
    # the fixed step: 128 steps of dt_max / 16
    fx = binary_cluster(nb, 1, dt=hs.dt / 16)
    dev = nb.DeviceSystem.from_host(fx)
    k0, p0 = dev.calc_energies(softening=eps)
    dev.hermite_start(eps)
    for _ in range(128):
        dev.hermite_step(eps)
    k1, p1 = dev.calc_energies(softening=eps)
    dev.close()
    de_fixed = abs((k1 + p1 - k0 - p0) / (k0 + p0))
    print(f"numpy: {nbs} block steps, {nbod} body steps ({nbod / hs.n:.1f} N), dE/E {de_np:.3g}")
    print(f"gpu:   {bs} block steps, {bod} body steps ({bod / hs.n:.1f} N), dE/E {de_gpu:.3g}; final levels {np.bincount(lev).tolist()}")
    print(f"gpu fixed step, 128 steps: dE/E {de_fixed:.3g} ({de_fixed / de_gpu:.3g} x the block steps')")
    print(f"final x against numpy: {maxrel(out.x, x):.3g}")
    assert abs(bs - nbs) <= 0.02 * nbs and abs(bod - nbod) <= 0.02 * nbod, (bs, nbs, bod, nbod)
    assert de_gpu <= 4 * de_np, (de_gpu, de_np)
    assert de_gpu <= de_fixed / 1000, (de_gpu, de_fixed)


# ---- 5. repeatability ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", [(1, 512), (0, 512), (1, 5000)])
def test_bitwise_repeatable(nb, dtype, n):
    """Two runs of 4 advances from the same upload give the same x, v, levels bit for bit; so does a run whose handle is destroyed after
    two advances and made again (block_start then restarts the levels from the state on the device, in both runs alike)."""
    eps, L, eta = 0.01, 10, 0.02
    hs = binary_cluster(nb, dtype, n=n, eps=eps, sep=0.02)

    def run(remake):
        dev = nb.DeviceSystem.from_host(hs)
        dev.hermite_block_start(eps, 0.01, L)
        counts = [dev.hermite_block_advance(eps, eta) for _ in range(2)]
        if remake:
            dev._hermite.close()
            dev._hermite = None
        dev.hermite_block_start(eps, 0.01, L)
        counts += [dev.hermite_block_advance(eps, eta) for _ in range(2)]
        out, lev = dev.download(), dev.hermite_block_levels()[0]
        dev.close()
        return out, lev, counts

    a, b, c = run(False), run(False), run(True)
    print(f"dtype={dtype} n={n}: {a[2]}")
    for other in (b, c):
        assert other[2] == a[2]
        assert np.array_equal(other[0].x, a[0].x) and np.array_equal(other[0].v, a[0].v) and np.array_equal(other[1], a[1])


# ---- 6. float ----------------------------------------------------------------------------------------------------------------------------
def test_binary_in_a_cluster_float(nb):
    """The case of test_binary_in_a_cluster in float with eps = 0.01, separation 0.02.  Block and body steps within 5 % of the float64 NumPy
    run's (334 / 14 496).  |dE / E| is rounding-dominated: its bound is 4 x the largest |dE / E| of float32 NumPy block runs with forward
    and reversed summation over the seeds 2024, 2025, 2026 (computed here, printed).  The positions at the end against the float64 GPU
    run from the same (float-rounded) start, judged as tests/test_gpu_hermite.py judges its float trajectory: the yardstick is the
    larger distance (max|dx| / max|x|) of the forward and the reversed float32 NumPy run from that float64 run, the margin 4 x."""
    eps, sep, L, eta, eta_start, nint = 0.01, 0.02, 12, 0.02, 0.01, 8
    e2 = e2_of(0, eps)
    hs = binary_cluster(nb, 0, eps=eps, sep=sep)
    m64, x64, v64 = (np.asarray(q, np.float64) for q in (hs.m, hs.x, hs.v))  # the same start, exactly
    _, _, nbs, nbod = ref_block_run(np.float64, m64, x64, v64, hs.dt, L, hs.c, e2, eta, eta_start, nint)
    bound, runs32 = 0.0, {}
    for seed in (2024, 2025, 2026):
        s = binary_cluster(nb, 0, seed=seed, eps=eps, sep=sep)
        e0 = ref_energy(s.m, s.x, s.v, s.c, e2)
        for rev in (False, True):
            x, v, b1, b2 = ref_block_run(np.float32, s.m, s.x, s.v, s.dt, L, s.c, e2, eta, eta_start, nint, reverse=rev)
            de = abs((ref_energy(s.m, x, v, s.c, e2) - e0) / e0)
            print(f"numpy float32 seed {seed} reversed {rev}: {b1} block steps, {b2} body steps, dE/E {de:.3g}")
            bound = max(bound, de)
            if seed == 2024:
                runs32[rev] = x
    out, bs, bod, _, _ = gpu_block_run(nb, hs, eps, eta, eta_start, L, nint)
    e0 = ref_energy(hs.m, hs.x, hs.v, hs.c, e2)
    de_gpu = abs((ref_energy(hs.m, out.x, out.v, hs.c, e2) - e0) / e0)  # in float64 from the downloaded state, as NumPy's is
    h64 = nb.HostSystem(1, 3, hs.n)
    h64.m[:], h64.x[:], h64.v[:], h64.dt, h64.c = m64, x64, v64, hs.dt, hs.c
    out64, bs64, bod64, _, _ = gpu_block_run(nb, h64, eps, eta, eta_start, L, nint)
    yard = max(maxrel(runs32[False], out64.x), maxrel(runs32[True], out64.x))
    dist = maxrel(out.x, out64.x)
    print(f"numpy float64: {nbs} block steps, {nbod} body steps; gpu float64: {bs64} / {bod64}")
    print(f"gpu float: {bs} block steps, {bod} body steps, dE/E {de_gpu:.3g} (bound 4 x {bound:.3g})")
    print(f"trajectory: yardstick {yard:.3g} gpu {dist:.3g} multiple {dist / yard:.2f}")
    assert abs(bs - nbs) <= 0.05 * nbs and abs(bod - nbod) <= 0.05 * nbod, (bs, nbs, bod, nbod)
    assert de_gpu <= 4 * bound, (de_gpu, bound)
    assert dist <= 4 * yard, (dist, yard)


# ---- 7. CLI ------------------------------------------------------------------------------------------------------------------------------
def read_energies(path):
    raw = open(path, "rb").read()
    steps, tsz = struct.unpack("<2I", raw[:8])
    return np.frombuffer(raw[8:], dtype=np.float32 if tsz == 4 else np.float64).reshape(-1, 2)


def test_cli_block_steps_hold_the_energy(nb):
    """--integrator hermite --hermite-eta 0.02 --softening 0.002 -n 512 -s 8 --workload load FILE --save energy runs; with --csv-detailed
    (which saves a frame per step, not only the first) the saved energies drift less than those of the same command without --hermite-eta."""
    hs = binary_cluster(nb, 0)
    exe = os.path.join(ROOT, "stdpar-nbody_amd", "bin", "nbody_hip_d3")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "binary.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<IIff", hs.n, 3, hs.dt, hs.c))
            f.write(np.concatenate([hs.m[:, None], hs.x, hs.v], 1).astype(np.float32).tobytes())
        base = ["--algorithm", "all-pairs", "--integrator", "hermite", "--softening", "0.002", "-n", "512", "-s", "8", "--workload", "load", path,
                "--save", "energy"]
        block = ["--hermite-eta", "0.02"]
        r = subprocess.run([exe] + base + block, cwd=d, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "Done simulation" in r.stdout, (r.stdout, r.stderr)
        assert read_energies(os.path.join(d, "energy.bin")).shape == (1, 2)
        drift = {}
        for name, extra in (("block", block), ("block L=14", block + ["--hermite-levels", "14"]), ("fixed", [])):
            r = subprocess.run([exe] + base + extra + ["--csv-detailed"], cwd=d, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, (name, r.stderr)
            en = read_energies(os.path.join(d, "energy.bin")).astype(np.float64).sum(1)
            assert en.shape == (9,) and np.isfinite(en).all(), (name, en)
            drift[name] = np.abs((en - en[0]) / en[0]).max()
    print("max |dE / E| over the 8 saved steps:", {k: f"{v:.3g}" for k, v in drift.items()})
    assert drift["block"] < drift["fixed"] and drift["block L=14"] < drift["fixed"]


# ---- 8. call sequence ----------------------------------------------------------------------------------------------------------------
def test_call_sequence_and_capture(nb):
    """block_step / block_advance / block_read before block_start, and after a later nbody_hermite_force_jerk: NBODY_ERR_STATE.  Under
    capture block_start and block_step (and advance, read) return NBODY_ERR_STATE and leave the capture usable: it goes on to record a
    fixed step that replays."""
    L = nb.lib()
    hs = random_system(nb, 1, 3, 300, seed=1)
    dev = nb.DeviceSystem.from_host(hs)
    st, stream = dev.state(), ctypes.c_void_p(dev.stream)
    h = nb.Hermite(1, 3, 300, dev.device)
    na, tau = ctypes.c_uint32(), ctypes.c_uint32()
    bs, bod = ctypes.c_uint64(), ctypes.c_uint64()
    buf = np.zeros(300, np.int32)
    step = lambda: L.nbody_hermite_block_step(h.h, ctypes.byref(st), 0.05, 0.02, stream, ctypes.byref(na), ctypes.byref(tau))
    advance = lambda: L.nbody_hermite_block_advance(h.h, ctypes.byref(st), 0.05, 0.02, stream, ctypes.byref(bs), ctypes.byref(bod))
    start = lambda: L.nbody_hermite_block_start(h.h, ctypes.byref(st), 0.05, 0.01, 6, stream)
    read = lambda: L.nbody_hermite_block_read(h.h, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, stream)
    assert (step(), advance(), read()) == (3, 3, 3)
    h.force_jerk(st, 0.05, dev.stream)
    assert (step(), advance(), read()) == (3, 3, 3)  # force_jerk starts a fixed-step run, not a block run
    other = nb.Hermite(1, 3, 301, dev.device)
    assert L.nbody_hermite_block_start(other.h, ctypes.byref(st), 0.05, 0.01, 6, stream) == 1
    other.close()
    assert start() == 0 and step() == 0 and na.value >= 1 and read() == 0
    assert L.nbody_hermite_block_read(h.h, 0, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes - 4, stream) == 1
    assert L.nbody_hermite_block_read(h.h, 3, buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes, stream) == 1
    st2 = dev.state()
    st2.dt = st.dt / 2  # another dt than block_start's
    assert L.nbody_hermite_block_step(h.h, ctypes.byref(st2), 0.05, 0.02, stream, None, None) == 1
    assert advance() == 0 and bs.value >= 1  # completes the interval: synchronous again, a fixed step may follow
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
