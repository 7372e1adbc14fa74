"""GPU: the direct-sum Hermite family (orders 4 and 6, fixed and block steps) against the wide per-body reference of
tests/hermite_wide_model.py.  What the older Hermite files cannot see and this one can: an error of a few ulps in the pair arithmetic,
an error confined to bodies whose force is far below the largest, the snap of a typical body, a factor c applied once too often or not
at all (c = 0.37 throughout), and the two ends of the range of q.

Every bound is P_g, the pair term's rounding error as csrc/hermite_tile.hpp derives it (2.5 / 5 / 7 eps in double, 4.5 / 8.5 / 12 in
float for a / jerk / snap), plus 1.5 for an isolated pair or plus the chain length L of the launch plan for a summed body, in units of
eps_T times the body's own magnitude scale S_g,i; none comes from what the kernels gave.  The measured worst values stand in each test's
docstring and in profiles/tests_hermite_wide/figures.txt."""
import numpy as np
import pytest

import hermite_wide_model as W
from hermite_wide_model import LD, P

pytestmark = pytest.mark.gpu

DTYPE = {np.float64: 1, np.float32: 0}
ORDER_CHUNKS = {4: 1, 6: 2}  # min_chunks of hermite_plan_for
NAMES = ("a", "jerk", "snap")


def host(nb, T, m, x, v, dt=0.0, c=W.C):
    hs = nb.HostSystem(DTYPE[T], x.shape[1], len(m))
    hs.m[:], hs.x[:], hs.v[:] = m, x, v
    hs.dt, hs.c = dt, c
    return hs


def start(dev, order, eps):
    dev.hermite_start(eps) if order == 4 else dev.hermite6_start(eps)


def state(dev, order):
    """(x, v, a, jerk) or (x, v, a, jerk, snap, crackle) as they are on the device."""
    out = dev.download()
    rest = (dev.hermite_jerk(),) if order == 4 else tuple(dev.hermite6_read(w) for w in range(3))
    return (out.x.copy(), out.v.copy(), out.a.copy()) + rest


def predicted(dev, order):
    """The state the last call evaluated, as the library reports it: (xp, vp) or (xp, vp, ap)."""
    return tuple(dev.hermite.read(w, dev.stream) for w in (1, 2)) if order == 4 else tuple(dev.hermite6_read(w) for w in (3, 4, 5))


def sums_of(S, order):
    return S[2:4] if order == 4 else S[2:5]


def worst_units(T, got, m, pred, c, e2, targets=None):
    """Worst E_g over `targets` of the sums `got` (arrays over all bodies) against the wide reference at the state `pred` = (x, v) or
    (x, v, acc); also the references and the largest magnitude among references and scales."""
    t = np.arange(len(m)) if targets is None else np.asarray(targets)
    refs, scales = W.wide(m, pred[0], pred[1], pred[2] if len(pred) == 3 else None, c, e2, t)
    worst = [float(W.err_units(g[t], r, S, T).max()) for g, r, S in zip(got, refs, scales)]
    big = max(float(np.abs(z).max()) for z in refs[:len(got)] + scales[:len(got)])
    return worst, refs, big


def fmt(worst, bounds):
    return " ".join(f"{k} {w:.3g} (<= {b:g})" for k, w, b in zip(NAMES, worst, bounds))


# ---- (a) isolated pairs: the pair arithmetic in ulps ---------------------------------------------------------------------------------
@pytest.mark.parametrize("T,eps", [(np.float64, 0.05), (np.float64, 1e-9), (np.float32, 0.05), (np.float32, 1e-4)])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("order", [4, 6])
def test_isolated_pairs_in_ulps(nb, order, dim, T, eps):
    """64 two-body systems per case (W.isolated_pairs: separations over eps [2^-10, 2^20], relative speeds over four decades, mass
    ratios over twelve, c = 0.37), uploaded one after the other into one DeviceSystem and started again.  At n = 2 a body's sum is one
    rounded term, exact zeros and the scaling by c, so E_g is the pair term's error in units of eps_T: bound P_g + 1.5, that is
    4 / 6.5 / 8.5 in double and 6 / 10 / 13.5 in float.
    Measured on an MI355X (worst over the cases): a 1.88, jerk 1.75, snap 1.59 in double; a 3.12, jerk 2.44, snap 3.15 in float."""
    m, x, v = W.isolated_pairs(T, dim, 64, eps, seed=order)
    e2 = W.e2_of(T, eps)
    bounds = [p + W.PAIR_EXTRA for p in P[T]][:order // 2]
    dev = nb.DeviceSystem(DTYPE[T], dim, 2)
    worst = np.zeros(len(bounds))
    for p in range(len(m)):
        dev.upload(host(nb, T, m[p], x[p], v[p]))
        start(dev, order, eps)
        got = sums_of(state(dev, order), order)
        assert all(np.isfinite(g).all() for g in got)
        worst = np.maximum(worst, worst_units(T, got, m[p], (x[p], v[p]) + ((got[0],) if order == 6 else ()), W.C, e2)[0])
    dev.close()
    print(f"pairs order={order} {T.__name__} dim={dim} eps={eps}: " + fmt(worst, bounds))
    assert all(w <= b for w, b in zip(worst, bounds)), (worst, bounds)


# ---- (b) adversarial systems, per body ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65, 257, 1000, 5889, 65537])
@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("order", [4, 6])
def test_adversarial_start_per_body(nb, order, dim, T, n):
    """W.adversarial (clusters over six decades of radius, masses over twelve, coincident pairs, a far body, zero masses; c = 0.37,
    eps = 1e-4 in double, 1e-2 in float) after the start of either order: every evaluated body (all below 4097, W.targets_for above)
    within E_g,i <= P_g + L, L the chain length of hermite_plan_for(n, min_chunks): 68 (n = 65), 69 (257), 71 (1000), 143 (5889),
    4167 (65537: four chunks of 65 tiles).  Everything finite, the references and scales below
    W.adv_limit, and with all velocities zero a jerk of exactly zero.
    Measured on an MI355X (worst over the cases): up to 5889 bodies a 3.22, jerk 3.36, snap 2.05 in double and a 4.29, jerk 2.15,
    snap 2.62 in float; at 65537 (two targets per lane, L = 4167) a 13.8, jerk 7.84, snap 2.89 and a 17.2, jerk 5.84, snap 0.61."""
    m, x, v, planted = W.adversarial(T, dim, n)
    eps = W.ADV_EPS[T]
    e2 = W.e2_of(T, eps)
    L = W.chain_length(W.plan_for(n, ORDER_CHUNKS[order]))
    bounds = [p + L for p in P[T]][:order // 2]
    dev = nb.DeviceSystem.from_host(host(nb, T, m, x, v))
    start(dev, order, eps)
    got = sums_of(state(dev, order), order)
    dev.upload(host(nb, T, m, x, np.zeros_like(v)))
    start(dev, order, eps)
    still = sums_of(state(dev, order), order)
    dev.close()
    assert all(np.isfinite(g).all() for g in got + still)
    assert not still[1].any()
    worst, _, big = worst_units(T, got, m, (x, v) + ((got[0],) if order == 6 else ()), W.C, e2, W.targets_for(n, planted))
    print(f"adversarial order={order} {T.__name__} dim={dim} n={n} L={L}: " + fmt(worst, bounds) + f"; largest |ref| or scale {big:.3g}")
    assert big < W.adv_limit(T, n)
    assert all(w <= b for w, b in zip(worst, bounds)), (worst, bounds)


# ---- (c) the edge of the softening range ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,eps", [(np.float64, 2.0 ** -340), (np.float32, 2.0 ** -42)])
@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("order", [4, 6])
def test_smallest_softening(nb, order, dim, T, eps):
    """eps^2 = 2^-680 in double, 2^-84 in float: the smallest check_softening accepts, where q^(-3/2) of a coincident pair is 2^1020
    (2^126).  n = 300 on a jittered lattice (mutual distances >= 1.2), five coincident pairs of equal velocity (and, from the start's
    first pass, bitwise equal acceleration), c = 0.37.  Everything finite; the two bodies of a pair get the same bits in every sum; the
    first body of each pair gets, in a and the jerk, the bits it gets when its partner has mass 0 and sits far away (the partner adds
    an exact zero either way; the snap sees the other bodies' accelerations, which do feel the partner's mass); and every body is
    within P_g + L (L = 69) of the wide reference.
    Measured on an MI355X (worst over the cases): a 1.24, jerk 1.10, snap 0.87 in double; a 0.98, jerk 1.08, snap 0.98 in float."""
    n, npairs = 300, 5
    m, x, v = W.lattice_system(T, dim, n, seed=3)
    first, second = np.arange(10, 10 + npairs) * 7, np.arange(10, 10 + npairs) * 7 + 150
    x[second], v[second] = x[first], v[first]
    e2 = W.e2_of(T, eps)
    assert e2 == T(2.0) ** (-680 if T is np.float64 else -84)
    L = W.chain_length(W.plan_for(n, ORDER_CHUNKS[order]))
    bounds = [p + L for p in P[T]][:order // 2]
    dev = nb.DeviceSystem.from_host(host(nb, T, m, x, v))
    start(dev, order, eps)
    got = sums_of(state(dev, order), order)
    assert all(np.isfinite(g).all() for g in got)
    for g in got:
        assert np.array_equal(g[first], g[second])
    for p, q in zip(first, second):  # one pair at a time: the other partners keep pulling on this pair's first body
        m2, x2 = m.copy(), x.copy()
        m2[q] = 0
        x2[q] = 0
        x2[q, 0] = -100
        dev.upload(host(nb, T, m2, x2, v))
        start(dev, order, eps)
        apart = sums_of(state(dev, order), order)
        assert all(np.isfinite(g).all() for g in apart)
        for g, h in zip(got[:2], apart[:2]):
            assert np.array_equal(g[p], h[p]), (p, g[p], h[p])
    dev.close()
    worst, _, _ = worst_units(T, got, m, (x, v) + ((got[0],) if order == 6 else ()), W.C, e2)
    print(f"smallest eps order={order} {T.__name__} dim={dim}: " + fmt(worst, bounds))
    assert all(w <= b for w, b in zip(worst, bounds)), (worst, bounds)


# ---- (d) c != 1 through the integrators --------------------------------------------------------------------------------------------------
STEP_DT = {np.float64: 2.0 ** -15, np.float32: 2.0 ** -9}  # a few per cent of the bodies have eta_start |a| / |j| below dt / 8
PREDICT_UNITS = 8    # Horner in h with one FMA per level: per level the rounding of h * constant, of the constant and of the FMA, <= 3 x
#                      0.5 eps of the magnitude sum, five levels at order 6: 7.5 eps
CORRECT_UNITS = 8    # v1 = v0 + fma(h/2, a0 + a1, fma(h2/10, j0 - j1, h3/120 (s0 + s1))): a term carries the rounding of its sum, of its
#                      factor (h h, h2 h, the constant: 1.5 eps) and of its product, 2.5 eps of its magnitude at most, and the three
#                      additions 1.5 eps of the magnitude sum M_v: 4 eps; x1 takes the same again with v1's error inside h/2 (v0 + v1)
CRACKLE_UNITS = 5    # k1 = fma(h2, 9 s1 - 3 s0, fma(-h, 24 j0 + 36 j1, 60 (a1 - a0))) * ih3: each term <= 3 roundings, two FMAs, the
#                      product and the three roundings of ih3 = 1 / (dt dt dt): 9 x 0.5 eps of the magnitude sum


def check_predictor(T, order, S0, h, pred, who):
    """The library's predicted state against the longdouble Taylor sum of the downloaded state: per component within PREDICT_UNITS eps_T
    of the sum of the terms' magnitudes."""
    ref = W.predict(S0, h)
    A = [np.abs(np.asarray(z, LD)) for z in S0]
    h = np.asarray(h, LD)
    facts = [LD(1), h, h ** 2 / 2, h ** 3 / 6, h ** 4 / 24, h ** 5 / 120]
    worst = []
    for k, (g, r) in enumerate(zip(pred, ref)):
        scale = sum(f * z for f, z in zip(facts, A[k:]))
        worst.append(float((np.abs(np.asarray(g, LD) - r) / (W.eps_of(T) * scale))[scale > 0].max()))
    print(f"{who}: predictor " + " ".join(f"{w:.3g}" for w in worst) + f" (<= {PREDICT_UNITS})")
    assert max(worst) <= PREDICT_UNITS, (who, worst)


def check_corrector(T, order, S0, S1, refs, h, t, who):
    """x and v of the bodies t against the longdouble corrector fed the wide a, jerk (and snap) at the library's predicted state, within
    the global TOL of the older tests, and per component within CORRECT_UNITS eps_T of the magnitude sum of the corrector's terms against
    the same formula fed the library's own new a, jerk (and snap); at order 6 the crackle against the longdouble formula from the library's own a, jerk and snap
    before and after, per component within CRACKLE_UNITS eps_T of the magnitude sum of its terms."""
    ht = np.asarray(h, LD) if np.ndim(h) == 0 else np.asarray(h, LD)[t]
    old = [np.asarray(z, LD)[t] for z in S0]
    x, v, a0, j0 = old[:4]
    a1, j1 = refs[:2]
    if order == 4:
        v1 = v + ht / 2 * (a0 + a1) + ht * ht / 12 * (j0 - j1)
        x1 = x + ht / 2 * (v + v1) + ht * ht / 12 * (a0 - a1)
    else:
        s0, s1 = old[4], refs[2]
        v1 = v + ht / 2 * (a0 + a1) + ht ** 2 / 10 * (j0 - j1) + ht ** 3 / 120 * (s0 + s1)
        x1 = x + ht / 2 * (v + v1) + ht ** 2 / 10 * (a0 - a1) + ht ** 3 / 120 * (j0 + j1)
    ex, ev = W.maxrel(S1[0][t], x1), W.maxrel(S1[1][t], v1)
    line = f"{who}: x {ex:.3g} v {ev:.3g} (<= {W.TOL[T]:g})"
    assert ex <= W.TOL[T] and ev <= W.TOL[T], (who, ex, ev)
    # the corrector's own arithmetic, per component: the longdouble formula fed the LIBRARY's new a, jerk (and snap)
    new = [np.asarray(z, LD)[t] for z in S1]
    la, lj = new[2], new[3]
    ab = np.abs
    if order == 4:
        lv = v + ht / 2 * (a0 + la) + ht * ht / 12 * (j0 - lj)
        lx = x + ht / 2 * (v + lv) + ht * ht / 12 * (a0 - la)
        mv = ab(v) + ht / 2 * (ab(a0) + ab(la)) + ht * ht / 12 * (ab(j0) + ab(lj))
        mx = ab(x) + ht / 2 * (ab(v) + mv) + ht * ht / 12 * (ab(a0) + ab(la))
    else:
        ls = new[4]
        lv = v + ht / 2 * (a0 + la) + ht ** 2 / 10 * (j0 - lj) + ht ** 3 / 120 * (s0 + ls)
        lx = x + ht / 2 * (v + lv) + ht ** 2 / 10 * (a0 - la) + ht ** 3 / 120 * (j0 + lj)
        mv = ab(v) + ht / 2 * (ab(a0) + ab(la)) + ht ** 2 / 10 * (ab(j0) + ab(lj)) + ht ** 3 / 120 * (ab(s0) + ab(ls))
        mx = ab(x) + ht / 2 * (ab(v) + mv) + ht ** 2 / 10 * (ab(a0) + ab(la)) + ht ** 3 / 120 * (ab(j0) + ab(lj))
    ux = float((ab(new[0] - lx) / (W.eps_of(T) * mx))[mx > 0].max())
    uv = float((ab(new[1] - lv) / (W.eps_of(T) * mv))[mv > 0].max())
    line += f"; per component x {ux:.3g} v {uv:.3g} (<= {CORRECT_UNITS})"
    assert ux <= CORRECT_UNITS and uv <= CORRECT_UNITS, (who, ux, uv)
    if order == 6:
        la, lj, ls = (np.asarray(z, LD)[t] for z in S1[2:5])
        k1 = (60 * (la - a0) - ht * (24 * j0 + 36 * lj) + ht ** 2 * (9 * ls - 3 * s0)) / ht ** 3
        scale = (60 * (np.abs(la) + np.abs(a0)) + ht * (24 * np.abs(j0) + 36 * np.abs(lj)) + ht ** 2 * (9 * np.abs(ls) + 3 * np.abs(s0))) / ht ** 3
        ek = float((np.abs(np.asarray(S1[5], LD)[t] - k1) / (W.eps_of(T) * scale))[scale > 0].max())
        line += f" crackle {ek:.3g} (<= {CRACKLE_UNITS})"
        assert ek <= CRACKLE_UNITS, (who, ek)
    print(line)


@pytest.mark.parametrize("T", [np.float64, np.float32])
@pytest.mark.parametrize("order", [4, 6])
def test_fixed_steps_with_c(nb, order, T):
    """The adversarial system at n = 1000 (3D, c = 0.37): one fixed step of order 4, two of order 6 (the second predictor carries the
    crackle).  Each step from the state downloaded before it: the predicted state the library reports against the longdouble predictor;
    a, jerk and snap of every body against the wide reference at that predicted state within P_g + L (L = 71); x, v (and the crackle)
    against the longdouble corrector.
    Measured on an MI355X: a 2.94, jerk 2.19, snap 1.04 in double and a 2.54, jerk 2.37, snap 1.73 in float; predictor 1.68, corrector 2.29 per
    component, crackle 1.28; x and v within 1.3e-16 (double) and 1.0e-7 (float) in the global norm."""
    n, dim = 1000, 3
    m, x, v, _ = W.adversarial(T, dim, n)
    eps, dt = W.ADV_EPS[T], STEP_DT[T]
    e2 = W.e2_of(T, eps)
    L = W.chain_length(W.plan_for(n, ORDER_CHUNKS[order]))
    bounds = [p + L for p in P[T]][:order // 2]
    dev = nb.DeviceSystem.from_host(host(nb, T, m, x, v, dt=dt))
    start(dev, order, eps)
    for step in range(1, order // 2):
        who = f"fixed order={order} {T.__name__} step {step}"
        S0 = state(dev, order)
        assert (step == 1) == (order == 4 or not S0[5].any())
        dev.hermite_step(eps) if order == 4 else dev.hermite6_step(eps)
        S1, pred = state(dev, order), predicted(dev, order)
        assert all(np.isfinite(z).all() for z in S1 + pred)
        check_predictor(T, order, S0, LD(T(dt)), pred, who)
        worst, refs, _ = worst_units(T, sums_of(S1, order), m, pred, W.C, e2)
        print(f"{who}: " + fmt(worst, bounds))
        assert all(w <= b for w, b in zip(worst, bounds)), (who, worst, bounds)
        check_corrector(T, order, S0, S1, refs, LD(T(dt)), np.arange(n), who)
    dev.close()


@pytest.mark.parametrize("order,T", [(4, np.float64), (4, np.float32), (6, np.float64)])
def test_block_interval_with_c(nb, order, T):
    """The same system through the block steps (order 6 has them in double only): a start with max_level = 4, eta_start = 0.3, then one
    whole interval.  Every step: tau_next and the number of active bodies are the schedule's.  The first step (a few bodies, all at
    level 4) and the step that closes the interval (all bodies): the active list is the schedule's; every inactive body is bitwise
    untouched in every array, level and tau; the predicted state of ALL bodies against the longdouble predictor with h_i = tau_next -
    tau_i; a, jerk and snap of the active bodies against the wide reference at that predicted state within P_g + L (L = 71: four chunks
    of one tile for any number of active bodies at n = 1000); x, v (and the crackle) against the longdouble corrector.
    Measured on an MI355X: active sets of 33 (26 in float), 51, 86 (91), 149 (170) and 1000 bodies; a 3.04, jerk 2.21, snap 1.03 in double, a 2.00,
    jerk 1.94 in float; predictor 1.53, corrector 2.27 per component, crackle 1.36; x and v within 2.6e-16 and 6.5e-8 in the global norm."""
    n, dim, LEV, eta = 1000, 3, 4, {4: 0.02, 6: 0.3}[order]
    m, x, v, _ = W.adversarial(T, dim, n)
    eps, dt = W.ADV_EPS[T], STEP_DT[T]
    e2 = W.e2_of(T, eps)
    dev = nb.DeviceSystem.from_host(host(nb, T, m, x, v, dt=dt))
    if order == 4:
        bstart, bstep, levels, active = dev.hermite_block_start, dev.hermite_block_step, dev.hermite_block_levels, dev.hermite_block_active
    else:
        bstart, bstep, levels, active = dev.hermite6_block_start, dev.hermite6_block_step, dev.hermite6_block_levels, dev.hermite6_block_active
    bstart(eps, 0.3, LEV)
    sizes = []
    while True:
        S0, (lev0, tau0) = state(dev, order), levels()
        n_act, nxt = bstep(eps, eta)
        rn, ract, _ = W.schedule(lev0, tau0, LEV)
        assert (nxt, n_act) == (rn, len(ract)), (nxt, rn, n_act, len(ract))
        sizes.append(n_act)
        closing = nxt == 1 << LEV
        if len(sizes) == 1 or closing:
            who = f"block order={order} {T.__name__} tau_next={nxt} n_act={n_act}"
            assert np.array_equal(active(n_act), ract)
            S1, (lev1, tau1), pred = state(dev, order), levels(), predicted(dev, order)
            assert all(np.isfinite(z).all() for z in S1 + pred)
            idle = np.ones(n, bool)
            idle[ract] = False
            for new, old in zip(S1 + (lev1, tau1), S0 + (lev0, tau0)):
                assert np.array_equal(new[idle], old[idle]), who
            assert np.array_equal(tau1[ract], np.full(n_act, 0 if closing else nxt, np.uint32))
            h = W.block_h(T, dt, LEV, nxt, tau0)
            check_predictor(T, order, S0, h, pred, who)
            L = W.chain_length(W.block_plan_for(n, n_act, ORDER_CHUNKS[order]))
            bounds = [p + L for p in P[T]][:order // 2]
            worst, refs, _ = worst_units(T, sums_of(S1, order), m, pred, W.C, e2, ract)
            print(f"{who} L={L}: " + fmt(worst, bounds))
            assert all(w <= b for w, b in zip(worst, bounds)), (who, worst, bounds)
            check_corrector(T, order, S0, S1, refs, h, ract, who)
        if closing:
            break
    dev.close()
    print(f"block order={order} {T.__name__}: active set sizes {sizes}")
    assert 1 <= sizes[0] <= n // 4 and sizes[-1] == n and len(sizes) > 1, sizes
