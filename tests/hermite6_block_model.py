"""A NumPy restatement of the sixth-order Hermite block time steps (nbody_hermite6_block_* of include/nbody_hip.h) in a chosen float
type, and the systems its tests share.  Not a test: tests/test_hermite6_block.py (CPU) and tests/test_gpu_hermite6_block.py import it.
It follows the shapes of tests/test_gpu_hermite_block.py: np.longdouble for single block steps and single evaluations, float64 for
runs.  `T` is the type the scheme's own numbers (dt, the tick, h_i) are made in, `ft` the type the arithmetic is done in."""
import numpy as np

LD = np.longdouble
TOL = {1: 1e-12}  # tests/test_gpu_hermite.py's bound for a summed force (and its derivatives) against NumPy longdouble, double


def maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def nrm(a):
    return np.sqrt((a * a).sum(-1))


def ref_force_jerk_snap(m, x, v, a, c, e2, dt=LD, targets=None):
    """a_i = c sum_j w d, j_i = c sum_j w (u - 3 alpha d), s_i = c sum_j w (b - 6 alpha u + (15 alpha^2 - 3 gamma) d) with d = x_j - x_i,
    u = v_j - v_i, b = a_j - a_i, q = |d|^2 + e2, w = m_j q^(-3/2), alpha = d.u / q, gamma = (|u|^2 + d.b) / q, in `dt`, for the targets
    only, a batch of targets at a time."""
    m, x, v, a = (np.asarray(q, dt) for q in (m, x, v, a))
    idx = np.arange(len(m)) if targets is None else np.asarray(targets)
    out = [np.zeros((len(idx), x.shape[1]), dt) for _ in range(3)]
    step = max(1, min(256, (1 << 21) // len(m)))
    for s in range(0, len(idx), step):
        t = idx[s:s + step]
        d = x[None, :, :] - x[t][:, None, :]
        u = v[None, :, :] - v[t][:, None, :]
        b = a[None, :, :] - a[t][:, None, :]
        q = (d * d).sum(-1) + dt(e2)
        w = m[None, :] / (q * np.sqrt(q))
        al = ((d * u).sum(-1) / q)[:, :, None]
        ga = (((u * u).sum(-1) + (d * b).sum(-1)) / q)[:, :, None]
        w = w[:, :, None]
        out[0][s:s + step] = (w * d).sum(1)
        out[1][s:s + step] = (w * (u - dt(3) * al * d)).sum(1)
        out[2][s:s + step] = (w * (b - dt(6) * al * u + (dt(15) * al * al - dt(3) * ga) * d)).sum(1)
    return tuple(dt(c) * o for o in out)


def level_for(want, dtmax, L):
    """The smallest level l with dtmax 2^-l <= want, clamped to [0, L] (the steps are exact scalings of dtmax)."""
    steps = dtmax * (want.dtype.type(2) ** -np.arange(L + 1))
    return np.minimum((steps[None, :] > np.asarray(want)[:, None]).sum(1), L).astype(np.int64)


def start_levels(a, j, eta_start, dtmax, L, ft):
    an, jn = nrm(np.asarray(a, ft)), nrm(np.asarray(j, ft))
    want = np.where(jn > 0, ft(eta_start) * an / np.where(jn > 0, jn, 1), ft(np.inf))
    return level_for(want, ft(dtmax), L), want


def ref_start(m, x, v, c, e2, eta_start, dt, L, ft):
    """nbody_hermite6_block_start: two evaluations (the first with a = 0 keeps a alone), crackle = 0, the first levels."""
    x, v = np.asarray(x, ft).copy(), np.asarray(v, ft).copy()
    a, _, _ = ref_force_jerk_snap(m, x, v, np.zeros_like(x), c, e2, ft)
    a, j, s = ref_force_jerk_snap(m, x, v, a, c, e2, ft)
    lev, _ = start_levels(a, j, eta_start, ft(dt), L, ft)
    return [x, v, a, j, s, np.zeros_like(a)], lev


def schedule(lev, tau, L):
    step = np.int64(1) << (L - lev.astype(np.int64))
    due = tau.astype(np.int64) + step
    nxt = int(due.min())
    return nxt, np.nonzero(due == nxt)[0], step


def derivs(a0, j0, s0, a1, j1, s1, h):
    """a3, a4, a5 at h of the quintic through (a0, j0, s0) at 0 and (a1, j1, s1) at h."""
    da = a1 - a0
    a3 = (60 * da - h * (24 * j0 + 36 * j1) + h * h * (9 * s1 - 3 * s0)) / h ** 3
    a4 = (360 * da - h * (168 * j0 + 192 * j1) + h * h * (36 * s1 - 24 * s0)) / h ** 4
    a5 = (720 * da - 360 * h * (j0 + j1) + 60 * h * h * (s1 - s0)) / h ** 5
    return a3, a4, a5


def ref_block_step(T, m, S, lev, tau, dt, L, c, e2, eta, ft=LD, subset=None):
    """One block step of the scheme from the state S = (x, v, a, jerk, snap, crackle) as downloaded, in `ft`.  dt, the tick and
    h_i = T(tau_next - tau_i) * T(tick) are numbers of T.  subset: positions in the active list to evaluate (None: all).  Returns
    tau_next, the active list, the evaluated positions `sel` in it, the new x, v, a, j, s, k of those, their new levels, `want` and h."""
    nxt, act, step = schedule(lev, tau, L)
    dtT = T(dt)
    tick = T(dtT * T(2.0 ** -L))
    h = (np.asarray(nxt - tau.astype(np.int64), T) * tick).astype(ft)[:, None]
    x, v, a, j, s, k = (np.asarray(q, ft) for q in S)
    xp = x + h * v + h ** 2 / 2 * a + h ** 3 / 6 * j + h ** 4 / 24 * s + h ** 5 / 120 * k
    vp = v + h * a + h ** 2 / 2 * j + h ** 3 / 6 * s + h ** 4 / 24 * k
    ap = a + h * j + h ** 2 / 2 * s + h ** 3 / 6 * k
    sel = np.arange(len(act)) if subset is None else np.asarray(subset)
    t = act[sel]
    a1, j1, s1 = ref_force_jerk_snap(m, xp, vp, ap, c, e2, ft, targets=t)
    ha, a0, j0, s0, v0 = h[t], a[t], j[t], s[t], v[t]
    v1 = v0 + ha / 2 * (a0 + a1) + ha ** 2 / 10 * (j0 - j1) + ha ** 3 / 120 * (s0 + s1)
    x1 = x[t] + ha / 2 * (v0 + v1) + ha ** 2 / 10 * (a0 - a1) + ha ** 3 / 120 * (j0 + j1)
    k1, a4, a5 = derivs(a0, j0, s0, a1, j1, s1, ha)
    num = nrm(a1) * nrm(s1) + nrm(j1) ** 2
    den = nrm(k1) * nrm(a5) + nrm(a4) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        want = np.where(den > 0, ft(eta) * (num / np.where(den > 0, den, 1)) ** (ft(1) / ft(6)), ft(np.inf))
    hh, l = ha[:, 0], lev[t].astype(np.int64)
    down = want < hh
    deeper = np.minimum(np.maximum(l + 1, level_for(want, ft(dtT), L)), L)
    up = (~down) & (want >= 2 * hh) & (l > 0) & (nxt % (2 * step[t]) == 0)
    newl = np.where(down, deeper, np.where(up, l - 1, l))
    return dict(nxt=nxt, act=act, sel=sel, x=x1, v=v1, a=a1, j=j1, s=s1, k=k1, lev=newl, want=want, h=hh)


def apply_step(S, lev, tau, r, L):
    """Writes the result of a whole-list ref_block_step into the state."""
    t = r["act"]
    for q, key in zip(S, "xvajsk"):
        q[t] = r[key]
    lev[t] = r["lev"]
    tau[t] = 0 if r["nxt"] == 1 << L else r["nxt"]


def near_boundary(want, h, dt, L, tol):
    """want within a relative tol of h, 2 h or one of the steps dt 2^-l."""
    ft = want.dtype.type
    b = np.concatenate([np.stack([h, 2 * h], 1), np.broadcast_to(ft(dt) * ft(2) ** -np.arange(L + 1), (len(h), L + 1))], 1)
    return (np.abs(want[:, None] - b) <= ft(tol) * b).any(1)


def ref_block_run(T, m, x, v, dt, L, c, e2, eta, eta_start, nint):
    """`nint` intervals of dt with block steps, all in T: x, v, block steps, body steps, the deepest level seen."""
    m = np.asarray(m, T)
    S, lev = ref_start(m, x, v, c, e2, eta_start, dt, L, T)
    bsteps = bodysteps = deepest = 0
    for _ in range(nint):
        tau = np.zeros(len(m), np.int64)
        while True:
            r = ref_block_step(T, m, S, lev, tau, dt, L, c, e2, eta, ft=T)
            apply_step(S, lev, tau, r, L)
            bsteps += 1
            bodysteps += len(r["act"])
            deepest = max(deepest, int(lev.max()))
            if r["nxt"] == 1 << L:
                assert len(r["act"]) == len(m)
                break
    return S[0], S[1], bsteps, bodysteps, deepest


def ref_energy(m, x, v, c, e2):
    m, x, v = np.asarray(m, np.float64), np.asarray(x, np.float64), np.asarray(v, np.float64)
    d = x[None] - x[:, None]
    inv = 1 / np.sqrt((d * d).sum(-1) + np.float64(e2))
    np.fill_diagonal(inv, 0)
    return 0.5 * (m * (v * v).sum(-1)).sum() - 0.5 * c * (m[:, None] * m[None, :] * inv).sum()


# ---- the systems (those of tests/test_gpu_hermite_block.py, as arrays of float64) ---------------------------------------------------
def random_arrays(dim, n, seed):
    rng = np.random.default_rng(seed)
    m = rng.uniform(0.5, 1.5, n).astype(np.float64) / n
    x = rng.normal(0, 1, (n, dim)).astype(np.float64)
    v = rng.normal(0, 0.3, (n, dim)).astype(np.float64)
    return m, x, v


def binary_arrays(n=512, seed=2024, eps=0.002, sep=0.004):
    """A Gaussian cluster (sigma_x = 1, sigma_v = 0.3, m = 1 / N, c = 1) with bodies 0 and 1 made a circular binary of separation `sep`
    (circular in the softened potential)."""
    rng = np.random.default_rng(seed)
    m = np.full(n, 1.0 / n)
    x, v = rng.normal(0, 1, (n, 3)), rng.normal(0, 0.3, (n, 3))
    vc = np.sqrt((m[0] + m[1]) / sep) * (sep * sep / (sep * sep + eps * eps)) ** 0.75
    x[1] = x[0] + [sep, 0, 0]
    v[1] = v[0] + [0, vc, 0]
    return m, x, v


def graded_arrays(n=20000, seed=7, eta=0.1):
    """tests/test_gpu_hermite_block.py's graded_system with eta = eta_start: a Gaussian cluster of n bodies whose own steps are all
    dt = 2^-12 (level 0), and 365 near-massless satellites on circular orbits around 365 cluster bodies, sized so that eta / omega is
    sqrt(2) x the step of the satellite's level: 1 satellite at level 8, 1 at 7, 61 at 6, 1 at 5, 1 at 4, 300 at 3.  On a circular
    orbit |a^(k)| = omega^k |a|, so the start's eta_start |a| / |j| and the step's eta (num / den)^(1/6) are both eta / omega and the
    levels stay.  Returns m, x, v, dt, eps, L."""
    rng = np.random.default_rng(seed)
    dt, eps, L = 2.0 ** -12, 5e-6, 8
    m = np.full(n, 1.0 / n)
    x, v = rng.normal(0, 1, (n, 3)), rng.normal(0, 0.3, (n, 3))
    counts = {8: 1, 7: 1, 6: 61, 5: 1, 4: 1, 3: 300}
    pick = rng.choice(n, 2 * sum(counts.values()), replace=False)
    sats, hosts = pick[:len(pick) // 2], pick[len(pick) // 2:]
    k = 0
    for l, cnt in counts.items():
        omega = eta / (np.sqrt(2.0) * dt * 2.0 ** -l)
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
    return m, x, v, dt, eps, L
