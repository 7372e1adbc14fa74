"""A wide (np.longdouble) reference of the three pair sums of csrc/hermite_tile.hpp with a per-body magnitude scale beside each, the
bounds that go with it, and the systems its tests share.  Not a test: tests/test_hermite_wide_model.py (CPU) and
tests/test_gpu_hermite_wide.py import it.  The construction is oracle.all_pairs_force_wide's, carried over to the jerk and the snap.

The sums, for a target i over all sources j (the self pair adds 0: d = u = b = 0):
    a_i = c sum w d,   j_i = c sum w (u - 3 alpha d),   s_i = c sum w (b - 6 alpha u + (15 alpha^2 - 3 gamma) d)
    d = x_j - x_i, u = v_j - v_i, b = acc_j - acc_i, q = |d|^2 + e2, w = m_j q^(-3/2), alpha = d.u / q, gamma = (|u|^2 + d.b) / q
The scales: the same expressions with every product replaced by the product of norms and every sum by the sum of absolute values:
    S0_i = |c| sum |w| |d|
    S1_i = |c| sum |w| (|u| + 3 |d|^2 |u| / q)
    S2_i = |c| sum |w| (|b| + 6 |d| |u|^2 / q + (15 |d|^2 |u|^2 / q^2 + 3 (|u|^2 + |d| |b|) / q) |d|)
The error measure of a quantity g of body i:  E_g,i = max_k |got - ref| / (eps_T S_g,i),  eps_T = np.finfo(T).eps.

The bounds.  P[T] = (P_a, P_j, P_s) is the rounding error of ONE pair term in units of eps_T times its scale, as the comment block of
csrc/hermite_tile.hpp derives it from the kernel's arithmetic (one rounding = 0.5): 2.5 / 5 / 7 in double, 4.5 / 8.5 / 12 in float; the
jerk's figure is the same for both orders.  A body's sum adds L = chain_length(plan) roundings to that, the longest addition chain
of the launch plan; an isolated pair (n = 2) adds 1.5: the difference d (or u, b), the FMA into the sum and the scaling by c."""
import numpy as np

LD = np.longdouble
TOL = {np.float64: 1e-12, np.float32: 2e-5}  # the global criterion of the older Hermite tests: max|got - ref| / max|ref|
P = {np.float64: (2.5, 5.0, 7.0), np.float32: (4.5, 8.5, 12.0)}
PAIR_EXTRA = 1.5
C = 0.37  # the factor c of every test that is about c: not 1, not a power of two
H_WAVES, H_TILE = 4, 256  # kHWaves, kHTile of csrc/hermite_tile.hpp


def eps_of(T):
    return LD(np.finfo(T).eps)


def maxrel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def nrm(a):
    return np.sqrt((a * a).sum(-1))


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def pair_sums(ft, m, x, v, acc, c, e2, targets=None, w_factor=None, snap_c_twice=False):
    """The sums and their scales in the float type `ft`, from arrays of any type, for the bodies `targets` (None: all); sources in
    index order.  acc None: no snap (its sum and scale come back as None).  Returns (a, j, s), (S0, S1, S2), each (len(targets), D)
    or (len(targets),).  w_factor and snap_c_twice are the seeded faults of the CPU tests: w scaled by a factor, c applied twice to the
    snap."""
    m, x, v = np.asarray(m, ft), np.asarray(x, ft), np.asarray(v, ft)
    acc = None if acc is None else np.asarray(acc, ft)
    n, D = x.shape
    idx = np.arange(n) if targets is None else np.asarray(targets)
    c, e2 = ft(c), ft(e2)
    out = [np.zeros((len(idx), D), ft) for _ in range(3)]
    scl = [np.zeros(len(idx), ft) for _ in range(3)]
    step = max(1, min(256, (1 << 18) // n))
    for o in range(0, len(idx), step):
        t = idx[o:o + step]
        d, u = x[None] - x[t][:, None], v[None] - v[t][:, None]
        dd, uu, du = (d * d).sum(-1), (u * u).sum(-1), (d * u).sum(-1)
        q = dd + e2
        w = m[None] / (q * np.sqrt(q))
        if w_factor is not None:
            w = w * ft(w_factor)
        al = du / q
        nd, nu = np.sqrt(dd), np.sqrt(uu)
        W, A = w[:, :, None], al[:, :, None]
        out[0][o:o + step] = (W * d).sum(1)
        out[1][o:o + step] = (W * (u - ft(3) * A * d)).sum(1)
        scl[0][o:o + step] = (np.abs(w) * nd).sum(1)
        scl[1][o:o + step] = (np.abs(w) * (nu + ft(3) * dd * nu / q)).sum(1)
        if acc is not None:
            b = acc[None] - acc[t][:, None]
            bb = (b * b).sum(-1)
            nb = np.sqrt(bb)
            ga = ((uu + (d * b).sum(-1)) / q)[:, :, None]
            out[2][o:o + step] = (W * (b - ft(6) * A * u + (ft(15) * A * A - ft(3) * ga) * d)).sum(1)
            scl[2][o:o + step] = (np.abs(w) * (nb + ft(6) * nd * uu / q + (ft(15) * dd * uu / (q * q) + ft(3) * (uu + nd * nb) / q) * nd)).sum(1)
    sums = [c * o for o in out]
    if snap_c_twice:
        sums[2] = c * sums[2]
    scales = [abs(c) * s for s in scl]
    if acc is None:
        sums[2] = scales[2] = None
    return tuple(sums), tuple(scales)


def wide(m, x, v, acc, c, e2, targets=None):
    """pair_sums in np.longdouble: the reference."""
    return pair_sums(LD, m, x, v, acc, c, e2, targets)


def err_units(got, ref, scale, T):
    """E_g,i per body: max_k |got - ref| / (eps_T S_g,i) as float64; where the scale is 0 (no source pulls), 0 if got == ref and inf
    otherwise."""
    diff = np.abs(np.asarray(got, LD) - np.asarray(ref, LD)).max(-1)
    scale = np.asarray(scale, LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, diff / (eps_of(T) * np.where(scale > 0, scale, 1)), np.where(diff == 0, LD(0), LD(np.inf)))
    return e.astype(np.float64)


# ---- the launch plans and the chain length -----------------------------------------------------------------------------------------
def plan_for(n, min_chunks):
    """hermite_plan_for(sz, min_chunks) of csrc/hermite_tile.hpp: (R, blocks, ntiles, chunks, tiles_per_chunk).  Order 4 passes 1,
    order 6 passes 2."""
    return block_plan_for(n, n, min_chunks, cap=64)


def block_plan_for(n, n_act, min_chunks, cap=None):
    """hermite_block_plan_for(sz, n_act, min_chunks) of csrc/hermite_block_plan.hpp: the blocks counted over the active targets, no cap
    of 64 on the chunks."""
    R = 2 if n_act >= 65536 else 1
    blocks = (n_act + 64 * R - 1) // (64 * R)
    ntiles = (n + H_TILE - 1) // H_TILE
    want = (2048 + blocks - 1) // blocks
    if cap is not None:
        want = min(want, cap)
    want = min(max(want, min_chunks), ntiles)
    tpc = (ntiles + want - 1) // want
    return R, blocks, ntiles, (ntiles + tpc - 1) // tpc, tpc


def chain_length(plan):
    """The longest addition chain of a body's sum under a plan: a wave adds its 64 records of every tile of the chunk, the block adds
    the other three waves' sums, the corrector adds the other chunks' sums (one after the other up to 64 chunks; more go through a
    reduce kernel, which no test here reaches) and scales by c."""
    _, _, _, chunks, tpc = plan
    assert chunks <= 64
    return 64 * tpc + (H_WAVES - 1) + (chunks - 1) + 1


# ---- the systems -------------------------------------------------------------------------------------------------------------------
def e2_of(T, eps):
    return T(T(eps) * T(eps))


def gaussian_cluster(T, dim, n, seed):
    """The system of the older Hermite tests: m = U(0.5, 1.5) / n, sigma_x = 1, sigma_v = 0.3 (used with eps = 0.05, c = 1)."""
    rng = np.random.default_rng(seed)
    return ((rng.uniform(0.5, 1.5, n) / n).astype(T), rng.normal(0, 1, (n, dim)).astype(T), rng.normal(0, 0.3, (n, dim)).astype(T))


def unit(rng, shape):
    g = rng.normal(0, 1, shape)
    return g / np.sqrt((g * g).sum(-1, keepdims=True))


ADV_EPS = {np.float64: 1e-4, np.float32: 1e-2}
ADV_LIMIT = {np.float64: 1e32, np.float32: 1e23}


def adv_limit(T, n):
    """Every reference value and scale of adversarial(T, dim, n) stays below this: 1e32 in double and 1e23 in float up to 5889 bodies
    (nine and fifteen decades under the largest float and far below the largest double: a same-precision evaluation stays finite).
    The largest scale is the snap's in the cores of the clusters, sum |w| |b| over the bodies within eps, where both the number of
    terms and |b| (a difference of accelerations made there) grow like n; so above 5889 bodies the limit grows like n^2: 1.24e34 and
    1.24e25 at 65537 (measured: 6.5e33 and 1.4e24, at 5889 bodies 8.6e31 and 1.8e22)."""
    return ADV_LIMIT[T] * max(1.0, n / 5889.0) ** 2


def adversarial(T, dim, n, seed=21):
    """Twelve cluster centres from N(0, 30^2); each body at a centre plus a Gaussian whose radius is log-uniform over [1e-5, 10] in
    double, [1e-3, 10] in float; speeds log-uniform over [1e-2, 10], masses over [1e-6, 1e6].  Planted, at 26 distinct random indices:
    ten exactly coincident pairs (different velocities), one body at 1e5 on the first axis, five zero masses.  Returns m, x, v of T
    and the planted indices."""
    rng = np.random.default_rng([seed, n, dim])
    centres = rng.normal(0, 30, (12, dim))
    radius = 10.0 ** rng.uniform(-5 if T is np.float64 else -3, 1, n)
    x = centres[rng.integers(0, 12, n)] + radius[:, None] * rng.normal(0, 1, (n, dim))
    v = 10.0 ** rng.uniform(-2, 1, n)[:, None] * unit(rng, (n, dim))
    m = 10.0 ** rng.uniform(-6, 6, n)
    planted = rng.choice(n, 26, replace=False)
    m, x, v = m.astype(T), x.astype(T), v.astype(T)
    x[planted[10:20]] = x[planted[:10]]
    x[planted[20]] = 0
    x[planted[20], 0] = 1e5
    m[planted[21:]] = 0
    return m, x, v, planted


def targets_for(n, planted, seed=5):
    """All bodies below 4097; from there the first and the last body, every planted body and a fixed random remainder: 256 in all up
    to 20 000 bodies, 64 above (a longdouble pair costs about 1 us)."""
    if n < 4097:
        return np.arange(n)
    total = 256 if n <= 20000 else 64
    fixed = np.unique(np.concatenate(([0, n - 1], planted)))
    rest = np.setdiff1d(np.arange(n), fixed)
    return np.sort(np.concatenate((fixed, np.random.default_rng(seed).choice(rest, total - len(fixed), replace=False))))


def isolated_pairs(T, dim, count, eps, seed):
    """`count` two-body systems: separations log-uniform over eps [2^-10, 2^20] in a random direction, the pair placed within two
    separations of the origin (so that the coordinates resolve the separation in float too); relative speeds over four decades
    (1e-2 .. 1e2), mass ratios over twelve (1e-6 .. 1e6).  Returns m (count, 2), x and v (count, 2, dim) of T."""
    rng = np.random.default_rng([seed, dim, int(np.dtype(T).itemsize)])
    sep = eps * 2.0 ** rng.uniform(-10, 20, count)
    x0 = sep[:, None] * rng.uniform(-2, 2, (count, dim))
    x = np.stack([x0, x0 + sep[:, None] * unit(rng, (count, dim))], 1)
    v0 = rng.normal(0, 1, (count, dim))
    v = np.stack([v0, v0 + 10.0 ** rng.uniform(-2, 2, count)[:, None] * unit(rng, (count, dim))], 1)
    m0 = 10.0 ** rng.uniform(-1, 1, count)
    m = np.stack([m0, m0 * 10.0 ** rng.uniform(-6, 6, count)], 1)
    return m.astype(T), x.astype(T), v.astype(T)


def lattice_system(T, dim, n, seed):
    """n bodies on a jittered lattice of spacing 2 (jitter +-0.4 per axis: mutual distances >= 1.2), m = U(0.5, 1.5), speeds N(0, 1)."""
    rng = np.random.default_rng([seed, dim])
    side = int(np.ceil(n ** (1.0 / dim)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * dim, indexing="ij"), -1).reshape(-1, dim)
    x = 2.0 * grid[rng.permutation(len(grid))[:n]] + rng.uniform(-0.4, 0.4, (n, dim))
    return rng.uniform(0.5, 1.5, n).astype(T), x.astype(T), rng.normal(0, 1, (n, dim)).astype(T)


# ---- the predictor and the block schedule in longdouble ------------------------------------------------------------------------------------------
def predict(S, h):
    """The Taylor predictor of either order from the state S = (x, v, a, jerk) or (x, v, a, jerk, snap, crackle), h of shape (n, 1)
    or a scalar, in longdouble: (xp, vp) or (xp, vp, ap)."""
    S = [np.asarray(z, LD) for z in S]
    h = np.asarray(h, LD)
    if len(S) == 4:
        x, v, a, j = S
        return x + h * (v + h / 2 * (a + h / 3 * j)), v + h * (a + h / 2 * j)
    x, v, a, j, s, k = S
    return (x + h * (v + h / 2 * (a + h / 3 * (j + h / 4 * (s + h / 5 * k)))), v + h * (a + h / 2 * (j + h / 3 * (s + h / 4 * k))),
            a + h * (j + h / 2 * (s + h / 3 * k)))


def schedule(lev, tau, L):
    """The block-step schedule: tau_next, the active list (ascending), the bodies' steps in ticks."""
    step = np.int64(1) << (L - lev.astype(np.int64))
    due = tau.astype(np.int64) + step
    nxt = int(due.min())
    return nxt, np.nonzero(due == nxt)[0], step


def block_h(T, dt, L, nxt, tau):
    """h_i = T(tau_next - tau_i) * T(tick) as the scheme makes them, (n, 1) in longdouble."""
    tick = T(T(dt) * T(2.0 ** -L))
    return (np.asarray(nxt - tau.astype(np.int64), T) * tick).astype(LD)[:, None]
