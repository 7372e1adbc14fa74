"""A NumPy restatement of the tree-pruned exact kNN of csrc/nntree.inc, in T arithmetic (float32 and float64), for the one part of
that method that can be proved without a GPU: that the structure and the walk's rules give EXACTLY the brute-force lists.

Restated as shipped: the keys (quantised in double on the bounds, 21 bits an axis in 3D and 32 in 2D, clamped, zero extent -> zero
bits), the sort by (key, position), buckets of B = 32 sorted records with the min / max box of their records p < n, the complete
binary tree of box unions in heap order with dead nodes decided by index, the walk's visiting order for a wave of 64 consecutive
sorted positions (one ballot per node: skipped only if bound > cap in EVERY lane), the bound's chain, the batches of U records with
the `<=` gate, the lexicographic insert into a list of capacity K in {4, 8, 16}, the cap at the k-th entry, masked records turned into
(+inf, 0xffffffff) — skipped —, lanes past n with a list of -inf, and the seed (the wave's two buckets and two on either side, kept
in the list and skipped by index in the walk).

fma(a, b, c) is emulated exactly (Boldo & Melquiond 2008: TwoProduct, TwoSum, one addition rounded to odd, one rounded to nearest)
in double, and for float through the exact double product and an addition rounded to odd; tests/test_nntree_model.py holds it to
libm's fma.  Not valid where a product underflows: the tests' data does not go there."""
import numpy as np

B = 32
SEED = 2  # buckets on either side of the wave's own that the seed sweeps
NONE = 0xFFFFFFFF
WAVE = 64


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _add_to_odd(a, b):
    """a + b in double rounded to ODD: exact sums stay, inexact ones take the neighbour with an odd last bit."""
    s, e = _two_sum(a, b)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0) & np.isfinite(s)
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s)


def _two_prod(a, b):
    p = a * b
    c = 134217729.0  # 2^27 + 1 (Veltkamp)
    ah = (a * c) - ((a * c) - a)
    al = a - ah
    bh = (b * c) - ((b * c) - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma(a, b, c):
    """Correctly rounded a * b + c, elementwise, in the arrays' type (float32 or float64)."""
    a, b, c = np.asarray(a), np.asarray(b), np.asarray(c)
    with np.errstate(invalid="ignore", over="ignore"):
        if a.dtype == np.float32:
            p = a.astype(np.float64) * b.astype(np.float64)  # exact: 48 bits
            return _add_to_odd(p, c.astype(np.float64)).astype(np.float32)
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        r = th + _add_to_odd(tl, ul)
        plain = a * b + c
        return np.where(np.isfinite(r), r, plain)  # inf / nan operands: what IEEE gives


def pair_d2(xs, xi):
    """pair_d2 of csrc/pair_sweep.hpp: d = xs - xi, t = d_0 d_0, t = fma(d_k, d_k, t).  xs (..., D), xi (D,) or (..., D)."""
    d = xs - xi
    t = d[..., 0] * d[..., 0]
    for k in range(1, d.shape[-1]):
        t = fma(d[..., k], d[..., k], t)
    return t


def box_bound(lo, hi, xi):
    """nntree_bound: g_k = max(lo_k - x_k, x_k - hi_k, 0), the same chain."""
    g = np.maximum(np.maximum(lo - xi, xi - hi), xi.dtype.type(0))
    t = g[..., 0] * g[..., 0]
    for k in range(1, g.shape[-1]):
        t = fma(g[..., k], g[..., k], t)
    return t


def _spread(q, dim):
    out = np.zeros(q.shape, np.uint64)
    step = np.uint64(3 if dim == 3 else 2)
    for bit in range(21 if dim == 3 else 32):
        out |= ((q >> np.uint64(bit)) & np.uint64(1)) << (np.uint64(bit) * step)
    return out


def morton_keys(x):
    n, dim = x.shape
    cells = 2097152.0 if dim == 3 else 4294967296.0
    key = np.zeros(n, np.uint64)
    xd = x.astype(np.float64)
    for k in range(dim):
        lo, hi = xd[:, k].min(), xd[:, k].max()
        ext = hi - lo
        sc = cells / ext if (ext > 0 and np.isfinite(ext)) else 0.0
        v = (xd[:, k] - lo) * sc
        q = np.where(v >= cells - 1, cells - 1, np.where(v > 0, np.floor(v), 0.0)).astype(np.uint64)
        key |= _spread(q, dim) << np.uint64(k)
    return key


class Tree:
    def __init__(self, x):
        self.x = x
        self.n, self.dim = x.shape
        n, T = self.n, x.dtype.type
        self.perm = np.lexsort((np.arange(n), morton_keys(x)))  # by (key, position)
        self.buckets = (n + B - 1) // B
        self.levels = 0
        while (1 << self.levels) < self.buckets:
            self.levels += 1
        self.leaves = 1 << self.levels
        padded = self.buckets * B
        self.sx = np.zeros((padded, self.dim), x.dtype)  # padding at the origin
        self.sx[:n] = x[self.perm]
        self.sj = np.full(padded, NONE, np.int64)
        self.sj[:n] = self.perm
        self.lo = np.full((2 * self.leaves, self.dim), np.nan, x.dtype)  # dead nodes stay NaN: reading one would poison a result
        self.hi = np.full((2 * self.leaves, self.dim), np.nan, x.dtype)
        for b in range(self.buckets):
            r = self.sx[b * B:min((b + 1) * B, n)]
            self.lo[self.leaves + b], self.hi[self.leaves + b] = r.min(0), r.max(0)
        for d in range(self.levels - 1, -1, -1):
            sh = self.levels - d
            for q in range(1 << d):
                first = q << sh
                if first * B >= n:
                    break
                i = (1 << d) + q
                lo, hi = self.lo[2 * i], self.hi[2 * i]
                if (first + (1 << (sh - 1))) * B < n:
                    lo, hi = np.minimum(lo, self.lo[2 * i + 1]), np.maximum(hi, self.hi[2 * i + 1])
                self.lo[i], self.hi[i] = lo, hi
        self.pairs = 0  # pairs evaluated, all waves


def _insert(ld, lj, d, j):
    """knn_insert<T, K, true> for the 64 lanes at once: (d, j) lexicographically into every lane's ascending list."""
    below = (d[:, None] < ld) | ((d[:, None] == ld) & (j[:, None] < lj))
    nd, nj = ld.copy(), lj.copy()
    nd[:, 1:] = np.where(below[:, :-1], ld[:, :-1], np.where(below[:, 1:], d[:, None], ld[:, 1:]))
    nj[:, 1:] = np.where(below[:, :-1], lj[:, :-1], np.where(below[:, 1:], j[:, None], lj[:, 1:]))
    nd[:, 0] = np.where(below[:, 0], d, ld[:, 0])
    nj[:, 0] = np.where(below[:, 0], j, lj[:, 0])
    return nd, nj


def _bucket(t, st, b, check):
    """nntree_bucket: bucket b against the wave's lanes; st = [ld, lj, cap, xi, tp, k]."""
    ld, lj, cap, xi, tp, k = st
    T = t.x.dtype.type
    U = 2 if t.x.dtype == np.float64 else 4
    for jj in range(0, B, U):
        p = b * B + jj + np.arange(U)
        d2 = pair_d2(t.sx[p][None, :, :], xi[:, None, :])  # (64, U)
        j = np.broadcast_to(t.sj[p], d2.shape).copy()
        t.pairs += d2.size
        if check:
            ok = (p[None, :] < t.n) & (p[None, :] != tp[:, None])
            d2 = np.where(ok, d2, T(np.inf))
            j = np.where(ok, j, NONE)
        if (d2.min(1) <= cap).any():
            for u in range(U):
                if (d2[:, u] <= cap).any():
                    ld, lj = _insert(ld, lj, d2[:, u], np.where(d2[:, u] < np.inf, j[:, u], NONE))
            cap = ld[:, k - 1].copy()
    st[0], st[1], st[2] = ld, lj, cap


def knn_tree(x, k):
    """(idx (n, k) uint32, d2 (n, k) of T) by the shipped structure and walk; also returns the Tree (its .pairs is the work)."""
    x = np.ascontiguousarray(x)
    t = Tree(x)
    n, T = t.n, x.dtype.type
    K = 4 if k <= 4 else 8 if k <= 8 else 16
    idx = np.full((n, k), NONE, np.uint32)
    out = np.full((n, k), np.inf, x.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for wave in range((n + WAVE - 1) // WAVE):
            tp = wave * WAVE + np.arange(WAVE)
            live = tp < n
            xi = np.zeros((WAVE, t.dim), x.dtype)
            xi[live] = t.sx[tp[live]]
            ld = np.where(live[:, None], T(np.inf), T(-np.inf)) * np.ones((WAVE, K), x.dtype)
            lj = np.full((WAVE, K), NONE, np.int64)
            st = [ld, lj, ld[:, K - 1].copy(), xi, tp, k]
            own = wave * 2
            s0, s1 = max(own - SEED, 0), min(own + 2 + SEED, t.buckets)
            for b in range(s0, s1):
                _bucket(t, st, b, True)
            node = 1
            while True:
                depth = node.bit_length() - 1
                sh = t.levels - depth
                first = (node - (1 << depth)) << sh
                if first * B >= n:
                    break
                bound = box_bound(t.lo[node][None, :], t.hi[node][None, :], xi)
                assert not np.isnan(bound).any(), "a dead node's box was read"
                if (~(bound > st[2])).any():
                    if sh != 0:
                        node = 2 * node
                        continue
                    if first < s0 or first >= s1:
                        _bucket(t, st, first, (first + 1) * B > n)
                node += 1
                while node % 2 == 0:
                    node >>= 1
                if node == 1:
                    break
            rows = t.sj[tp[live]]
            idx[rows] = st[1][live][:, :k].astype(np.uint32)
            out[rows] = st[0][live][:, :k]
    return idx, out, t


def brute(x, k):
    """The definition: per body the k smallest (d2 by pair_d2's chain in T, index), j != i; unused slots (0xffffffff, +inf)."""
    x = np.ascontiguousarray(x)
    n = len(x)
    idx = np.full((n, k), NONE, np.uint32)
    out = np.full((n, k), np.inf, x.dtype)
    have = min(k, n - 1)
    order = np.arange(n)
    for i in range(n):
        d2 = pair_d2(x, x[i])
        keep = order != i
        o = np.lexsort((order[keep], d2[keep]))[:have]
        idx[i, :have] = order[keep][o]
        out[i, :have] = d2[keep][o]
    return idx, out
