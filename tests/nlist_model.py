"""A NumPy restatement of the fixed-radius neighbour lists of csrc/nlist.inc, in T arithmetic (float32 and float64): the definition by
brute force, a cell-list reference for large n, and the per-lane-cap walk over the shipped structure, for the part that can be
proved without a GPU — that the structure and the walk's rules give EXACTLY the brute-force lists.

The structure (keys, sort, buckets, boxes, the tree) and the arithmetic (fma, pair_d2, box_bound) are tests/nntree_model.py's, and
b2_of is tests/fof_model.py's, imported and not copied.  Restated here as shipped: r2_i = T(r) * T(r), or v_i * v_i, or v_i; the walk
of a wave of 64 consecutive sorted positions with a cap per lane — a node is skipped iff bound > r2_i in every lane (strict), lanes
past n carry -inf, the walk is FULL (every q != p, both sides) and ends at the root or the first dead node, padding is out by q < n
and the self pair by position; the hits of a lane come in ascending sorted position, and the segment is then put in ascending
original index by rank."""
import numpy as np

from fof_model import b2_of
from nntree_model import B, WAVE, Tree, box_bound, pair_d2

MAX_PER_BODY = 4096
OVER_CAPACITY, OVER_PER_BODY = 1, 2


def r2_of(dtype, n, r=None, radii=None, squared=False):
    """r2 (n,) of T: the scalar radius squared once in T, or the per-body values (one multiply in T, or none)."""
    if radii is None:
        return np.full(n, b2_of(r, dtype), dtype)
    v = np.asarray(radii, dtype)
    assert v.shape == (n,)
    with np.errstate(over="ignore"):
        return v.copy() if squared else (v * v).astype(dtype)


def pack(lists):
    """(count uint32 (n,), offset uint64 (n + 1,), idx uint32 (total,)) from one ascending index array per body."""
    count = np.array([len(l) for l in lists], np.uint32)
    offset = np.zeros(len(lists) + 1, np.uint64)
    offset[1:] = np.cumsum(count.astype(np.uint64))
    idx = np.concatenate(lists).astype(np.uint32) if len(lists) and offset[-1] else np.zeros(0, np.uint32)
    return count, offset, idx


def summary(count, capacity=None):
    """uint64[4]: total, the largest count, the lowest index that has it, status (for this capacity; None: whatever fits)."""
    total = int(count.astype(np.uint64).sum())
    most = int(count.max())
    status = (OVER_CAPACITY if capacity is not None and total > capacity else 0) | (OVER_PER_BODY if most > MAX_PER_BODY else 0)
    return np.array([total, most, int(np.argmax(count)), status], np.uint64)  # argmax: the first, so the lowest index


def brute(x, r=None, radii=None, squared=False):
    """The definition: L_i = {j != i : pair_d2(x_j, x_i) <= r2_i}, ascending.  O(n^2).  Returns (count, offset, idx)."""
    x = np.ascontiguousarray(x)
    n = len(x)
    r2 = r2_of(x.dtype, n, r, radii, squared)
    lists = []
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            hit = pair_d2(x, x[i]) <= r2[i]
            hit[i] = False
            lists.append(np.nonzero(hit)[0])
    return pack(lists)


def brute_many(x, rs):
    """The definition for several scalar radii at once (the d2 are computed once): [(count, offset, idx)] in the order of rs."""
    x = np.ascontiguousarray(x)
    n = len(x)
    r2s = [b2_of(r, x.dtype) for r in rs]
    lists = [[] for _ in rs]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            d2 = pair_d2(x, x[i])
            for k, r2 in enumerate(r2s):
                hit = d2 <= r2
                hit[i] = False
                lists[k].append(np.nonzero(hit)[0])
    return [pack(l) for l in lists]


def from_pairs(n, i, j):
    """(count, offset, idx) from the directed pairs (i lists j)."""
    order = np.lexsort((j, i))
    i, j = np.asarray(i, np.int64)[order], np.asarray(j, np.int64)[order]
    count = np.bincount(i, minlength=n).astype(np.uint32)
    offset = np.zeros(n + 1, np.uint64)
    offset[1:] = np.cumsum(count.astype(np.uint64))
    return count, offset, j.astype(np.uint32)


def cell_list_pairs(x, r):
    """The directed pairs (i, j), j != i, pair_d2 <= r2, of one scalar radius r > 0, for large n: only pairs in the same or in
    adjacent cells meet the emulated chain.  The cells' side is r (1 + 2^-10) — wider than r by far more than the rounding of the
    chain and of the cell coordinates, as fof_model.cell_list argues — so every pair with a computed d2 <= r2 is met."""
    x = np.ascontiguousarray(x)
    n, dim = x.shape
    r2 = b2_of(r, x.dtype)
    xd = x.astype(np.float64)
    side = float(r) * (1.0 + 2.0**-10)
    assert side > 0
    cell = np.floor((xd - xd.min(0)) / side).astype(np.int64) + 1  # >= 1: a neighbour's coordinate is never negative
    ext = cell.max(0) + 2
    mult = np.ones(dim, np.int64)
    for k in range(1, dim):
        mult[k] = mult[k - 1] * ext[k - 1]
    assert float(np.prod(ext.astype(np.float64))) < 2.0**62
    key = cell @ mult
    order = np.argsort(key, kind="stable")
    skey = key[order]
    offs = np.stack(np.meshgrid(*([np.array([-1, 0, 1])] * dim), indexing="ij"), -1).reshape(-1, dim)
    ei, ej = [], []
    for off in offs:
        nk = (cell + off) @ mult
        lo, hi = np.searchsorted(skey, nk, "left"), np.searchsorted(skey, nk, "right")
        cnt = hi - lo
        tot = int(cnt.sum())
        if tot == 0:
            continue
        i = np.repeat(np.arange(n), cnt)
        j = order[np.repeat(lo, cnt) + (np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
        keep = j != i
        i, j = i[keep], j[keep]
        with np.errstate(invalid="ignore", over="ignore"):
            ok = pair_d2(x[j], x[i]) <= r2
        ei.append(i[ok])
        ej.append(j[ok])
    ei = np.concatenate(ei) if ei else np.zeros(0, np.int64)
    ej = np.concatenate(ej) if ej else np.zeros(0, np.int64)
    return ei, ej


def cell_list(x, r):
    return from_pairs(len(x), *cell_list_pairs(x, r))


def rank_order(seg):
    """nlist_order_kernel: entry e goes to slot #{u in seg : u < e}."""
    seg = np.asarray(seg, np.int64)
    out = np.full(len(seg), -1, np.int64)
    rank = (seg[None, :] < seg[:, None]).sum(1)
    out[rank] = seg
    return out


def walk(x, r=None, radii=None, squared=False):
    """(count, offset, idx, Tree) by the shipped structure and walk; Tree.pairs counts the pairs evaluated (one pass)."""
    x = np.ascontiguousarray(x)
    t = Tree(x)
    n = t.n
    r2 = r2_of(x.dtype, n, r, radii, squared)
    padded = ((n + 255) // 256) * 256
    sx = np.zeros((padded, t.dim), x.dtype)  # the sorted records are padded to whole blocks, padding at the origin
    sx[:len(t.sx)] = t.sx
    sj = np.full(padded, -1, np.int64)
    sj[:n] = t.sj[:n]
    U = 2 if x.dtype == np.float64 else 4
    lists = [None] * n
    with np.errstate(invalid="ignore", over="ignore"):
        for wave in range((n + WAVE - 1) // WAVE):
            tp = wave * WAVE + np.arange(WAVE)
            live = tp < n
            xi = sx[tp]
            cap = np.full(WAVE, -np.inf, x.dtype)
            cap[live] = r2[sj[tp[live]]]
            hits = [[] for _ in range(WAVE)]
            node = 1
            while True:
                depth = node.bit_length() - 1
                sh = t.levels - depth
                first = (node - (1 << depth)) << sh
                q0 = first * B
                if q0 >= n:
                    break
                bound = box_bound(t.lo[node][None, :], t.hi[node][None, :], xi)
                assert not np.isnan(bound).any(), "a dead node's box was read"
                if (~(bound > cap)).any():
                    if sh != 0:
                        node = 2 * node
                        continue
                    for jj in range(0, B, U):
                        q = q0 + jj + np.arange(U)
                        d2 = pair_d2(sx[q][None, :, :], xi[:, None, :])  # (64, U)
                        t.pairs += d2.size
                        hit = live[:, None] & (q[None, :] < n) & (q[None, :] != tp[:, None]) & (d2 <= cap[:, None])
                        for u in range(U):
                            for lane in np.nonzero(hit[:, u])[0]:
                                hits[lane].append(sj[q[u]])
                node += 1
                while node % 2 == 0:
                    node >>= 1
                if node == 1:
                    break
            for lane in np.nonzero(live)[0]:
                lists[sj[tp[lane]]] = rank_order(hits[lane])
    return (*pack(lists), t)
