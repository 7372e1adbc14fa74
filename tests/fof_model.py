"""A NumPy restatement of the friends-of-friends group finder of csrc/fof.inc, in T arithmetic (float32 and float64), for the part of
it that can be proved without a GPU: that the structure and the link walk's rules give EXACTLY the brute-force partition.

The structure (keys, sort, buckets, boxes, the tree) and the arithmetic (fma, pair_d2, box_bound) are tests/nntree_model.py's, imported
and not copied.  Restated here as shipped: b2 = T(b) * T(b); the link walk of a wave of 64 consecutive sorted positions — a node is
skipped iff no lane has !(bound > b2) (strict), dead lanes take part in that ballot with the padding record's position, a lane at p
links only to records at q < p, the walk ends at the first dead node or the first node that starts past the wave's last position —
and a sequential union-find with the kernel's rule (the larger root is pointed at the smaller).  Also here, because the GPU tests need
them: the brute-force O(n^2) reference over the emulated chain, a cell-list reference for large n, the summary and the catalogue's
wide reference with its error bound."""
import numpy as np

from nntree_model import B, NONE, WAVE, Tree, box_bound, fma, morton_keys, pair_d2  # noqa: F401  (re-exported for the tests)


def b2_of(b, dtype):
    """T(b) * T(b), rounded once in T."""
    t = np.dtype(dtype).type
    with np.errstate(over="ignore"):
        return t(t(b) * t(b))


def find(parent, x):
    """fof_find: the root of x, with path halving."""
    while True:
        p = parent[x]
        if p == x:
            return x
        g = parent[p]
        if g == p:
            return p
        parent[x] = g
        x = g


def hook(parent, a, b):
    """fof_hook without a rival: the larger root is pointed at the smaller."""
    ra, rb = find(parent, a), find(parent, b)
    if ra == rb:
        return False
    if ra < rb:
        ra, rb = rb, ra
    parent[ra] = rb
    return True


def labels_from_parent(parent, index, n):
    """label (the lowest original index of the set) and size per ORIGINAL body, from a forest over positions whose body is index[p]."""
    root = np.array([find(parent, p) for p in range(n)], np.int64)
    minidx = np.full(n, NONE, np.int64)
    np.minimum.at(minidx, root, index[:n])
    count = np.bincount(root, minlength=n)
    label = np.zeros(n, np.uint32)
    size = np.zeros(n, np.uint32)
    label[index[:n]] = minidx[root]
    size[index[:n]] = count[root]
    return label, size


def fof_tree(x, b):
    """(label, size, Tree) by the shipped structure and link walk; Tree.pairs counts the pairs evaluated."""
    x = np.ascontiguousarray(x)
    t = Tree(x)
    n = t.n
    b2 = b2_of(b, x.dtype)
    padded = ((n + 255) // 256) * 256
    parent = list(range(padded))
    sx = np.zeros((padded, t.dim), x.dtype)  # the sorted records are padded to whole blocks, padding at the origin
    sx[:len(t.sx)] = t.sx
    U = 2 if x.dtype == np.float64 else 4
    with np.errstate(invalid="ignore", over="ignore"):
        for wave in range((n + WAVE - 1) // WAVE):
            tp = wave * WAVE + np.arange(WAVE)
            last = wave * WAVE + WAVE - 1
            live = tp < n
            xi = sx[tp]
            node = 1
            while True:
                depth = node.bit_length() - 1
                sh = t.levels - depth
                first = (node - (1 << depth)) << sh
                q0 = first * B
                if q0 >= n or q0 > last:
                    break
                bound = box_bound(t.lo[node][None, :], t.hi[node][None, :], xi)
                assert not np.isnan(bound).any(), "a dead node's box was read"
                if (~(bound > b2)).any():
                    if sh != 0:
                        node = 2 * node
                        continue
                    for jj in range(0, B, U):
                        if q0 + jj > last:
                            break
                        q = q0 + jj + np.arange(U)
                        d2 = pair_d2(sx[q][None, :, :], xi[:, None, :])  # (64, U)
                        t.pairs += d2.size
                        hit = live[:, None] & (q[None, :] < tp[:, None]) & (d2 <= b2)
                        for u in range(U):
                            for lane in np.nonzero(hit[:, u])[0]:
                                hook(parent, int(tp[lane]), int(q[u]))
                node += 1
                while node % 2 == 0:
                    node >>= 1
                if node == 1:
                    break
    label, size = labels_from_parent(parent, t.sj, n)
    return label, size, t


def labels_from_edges(n, ei, ej):
    """(label, size) of the components of the graph on 0 .. n - 1 with edges (ei, ej): minimum-label propagation with pointer
    jumping, integers only."""
    label = np.arange(n, dtype=np.int64)
    ei, ej = np.asarray(ei, np.int64), np.asarray(ej, np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, ei, label[ej])
        np.minimum.at(new, ej, label[ei])
        while True:
            nn = new[new]
            if (nn == new).all():
                break
            new = nn
        if (new == label).all():
            break
        label = new
    size = np.bincount(label, minlength=n)[label]
    return label.astype(np.uint32), size.astype(np.uint32)


def brute_many(x, bs):
    """The definition, for several linking lengths at once: every pair's d2 by pair_d2's chain in T against each b2, components of
    that graph.  O(n^2); the d2 are computed once.  Returns [(label, size)] in the order of bs."""
    x = np.ascontiguousarray(x)
    n = len(x)
    b2s = [b2_of(b, x.dtype) for b in bs]
    ei, ej = [[] for _ in bs], [[] for _ in bs]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(1, n):
            d2 = pair_d2(x[:i], x[i])
            for k, b2 in enumerate(b2s):
                j = np.nonzero(d2 <= b2)[0]
                ei[k].append(np.full(len(j), i))
                ej[k].append(j)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.int64)
    return [labels_from_edges(n, cat(ei[k]), cat(ej[k])) for k in range(len(bs))]


def brute(x, b):
    return brute_many(x, [b])[0]


def cell_list(x, b):
    """The same partition for large n: only pairs in adjacent cells meet the emulated chain.  The cells' side is b (1 + 2^-10) — wider
    than b by far more than the rounding of the chain and of the cell coordinates — so every pair with a computed d2 <= b2 lies in
    the same or in adjacent cells."""
    x = np.ascontiguousarray(x)
    n, dim = x.shape
    b2 = b2_of(b, x.dtype)
    xd = x.astype(np.float64)
    side = float(b) * (1.0 + 2.0**-10)
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
        keep = j < i
        i, j = i[keep], j[keep]
        with np.errstate(invalid="ignore", over="ignore"):
            d2 = pair_d2(x[j], x[i])
        ok = d2 <= b2
        ei.append(i[ok])
        ej.append(j[ok])
    ei = np.concatenate(ei) if ei else np.zeros(0, np.int64)
    ej = np.concatenate(ej) if ej else np.zeros(0, np.int64)
    return labels_from_edges(n, ei, ej)


def summary(label, size, min_members):
    """uint32[4]: groups, catalogued groups, the largest size, its label (the lowest among equals)."""
    heads = np.nonzero(label == np.arange(len(label)))[0]
    s = size[heads].astype(np.int64)
    best = heads[np.lexsort((heads, -s))[0]]
    return np.array([len(heads), int((s >= min_members).sum()), size[best], best], np.uint32)


def catalogue(label, size, m, x, min_members):
    """The catalogue's reference: labels and sizes exactly; mass and com in longdouble with, per entry, the bound a double
    accumulation of `size` terms plus one rounding to T may differ from it by (see tests/test_gpu_fof.py)."""
    heads = np.nonzero((label == np.arange(len(label))) & (size >= min_members))[0]
    ld = np.longdouble
    out = {"label": heads.astype(np.uint32), "size": size[heads].astype(np.uint32), "mass": [], "com": [], "sum_abs_mx": []}
    order = np.argsort(label, kind="stable")
    starts = np.searchsorted(label[order], heads)
    for h, s0 in zip(heads, starts):
        mem = order[s0:s0 + int(size[h])]
        mm, xx = m[mem].astype(ld), x[mem].astype(ld)
        out["mass"].append(mm.sum())
        out["com"].append((mm[:, None] * xx).sum(0) / mm.sum())
        out["sum_abs_mx"].append(np.abs(mm[:, None] * xx).sum(0))
    for k in ("mass", "com", "sum_abs_mx"):
        out[k] = np.array(out[k], ld).reshape((len(heads),) if k == "mass" else (len(heads), x.shape[1]))
    return out
