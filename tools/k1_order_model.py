#!/usr/bin/env python3
"""K1's space order (csrc/k1_order_key.hpp, csrc/all_pairs.hip) restated in NumPy, on the CPU: the key, the order, the source
chunks' boxes and the far certificate (csrc/common.hpp: k1_block_is_far) of a whole-system launch — and, as a command, the share of
(target group, source chunk) blocks that certify and the share of the remaining batches that are "mixed" (some lane holds a pair
closer than 2) for a host-generated system, in natural order and in space order.

    python tools/k1_order_model.py [--n 1048576] [--workload galaxy] [--dim 3] [--r 2] [--mixed-sample 200]

tests/test_k1_space_order_model.py and tests/test_gpu_space_order.py import the functions."""
import argparse
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP = 3.0          # common.hpp: kFarGap
TILE = 512         # common.hpp: kTileJ
HALF = 512         # k1_order_key.hpp: kOrderHalf (cells of side 1 on either side of the origin)
SAFE = 1e150       # all_pairs.hip: kOrderSafe (coordinates of the ordered copies are clamped there on the sparse rule)


def launch_positions(x):
    """The positions K1 reads in an ordered launch on the sparse rule: every coordinate clamped to +-SAFE, NaN kept."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(x > SAFE, SAFE, np.where(x < -SAFE, -SAFE, x))


def order_cell(x):
    """k1_order_cell: the cell number 0 .. 1023 of every coordinate; NaN and everything below -512 -> 0, everything >= 512 -> 1023."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        low = ~(x >= -HALF)
        high = x >= HALF
        inner = np.floor(np.where(low | high, 0.0, x)).astype(np.int64) + HALF
    return np.where(low, 0, np.where(high, 2 * HALF - 1, inner)).astype(np.uint64)


def order_key(x):
    """k1_order_key: bit b of axis k's cell number at bit 3 b + k (30-bit Morton; the third axis is absent in 2D)."""
    q = order_cell(x)
    key = np.zeros(len(q), np.uint64)
    for k in range(q.shape[1]):
        for b in range(10):
            key |= ((q[:, k] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + k)
    return key


def space_order(x):
    """The permutation of an ordered launch: bodies by (key, index)."""
    return np.argsort(order_key(x), kind="stable")


def auto_chunks(n):
    """ap_auto_chunks -> (chunks, tiles per chunk)."""
    ntiles = (n + TILE - 1) // TILE
    y = 16
    while y < 64 and y * 65536 < n:
        y *= 2
    y = min(y, ntiles) or 1
    tpc = (ntiles + y - 1) // y if ntiles else 1
    return ((ntiles + tpc - 1) // tpc if ntiles else 1), tpc


def chunk_boxes(src, chunks, tpc):
    """Boxes over the padded records in the order given (padding at the origin; the whole line if a record is not finite)."""
    n, d = src.shape
    ntiles = (n + TILE - 1) // TILE
    xp = np.zeros((ntiles * TILE, d))
    xp[:n] = src
    lo, hi = np.empty((chunks, d)), np.empty((chunks, d))
    for c in range(chunks):
        rec = xp[c * tpc * TILE:(c + 1) * tpc * TILE]
        ok = np.isfinite(rec).all()
        lo[c] = rec.min(axis=0) if ok else -np.inf
        hi[c] = rec.max(axis=0) if ok else np.inf
    return lo, hi


def certified(src, tgt, r, chunks=None, tpc=None):
    """-> (certified blocks, all blocks, boolean matrix [group, chunk]) for sources `src` and targets `tgt` in launch order; target
    groups of 64 r lanes, lanes past the end hold target 0, gaps formed as the kernel forms them."""
    if chunks is None:
        chunks, tpc = auto_chunks(len(src))
    lo, hi = chunk_boxes(src, chunks, tpc)
    g = 64 * r
    count = len(tgt)
    groups = (count + g - 1) // g
    idx = np.arange(groups * g)
    t = tgt[np.where(idx < count, idx, 0)].reshape(groups, g, -1)
    tmin, tmax = t.min(axis=1), t.max(axis=1)
    finite = np.isfinite(t).all(axis=(1, 2))
    with np.errstate(invalid="ignore"):
        above = tmin[:, None, :] - hi[None, :, :]
        below = lo[None, :, :] - tmax[:, None, :]
        far = (((above >= GAP) & np.isfinite(above)) | ((below >= GAP) & np.isfinite(below))).any(axis=2)
    far &= finite[:, None]
    return int(far.sum()), groups * chunks, far


def mixed_rate(src, tgt, r, far, tpc, sample, seed=0):
    """Share of the batches (64 lanes x r targets x 2 sources) of blocks that did NOT certify in which some pair has r2 < 4,
    estimated from `sample` such blocks and 4096 sources of each."""
    rng = np.random.default_rng(seed)
    open_blocks = np.argwhere(~far)
    if len(open_blocks) == 0:
        return float("nan")
    pick = open_blocks[rng.choice(len(open_blocks), min(sample, len(open_blocks)), replace=False)]
    g = 64 * r
    mixed = total = 0
    for grp, c in pick:
        t = tgt[grp * g:(grp + 1) * g]
        s0 = c * tpc * TILE
        s = src[s0:min(len(src), s0 + tpc * TILE)]
        s = s[:len(s) // 2 * 2][:4096]
        if len(t) == 0 or len(s) == 0:
            continue
        r2 = ((t[:, None, :] - s[None, :, :]) ** 2).sum(axis=2)
        near = (r2 < 4.0).any(axis=0).reshape(-1, 2).any(axis=1)
        mixed += int(near.sum())
        total += len(near)
    return mixed / total if total else float("nan")


def load_package():
    name = "stdpar_nbody_amd"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "stdpar-nbody_amd", "__init__.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def report(x, r, sample):
    """-> {order: (certified share, mixed rate)} for the natural and the space order of a whole-system launch."""
    chunks, tpc = auto_chunks(len(x))
    out = {}
    for name, perm in (("natural", np.arange(len(x))), ("space", space_order(x))):
        xs = launch_positions(x[perm]) if name == "space" else x[perm]
        cert, blocks, far = certified(xs, xs, r, chunks, tpc)
        out[name] = (cert / blocks, mixed_rate(xs, xs, r, far, tpc, sample))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--workload", default="galaxy")
    ap.add_argument("--dim", type=int, default=3)
    ap.add_argument("--r", type=int, default=2, help="targets per lane")
    ap.add_argument("--mixed-sample", type=int, default=200)
    args = ap.parse_args()
    nb = load_package()
    hs = nb.build_model(nb.F64, args.dim, args.workload, args.n)
    x = np.array(hs.x, np.float64).reshape(hs.n, args.dim)
    chunks, tpc = auto_chunks(len(x))
    print(f"{args.workload} n={len(x)} D={args.dim} R={args.r}: {chunks} chunks of {tpc * TILE} sources; "
          f"extent {x.min(axis=0)} .. {x.max(axis=0)}")
    for name, (share, mixed) in report(x, args.r, args.mixed_sample).items():
        print(f"  {name:8s} order: certified share {share:.4f}, mixed batches in the rest {mixed:.4f}")


if __name__ == "__main__":
    main()
