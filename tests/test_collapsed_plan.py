"""K2's launch plan (csrc/all_pairs.hip: k2_plan, plan_collapsed) through nbody_all_pairs_collapsed_describe, on the CPU: the call is
host arithmetic on a hand-built state and needs no GPU.  The invariants every launch shape must keep, the shapes of four sizes
as literals worked out by hand from the formulas, the sizes at which the cross-trip and the several-tiles-per-block machinery
first run, and what the experiments build's two switches select.  tests/test_gpu_collapsed_wide.py asserts these lines before it
launches, so that a test means the shape it names."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

F32, F64 = 0, 1
SWEEP = list(range(1, 5001)) + list(range(5000 + 257, 300001, 257)) + [1 << 20]


def describe(L, dtype, dim, n, first=0, count=None):
    st = _state(dtype, dim, n, first, count)
    buf = ctypes.create_string_buffer(256)
    rc = L.nbody_all_pairs_collapsed_describe(ctypes.byref(st), buf, ctypes.c_size_t(256))
    assert rc == 0, (rc, L.nbody_last_error())
    return buf.value.decode()


_NB = []


def _state(dtype, dim, n, first=0, count=None):
    st = _NB[0].nbody_state()
    st.dtype, st.dim, st.sz, st.first, st.count = dtype, dim, n, first, n if count is None else count
    st.m = st.x = st.v = st.a = st.ao = 0x1000  # never dereferenced: describe is host arithmetic
    return st


def fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line)}


@pytest.fixture(scope="module")
def L(nb):
    _NB[:] = [nb]
    lib = nb.lib()
    lib.nbody_last_error.restype = ctypes.c_char_p
    return lib


def test_describe_runs_on_a_hand_built_state_without_a_gpu(nb, L):
    """No stream, no GPU work; the lines of include/nbody_hip.h word for word; K2 is single-GPU, so a shard window is refused as
    the force call refuses it; the wrapper of the binding returns the same line."""
    assert describe(L, F32, 3, 33001) == "all_pairs_collapsed_stream_kernel<8> hand float 3 padded=33792 nbatches=66 bpc=4 chunks=17"
    assert describe(L, F64, 3, 33001) == "all_pairs_collapsed_kernel<double,3,NT=8,KS=8,NB=1> tile=1024 iblocks=129 ntiles=33 tpb=2 ysplit=17"
    assert describe(L, F32, 2, 33001) == ("all_pairs_collapsed_stream_cxx_kernel<float,2,4> compiled float 2 padded=33280 nbatches=130 "
                                          "bpc=6 chunks=22")
    assert describe(L, F64, 2, 2049).startswith("all_pairs_collapsed_kernel<double,2,NT=8,KS=8,NB=1> tile=1024 ")
    assert nb.describe_all_pairs_collapsed(_state(F64, 3, 33001)) == describe(L, F64, 3, 33001)
    assert "no launch" in describe(L, F32, 3, 0)
    buf = ctypes.create_string_buffer(256)
    st = _state(F64, 3, 1000, 100, 200)
    assert L.nbody_all_pairs_collapsed_describe(ctypes.byref(st), buf, ctypes.c_size_t(256)) == 1
    assert b"single-GPU" in L.nbody_last_error()
    st = _state(F64, 3, 1000)
    assert L.nbody_all_pairs_collapsed_describe(ctypes.byref(st), None, ctypes.c_size_t(256)) == 1
    st.tuning = 0xdeadbeef
    assert L.nbody_all_pairs_collapsed_describe(ctypes.byref(st), buf, ctypes.c_size_t(256)) == 1
    assert L.nbody_abi_version() == 2004  # additive: the version stays


@pytest.mark.parametrize("dim", [3, 2])
def test_streamed_form_invariants(L, dim):
    """Float.  The kernel takes two batches per trip and reads batch b1 - 1 at the latest: the record array is whole pairs of
    batches and covers every body, a chunk is an even number of batches, the chunks cover the batches with none empty (the last
    may be short, by whole pairs), and grid.y fits."""
    ks = 8 if dim == 3 else 4
    for n in SWEEP:
        line = describe(L, F32, dim, n)
        assert line.startswith("all_pairs_collapsed_stream_kernel<8> hand float 3 " if dim == 3 else
                               "all_pairs_collapsed_stream_cxx_kernel<float,2,4> compiled float 2 "), (n, line)
        f = fields(line)
        assert f["padded"] % (2 * 64 * ks) == 0 and f["padded"] >= n, (n, line)
        assert f["padded"] - n < 2 * 64 * ks, (n, line)                       # no more padding than the pair of batches asks
        assert f["nbatches"] * 64 * ks == f["padded"], (n, line)
        assert f["bpc"] % 2 == 0 and f["bpc"] >= 2, (n, line)
        assert (f["chunks"] - 1) * f["bpc"] < f["nbatches"] <= f["chunks"] * f["bpc"], (n, line)
        assert 1 <= f["chunks"] <= 65535, (n, line)


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [F64])
def test_tile_form_invariants(L, dtype, dim):
    """Double.  Block rows of tpb tiles cover the tiles with no row empty; grid.y fits; blocks of 256 targets cover the bodies."""
    for n in SWEEP:
        line = describe(L, dtype, dim, n)
        assert line.startswith(f"all_pairs_collapsed_kernel<double,{dim},NT=8,KS=8,NB=1> tile=1024 "), (n, line)
        f = fields(line)
        assert f["ntiles"] == (n + 1023) // 1024 and f["iblocks"] == (n + 255) // 256, (n, line)
        assert f["tpb"] >= 1 and (f["ysplit"] - 1) * f["tpb"] < f["ntiles"] <= f["ysplit"] * f["tpb"], (n, line)
        assert 1 <= f["ysplit"] <= 65535, (n, line)


# Worked out by hand from the formulas of the commit before plan_collapsed existed (literals, not a copy of the arithmetic).
#   float 3D: ks 8, padded to 1024; chunks wanted ceil(65536 / ceil(n / 16)), at most nbatches; bpc = ceil(nbatches / chunks) made even
#   float 2D: ks 4, padded to 512
#   double:   iblocks ceil(n / 256), ntiles ceil(n / 1024), ysplit wanted ceil(4096 / iblocks), tpb = ceil(ntiles / ysplit)
PINNED = [
    (33001, F32, 3, dict(padded=33792, nbatches=66, bpc=4, chunks=17)),     # the last chunk holds 2 batches
    (33001, F32, 2, dict(padded=33280, nbatches=130, bpc=6, chunks=22)),    # the last chunk holds 4
    (33001, F64, 3, dict(iblocks=129, ntiles=33, tpb=2, ysplit=17)),        # the last block row holds 1 tile
    (33001, F64, 2, dict(iblocks=129, ntiles=33, tpb=2, ysplit=17)),
    (16385, F32, 3, dict(nbatches=34, bpc=2, chunks=17)),
    (16385, F32, 2, dict(nbatches=66, bpc=2, chunks=33)),
    (16385, F64, 3, dict(ntiles=17, tpb=1, ysplit=17)),
    (16385, F64, 2, dict(ntiles=17, tpb=1, ysplit=17)),
    (100000, F32, 3, dict(bpc=18, chunks=11)),
    (100000, F32, 2, dict(bpc=36, chunks=11)),
    (100000, F64, 3, dict(tpb=9, ysplit=11)),
    (100000, F64, 2, dict(tpb=9, ysplit=11)),
    (262144, F32, 3, dict(nbatches=512, bpc=128, chunks=4)),
    (262144, F32, 2, dict(nbatches=1024, bpc=256, chunks=4)),
    (262144, F64, 3, dict(tpb=64, ysplit=4)),
    (262144, F64, 2, dict(tpb=64, ysplit=4)),
]


@pytest.mark.parametrize("n, dtype, dim, want", PINNED, ids=[f"{n}-{'fd'[t]}{d}" for n, t, d, _ in PINNED])
def test_pinned_shapes(L, n, dtype, dim, want):
    f = fields(describe(L, dtype, dim, n))
    assert {k: f[k] for k in want} == want, (n, dtype, dim, f)


def _first(L, dtype, dim, key, above, stop=60000):
    for n in range(1, stop):
        if fields(describe(L, dtype, dim, n))[key] > above:
            return n
    return None


def test_onsets(L):
    """The smallest systems that run more than one trip per chunk (float: the bridge from trip to trip, the clamped prefetch) and
    more than one, more than two tiles per block (double): every size below them leaves that code unrun."""
    assert _first(L, F32, 3, "bpc", 2) == 32769
    assert _first(L, F32, 2, "bpc", 2) == 23297
    for dim in (3, 2):
        assert _first(L, F64, dim, "tpb", 1) == 32769
        assert _first(L, F64, dim, "tpb", 2) == 47105
        assert _first(L, F64, dim, "ysplit", 1) == 1025       # one partial sum per target up to 1024 bodies
    assert _first(L, F32, 3, "chunks", 1) == 1025
    assert _first(L, F32, 2, "chunks", 1) == 513


# ---- the experiments build: NBODY_K2_CFG / NBODY_K2_CHUNKS select what describe prints (and what the launch takes) ---------------
STREAM3 = {20: "all_pairs_collapsed_stream_kernel<8> hand float 3 ", 21: "all_pairs_collapsed_stream_kernel<4> hand float 3 ",
           22: "all_pairs_collapsed_stream_cxx_kernel<float,3,8> compiled float 3 ",
           23: "all_pairs_collapsed_stream_cxx_kernel<float,3,4> compiled float 3 ",
           24: "all_pairs_collapsed_stream_cxx_kernel<float,3,4> compiled float 3 "}  # 2 records per batch: below one pair_batch call in float
STREAM2 = {22: "all_pairs_collapsed_stream_cxx_kernel<float,2,8> compiled float 2 ",
           23: "all_pairs_collapsed_stream_cxx_kernel<float,2,4> compiled float 2 ",
           24: "all_pairs_collapsed_stream_cxx_kernel<float,2,4> compiled float 2 "}
TILE3 = {0: (16, 8, 0), 8: (16, 8, 1), 10: (16, 4, 0), 11: (8, 8, 0), 12: (8, 4, 0)}
TILE2 = {0: (16, 8, 1), 2: (8, 4, 1)}
TILE_DOUBLE = {0: (16, 8, 1), 1: (8, 4, 4), 2: (8, 4, 1), 4: (8, 4, 2), 5: (8, 8, 1), 6: (8, 2, 1), 7: (8, 2, 2)}


def tile_prefix(dtype, dim, shape):
    return "all_pairs_collapsed_kernel<%s,%d,NT=%d,KS=%d,NB=%d> tile=%d " % (("float", "double")[dtype], dim, *shape, (2048, 1024)[dtype])


def experiment_forms(dtype, dim):
    """[(NBODY_K2_CFG, NBODY_K2_CHUNKS or None, the start of the describe line)] of tests/test_gpu_collapsed_wide.py's form test."""
    if dtype == F64:
        return [(cfg, None, tile_prefix(F64, dim, s)) for cfg, s in TILE_DOUBLE.items()]
    stream, tile = (STREAM3, TILE3) if dim == 3 else (STREAM2, TILE2)
    out = [(cfg, ch, line) for cfg, line in stream.items() for ch in (None, 1, 3)]
    return out + [(cfg, None, tile_prefix(F32, dim, s)) for cfg, s in tile.items()]


class k2_switches:
    """NBODY_K2_CFG / NBODY_K2_CHUNKS for the experiments build's calls inside, restored on the way out."""

    def __init__(self, cfg=None, chunks=None):
        self.want = {"NBODY_K2_CFG": cfg, "NBODY_K2_CHUNKS": chunks}

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.want}
        for k, v in self.want.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.fixture(scope="module")
def LX(L):
    path = os.path.join(ROOT, "stdpar-nbody_amd", "libnbody_hip_exp.so")
    assert os.path.exists(path), "libnbody_hip_exp.so is not built (make -C stdpar-nbody_amd experiments)"
    lib = ctypes.CDLL(path)
    lib.nbody_last_error.restype = ctypes.c_char_p
    return lib


@pytest.mark.parametrize("dim", [3, 2])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_experiment_switches_select_the_described_form(L, LX, dtype, dim):
    """Every form of the GPU test at its 6000 bodies: the kernel named, the invariants kept, NBODY_K2_CHUNKS = 1 one chunk of every
    batch and 3 an odd count that the even-bpc rule rounds; without the switches the experiments build plans what ships; the
    shipped library ignores them."""
    n = 6000
    shipped = describe(L, dtype, dim, n)
    with k2_switches():
        assert describe(LX, dtype, dim, n) == shipped
    for cfg, chunks, prefix in experiment_forms(dtype, dim):
        with k2_switches(cfg, chunks):
            line = describe(LX, dtype, dim, n)
            assert describe(L, dtype, dim, n) == shipped
        assert line.startswith(prefix), (cfg, chunks, line)
        f = fields(line)
        if "stream" in prefix:
            ks = int(re.search(r"kernel<(?:float,\d,)?(\d)>", line).group(1))
            assert f["padded"] % (128 * ks) == 0 and 0 <= f["padded"] - n < 128 * ks and f["nbatches"] * 64 * ks == f["padded"], line
            assert f["bpc"] % 2 == 0 and (f["chunks"] - 1) * f["bpc"] < f["nbatches"] <= f["chunks"] * f["bpc"], line
            if chunks == 1:
                assert f["chunks"] == 1 and f["bpc"] == f["nbatches"], line
            if chunks == 3:   # ks 8: 12 batches, 4 per chunk; ks 4: 24 batches, 8 per chunk
                assert (f["nbatches"], f["bpc"], f["chunks"]) == ((12, 4, 3) if ks == 8 else (24, 8, 3)), line
        else:
            assert (f["ysplit"] - 1) * f["tpb"] < f["ntiles"] <= f["ysplit"] * f["tpb"] and f["iblocks"] == 24, line
    # a streamed form that this (type, dimension) does not have falls to the shipped tile shape, and says so
    with k2_switches(20):
        assert describe(LX, F64, dim, n).startswith(tile_prefix(F64, dim, (8, 8, 1)))
        assert describe(LX, F32, 2, n).startswith(tile_prefix(F32, 2, (16, 8, 1)))
    with k2_switches(9):
        assert describe(LX, dtype, dim, n).startswith(tile_prefix(dtype, dim, (16, 8, 4)))
