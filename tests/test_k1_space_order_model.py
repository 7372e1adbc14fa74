"""CPU: K1's space order (csrc/k1_order_key.hpp, csrc/all_pairs.hip) on the flagship system, restated in NumPy
(tools/k1_order_model.py: the committed key, the stable order by (key, index), the chunk boxes and k1_block_is_far).

The order exists to make blocks certify: with the bodies of a disc in random order only the blocks that set one disc against
the other do (half of them).  The bound asked of the committed key is a certified share of at least 0.78 on the 2^20-body galaxy
of the host generator — the weakest key that was acceptable when the order was proposed (30-bit Morton on cells of side 1: 0.802),
less rounding.  The key's own edge cases are checked by the stand-alone program tools/k1_order_key_check.cpp, which this module
builds with the host compiler and the address and undefined-behaviour sanitizers, runs, and holds to the NumPy restatement."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

N = 1 << 20
MIN_SHARE = 0.78


@pytest.fixture(scope="module")
def model():
    spec = importlib.util.spec_from_file_location("k1_order_model", os.path.join(ROOT, "tools", "k1_order_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_key_restatement_on_boundaries(model):
    """Cell edges, +-0, clamping at both ends, NaN and the infinities: a defined cell each, and a total order."""
    x = np.array([-0.0, 0.0, 1.0, np.nextafter(1.0, 0.0), -1.0, np.nextafter(-1.0, -np.inf), -512.0, np.nextafter(-512.0, -np.inf),
                  np.nextafter(512.0, 0.0), 512.0, 1e6, -1e300, np.inf, -np.inf, np.nan])
    want = [512, 512, 513, 512, 511, 510, 0, 0, 1023, 1023, 1023, 0, 1023, 0, 0]
    assert model.order_cell(x).tolist() == want
    p = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-512.0, -512.0, -512.0], [600.0, 600.0, 600.0]])
    k = model.order_key(p)
    base = int(model.order_key(np.zeros((1, 3)))[0])
    assert base == 1 << 27 | 1 << 28 | 1 << 29                         # cell 512 on every axis: bit 9 of each
    assert [int(v) ^ base for v in k[:3]] == [1, 2, 4]                 # bit 0 of axis k at bit k
    assert int(k[3]) == 0 and int(k[4]) == (1 << 30) - 1
    assert int(model.order_key(np.array([[3.0, -7.0]]))[0]) < 1 << 29  # 2D: the third axis' bits stay 0
    assert int(model.order_key(np.array([[3.0, -7.0]]))[0]) & 0x24924924 == 0


def test_host_program_under_sanitizers(model, tmp_path):
    """tools/k1_order_key_check.cpp: the committed key function itself, compiled for the host with -fsanitize=address,undefined,
    checks its boundary cases and prints the key of every probe; the NumPy restatement must give the same keys."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "k1_order_key_check"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "stdpar-nbody_amd", "csrc"), os.path.join(ROOT, "tools", "k1_order_key_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = [line.split() for line in out.splitlines() if line.startswith("key ")]
    assert len(rows) >= 100 and out.rstrip().endswith("ok")
    for dim in (2, 3):
        sel = [r for r in rows if int(r[1]) == dim]
        p = np.array([[float.fromhex(v) if v not in ("nan", "inf", "-inf") else float(v) for v in r[2:2 + dim]] for r in sel])
        got = np.array([int(r[2 + dim], 16) for r in sel], np.uint64)
        assert np.array_equal(model.order_key(p), got), dim


def test_space_order_certifies_the_flagship(nb, model):
    """The 2^20-body galaxy of the host generator, whole-system launch, R = 2, 16 chunks."""
    hs = nb.build_model(nb.F64, 3, "galaxy", N)
    assert hs.n == N
    x = np.array(hs.x, np.float64).reshape(N, 3)
    got = model.report(x, 2, 100)
    for name, (share, mixed) in got.items():
        print(f"{name} order: certified share {share:.4f}, mixed batches in the rest {mixed:.4f}")
    perm = model.space_order(x)
    assert np.array_equal(np.sort(perm), np.arange(N))
    key = model.order_key(x)
    assert (np.diff(key[perm].astype(np.int64)) >= 0).all()
    same = np.diff(key[perm].astype(np.int64)) == 0
    assert (np.diff(perm)[same] > 0).all()                              # equal keys keep their index order
    assert abs(got["natural"][0] - 0.5) < 0.01                          # one disc against the other, nothing else
    assert got["space"][0] >= MIN_SHARE
