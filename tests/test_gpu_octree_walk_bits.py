"""GPU: the six compiler-scheduled octree walks give the bits recorded in tests/golden/octree_walk_bits.json, hash for hash.  The
fixture was made once from the code while the walk was a text pasted into six kernels (inputs, sizes and what is recorded:
tests/golden/generate_octree_walk_bits.py, whose run_case this test calls); a body's result depends on nothing but the tree and that
body, so any difference is a changed operation, contraction, order of the 2^D partial sums, index or bound in the walk under test.
Every recorded case is compared."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("generate_octree_walk_bits", os.path.join(GOLDEN, "generate_octree_walk_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(GOLDEN, "octree_walk_bits.json")))


def test_every_recorded_case_is_run(recorded):
    assert sorted(recorded) == sorted(gen.case_key(*c) for c in gen.CASES)
    assert len(set(gen.CASES)) == len(gen.CASES)


@pytest.mark.parametrize("dtype,dim,n,theta,first,count", gen.CASES, ids=[gen.case_key(*c) for c in gen.CASES])
def test_bits_are_the_recorded_ones(nb, recorded, dtype, dim, n, theta, first, count):
    want = gen.expand(recorded[gen.case_key(dtype, dim, n, theta, first, count)])
    got = gen.run_case(nb, dtype, dim, n, theta, first, count)
    assert sorted(got) == sorted(want)
    assert got == want, [name for name in want if got[name] != want[name]]
