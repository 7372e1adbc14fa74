"""GPU: nbody_neighbours_* and nbody_knn_* give the bits recorded in tests/golden/pair_sweep_bits.json, hash for hash.  The fixture was
made once from the code before the two files shared csrc/pair_sweep.hpp (inputs, sizes and what is recorded:
tests/golden/generate_pair_sweep_bits.py, whose run_case this test calls); the results are a function of the input and sz alone, so
any difference is a changed operation, contraction, merge order or index bound in the code under test.  Every recorded case is
compared."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("generate_pair_sweep_bits", os.path.join(GOLDEN, "generate_pair_sweep_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(GOLDEN, "pair_sweep_bits.json")))


def test_every_recorded_case_is_run(recorded):
    assert sorted(recorded) == sorted(gen.case_key(*c) for c in gen.CASES)
    assert len(set(gen.CASES)) == len(gen.CASES)


@pytest.mark.parametrize("kind,dtype,dim,n,k", gen.CASES, ids=[gen.case_key(*c) for c in gen.CASES])
def test_bits_are_the_recorded_ones(nb, recorded, kind, dtype, dim, n, k):
    want = recorded[gen.case_key(kind, dtype, dim, n, k)]
    got = gen.run_case(nb, kind, dtype, dim, n, k)
    assert sorted(got) == sorted(want)
    assert got == want, [name for name in want if got[name] != want[name]]
