"""GPU: the Hermite integrators (orders 4 and 6, block time steps) give the bits recorded in tests/golden/hermite_bits.json, hash for
hash.  The fixture was made once from the code before the two orders shared csrc/hermite_tile.hpp (inputs, sizes and what is recorded:
tests/golden/generate_hermite_bits.py, whose run_case this test calls); the rounding order of these kernels is a function of sz alone,
so any difference is a changed operation, contraction or summation order in the code under test.  Every recorded case is compared."""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("generate_hermite_bits", os.path.join(GOLDEN, "generate_hermite_bits.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(os.path.join(GOLDEN, "hermite_bits.json")))


def test_every_recorded_case_is_run(recorded):
    assert sorted(recorded) == sorted(gen.case_key(*c) for c in gen.CASES)
    assert sorted(k for k, r in recorded.items() if "block" in r) == sorted(gen.case_key(*c) for c in gen.CASES if c[2] in gen.BLOCK_SIZES)


@pytest.mark.parametrize("dtype,dim,n", gen.CASES, ids=[gen.case_key(*c) for c in gen.CASES])
def test_bits_are_the_recorded_ones(nb, recorded, dtype, dim, n):
    want = recorded[gen.case_key(dtype, dim, n)]
    got = gen.run_case(nb, dtype, dim, n)
    assert sorted(got) == sorted(want)
    for part in want:
        for stage in want[part]:
            assert got[part][stage] == want[part][stage], (part, stage, [k for k in want[part][stage] if stage != "counts" and
                                                                         got[part][stage][k] != want[part][stage][k]])
