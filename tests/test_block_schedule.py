"""CPU: the kernels of csrc/block_schedule.hpp and csrc/hermite_block_common.hpp in the built code objects.  They are static kernels of a
header, so every translation unit that includes it carries a copy under the same symbol: the four schedule kernels are in three code
objects (hermite.hip, hermite6.hip, octree.hip), the Hermite start-level and chunk-sum kernels in two.  tools/check_smem_pipeline.functions
keys by symbol name and would show one copy of each; here the disassembly is cut per code object, and every copy is held to the same
rules: the copies are the same instruction text, none uses scratch, and the only atomic is the unsigned minimum of tau_next."""
import importlib.util
import os
import re

import pytest

from conftest import ROOT

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
SCHED = ("block_sched_min_kernel", "block_sched_count_kernel", "block_sched_scan_kernel", "block_sched_compact_kernel")
HERMITE = ("hermite_block_init_kernel", "hermite_block_reduce_kernel")


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_block_schedule", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def code_objects(nb):
    """One {symbol: [instruction text]} per code object of the library that holds a kernel of the two headers."""
    if not os.path.exists(OBJDUMP):
        pytest.skip("llvm-objdump not available")
    sp = _tool("check_smem_pipeline")
    chunks = re.split(r"^.*file format.*$", sp.disassemble(nb.LIB_PATH), flags=re.M)[1:]
    assert len(chunks) >= 3, len(chunks)
    out = []
    for chunk in chunks:
        funcs = {n: [ins for _, ins, _ in c] for n, c in sp.functions(chunk).items() if c and any(k in n for k in SCHED + HERMITE)}
        if funcs:
            out.append(funcs)
    return out


def _copies(code_objects, kernel):
    """[{symbol: text} of the symbols that contain `kernel`] for every code object that has one"""
    found = [{n: t for n, t in co.items() if kernel in n} for co in code_objects]
    return [f for f in found if f]


def test_schedule_kernels_are_in_three_code_objects_with_the_same_text(code_objects):
    for kernel in SCHED:
        copies = _copies(code_objects, kernel)
        assert len(copies) == 3, (kernel, len(copies))
        assert all(len(c) == 1 for c in copies), (kernel, [sorted(c) for c in copies])  # not templates: one symbol each
        first = copies[0]
        assert next(iter(first.values())), kernel
        assert all(c == first for c in copies[1:]), kernel  # the same symbol, the same instructions in the same order


def test_hermite_start_and_chunk_sum_kernels_are_in_two_code_objects(code_objects):
    """hermite.hip has them in float and double, hermite6.hip in double alone (its block steps are refused in float); what both have is
    the same text."""
    for kernel, n4, n6 in (("hermite_block_init_kernel", 4, 2), ("hermite_block_reduce_kernel", 2, 1)):
        copies = sorted(_copies(code_objects, kernel), key=len)
        assert [len(c) for c in copies] == [n6, n4], (kernel, [sorted(c) for c in copies])
        six, four = copies
        assert all("kernelId" in n for n in six), sorted(six)  # <double, ...>: no float instance in the sixth order's code object
        for name, text in six.items():
            assert four[name] == text, name


def test_no_copy_spills_and_the_only_atomic_is_the_minimum(nb, code_objects):
    seen = 0
    for co in code_objects:
        for name, text in co.items():
            seen += 1
            assert not any("scratch_" in ins for ins in text), name
            atomics = [ins for ins in text if "atomic" in ins]
            if "block_sched_min_kernel" in name:
                assert atomics and all("atomic_umin" in a for a in atomics), (name, atomics)
            else:
                assert not atomics, (name, atomics)
    assert seen == 3 * len(SCHED) + (4 + 2) + (2 + 1), seen
    kr = _tool("kernel_resources")
    records = [k for k in kr.kernels(nb.LIB_PATH) if any(s in k["symbol"] for s in SCHED + HERMITE)]
    assert len(records) == seen, (len(records), seen)  # one record per copy: nothing is keyed by name here
    for k in records:
        assert int(k.get("private_segment_fixed_size", 0)) == 0, k
