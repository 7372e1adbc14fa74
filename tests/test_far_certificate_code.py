"""The built gfx950 code object of K1's scalar stream with the far certificate (no GPU needed): every f64 unsoftened kernel holds
a third copy of the source loop whose steady state has no near/far test — nothing that looks at r2 — and the arithmetic of an
all-far batch; the softened twins and the f32 kernels hold the loops they had."""
import importlib.util
import os
import re
import sys

from conftest import ROOT


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location(name + "_far_certificate", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _kernels(nb):
    sp = _tool("check_smem_pipeline")
    return {n: c for n, c in sp.functions(sp.disassemble(nb.LIB_PATH)).items()
            if c and re.search(r"all_pairs_(force|softened)_sgpr_kernelI[df]", n)}


def _blocks(code):
    targets = {t for _, _, t in code if t is not None}
    blocks, cur = [], []
    for addr, ins, _ in code:
        if addr in targets and cur:
            blocks.append(cur)
            cur = []
        cur.append(ins)
        if ins.startswith(("s_branch", "s_cbranch", "s_endpgm")):
            blocks.append(cur)
            cur = []
    return blocks


def _stream_loops(code):
    """Copies of the source loop: each holds three requests for records (s_load_dwordx16) — one ahead of the loop, two inside."""
    requests = sum(ins.startswith("s_load_dwordx16") for _, ins, _ in code)
    assert requests % 3 == 0, requests
    return requests // 3


def test_certified_copy_has_no_test_and_the_far_arithmetic(nb):
    funcs = {n: c for n, c in _kernels(nb).items() if "all_pairs_force_sgpr_kernelId" in n}
    assert len(funcs) == 16, sorted(funcs)  # 2 dims x R in {1, 2} x JS in {1, 2, 4, 8}
    for name, code in funcs.items():
        steady = [b for b in _blocks(code) if any(i.startswith("s_load_dwordx16") for i in b) and any(i.startswith("v_rsq_f64") for i in b)]
        free = [b for b in steady if not any(i.startswith(("v_min3_u32", "v_min_u32", "v_cmp")) for i in b)]
        assert len(free) == 1 and len(steady) == 3, (name, len(steady), len(free))  # the two rules' halves keep their test
        b = free[0]
        pairs = sum(i.startswith("v_rsq_f64") for i in b)
        assert pairs >= 4 and sum(i.startswith("v_mul_f64") for i in b) == 3 * pairs, (name, pairs)
        # 2 D + 7 full-rate operations beside the v_rsq_f64 of a pair (D differences, D for r2, 6 for the weight, D accumulations:
        # 3 D + 6), and nothing else on the VALU: no move, no select
        dim = int(re.search(r"kernelIdLi(\d)E", name).group(1))
        valu = [i for i in b if i.startswith("v_")]
        assert len(valu) == pairs * (3 * dim + 7), (name, len(valu), pairs)
        assert all(i.startswith(("v_add_f64", "v_fma_f64", "v_fmac_f64", "v_mul_f64", "v_rsq_f64")) for i in valu), (name, valu)


def test_other_kernels_hold_the_loops_they_had(nb):
    funcs = _kernels(nb)
    assert len(funcs) == 64, len(funcs)
    for name, code in funcs.items():
        want = 1 if "softened" in name else 3 if "all_pairs_force_sgpr_kernelId" in name else 2
        assert _stream_loops(code) == want, (name, _stream_loops(code))
