"""The built gfx950 code object of K1's f64 scalar stream with the folded pair form (no GPU needed): the constant loads are
pipelined and nothing touches their registers in flight (tools/check_k1_cst_loads.py, with its self-test), and the far-pair code
holds three v_mul_f64 per pair — a = y y, y3 = a y, w = y3 s; the form it replaces had four — with no v_mov for the constants."""
import importlib.util
import os
import re
import sys

from conftest import ROOT


def _tool(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location(name + "_k1_folded", os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_constant_loads_are_pipelined_and_left_alone(nb):
    mod = _tool("check_k1_cst_loads")
    seen, problems = mod.check(nb.LIB_PATH)
    assert not problems, "\n".join(problems[:10])
    # 2 dims x R in {1, 2} x JS in {1, 2, 4, 8}, both twins; the prologue's request and two per loop copy in each
    assert len(seen) == 32 and all(n >= 3 for n in seen.values()), seen
    tried, missed = mod.self_test(nb.LIB_PATH)
    assert tried >= 3 * len(seen) and missed == 0, (tried, missed)


def test_far_pair_code_has_three_multiplies_per_pair_and_no_moves(nb):
    sp = _tool("check_smem_pipeline")
    funcs = {n: c for n, c in sp.functions(sp.disassemble(nb.LIB_PATH)).items()
             if c and re.search(r"all_pairs_(force|softened)_sgpr_kernelId", n)}
    assert len(funcs) == 32, sorted(funcs)
    for name, code in funcs.items():
        targets = {t for _, _, t in code if t is not None}
        blocks, cur = [], []
        for addr, ins, target in code:
            if addr in targets and cur:
                blocks.append(cur)
                cur = []
            cur.append(ins)
            if ins.startswith(("s_branch", "s_cbranch", "s_endpgm")):
                blocks.append(cur)
                cur = []
        far = [b for b in blocks if any(i.startswith("v_rsq_f64") for i in b)
               and not any(i.startswith(("v_rcp_f64", "v_cndmask", "v_cmp_gt_u32_e64", "v_cmp_lt_u32_e64")) for i in b)]
        assert far, name
        for b in far:
            pairs = sum(i.startswith("v_rsq_f64") for i in b)
            assert sum(i.startswith("v_mul_f64") for i in b) == 3 * pairs, (name, pairs, b)
            if any(i.startswith("s_load_dwordx16") for i in b) or pairs >= 2:   # a block of the steady-state loop
                assert not any(re.match(r"v_mov_b(32|64)", i) for i in b), (name, [i for i in b if i.startswith("v_mov")])


def test_flagship_kernel_keeps_its_waves_and_spills_nothing(nb):
    kr = _tool("kernel_resources")
    ks = kr.kernels(nb.LIB_PATH)
    names = kr.demangle([k["symbol"].replace(".kd", "") for k in ks])
    seen = 0
    for k, n in zip(ks, names):
        if "all_pairs_force_sgpr_kernel<double, 3, 2, 8, 0>" in n:
            seen += 1
            v = (int(k["vgpr_count"]) + int(k.get("agpr_count", 0)) + 7) // 8 * 8
            assert v <= 128 and int(k["sgpr_count"]) <= 184, (v, k["sgpr_count"])    # 4 waves per SIMD, as before
            assert int(k.get("private_segment_fixed_size", 0)) == 0
    assert seen == 1
