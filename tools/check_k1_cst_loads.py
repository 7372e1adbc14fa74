#!/usr/bin/env python3
"""Static check of the constant loads of K1's f64 scalar stream in the shipped gfx950 code object.

The loop of all_pairs_force_sgpr_kernel<double, ...> and of its softened twin requests, beside every batch of records, the
batch's pair constants (csrc/common.hpp: cload / cswait): M15 with a wave-uniform `global_load_dwordx4 v[..], vZ, s[base]` and
M1875 with the `s_load_dwordx4 s[..], s[base], 0x10` that follows it, both in inline asm, one compute phase ahead of the
`s_waitcnt vmcnt(0) lgkmcnt(0)` that completes them.  hipcc does not know that the asm's results are still in flight: nothing but
the register allocator's cooperation keeps other instructions off them until that wait.  This tool propagates the in-flight
register ranges along the control-flow graph of every such kernel (union at joins; a wait on vmcnt(0) clears the VGPRs, one on
lgkmcnt(0) the SGPRs) and reports
  * any instruction that reads or writes a range in flight,
  * a request still in flight at s_endpgm,
  * a vector-memory wait inside the source loop other than the pipeline's own (a stray `s_waitcnt vmcnt(n)` between a request and
    the batch's wait would stall every trip on the constants just requested),
and counts, per kernel, the requests it saw (none = the loop is not what this file describes).

    python tools/check_k1_cst_loads.py [path/to/libnbody_hip.so]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_smem_pipeline import disassemble, functions  # noqa: E402

KERNELS = ("all_pairs_force_sgpr_kernelId", "all_pairs_softened_sgpr_kernelId")  # mangled: the <double, ...> instantiations
VLOAD = re.compile(r"global_load_dwordx4 v\[(\d+):(\d+)\], v\d+, s\[(\d+):(\d+)\]\s*$")
SLOAD = re.compile(r"s_load_dwordx4 s\[(\d+):(\d+)\], s\[(\d+):(\d+)\], 0x10\s*$")


def regs_named(ins):
    out = []
    body = ins.split(None, 1)[1] if " " in ins else ""
    for f, a, b in re.findall(r"\b([vs])\[(\d+):(\d+)\]", body):
        out.append((f, int(a), int(b)))
    for f, a in re.findall(r"\b([vs])(\d+)\b", body):
        out.append((f, int(a), int(a)))
    return out


def check_function(name, code, inflight_at=None):
    """-> (requests seen, problems); with inflight_at = i: whether some path reaches instruction i with a request in flight"""
    index = {addr: i for i, (addr, _, _) in enumerate(code)}
    state = [None] * len(code)
    state[0] = frozenset()
    work, problems, requests = [0], [], 0
    while work:
        i = work.pop()
        addr, ins, target = code[i]
        out = state[i]
        m = VLOAD.match(ins)
        if m:
            out = out | {("v", int(m.group(1)), int(m.group(2)))}
        m = SLOAD.match(ins)
        if m and i > 0 and VLOAD.match(code[i - 1][1]) and VLOAD.match(code[i - 1][1]).group(3) == m.group(3):
            out = out | {("s", int(m.group(1)), int(m.group(2)))}
        if ins.startswith("s_waitcnt"):
            if "vmcnt(0)" in ins:
                out = frozenset(r for r in out if r[0] != "v")
            if "lgkmcnt(0)" in ins:
                out = frozenset(r for r in out if r[0] != "s")
        succ = []
        if not ins.startswith(("s_endpgm", "s_branch")) and i + 1 < len(code):
            succ.append(i + 1)
        if target is not None and target in index:
            succ.append(index[target])
        for j in succ:
            new = out if state[j] is None else state[j] | out
            if new != state[j]:
                state[j] = new
                work.append(j)
    if inflight_at is not None:
        return bool(state[inflight_at])
    for i, (addr, ins, _) in enumerate(code):
        if state[i] is None:
            continue
        if VLOAD.match(ins):
            requests += 1
        if ins.startswith("s_endpgm"):
            for f, lo, hi in state[i]:
                problems.append(f"{name} @{addr:x}: {f}[{lo}:{hi}] still in flight at s_endpgm")
        if ins.startswith("s_waitcnt") and "vmcnt" in ins and any(f == "v" for f, _, _ in state[i]) and "vmcnt(0)" not in ins:
            problems.append(f"{name} @{addr:x}: `{ins}` while the constants are in flight")
        if ins.startswith("s_waitcnt") and "vmcnt(0)" in ins and "lgkmcnt(0)" not in ins and any(f == "v" for f, _, _ in state[i]):
            problems.append(f"{name} @{addr:x}: a wait on vmcnt(0) that is not the pipeline's own, while the constants are in flight")
        for f, lo, hi in state[i]:
            for g, a, b in regs_named(ins):
                if g == f and not (b < lo or a > hi):
                    problems.append(f"{name} @{addr:x}: in-flight {f}[{lo}:{hi}] touched by `{ins}`")
    return requests, problems


def check(lib_path):
    """({kernel: requests}, problems)"""
    seen, problems = {}, []
    for name, code in functions(disassemble(lib_path)).items():
        if not code or not any(k in name for k in KERNELS):
            continue
        n, p = check_function(name, code)
        seen[name] = n
        if n == 0:
            p.append(f"{name}: no request for pair constants found")
        problems += p
    return seen, problems


def self_test(lib_path):
    """Each wait that some path reaches with a request in flight is replaced by a no-op in turn: -> (waits tried, removals NOT
    reported)."""
    tried = missed = 0
    for name, code in functions(disassemble(lib_path)).items():
        if not code or not any(k in name for k in KERNELS):
            continue
        for i, (addr, ins, _) in enumerate(code):
            if ins.startswith("s_waitcnt") and "vmcnt(0)" in ins and "lgkmcnt(0)" in ins and check_function(name, code, i):
                tried += 1
                if not check_function(name, code[:i] + [(addr, "s_nop 0", None)] + code[i + 1:])[1]:
                    missed += 1
    return tried, missed


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "stdpar-nbody_amd", "libnbody_hip.so")
    seen, bad = check(lib)
    for b in bad:
        print(b)
    print(f"{len(seen)} f64 scalar-stream kernels, {sum(seen.values())} requests for pair constants, {len(bad)} violation(s)")
    tried, missed = self_test(lib)
    print(f"self-test: {tried} pipeline waits removed in turn, {missed} removal(s) not reported")
    sys.exit(1 if bad or not seen or missed or not tried else 0)
