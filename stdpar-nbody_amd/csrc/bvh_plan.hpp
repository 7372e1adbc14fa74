// Launch plan of the BVH traversal (K9) and the host's account of the opening thresholds: host arithmetic only, no kernel and no HIP
// call, so that tools/bvh_plan_check.cpp can sweep its invariants and pin its shapes without a device.  force_run (bvh.hip) fills a
// k9_request, calls plan_bvh_force and launches what the k9_plan says.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/nbody_hip.h"

namespace nbody {

// ---- the sweep's work items (bvh_items_kernel) ----
constexpr uint32_t kOrderMax = 8192;  // groups per XCD range one block handles (N <= 4.2M bodies); more: plain index order
constexpr uint32_t kSplitMax = 2048;  // groups per XCD range that may be cut
__host__ __device__ __forceinline__ void xcd_range(uint32_t xcd, uint32_t nblocks, uint32_t* start, uint32_t* len) {
  const uint32_t q = nblocks / 8u, r = nblocks % 8u;
  *start = xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q;
  *len   = q + (xcd < r ? 1u : 0u);
}
__host__ __device__ __forceinline__ uint32_t split_budget(uint32_t len, uint32_t den = 16u) {
  const uint32_t b = len / den;
  return len > kOrderMax ? 0u : (b < kSplitMax ? b : kSplitMax);
}
// Words of the `order` buffer of a tree of n bodies: 8 lists of `stride` items.  A traversal of count <= n bodies has
// groups <= G = ceil(n / 64), its longest XCD range is l0 = ceil(groups / 8) <= G / 8 + 1 and split_budget(l0, den) <= l0 for every
// den >= 1, so 8 * stride <= 16 * (G / 8 + 1); the 64 words beyond are slack.  tools/bvh_plan_check.cpp holds every plan to it.
inline size_t k9_items_capacity(uint32_t n) { return (((size_t(n) + 63) / 64 / 8 + 1) * 2 + 8) * 8; }

// ---- the per-lane walk over a copy of the tree in LDS (bvh_force_lds_kernel) ----
constexpr int kTreeLdsThreads    = 256;
constexpr uint32_t kTreeLdsBytes = 144u << 10;  // of the CU's 160 KB
// Float trees whose nnodes + 2^nlevels records of 32 bytes fit (up to 2048 bodies): nbody_bvh_create raises the kernel's
// dynamic-LDS limit on this predicate and the plan chooses the form on it.
inline bool k9_lds_fits(int dtype, uint32_t nlevels) {
  return dtype == NBODY_F32 && ((uint64_t(2) << nlevels) - 1u) * 32u <= kTreeLdsBytes;
}

// ---- the plan ----
// What the -DNBODY_EXPERIMENTS build reads from the environment (k9_read_overrides, experiments/bvh_forms.inc); the shipped build
// leaves it as it stands.
struct k9_overrides {
  int mode           = 0;      // NBODY_K9_MODE: the traversal when the tree's own setting is 0 (auto)
  bool plain_order   = false;  // NBODY_K9_ORDER=0: one block per group in index order
  uint32_t parts     = 0;      // NBODY_K9_PARTS: 1, 2, 4, 8 or 16 lane ranges per group; 0: k9_parts
  uint32_t split_den = 16;     // NBODY_K9_SPLIT: one group in split_den is cut by bvh_items_kernel
  uint32_t lds_bytes = 0;      // NBODY_K9_LDS: dynamic LDS per sweep block, to cap the waves per SIMD
  bool timeline      = false;  // NBODY_K9_TIMELINE=1: the sweep records its items' start and end; no part of the plan
};
// Everything the decision depends on.  Neither the size of the system nor the counters are in it: the plan follows `count`, the
// bodies of this call, and the counting instantiation of a form is launched in the shape of the plain one.
struct k9_request {
  uint32_t elem = 8, nlevels = 0, nnodes = 0, count = 0;  // elem: sizeof(T)
  int traversal = 0, launch_order = 0;                    // nbody_bvh_set_traversal, nbody_bvh_set_launch_order
  bool sorted   = false;  // nbody_bvh_hilbert_sort has run ...
  int final_buf = 0;      // ... and ended in the buffer it started from: keys[1] holds the sorted keys
  k9_overrides overrides;
};
// bvh_force_kernel, bvh_force_lds_kernel, and the sweep: the step program written out as ISA (bvh_force_sweep_isa_kernel: auto, 2, 5).
// The -DNBODY_EXPERIMENTS build (experiments/bvh_forms.inc) also has the compiler-scheduled step (3; with 2 bodies per lane: 4 — 128
// bodies per wave, config 4 12.2 ms against 9.55) and the row sweeps (6).  All forms are bitwise identical.
enum class k9_form { lane_global, lane_lds, sweep, compiled_sweep, compiled_sweep_2, row_sweeps };
struct k9_plan {
  k9_form form  = k9_form::lane_global;
  uint32_t grid = 0, threads = 64, lds_bytes = 0;
  uint32_t groups = 0;      // blocks before any cutting: `threads` bodies each (twice that for compiled_sweep_2)
  uint32_t parts  = 1;      // sweep: every group as `parts` equal lane ranges side by side, grid = groups * parts
  bool items      = false;  // sweep: bvh_items_kernel lists the work items first, 8 lists of up to `stride`, grid = 8 * stride
  uint32_t stride = 0, split_den = 16;
};
constexpr const char* kK9LevelsRefusal = "wave-cooperative traversal needs nlevels <= 26 (n <= 2^26), tree has %u levels";
constexpr const char* kK9RowsRefusal   = "traversal mode 6 (row sweeps) has no counters and needs nlevels <= 26";

// auto: the wave-cooperative sweep needs enough waves in flight to hide its serial chain.  Measured in the CLI's step loop on
// 256 CUs (ms per whole bvh step over the first 200 steps of the galaxy, sweep / per-lane): f64 (hand-scheduled sweep) 0.90 / 0.85
// at 4*10^4, 1.0 / 1.0 at 6*10^4, 1.1 / 1.15 at 8*10^4, 1.2 / 1.25 at 10^5, 1.3 / 1.5 at 1.3*10^5, 2.05 / 3.45 at 2.5*10^5, 3.45 / 7.1
// at 5*10^5; f32 0.90 / 0.65 at 6*10^4, 1.05 / 0.80 at 10^5, 1.25 / 1.15 at 1.6*10^5, 1.5 / 1.9 at 2.5*10^5, 4.45 / 10.6 at 10^6.  A system that has
// evolved favours the sweep further: escapers inflate the box, walks get 3x longer and the per-lane form's divergent
// gathers pay for every entry (10^5 bodies after 400-1000 steps: sweep 1.7-2.1 ms, per-lane 3.0-3.7 ms per traversal).
// f64 below 5*10^4: the first steps of the galaxy favour the per-lane form by 7 % (4*10^4) to 20 % (10^4), its evolved states the
// sweep by 25-40 % (whole 1000-step runs, sweep / per-lane: 0.86 / 0.91 s at 10^4, 0.99 / 1.07 at 2*10^4, 1.16 / 1.47 at 3*10^4)
// f64 with the finer work items of small systems (k9_parts): the sweep wins from the smallest sizes measured (10^4: 0.27 against 0.33 ms)
inline uint32_t k9_crossover(uint32_t elem) { return elem == 8 ? 4096u : 180000u; }

// Finer work items (profiles/r03/k9_parts.txt, ms per traversal of the initial galaxy, f64): every group swept as `parts` equal
// lane ranges side by side has shorter unions (16 Hilbert-adjacent walks: 5.7k steps against 7.4k for 64 at config 4) but
// more of them.  That pays only while the chip is nearly empty — N = 10^4: 0.40 (1 part) / 0.36 (4) / 0.27 (8), per-lane form
// 0.33; N = 3*10^4: 0.64 / 0.56 / 0.56, per-lane 0.58 — and costs from 6*10^4 bodies on (10^5: 1.06 / 1.62 / 1.86; 10^6: 6.96 /
// 16.6 / 28.2).  The key-jump cutter behaves the same way at N = 10^6: 1/16 of the groups cut 6.97 ms, 1/8 7.11, 1/4 7.39,
// 1/2 7.84, all 10.3 — the filling and draining of a launch cannot be bought back with more, shorter items.
inline uint32_t k9_parts(uint32_t groups) { return groups <= 320u ? 8u : (groups <= 640u ? 4u : 1u); }

// The launch of one traversal.  Returns NBODY_OK and the plan, or NBODY_ERR_ARG and the refusal (a format that takes nlevels).
inline int plan_bvh_force(const k9_request& r, k9_plan* out, const char** refusal) {
  const k9_overrides& o = r.overrides;
  const int traversal   = r.traversal == 0 ? o.mode : r.traversal;
  const bool wave = traversal >= 2 || (traversal == 0 && r.nlevels <= 26 && r.count >= k9_crossover(r.elem));
  if (wave && r.nlevels > 26)  // the packed key: covered << 5 | level (mode 6's other refusal, counters, is its launch's: bvh_forms.inc)
    return *refusal = traversal == 6 ? kK9RowsRefusal : kK9LevelsRefusal, NBODY_ERR_ARG;
  k9_plan p;
  if (traversal == 6) p.form = k9_form::row_sweeps;
  // (nbody_bvh_set_traversal(t, 1) keeps the walk over global memory: the tests compare the two bit for bit)
  if (!wave && traversal == 0 && k9_lds_fits(r.elem == 4 ? NBODY_F32 : NBODY_F64, r.nlevels)) {
    p.form      = k9_form::lane_lds;
    p.threads   = kTreeLdsThreads;
    p.lds_bytes = (r.nnodes + (1u << r.nlevels)) * 8u * r.elem;
  }
  const uint32_t bpl = wave && traversal == 4 ? 2u : 1u;
  p.groups = p.grid = (r.count + p.threads * bpl - 1u) / (p.threads * bpl);
  if (!wave || traversal == 6) return *out = p, NBODY_OK;
  p.form      = bpl == 2 ? k9_form::compiled_sweep_2
                         : (traversal == 0 || traversal == 2 || traversal == 5 ? k9_form::sweep : k9_form::compiled_sweep);
  p.lds_bytes = o.lds_bytes;
  const bool cut = bpl == 1 && r.launch_order == 0 && !o.plain_order;  // else one block per group in index order
  if (cut) p.parts = o.parts ? o.parts : k9_parts(p.groups);
  if (p.parts > 1u) {
    p.grid = p.groups * p.parts;
  } else if (cut && r.sorted && r.final_buf == 0) {
    // Work items (bvh_items_kernel): groups that straddle a jump of the key order are cut in two and started first.  Measured
    // in the CLI's step loop (ms per whole bvh step; index order / start order only / start order + cut): N = 10^6 8.05 / 7.4 /
    // 7.4, 5*10^5 5.3 / 4.6 / 4.3.  The sorted keys are in keys[1] when the sort ends in the buffer it started from
    // (final_buf == 0: the splitter sort, the radix sort's 8 passes; not the one-block sort, whose small trees take finer work items instead).
    uint32_t s0, l0;
    xcd_range(0, p.groups, &s0, &l0);  // XCD 0 has the longest range
    p.items     = true;
    p.split_den = o.split_den;
    p.stride    = l0 + split_budget(l0, o.split_den);
    p.grid      = 8u * p.stride;  // blocks are dealt round-robin over the XCDs: 8 lists of up to `stride` items
  }
  return *out = p, NBODY_OK;
}

// What the records' opening thresholds hold, as far as the host can know.  The sweep trusts them.  The host knows what they hold
// only along its own eager calls: a recorded step rewrites them whenever it is replayed.  So a recorded traversal skips the
// rewrite only behind a build (or traversal) of the SAME capture for the same angle, and once anything of this tree has been
// recorded an eager traversal always rewrites.  capture_id: 0 for an eager call.
struct k9_thresholds {
  double th2_built   = -1.0;      // theta^2 (in T) the host's own eager calls last wrote them for; -1: none
  bool ever_recorded = false;     // a build or traversal of this tree has been recorded
  unsigned long long rec_id = 0;  // the capture whose recorded build / traversal last wrote them ...
  double rec_th2     = -1.0;      // ... and the theta^2 it wrote them for (valid inside that capture only)
  bool fresh(unsigned long long capture_id, double th2) const {
    return capture_id ? (rec_id == capture_id && rec_th2 == th2) : (!ever_recorded && th2_built == th2);
  }
  void written(unsigned long long capture_id, double th2) {
    if (capture_id) ever_recorded = true, rec_id = capture_id, rec_th2 = th2;  // replayed at times the host does not see
    th2_built = th2;
  }
};

}  // namespace nbody
