// Host check of csrc/bvh_plan.hpp: the launch plan of the BVH traversal (K9), the bound of its work-item lists and the host's account of
// the opening thresholds.  No kernel is launched and no device is opened.
//     hipcc -std=c++17 --offload-host-only -I stdpar-nbody_amd/csrc -I include tools/bvh_plan_check.cpp -o bvh_plan_check
// Swept over count = 1 .. 5000, every 257th up to 300 000, 10^6, 2^21, 2^22, 2^22 + 512 and 2^26, both precisions and every shipped
// traversal x launch_order x sorted x final_buf (the tree as small as it can be for `count` bodies, and up to 26 levels where the plan
// must not depend on it):
//  1. cover: groups blocks of `threads` bodies cover count and the last one is not empty; grid = groups * parts when parts > 1;
//  2. parts is 1, 4 or 8, and more than 1 only for the sweep in work-item order;
//  3. items exactly for the sweep with parts = 1 over sorted keys left in keys[1] in work-item order; then stride = len0 +
//     split_budget(len0), grid = 8 * stride, every XCD range with its budget fits the stride, and xcd_range tiles [0, groups)
//     contiguously with lengths that differ by at most one, range 0 the longest;
//  4. 8 * stride <= k9_items_capacity(n) for every count <= n (the capacity grows with n: n = count is checked), also with the
//     experiments' denominator 1, which cuts every group;
//  5. the LDS form exactly where k9_lds_fits holds (float, auto, below the sweep's crossover), with (nnodes + 2^nlevels) * 32 bytes;
//  6. the plan depends on count and not on the size of the tree (the LDS rule apart, which is the tree's), and not on the counters:
//     k9_request has no member for them, the counting kernels are launched in the plain ones' shape;
//  7. the truth table of k9_thresholds; 8. shapes pinned by hand from the rule; 9. the two refusals.
// Where each branch runs on hardware (tests/test_gpu_bvh.py unless said otherwise):
//   per-lane global    every test at traversal 1; double auto below 4096: test_traversal_forms_fuzz; float auto at 2049 and 20 000:
//                      test_wave_cooperative_equals_per_lane_bitwise
//   per-lane LDS       float auto at 2 .. 2048: test_wave_cooperative_equals_per_lane_bitwise, test_traversal_forms_fuzz
//   sweep, parts = 8   test_traversal_shard_windows_bitwise at 9000 (windows of 1000, 4001, 3999); double auto at 4096, 4097, 20 000
//   sweep, parts = 4   test_recorded_steps_and_eager_traversals_at_other_angles at 30 000
//   every form and launch shape of the sweep, float and double, 2D and 3D, counters on and off, per body against the wide walk:
//                      tests/test_gpu_bvh_wide.py (4099, 20 545 and 41 001 bodies, pinned below)
//   sweep, items       test_sweep_work_items_and_shard_windows at 200 003 (windows of 70 000, 65 539, 64 464),
//                      test_config4_n1e6_galaxy_theta05_vs_oracle at 10^6, test_bvh_whole_force_phase_at_2pow21; in float at traversal 5:
//                      70 000 (tests/test_gpu_cli.py, the long runs of both forms).  Float in auto mode takes the sweep from 180 000
//                      bodies on: the same launch, no GPU test of its own (pinned below)
//   sweep, index order test_sweep_work_items_and_shard_windows at 200 003 with launch order 1.  The same launch serves keys that are
//                      not in keys[1]: an unsorted tree, or final_buf = 1, which the sort leaves only up to 2048 bodies, where
//                      parts = 8 comes first
//   a range longer than kOrderMax (budget 0, from 2^22 + 1 bodies) and the refusal beyond 26 levels: not run on hardware
//   traversal 3, 4, 6  test_experiment_forms_are_bitwise_equal at 60 001 (experiments library)
#include <cstdio>
#include <initializer_list>

#include "bvh_plan.hpp"

using namespace nbody;

static int fail(const char* what, const k9_request& r) {
  std::printf("FAILED %s at elem = %u, count = %u, nlevels = %u, traversal = %d, launch_order = %d, sorted = %d, final_buf = %d\n", what,
              r.elem, r.count, r.nlevels, r.traversal, r.launch_order, int(r.sorted), r.final_buf);
  return 1;
}

static uint32_t levels_for(uint32_t n) {  // nbody_bvh_create's
  uint32_t nl = 0;
  while ((uint64_t(1) << nl) < n) ++nl;
  return nl;
}

static k9_request request(uint32_t elem, uint32_t count, uint32_t nlevels, int traversal = 0, int order = 0, bool sorted = true, int final_buf = 0) {
  k9_request r;
  r.elem = elem, r.count = count, r.nlevels = nlevels, r.nnodes = uint32_t((uint64_t(1) << nlevels) - 1u);
  r.traversal = traversal, r.launch_order = order, r.sorted = sorted, r.final_buf = final_buf;
  return r;
}

static bool same(const k9_plan& a, const k9_plan& b) {
  return a.form == b.form && a.grid == b.grid && a.threads == b.threads && a.lds_bytes == b.lds_bytes && a.groups == b.groups &&
         a.parts == b.parts && a.items == b.items && a.stride == b.stride && a.split_den == b.split_den;
}

static int check(const k9_request& r) {
  k9_plan p;
  const char* why = nullptr;
  if (plan_bvh_force(r, &p, &why)) return fail("refused", r);
  const bool sweep = p.form == k9_form::sweep, lds = p.form == k9_form::lane_lds;
  if (!sweep && !lds && p.form != k9_form::lane_global) return fail("a form that is not shipped", r);
  // 1
  if (p.threads != (lds ? 256u : 64u)) return fail("threads", r);
  if (uint64_t(p.groups) * p.threads < r.count || uint64_t(p.groups - 1u) * p.threads >= r.count) return fail("cover", r);
  if (p.parts > 1u ? p.grid != p.groups * p.parts : (!p.items && p.grid != p.groups)) return fail("grid", r);
  // 2
  if (p.parts != 1u && p.parts != 4u && p.parts != 8u) return fail("parts", r);
  if (p.parts > 1u && !(sweep && r.launch_order == 0)) return fail("parts outside the sweep in work-item order", r);
  // 3, 4
  if (p.items != (sweep && p.parts == 1u && r.sorted && r.final_buf == 0 && r.launch_order == 0)) return fail("items", r);
  if (p.items) {
    uint32_t next = 0, len0 = 0;
    for (uint32_t xcd = 0; xcd < 8u; ++xcd) {
      uint32_t start, len;
      xcd_range(xcd, p.groups, &start, &len);
      if (xcd == 0) len0 = len;
      if (start != next || len > len0 || len + 1u < len0) return fail("xcd_range", r);
      if (len + split_budget(len) > p.stride) return fail("a range and its budget beyond the stride", r);
      next = start + len;
    }
    if (next != p.groups) return fail("xcd_range does not end at groups", r);
    if (p.split_den != 16u || p.stride != len0 + split_budget(len0) || p.grid != 8u * p.stride) return fail("stride", r);
    if (size_t(p.grid) > k9_items_capacity(r.count)) return fail("capacity", r);
    k9_request all = r;
    all.overrides.split_den = 1;
    k9_plan q;
    if (plan_bvh_force(all, &q, &why) || !q.items || q.stride != len0 + split_budget(len0, 1u) || size_t(q.grid) > k9_items_capacity(r.count))
      return fail("capacity with every group cut", r);
  }
  // 5
  const bool lane = r.traversal == 1 || (r.traversal == 0 && (r.nlevels > 26 || r.count < k9_crossover(r.elem)));
  if (lane == sweep) return fail("per-lane or sweep", r);
  if (lds != (lane && r.traversal == 0 && k9_lds_fits(r.elem == 4 ? NBODY_F32 : NBODY_F64, r.nlevels))) return fail("LDS form", r);
  if (lds && (r.elem != 4 || p.lds_bytes != (r.nnodes + (1u << r.nlevels)) * 32u || p.lds_bytes > kTreeLdsBytes)) return fail("LDS bytes", r);
  if (!lds && p.lds_bytes != 0) return fail("LDS bytes of another form", r);
  // 6: a larger tree around the same bodies (from 12 levels on no float tree fits LDS)
  for (uint32_t nl = r.nlevels < 12u ? 12u : r.nlevels + 1u; nl <= 26u && !lds; nl += 7u) {
    k9_request big = r;
    big.nlevels = nl, big.nnodes = (1u << nl) - 1u;
    k9_plan q;
    if (plan_bvh_force(big, &q, &why) || !same(p, q)) return fail("the plan follows the size of the tree", r);
  }
  return 0;
}

static int check_count(uint32_t count) {
  for (uint32_t elem : {8u, 4u})
    for (int traversal : {0, 1, 2, 5})
      for (int order : {0, 1})
        for (int sorted : {1, 0})
          for (int final_buf : {0, 1})
            if (check(request(elem, count, levels_for(count < 2u ? 2u : count), traversal, order, sorted != 0, final_buf))) return 1;
  return 0;
}

static int check_thresholds() {
  const double a = 0.25, b = 0.81;
  k9_thresholds t;
  if (t.fresh(0, a)) return 1;  // nothing built
  t.written(0, a);              // eager build
  if (!t.fresh(0, a) || t.fresh(0, b) || t.fresh(7, a)) return 1;
  t.written(0, b);  // eager force at another angle
  if (!t.fresh(0, b) || t.fresh(0, a)) return 1;
  t.written(7, a);  // a recorded build: from now on no eager force is fresh
  if (t.fresh(0, a) || t.fresh(0, b)) return 1;
  if (!t.fresh(7, a) || t.fresh(7, b) || t.fresh(8, a)) return 1;  // the same capture and angle only
  t.written(0, a);  // eager again
  if (t.fresh(0, a) || !t.fresh(7, a)) return 1;
  t.written(8, b);
  if (t.fresh(7, a) || t.fresh(7, b) || !t.fresh(8, b) || t.fresh(0, b)) return 1;
  return 0;
}

struct pin {
  k9_request r;
  k9_form form;
  uint32_t grid, groups, parts, stride, lds_bytes;  // groups, parts = 0: not pinned
};

static int check_pins() {
  const auto d = [](uint32_t count, uint32_t n = 0, int order = 0, int final_buf = 0) {
    return request(8, count, levels_for(n ? n : count), 0, order, true, final_buf);
  };
  const auto f = [](uint32_t count, int traversal = 0, int order = 0) { return request(4, count, levels_for(count), traversal, order); };
  const k9_form lane = k9_form::lane_global, lds = k9_form::lane_lds, sweep = k9_form::sweep;
  const pin pins[] = {
      {d(4095), lane, 64, 0, 1, 0, 0},
      {d(4096), sweep, 512, 0, 8, 0, 0},
      {d(9000), sweep, 1128, 141, 8, 0, 0},
      {d(10000), sweep, 1256, 0, 8, 0, 0},
      {d(10000, 0, 1), sweep, 157, 0, 1, 0, 0},
      {d(20480), sweep, 2560, 320, 8, 0, 0},
      {d(20481), sweep, 1284, 0, 4, 0, 0},
      {d(30000), sweep, 1876, 0, 4, 0, 0},
      {d(40960), sweep, 2560, 0, 4, 0, 0},
      {d(40961), sweep, 688, 0, 1, 86, 0},
      {d(40961, 0, 0, 1), sweep, 641, 0, 1, 0, 0},
      {d(200003), sweep, 3320, 3126, 1, 415, 0},
      {d(65539, 200003), sweep, 1096, 1025, 1, 137, 0},
      {d(1000000), sweep, 16608, 0, 1, 2076, 0},
      {d(1u << 21), sweep, 34816, 0, 1, 4352, 0},
      {d(1u << 22), sweep, 69632, 0, 1, 8704, 0},
      {d((1u << 22) + 512u), sweep, 65544, 0, 1, 8193, 0},  // a range longer than kOrderMax: budget 0
      {f(2048), lds, 8, 0, 1, 0, 131040},
      {f(2048, 1), lane, 32, 0, 1, 0, 0},
      {f(2049), lane, 33, 0, 1, 0, 0},
      {f(1000, 2), sweep, 128, 0, 8, 0, 0},
      {f(179999), lane, 2813, 0, 1, 0, 0},
      {f(180000), sweep, 2992, 0, 1, 374, 0},
      {d((1u << 26) + 1u), lane, 1048577, 0, 1, 0, 0},  // 27 levels in auto mode: per-lane
      // what tests/test_gpu_bvh_wide.py launches, count -> groups -> shape, double on auto and float at traversal 5: 4099 -> 65 -> 8 lane
      // ranges; 20545 -> 322 -> 4 ranges; 41001 -> 641 -> 1 range with work items (81 + 5 per list), and in index order without
      {d(4099), sweep, 520, 65, 8, 0, 0},
      {d(20545), sweep, 1288, 322, 4, 0, 0},
      {d(41001), sweep, 688, 641, 1, 86, 0},
      {d(41001, 0, 1), sweep, 641, 641, 1, 0, 0},
      {f(4099, 5), sweep, 520, 65, 8, 0, 0},
      {f(20545, 5), sweep, 1288, 322, 4, 0, 0},
      {f(41001, 5), sweep, 688, 641, 1, 86, 0},
      {f(41001, 5, 1), sweep, 641, 641, 1, 0, 0},
      {f(4099), lane, 65, 65, 1, 0, 0},  // float on auto above 2048 bodies: per-lane over global memory
  };
  for (const pin& q : pins) {
    k9_plan p;
    const char* why = nullptr;
    if (plan_bvh_force(q.r, &p, &why)) return fail("pinned shape refused", q.r);
    if (p.form != q.form || p.grid != q.grid || (q.groups && p.groups != q.groups) || (q.parts && p.parts != q.parts) ||
        p.items != (q.stride != 0) || p.stride != q.stride || p.lds_bytes != q.lds_bytes)
      return fail("pinned shape", q.r);
  }
  // 9: 27 levels and the sweep asked for; mode 6 (experiments) on the same tree
  k9_request r = request(8, (1u << 26) + 1u, 27, 2);
  k9_plan p;
  const char* why = nullptr;
  if (plan_bvh_force(r, &p, &why) != NBODY_ERR_ARG || why != kK9LevelsRefusal) return fail("refusal beyond 26 levels", r);
  r.traversal = 6;
  if (plan_bvh_force(r, &p, &why) != NBODY_ERR_ARG || why != kK9RowsRefusal) return fail("refusal of the row sweeps beyond 26 levels", r);
  return 0;
}

int main() {
  for (uint32_t count = 1; count <= 5000u; ++count)
    if (check_count(count)) return 1;
  for (uint32_t count = 5000u + 257u; count <= 300000u; count += 257u)
    if (check_count(count)) return 1;
  for (uint32_t count : {1000000u, 1u << 21, 1u << 22, (1u << 22) + 512u, 1u << 26})
    if (check_count(count)) return 1;
  if (check_thresholds()) return std::printf("FAILED thresholds truth table\n"), 1;
  if (check_pins()) return 1;
  std::printf("ok\n");
  return 0;
}
