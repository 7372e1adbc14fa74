// The space key of K1's ordered launches (all_pairs.hip: "space order").  Plain C++: the device code takes it through common.hpp,
// tools/k1_order_key_check.cpp compiles it for the host alone (with the sanitizers) and tools/k1_order_model.py restates it in NumPy.
//
// A body's key is the 30-bit Morton code of the cell of side kOrderCell = 1 that holds it, on a FIXED absolute grid — the sparse
// rule's thresholds (r2 >= 4, a box gap of 3) are absolute lengths, so the cells are too, and the key of a body is a function of
// its own position only (never of the system's extent, which one escaper moves at will):
//     q_k  = clamp(floor(x_k) + 512, 0, 1023)         per axis, k < D (0 for the third axis in 2D);
//     key  = sum over bits b < 10 of  bit_b(q_0) << 3b  |  bit_b(q_1) << (3b + 1)  |  bit_b(q_2) << (3b + 2).
// Everything at or beyond +-512 shares the outermost cell of its side, so escapers and huge values still give a total order, and a
// coordinate that is NaN takes cell 0 (a defined key; such a system is dense by its moments and is never ordered in the first
// place).  -0.0 and +0.0 lie in the same cell (512).  Bodies are ordered by (key, index): a stable sort.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NB_KEY_FN __host__ __device__ inline
#else
#define NB_KEY_FN inline
#endif

namespace nbody {

constexpr int kOrderKeyBits    = 30;
constexpr int kOrderAxisBits   = 10;
constexpr double kOrderCell    = 1.0;
constexpr double kOrderHalf    = 512.0;  // cells on either side of the origin

// the cell number of one coordinate, 0 .. 1023
NB_KEY_FN uint32_t k1_order_cell(double x) {
  if (!(x >= -kOrderHalf)) return 0u;           // below the grid, -inf, NaN
  if (x >= kOrderHalf) return 1023u;            // above the grid, +inf
  // x in [-512, 512): floor(x) is exact, + 512 is exact, the conversion is in range
  return uint32_t(int32_t(__builtin_floor(x / kOrderCell)) + int32_t(kOrderHalf));
}

// bit b of q goes to bit 3 b
NB_KEY_FN uint32_t k1_order_spread(uint32_t q) {
  q &= 0x3ffu;
  q = (q | (q << 16)) & 0x030000ffu;
  q = (q | (q << 8)) & 0x0300f00fu;
  q = (q | (q << 4)) & 0x030c30c3u;
  q = (q | (q << 2)) & 0x09249249u;
  return q;
}

template <int D>
NB_KEY_FN uint64_t k1_order_key(const double* p) {
  uint32_t key = 0;
  for (int k = 0; k < D; ++k) key |= k1_order_spread(k1_order_cell(p[k])) << k;
  return uint64_t(key);
}

}  // namespace nbody
