// Stand-alone host check of K1's space key (stdpar-nbody_amd/csrc/k1_order_key.hpp): the committed function, compiled for the
// host alone, on its boundaries — cell edges, +-0, clamping at both ends, the infinities and NaN.  Meant to be built with the
// sanitizers (a conversion of an out-of-range double to an integer is undefined behaviour: the clamps must come first):
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I stdpar-nbody_amd/csrc tools/k1_order_key_check.cpp -o k1_order_key_check
// Prints one line per probe, `key D x0 x1 [x2] hexkey` (coordinates as hexadecimal floats), for tests/test_k1_space_order_model.py
// to hold the NumPy restatement to, then `ok`.  Exit status 1 on the first failed expectation.
#include "k1_order_key.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace nbody;

static int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static void print_coord(double v) {
  if (std::isnan(v)) std::printf(" nan");
  else if (std::isinf(v)) std::printf(v > 0 ? " inf" : " -inf");
  else std::printf(" %a", v);
}

template <int D>
static void probe(const double* p) {
  std::printf("key %d", D);
  for (int k = 0; k < D; ++k) print_coord(p[k]);
  std::printf(" %llx\n", static_cast<unsigned long long>(k1_order_key<D>(p)));
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double dmax = std::numeric_limits<double>::max(), dmin = std::numeric_limits<double>::denorm_min();
  // cells
  EXPECT(k1_order_cell(0.0) == 512u && k1_order_cell(-0.0) == 512u);
  EXPECT(k1_order_cell(dmin) == 512u && k1_order_cell(-dmin) == 511u);
  EXPECT(k1_order_cell(1.0) == 513u && k1_order_cell(std::nextafter(1.0, 0.0)) == 512u);
  EXPECT(k1_order_cell(-1.0) == 511u && k1_order_cell(std::nextafter(-1.0, -inf)) == 510u);
  EXPECT(k1_order_cell(-512.0) == 0u && k1_order_cell(std::nextafter(-512.0, -inf)) == 0u && k1_order_cell(std::nextafter(-512.0, 0.0)) == 0u);
  EXPECT(k1_order_cell(-511.0) == 1u);
  EXPECT(k1_order_cell(std::nextafter(512.0, 0.0)) == 1023u && k1_order_cell(512.0) == 1023u && k1_order_cell(511.0) == 1023u);
  EXPECT(k1_order_cell(std::nextafter(511.0, 0.0)) == 1022u);
  EXPECT(k1_order_cell(1e6) == 1023u && k1_order_cell(-1e300) == 0u && k1_order_cell(dmax) == 1023u && k1_order_cell(-dmax) == 0u);
  EXPECT(k1_order_cell(inf) == 1023u && k1_order_cell(-inf) == 0u && k1_order_cell(nan) == 0u && k1_order_cell(-nan) == 0u);
  // monotone over every cell edge of the grid
  uint32_t before = 0;
  for (int e = -513; e <= 513; ++e) {
    const uint32_t below = k1_order_cell(std::nextafter(double(e), -inf)), at = k1_order_cell(double(e));
    EXPECT(before <= below && below <= at && at <= 1023u);
    if (e > -512 && e < 512) EXPECT(at == below + 1u && at == uint32_t(e + 512));
    before = at;
  }
  // the interleave: bit b of axis k at bit 3 b + k
  for (uint32_t b = 0; b < 10; ++b) EXPECT(k1_order_spread(1u << b) == 1u << (3 * b));
  EXPECT(k1_order_spread(1023u) == 0x09249249u && k1_order_spread(0xfffffc00u) == 0u);
  {
    const double lo[3] = {-512.0, -512.0, -512.0}, hi[3] = {600.0, 600.0, 600.0}, mid[3] = {0.0, -0.0, 0.0};
    EXPECT(k1_order_key<3>(lo) == 0u && k1_order_key<3>(hi) == (1ull << kOrderKeyBits) - 1u);
    EXPECT(k1_order_key<3>(mid) == (7ull << 27));
    EXPECT(k1_order_key<2>(hi) == 0x1b6db6dbull && k1_order_key<2>(mid) == (3ull << 27));
    const double bad[3] = {nan, inf, -inf};
    EXPECT(k1_order_key<3>(bad) == (0x09249249ull << 1));
  }
  // the probes the NumPy restatement is held to
  const std::vector<double> edge = {0.0,   -0.0,  dmin,  -dmin, 0.5,   -0.5,  1.0,  -1.0, std::nextafter(1.0, 0.0), std::nextafter(-1.0, -inf),
                                    3.25,  -7.75, 100.0, -99.999, 255.0, 256.0, -256.0, 511.0, std::nextafter(512.0, 0.0), 512.0,
                                    -512.0, std::nextafter(-512.0, -inf), 1e6, -1e300, dmax, -dmax, inf, -inf, nan};
  for (size_t i = 0; i < edge.size(); ++i)
    for (size_t j = 0; j < edge.size(); j += 3) {
      const double p3[3] = {edge[i], edge[j], edge[(i + 2 * j + 1) % edge.size()]};
      const double p2[2] = {edge[j], edge[i]};
      probe<3>(p3);
      probe<2>(p2);
    }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
