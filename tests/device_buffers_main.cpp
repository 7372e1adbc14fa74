// csrc/device_buffers.hpp against a stand-in runtime: hipMalloc, hipFree, hipHostMalloc and hipHostFree are defined here over malloc,
// count the live blocks, refuse a block that is not live (a double free, or memory freed as the wrong kind) and fail at a chosen
// call.  No HIP library is linked.  tests/test_device_buffers.py builds this with the host compiler and runs it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <type_traits>

#include "../stdpar-nbody_amd/csrc/device_buffers.hpp"

namespace {
std::map<void*, bool> g_live;  // block -> pinned host memory
int g_calls   = 0;             // allocation calls that reached the runtime
int g_fail_at = -1;            // the call (counted from 0) that fails; -1: none
int g_bad     = 0;             // frees of a block that is not live, or as the wrong kind
int g_errors  = 0;

hipError_t fake_alloc(void** p, size_t bytes, bool pinned) {
  if (g_calls++ == g_fail_at) return hipErrorOutOfMemory;  // *p is left as it was, like the runtime
  *p          = malloc(bytes ? bytes : 1);
  g_live[*p]  = pinned;
  return hipSuccess;
}
hipError_t fake_free(void* p, bool pinned) {
  if (!p) return hipSuccess;
  auto it = g_live.find(p);
  if (it == g_live.end() || it->second != pinned) {
    ++g_bad;
    return hipErrorInvalidValue;
  }
  g_live.erase(it);
  free(p);
  return hipSuccess;
}
}  // namespace

extern "C" hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes, false); }
extern "C" hipError_t hipFree(void* p) { return fake_free(p, false); }
extern "C" hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return fake_alloc(p, bytes, true); }
extern "C" hipError_t hipHostFree(void* p) { return fake_free(p, true); }

#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      ++g_errors;                                                                        \
      fprintf(stderr, "%s:%d: fail_at %d: %s\n", __FILE__, __LINE__, g_fail_at, #cond); \
    }                                                                                    \
  } while (0)

static_assert(!std::is_copy_constructible_v<nbody::device_buffers> && !std::is_copy_assignable_v<nbody::device_buffers>,
              "the owner is not copyable");

constexpr int kAllocs = 12;
const char* const kGarbage = "x";

// allocation i of the 12: every fourth one pinned, the pointer types mixed as in the handles
static void one_alloc(nbody::device_buffers& mem, int i, void** slot) {
  *slot = const_cast<char*>(kGarbage);  // a failed or skipped call must overwrite this with NULL
  const size_t bytes = size_t(16) * size_t(i + 1);
  if (i % 4 == 3) mem.alloc_pinned(reinterpret_cast<uint32_t**>(slot), bytes, hipHostMallocMapped);
  else if (i % 4 == 1) mem.alloc(reinterpret_cast<uint64_t**>(slot), bytes);
  else mem.alloc(slot, bytes);
}

// fail_at in 0 ... 11: that allocation fails; 12: none does
static void run(int fail_at, bool by_destructor) {
  g_fail_at = fail_at < kAllocs ? fail_at : -1;
  g_calls   = 0;
  void* p[kAllocs];
  void* late = nullptr;
  {
    nbody::device_buffers mem;
    for (int i = 0; i < kAllocs; ++i) {
      const int before = g_calls;
      one_alloc(mem, i, &p[i]);
      if (i < fail_at) {
        CHECK(mem.error() == hipSuccess && p[i] != nullptr && p[i] != kGarbage);
      } else {  // the failing call and every later one: the first error stands, the pointer is NULL
        CHECK(mem.error() == hipErrorOutOfMemory);
        CHECK(p[i] == nullptr);
      }
      CHECK(g_calls == before + (i <= fail_at ? 1 : 0));  // nothing after the failure reaches the runtime
    }
    CHECK(int(g_live.size()) == (fail_at < kAllocs ? fail_at : kAllocs));

    mem.release();
    CHECK(g_live.empty());
    CHECK(g_bad == 0);
    CHECK(mem.error() == hipSuccess);
    mem.release();  // nothing left to free
    CHECK(g_bad == 0);

    // after a release the owner is as new: a late allocation is made, owned and freed
    g_fail_at = -1;
    CHECK(mem.alloc_late(&late, 64) == hipSuccess && late != nullptr);
    CHECK(g_live.size() == 1);
    // a late allocation that fails leaves NULL, no record and no error behind, and can be repeated
    void* again = const_cast<char*>(kGarbage);
    g_fail_at   = g_calls;
    CHECK(mem.alloc_late(&again, 64) == hipErrorOutOfMemory && again == nullptr);
    CHECK(mem.error() == hipSuccess && g_live.size() == 1);
    CHECK(mem.alloc_late(&again, 64) == hipSuccess && again != nullptr);
    CHECK(g_live.size() == 2);
    if (!by_destructor) {
      mem.release();
      CHECK(g_live.empty());
    }
  }
  CHECK(g_live.empty());  // the destructor freed what was left, and nothing twice
  CHECK(g_bad == 0);
}

int main() {
  for (int fail_at = 0; fail_at <= kAllocs; ++fail_at) {
    run(fail_at, false);
    run(fail_at, true);
  }
  if (g_errors) {
    fprintf(stderr, "device_buffers: %d checks failed\n", g_errors);
    return 1;
  }
  printf("device_buffers ok: %d allocations, failure at every position 0..%d, release and destructor\n", kAllocs, kAllocs);
  return 0;
}
