// csrc/fof_union.hpp — the find and hook the friends-of-friends link kernel runs — on host threads: the same text, with std::atomic in
// place of the device's relaxed agent-scope atomics.  8 threads unite the edges of random graphs, chains and stars in interleaved
// slices; the partition must equal a sequential union-find's, every root must be its set's lowest element, parent[x] <= x must hold,
// and the successful hooks must number n minus the sets.  tests/test_fof.py builds this with -fsanitize=address,undefined and with
// -fsanitize=thread and runs it.  No HIP, no GPU.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../stdpar-nbody_amd/csrc/fof_union.hpp"

namespace {

struct host_atomics {
  static uint32_t load(std::atomic<uint32_t>* p) { return p->load(std::memory_order_relaxed); }
  static void store(std::atomic<uint32_t>* p, uint32_t v) { p->store(v, std::memory_order_relaxed); }
  static bool cas(std::atomic<uint32_t>* p, uint32_t expect, uint32_t want) {
    return p->compare_exchange_strong(expect, want, std::memory_order_relaxed, std::memory_order_relaxed);
  }
};

struct plain_ops {  // the sequential reference: the same functions over plain words
  static uint32_t load(uint32_t* p) { return *p; }
  static void store(uint32_t* p, uint32_t v) { *p = v; }
  static bool cas(uint32_t* p, uint32_t expect, uint32_t want) {
    if (*p != expect) return false;
    *p = want;
    return true;
  }
};

using edge  = std::pair<uint32_t, uint32_t>;
int g_errors = 0;

void fail(const char* what, const char* name, uint32_t at) {
  if (g_errors++ < 10) std::fprintf(stderr, "%s: %s at %u\n", name, what, at);
}

void run(const char* name, uint32_t n, const std::vector<edge>& edges, int threads) {
  std::vector<uint32_t> seq(n);
  std::iota(seq.begin(), seq.end(), 0u);
  uint32_t seq_hooks = 0;
  for (const edge& e : edges) seq_hooks += nbody::fof_hook<plain_ops>(seq.data(), e.first, e.second) ? 1u : 0u;

  std::vector<std::atomic<uint32_t>> par(n);
  for (uint32_t i = 0; i < n; ++i) par[i].store(i, std::memory_order_relaxed);
  std::atomic<uint32_t> hooks{0};
  std::vector<std::thread> pool;
  for (int t = 0; t < threads; ++t)
    pool.emplace_back([&, t] {
      uint32_t mine = 0;
      for (size_t k = size_t(t); k < edges.size(); k += size_t(threads))  // interleaved: neighbouring edges race
        mine += nbody::fof_hook<host_atomics>(par.data(), edges[k].first, edges[k].second) ? 1u : 0u;
      hooks.fetch_add(mine, std::memory_order_relaxed);
    });
  for (std::thread& t : pool) t.join();

  uint32_t sets = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (par[i].load() > i) fail("parent[x] > x", name, i);
    const uint32_t a = nbody::fof_find<host_atomics>(par.data(), i), b = nbody::fof_find<plain_ops>(seq.data(), i);
    if (a != b) fail("root differs from the sequential one", name, i);  // both are the set's lowest element
    if (a > i) fail("root above a member", name, i);
    sets += a == i ? 1u : 0u;
  }
  if (hooks.load() != n - sets) fail("successful hooks != n - sets", name, hooks.load());
  if (seq_hooks != n - sets) fail("sequential hooks != n - sets", name, seq_hooks);
}

}  // namespace

int main() {
  const int threads = 8;
  std::mt19937 rng(12345);
  for (uint32_t n : {1u, 2u, 3u, 64u, 1000u, 20000u}) {
    std::vector<uint32_t> shuffled(n);
    std::iota(shuffled.begin(), shuffled.end(), 0u);
    for (uint32_t i = n; i > 1; --i) std::swap(shuffled[i - 1], shuffled[rng() % i]);

    std::vector<edge> random_sparse, random_dense, chain, chain_shuffled, star_low, star_high, repeated;
    for (uint32_t k = 0; k < n / 2; ++k) random_sparse.emplace_back(rng() % n, rng() % n);
    for (uint32_t k = 0; k < 4 * n; ++k) random_dense.emplace_back(rng() % n, rng() % n);
    for (uint32_t i = 1; i < n; ++i) {
      chain.emplace_back(i, i - 1);                                      // the deepest forest before halving
      chain_shuffled.emplace_back(shuffled[i], shuffled[i - 1]);
      star_low.emplace_back(i, 0u);                                      // every hook races for one root
      star_high.emplace_back(n - 1, i - 1);
      for (int r = 0; r < 4; ++r) repeated.emplace_back(i, i / 2);       // mostly already joined: the no-CAS path
    }
    for (uint32_t i = n; i > 1; --i) std::swap(chain[i - 2], chain[rng() % (i - 1)]);
    run("random sparse", n, random_sparse, threads);
    run("random dense", n, random_dense, threads);
    run("chain", n, chain, threads);
    run("chain shuffled", n, chain_shuffled, threads);
    run("star low", n, star_low, threads);
    run("star high", n, star_high, threads);
    run("repeated", n, repeated, threads);
    run("no edges", n, {}, threads);
  }
  if (g_errors) {
    std::fprintf(stderr, "%d errors\n", g_errors);
    return 1;
  }
  std::puts("fof_union ok");
  return 0;
}
