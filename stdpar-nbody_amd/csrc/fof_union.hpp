// The lock-free union-find of the friends-of-friends link kernel (fof.inc), as text that also compiles for the host: find and hook are
// templated on the atomic operations A, so tests/fof_union_main.cpp runs THESE functions with std::atomic on host threads under the
// sanitizers, and fof.inc runs them with relaxed agent-scope __hip_atomic_* on the device.
//   A::load(p)                relaxed load of *p
//   A::store(p, v)            relaxed store
//   A::cas(p, expect, want)   relaxed compare-and-swap; true iff *p was `expect` and is now `want`
//
// parent[] is a forest over 0 .. n - 1, identity at the start.  Invariants, true at every moment and for every interleaving:
//   (a) parent[x] <= x.  The identity has it; hook writes a SMALLER root into a larger one; halving writes an ancestor of x, and an
//       ancestor is < x by (a) itself.  So a chain x, parent[x], parent[parent[x]], ... strictly decreases until it reaches an r with
//       parent[r] == r: a root.  find therefore ends after at most x steps whatever the other lanes do.
//   (b) only a root is ever hooked, and only by a CAS that expects parent[r] == r; a node that has stopped being a root never becomes
//       one again (halving only ever stores to a node whose parent it has SEEN to differ from it).  So every set has exactly one
//       root, it is the set's lowest element, and every stale value a relaxed load may return is a value that was true once — an
//       ancestor once is in the same set for ever, and still smaller.
// Termination of hook: its loop repeats only after a FAILED CAS on a root r it had just found.  The CAS fails only if parent[r] != r,
// and the only write that does that to a root is another lane's SUCCESSFUL hook.  Every successful hook removes one root, there are
// n of them at the start and at least one at the end: at most n - 1 successes in the whole run, so at most n - 1 failures per caller.
// No loop here waits for another lane, wave, block or thread to do something: there is no spin, no flag and no ticket — a lane that
// is alone makes progress, and a lane that loses a race has been handed the progress of the one that won.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FOF_UNION_FN __host__ __device__ inline
#else
#define FOF_UNION_FN inline
#endif

namespace nbody {

// The root of x, with path halving: every node on the way is pointed at its grandparent.
template <typename A, typename P>
FOF_UNION_FN uint32_t fof_find(P* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = A::load(parent + x);
    if (p == x) return x;
    const uint32_t g = A::load(parent + p);
    if (g == p) return p;
    A::store(parent + x, g);  // x is not a root (p != x was seen) and g is an ancestor of x: (a) and (b) hold
    x = g;
  }
}

// Joins the sets of a and b: the LARGER root is pointed at the smaller.  Equal roots — the usual case in a dense group — cost the two
// finds and no CAS.  Returns true iff this call removed a root.
template <typename A, typename P>
FOF_UNION_FN bool fof_hook(P* parent, uint32_t a, uint32_t b) {
  for (;;) {
    uint32_t ra = fof_find<A>(parent, a), rb = fof_find<A>(parent, b);
    if (ra == rb) return false;
    if (ra < rb) {
      const uint32_t t = ra;
      ra               = rb;
      rb               = t;
    }
    if (A::cas(parent + ra, ra, rb)) return true;
    a = ra;  // a failed CAS: ra has been hooked by someone else (one of at most n - 1 hooks); go on from the two roots
    b = rb;
  }
}

}  // namespace nbody
