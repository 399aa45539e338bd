// The lock-free union-find of the map's connected components (ef_components.inc: k_comp_hook, k_comp_label).
// parent[] holds one word per row: parent[x] == x for a root, a smaller row for every other node, UF_NONE for a row that is no node (never
// passed in here).
//   INVARIANT   parent[x] <= x always, and a word only ever DECREASES: a root r is linked by compare-and-swap(parent[r], r, lo) with lo < r, and
//               path halving lowers parent[x] to an ancestor by an atomic minimum.  Hence chains are acyclic, every value the word of x ever
//               held is a row of x's set (sets only ever grow) and not above x, a set has exactly one root, which is its smallest row (a link
//               removes the greater of two roots), and every step of uf_find and every retry of uf_union follows a strictly smaller value: both
//               end after at most x steps whatever other threads do.  Nobody waits for anybody.
//   STALE READS A load may return any value the word held earlier.  That is an earlier ancestor, a row of the same set: it costs steps, never
//               a wrong union.  "The roots agree" is only ever concluded from both walks reaching the same row, which makes a and b members of
//               one set for ever; a row that is no root any more fails its compare-and-swap, which returns the word's present value, and the
//               union goes on from there; a link root hi -> lo is right for any row lo < hi of the other set, root or not.
//   CAP         every loop counts its steps and gives up beyond `cap` (the caller passes n + 64), and a word found ABOVE its row (UF_NONE
//               included) ends the call the same way before it is followed: both unreachable by the argument above, they turn a logic error
//               into an error code instead of a thread that never ends or a read outside the array.
// The atomic operations come from a trait, so that the same text runs on the device (ef_components.inc: relaxed agent-scope loads, atomicCAS,
// atomicMin) and on host threads (tests/uf_threads.cpp: the compiler's __atomic builtins, which a thread sanitizer understands).
//   struct Ops { static uint32_t load(const uint32_t* p);                         // relaxed
//                static uint32_t cas(uint32_t* p, uint32_t expect, uint32_t want);  // returns the value found
//                static void lower(uint32_t* p, uint32_t v); };                    // *p = min(*p, v), atomically
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EF_UF_HD __host__ __device__ __forceinline__
#else
#define EF_UF_HD inline
#endif

namespace efm {

constexpr uint32_t UF_NONE = 0xFFFFFFFFu;

// the root of x as far as this thread's loads show it, halving the path on the way; false: the cap tripped or a word stood above its row
template <class Ops>
EF_UF_HD bool uf_find(uint32_t* parent, uint32_t x, uint32_t cap, uint32_t* root) {
  for (uint32_t steps = 0;; ++steps) {
    if (steps > cap) return false;
    const uint32_t p = Ops::load(parent + x);
    if (p == x) { *root = x; return true; }
    if (p > x) return false;   // a word above its row (UF_NONE of a row that is no node included): the invariant is broken, say so
    const uint32_t g = Ops::load(parent + p);
    if (g == p) { *root = p; return true; }
    if (g > p) return false;
    Ops::lower(parent + x, g);   // path halving: x now hangs under its grandparent, and the walk goes on from there
    x = g;
  }
}

// joins the sets of a and b; *root = a row both then descend from (the smaller root seen); false: as uf_find
template <class Ops>
EF_UF_HD bool uf_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t cap, uint32_t* root) {
  for (uint32_t tries = 0;; ++tries) {
    if (tries > cap) return false;
    if (!uf_find<Ops>(parent, b, cap, &b)) return false;
    if (a == b) { *root = a; return true; }   // b descends to the row a itself: one set, whether or not a is a root (most edges: no write,
                                              // and a caller that passes the root its last union returned pays no load for a)
    if (!uf_find<Ops>(parent, a, cap, &a)) return false;
    if (a == b) { *root = a; return true; }
    const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const uint32_t found = Ops::cas(parent + hi, hi, lo);
    if (found == hi) { *root = lo; return true; }
    if (found > hi) return false;   // (the invariant again: nothing above a row is ever followed)
    a = found;   // hi was linked by somebody else meanwhile: found < hi is its parent, go on from there
    b = lo;
  }
}

}  // namespace efm
