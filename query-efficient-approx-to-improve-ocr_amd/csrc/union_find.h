// Lock-free min-index union-find over an int array L with L[x] <= x (Playne & Hawick 2018; Komura 2015), shared by csrc/components.hip
// (a tile's pixels in LDS, a page's pixels in global memory) and csrc/lines.hip (a page's word boxes in LDS).
//
// The invariant: L[x] <= x, and L[x] is a member of x's set; a negative L[x] marks an x that is in no set.  A link is only ever replaced
// by a smaller one, and the thread that replaces the link x -> old by x -> b goes on to unite old with b, so no connection is lost.  The
// smallest member m of a set can only point to itself, so it is a root throughout; once every pair that belongs together has been united a
// set has one root, and that root is m.  A load that returns an older value returns an older parent, which is still a smaller member of
// the same set: only the value the atomic minimum returns decides whether a union is complete.
//
// Termination: find moves to a strictly smaller index or exits; unite strictly lowers the larger of its two indices or exits.  Either
// loop's length is bounded by the chain it walks.  A value that is no index (negative) ends a walk and is never used as an address.
#pragma once

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
#define RLX_GROUP __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP

struct LdsForest {      // workgroup scope: L lives in LDS
  int* L;
  __device__ __forceinline__ int load(int x) const { return __hip_atomic_load(L + x, RLX_GROUP); }
  __device__ __forceinline__ int lower(int x, int v) const { return __hip_atomic_fetch_min(L + x, v, RLX_GROUP); }
};
struct PageForest {     // agent scope: L lives in global memory and several workgroups walk it
  int* L;
  __device__ __forceinline__ int load(int x) const { return __hip_atomic_load(L + x, RLX_AGENT); }
  __device__ __forceinline__ int lower(int x, int v) const { return __hip_atomic_fetch_min(L + x, v, RLX_AGENT); }
};

template <class F>
__device__ __forceinline__ int find_root(const F f, int x) {
  for (;;) {                    // moves to a strictly smaller index or exits: at most the length of the chain it walks
    const int p = f.load(x);
    if (p >= x || p < 0) return x;
    x = p;
  }
}

template <class F>
__device__ __forceinline__ void unite(const F f, int a, int b) {
  for (;;) {                    // max(a, b) strictly falls from one round to the next, or the loop exits
    a = find_root(f, a);
    b = find_root(f, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = f.lower(a, b);            // a > b
    if (old == a) return;                     // a was a root and now points to b
    a = old;                                  // a had a parent old < a already: old and b remain to be united
  }
}
