// union_find.h — the lock-free least-index union-find that mesh_ops.hip (components of a mesh's vertices) and point_segment.hip
// (clusters of a cloud's core points) share, written ONCE.
//
// A lock-free union-find over parent [nv] (the workspace).  parent[x] <= x always, and parent[x] is an ancestor of x in
// every interleaving, because the only writes are (a) atomicCAS(parent + hi, hi, lo) with lo < hi on a word that is still a root
// and (b) path halving, atomicMin(parent + x, grandparent), which can only move x to a lower ancestor.  A find therefore descends
// strictly and ends within nv steps.  parent words change under the linking kernel's feet — written by other workgroups, on other
// XCDs — so every read of them in that kernel is a relaxed agent-scope atomic load (an sc1 load: it bypasses the CU's L1 and is
// coherent at device scope, like the atomics that write the words; a plain load may keep hitting a stale L1 line).  A stale value
// would still be an ancestor, and nothing here waits for a value to change.  unite(a, b): find both roots; equal: done; else CAS the
// larger under the smaller; a failed CAS returns what the word holds now, a lower ancestor, and the loop goes on from there — the
// larger of the two roots strictly decreases, so at most nv rounds.  The final root of a component is its least index whatever
// the order of arrival.
#pragma once
#include "sgam_common.h"

namespace {

__device__ __forceinline__ int32_t load_relaxed(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x (-1: the bound was reached), halving the path on the way
__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x, int nv) {
    for (int step = 0; step <= nv; ++step) {
        const int32_t p = load_relaxed(parent + x);
        if (p == x) return x;
        const int32_t g = load_relaxed(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
    }
    return -1;
}

__device__ __forceinline__ bool uf_unite(int32_t *parent, int32_t a, int32_t b, int nv) {
    for (int round = 0; round <= nv; ++round) {
        a = uf_find(parent, a, nv);
        b = uf_find(parent, b, nv);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t was = atomicCAS(parent + hi, hi, lo);
        if (was == hi) return true;
        a = was;              // somebody else linked hi first: `was` < hi is an ancestor of hi
        b = lo;
    }
    return false;
}

}  // namespace
