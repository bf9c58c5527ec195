// The union-find of disparity_speckle.hip, apart from where the parents live: in LDS (the tile pass), in global memory (the merge
// pass) or in a host array (tools/speckle_union_host.cpp drives the same text on the CPU, where a sanitizer can watch it).
//
// Mem is a view of a parent array:  int load(int i) const            the parent of i
//                                   int fetch_min(int i, int v) const   parent[i] = min(parent[i], v) as ONE atomic; returns the value before
// The invariant every user keeps: parent[i] starts as i (or, before anybody walks, as a smaller element of i's own set whose chain
// ends in one that is its own parent) and is then changed by fetch_min alone, with the index of an element of i's own set.  So
// parent[i] <= i always, every value parent[i] ever held names an element of i's set, and a walk that follows a STALE parent still
// walks inside the set and still descends.  Smaller index wins: the root of a finished set is its smallest element.
#pragma once

#if defined(__HIPCC__)
#define SS_UNION_FN __host__ __device__ __forceinline__
#else
#define SS_UNION_FN inline
#endif

namespace ss {
namespace speckle {

// An element of x's set that was its own parent when it was read.  Descent: x takes the value p < x or the loop ends.
template <class Mem>
SS_UNION_FN int find(const Mem& m, int x) {
    for (;;) {
        const int p = m.load(x);
        if (p >= x) return x;              // (p == x under the invariant; >= so that the descent can be read off this line)
        x = p;
    }
}

// The sets of a and b become one.  Every decision rests on what the atomic returned: `old == hi` means hi was a root at that instant
// and now hangs under lo -- done.  Otherwise hi already had the parent old < hi; the atomic may have replaced that link by lo (when
// lo < old), so the sets of old and lo are united next, which covers both outcomes.  Descent: the larger of the two roots in hand,
// hi, is replaced by find(old) <= old < hi while lo only shrinks, so max(hi, lo) strictly decreases and is never below 0.
template <class Mem>
SS_UNION_FN void unite(const Mem& m, int a, int b) {
    int hi = find(m, a), lo = find(m, b);
    while (hi != lo) {
        if (hi < lo) {
            const int t = hi;
            hi = lo, lo = t;
        }
        const int old = m.fetch_min(hi, lo);
        if (old >= hi) return;             // (old == hi under the invariant)
        hi = find(m, old), lo = find(m, lo);
    }
}

}  // namespace speckle
}  // namespace ss
