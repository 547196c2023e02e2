// What every entry point that takes strided device views checks, written once (DESIGN.md "Views and sessions").  Host code
// only: nothing here is __device__, no kernel sees this header.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <initializer_list>

#define BAS_VIEW_MAX_DIMS 4

// The byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte.  A null pointer or an empty range meets nothing.
static inline bool bas_ranges_meet(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    if (!a || !b || a_bytes == 0 || b_bytes == 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// Elements from the first to one past the last of a view of n dimensions (extents >= 1, strides >= 0).
static inline long bas_view_extent(int n, const long *extent, const long *stride) {
    long last = 0;
    for (int k = 0; k < n; ++k) last += (extent[k] - 1) * stride[k];
    return last + 1;
}

// A written view of n <= BAS_VIEW_MAX_DIMS dimensions (extents >= 1, strides >= 0) addresses no element twice when every
// dimension of more than one element, in ascending stride order, steps over the whole span of the ones before it.
// Sufficient, not necessary (interleaved layouts fail it); a span beyond a long fails it too.
static inline bool bas_layout_nested(int n, const long *extent, const long *stride) {
    if (n > BAS_VIEW_MAX_DIMS) return false;
    long e[BAS_VIEW_MAX_DIMS], s[BAS_VIEW_MAX_DIMS];
    for (int k = 0; k < n; ++k) {                        // insertion sort by stride
        int i = k;
        for (; i > 0 && s[i - 1] > stride[k]; --i) {
            s[i] = s[i - 1];
            e[i] = e[i - 1];
        }
        s[i] = stride[k];
        e[i] = extent[k];
    }
    long span = 1;                                       // elements from the first to one past the last, so far
    for (int k = 0; k < n; ++k) {
        if (e[k] == 1) continue;
        long reach;
        if (s[k] < span || __builtin_mul_overflow(s[k], e[k] - 1, &reach) || __builtin_add_overflow(reach, span, &span))
            return false;
    }
    return true;
}

// A written layout [G][rows][nb] with element strides (sg, ss, 1), all >= 0, addresses no element twice.  Exact: two
// elements share an address exactly when some (dr, dg) != (0, 0) with |dr| < rows, |dg| < G has |dr ss + dg sg| < nb.
// The nested layouts every renderer uses pass the first test (bas_layout_nested, bas_views.h); the others - interleaved,
// non-nested - take the search: for every dg the dr that brings dr ss + dg sg nearest to zero, min(G, rows) steps in
// 128-bit arithmetic.
static inline bool bas_layout_one_to_one(long G, long rows, long nb, long sg, long ss) {
    if (G <= 0 || rows <= 0 || nb <= 0 || sg < 0 || ss < 0) return false;
    const long st[3] = {1, ss, sg}, ex[3] = {nb, rows, G};
    if (bas_layout_nested(3, ex, st)) return true;
    if (G > rows) {                                      // the outer loop over the shorter dimension
        const long t = G, u = sg;
        G = rows; sg = ss; rows = t; ss = u;
    }
    if (rows > 1 && ss < nb) return false;               // dg = 0
    for (long dg = 1; dg < G; ++dg) {
        const __int128 v = (__int128)dg * sg;            // dr = -k: v - k ss, k = 0 .. rows - 1
        if (ss == 0) {
            if (v < nb) return false;
            continue;
        }
        __int128 k = v / ss;
        if (k > rows - 1) k = rows - 1;
        if (v - k * ss < nb) return false;               // from above (>= 0)
        if (k + 1 <= rows - 1 && (k + 1) * ss - v < nb) return false;   // from below
    }
    return true;
}

// p is a multiple of a (a power of two).  A null pointer passes: what may be null is decided elsewhere.
static inline bool bas_aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// every stride >= 0 / below a bound
static inline bool bas_none_negative(std::initializer_list<long> v) {
    for (long x : v)
        if (x < 0) return false;
    return true;
}
static inline bool bas_all_below(long bound, std::initializer_list<long> v) {
    for (long x : v)
        if (x >= bound) return false;
    return true;
}
