// Sample-rate conversion: sizes and host arithmetic (bas_rate.hip; include/bas_rate.h).  The functions
// here are host code (no kernel calls them); tests/hostsan/hostsan_rate.cpp includes this header for them.
#pragma once
#include <limits.h>

#include "bas_internal.h"
#include "../../include/bas_rate.h"

#define RATE_THREADS 256
#define RATE_TILE BAS_RATE_TILE                       // outputs per workgroup (rate.TILE)
#define RATE_PER_THREAD (RATE_TILE / RATE_THREADS)    // outputs a thread sums side by side
#define RATE_LDS_FLOATS 15360                         // dynamic LDS of a workgroup: 60 KiB (two workgroups share a CU)
#define RATE_WINDOW_LDS_FLOATS 12288                  // the staged window's share of it

// ---- the stream counts, for any long (128-bit inside, saturated) ---------------------------------------------------------
static inline long rate_saturate(__int128 v) { return v > (__int128)LONG_MAX ? LONG_MAX : (long)v; }
static inline long rate_produced(long n_in, int p, int q, int K0) {
    if (p < 1 || q < 1 || K0 < 0) return -1;
    if (n_in <= K0) return 0;
    return rate_saturate((((__int128)n_in - K0) * p + (q - 1)) / q);
}
static inline long rate_needed(long m_out, int p, int q, int K0) {
    if (p < 1 || q < 1 || K0 < 0) return -1;
    if (m_out <= 0) return 0;
    return rate_saturate(((__int128)m_out - 1) * q / p + K0 + 1);
}

static inline bool rate_params_ok(int p, int q, int N, int K0) {
    return p >= 1 && p <= BAS_RATE_MAX_RATIO && q >= 1 && q <= BAS_RATE_MAX_RATIO && N >= 1 && N <= BAS_RATE_MAX_TAPS &&
           (long)p * N <= BAS_RATE_MAX_TABLE && K0 >= 0 && K0 < N;
}

// Floats of the window a tile of RATE_TILE outputs reads, at most: the tile's first output has b = b_a and a remainder
// r_a <= p - 1, its last b_a + (r_a + (RATE_TILE - 1) q) / p; N - 1 more samples in front.  Rounded up to whole quads.
static inline long rate_window_floats(int p, int q, int N) {
    return (((long)(p - 1) + (long)(RATE_TILE - 1) * q) / p + N + 3) & ~3L;
}

// The row pitch of the tap table in LDS.  The 64 lanes of a wave hold consecutive outputs, so lane l reads row
// ph = (r_a + l q) mod p at the same k: float address ph pitch + k.  ds_read_b32 serves lanes 0-31 and 32-63 as two groups
// over 32 banks of 4 bytes, equal addresses broadcast, and every further distinct address on a bank costs a cycle.  The
// pitch is the first of N .. N + 31 with the fewest such addresses on the busiest bank (r_a = 0; another r_a moves every
// row by the same amount but for the wrap).  An up-conversion visits few rows per wave and any pitch serves; 160 / 147
// with N = 65 keeps 65 (neighbouring lanes are 13 rows apart: 13 x 65 floats, an odd number of banks).
static inline int rate_pitch(int p, int q, int N) {
    int best = N, best_cost = INT_MAX;
    for (int pitch = N; pitch < N + 32 && best_cost > 1; ++pitch) {
        int cost = 0;
        for (int g = 0; g < 2; ++g) {
            int addr[32], per_bank[32] = {0};
            for (int l = 0; l < 32; ++l) {
                const int a = (int)(((long)(32 * g + l) * q) % p) * pitch;
                bool seen = false;
                for (int j = 0; j < l && !seen; ++j) seen = addr[j] == a;
                addr[l] = a;
                if (!seen && ++per_bank[a & 31] > cost) cost = per_bank[a & 31];
            }
        }
        if (cost < best_cost) {
            best_cost = cost;
            best = pitch;
        }
    }
    return best;
}

// What a launch keeps in LDS: the window where it fits its share, the taps (at their pitch) where they fit beside it.
struct RatePlan {
    bool x_lds, t_lds;
    int pitch;              // floats between tap rows in LDS (t_lds)
    int x_floats;           // floats of the window's LDS area (0 without x_lds); the tap rows start behind it
    size_t lds_bytes;
};
static inline RatePlan rate_plan(int p, int q, int N) {
    RatePlan P;
    const long w = rate_window_floats(p, q, N);
    P.x_lds = w <= RATE_WINDOW_LDS_FLOATS;
    P.x_floats = P.x_lds ? (int)w : 0;
    P.pitch = rate_pitch(p, q, N);
    P.t_lds = P.x_floats + (long)p * P.pitch <= RATE_LDS_FLOATS;
    P.lds_bytes = sizeof(float) * ((size_t)P.x_floats + (P.t_lds ? (size_t)p * P.pitch : 0));
    return P;
}
