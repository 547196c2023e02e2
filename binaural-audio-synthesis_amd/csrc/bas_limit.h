// The look-ahead limiter's sizes (bas_limit.hip; include/bas.h "look-ahead limiter").
#pragma once
#include "bas_internal.h"

#define LIM_THREADS 256
#define LIM_TILE 1024                              // output samples per workgroup (limiter.TILE)
#define LIM_PER_THREAD (LIM_TILE / LIM_THREADS)    // outputs a thread sums side by side
#define LIM_MAX_A BAS_LIMIT_MAX_LOOKAHEAD
#define LIM_MAX_HD BAS_LIMIT_MAX_HOLD
#define LIM_STATE_HEAD 4                           // floats in front of a session's ring: two positions, two spare

// context in front of an output: 2 A + Hd samples
static inline int lim_history(int A, int Hd) { return 2 * A + Hd; }
// floats of one of the kernel's two LDS arrays: history + tile, rounded up to whole quads
static inline int lim_span(int A, int Hd) { return (lim_history(A, Hd) + LIM_TILE + 3) & ~3; }
// dynamic LDS of the kernel: the two arrays (8 KiB .. 56 KiB: 56 KiB at A = 1024, Hd = 4096, so two workgroups share a
// CU's 160 KiB at the largest setting and eight at 5 ms / 20 ms)
static inline size_t lim_lds_bytes(int A, int Hd) { return 2 * (size_t)lim_span(A, Hd) * sizeof(float); }
