// The true-peak limiter's sizes and taps (bas_limit_tp.hip; include/bas_limit_tp.h).  The stages behind
// the detector are the look-ahead limiter's own (bas_limit.h).
#pragma once
#include "../../include/bas_limit_tp.h"
#include "bas_limit.h"

#define LIM_TP_REACH 6                             // samples on either side of n that d[n] reads
#define LIM_TP_TAPS 12                             // taps of a phase: j = -5 .. 6
#define LIM_TP_PHASES 3                            // p = 1, 2, 3: the values at m + p / 4
#define LIM_TP_QUAD_WINDOWS 5                      // interpolated positions a thread forms for its four d: m = n - 1 .. n + 3

// g_p[j] of DESIGN.md §3.20, row p - 1, j = -5 .. 6: the bits of loudness.true_peak_taps() (tests/test_limiter_tp_cpu.py
// compares them), which the meter takes as an argument and this kernel holds as constants
#define LIM_TP_TAP_VALUES                                                                                                  \
    {-0x1.0a4bb8p-10f, 0x1.8be736p-8f, -0x1.5af0fep-6f, 0x1.db6a28p-5f, -0x1.38f966p-3f, 0x1.c9f84cp-1f,                   \
     0x1.21cb3ep-2f, -0x1.7cb68ep-4f, 0x1.24cc54p-5f, -0x1.82e922p-7f, 0x1.65f152p-9f, -0x1.0cad96p-12f,                   \
     -0x1.96e6ecp-11f, 0x1.7f8886p-8f, -0x1.71ad5p-6f, 0x1.08b722p-4f, -0x1.56c4a8p-3f, 0x1.3d8e58p-1f,                    \
     0x1.3d8e58p-1f, -0x1.56c4a8p-3f, 0x1.08b722p-4f, -0x1.71ad5p-6f, 0x1.7f8886p-8f, -0x1.96e6ecp-11f,                    \
     -0x1.0cad96p-12f, 0x1.65f152p-9f, -0x1.82e922p-7f, 0x1.24cc54p-5f, -0x1.7cb68ep-4f, 0x1.21cb3ep-2f,                   \
     0x1.c9f84cp-1f, -0x1.38f966p-3f, 0x1.db6a28p-5f, -0x1.5af0fep-6f, 0x1.8be736p-8f, -0x1.0a4bb8p-10f}

// samples per ear that an output depends on in front of it, and that a stream carries: 2 A + Hd + 12
static inline int lim_tp_history(int A, int Hd) { return lim_history(A, Hd) + 2 * LIM_TP_REACH; }
// samples by which a stream is late: A + 6
static inline int lim_tp_latency(int A) { return A + LIM_TP_REACH; }
// floats of one of the kernel's two LDS arrays: the limiter's span, and the 12 raw samples more that the detector reads
// around it (a multiple of 4: the second array stays on a 16-byte boundary)
static inline int lim_tp_span(int A, int Hd) { return lim_span(A, Hd) + 2 * LIM_TP_REACH; }
// dynamic LDS of the kernel: 96 bytes more than the look-ahead limiter's (8 288 bytes .. 57 440)
static inline size_t lim_tp_lds_bytes(int A, int Hd) { return 2 * (size_t)lim_tp_span(A, Hd) * sizeof(float); }
// launches of a call: the limiter's rule - a stream block of more than one tile leaves its carry to a second launch
static inline int lim_tp_advance(bool state, long T_in, long T_out) {
    return !(state && T_in > 0) ? 0 : T_out <= LIM_TILE ? 2 : 1;
}
