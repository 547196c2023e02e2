/* bas_rate.h - sample-rate conversion of libbas_hip.so, beside the ABI of bas.h: the same conventions
 * (device pointers unless marked "host", one stream, no allocation, no synchronisation, 0 / BAS_E_* / hipError_t, the
 * text of bas_last_error), the same library, BAS_ABI_VERSION untouched.  The reference has no counterpart: it runs at the
 * rate of its HRIR table.
 *
 * ---- the conversion ---------------------------------------------------------------------------------------------------
 * A rational ratio p / q (p output samples for q input samples, p, q <= 4096) and a table of taps T[p][N] (float32, dense,
 * row ph = the filter phase ph; rate.py designs it: a Kaiser-windowed sinc whose stop band begins at the lower Nyquist)
 * with K0 taps on the early side:
 *     y[m] = sum_{k = 0}^{N - 1} T[ph][k] x~[b + K0 - k],     b = floor(m q / p),  ph = m q mod p,
 * where x~ is x inside the signal and 0 outside it.  The arithmetic (rate.convert_rate_f32_ref gives these bits): the N
 * products of a binary32 tap and a binary32 sample are exact in binary64; they are added one by one from +0 with k
 * ascending in binary64; the sum is rounded ONCE to binary32.  A sample outside the window is selected as 0 and never
 * read; a non-finite sample makes non-finite exactly the outputs whose N-sample window holds it (0 x Inf is NaN).
 *
 *   bas_rate_produced, bas_rate_needed: the stream counts, pure host functions (no device, no error text), any long:
 *     produced(n_in) = max(0, ceil((n_in - K0) p / q))     the outputs that n_in inputs determine,
 *     needed(m_out)  = floor((m_out - 1) q / p) + K0 + 1   the least n with produced(n) >= m_out; 0 for m_out <= 0,
 *     computed in 128-bit arithmetic and saturated to LONG_MAX; -1 for p < 1, q < 1 or K0 < 0.
 *   bas_rate_convert_f32: ONE stateless function for whole signals, stream blocks and a stream's end.
 *     x + g x_stride_g + r x_stride_r + i x_stride_t is the sample of ABSOLUTE index t0 + i of row (g, r), i in
 *     [0, T_win): the window.  Everything outside [t0, t0 + T_win) is zero and is not read.  The outputs written are those
 *     of absolute index m0 + j, j in [0, T_out), at out + g out_stride_g + r out_stride_r + j out_stride_t.
 *     A whole signal is t0 = m0 = 0 with T_out = ceil(T_win p / q).  A stream block is the same call on [history | block]
 *     with the history the row's last N - 1 samples (bas_delay_carry_f32 of bas.h moves them to the front afterwards), t0
 *     the absolute index of the history's first sample (negative at a stream's start: the zeroed history stands for the
 *     zeros in front of the signal), m0 = produced(inputs before the block) and T_out = produced(inputs with the block) -
 *     m0.  A stream's end is the call on the history alone, up to ceil(n_total p / q).  An output's bits depend on the
 *     samples of its own N-sample window alone: not on t0, m0, the block boundaries or how outputs are dealt to workgroups.
 *     Any strides >= 0: rows [n_rows][n], frames [n][2] (x_stride_r = 1, x_stride_t = 2), [G][n][2].  The output's strides
 *     must address every element once; input, taps and output must not overlap.
 *     One launch: one workgroup per (tile of BAS_RATE_TILE outputs, row, group); it stages its part of the window in LDS
 *     where that fits, and the taps beside it where they fit (otherwise they are read through the cache).
 *     Every argument check runs before any launch: 1 <= p, q <= 4096, 1 <= N <= 1024, p N <= 65536, 0 <= K0 < N,
 *     0 <= n_groups, n_rows <= 65535, 0 <= T_win < 2^31, -2^50 <= t0 <= 2^62, 0 <= T_out < 2^30, m0 >= 0,
 *     m0 + T_out <= 2^50 (so that m q stays inside a long), strides >= 0, below 2^40 (group, row) and 2^31 (sample), the
 *     output addressing no element twice, no overlap (BAS_E_SHAPE); x (T_win > 0), taps, out required (BAS_E_NULL) and
 *     4-byte aligned (BAS_E_ALIGN).  n_groups, n_rows or T_out of 0: nothing to do, no pointer is looked at. */
#ifndef BAS_RATE_H
#define BAS_RATE_H

#include "bas.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BAS_RATE_TILE 512          /* outputs per workgroup (rate.TILE) */
#define BAS_RATE_MAX_RATIO 4096    /* p, q */
#define BAS_RATE_MAX_TAPS 1024     /* N */
#define BAS_RATE_MAX_TABLE 65536   /* p N */

long bas_rate_produced(long n_in, int p, int q, int K0);
long bas_rate_needed(long m_out, int p, int q, int K0);
int bas_rate_convert_f32(const float *x, long x_stride_g, long x_stride_r, long x_stride_t, int n_groups, int n_rows,
                         long T_win, long t0, const float *taps, int p, int q, int N, int K0, float *out,
                         long out_stride_g, long out_stride_r, long out_stride_t, long m0, long T_out,
                         bas_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
