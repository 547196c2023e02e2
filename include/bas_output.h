/* bas_output.h - the stereo output filter of libbas_hip.so, beside the ABI of bas.h: the same conventions
 * (device pointers, one stream, no allocation, no synchronisation, 0 / BAS_E_* / hipError_t, the text of bas_last_error),
 * the same library, BAS_ABI_VERSION untouched.  The reference has no counterpart: it hands out the raw stereo sum.
 *
 * ---- the filter -------------------------------------------------------------------------------------------------------
 * A filter set is h[o][i][k], output channel o, input channel i, k = 0 .. M - 1 (float32, 1 <= M <= 2048), in one of two
 * forms: full, dense [2][2][M], or diagonal, dense [2][M] with h[o][i] = 0 for o != i (the cross terms are neither read nor
 * multiplied).  For frames y[n][i], zero outside the signal,
 *     z[n][o] = sum_i sum_{k < M} h[o][i][k] y[n - k][i].
 * The arithmetic (output.filter_output_f32_ref gives these bits): the products of a binary32 tap and a binary32 sample are
 * exact in binary64; for each (n, o) they are added one by one from +0, i ascending (full form) and k ascending inside, in
 * binary64; the sum is rounded ONCE to binary32.  A frame outside the window is selected as 0 and never read; all M taps are
 * multiplied, zeros included, so a non-finite sample at (j, i) makes non-finite exactly the outputs j .. j + M - 1 of the
 * channels whose filter rows read channel i (0 x Inf is NaN): both in the full form, channel i alone in the diagonal one.
 *
 *   bas_output_filter_f32: ONE stateless function for whole signals, stream blocks and a stream's end.
 *     y + g y_stride_g + w y_stride_t + i y_stride_c is channel i of frame w of session g's window, w in [0, T_win).
 *     Everything outside the window is zero and is not read.  Output j, j in [0, T_out), is the one whose newest frame
 *     (k = 0) is frame first + j of the window; it is written to out + g out_stride_g + j out_stride_t + o out_stride_c.
 *     A whole signal of n frames is first = 0, T_win = n, T_out = n + M - 1.  A stream block of B frames is the same call on
 *     [history | block] with the history the session's last H >= M - 1 frames (zeros at a stream's start;
 *     bas_delay_carry_f32 of bas.h, stream-ordered behind this call, moves the last H frames to the front: correct for
 *     B < H too), first = H, T_win = H + B, T_out = B.  A stream's end is the call on the history alone: first = H,
 *     T_win = H, T_out = M - 1.  An output's bits depend on the frames of its own M-frame span alone: not on `first`, the
 *     block boundaries or how outputs are dealt to workgroups.
 *     taps + g taps_stride_g is session g's filter set (taps_stride_g = 0: one set for all; otherwise >= the set's floats);
 *     full != 0: [2][2][M], full == 0: [2][M].
 *     Any strides >= 0: frames [n][2] (y_stride_t = 2, y_stride_c = 1), planar [2][n], [G][..].  The output's strides must
 *     address every element once; window, taps and output must not overlap.
 *     One launch: one workgroup per (tile of BAS_OUTPUT_TILE frames, session); it stages the session's taps and its part
 *     of the window in LDS as binary64.
 *     Every argument check runs before the launch: 1 <= M <= 2048, 0 <= n_sessions <= 65535, 0 <= T_win < 2^31,
 *     0 <= first < 2^31, 0 <= T_out < 2^30, strides >= 0, below 2^40 (session) and 2^31 (frame, channel), taps_stride_g 0
 *     or >= the set's floats, the output addressing no element twice, no overlap (BAS_E_SHAPE); y (T_win > 0), taps, out
 *     required (BAS_E_NULL) and 4-byte aligned (BAS_E_ALIGN).  n_sessions or T_out of 0: nothing to do, no pointer is
 *     looked at. */
#ifndef BAS_OUTPUT_H
#define BAS_OUTPUT_H

#include "bas.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BAS_OUTPUT_TILE 576         /* output frames per workgroup (output.TILE) */
#define BAS_OUTPUT_MAX_TAPS 2048    /* M */

int bas_output_filter_f32(const float *y, long y_stride_g, long y_stride_t, long y_stride_c, int n_sessions, long T_win,
                          long first, const float *taps, long taps_stride_g, int M, int full, float *out,
                          long out_stride_g, long out_stride_t, long out_stride_c, long T_out, bas_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
