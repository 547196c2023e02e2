/* bas_limit_tp.h - the true-peak limiter of libbas_hip.so, beside the ABI of bas.h: the same conventions
 * (device pointers, one stream, no allocation, no synchronisation, 0 / BAS_E_* / hipError_t, the text of bas_last_error),
 * the same library, BAS_ABI_VERSION untouched.  The reference has no counterpart.
 *
 * ---- the limiter ------------------------------------------------------------------------------------------------------
 * bas_limit_f32 of bas.h bounds the samples; the waveform a converter or a resampler rebuilds between them can pass the
 * ceiling.  This stage takes its required gain from the 4x oversampled signal - the interpolation of the meter (bas.h
 * "loudness meter") - and is the look-ahead limiter from there on.  For a ceiling c, a look-ahead of A and
 * a hold of Hd samples (the ranges of bas.h), float32 stereo frames y[n], zeros before and after the signal:
 *   0. u_p[m], p = 1, 2, 3, per ear: the value at time m + p/4, the 12 products y[m + j] g_p[j], j = -5 .. 6, exact in
 *      binary64, added one by one from +0 with j ascending and rounded ONCE to binary32.  g_p[j] are the meter's taps
 *      (loudness.true_peak_taps()); the library holds their bits;
 *   1. d[n] = the maximum over both ears of |y[n]|, |u_p[n]| and |u_p[n - 1]|, p = 1 .. 3: the largest value on the 4x grid
 *      in the open interval (n - 1, n + 1).  Exact, and ONE value for both ears;
 *   2. r[n] = d[n] > c ? c / d[n] : 1                          (one binary32 division), for EVERY n: r is below 1 up to 6
 *      samples in front of a signal that starts loud, and behind one that ends loud;
 *   3. - 6. steps 3 to 6 of bas_limit_f32: e[k] = min r[j] over [k - Hd, k + A]; s[n] the mean of e[n - A .. n] (binary64
 *      adds from +0 with k ascending, one division, one rounding); g[n] = min(s[n], r[n]); out[n] = min(max(y[n] g[n], -c), c).
 * out[n] depends on y[n - A - Hd - 6 .. n + A + 6] and on nothing else; there is no recursion, so a stream gives the whole
 * signal's bits whatever its block lengths.  limiter.limit_tp_f32_ref gives these bits.
 *   |out[n]| <= c exactly, since d >= |y|.  A signal whose true peak (the meter's reading) is at most c passes with its own
 *   bits and g = 1.  Where g is constant over a 12-sample window the window's interpolated output is g times the input's
 *   up to rounding; where g moves inside a window there is no a-priori bound on the output's true peak (DESIGN.md §3.27
 *   quotes what was measured).
 * Non-finite inputs: for ANY input bits every output is finite and |out| <= c.  The maxima are taken on
 * the bit patterns, so a NaN that reaches d[n] - a NaN or an infinite frame within 6 samples of n - gives d = NaN and r = 1
 * or d = Inf and r = 0; the frames whose d it reaches and what steps 3 to 5 spread from them are not specified; a
 * non-finite product in step 6 leaves as -c.  No other session's outputs, meters or state change.
 *
 *   bas_limit_tp_state_floats(A, Hd) = 4 + 2 (2 A + Hd + 12) floats per session (0 for parameters out of range): two ring
 *     positions, two spare words, and the session's last 2 A + Hd + 12 frames - samples only.
 *   bas_limit_tp_f32: the parameter list and every convention of bas_limit_f32 (strided y and out, any strides >= 0, the
 *     output addressing every element once, no overlap of input, output and state; reduction and peak meters, each may be
 *     NULL).
 *     state == NULL: a whole signal.  T_in == T_out; out[n] belongs to y[n].
 *     state != NULL: a block of a stream, the state zeroed before its first block.  out[j] is the limited sample of time
 *     t0 + j - A - 6 for a block that starts at t0: the stream is A + 6 samples late and begins with A + 6 zeros.
 *     T_in == T_out: a block, whose last min(T_in, 2 A + Hd + 12) frames then go into the ring - by the session's own
 *     workgroup where the block is one tile (1024 samples) or less, by a second launch where it is longer.  T_in == 0: the
 *     stream's end - T_out (usually A + 6) more samples with zeros behind the history; the state is left as it is, y is
 *     not read.  Any block length >= 1.
 * One stream, no allocation, no synchronisation (capturable: the ring's position lives on the device); one launch, two
 * for a stream block of more than 1024 samples.  Every argument check of bas_limit_f32 runs before any launch, with the
 * same codes; state_stride must be a multiple of 4 and >= bas_limit_tp_state_floats. */
#ifndef BAS_LIMIT_TP_H
#define BAS_LIMIT_TP_H

#include "bas.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t bas_limit_tp_state_floats(int lookahead, int hold);
int bas_limit_tp_f32(const float *y, long y_stride_g, long y_stride_t, long y_stride_e, float *out, long out_stride_g,
                     long out_stride_t, long out_stride_e, int n_sessions, long T_in, long T_out, double ceiling,
                     int lookahead, int hold, float *state, long state_stride, float *reduction, float *peak,
                     bas_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
