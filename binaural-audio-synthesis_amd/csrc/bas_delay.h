// Per-source propagation delay: the one device function that computes a delayed input sample
// (bas_delay_sample_tap; the two readers below wrap it).  Every caller - bas_delay_rows_f32 (bas_delay.hip), the batch pack
// (bas_batch.hip) and the stream-batch pack (bas_stream_batch.hip) - inlines it, so every path produces the same bits.
#pragma once
#include "bas_internal.h"

#define BAS_DELAY_LINEAR 0
#define BAS_DELAY_CUBIC 1

// the smallest delay an interpolator can take without reading a sample later than t (linear: 1, cubic: 2)
__device__ __forceinline__ double bas_delay_min(int interp) { return interp == BAS_DELAY_CUBIC ? 2.0 : 1.0; }

// x'(kK + j), 0 <= j < K, with d(t) = d0 + (j/K)(d1 - d0) clamped to [dmin, dmax] (fmax(fmin(.)): NaN reads as dmax).
// tap(i) returns input sample i (0 outside the readable range).  The position arithmetic is relative to the chunk start kK,
// so the result depends only on (j, K, d0, d1) and the input values, never on the absolute time.  Contraction is off: the
// product form of the weights and the sum are evaluated exactly as written (and as the float64 host definition,
// propagation.delayed_inputs, evaluates them) in every kernel the function is inlined into.
template <class Tap>
__device__ __forceinline__ float bas_delay_sample_tap(const Tap &tap, long kK, int j, int K, double d0, double d1,
                                                      double dmin, double dmax, int interp) {
#pragma clang fp contract(off)
    double d = d0 + ((double)j / (double)K) * (d1 - d0);
    d = fmax(fmin(d, dmax), dmin);
    const double u = (double)j - d;
    const double fl = floor(u);
    const double f = u - fl;
    const long i = kK + (long)fl;
    const double x0 = tap(i);
    const double x1 = tap(i + 1);
    if (interp == BAS_DELAY_CUBIC) {
        const double xm = tap(i - 1);
        const double x2 = tap(i + 2);
        const double cm = -f * (f - 1.0) * (f - 2.0) / 6.0;
        const double c0 = (f + 1.0) * (f - 1.0) * (f - 2.0) / 2.0;
        const double c1 = -(f + 1.0) * f * (f - 2.0) / 2.0;
        const double c2 = (f + 1.0) * f * (f - 1.0) / 6.0;
        return (float)(cm * xm + c0 * x0 + c1 * x1 + c2 * x2);
    }
    return (float)((1.0 - f) * x0 + f * x1);
}

// One row: row points at the source's sample 0; samples [lo, hi) are readable, every other one is 0.
__device__ __forceinline__ float bas_delay_sample(const float *__restrict__ row, long lo, long hi, long kK, int j, int K,
                                                  double d0, double d1, double dmin, double dmax, int interp) {
    const auto tap = [row, lo, hi](long i) -> double { return (i >= lo && i < hi) ? (double)row[i] : 0.0; };
    return bas_delay_sample_tap(tap, kK, j, K, d0, d1, dmin, dmax, interp);
}

// Two pieces (a stream block beside its carried history): samples -H .. -1 are hist[0 .. H), samples 0 .. B-1 are
// blk[0 .. B); every other one is 0.  The same arithmetic and the same bits as bas_delay_sample on [hist | blk].
__device__ __forceinline__ float bas_delay_sample_split(const float *__restrict__ hist, int H, const float *__restrict__ blk,
                                                        long B, long kK, int j, int K, double d0, double d1, double dmin,
                                                        double dmax, int interp) {
    const auto tap = [hist, H, blk, B](long i) -> double {
        return i < 0 ? (i >= -(long)H ? (double)hist[H + i] : 0.0) : (i < B ? (double)blk[i] : 0.0);
    };
    return bas_delay_sample_tap(tap, kK, j, K, d0, d1, dmin, dmax, interp);
}
