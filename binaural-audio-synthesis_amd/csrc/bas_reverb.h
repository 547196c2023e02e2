// The device FFT of the long-FIR convolver (bas_reverb.hip): one transform of N = 2 Np <= 1024 complex
// points in the LDS of one workgroup of Np threads, radix 2, self-sorting (Stockham: two buffers, no bit reversal).
#pragma once
#include "bas_internal.h"

#define RV_MAX_NP 512
#define RV_MIN_NP 32
#define RV_MAX_LR (1 << 17)
#define RV_MAX_LAG (1 << 20)

// 8 + 8 + 4 KiB: the two buffers a stage reads and writes, and the twiddles w[m] = exp(-2 pi i m / N), m < Np (binary32
// roundings of binary64 values: made once per tail by bas_long_fir_tail_f32 with sincospi, read from there afterwards)
struct RvFft {
    f32x2 a[2 * RV_MAX_NP];
    f32x2 b[2 * RV_MAX_NP];
    f32x2 tw[RV_MAX_NP];
};

// w b, every operation written out: (wr br - wi bi, wr bi + wi br), one product rounded and one fused multiply-add each
__device__ __forceinline__ f32x2 rv_cmul(f32x2 w, f32x2 b) {
    f32x2 r;
    r.x = fmaf(-w.y, b.y, w.x * b.x);
    r.y = fmaf(w.y, b.x, w.x * b.y);
    return r;
}

// The transform of s.a by the Np threads of the workgroup (all of them call it; blockDim.x == Np, a power of two).  The
// caller has written s.a and s.tw (no barrier needed in between: the first stage starts with one).  INV: the conjugate
// twiddles, no scaling.  Returns the buffer that holds the result (s.a or s.b), visible to every thread.  Stage Ns joins
// the transforms of Ns points into those of 2 Ns: thread j takes x[j] and x[j + Np], writes y[j0] and y[j0 + Ns] with
// k = j mod Ns, j0 = 2 (j - k) + k.  A zero input gives +0 everywhere (x[j] = +0 absorbs a product of either sign).
template <bool INV>
__device__ __forceinline__ f32x2 *rv_fft(RvFft &s, int Np) {
    const int j = threadIdx.x;
    f32x2 *x = s.a, *y = s.b;
    int step = Np;                                         // Np / Ns: the twiddle of (k, Ns) is w[k Np / Ns]
    for (int Ns = 1; Ns <= Np; Ns <<= 1, step >>= 1) {
        __syncthreads();
        const int k = j & (Ns - 1);
        f32x2 w = s.tw[k * step];
        if (INV) w.y = -w.y;
        const f32x2 a = x[j];
        const f32x2 b = rv_cmul(w, x[j + Np]);
        const int j0 = ((j - k) << 1) + k;
        y[j0] = a + b;
        y[j0 + Ns] = a - b;
        f32x2 *t = x;
        x = y;
        y = t;
    }
    __syncthreads();
    return x;
}
