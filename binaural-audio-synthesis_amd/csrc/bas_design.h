// Colour design on the device (include/bas.h "colour design"): one filter's arithmetic, from the band
// log-magnitudes of one (row, boundary) to the first M taps of the minimum-phase response, in binary64.  One function for
// the kernel (bas_design.hip: a lane per filter, c and h in LDS with a lane stride) and for a host build (tests/hostsan:
// stride 1), so that the arithmetic can be checked on a machine without a GPU.
//
//   L[b] = max(logmag[b], floor)                      (a NaN reads as the floor)
//   c[m] = sum_b L[b] basis[b][m]                     fused multiply-adds from 0, b ascending
//   h[0] = exp(c[0]),  h[n] = (sum_{k=1..n} (k c[k]) h[n-k]) / n      fused multiply-adds from 0, k ascending
//
// Nothing depends on where the filter sits in a launch: equal inputs give equal bits.  propagation.min_phase_from_logmag is
// the numpy statement of the same three lines.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define BAS_DESIGN_MAX_BANDS 16
#define BAS_DESIGN_MAX_TAPS 64

// R terms of the recursion's sum, k ascending from the one c points at while h walks down: every load first, then the chain
// of fused multiply-adds.  The loads are what a lane waits for (the arrays sit in LDS on the device); issued together they
// cost one latency per R terms instead of one per term.  The order of the additions is the plain loop's.
template <int R>
__host__ __device__ inline double bas_design_terms(const double *c, long cs, const double *h, long hs, double acc) {
    double cv[R], hv[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        cv[i] = c[i * cs];
        hv[i] = h[-i * hs];
    }
#pragma unroll
    for (int i = 0; i < R; ++i) acc = fma(cv[i], hv[i], acc);
    return acc;
}

// c[m] = sum_b L[b] basis[b][m] (stored as m c[m] for m > 0) with the band count rounded up to NB: L[b] is 0 for
// b >= n_bands and those terms read the last band's row, so they add an exact zero and nothing is read outside the basis.
// No branch inside: the NB loads of a tap go out together (broadcasts on the device), then the chain, b ascending.
template <int NB>
__host__ __device__ inline void bas_design_compose(const double *L, const double *basis, int n_bands, int M, double *c,
                                                   long cs) {
    int row[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) row[b] = (b < n_bands ? b : n_bands - 1) * M;
#pragma unroll 2
    for (int m = 0; m < M; ++m) {
        double bv[NB], acc = 0.0;
#pragma unroll
        for (int b = 0; b < NB; ++b) bv[b] = basis[row[b] + m];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc = fma(L[b], bv[b], acc);
        c[m * cs] = m ? (double)m * acc : acc;
    }
}

// logmag: n_bands values (unit stride); basis: [n_bands][M]; c, h: M values each at element strides cs, hs (work space and
// result: h[n hs], n < M, are the taps; c is left holding c[0], 1 c[1], 2 c[2], ..).
__host__ __device__ inline void bas_design_filter(const double *logmag, const double *basis, int n_bands, int M,
                                                  double floor, double *c, long cs, double *h, long hs) {
    double L[BAS_DESIGN_MAX_BANDS];
#pragma unroll
    for (int b = 0; b < BAS_DESIGN_MAX_BANDS; ++b) L[b] = b < n_bands ? fmax(logmag[b], floor) : 0.0;
    switch ((n_bands + 3) >> 2) {
    case 1: bas_design_compose<4>(L, basis, n_bands, M, c, cs); break;
    case 2: bas_design_compose<8>(L, basis, n_bands, M, c, cs); break;
    case 3: bas_design_compose<12>(L, basis, n_bands, M, c, cs); break;
    default: bas_design_compose<16>(L, basis, n_bands, M, c, cs); break;
    }
    h[0] = exp(c[0]);
    for (int n = 1; n < M; ++n) {
        double acc = 0.0;
        int k = 1;
        for (; k + 8 <= n + 1; k += 8) acc = bas_design_terms<8>(c + k * cs, cs, h + (n - k) * hs, hs, acc);
        const int left = n + 1 - k;                                    // < 8 terms left (uniform over a wave)
        const double *cr = c + (left ? k : 0) * cs, *hr = h + (left ? n - k : 0) * hs;
        switch (left) {
        case 7: acc = bas_design_terms<7>(cr, cs, hr, hs, acc); break;
        case 6: acc = bas_design_terms<6>(cr, cs, hr, hs, acc); break;
        case 5: acc = bas_design_terms<5>(cr, cs, hr, hs, acc); break;
        case 4: acc = bas_design_terms<4>(cr, cs, hr, hs, acc); break;
        case 3: acc = bas_design_terms<3>(cr, cs, hr, hs, acc); break;
        case 2: acc = bas_design_terms<2>(cr, cs, hr, hs, acc); break;
        case 1: acc = bas_design_terms<1>(cr, cs, hr, hs, acc); break;
        default: break;
        }
        h[n * hs] = acc / (double)n;
    }
}
