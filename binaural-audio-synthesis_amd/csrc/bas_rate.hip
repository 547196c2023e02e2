// Sample-rate conversion by a rational ratio p / q (include/bas_rate.h):
//   bas_rate_convert_f32                  - a whole signal, a block of a stream on [history | block], or a stream's end
//   bas_rate_produced, bas_rate_needed    - the stream counts (host arithmetic of bas_rate.h)
// Output m is sum_k T[ph][k] x~[b + K0 - k] with b = floor(m q / p), ph = m q mod p: N products of two binary32 values,
// exact in binary64, added from +0 with k ascending in binary64, rounded once.  No state: what a stream carries is samples.
#include "bas_rate.h"

// The sums of NJ outputs per thread (outputs tid + j RATE_THREADS of the tile), side by side: every chain takes its terms in
// ascending k.  X_LDS: xs[j] points at the chain's newest sample in the staged window and the samples lie behind it.
// Otherwise the chain reads the row itself: w[j] is the newest sample's index in the window [0, T_win), a sample outside it
// is selected as 0 and not read.
template <bool X_LDS, int NJ>
__device__ __forceinline__ void rate_sums(const float *const *ts, const float *const *xs, const float *__restrict__ xr,
                                          long x_t, long T_win, const long *w, int N, double *acc) {
    double a[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) a[j] = 0.0;
#pragma unroll 4
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float v;
            if (X_LDS) {
                v = xs[j][-k];
            } else {
                const long i = w[j] - k;
                v = (i >= 0 && i < T_win) ? xr[i * x_t] : 0.f;
            }
            a[j] = fma((double)ts[j][k], (double)v, a[j]);               // (an exact product: fma or multiply-then-add, same bits)
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = a[j];
}

// One workgroup per (tile of RATE_TILE outputs, row, group).  The tile's first output is m_a = m0 + tile RATE_TILE with
// m_a q = b_a p + r_a; output u of the tile has m q = b_a p + (r_a + u q), so b = b_a + d, ph = (r_a + u q) - d p with
// d = (r_a + u q) / p: 32-bit arithmetic (r_a + u q < 2^12 + 2^9 2^12).  Its samples have the absolute indices
// b + K0 - k, k < N; slot i of the staged window holds absolute index b_a + K0 - (N - 1) + i, so the chain reads slots
// d + N - 1 - k: [d, d + N - 1], inside the d_last + N slots staged.
//   X_LDS  the window's part is staged in LDS (zeros selected outside [0, T_win)); else it is read from the row;
//   T_LDS  the taps are staged behind it, rows `pitch` floats apart (rate_pitch); else they are read from the table.
template <bool X_LDS, bool T_LDS>
__global__ __launch_bounds__(RATE_THREADS) void bas_rate_kernel(const float *__restrict__ x, long x_g, long x_r, long x_t,
                                                                long T_win, long t0, const float *__restrict__ taps, int p,
                                                                int q, int N, int K0, int pitch, int x_floats,
                                                                float *__restrict__ out, long o_g, long o_r, long o_t,
                                                                long m0, long T_out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float rate_lds[];
    const int tid = threadIdx.x;
    const long o0 = (long)blockIdx.x * RATE_TILE;
    const int Tcur = (int)(T_out - o0 < RATE_TILE ? T_out - o0 : RATE_TILE);
    const long mq = (m0 + o0) * q;                                       // <= 2^50 2^12
    const long b_a = mq / p;
    const int r_a = (int)(mq - b_a * p);
    const float *xr = x + blockIdx.z * x_g + blockIdx.y * x_r;
    float *orow = out + blockIdx.z * o_g + blockIdx.y * o_r;
    const long lo = b_a + K0 - (N - 1) - t0;                             // slot 0 as an index into the window
    float *X = rate_lds, *Tl = rate_lds + x_floats;
    if (X_LDS) {
        const int slots = (r_a + (Tcur - 1) * q) / p + N;                // <= rate_window_floats
        for (int i = tid; i < slots; i += RATE_THREADS) {
            const long w = lo + i;
            X[i] = (w >= 0 && w < T_win) ? xr[w * x_t] : 0.f;
        }
    }
    if (T_LDS) {                                     // element i = ph N + k, walked without a division; eight loads of a
        int ph = tid / N, k = tid - ph * N;          // thread are in flight together (147 / 160 over 10 s: 3.05 ms against
        const int dph = RATE_THREADS / N, dk = RATE_THREADS - dph * N, total = p * N;   // 3.39 one by one; 160 / 147: 2.91, 2.84)
        for (int i0 = tid; i0 < total; i0 += 8 * RATE_THREADS) {
            float v[8];
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int i = i0 + b * RATE_THREADS;
                v[b] = i < total ? taps[i] : 0.f;
            }
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                if (i0 + b * RATE_THREADS < total) Tl[ph * pitch + k] = v[b];
                ph += dph;
                k += dk;
                if (k >= N) {
                    k -= N;
                    ++ph;
                }
            }
        }
    }
    if (X_LDS || T_LDS) __syncthreads();
    const float *ts[RATE_PER_THREAD], *xs[RATE_PER_THREAD];
    long w[RATE_PER_THREAD];
#pragma unroll
    for (int j = 0; j < RATE_PER_THREAD; ++j) {
        int u = tid + j * RATE_THREADS;
        if (u >= Tcur) u = Tcur - 1;                                     // (an idle chain repeats the tile's last output)
        const int v = r_a + u * q, d = v / p, ph = v - d * p;
        ts[j] = T_LDS ? Tl + ph * pitch : taps + ph * N;
        xs[j] = X + d + (N - 1);
        w[j] = lo + d + (N - 1);
    }
    double acc[RATE_PER_THREAD];
    if (Tcur <= RATE_THREADS) rate_sums<X_LDS, 1>(ts, xs, xr, x_t, T_win, w, N, acc);
    else rate_sums<X_LDS, RATE_PER_THREAD>(ts, xs, xr, x_t, T_win, w, N, acc);
#pragma unroll
    for (int j = 0; j < RATE_PER_THREAD; ++j) {
        const int u = tid + j * RATE_THREADS;
        if (u < Tcur) orow[(o0 + u) * o_t] = (float)acc[j];              // the ONE rounding
    }
}

extern "C" long bas_rate_produced(long n_in, int p, int q, int K0) { return rate_produced(n_in, p, q, K0); }
extern "C" long bas_rate_needed(long m_out, int p, int q, int K0) { return rate_needed(m_out, p, q, K0); }

template <bool X_LDS, bool T_LDS>
static void rate_launch(dim3 grid, const RatePlan &P, hipStream_t st, const float *x, long x_g, long x_r, long x_t,
                        long T_win, long t0, const float *taps, int p, int q, int N, int K0, float *out, long o_g, long o_r,
                        long o_t, long m0, long T_out) {
    hipLaunchKernelGGL((bas_rate_kernel<X_LDS, T_LDS>), grid, dim3(RATE_THREADS), P.lds_bytes, st, x, x_g, x_r, x_t, T_win,
                       t0, taps, p, q, N, K0, P.pitch, P.x_floats, out, o_g, o_r, o_t, m0, T_out);
}

extern "C" int bas_rate_convert_f32(const float *x, long x_stride_g, long x_stride_r, long x_stride_t, int n_groups,
                                    int n_rows, long T_win, long t0, const float *taps, int p, int q, int N, int K0,
                                    float *out, long out_stride_g, long out_stride_r, long out_stride_t, long m0, long T_out,
                                    bas_stream_t stream) {
    BAS_REQUIRE(p >= 1 && p <= BAS_RATE_MAX_RATIO && q >= 1 && q <= BAS_RATE_MAX_RATIO, BAS_E_SHAPE,
                "bas_rate_convert_f32: p (%d) and q (%d) must be in 1..%d", p, q, BAS_RATE_MAX_RATIO);
    BAS_REQUIRE(N >= 1 && N <= BAS_RATE_MAX_TAPS && (long)p * N <= BAS_RATE_MAX_TABLE, BAS_E_SHAPE,
                "bas_rate_convert_f32: N (%d) must be in 1..%d with p N <= %d", N, BAS_RATE_MAX_TAPS, BAS_RATE_MAX_TABLE);
    BAS_REQUIRE(K0 >= 0 && K0 < N, BAS_E_SHAPE, "bas_rate_convert_f32: K0 (%d) must be in 0..N - 1", K0);
    BAS_REQUIRE(n_groups >= 0 && n_groups <= 65535 && n_rows >= 0 && n_rows <= 65535, BAS_E_SHAPE,
                "bas_rate_convert_f32: n_groups (%d) and n_rows (%d) must be in 0..65535", n_groups, n_rows);
    BAS_REQUIRE(T_win >= 0 && T_win < (1L << 31), BAS_E_SHAPE, "bas_rate_convert_f32: T_win (%ld) must be in 0..2^31 - 1", T_win);
    BAS_REQUIRE(t0 >= -(1L << 50) && t0 <= (1L << 62), BAS_E_SHAPE, "bas_rate_convert_f32: t0 (%ld) must be in -2^50..2^62", t0);
    BAS_REQUIRE(T_out >= 0 && T_out < (1L << 30), BAS_E_SHAPE, "bas_rate_convert_f32: T_out (%ld) must be in 0..2^30 - 1", T_out);
    BAS_REQUIRE(m0 >= 0 && m0 <= (1L << 50) - T_out, BAS_E_SHAPE,
                "bas_rate_convert_f32: m0 (%ld) must be >= 0 with m0 + T_out <= 2^50", m0);
    BAS_REQUIRE(bas_none_negative({x_stride_g, x_stride_r, x_stride_t, out_stride_g, out_stride_r, out_stride_t}), BAS_E_SHAPE,
                "bas_rate_convert_f32: strides must be >= 0");
    BAS_REQUIRE(bas_all_below(1L << 40, {x_stride_g, x_stride_r, out_stride_g, out_stride_r}) &&
                    bas_all_below(1L << 31, {x_stride_t, out_stride_t}),
                BAS_E_SHAPE, "bas_rate_convert_f32: strides must be below 2^40 (group, row) and 2^31 (sample)");
    if (n_groups == 0 || n_rows == 0 || T_out == 0) return 0;
    BAS_REQUIRE(out && taps && (x || T_win == 0), BAS_E_NULL, "bas_rate_convert_f32: null pointer");
    BAS_REQUIRE(bas_aligned(x, 4) && bas_aligned(taps, 4) && bas_aligned(out, 4), BAS_E_ALIGN,
                "bas_rate_convert_f32: x, taps and out must be 4-byte aligned");
    const long in_extent[3] = {n_groups, n_rows, T_win}, in_stride[3] = {x_stride_g, x_stride_r, x_stride_t};
    const long out_extent[3] = {n_groups, n_rows, T_out}, out_stride[3] = {out_stride_g, out_stride_r, out_stride_t};
    BAS_REQUIRE(bas_layout_nested(3, out_extent, out_stride), BAS_E_SHAPE,
                "bas_rate_convert_f32: the output's strides address an element twice");
    const size_t out_bytes = 4 * (size_t)bas_view_extent(3, out_extent, out_stride);
    BAS_REQUIRE(T_win == 0 || !bas_ranges_meet(x, 4 * (size_t)bas_view_extent(3, in_extent, in_stride), out, out_bytes),
                BAS_E_SHAPE, "bas_rate_convert_f32: input and output overlap");
    BAS_REQUIRE(!bas_ranges_meet(taps, 4 * (size_t)p * N, out, out_bytes), BAS_E_SHAPE,
                "bas_rate_convert_f32: taps and output overlap");
    const RatePlan P = rate_plan(p, q, N);
    const dim3 grid((unsigned)((T_out + RATE_TILE - 1) / RATE_TILE), (unsigned)n_rows, (unsigned)n_groups);
    const hipStream_t st = bas_stream(stream);
#define RATE_LAUNCH(XL, TL)                                                                                               \
    rate_launch<XL, TL>(grid, P, st, x, x_stride_g, x_stride_r, x_stride_t, T_win, t0, taps, p, q, N, K0, out, out_stride_g, \
                        out_stride_r, out_stride_t, m0, T_out)
    if (P.x_lds && P.t_lds) RATE_LAUNCH(true, true);
    else if (P.x_lds) RATE_LAUNCH(true, false);
    else if (P.t_lds) RATE_LAUNCH(false, true);
    else RATE_LAUNCH(false, false);
#undef RATE_LAUNCH
    return bas_check_launch("bas_rate_convert_f32");
}
