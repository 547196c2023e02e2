// True-peak limiter (include/bas_limit_tp.h): the look-ahead limiter of bas_limit.hip behind a detector that
// reads the 4x oversampled signal, one gain for both ears:
//   bas_limit_tp_f32          - a whole signal, or one block of a stream with its carried history in front
//   bas_limit_tp_state_floats - the carried state of one session
// No recursion: output j of a block is a function of the inputs j - (2 A + Hd + 12) .. j, so a stream block that finds those
// samples in its history gives the whole signal's bits.
#include "bas_limit_tp.h"

// One workgroup per (tile of LIM_TILE outputs, session).  Output u of the tile sits at block position j = j0 + u and is the
// limited sample of position j - A - 6.  With jr = j0 - 6, r index i is position jr - H + i (H = 2 A + Hd), exactly
// bas_limit_kernel's image with jr for its j0, and raw index k is position jr - H - 6 + k: the sample of r index i is raw
// index i + 6.
//   0. both ears of positions jr - H - 6 .. jr - H + lenq + 5 into the two arrays, left in P and right in Q, from the block,
//      the ring or zeros (eight frames per thread are in flight together);
//   1. d and r in place: a thread takes four consecutive r indices i0 .. i0 + 3, reads raw i0 .. i0 + 15 of each ear (four
//      16-byte LDS reads), forms the five interpolated positions i0 - 1 .. i0 + 3 (window t: raw i0 + t .. i0 + t + 11; 3 x 12
//      binary64 multiply-adds each and ear, the products exact), and d from |y| and two neighbouring positions.  r index i
//      takes the place of raw index i, which only r indices <= i read: the workgroup walks the indices upwards in chunks of
//      1024, and a barrier stands between a chunk's reads and its writes;
//   2. - 5. bas_limit_kernel's steps 2 to 5 (lim_window_sums, lim_epilogue), the required gain of an output read back from
//      P before the minimum passes overwrite it;
//   6. the state moves forward as there, the ring holding H + 12 frames.
__global__ __launch_bounds__(LIM_THREADS) void bas_limit_tp_kernel(const float *__restrict__ y, long y_g, long y_t, long y_e,
                                                                   long T_in, float *__restrict__ out, long o_g, long o_t,
                                                                   long o_e, long T_out, int lead, float c, int A, int Hd,
                                                                   float *state, long state_stride, int advance,
                                                                   float *reduction, float *peak) {
    extern __shared__ __attribute__((aligned(16))) float lim_tp_lds[];
    const int tid = threadIdx.x, g = blockIdx.y;
    const int H = 2 * A + Hd, HT = H + 2 * LIM_TP_REACH;
    const int span = ((H + LIM_TILE + 3) & ~3) + 2 * LIM_TP_REACH;       // (lim_tp_span)
    float *P = lim_tp_lds, *Q = lim_tp_lds + span;
    const long o0 = (long)blockIdx.x * LIM_TILE;
    const int Tcur = (int)(T_out - o0 < LIM_TILE ? T_out - o0 : LIM_TILE);
    const long jr = o0 + lead - LIM_TP_REACH;
    const float *yg = T_in > 0 ? y + g * y_g : nullptr;
    int w;
    const f32x2 *ring = lim_ring(state, state_stride, g, HT, advance, &w);
    const int len = H + Tcur, lenq = (len + 3) & ~3, nraw = lenq + 2 * LIM_TP_REACH;     // nraw <= span
    const long p0 = jr - H - LIM_TP_REACH;                               // (>= -HT: inside the ring)
    for (int k0 = tid; k0 < nraw; k0 += 8 * LIM_THREADS) {
        f32x2 v[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int k = k0 + b * LIM_THREADS;
            v[b].x = v[b].y = 0.f;
            if (k < nraw) v[b] = lim_sample(yg, y_t, y_e, T_in, ring, HT, w, p0 + k);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int k = k0 + b * LIM_THREADS;
            if (k < nraw) {
                P[k] = v[b].x;
                Q[k] = v[b].y;
            }
        }
    }
    __syncthreads();
    constexpr float taps[LIM_TP_PHASES * LIM_TP_TAPS] = LIM_TP_TAP_VALUES;
    for (int c0 = 0; c0 < lenq; c0 += 4 * LIM_THREADS) {                 // (uniform)
        const int i0 = c0 + 4 * tid;
        f32x4 rq = {1.0f, 1.0f, 1.0f, 1.0f};
        if (i0 < lenq) {
            float U[LIM_TP_QUAD_WINDOWS], m[4];
#pragma unroll
            for (int t = 0; t < LIM_TP_QUAD_WINDOWS; ++t) U[t] = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) m[q] = 0.f;
#pragma unroll
            for (int ear = 0; ear < 2; ++ear) {
                const float *X = (ear ? Q : P) + i0;
                double x[16];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(X + 4 * b);
                    x[4 * b] = (double)a.x;
                    x[4 * b + 1] = (double)a.y;
                    x[4 * b + 2] = (double)a.z;
                    x[4 * b + 3] = (double)a.w;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) m[q] = bas_peak_max(m[q], (float)x[q + LIM_TP_REACH]);
#pragma unroll
                for (int t = 0; t < LIM_TP_QUAD_WINDOWS; ++t) {
#pragma unroll
                    for (int p = 0; p < LIM_TP_PHASES; ++p) {
                        double s = 0.0;
#pragma unroll
                        for (int k = 0; k < LIM_TP_TAPS; ++k) s = __builtin_fma(x[t + k], (double)taps[p * LIM_TP_TAPS + k], s);
                        U[t] = bas_peak_max(U[t], (float)s);
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float d = bas_peak_max(bas_peak_max(m[q], U[q]), U[q + 1]);
                rq[q] = i0 + q < len ? lim_required_of(d, c) : 1.0f;     // (past len: r = 1, no window reaches it)
            }
        }
        __syncthreads();                                                 // every read of this chunk's raw samples is done
        if (i0 < lenq) *reinterpret_cast<f32x4 *>(P + i0) = rq;
    }
    __syncthreads();
    float req[LIM_PER_THREAD];
#pragma unroll
    for (int k = 0; k < LIM_PER_THREAD; ++k) {
        const int u = tid + k * LIM_THREADS;
        req[k] = u < Tcur ? P[H - A + u] : 1.0f;                         // r of position jr + u - A
    }
    double acc[LIM_PER_THREAD];
    lim_window_sums(P, Q, lenq, A, Hd, Tcur, acc);
    f32x2 v[LIM_PER_THREAD];
#pragma unroll
    for (int k = 0; k < LIM_PER_THREAD; ++k) {
        const int u = tid + k * LIM_THREADS;
        v[k].x = v[k].y = 0.f;
        if (u < Tcur) v[k] = lim_sample(yg, y_t, y_e, T_in, ring, HT, w, jr + u - A);
    }
    lim_epilogue(v, req, acc, A, c, Tcur, out + g * o_g + o0 * o_t, o_t, o_e, reduction, peak, g);
    if (advance == 2) {                                                  // (uniform; this workgroup alone reads this state)
        __syncthreads();                                                 // every value read from the ring has been used
        const int cnt = (int)(T_in < HT ? T_in : HT);
        for (int i = tid; i < cnt; i += LIM_THREADS) lim_carry(yg, y_t, y_e, T_in, HT, w, state + g * state_stride, i, false);
        if (tid == 0) lim_carry(yg, y_t, y_e, T_in, HT, w, state + g * state_stride, cnt, true);
    }
}

// The state moves forward behind a block of more than one tile (lim_carry_launch).
__global__ __launch_bounds__(LIM_THREADS) void bas_limit_tp_carry_kernel(const float *__restrict__ y, long y_g, long y_t,
                                                                         long y_e, long T_in, int H, float *state,
                                                                         long state_stride) {
    lim_carry_launch(y, y_g, y_t, y_e, T_in, H, state, state_stride);
}

extern "C" size_t bas_limit_tp_state_floats(int lookahead, int hold) {
    if (!lim_params_ok(lookahead, hold)) return 0;
    return (size_t)LIM_STATE_HEAD + 2 * (size_t)lim_tp_history(lookahead, hold);
}

extern "C" int bas_limit_tp_f32(const float *y, long y_stride_g, long y_stride_t, long y_stride_e, float *out,
                                long out_stride_g, long out_stride_t, long out_stride_e, int n_sessions, long T_in,
                                long T_out, double ceiling, int lookahead, int hold, float *state, long state_stride,
                                float *reduction, float *peak, bas_stream_t stream) {
    // (out of range: lim_check refuses the call before HT is used)
    const int HT = lim_params_ok(lookahead, hold) ? lim_tp_history(lookahead, hold) : 0;
    float c;
    bool nothing;
    const int rc = lim_check("bas_limit_tp_f32", y, y_stride_g, y_stride_t, y_stride_e, out, out_stride_g, out_stride_t,
                             out_stride_e, n_sessions, T_in, T_out, ceiling, lookahead, hold, state, state_stride, reduction,
                             peak, HT, "bas_limit_tp_state_floats", &c, &nothing);
    if (rc || nothing) return rc;
    const hipStream_t st = bas_stream(stream);
    const unsigned tiles = (unsigned)((T_out + LIM_TILE - 1) / LIM_TILE);
    // a block of one tile per session moves its state forward itself; longer blocks leave it to a second launch
    const int advance = lim_tp_advance(state != nullptr, T_in, T_out);
    hipLaunchKernelGGL(bas_limit_tp_kernel, dim3(tiles, (unsigned)n_sessions), dim3(LIM_THREADS),
                       lim_tp_lds_bytes(lookahead, hold), st, y, y_stride_g, y_stride_t, y_stride_e, T_in, out, out_stride_g,
                       out_stride_t, out_stride_e, T_out, state ? 0 : lim_tp_latency(lookahead), c, lookahead, hold, state,
                       state_stride, advance, reduction, peak);
    if (advance == 1) {
        const long cnt = T_in < HT ? T_in : HT;
        hipLaunchKernelGGL(bas_limit_tp_carry_kernel,
                           dim3((unsigned)((cnt + LIM_THREADS - 1) / LIM_THREADS), (unsigned)n_sessions), dim3(LIM_THREADS), 0,
                           st, y, y_stride_g, y_stride_t, y_stride_e, T_in, HT, state, state_stride);
    }
    return bas_check_launch("bas_limit_tp_f32");
}
