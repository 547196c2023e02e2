// Look-ahead peak limiter, one gain for both ears (include/bas.h "look-ahead limiter"):
//   bas_limit_f32          - a whole signal, or one block of a stream with its carried history in front
//   bas_limit_state_floats - the carried state of one session
// No recursion: output j of a block is a function of the inputs j - (2 A + Hd) .. j, so a stream block that finds those
// samples in its history gives the whole signal's bits.
#include "bas_limit.h"

// the required gain of one stereo sample: ONE binary32 division
__device__ __forceinline__ float lim_required(f32x2 v, float c) {
    return lim_required_of(bas_peak_max(bas_peak_max(0.f, v.x), v.y), c);   // (a NaN in either ear: m NaN, r = 1, as np.abs(y).max(-1))
}

// One workgroup per (tile of LIM_TILE outputs, session).  Output u of the tile sits at block position j = j0 + u and is
// the limited sample of position j - A.  In LDS, index i is position j0 - H + i:
//   1. r over positions j0 - H .. j0 + Tcur - 1 (eight samples per thread are in flight together);
//   2. minima over 2^k neighbours by doubling between the two arrays (a minimum has no rounding), 2^k <= W = Hd + A + 1:
//      four neighbours in the first pass, then a quad of entries per thread and pass (16-byte LDS accesses; entries past
//      the end read as 1, the largest r there is);
//   3. e[q] = min r over [q, q + W): two overlapping power-of-two windows; q = 0 .. Tcur + A - 1;
//   4. s[u] = (e[u] + e[u + 1] + ... + e[u + A]) / (A + 1): sequential binary64 adds from +0, one binary64 division, one
//      rounding; a thread carries one chain per 256 outputs of the tile side by side;
//   5. g = min(s, r), out = clamp(y g), the meters;
//   6. (advance == 2: the session's only workgroup) the state moves forward here, behind a barrier that every read of the
//      ring has passed; with more tiles per session (advance == 1) a second launch does it.
__global__ __launch_bounds__(LIM_THREADS) void bas_limit_kernel(const float *__restrict__ y, long y_g, long y_t, long y_e,
                                                                long T_in, float *__restrict__ out, long o_g, long o_t,
                                                                long o_e, long T_out, int lead, float c, int A, int Hd,
                                                                float *state, long state_stride, int advance,
                                                                float *reduction, float *peak) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lim_lds[];
    const int tid = threadIdx.x, g = blockIdx.y;
    const int H = 2 * A + Hd, span = (H + LIM_TILE + 3) & ~3;            // (lim_span)
    float *P = lim_lds, *Q = lim_lds + span;
    const long o0 = (long)blockIdx.x * LIM_TILE;
    const int Tcur = (int)(T_out - o0 < LIM_TILE ? T_out - o0 : LIM_TILE);
    const long j0 = o0 + lead;
    const float *yg = T_in > 0 ? y + g * y_g : nullptr;
    int w;
    const f32x2 *ring = lim_ring(state, state_stride, g, H, advance, &w);
    const int len = H + Tcur, lenq = (len + 3) & ~3;
    for (int i0 = tid; i0 < lenq; i0 += 8 * LIM_THREADS) {
        f32x2 v[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int i = i0 + b * LIM_THREADS;
            v[b].x = v[b].y = 0.f;
            if (i < len) v[b] = lim_sample(yg, y_t, y_e, T_in, ring, H, w, j0 - H + i);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int i = i0 + b * LIM_THREADS;
            if (i < lenq) P[i] = lim_required(v[b], c);                  // (zeros past len: r = 1)
        }
    }
    __syncthreads();
    double acc[LIM_PER_THREAD];
    lim_window_sums(P, Q, lenq, A, Hd, Tcur, acc);
    f32x2 v[LIM_PER_THREAD];
    float req[LIM_PER_THREAD];
#pragma unroll
    for (int k = 0; k < LIM_PER_THREAD; ++k) {
        const int u = tid + k * LIM_THREADS;
        v[k].x = v[k].y = 0.f;
        if (u < Tcur) v[k] = lim_sample(yg, y_t, y_e, T_in, ring, H, w, j0 + u - A);
    }
#pragma unroll
    for (int k = 0; k < LIM_PER_THREAD; ++k) req[k] = lim_required(v[k], c);
    lim_epilogue(v, req, acc, A, c, Tcur, out + g * o_g + o0 * o_t, o_t, o_e, reduction, peak, g);
    if (advance == 2) {                                                  // (uniform; this workgroup alone reads this state)
        __syncthreads();                                                 // every value read from the ring has been used
        const int cnt = (int)(T_in < H ? T_in : H);
        for (int i = tid; i < cnt; i += LIM_THREADS) lim_carry(yg, y_t, y_e, T_in, H, w, state + g * state_stride, i, false);
        if (tid == 0) lim_carry(yg, y_t, y_e, T_in, H, w, state + g * state_stride, cnt, true);
    }
}

// The state moves forward behind a block of more than one tile (lim_carry_launch).
__global__ __launch_bounds__(LIM_THREADS) void bas_limit_carry_kernel(const float *__restrict__ y, long y_g, long y_t,
                                                                      long y_e, long T_in, int H, float *state,
                                                                      long state_stride) {
    lim_carry_launch(y, y_g, y_t, y_e, T_in, H, state, state_stride);
}

extern "C" size_t bas_limit_state_floats(int lookahead, int hold) {
    if (!lim_params_ok(lookahead, hold)) return 0;
    return (size_t)LIM_STATE_HEAD + 2 * (size_t)lim_history(lookahead, hold);
}

extern "C" int bas_limit_f32(const float *y, long y_stride_g, long y_stride_t, long y_stride_e, float *out,
                             long out_stride_g, long out_stride_t, long out_stride_e, int n_sessions, long T_in, long T_out,
                             double ceiling, int lookahead, int hold, float *state, long state_stride, float *reduction,
                             float *peak, bas_stream_t stream) {
    const int H = lim_history(lookahead, hold);
    float c;
    bool nothing;
    const int rc = lim_check("bas_limit_f32", y, y_stride_g, y_stride_t, y_stride_e, out, out_stride_g, out_stride_t,
                             out_stride_e, n_sessions, T_in, T_out, ceiling, lookahead, hold, state, state_stride, reduction,
                             peak, H, "bas_limit_state_floats", &c, &nothing);
    if (rc || nothing) return rc;
    const hipStream_t st = bas_stream(stream);
    const unsigned tiles = (unsigned)((T_out + LIM_TILE - 1) / LIM_TILE);
    // a block of one tile per session moves its state forward itself; longer blocks leave it to a second launch
    const int advance = !(state && T_in > 0 && H > 0) ? 0 : tiles == 1 ? 2 : 1;
    hipLaunchKernelGGL(bas_limit_kernel, dim3(tiles, (unsigned)n_sessions), dim3(LIM_THREADS), lim_lds_bytes(lookahead, hold),
                       st, y, y_stride_g, y_stride_t, y_stride_e, T_in, out, out_stride_g, out_stride_t, out_stride_e, T_out,
                       state ? 0 : lookahead, c, lookahead, hold, state, state_stride, advance, reduction, peak);
    if (advance == 1) {
        const long cnt = T_in < H ? T_in : H;
        hipLaunchKernelGGL(bas_limit_carry_kernel, dim3((unsigned)((cnt + LIM_THREADS - 1) / LIM_THREADS), (unsigned)n_sessions),
                           dim3(LIM_THREADS), 0, st, y, y_stride_g, y_stride_t, y_stride_e, T_in, H, state, state_stride);
    }
    return bas_check_launch("bas_limit_f32");
}
