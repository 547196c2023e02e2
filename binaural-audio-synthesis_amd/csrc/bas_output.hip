// The stereo output filter (include/bas_output.h):
//   bas_output_filter_f32   - a whole signal, a block of a stream on [history | block], or a stream's end
// Output (n, o) is sum_i sum_k h[o][i][k] y[n - k][i]: products of two binary32 values, exact in binary64, added from +0 with
// i ascending and k ascending inside in binary64, rounded once.  No state: what a stream carries is frames.
#include "bas_output.h"

// One pass over the M taps of one input channel for the thread's OUT_U consecutive frames: NO chains per frame (both output
// channels in the full form, one in the diagonal form).  xp points at the staged sample of the thread's first frame at
// k = 0 and the older samples lie in front of it: with a[m] = xp[-m], frame u takes a[k - u] at step k, so a step needs ONE
// new sample, a[k], and the frames' window slides.  tp points at the pass's taps, NO per step (wave-uniform: LDS broadcasts).
// The steps run in blocks of OUT_KB whose samples and taps are read together, one block ahead of the block being summed (A
// and B take turns, so the window slides by register names); what M leaves over runs one step at a time.  Every chain
// takes its terms with k ascending.
template <int NO>
struct OutBlock {
    double s[OUT_KB], t[OUT_KB][NO];
};

template <int NO>
__device__ __forceinline__ void out_load(OutBlock<NO> &b, const double *xk, const double *tk) {
#pragma unroll
    for (int j = 0; j < OUT_KB; ++j) {
        b.s[j] = xk[-j];
        if (NO == 2) {
            const double2 t = reinterpret_cast<const double2 *>(tk)[j];      // (16-byte aligned: the taps start the LDS image)
            b.t[j][0] = t.x;
            b.t[j][NO - 1] = t.y;
        } else {
            b.t[j][0] = tk[j];
        }
    }
}

// tail[v] = a[k - 1 - v]: the samples the frames u > 0 still need from before the block
template <int NO>
__device__ __forceinline__ void out_sum(const OutBlock<NO> &b, double (&tail)[OUT_U - 1], double (&acc)[OUT_U][NO]) {
#pragma unroll
    for (int j = 0; j < OUT_KB; ++j) {
#pragma unroll
        for (int u = 0; u < OUT_U; ++u) {
            const double s = j >= u ? b.s[j >= u ? j - u : 0] : tail[j >= u ? 0 : u - j - 1];
#pragma unroll
            for (int o = 0; o < NO; ++o) acc[u][o] = fma(b.t[j][o], s, acc[u][o]);   // (an exact product: fma or multiply-then-add, same bits)
        }
    }
#pragma unroll
    for (int v = 0; v < OUT_U - 1; ++v) tail[v] = b.s[OUT_KB - 1 - v];
}

template <int NO>
__device__ __forceinline__ void out_pass(const double *xp, const double *tp, int M, double (&acc)[OUT_U][NO]) {
    double tail[OUT_U - 1];
#pragma unroll
    for (int v = 0; v < OUT_U - 1; ++v) tail[v] = xp[v + 1];
    OutBlock<NO> A, B;
    const int pairs = M / (2 * OUT_KB);
    int k = 0;
    if (pairs) {
        out_load<NO>(A, xp, tp);
        for (int it = 1; it < pairs; ++it) {
            out_load<NO>(B, xp - (k + OUT_KB), tp + (k + OUT_KB) * NO);
            out_sum<NO>(A, tail, acc);
            __builtin_amdgcn_sched_barrier(0);                           // (A's next reads behind A's last use: the same
            out_load<NO>(A, xp - (k + 2 * OUT_KB), tp + (k + 2 * OUT_KB) * NO);   // registers take them, no copies)
            out_sum<NO>(B, tail, acc);
            __builtin_amdgcn_sched_barrier(0);
            k += 2 * OUT_KB;
        }
        out_load<NO>(B, xp - (k + OUT_KB), tp + (k + OUT_KB) * NO);
        out_sum<NO>(A, tail, acc);
        out_sum<NO>(B, tail, acc);
        k += 2 * OUT_KB;
    }
    for (; k < M; ++k) {
        const double s = xp[-k];
#pragma unroll
        for (int u = 0; u < OUT_U; ++u) {
            const double w = u == 0 ? s : tail[u == 0 ? 0 : u - 1];
#pragma unroll
            for (int o = 0; o < NO; ++o) acc[u][o] = fma(tp[k * NO + o], w, acc[u][o]);
        }
#pragma unroll
        for (int v = OUT_U - 2; v > 0; --v) tail[v] = tail[v - 1];
        tail[0] = s;
    }
}

// One workgroup per (tile of OUT_TILE output frames, session).  Output j's newest frame is frame first + j of the window;
// slot s of the staged window holds window frame first + j0 - (M - 1) + s (zero where that is outside [0, T_win)), so frame
// u of thread tid at step k reads slot tid OUT_U + u + (M - 1) - k: [0, OUT_TILE + M - 2], all staged.
template <bool FULL>
__global__ __launch_bounds__(OUT_THREADS) void bas_output_kernel(const float *__restrict__ y, long y_g, long y_t, long y_c,
                                                                 long T_win, long first, const float *__restrict__ taps,
                                                                 long taps_g, int M, float *__restrict__ out, long o_g,
                                                                 long o_t, long o_c, long T_out) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double out_lds[];
    const int tid = threadIdx.x;
    const long j0 = (long)blockIdx.x * OUT_TILE;
    const int Tcur = (int)(T_out - j0 < OUT_TILE ? T_out - j0 : OUT_TILE);
    const int W = OUT_TILE + M - 1;
    double *Tl = out_lds, *X = out_lds + (FULL ? 4 : 2) * M;
    const float *tg = taps + blockIdx.y * taps_g;
    if (FULL) {                                                          // [o][i][k] -> [i][k][o]: a step's two taps side by side
#pragma unroll
        for (int oi = 0; oi < 4; ++oi)
            for (int k = tid; k < M; k += OUT_THREADS) Tl[((oi & 1) * M + k) * 2 + (oi >> 1)] = (double)tg[oi * M + k];
    } else {
        for (int e = tid; e < 2 * M; e += OUT_THREADS) Tl[e] = (double)tg[e];
    }
    const float *yg = y + blockIdx.y * y_g;
    const long lo = first + j0 - (M - 1);                                // slot 0 as a frame of the window
    for (int s = tid; s < W; s += OUT_THREADS) {
        const long w = lo + s;
        const bool inside = w >= 0 && w < T_win;
        X[s] = inside ? (double)yg[w * y_t] : 0.0;
        X[W + s] = inside ? (double)yg[w * y_t + y_c] : 0.0;
    }
    __syncthreads();
    if (tid * OUT_U >= Tcur) return;                                     // (no barrier follows)
    const double *xp = X + tid * OUT_U + (M - 1);
    float *og = out + blockIdx.y * o_g + (j0 + tid * OUT_U) * o_t;
    if (FULL) {
        double acc[OUT_U][2];
#pragma unroll
        for (int u = 0; u < OUT_U; ++u) acc[u][0] = acc[u][1] = 0.0;
        out_pass<2>(xp, Tl, M, acc);
        out_pass<2>(xp + W, Tl + 2 * M, M, acc);
#pragma unroll
        for (int u = 0; u < OUT_U; ++u) {
            if (tid * OUT_U + u < Tcur) {
                og[u * o_t] = (float)acc[u][0];                          // the ONE rounding
                og[u * o_t + o_c] = (float)acc[u][1];
            }
        }
    } else {
        double a0[OUT_U][1], a1[OUT_U][1];
#pragma unroll
        for (int u = 0; u < OUT_U; ++u) a0[u][0] = a1[u][0] = 0.0;
        out_pass<1>(xp, Tl, M, a0);
        out_pass<1>(xp + W, Tl + M, M, a1);
#pragma unroll
        for (int u = 0; u < OUT_U; ++u) {
            if (tid * OUT_U + u < Tcur) {
                og[u * o_t] = (float)a0[u][0];
                og[u * o_t + o_c] = (float)a1[u][0];
            }
        }
    }
}

extern "C" int bas_output_filter_f32(const float *y, long y_stride_g, long y_stride_t, long y_stride_c, int n_sessions,
                                     long T_win, long first, const float *taps, long taps_stride_g, int M, int full,
                                     float *out, long out_stride_g, long out_stride_t, long out_stride_c, long T_out,
                                     bas_stream_t stream) {
    bool nothing;
    const int rc = output_check(y, y_stride_g, y_stride_t, y_stride_c, n_sessions, T_win, first, taps, taps_stride_g, M, full,
                                out, out_stride_g, out_stride_t, out_stride_c, T_out, &nothing);
    if (rc || nothing) return rc;
    const OutputPlan P = output_plan(M, full);
    const dim3 grid((unsigned)((T_out + OUT_TILE - 1) / OUT_TILE), (unsigned)n_sessions);
    const hipStream_t st = bas_stream(stream);
    const void *fn = full ? reinterpret_cast<const void *>(bas_output_kernel<true>)
                          : reinterpret_cast<const void *>(bas_output_kernel<false>);
    if (P.lds_bytes > 64 * 1024) {
        const hipError_t e = bas_allow_full_lds(fn);
        if (e != hipSuccess) return bas_fail((int)e, "bas_output_filter_f32: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    if (full)
        hipLaunchKernelGGL(bas_output_kernel<true>, grid, dim3(OUT_THREADS), P.lds_bytes, st, y, y_stride_g, y_stride_t,
                           y_stride_c, T_win, first, taps, taps_stride_g, M, out, out_stride_g, out_stride_t, out_stride_c,
                           T_out);
    else
        hipLaunchKernelGGL(bas_output_kernel<false>, grid, dim3(OUT_THREADS), P.lds_bytes, st, y, y_stride_g, y_stride_t,
                           y_stride_c, T_win, first, taps, taps_stride_g, M, out, out_stride_g, out_stride_t, out_stride_c,
                           T_out);
    return bas_check_launch("bas_output_filter_f32");
}
