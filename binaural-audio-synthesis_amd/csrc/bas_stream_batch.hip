// Carried state of block-wise rendering (bas.h "streaming", "batched streams").  A stream
// is rendered as [halo | block] windows (the reference's chunk loop is causal, apply_hrtf.py:431-453).  Batched streams: G
// independent streams of n_src sources advance by one block of B samples in ONE render.  Session g's window starts at g·W
// of every source row, W = halo + B + K: a zero chunk follows every window (its two boundaries are the end of session g and
// the start of session g+1, so the crossfade of apply_hrtf.py:431-442 never mixes two sessions' angles into an emitted
// sample).  The angle rows hold nh + nb boundaries per session, session g's from g·(nh + nb).  Entry points:
//   bas_stream_batch_pack_f32      - scatter [G][n_src][B] blocks and [G][n_src][nb] angles into the windows' block columns
//                                    and angle slots (never the halo columns, the halo angles or the gaps), one launch;
//   bas_stream_batch_pack_head_f32 - the same scatter with world-frame angles and [G][nb][4] head orientations: the angle
//                                    slots get the head-relative angles (bas_head.h), still one launch;
//   bas_stream_batch_epilogue_f32  - behind the render, per session: the running peak over the samples the block emits (the
//                                    window's first `halo` outputs were emitted before, its last L-1 are incomplete) and
//                                    the moves of the carried state (bas_carry_moves), one launch;
//   bas_stream_epilogue_f32        - the same kernel on ONE stream (one session row), behind renders that do not move the
//                                    carried state themselves (stream.py's two-call blocks, direct-output fused blocks).
#include "bas_internal.h"
#include "bas_head.h"
#include "bas_delay.h"

#define SB_THREADS 256

__device__ __forceinline__ bool sb_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One row of workgroups per session (blockIdx.y = g).  Items of a session: n_src rows of ceil(B/4) quads, then n_src rows
// of nb (elev, azim) pairs.  A quad moves as one 16-byte load and store when both rows are 16-byte aligned and B % 4 == 0
// (every quad of the row then is), else as up to 4 scalars (still coalesced across a wave).  HEAD: the angles are world-frame
// and head [G][nb][4] holds session g's orientation at each boundary; the slots get bas_head_relative's angles.
// GAIN: gain [G][n_src][nb] goes into gain_out's slots beside the angles, in the same launch.
// DELAY: a block quad goes into the window as its delayed samples, read from the session's carried raw
// history raw[g][s][0 .. H) and the dense block (bas_delay_sample_split, the same bits as bas_delay_rows_f32), with the
// delays delay[G][n_src][nb] clamped to [d_min, max_delay]; the raw block is copied behind the history (raw[g][s][H ..)),
// where bas_delay_carry_f32 finds it.  Nothing the launch reads is written by it.
template <bool HEAD, bool GAIN, bool DELAY>
__global__ __launch_bounds__(SB_THREADS) void bas_stream_batch_pack_kernel(
    const float *__restrict__ blocks, const double *__restrict__ elev, const double *__restrict__ azim, int n_src,
    long B, long W, int halo, int nh, int nb, float *__restrict__ x, long x_stride, double *__restrict__ elev_out,
    double *__restrict__ azim_out, long ang_stride, const double *__restrict__ head, const double *__restrict__ gain,
    double *__restrict__ gain_out, float *__restrict__ raw, long raw_g, long raw_s, int H, const double *__restrict__ delay,
    int K, int interp, double max_delay) {
    const int g = blockIdx.y;
    const long nq = (B + 3) >> 2;
    const long n_x = (long)n_src * nq, n_items = n_x + (long)n_src * nb;
    const long gstride = (long)gridDim.x * SB_THREADS;
    for (long i = blockIdx.x * (long)SB_THREADS + threadIdx.x; i < n_items; i += gstride) {
        if (i < n_x) {
            const int s = (int)(i / nq);
            const long j0 = (i - (long)s * nq) << 2;
            const float *src = blocks + ((long)g * n_src + s) * B;
            float *dst = x + (long)s * x_stride + (long)g * W + halo;
            if constexpr (DELAY) {
                float *hist = raw + (long)g * raw_g + (long)s * raw_s;
                const double *drow = delay + ((long)g * n_src + s) * nb;
                const double dmin = bas_delay_min(interp);
                for (int m = 0; m < 4 && j0 + m < B; ++m) {
                    const long t = j0 + m, k = t / K;
                    dst[t] = bas_delay_sample_split(hist, H, src, B, k * K, (int)(t - k * K), K, drow[k], drow[k + 1], dmin,
                                                    max_delay, interp);
                    hist[H + t] = src[t];
                }
            } else if ((B & 3) == 0 && sb_aligned16(src) && sb_aligned16(dst)) {
                *reinterpret_cast<f32x4 *>(dst + j0) = *reinterpret_cast<const f32x4 *>(src + j0);
            } else {
                for (int k = 0; k < 4 && j0 + k < B; ++k) dst[j0 + k] = src[j0 + k];
            }
        } else {
            const long r = i - n_x;
            const int s = (int)(r / nb);
            const int c = (int)(r - (long)s * nb);
            const long from = ((long)g * n_src + s) * nb + c;
            const long to = (long)s * ang_stride + (long)g * (nh + nb) + nh + c;
            if constexpr (HEAD) {
                const double *q = head + ((long)g * nb + c) * 4;
                double el_h, az_h;
                bas_head_relative(q[0], q[1], q[2], q[3], elev[from], azim[from], el_h, az_h);
                elev_out[to] = el_h;
                azim_out[to] = az_h;
            } else {
                elev_out[to] = elev[from];
                azim_out[to] = azim[from];
            }
            if constexpr (GAIN) gain_out[to] = gain[from];
        }
    }
}

// One row of workgroups per session.  peaks[g] = max(peaks[g], max|y[e][g·W + halo .. g·W + halo + B)|), e = 0, 1
// (atomicMax on the bits of non-negative floats: exact and order-free), then bas_carry_moves on session g's offset pointers.
// peak_bits may be null (bas_stream_epilogue_f32): the test is on a kernel argument, the same for the whole workgroup, as
// bas_block_peak_max's barrier needs.
__global__ __launch_bounds__(SB_THREADS) void bas_stream_block_epilogue_kernel(
    float *__restrict__ x, long x_stride, int n_src, int halo, long B, long W, double *__restrict__ elev,
    double *__restrict__ azim, long ang_stride, int nh, int nb, double *__restrict__ last, const float *__restrict__ y,
    long y_stride, unsigned int *__restrict__ peak_bits, double *__restrict__ gain, double *__restrict__ gain_last) {
    const int g = blockIdx.y;
    const long tid = blockIdx.x * (long)SB_THREADS + threadIdx.x;
    const long nthreads = (long)gridDim.x * SB_THREADS;
    float lmax = 0.f;
    for (int e = 0; e < 2; ++e) {
        const float *w = y + e * y_stride + (long)g * W + halo;
        const long head = sb_aligned16(w) ? 0 : min(B, (long)((16 - (reinterpret_cast<uintptr_t>(w) & 15)) >> 2));
        if (blockIdx.x == 0 && threadIdx.x < head) lmax = bas_peak_max(lmax, w[threadIdx.x]);
        const float *wa = w + head;
        const long nq = (B - head) >> 2;
        for (long i = tid; i < nq; i += nthreads) {
            const f32x4 q = *reinterpret_cast<const f32x4 *>(wa + 4 * i);
            lmax = bas_peak_max4(lmax, q);
        }
        const long tail0 = head + 4 * nq;
        if (blockIdx.x == 0 && tail0 + threadIdx.x < B) lmax = bas_peak_max(lmax, w[tail0 + threadIdx.x]);
    }
    if (peak_bits) bas_block_peak_max(lmax, peak_bits + g);
    BasCarry C;
    C.x = x + (long)g * W; C.x_stride = x_stride; C.n_src = n_src; C.halo = halo; C.B = B;
    C.elev = elev + (long)g * (nh + nb); C.azim = azim + (long)g * (nh + nb); C.ang_stride = ang_stride;
    C.nh = nh; C.nb = nb; C.last = last + 2L * n_src * g; C.running_peak = nullptr;
    C.gain = gain ? gain + (long)g * (nh + nb) : nullptr;      // (null: no gain row, as before)
    C.gain_last = gain ? gain_last + (long)n_src * g : nullptr;
    bas_carry_moves(C, tid, nthreads);
}

// workgroups per session: about 8 per CU over all sessions, at least one, at most one per 1024 items of a session's work
static int sb_blocks_x(int n_sessions, long work) {
    long want = (8L * bas_device_cus() + n_sessions - 1) / n_sessions;
    const long cap = (work + 1023) / 1024;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    if (want > 65535) want = 65535;
    return (int)want;
}

// the checks both entry points share: sizes, then the strides against the layout's extent
static int sb_check_layout(const char *what, int n_sessions, int n_src, long B, int K, int halo, long x_stride,
                           long ang_stride) {
    BAS_REQUIRE(n_sessions > 0 && n_sessions <= 65535 && n_src > 0 && K > 0 && B > 0 && B <= BAS_MAX_T_IN && halo >= 0, BAS_E_SHAPE,
                "%s: need 0 < n_sessions <= 65535, n_src > 0, K > 0, 0 < B <= 2^41, halo >= 0 (G=%d n_src=%d K=%d B=%ld halo=%d)",
                what, n_sessions, n_src, K, B, halo);
    BAS_REQUIRE(B % K == 0 && halo % K == 0, BAS_E_SHAPE, "%s: B (%ld) and halo (%d) must be multiples of K (%d)", what, B,
                halo, K);
    const long W = (long)halo + B + K, nh = halo / K, nb = B / K + 1;
    BAS_REQUIRE(x_stride >= n_sessions * W - K && ang_stride >= n_sessions * (nh + nb), BAS_E_SHAPE,
                "%s: strides shorter than the layout (x_stride %ld < %ld or ang_stride %ld < %ld)", what, x_stride,
                n_sessions * W - K, ang_stride, n_sessions * (nh + nb));
    return 0;
}

// every pack entry point: the layout checks, the pointers (head only with HEAD, gain and gain_out only with GAIN, raw and
// delay only with DELAY), one launch
template <bool HEAD, bool GAIN, bool DELAY = false>
static int sb_pack(const char *what, const float *blocks, const double *elev, const double *azim, const double *head,
                   const double *gain, int n_sessions, int n_src, long B, int K, int halo, float *x, long x_stride,
                   double *elev_out, double *azim_out, double *gain_out, long ang_stride, bas_stream_t stream,
                   float *raw = nullptr, long raw_g = 0, long raw_s = 0, int H = 0, const double *delay = nullptr,
                   int interp = 0, double max_delay = 0.0) {
    int rc = sb_check_layout(what, n_sessions, n_src, B, K, halo, x_stride, ang_stride);
    if (rc) return rc;
    BAS_REQUIRE(blocks && elev && azim && (!HEAD || head) && (!GAIN || (gain && gain_out)) && x && elev_out && azim_out &&
                    (!DELAY || (raw && delay)),
                BAS_E_NULL, "%s: null pointer", what);
    if (DELAY) {
        BAS_REQUIRE(interp == BAS_DELAY_LINEAR || interp == BAS_DELAY_CUBIC, BAS_E_SHAPE,
                    "%s: interp must be 0 (linear) or 1 (cubic)", what);
        BAS_REQUIRE(max_delay >= (interp == BAS_DELAY_CUBIC ? 2.0 : 1.0) && max_delay + 2.0 <= (double)H, BAS_E_SHAPE,
                    "%s: max_delay must lie in [d_min, H - 2]", what);
        BAS_REQUIRE(raw_s >= H + B && raw_g / raw_s >= n_src, BAS_E_SHAPE,
                    "%s: raw strides shorter than [H | B] rows", what);
    }
    const long W = (long)halo + B + K;
    const int nh = halo / K, nb = (int)(B / K + 1);
    const dim3 grid(sb_blocks_x(n_sessions, (long)n_src * (((B + 3) >> 2) + nb)), n_sessions);
    hipLaunchKernelGGL((bas_stream_batch_pack_kernel<HEAD, GAIN, DELAY>), grid, dim3(SB_THREADS), 0, bas_stream(stream),
                       blocks, elev, azim, n_src, B, W, halo, nh, nb, x, x_stride, elev_out, azim_out, ang_stride, head, gain,
                       gain_out, raw, raw_g, raw_s, H, delay, K, interp, max_delay);
    return bas_check_launch(what);
}

extern "C" int bas_stream_batch_pack_f32(const float *blocks, const double *elev, const double *azim, int n_sessions,
                                         int n_src, long B, int K, int halo, float *x, long x_stride, double *elev_out,
                                         double *azim_out, long ang_stride, bas_stream_t stream) {
    return sb_pack<false, false>("bas_stream_batch_pack_f32", blocks, elev, azim, nullptr, nullptr, n_sessions, n_src, B, K,
                                 halo, x, x_stride, elev_out, azim_out, nullptr, ang_stride, stream);
}

extern "C" int bas_stream_batch_pack_head_f32(const float *blocks, const double *elev, const double *azim,
                                              const double *head, int n_sessions, int n_src, long B, int K, int halo,
                                              float *x, long x_stride, double *elev_out, double *azim_out, long ang_stride,
                                              bas_stream_t stream) {
    return sb_pack<true, false>("bas_stream_batch_pack_head_f32", blocks, elev, azim, head, nullptr, n_sessions, n_src, B, K,
                                halo, x, x_stride, elev_out, azim_out, nullptr, ang_stride, stream);
}

// apply_hrtf.py:429-447 per session with per-boundary gains: the pack with gain [G][n_src][nb] ->
// gain_out[s][g (nh + nb) + nh + c]; head may be null (head-relative angles, as bas_stream_batch_pack_f32)
extern "C" int bas_stream_batch_pack_gain_f32(const float *blocks, const double *elev, const double *azim,
                                              const double *head, const double *gain, int n_sessions, int n_src, long B,
                                              int K, int halo, float *x, long x_stride, double *elev_out, double *azim_out,
                                              double *gain_out, long ang_stride, bas_stream_t stream) {
    if (head)
        return sb_pack<true, true>("bas_stream_batch_pack_gain_f32", blocks, elev, azim, head, gain, n_sessions, n_src, B, K,
                                   halo, x, x_stride, elev_out, azim_out, gain_out, ang_stride, stream);
    return sb_pack<false, true>("bas_stream_batch_pack_gain_f32", blocks, elev, azim, nullptr, gain, n_sessions, n_src, B, K,
                                halo, x, x_stride, elev_out, azim_out, gain_out, ang_stride, stream);
}

// the pack with per-source propagation delays: head and gain may each be NULL (then gain_out is ignored)
extern "C" int bas_stream_batch_pack_delay_f32(const float *blocks, const double *elev, const double *azim,
                                               const double *head, const double *gain, const double *delay, int interp,
                                               double max_delay, float *raw, long raw_stride_g, long raw_stride_s, int H,
                                               int n_sessions, int n_src, long B, int K, int halo, float *x, long x_stride,
                                               double *elev_out, double *azim_out, double *gain_out, long ang_stride,
                                               bas_stream_t stream) {
    const char *w = "bas_stream_batch_pack_delay_f32";
#define SB_PACK_DELAY(HD, GN)                                                                                              \
    return sb_pack<HD, GN, true>(w, blocks, elev, azim, head, gain, n_sessions, n_src, B, K, halo, x, x_stride, elev_out,  \
                                 azim_out, gain_out, ang_stride, stream, raw, raw_stride_g, raw_stride_s, H, delay, interp, \
                                 max_delay)
    if (head && gain) SB_PACK_DELAY(true, true);
    if (head) SB_PACK_DELAY(true, false);
    if (gain) SB_PACK_DELAY(false, true);
    SB_PACK_DELAY(false, false);
#undef SB_PACK_DELAY
}

static int sb_epilogue(const char *what, float *x, long x_stride, int n_sessions, int n_src, int halo, long B, int K,
                       double *elev, double *azim, double *gain, long ang_stride, double *last, double *gain_last,
                       bool need_gain, const float *y, long y_stride, float *peaks, bas_stream_t stream) {
    int rc = sb_check_layout(what, n_sessions, n_src, B, K, halo, x_stride, ang_stride);
    if (rc) return rc;
    const long W = (long)halo + B + K;
    BAS_REQUIRE(y_stride >= n_sessions * W - K, BAS_E_SHAPE, "%s: y_stride %ld < T_in %ld", what, y_stride,
                n_sessions * W - K);
    BAS_REQUIRE(x && elev && azim && last && y && peaks && (!need_gain || (gain && gain_last)), BAS_E_NULL,
                "%s: null pointer", what);
    const int nh = halo / K, nb = (int)(B / K + 1);
    const long work = (2 * B) / 4 > (long)n_src * halo ? (2 * B) / 4 : (long)n_src * halo;
    const dim3 grid(sb_blocks_x(n_sessions, work), n_sessions);
    hipLaunchKernelGGL(bas_stream_block_epilogue_kernel, grid, dim3(SB_THREADS), 0, bas_stream(stream), x, x_stride, n_src,
                       halo, B, W, elev, azim, ang_stride, nh, nb, last, y, y_stride,
                       reinterpret_cast<unsigned int *>(peaks), gain, gain_last);
    return bas_check_launch(what);
}

extern "C" int bas_stream_batch_epilogue_f32(float *x, long x_stride, int n_sessions, int n_src, int halo, long B, int K,
                                             double *elev, double *azim, long ang_stride, double *last, const float *y,
                                             long y_stride, float *peaks, bas_stream_t stream) {
    return sb_epilogue("bas_stream_batch_epilogue_f32", x, x_stride, n_sessions, n_src, halo, B, K, elev, azim, nullptr,
                       ang_stride, last, nullptr, false, y, y_stride, peaks, stream);
}

// apply_hrtf.py:429-447, carried per session: gain rows at the angles' stride move as the angles; gain_last [G][n_src]
extern "C" int bas_stream_batch_epilogue_gain_f32(float *x, long x_stride, int n_sessions, int n_src, int halo, long B,
                                                  int K, double *elev, double *azim, double *gain, long ang_stride,
                                                  double *last, double *gain_last, const float *y, long y_stride,
                                                  float *peaks, bas_stream_t stream) {
    return sb_epilogue("bas_stream_batch_epilogue_gain_f32", x, x_stride, n_sessions, n_src, halo, B, K, elev, azim, gain,
                       ang_stride, last, gain_last, true, y, y_stride, peaks, stream);
}

static int stream_epilogue(const char *what, float *x, long x_stride, int n_src, int halo, long B, double *elev,
                           double *azim, double *gain, long ang_stride, int nh, int nb, double *last, double *gain_last,
                           bool need_gain, const float *y, long y_stride, float *running_peak, bas_stream_t stream) {
    BAS_REQUIRE(n_src >= 0 && halo >= 0 && B > 0 && nh >= 0 && nb >= 2, BAS_E_SHAPE,
                "%s: need n_src>=0, halo>=0, B>0, nh>=0, nb>=2 (n_src=%d halo=%d B=%ld nh=%d nb=%d)", what, n_src, halo, B,
                nh, nb);
    BAS_REQUIRE(B <= BAS_MAX_T_IN && x_stride >= halo + B && ang_stride >= (long)nh + nb && y_stride >= halo + B, BAS_E_SHAPE,
                "%s: strides shorter than the window", what);
    BAS_REQUIRE(y && (n_src == 0 || (x && elev && azim && last && (!need_gain || (gain && gain_last)))), BAS_E_NULL,
                "%s: null pointer", what);
    long work = 2 * B > (long)n_src * halo ? 2 * B : (long)n_src * halo;
    hipLaunchKernelGGL(bas_stream_block_epilogue_kernel, dim3(bas_grid_for(work, 1024)), dim3(SB_THREADS), 0,
                       bas_stream(stream), x, x_stride, n_src, halo, B, 0L, elev, azim, ang_stride, nh, nb, last, y,
                       y_stride, reinterpret_cast<unsigned int *>(running_peak), gain, gain_last);   // (one session: W unused)
    return bas_check_launch(what);
}

extern "C" int bas_stream_epilogue_f32(float *x, long x_stride, int n_src, int halo, long B, double *elev, double *azim,
                                       long ang_stride, int nh, int nb, double *last, const float *y, long y_stride,
                                       float *running_peak, bas_stream_t stream) {
    return stream_epilogue("bas_stream_epilogue_f32", x, x_stride, n_src, halo, B, elev, azim, nullptr, ang_stride, nh, nb,
                           last, nullptr, false, y, y_stride, running_peak, stream);
}

// apply_hrtf.py:429-447, carried: gain [n_src] rows at the angles' stride move as the angles, gain_last [n_src]
extern "C" int bas_stream_epilogue_gain_f32(float *x, long x_stride, int n_src, int halo, long B, double *elev,
                                            double *azim, double *gain, long ang_stride, int nh, int nb, double *last,
                                            double *gain_last, const float *y, long y_stride, float *running_peak,
                                            bas_stream_t stream) {
    return stream_epilogue("bas_stream_epilogue_gain_f32", x, x_stride, n_src, halo, B, elev, azim, gain, ang_stride, nh, nb,
                           last, gain_last, true, y, y_stride, running_peak, stream);
}
