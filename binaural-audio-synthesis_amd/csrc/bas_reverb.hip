// Late reverberation (include/bas.h "late reverberation"):
//   bas_bus_mix_f32        - the send bus: a weighted mono mix of the source rows, weights interpolated between chunk boundaries
//   bas_long_fir_tail_f32  - a stereo tail of up to 2^17 taps -> the spectra of its partitions (once per tail)
//   bas_long_fir_f32       - the bus through the tail, added to a stereo signal: uniformly partitioned overlap-save, three
//                            launches (frame spectra, the sum over partitions per bin, inverse transform + add + peak)
#include "bas_reverb.h"

// ---------------------------------------------------------------------------------------------------------------------
// the bus
// ---------------------------------------------------------------------------------------------------------------------
#define BM_THREADS 256

// A lane makes outputs t0 .. t0 + 3 of group blockIdx.y: per source one quad of inputs and the weights of its chunk (the
// same addresses for every lane of a chunk), formed in binary64 and rounded once; four fused multiply-adds, s ascending.
// Lanes whose quad straddles a chunk boundary (K not a multiple of 4) take each sample's own boundaries.  Nothing depends
// on the tiling: an output's bits are a function of (j, K, the weights at its two boundaries) and its inputs alone.
__global__ __launch_bounds__(BM_THREADS) void bas_bus_mix_kernel(const float *__restrict__ x, long x_g, long x_s,
                                                                 const double *__restrict__ send, long s_g, long s_s, long s_k,
                                                                 int n_src, int T, int K, float *__restrict__ bus,
                                                                 long bus_stride) {
#pragma clang fp contract(off)
    const int g = blockIdx.y;
    const double *sg = send + g * s_g;
    float *out = bus + g * bus_stride;
    const bool out_quads = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    for (long q = (long)blockIdx.x * BM_THREADS + threadIdx.x; (q << 2) < T; q += (long)gridDim.x * BM_THREADS) {
        const int t0 = (int)(q << 2);
        int kk[4];
        double fr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            kk[i] = (t0 + i) / K;
            fr[i] = (double)(t0 + i - kk[i] * K) / (double)K;
        }
        const bool same = kk[0] == kk[3];
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < n_src; ++s) {
            const float *row = x + g * x_g + s * x_s + t0;
            float v[4];
            if (t0 + 3 < T && (reinterpret_cast<uintptr_t>(row) & 15) == 0) {
                const f32x4 r = *reinterpret_cast<const f32x4 *>(row);
                v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = t0 + i < T ? row[i] : 0.f;
            }
            const double *sp = sg + s * s_s;
            if (s_k == 0) {                                               // static: one weight per row
                const float w = (float)sp[0];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(w, v[i], acc[i]);
            } else if (same) {
                const double ga = sp[kk[0] * s_k], d = sp[(kk[0] + 1) * s_k] - ga;
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf((float)(ga + fr[i] * d), v[i], acc[i]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (t0 + i < T) {
                        const double ga = sp[kk[i] * s_k], d = sp[(kk[i] + 1) * s_k] - ga;
                        acc[i] = fmaf((float)(ga + fr[i] * d), v[i], acc[i]);
                    }
            }
        }
        if (out_quads && t0 + 3 < T) {
            f32x4 r;
            r.x = acc[0]; r.y = acc[1]; r.z = acc[2]; r.w = acc[3];
            *reinterpret_cast<f32x4 *>(out + t0) = r;
        } else {
            for (int i = 0; i < 4 && t0 + i < T; ++i) out[t0 + i] = acc[i];
        }
    }
}

extern "C" int bas_bus_mix_f32(const float *x, long x_stride_g, long x_stride_s, const double *send, long s_stride_g,
                               long s_stride_s, long s_stride_k, int n_groups, int n_src, long T, int K, float *bus,
                               long bus_stride, bas_stream_t stream) {
    BAS_REQUIRE(n_groups >= 0 && n_src >= 0 && T >= 0 && K > 0, BAS_E_SHAPE,
                "bas_bus_mix_f32: need n_groups, n_src, T >= 0 and K > 0");
    BAS_REQUIRE(T < (1L << 30), BAS_E_SHAPE, "bas_bus_mix_f32: T (%ld) must be below 2^30", T);
    BAS_REQUIRE(n_groups <= 65535, BAS_E_SHAPE, "bas_bus_mix_f32: more than 65535 buses in one call");
    BAS_REQUIRE(x_stride_g >= 0 && x_stride_s >= 0 && s_stride_g >= 0 && s_stride_s >= 0 && s_stride_k >= 0 &&
                    bus_stride >= 0,
                BAS_E_SHAPE, "bas_bus_mix_f32: strides must be >= 0");
    BAS_REQUIRE(n_groups <= 1 || bus_stride >= T, BAS_E_SHAPE, "bas_bus_mix_f32: bus_stride (%ld) must be >= T", bus_stride);
    if (n_groups == 0 || T == 0) return 0;
    BAS_REQUIRE(bus && (n_src == 0 || (x && send)), BAS_E_NULL, "bas_bus_mix_f32: null pointer");
    BAS_REQUIRE(bas_aligned(x, 4) && bas_aligned(bus, 4) && bas_aligned(send, 8),
                BAS_E_ALIGN, "bas_bus_mix_f32: x and bus must be 4-byte aligned, send 8-byte");
    const long quads = (T + 3) >> 2;
    const long blocks = (quads + BM_THREADS - 1) / BM_THREADS;
    const dim3 grid((unsigned)(blocks < 65535 ? blocks : 65535), (unsigned)n_groups);
    hipLaunchKernelGGL(bas_bus_mix_kernel, grid, dim3(BM_THREADS), 0, bas_stream(stream), x, x_stride_g, x_stride_s, send,
                       s_stride_g, s_stride_s, s_stride_k, n_src, (int)T, K, bus, bus_stride);
    return bas_check_launch("bas_bus_mix_f32");
}

// ---------------------------------------------------------------------------------------------------------------------
// the tail's spectra
// ---------------------------------------------------------------------------------------------------------------------
static inline bool rv_np_ok(int Np) { return Np == 32 || Np == 64 || Np == 128 || Np == 256 || Np == 512; }
static inline long rv_partitions(int Lr, int Np) { return ((long)Lr + Np - 1) / Np; }

// tail = [Np twiddles (re, im)] [P][Np + 1] x (left re, left im, right re, right im): partition p of ear e is
// [h_e[p Np .. (p + 1) Np) | Np zeros] under a DFT of size N = 2 Np, bins 0 .. Np, times 1 / N (exact: the inverse
// transform of the convolver then needs no scaling).  One workgroup of Np threads per partition, the ears one after the
// other; the twiddles come from binary64 sincospi, and workgroup 0 stores them for every later transform of this tail.
__global__ __launch_bounds__(RV_MAX_NP) void bas_long_fir_tail_kernel(const float *__restrict__ h, long h_stride, int Lr,
                                                                      int Np, float *__restrict__ tail) {
    __shared__ RvFft s;
    const int t = threadIdx.x, p = blockIdx.x;
    double sn, cs;
    sincospi((double)t / (double)Np, &sn, &cs);                          // 2 pi t / N = pi t / Np
    f32x2 w;
    w.x = (float)cs;
    w.y = (float)-sn;
    s.tw[t] = w;
    if (p == 0) reinterpret_cast<f32x2 *>(tail)[t] = w;
    float *spec = tail + 2 * Np + (long)p * (Np + 1) * 4;
    const float scale = 1.0f / (float)(2 * Np);
    const long n = (long)p * Np + t;
    for (int e = 0; e < 2; ++e) {
        __syncthreads();                                                  // (the first ear's result has been read)
        f32x2 v;
        v.x = n < Lr ? h[e * h_stride + n] : 0.f;
        v.y = 0.f;
        s.a[t] = v;
        v.x = 0.f;
        s.a[t + Np] = v;
        const f32x2 *r = rv_fft<false>(s, Np);
        spec[t * 4 + 2 * e] = r[t].x * scale;
        spec[t * 4 + 2 * e + 1] = r[t].y * scale;
        if (t == 0) {
            spec[Np * 4 + 2 * e] = r[Np].x * scale;
            spec[Np * 4 + 2 * e + 1] = r[Np].y * scale;
        }
    }
}

extern "C" size_t bas_long_fir_tail_floats(int Lr, int Np) {
    if (!rv_np_ok(Np) || Lr < 1 || Lr > RV_MAX_LR) return 0;
    return (size_t)(2 * Np) + (size_t)rv_partitions(Lr, Np) * (Np + 1) * 4;
}

extern "C" int bas_long_fir_tail_f32(const float *h, long h_stride, int Lr, int Np, float *tail, bas_stream_t stream) {
    BAS_REQUIRE(rv_np_ok(Np), BAS_E_SHAPE, "bas_long_fir_tail_f32: Np (%d) must be 32, 64, 128, 256 or 512", Np);
    BAS_REQUIRE(Lr >= 1 && Lr <= RV_MAX_LR, BAS_E_SHAPE, "bas_long_fir_tail_f32: Lr (%d) must be in 1..2^17", Lr);
    BAS_REQUIRE(h_stride >= Lr, BAS_E_SHAPE, "bas_long_fir_tail_f32: h_stride (%ld) must be >= Lr", h_stride);
    BAS_REQUIRE(h && tail, BAS_E_NULL, "bas_long_fir_tail_f32: null pointer");
    BAS_REQUIRE(bas_aligned(h, 4) && bas_aligned(tail, 16), BAS_E_ALIGN,
                "bas_long_fir_tail_f32: h must be 4-byte aligned, tail 16-byte");
    hipLaunchKernelGGL(bas_long_fir_tail_kernel, dim3((unsigned)rv_partitions(Lr, Np)), dim3(Np), 0, bas_stream(stream), h,
                       h_stride, Lr, Np, tail);
    return bas_check_launch("bas_long_fir_tail_f32");
}

// ---------------------------------------------------------------------------------------------------------------------
// the convolver
// ---------------------------------------------------------------------------------------------------------------------
// Workspace: X [n_bus][F + P - 1][Np + 1] complex, the spectrum of frame f (f = -(P - 1) .. F - 1) in row f + P - 1, then
// Y [n_bus][F][2][Np + 1] complex, F = ceil(T_out / Np).
struct RvPlan {
    long F, P, n_frames;
    size_t x_bytes, y_bytes;
};
static inline RvPlan rv_plan(int n_bus, long T_out, int Lr, int Np) {
    RvPlan pl;
    pl.F = (T_out + Np - 1) / Np;
    pl.P = rv_partitions(Lr, Np);
    pl.n_frames = pl.F + pl.P - 1;
    pl.x_bytes = (size_t)n_bus * pl.n_frames * (Np + 1) * sizeof(f32x2);
    pl.y_bytes = (size_t)n_bus * pl.F * 2 * (Np + 1) * sizeof(f32x2);
    return pl;
}

// Frame spectra: one workgroup of Np threads per (frame row, bus).  The frame's window is bus samples
// [(f - 1) Np - lag, (f + 1) Np - lag), zeros outside the readable range [-Hb, T_bus); a window wholly outside it is
// written as zeros without a transform (the transform of zeros is +0 everywhere: the same bits).
__global__ __launch_bounds__(RV_MAX_NP) void bas_long_fir_forward_kernel(const float *__restrict__ bus, long bus_stride,
                                                                         long Hb, long T_bus, const float *__restrict__ tail,
                                                                         int Np, int P, int lag, f32x2 *__restrict__ X,
                                                                         long n_frames) {
    __shared__ RvFft s;
    const int t = threadIdx.x, g = blockIdx.y;
    const long fi = blockIdx.x;
    f32x2 *dst = X + ((long)g * n_frames + fi) * (Np + 1);
    const long w0 = (fi - P) * Np - lag;                                 // f - 1 = fi - (P - 1) - 1
    if (w0 + 2 * Np <= -Hb || w0 >= T_bus) {                             // (uniform over the workgroup)
        f32x2 z;
        z.x = z.y = 0.f;
        dst[t] = z;
        if (t == 0) dst[Np] = z;
        return;
    }
    const float *row = bus + g * bus_stride;
    const long p0 = w0 + t, p1 = p0 + Np;
    f32x2 v;
    v.y = 0.f;
    v.x = p0 >= -Hb && p0 < T_bus ? row[p0] : 0.f;
    s.a[t] = v;
    v.x = p1 >= -Hb && p1 < T_bus ? row[p1] : 0.f;
    s.a[t + Np] = v;
    s.tw[t] = reinterpret_cast<const f32x2 *>(tail)[t];
    const f32x2 *r = rv_fft<false>(s, Np);
    dst[t] = r[t];
    if (t == 0) dst[Np] = r[Np];
}

// Y_e[f][k] = sum_p X[f - p][k] H_e[p][k]: ONE thread per (bin, frame), p ascending from +0, four fused multiply-adds per
// ear and partition in a fixed order - so the bits do not depend on FB, the frames a thread carries side by side to
// read each H once for all of them: its window of X slides one frame back per partition (one load).  One wave per
// workgroup: blockIdx.x deals the frames, blockIdx.y the bins 64 at a time, blockIdx.z the buses.
template <int FB>
__global__ __launch_bounds__(64) void bas_long_fir_mac_kernel(const f32x2 *__restrict__ X, const float *__restrict__ tail,
                                                              int Np, int P, long F, long n_frames, f32x2 *__restrict__ Y) {
    const int k = blockIdx.y * 64 + threadIdx.x;
    if (k > Np) return;
    const int nb = Np + 1, g = blockIdx.z;
    const long f0 = (long)blockIdx.x * FB;
    const f32x2 *Xg = X + (long)g * n_frames * nb + k;
    const f32x4 *H = reinterpret_cast<const f32x4 *>(tail + 2 * Np) + k;
    f32x2 xw[FB], yl[FB], yr[FB];
#pragma unroll
    for (int i = 0; i < FB; ++i) {
        const long f = f0 + i < F ? f0 + i : F - 1;                     // (frames past the last: any valid row, never stored)
        xw[i] = Xg[(f + P - 1) * nb];
        yl[i].x = yl[i].y = yr[i].x = yr[i].y = 0.f;
    }
    for (int p = 0; p < P; ++p) {
        const f32x4 h = H[(long)p * nb];
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            const f32x2 x = xw[i];
            yl[i].x = fmaf(x.x, h.x, yl[i].x);
            yl[i].x = fmaf(-x.y, h.y, yl[i].x);
            yl[i].y = fmaf(x.x, h.y, yl[i].y);
            yl[i].y = fmaf(x.y, h.x, yl[i].y);
            yr[i].x = fmaf(x.x, h.z, yr[i].x);
            yr[i].x = fmaf(-x.y, h.w, yr[i].x);
            yr[i].y = fmaf(x.x, h.w, yr[i].y);
            yr[i].y = fmaf(x.y, h.z, yr[i].y);
        }
        if (p + 1 < P) {                                                 // frame f0 - (p + 1): row f0 + P - 2 - p >= 0
#pragma unroll
            for (int i = FB - 1; i > 0; --i) xw[i] = xw[i - 1];
            xw[0] = Xg[(f0 + P - 2 - p) * nb];
        }
    }
#pragma unroll
    for (int i = 0; i < FB; ++i)
        if (f0 + i < F) {
            f32x2 *dst = Y + (((long)g * F + f0 + i) * 2) * nb + k;
            dst[0] = yl[i];
            dst[nb] = yr[i];
        }
}

// One workgroup of Np threads per (frame, bus): Z = Y_left + i Y_right over all N bins (bins above Np by conjugate
// symmetry), ONE inverse transform, whose second half holds the frame's Np outputs: the left ear in the real part,
// the right ear in the imaginary part.  out = y_in + r (y_in is zero past T_y, or absent), then the frame's max|out|
// into *peak.
__global__ __launch_bounds__(RV_MAX_NP) void bas_long_fir_inverse_kernel(const f32x2 *__restrict__ Y,
                                                                         const float *__restrict__ tail, int Np, long F,
                                                                         const float *y_in, long y_g, long y_e, long T_y,
                                                                         float *out, long o_g, long o_e, long T_out,
                                                                         float *peak) {
    __shared__ RvFft s;
    const int t = threadIdx.x, g = blockIdx.y, nb = Np + 1;
    const long f = blockIdx.x;
    const f32x2 *yl = Y + (((long)g * F + f) * 2) * nb, *yr = yl + nb;
    s.tw[t] = reinterpret_cast<const f32x2 *>(tail)[t];
    f32x2 l = yl[t], r = yr[t], z;
    z.x = l.x - r.y;                                                     // L + i R
    z.y = l.y + r.x;
    s.a[t] = z;
    if (t > 0) {                                                         // bin N - t: conj(L) + i conj(R)
        z.x = l.x + r.y;
        z.y = r.x - l.y;
        s.a[2 * Np - t] = z;
    } else {
        l = yl[Np];
        r = yr[Np];
        z.x = l.x - r.y;
        z.y = l.y + r.x;
        s.a[Np] = z;
    }
    const f32x2 v = rv_fft<true>(s, Np)[Np + t];
    const long n = f * Np + t;
    float ol = 0.f, orr = 0.f;
    if (n < T_out) {
        const bool dry = y_in != nullptr && n < T_y;
        ol = (dry ? y_in[g * y_g + n] : 0.f) + v.x;
        orr = (dry ? y_in[g * y_g + y_e + n] : 0.f) + v.y;
        out[g * o_g + n] = ol;
        out[g * o_g + o_e + n] = orr;
    }
    if (peak) {                                                          // (uniform) the workgroup's maximum through LDS
        float *m = reinterpret_cast<float *>(s.tw);                      // (the twiddles have been used)
        __syncthreads();
        m[t] = bas_peak_max(bas_peak_max(0.f, ol), orr);
        __syncthreads();
        for (int o = Np >> 1; o > 0; o >>= 1) {
            if (t < o) m[t] = bas_peak_max(m[t], m[t + o]);
            __syncthreads();
        }
        if (t == 0) {
            unsigned int *bits = reinterpret_cast<unsigned int *>(peak) + g;
            const unsigned int mine = __float_as_uint(m[0]);
            if (mine > __hip_atomic_load(bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(bits, mine);
        }
    }
}

extern "C" size_t bas_long_fir_workspace_bytes(int n_bus, long T_out, int Lr, int Np) {
    if (!rv_np_ok(Np) || Lr < 1 || Lr > RV_MAX_LR || n_bus < 0 || n_bus > 65535 || T_out < 0 || T_out >= (1L << 30)) return 0;
    const RvPlan pl = rv_plan(n_bus, T_out, Lr, Np);
    return pl.x_bytes + pl.y_bytes;
}

extern "C" int bas_long_fir_f32(const float *bus, long bus_stride, long Hb, long T_bus, int n_bus, const float *tail, int Lr,
                                int Np, int lag, const float *y_in, long y_stride_g, long y_stride_e, long T_y, float *out,
                                long out_stride_g, long out_stride_e, long T_out, float *peak, void *ws, size_t ws_bytes,
                                bas_stream_t stream) {
    BAS_REQUIRE(rv_np_ok(Np), BAS_E_SHAPE, "bas_long_fir_f32: Np (%d) must be 32, 64, 128, 256 or 512", Np);
    BAS_REQUIRE(Lr >= 1 && Lr <= RV_MAX_LR, BAS_E_SHAPE, "bas_long_fir_f32: Lr (%d) must be in 1..2^17", Lr);
    BAS_REQUIRE(lag >= 0 && lag <= RV_MAX_LAG, BAS_E_SHAPE, "bas_long_fir_f32: lag (%d) must be in 0..2^20", lag);
    BAS_REQUIRE(n_bus >= 0 && n_bus <= 65535, BAS_E_SHAPE, "bas_long_fir_f32: n_bus (%d) must be in 0..65535", n_bus);
    BAS_REQUIRE(T_bus >= 0 && T_bus < (1L << 30) && T_out >= 0 && T_out < (1L << 30) && T_y >= 0 && T_y < (1L << 30) &&
                    Hb >= 0 && Hb < (1L << 30),
                BAS_E_SHAPE, "bas_long_fir_f32: T_bus, T_out, T_y and Hb must be in 0..2^30 - 1");
    BAS_REQUIRE(bus_stride >= 0 && y_stride_g >= 0 && y_stride_e >= 0 && out_stride_g >= 0 && out_stride_e >= 0,
                BAS_E_SHAPE, "bas_long_fir_f32: strides must be >= 0");
    BAS_REQUIRE(out_stride_e >= T_out && (n_bus <= 1 || out_stride_g >= out_stride_e + T_out), BAS_E_SHAPE,
                "bas_long_fir_f32: the output's ears and buses must not overlap (out_stride_e >= T_out, out_stride_g >= "
                "out_stride_e + T_out)");
    if (n_bus == 0 || T_out == 0) return 0;
    BAS_REQUIRE(tail && out && ws && (bus || Hb + T_bus == 0), BAS_E_NULL, "bas_long_fir_f32: null pointer");
    BAS_REQUIRE(bas_aligned(bus, 4) && bas_aligned(y_in, 4) && bas_aligned(out, 4) && bas_aligned(peak, 4) &&
                    bas_aligned(tail, 16) && bas_aligned(ws, 16),
                BAS_E_ALIGN, "bas_long_fir_f32: bus, y_in, out, peak must be 4-byte aligned, tail and ws 16-byte");
    const RvPlan pl = rv_plan(n_bus, T_out, Lr, Np);
    BAS_REQUIRE(ws_bytes >= pl.x_bytes + pl.y_bytes, BAS_E_WORKSPACE,
                "bas_long_fir_f32: workspace of %zu bytes, bas_long_fir_workspace_bytes says %zu", ws_bytes,
                pl.x_bytes + pl.y_bytes);
    f32x2 *X = reinterpret_cast<f32x2 *>(ws);
    f32x2 *Y = reinterpret_cast<f32x2 *>(reinterpret_cast<char *>(ws) + pl.x_bytes);
    const hipStream_t st = bas_stream(stream);
    const int P = (int)pl.P;
    hipLaunchKernelGGL(bas_long_fir_forward_kernel, dim3((unsigned)pl.n_frames, (unsigned)n_bus), dim3(Np), 0, st, bus,
                       bus_stride, Hb, T_bus, tail, Np, P, lag, X, pl.n_frames);
    // a stream block of a few frames: one frame per thread, so that its bins are spread as widely as they can be; a whole
    // signal: eight frames per thread share every H they read
    const unsigned bin_tiles = (unsigned)((Np + 1 + 63) / 64);
    if (pl.F < 4)
        hipLaunchKernelGGL(bas_long_fir_mac_kernel<1>, dim3((unsigned)pl.F, bin_tiles, (unsigned)n_bus), dim3(64), 0, st, X,
                           tail, Np, P, pl.F, pl.n_frames, Y);
    else
        hipLaunchKernelGGL(bas_long_fir_mac_kernel<8>, dim3((unsigned)((pl.F + 7) / 8), bin_tiles, (unsigned)n_bus), dim3(64),
                           0, st, X, tail, Np, P, pl.F, pl.n_frames, Y);
    hipLaunchKernelGGL(bas_long_fir_inverse_kernel, dim3((unsigned)pl.F, (unsigned)n_bus), dim3(Np), 0, st, Y, tail, Np, pl.F,
                       y_in, y_stride_g, y_stride_e, T_y, out, out_stride_g, out_stride_e, T_out, peak);
    return bas_check_launch("bas_long_fir_f32");
}
