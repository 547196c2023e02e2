// Per-source FIR colouring (include/bas.h "per-source colour"):
//   bas_color_rows_f32 - a short FIR per (group, source) row, its coefficients interpolated between chunk boundaries,
//                        with the addressing of bas_delay_rows_f32 (strided rows, readable history in front), one launch.
#include "bas_internal.h"

#define CL_THREADS 256
#define CL_TILE (4 * CL_THREADS)        // outputs of one workgroup pass: four per lane
#define CL_MAX_TAPS 64
#define CL_SETS 34                      // coefficient sets a tile can touch: (CL_TILE - 1) / K + 3 at K >= 32 (the launcher
                                        // shortens the tile for smaller chunks)

// One workgroup per (tile, row): blockIdx.y is the row r = g n_src + s, blockIdx.x strides over the row's tiles.
// LDS holds the tile's inputs with MP = M rounded up to 4 samples in front of them (xs[i] = x'(t0 - MP + i); zeros outside
// the row's readable range [-Hc, valid length)) and the coefficient sets of the boundaries the tile touches, each padded
// with zeros to MP taps (a zero tap adds an exact zero).  A lane makes outputs t .. t + 3: per group of four taps it reads
// one more quad of inputs (its eight-sample register window slides back) and one quad of each coefficient set - the same
// address for every lane of a chunk, a broadcast - and does 16 (STATIC) or 32 fused multiply-adds, taps ascending.  Lanes
// whose four outputs straddle a chunk boundary (K not a multiple of 4) do theirs one by one, the same operations in the
// same order.  Nothing depends on t0: an output's bits are a function of (j, K, c_k, c_{k+1}) and its inputs alone.
template <bool STATIC>
__global__ __launch_bounds__(CL_THREADS) void bas_color_rows_kernel(
    const float *__restrict__ x, long x_g, long x_s, int Hc, const long *__restrict__ len, const float *__restrict__ color,
    long c_g, long c_s, long c_k, int M, int n_src, int T, int K, int tile, float *__restrict__ y, long y_g, long y_s) {
    __shared__ __attribute__((aligned(16))) float xs[CL_MAX_TAPS + CL_TILE];
    __shared__ __attribute__((aligned(16))) float cs[CL_SETS * CL_MAX_TAPS];
    const int r = blockIdx.y;
    const int g = r / n_src, s = r - g * n_src;
    const float *row = x + g * x_g + s * x_s;
    const float *crow = color + g * c_g + s * c_s;
    float *out = y + g * y_g + s * y_s;
    const int hi = (int)(len ? min(len[r], (long)T) : (long)T);
    const int MP = (M + 3) & ~3;
    const bool in_quads = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const bool out_quads = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const float inv_K = 1.0f / (float)K;
    const int n_tiles = (T + tile - 1) / tile;
    for (int it = blockIdx.x; it < n_tiles; it += gridDim.x) {
        const int t0 = it * tile;
        const int t1 = min(t0 + tile, T);                                // the tile's outputs are [t0, t1)
        // ---- inputs: quads of [t0 - MP, t1), zeros where the row has nothing to read
        for (int q = threadIdx.x; q < (MP + t1 - t0 + 3) >> 2; q += CL_THREADS) {
            const int t = t0 - MP + (q << 2);
            f32x4 v;
            if (in_quads && t >= -Hc && t + 3 < hi) {
                v = *reinterpret_cast<const f32x4 *>(row + t);
            } else {
                v.x = t >= -Hc && t < hi ? row[t] : 0.f;
                v.y = t + 1 >= -Hc && t + 1 < hi ? row[t + 1] : 0.f;
                v.z = t + 2 >= -Hc && t + 2 < hi ? row[t + 2] : 0.f;
                v.w = t + 3 >= -Hc && t + 3 < hi ? row[t + 3] : 0.f;
            }
            *reinterpret_cast<f32x4 *>(xs + (q << 2)) = v;
        }
        // ---- coefficients: the sets of boundaries k0 .. k1 + 1 (STATIC: the one set)
        const int k0 = t0 / K;
        const int n_sets = STATIC ? 1 : (t1 - 1) / K - k0 + 2;
        for (int i = threadIdx.x; i < n_sets * MP; i += CL_THREADS) {
            const int set = i / MP, m = i - set * MP;
            cs[i] = m < M ? crow[(long)(k0 + set) * c_k + m] : 0.f;
        }
        __syncthreads();
        const int tl = t0 + (threadIdx.x << 2);
        if (tl < t1) {
            const int p = MP + (threadIdx.x << 2);                        // xs index of output tl
            const int k = tl / K, j = tl - k * K;
            float o[4];
            if (j + 3 < K) {                                              // the lane's four outputs share a chunk
                const f32x4 *ca = reinterpret_cast<const f32x4 *>(cs + (STATIC ? 0 : (k - k0) * MP));
                const f32x4 *cb = reinterpret_cast<const f32x4 *>(cs + (STATIC ? 0 : (k - k0 + 1) * MP));
                float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
                f32x4 cur = *reinterpret_cast<const f32x4 *>(xs + p);
#pragma unroll 2                                                          // (fully unrolled it takes 116 VGPRs: 4 waves per SIMD)
                for (int gq = 0; gq < MP >> 2; ++gq) {
                    const f32x4 prev = *reinterpret_cast<const f32x4 *>(xs + p - 4 - (gq << 2));
                    const float w[8] = {prev.x, prev.y, prev.z, prev.w, cur.x, cur.y, cur.z, cur.w};
                    const f32x4 qa = ca[gq];
                    const float ta[4] = {qa.x, qa.y, qa.z, qa.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int i = 0; i < 4; ++i) a[i] = fmaf(ta[e], w[4 + i - e], a[i]);
                    if (!STATIC) {
                        const f32x4 qb = cb[gq];
                        const float tb[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int i = 0; i < 4; ++i) b[i] = fmaf(tb[e], w[4 + i - e], b[i]);
                    }
                    cur = prev;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    o[i] = STATIC ? a[i] : bas_crossfade(a[i], b[i], (float)(j + i) * inv_K);
            } else {                                                      // a chunk boundary inside the quad: one by one
                int ki = k, ji = j;
                for (int i = 0; i < 4; ++i) {
                    const float *ca = cs + (STATIC ? 0 : (ki - k0) * MP);
                    const float *cb = cs + (STATIC ? 0 : (ki - k0 + 1) * MP);
                    float a = 0.f, b = 0.f;
                    if (tl + i < t1)
                        for (int m = 0; m < MP; ++m) {
                            const float v = xs[p + i - m];
                            a = fmaf(ca[m], v, a);
                            if (!STATIC) b = fmaf(cb[m], v, b);
                        }
                    o[i] = STATIC ? a : bas_crossfade(a, b, (float)ji * inv_K);
                    if (++ji == K) { ji = 0; ++ki; }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (tl + i >= hi) o[i] = 0.f;                             // at and past the valid length: silence
            if (out_quads && tl + 3 < T) {
                f32x4 v;
                v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
                *reinterpret_cast<f32x4 *>(out + tl) = v;
            } else {
                for (int i = 0; i < 4 && tl + i < T; ++i) out[tl + i] = o[i];
            }
        }
        __syncthreads();                                                  // (the next tile overwrites xs and cs)
    }
}

extern "C" int bas_color_rows_f32(const float *x, long x_stride_g, long x_stride_s, int Hc, const long *lengths,
                                  const float *color, long c_stride_g, long c_stride_s, long c_stride_k, int M,
                                  int n_groups, int n_src, long T, int K, float *y, long y_stride_g, long y_stride_s,
                                  bas_stream_t stream) {
    BAS_REQUIRE(n_groups >= 0 && n_src >= 0 && T >= 0 && K > 0 && Hc >= 0, BAS_E_SHAPE,
                "bas_color_rows_f32: need n_groups, n_src, T, Hc >= 0 and K > 0");
    BAS_REQUIRE(M >= 1 && M <= CL_MAX_TAPS, BAS_E_SHAPE, "bas_color_rows_f32: M (%d) must be in 1..%d", M, CL_MAX_TAPS);
    BAS_REQUIRE(T < (1L << 30), BAS_E_SHAPE, "bas_color_rows_f32: T (%ld) must be below 2^30", T);
    BAS_REQUIRE((long)n_groups * n_src <= 65535, BAS_E_SHAPE, "bas_color_rows_f32: more than 65535 rows in one call");
    BAS_REQUIRE(x_stride_g >= 0 && x_stride_s >= 0 && c_stride_g >= 0 && c_stride_s >= 0 && c_stride_k >= 0 &&
                    y_stride_g >= 0 && y_stride_s >= 0,
                BAS_E_SHAPE, "bas_color_rows_f32: strides must be >= 0");
    BAS_REQUIRE(c_stride_k == 0 || c_stride_k >= M, BAS_E_SHAPE,
                "bas_color_rows_f32: c_stride_k must be 0 (static) or >= M (the sets of two boundaries overlap)");
    if ((long)n_groups * n_src == 0 || T == 0) return 0;
    BAS_REQUIRE(x && color && y, BAS_E_NULL, "bas_color_rows_f32: null pointer");
    BAS_REQUIRE(bas_aligned(x, 4) && bas_aligned(color, 4) && bas_aligned(y, 4) && bas_aligned(lengths, 8),
                BAS_E_ALIGN, "bas_color_rows_f32: x, color, y must be 4-byte aligned, lengths 8-byte");
    // a tile touches (tile - 1) / K + 3 coefficient sets at most: whole tiles down to K = 32, shorter ones below
    const int tile = K >= 32 ? CL_TILE : (32 * K) & ~3;
    const long n_tiles = (T + tile - 1) / tile;
    const dim3 grid((unsigned)(n_tiles < 65535 ? n_tiles : 65535), (unsigned)(n_groups * n_src));
    if (c_stride_k == 0)
        hipLaunchKernelGGL(bas_color_rows_kernel<true>, grid, dim3(CL_THREADS), 0, bas_stream(stream), x, x_stride_g,
                           x_stride_s, Hc, lengths, color, c_stride_g, c_stride_s, c_stride_k, M, n_src, (int)T, K, tile, y,
                           y_stride_g, y_stride_s);
    else
        hipLaunchKernelGGL(bas_color_rows_kernel<false>, grid, dim3(CL_THREADS), 0, bas_stream(stream), x, x_stride_g,
                           x_stride_s, Hc, lengths, color, c_stride_g, c_stride_s, c_stride_k, M, n_src, (int)T, K, tile, y,
                           y_stride_g, y_stride_s);
    return bas_check_launch("bas_color_rows_f32");
}
