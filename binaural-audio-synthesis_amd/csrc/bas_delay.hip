// Per-source propagation delay (include/bas.h "propagation delay"):
//   bas_delay_rows_f32  - delayed inputs of strided rows with a readable history in front, two-level (group, source)
//                         addressing on both sides, one launch;
//   bas_delay_carry_f32 - the raw-history move of a stream block: the last H samples of [history | block] to the front.
// The batch packs (bas_batch.hip, bas_stream_batch.hip) inline the same bas_delay_sample.
#include "bas_internal.h"
#include "bas_delay.h"

#define DL_THREADS 256

// One row of workgroups per (g, s) row (blockIdx.y), 4 consecutive outputs per thread (one 16-byte store when the output
// row is 16-byte aligned; else scalars, still coalesced across a wave).  The reads are direct: d(t) varies slowly, so the
// 2 or 4 taps of neighbouring outputs are neighbouring samples and a workgroup's reads come from one short span in L1/L2.
// Outputs at t >= the row's valid length are 0.
__global__ __launch_bounds__(DL_THREADS) void bas_delay_rows_kernel(
    const float *__restrict__ x, long x_g, long x_s, int H, const long *__restrict__ len, const double *__restrict__ delay,
    long d_g, long d_s, int n_src, int T, int K, int interp, double dmax, float *__restrict__ y, long y_g, long y_s) {
    const int r = blockIdx.y;
    const int g = r / n_src, s = r - g * n_src;
    const float *row = x + g * x_g + s * x_s;
    const double *drow = delay + g * d_g + s * d_s;
    float *out = y + g * y_g + s * y_s;
    const long hi = len ? min(len[r], (long)T) : (long)T;
    const double dmin = bas_delay_min(interp);
    const double dhi = dmax > 0.0 ? dmax : (double)hi + 4.0;      // offline: any delay past the row reads before sample 0
    const bool quads = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int nq = (T + 3) >> 2;
    for (int q = blockIdx.x * DL_THREADS + threadIdx.x; q < nq; q += gridDim.x * DL_THREADS) {
        const int t0 = q << 2;
        int k = t0 / K, j = t0 - k * K;
        float v[4];
        for (int m = 0; m < 4; ++m) {
            v[m] = t0 + m < hi ? bas_delay_sample(row, -(long)H, hi, (long)k * K, j, K, drow[k], drow[k + 1], dmin, dhi, interp)
                               : 0.f;
            if (++j == K) { j = 0; ++k; }
        }
        if (quads && t0 + 3 < T) {
            f32x4 o;
            o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
            *reinterpret_cast<f32x4 *>(out + t0) = o;
        } else {
            for (int m = 0; m < 4 && t0 + m < T; ++m) out[t0 + m] = v[m];
        }
    }
}

// One workgroup per row: row[0 .. H) = row[B .. B + H) in passes of DL_THREADS samples, front to back, each pass reading
// before it writes.  A pass writes [j0, j0 + 256) and later passes read from B + j0 + 256 on, so the overlapping case
// B < H moves correctly too.
__global__ __launch_bounds__(DL_THREADS) void bas_delay_carry_kernel(float *x, long x_g, long x_s, int n_src, int H, long B) {
    const int r = blockIdx.x;
    const int g = r / n_src, s = r - g * n_src;
    float *row = x + g * x_g + s * x_s;
    for (int j0 = 0; j0 < H; j0 += DL_THREADS) {
        const int j = j0 + threadIdx.x;
        const float v = j < H ? row[B + j] : 0.f;
        __syncthreads();
        if (j < H) row[j] = v;
        __syncthreads();
    }
}

extern "C" int bas_delay_rows_f32(const float *x, long x_stride_g, long x_stride_s, int H, const long *lengths,
                                  const double *delay, long d_stride_g, long d_stride_s, int n_groups, int n_src, long T,
                                  int K, int interp, double max_delay, float *y, long y_stride_g, long y_stride_s,
                                  bas_stream_t stream) {
    BAS_REQUIRE(n_groups >= 0 && n_src >= 0 && T >= 0 && K > 0 && H >= 0, BAS_E_SHAPE,
                "bas_delay_rows_f32: need n_groups, n_src, T, H >= 0 and K > 0");
    BAS_REQUIRE(interp == BAS_DELAY_LINEAR || interp == BAS_DELAY_CUBIC, BAS_E_SHAPE,
                "bas_delay_rows_f32: interp must be 0 (linear) or 1 (cubic)");
    BAS_REQUIRE(T < (1L << 30), BAS_E_SHAPE, "bas_delay_rows_f32: T (%ld) must be below 2^30", T);
    BAS_REQUIRE((long)n_groups * n_src <= 65535, BAS_E_SHAPE, "bas_delay_rows_f32: more than 65535 rows in one call");
    BAS_REQUIRE(max_delay == 0.0 || (max_delay >= (interp == BAS_DELAY_CUBIC ? 2.0 : 1.0) && max_delay + 2.0 <= (double)H),
                BAS_E_SHAPE, "bas_delay_rows_f32: max_delay must be 0 (offline) or in [d_min, H - 2]");
    if ((long)n_groups * n_src == 0 || T == 0) return 0;
    BAS_REQUIRE(x && delay && y, BAS_E_NULL, "bas_delay_rows_f32: null pointer");
    const long nq = (T + 3) >> 2;
    const long bx = (nq + DL_THREADS - 1) / DL_THREADS;
    const dim3 grid((unsigned)(bx < 65535 ? bx : 65535), (unsigned)(n_groups * n_src));
    hipLaunchKernelGGL(bas_delay_rows_kernel, grid, dim3(DL_THREADS), 0, bas_stream(stream), x, x_stride_g, x_stride_s, H,
                       lengths, delay, d_stride_g, d_stride_s, n_src, (int)T, K, interp, max_delay, y, y_stride_g,
                       y_stride_s);
    return bas_check_launch("bas_delay_rows_f32");
}

extern "C" int bas_delay_carry_f32(float *x, long x_stride_g, long x_stride_s, int n_groups, int n_src, int H, long B,
                                   bas_stream_t stream) {
    BAS_REQUIRE(n_groups >= 0 && n_src >= 0 && H >= 0 && B > 0, BAS_E_SHAPE,
                "bas_delay_carry_f32: need n_groups, n_src, H >= 0 and B > 0");
    BAS_REQUIRE((long)n_groups * n_src <= 0x7fffffffL, BAS_E_SHAPE, "bas_delay_carry_f32: n_groups n_src must be below 2^31");
    if ((long)n_groups * n_src == 0 || H == 0) return 0;
    BAS_REQUIRE(x, BAS_E_NULL, "bas_delay_carry_f32: null pointer");
    hipLaunchKernelGGL(bas_delay_carry_kernel, dim3((unsigned)(n_groups * n_src)), dim3(DL_THREADS), 0, bas_stream(stream), x,
                       x_stride_g, x_stride_s, n_src, H, B);
    return bas_check_launch("bas_delay_carry_f32");
}
