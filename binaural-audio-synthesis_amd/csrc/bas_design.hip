// Colour design on the device (include/bas.h "colour design"):
//   bas_color_design_f32 - the band log-magnitudes of every (group, row, boundary) -> the M float32 taps of its
//                          minimum-phase FIR, written where bas_color_rows_f32 reads them (a stream's color_view).  One launch.
#include "bas_internal.h"
#include "bas_design.h"

#define DS_THREADS 64                   // one wave per workgroup: a lane per filter
#define DS_PITCH (DS_THREADS + 1)       // h's row pitch: the store pass reads it along m, 65 doubles apart (all banks)

struct BasDesignArgs {
    const double *logmag; long l_g, l_s, l_k;
    const double *basis;
    int n_bands, M;
    double floor;
    long rows, nb;
    float *color; long c_g, c_s, c_k;
};

// Dynamic LDS, doubles: basis [n_bands][M] | c [M][DS_THREADS] | h [M][DS_PITCH] | out offsets [DS_THREADS] (as long).
// A workgroup takes 64 consecutive filters (k fastest) per pass.  Pass 1: lane f runs bas_design_filter on filter
// base + f with c and h at a lane stride, so that the run-time indexed reads of the recursion, c[k] and h[n - k], are one
// bank row per half wave (8 bytes per lane, consecutive lanes): no conflicts, the basis a broadcast.  Pass 2: the 64 M taps
// leave through LDS transposed - lane e of a pass stores tap e % M of filter e / M, so that a wave's stores are runs of M
// consecutive floats (a filter per lane would store 64 floats M apart) - and h's pitch of 65 doubles keeps the reads of
// that pass on distinct banks for consecutive m.
__global__ __launch_bounds__(DS_THREADS) void bas_color_design_kernel(BasDesignArgs A, long n_filters) {
    extern __shared__ __attribute__((aligned(16))) double ds_lds[];
    const int M = A.M, tid = threadIdx.x;
    double *bs = ds_lds;
    double *c = bs + A.n_bands * M;
    double *h = c + M * DS_THREADS;
    long *off = reinterpret_cast<long *>(h + M * DS_PITCH);
    for (int i = tid; i < A.n_bands * M; i += DS_THREADS) bs[i] = A.basis[i];
    __syncthreads();
    const long per_g = A.rows * A.nb;
    for (long base = (long)blockIdx.x * DS_THREADS; base < n_filters; base += (long)gridDim.x * DS_THREADS) {
        const long it = base + tid;
        if (it < n_filters) {
            const long g = it / per_g, r0 = it - g * per_g;
            const long s = r0 / A.nb, k = r0 - s * A.nb;
            off[tid] = g * A.c_g + s * A.c_s + k * A.c_k;
            bas_design_filter(A.logmag + g * A.l_g + s * A.l_s + k * A.l_k, bs, A.n_bands, M, A.floor, c + tid, DS_THREADS,
                              h + tid, DS_PITCH);
        }
        __syncthreads();
        const long left = n_filters - base;
        const int n_here = (int)(left < DS_THREADS ? left : DS_THREADS);
        for (int e = tid; e < n_here * M; e += DS_THREADS) {
            const int f = e / M, m = e - f * M;
            A.color[off[f] + m] = (float)h[m * DS_PITCH + f];
        }
        __syncthreads();                                                  // (the next pass overwrites c, h and off)
    }
}


extern "C" int bas_color_design_f32(const double *logmag, long l_stride_g, long l_stride_s, long l_stride_k,
                                    const double *basis, int n_bands, int M, double logmag_floor, int n_groups, int n_src,
                                    int nb, float *color, long c_stride_g, long c_stride_s, long c_stride_k,
                                    bas_stream_t stream) {
    const char *fn = "bas_color_design_f32";
    BAS_REQUIRE(n_groups >= 0 && n_src >= 0 && nb >= 0, BAS_E_SHAPE, "%s: need n_groups, n_src, nb >= 0", fn);
    BAS_REQUIRE(M >= 1 && M <= BAS_DESIGN_MAX_TAPS, BAS_E_SHAPE, "%s: M (%d) must be in 1..%d", fn, M, BAS_DESIGN_MAX_TAPS);
    BAS_REQUIRE(n_bands >= 1 && n_bands <= BAS_DESIGN_MAX_BANDS, BAS_E_SHAPE, "%s: n_bands (%d) must be in 1..%d", fn,
                n_bands, BAS_DESIGN_MAX_BANDS);
    BAS_REQUIRE(logmag_floor <= 0.0 && logmag_floor > -HUGE_VAL, BAS_E_SHAPE,
                "%s: the log-magnitude floor (%g) must be finite and <= 0", fn, logmag_floor);
    BAS_REQUIRE((long)n_groups * n_src * nb < (1L << 40), BAS_E_SHAPE, "%s: more than 2^40 filters in one call", fn);
    BAS_REQUIRE(l_stride_g >= 0 && l_stride_s >= 0 && l_stride_k >= 0 && l_stride_g < (1L << 40) && l_stride_s < (1L << 40) &&
                l_stride_k < (1L << 40), BAS_E_SHAPE, "%s: logmag strides must be in 0..2^40", fn);
    if ((long)n_groups * n_src * nb == 0) return 0;
    // taps at [g c_stride_g + s c_stride_s + k c_stride_k + m]: a boundary's M must not meet the next one's, and the rows'
    // extents (nb - 1) c_stride_k + M are held to the rule of the scene outputs (bas_internal.h)
    long extent = 0;
    BAS_REQUIRE(c_stride_g >= 0 && c_stride_s >= 0 && c_stride_k >= M &&
                !__builtin_mul_overflow((long)(nb - 1), c_stride_k, &extent) &&
                !__builtin_add_overflow(extent, (long)M, &extent) &&
                bas_layout_one_to_one(n_groups, n_src, extent, c_stride_g, c_stride_s), BAS_E_SHAPE,
                "%s: output strides (%ld, %ld, %ld, 1) overlap for [%d][%d][%d][%d] (c_stride_k must be >= M)", fn, c_stride_g,
                c_stride_s, c_stride_k, n_groups, n_src, nb, M);
    BAS_REQUIRE(logmag && basis && color, BAS_E_NULL, "%s: null pointer", fn);
    BAS_REQUIRE(bas_aligned(logmag, 8) && bas_aligned(basis, 8) && bas_aligned(color, 4), BAS_E_ALIGN,
                "%s: logmag and basis must be 8-byte aligned, color 4-byte", fn);
    BasDesignArgs A;
    A.logmag = logmag; A.l_g = l_stride_g; A.l_s = l_stride_s; A.l_k = l_stride_k;
    A.basis = basis; A.n_bands = n_bands; A.M = M; A.floor = logmag_floor;
    A.rows = n_src; A.nb = nb;
    A.color = color; A.c_g = c_stride_g; A.c_s = c_stride_s; A.c_k = c_stride_k;
    const long n_filters = (long)n_groups * n_src * nb;
    const size_t lds = sizeof(double) * ((size_t)n_bands * M + (size_t)M * DS_THREADS + (size_t)M * DS_PITCH + DS_THREADS);
    const hipError_t e = bas_allow_full_lds(reinterpret_cast<const void *>(bas_color_design_kernel));
    if (e != hipSuccess) return bas_fail((int)e, "%s: hipFuncSetAttribute: %s", fn, hipGetErrorString(e));
    const long passes = (n_filters + DS_THREADS - 1) / DS_THREADS;
    const long cap = 16L * bas_device_cus();
    hipLaunchKernelGGL(bas_color_design_kernel, dim3((unsigned)(passes < cap ? passes : cap)), dim3(DS_THREADS), lds,
                       bas_stream(stream), A, n_filters);
    return bas_check_launch(fn);
}
