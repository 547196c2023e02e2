// Head tracking, standalone (include/bas.h "head tracking"): world-frame angles [G][n_src][nb] and head
// orientations [G][nb][4] -> head-relative angles, strided on both sides, in place allowed.  The stream batch's dense
// inputs take the same rotation inside its pack launch instead (bas_stream_batch_pack_head_f32); both run bas_head_relative.
#include "bas_internal.h"
#include "bas_head.h"

#define HR_THREADS 256

// one thread per (g, s, c) item, grid-stride.  No __restrict__: out may be in (each item reads its two angles before it
// writes them, and no other item touches them).
__global__ __launch_bounds__(HR_THREADS) void bas_head_relative_kernel(
    const double *elev, const double *azim, long in_g, long in_s, const double *__restrict__ head, long head_g,
    long head_c, int n_src, int nb, long n_items, double *elev_out, double *azim_out, long out_g, long out_s) {
    const long per_g = (long)n_src * nb;
    for (long i = blockIdx.x * (long)HR_THREADS + threadIdx.x; i < n_items; i += (long)gridDim.x * HR_THREADS) {
        const long g = i / per_g, r = i - g * per_g;
        const long s = r / nb, c = r - s * nb;
        const double *q = head + g * head_g + c * head_c;
        const long from = g * in_g + s * in_s + c, to = g * out_g + s * out_s + c;
        double el_h, az_h;
        bas_head_relative(q[0], q[1], q[2], q[3], elev[from], azim[from], el_h, az_h);
        elev_out[to] = el_h;
        azim_out[to] = az_h;
    }
}

// the written layout [G][n_src][nb] with strides (sg, ss, 1) addresses no element twice (bas_internal.h)
static bool hr_one_to_one(int G, int n_src, int nb, long sg, long ss) { return bas_layout_one_to_one(G, n_src, nb, sg, ss); }


extern "C" int bas_head_relative_f64(const double *elev, const double *azim, long in_stride_g, long in_stride_s,
                                     const double *head, long head_stride_g, long head_stride_c, int n_groups, int n_src,
                                     int nb, double *elev_out, double *azim_out, long out_stride_g, long out_stride_s,
                                     bas_stream_t stream) {
    BAS_REQUIRE(n_groups > 0 && n_src > 0 && nb > 0, BAS_E_SHAPE,
                "bas_head_relative_f64: need n_groups, n_src, nb > 0 (G=%d n_src=%d nb=%d)", n_groups, n_src, nb);
    BAS_REQUIRE(in_stride_g >= 0 && in_stride_s >= 0 && head_stride_g >= 0 && head_stride_c >= 4, BAS_E_SHAPE,
                "bas_head_relative_f64: need non-negative strides and head_stride_c >= 4 (in %ld %ld, head %ld %ld)",
                in_stride_g, in_stride_s, head_stride_g, head_stride_c);
    BAS_REQUIRE(out_stride_g >= 0 && out_stride_s >= 0 && hr_one_to_one(n_groups, n_src, nb, out_stride_g, out_stride_s),
                BAS_E_SHAPE, "bas_head_relative_f64: output strides (%ld, %ld, 1) overlap for [%d][%d][%d]", out_stride_g,
                out_stride_s, n_groups, n_src, nb);
    BAS_REQUIRE(elev && azim && head && elev_out && azim_out, BAS_E_NULL, "bas_head_relative_f64: null pointer");
    BAS_REQUIRE(elev_out != azim_out, BAS_E_SHAPE, "bas_head_relative_f64: elev_out and azim_out are one buffer");
    BAS_REQUIRE(((elev_out != elev && azim_out != azim) || (out_stride_g == in_stride_g && out_stride_s == in_stride_s)),
                BAS_E_SHAPE, "bas_head_relative_f64: in place needs the input strides (%ld, %ld) on the output (%ld, %ld)",
                in_stride_g, in_stride_s, out_stride_g, out_stride_s);
    BAS_REQUIRE(bas_aligned(elev, 8) && bas_aligned(azim, 8) && bas_aligned(head, 8) && bas_aligned(elev_out, 8) &&
                bas_aligned(azim_out, 8), BAS_E_ALIGN, "bas_head_relative_f64: float64 arrays must be 8-byte aligned");
    const long n_items = (long)n_groups * n_src * nb;
    const int blocks = bas_grid_for(n_items, 8 * bas_device_cus());
    hipLaunchKernelGGL(bas_head_relative_kernel, dim3(blocks), dim3(HR_THREADS), 0, bas_stream(stream), elev, azim,
                       in_stride_g, in_stride_s, head, head_stride_g, head_stride_c, n_src, nb, n_items, elev_out,
                       azim_out, out_stride_g, out_stride_s);
    return bas_check_launch("bas_head_relative_f64");
}
