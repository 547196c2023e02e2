// Ambisonic beds (include/bas.h "ambisonic beds"):
//   bas_ambi_matrices_f32 - head orientations at chunk boundaries -> mixing matrices M = D Rot(q), one launch;
//   bas_matrix_mix_f32    - the hot path: y_v(t) = sum_c M(t)[v][c] x_c(t) with M interpolated between chunk boundaries,
//                           strided rows in and out (a renderer's input rows are written in place), one launch.
#include "bas_internal.h"
#include "bas_ambi.h"

// One workgroup per (group, boundary); Q is staged in LDS.  Thread j < J evaluates Y at R^T s_j into LDS; the 84 (order 3)
// entries of the order blocks of Rot are sums over j ascending from +0; the V C entries of M are sums over b ascending over c's order block.  All
// binary64 without contraction, one rounding to binary32.  The identity (bas_ambi_unit_head) stores (float)D.
__global__ __launch_bounds__(AMBI_THREADS) void bas_ambi_matrices_kernel(
    const double *__restrict__ head, long hs_g, long hs_c, const double *__restrict__ D, const double *__restrict__ Q,
    const double *__restrict__ S, int J, int order, int V, int nb, float *__restrict__ m, long ms_g, long ms_k) {
#pragma clang fp contract(off)
    __shared__ double Ys[AMBI_MAX_J][AMBI_MAX_C + 1];
    __shared__ double Rot[AMBI_MAX_C][AMBI_MAX_C];
    __shared__ double Qs[AMBI_MAX_J * AMBI_MAX_C];
    const int C = (order + 1) * (order + 1);
    const long gk = blockIdx.x;
    const long g = gk / nb, k = gk - g * nb;
    const double *q = head + g * hs_g + k * hs_c;
    float *out = m + g * ms_g + k * ms_k;
    double w = q[0], x = q[1], y = q[2], z = q[3];
    if (bas_ambi_unit_head(w, x, y, z)) {
        for (int i = threadIdx.x; i < V * C; i += AMBI_THREADS) out[i] = (float)D[i];
        return;
    }
    for (int i = threadIdx.x; i < J * C; i += AMBI_THREADS) Qs[i] = Q[i];
    if ((int)threadIdx.x < J) {
        const int j = threadIdx.x;
        double hx, hy, hz, Y[AMBI_MAX_C];
        bas_ambi_rotate_t(w, x, y, z, S[3 * j], S[3 * j + 1], S[3 * j + 2], hx, hy, hz);
        bas_sh_n3d(hx, hy, hz, order, Y);
#pragma unroll
        for (int a = 0; a < AMBI_MAX_C; ++a)
            if (a < C) Ys[j][a] = Y[a];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += AMBI_THREADS) {
        const int a = i / C, b = i - a * C;
        const int la = a >= 9 ? 3 : a >= 4 ? 2 : a >= 1 ? 1 : 0, lb = b >= 9 ? 3 : b >= 4 ? 2 : b >= 1 ? 1 : 0;
        double acc = 0.0;
        if (la == lb)
            for (int j = 0; j < J; ++j) acc = acc + Ys[j][a] * Qs[j * C + b];
        Rot[a][b] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < V * C; i += AMBI_THREADS) {
        const int v = i / C, c = i - v * C;
        const int l = c >= 9 ? 3 : c >= 4 ? 2 : c >= 1 ? 1 : 0;
        double acc = 0.0;
        for (int b = l * l; b < (l + 1) * (l + 1); ++b) acc = acc + D[v * C + b] * Rot[b][c];
        out[i] = (float)acc;
    }
}

// One workgroup per (tile, group, slice of speaker rows): blockIdx.y is the group, blockIdx.x strides over the tiles,
// blockIdx.z takes the rows [z v_per, (z + 1) v_per) - one slice for long signals, where the inputs are then read once, more
// where tiles and groups alone would leave most of the chip idle (a stream block).  LDS holds the slice's rows of the matrices
// of the boundaries the tile touches, each row padded with zeros to CP = C rounded up to 4 columns (a zero column adds an exact
// zero to a sum that is never -0).  A lane makes outputs t .. t + 3: it holds the C x 4 inputs in registers and walks the
// V rows, per row one quad of each matrix per four columns - the same address for every lane of a chunk, a broadcast -
// and 4 C (STATIC) or 8 C fused multiply-adds, c ascending, then one 16-byte store.  Lanes whose four outputs straddle a chunk
// boundary (K not a multiple of 4) do theirs one by one, the same operations in the same order.  Nothing depends on t0: an
// output's bits are a function of (j, K, M_k, M_{k+1}) and its C inputs alone.
template <int CP, bool STATIC>
__global__ __launch_bounds__(MM_THREADS) void bas_matrix_mix_kernel(
    const float *__restrict__ x, long xs_g, long xs_c, const float *__restrict__ m, long ms_g, long ms_k, int C, int V, int T,
    int K, int tile, int v_per, float *__restrict__ y, long ys_g, long ys_v) {
    __shared__ __attribute__((aligned(16))) float ms[MM_LDS_FLOATS];
    const int g = blockIdx.y;
    const int v0 = blockIdx.z * v_per, v1 = min(v0 + v_per, V);      // the slice's rows
    const float *xg = x + g * xs_g;
    const float *mg = m + g * ms_g;
    float *yg = y + g * ys_g;
    const int set_floats = (v1 - v0) * CP;
    const float inv_K = 1.0f / (float)K;
    const int n_tiles = (T + tile - 1) / tile;
    for (int it = blockIdx.x; it < n_tiles; it += gridDim.x) {
        const int t0 = it * tile;
        const int t1 = min(t0 + tile, T);                                // the tile's outputs are [t0, t1)
        // ---- matrices: the boundaries k0 .. k1 + 1 (STATIC: the one matrix)
        const int k0 = t0 / K;
        const int n_sets = STATIC ? 1 : (t1 - 1) / K - k0 + 2;
        for (int i = threadIdx.x; i < n_sets * set_floats; i += MM_THREADS) {
            const int set = i / set_floats, r = i - set * set_floats;
            const int v = r / CP, c = r - v * CP;
            ms[i] = c < C ? mg[(long)(k0 + set) * ms_k + (v0 + v) * C + c] : 0.f;
        }
        __syncthreads();
        const int tl = t0 + (threadIdx.x << 2);
        if (tl < t1) {
            // ---- inputs: C rows of four samples, zeros past T and in the padding columns
            float xr[CP][4];
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                xr[c][0] = xr[c][1] = xr[c][2] = xr[c][3] = 0.f;
                if (c < C) {
                    const float *row = xg + c * xs_c;
                    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0 && tl + 3 < T) {
                        const f32x4 q = *reinterpret_cast<const f32x4 *>(row + tl);
                        xr[c][0] = q.x; xr[c][1] = q.y; xr[c][2] = q.z; xr[c][3] = q.w;
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (tl + i < T) xr[c][i] = row[tl + i];
                    }
                }
            }
            const int k = tl / K, j = tl - k * K;
            const bool one_chunk = STATIC || j + 3 < K;                   // the lane's four outputs share a chunk
            for (int v = 0; v < v1 - v0; ++v) {
                float o[4];
                if (one_chunk) {
                    const f32x4 *ma = reinterpret_cast<const f32x4 *>(ms + (STATIC ? 0 : (k - k0) * set_floats) + v * CP);
                    const f32x4 *mb = reinterpret_cast<const f32x4 *>(ms + (STATIC ? 0 : (k - k0 + 1) * set_floats) + v * CP);
                    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int cq = 0; cq < CP / 4; ++cq) {
                        const f32x4 qa = ma[cq];
                        const float ta[4] = {qa.x, qa.y, qa.z, qa.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int i = 0; i < 4; ++i) a[i] = fmaf(ta[e], xr[4 * cq + e][i], a[i]);
                        if (!STATIC) {
                            const f32x4 qb = mb[cq];
                            const float tb[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                            for (int e = 0; e < 4; ++e)
#pragma unroll
                                for (int i = 0; i < 4; ++i) b[i] = fmaf(tb[e], xr[4 * cq + e][i], b[i]);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        o[i] = STATIC ? a[i] : bas_crossfade(a[i], b[i], (float)(j + i) * inv_K);
                } else {                                                  // a chunk boundary inside the quad: one by one
                    int ki = k, ji = j;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int last = tl + i < t1 ? ki : k;            // (past the tile's end: any matrix the tile holds)
                        const float *ma = ms + (last - k0) * set_floats + v * CP;
                        const float *mb = ma + set_floats;
                        float a = 0.f, b = 0.f;
#pragma unroll
                        for (int c = 0; c < CP; ++c) {
                            a = fmaf(ma[c], xr[c][i], a);
                            b = fmaf(mb[c], xr[c][i], b);
                        }
                        o[i] = bas_crossfade(a, b, (float)ji * inv_K);
                        if (++ji == K) { ji = 0; ++ki; }
                    }
                }
                float *out = yg + (v0 + v) * ys_v;
                if ((reinterpret_cast<uintptr_t>(out) & 15) == 0 && tl + 3 < T) {
                    f32x4 q;
                    q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
                    *reinterpret_cast<f32x4 *>(out + tl) = q;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (tl + i < T) out[tl + i] = o[i];
                }
            }
        }
        __syncthreads();                                                  // (the next tile overwrites ms)
    }
}

extern "C" int bas_ambi_matrices_f32(const double *head, long hs_g, long hs_c, const double *D, const double *Q,
                                     const double *S, int J, int order, int V, int n_groups, int nb, float *m, long ms_g,
                                     long ms_k, bas_stream_t stream) {
    BAS_REQUIRE(order >= 1 && order <= AMBI_MAX_ORDER, BAS_E_SHAPE, "bas_ambi_matrices_f32: order (%d) must be in 1..%d",
                order, AMBI_MAX_ORDER);
    BAS_REQUIRE(V >= 1 && V <= AMBI_MAX_V, BAS_E_SHAPE, "bas_ambi_matrices_f32: V (%d) must be in 1..%d", V, AMBI_MAX_V);
    BAS_REQUIRE(J >= 1 && J <= AMBI_MAX_J, BAS_E_SHAPE, "bas_ambi_matrices_f32: J (%d) must be in 1..%d", J, AMBI_MAX_J);
    BAS_REQUIRE(n_groups >= 0 && nb >= 0 && (long)n_groups * nb <= (1L << 30), BAS_E_SHAPE,
                "bas_ambi_matrices_f32: need n_groups, nb >= 0 and n_groups nb <= 2^30");
    BAS_REQUIRE(hs_g >= 0 && hs_c >= 4 && ms_g >= 0 && ms_k >= 0, BAS_E_SHAPE,
                "bas_ambi_matrices_f32: strides must be >= 0 and hs_c >= 4");
    if ((long)n_groups * nb == 0) return 0;
    const int C = (order + 1) * (order + 1);
    BAS_REQUIRE(bas_layout_one_to_one(n_groups, nb, (long)V * C, ms_g, ms_k), BAS_E_SHAPE,
                "bas_ambi_matrices_f32: the output's strides address an element twice");
    BAS_REQUIRE(head && D && Q && S && m, BAS_E_NULL, "bas_ambi_matrices_f32: null pointer");
    BAS_REQUIRE(bas_aligned(head, 8) && bas_aligned(D, 8) && bas_aligned(Q, 8) && bas_aligned(S, 8) && bas_aligned(m, 4),
                BAS_E_ALIGN, "bas_ambi_matrices_f32: head, D, Q, S must be 8-byte aligned, m 4-byte");
    hipLaunchKernelGGL(bas_ambi_matrices_kernel, dim3((unsigned)((long)n_groups * nb)), dim3(AMBI_THREADS), 0,
                       bas_stream(stream), head, hs_g, hs_c, D, Q, S, J, order, V, nb, m, ms_g, ms_k);
    return bas_check_launch("bas_ambi_matrices_f32");
}

template <int CP>
static void ambi_launch_mix(bool is_static, dim3 grid, hipStream_t st, const float *x, long xs_g, long xs_c, const float *m,
                            long ms_g, long ms_k, int C, int V, int T, int K, int tile, int v_per, float *y, long ys_g,
                            long ys_v) {
    if (is_static)
        hipLaunchKernelGGL((bas_matrix_mix_kernel<CP, true>), grid, dim3(MM_THREADS), 0, st, x, xs_g, xs_c, m, ms_g, ms_k, C,
                           V, T, K, tile, v_per, y, ys_g, ys_v);
    else
        hipLaunchKernelGGL((bas_matrix_mix_kernel<CP, false>), grid, dim3(MM_THREADS), 0, st, x, xs_g, xs_c, m, ms_g, ms_k, C,
                           V, T, K, tile, v_per, y, ys_g, ys_v);
}

extern "C" int bas_matrix_mix_f32(const float *x, long xs_g, long xs_c, const float *m, long ms_g, long ms_k, int C, int V,
                                  int n_groups, long T, int K, float *y, long ys_g, long ys_v, bas_stream_t stream) {
    BAS_REQUIRE(C >= 1 && C <= AMBI_MAX_C, BAS_E_SHAPE, "bas_matrix_mix_f32: C (%d) must be in 1..%d", C, AMBI_MAX_C);
    BAS_REQUIRE(V >= 1 && V <= AMBI_MAX_V, BAS_E_SHAPE, "bas_matrix_mix_f32: V (%d) must be in 1..%d", V, AMBI_MAX_V);
    BAS_REQUIRE(n_groups >= 0 && n_groups <= 65535 && T >= 0 && K > 0, BAS_E_SHAPE,
                "bas_matrix_mix_f32: need 0 <= n_groups <= 65535, T >= 0 and K > 0");
    BAS_REQUIRE(T < (1L << 30), BAS_E_SHAPE, "bas_matrix_mix_f32: T (%ld) must be below 2^30", T);
    BAS_REQUIRE(bas_none_negative({xs_g, xs_c, ms_g, ms_k, ys_g, ys_v}), BAS_E_SHAPE,
                "bas_matrix_mix_f32: strides must be >= 0");
    BAS_REQUIRE(bas_all_below(1L << 40, {xs_g, xs_c, ms_g, ms_k, ys_g, ys_v}), BAS_E_SHAPE,
                "bas_matrix_mix_f32: strides must be below 2^40");
    BAS_REQUIRE(ms_k == 0 || ms_k >= (long)V * C, BAS_E_SHAPE,
                "bas_matrix_mix_f32: ms_k must be 0 (static) or >= V C (the matrices of two boundaries overlap)");
    if (n_groups == 0 || T == 0) return 0;
    BAS_REQUIRE(bas_layout_one_to_one(n_groups, V, T, ys_g, ys_v), BAS_E_SHAPE,
                "bas_matrix_mix_f32: the output's strides address an element twice");
    BAS_REQUIRE(x && m && y, BAS_E_NULL, "bas_matrix_mix_f32: null pointer");
    BAS_REQUIRE(bas_aligned(x, 4) && bas_aligned(m, 4) && bas_aligned(y, 4), BAS_E_ALIGN,
                "bas_matrix_mix_f32: x, m, y must be 4-byte aligned");
    const long x_ext[3] = {n_groups, C, T}, x_str[3] = {xs_g, xs_c, 1};
    const long y_ext[3] = {n_groups, V, T}, y_str[3] = {ys_g, ys_v, 1};
    const size_t y_bytes = 4 * (size_t)bas_view_extent(3, y_ext, y_str);
    BAS_REQUIRE(!bas_ranges_meet(x, 4 * (size_t)bas_view_extent(3, x_ext, x_str), y, y_bytes), BAS_E_SHAPE,
                "bas_matrix_mix_f32: input and output overlap (the mix does not run in place)");
    const long n_k = ms_k == 0 ? 1 : (T - 1) / K + 2;
    const long m_ext[3] = {n_groups, n_k, (long)V * C}, m_str[3] = {ms_g, ms_k, 1};
    BAS_REQUIRE(!bas_ranges_meet(m, 4 * (size_t)bas_view_extent(3, m_ext, m_str), y, y_bytes), BAS_E_SHAPE,
                "bas_matrix_mix_f32: matrices and output overlap");
    // a tile touches (tile - 1) / K + 3 boundaries at most, and LDS holds MM_LDS_FLOATS / (V CP) matrices (>= 8): whole
    // tiles where the chunks are long enough, shorter ones (a multiple of 4 samples) below
    const int CP = (C + 3) & ~3;
    const long fit = ((long)(MM_LDS_FLOATS / (V * CP)) - 2) * K;
    const int tile = fit >= MM_TILE ? MM_TILE : (int)(fit & ~3L);
    const long n_tiles = (T + tile - 1) / tile;
    // slices of speaker rows where tiles x groups are fewer workgroups than the chip has CUs: MM_FILL workgroups then (every
    // slice reads the inputs again, which a long signal must not: it is bound by those bytes)
    const long n_wg = (n_tiles < 65535 ? n_tiles : 65535) * n_groups;
    const long want = 2 * n_wg >= MM_FILL ? 1 : (MM_FILL + n_wg - 1) / n_wg;
    const int v_per = (int)((V + want - 1) / want) > 0 ? (int)((V + want - 1) / want) : 1;
    const dim3 grid((unsigned)(n_tiles < 65535 ? n_tiles : 65535), (unsigned)n_groups, (unsigned)((V + v_per - 1) / v_per));
    const hipStream_t st = bas_stream(stream);
    const bool is_static = ms_k == 0;
    switch (CP) {
    case 4: ambi_launch_mix<4>(is_static, grid, st, x, xs_g, xs_c, m, ms_g, ms_k, C, V, (int)T, K, tile, v_per, y, ys_g, ys_v); break;
    case 8: ambi_launch_mix<8>(is_static, grid, st, x, xs_g, xs_c, m, ms_g, ms_k, C, V, (int)T, K, tile, v_per, y, ys_g, ys_v); break;
    case 12: ambi_launch_mix<12>(is_static, grid, st, x, xs_g, xs_c, m, ms_g, ms_k, C, V, (int)T, K, tile, v_per, y, ys_g, ys_v); break;
    default: ambi_launch_mix<16>(is_static, grid, st, x, xs_g, xs_c, m, ms_g, ms_k, C, V, (int)T, K, tile, v_per, y, ys_g, ys_v); break;
    }
    return bas_check_launch("bas_matrix_mix_f32");
}

// ---- the encoder (include/bas.h "ambisonic encoder") -----------------------------------------------------
//   bas_ambi_encode_gains_f32 - source directions and gains at chunk boundaries -> encoding banks E [nb][n_src][C], one launch;
//   bas_ambi_encode_f32       - the hot path: bed_c(t) = base_c(t) + sum_s E(t)[s][c] x_s(t), the reduction in the two-level
//                               order of bas.h (blocks of ENCODE_BLOCK sources), one launch.
struct ambi_scale_t {
    double v[AMBI_MAX_ORDER + 1];
};

// One thread per (group, boundary, source): binary64 without contraction, one rounding to binary32 per coefficient.
__global__ __launch_bounds__(AMBI_THREADS) void bas_ambi_encode_gains_kernel(
    const double *__restrict__ elev, const double *__restrict__ azim, long as_g, long as_s, const double *__restrict__ gain,
    long gs_g, long gs_s, ambi_scale_t scale, int order, long total, int n_src, int nb, float *__restrict__ e, long es_g,
    long es_k) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * AMBI_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int C = (order + 1) * (order + 1);
    const long gk = idx / n_src;
    const int s = (int)(idx - gk * n_src);
    const long g = gk / nb, k = gk - g * nb;
    const double el = elev[g * as_g + s * as_s + k], az = azim[g * as_g + s * as_s + k];
    const double gn = gain ? gain[g * gs_g + s * gs_s + k] : 1.0;
    const double ce = cos(el);
    double Y[AMBI_MAX_C];
    bas_sh_n3d(-sin(az) * ce, cos(az) * ce, sin(el), order, Y);
    float *out = e + g * es_g + k * es_k + (long)s * C;
#pragma unroll
    for (int c = 0; c < AMBI_MAX_C; ++c)
        if (c < C) out[c] = (float)((gn * scale.v[c >= 9 ? 3 : c >= 4 ? 2 : c >= 1 ? 1 : 0]) * Y[c]);
}

// Four samples of a row at tl: one 16-byte load where the row is 16-byte aligned and the quad inside T, else one by one
// (zeros past T).
__device__ __forceinline__ f32x4 enc_load4(const float *row, int tl, int T) {
    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0 && tl + 3 < T) return *reinterpret_cast<const f32x4 *>(row + tl);
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    if (tl < T) q.x = row[tl];
    if (tl + 1 < T) q.y = row[tl + 1];
    if (tl + 2 < T) q.z = row[tl + 2];
    if (tl + 3 < T) q.w = row[tl + 3];
    return q;
}

// One workgroup per (tile, slice of channels) and group: blockIdx.y is the group, blockIdx.x strides over tiles x slices with
// the slices of a tile next to each other (they read the same x).  A workgroup takes CW = CPS SPLIT channels: with SPLIT = 2
// its two halves of 128 lanes take the two slices of CPS channels of the SAME tile of 512 outputs, so that the second read
// of x is served by the caches of that CU and x comes from HBM once.  A lane makes outputs t .. t + 3 of every channel of
// its slice.  The sources are walked in slabs of `slab` (a multiple of ENCODE_BLOCK,
// so that slab edges are block edges and never show in the bits): per slab the slice's columns of the banks of the
// boundaries the tile touches are staged in LDS as [n_sets][slab][CW], padding columns zero; then per source one quad of x
// from global memory, CPS / 4 broadcast 16-byte LDS reads per bank and 4 CPS (STATIC) or 8 CPS fused multiply-adds into the
// block sums a, b, which join the totals A, B after every ENCODE_BLOCK sources - the order of bas.h.  A total starts at +0
// and A = 0 + A_0 is A_0 bit for bit: a block sum from +0 is never -0.  Lanes whose four outputs straddle a chunk boundary
// read each output's own banks, the same operations in the same order.
template <int CPS, bool STATIC, int SPLIT>
__global__ __launch_bounds__(ENC_THREADS) void bas_ambi_encode_kernel(
    const float *__restrict__ x, long xs_g, long xs_s, const float *__restrict__ e, long es_g, long es_k, int n_src, int C,
    int T, int K, int tile, int slab, int n_slices, const float *base, long bs_g, long bs_c, float *y, long ys_g,
    long ys_c) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float es[ENC_LDS_FLOATS];
    const int g = blockIdx.y;
    const float *xg = x + g * xs_g;
    const float *eg = e + g * es_g;
    const float *bg = base ? base + g * bs_g : nullptr;
    float *yg = y + g * ys_g;
    constexpr int CW = CPS * SPLIT, LANES = ENC_THREADS / SPLIT;          // the workgroup's columns; lanes per slice
    const int zl = threadIdx.x / LANES, li = threadIdx.x - zl * LANES;
    const int set_floats = slab * CW;
    const float inv_K = 1.0f / (float)K;
    const int n_tiles = (T + tile - 1) / tile;
    const long n_work = (long)n_tiles * n_slices;
    for (long wk = blockIdx.x; wk < n_work; wk += gridDim.x) {
        const int it = (int)(wk / n_slices), z = (int)(wk - (long)it * n_slices);
        const int w0 = z * CW;                                               // the workgroup's first channel
        const int c0 = w0 + zl * CPS, c1 = min(c0 + CPS, C);                // the lane's slice of channels
        const int t0 = it * tile;
        const int t1 = min(t0 + tile, T);                                    // the tile's outputs are [t0, t1)
        const int k0 = t0 / K;
        const int n_sets = STATIC ? 1 : (t1 - 1) / K - k0 + 2;
        const int tl = t0 + (li << 2);
        const bool active = tl < t1 && c0 < C;
        const int k = tl / K, j = tl - k * K;
        const bool one_chunk = STATIC || j + 3 < K;                          // the lane's four outputs share a chunk
        int off[4] = {0, 0, 0, 0};                                           // per output: its first bank in es
        if (!STATIC) {
            int ki = k, ji = j;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                off[i] = ((tl + i < t1 ? ki : k) - k0) * set_floats;         // (past the tile's end: a bank the tile holds)
                if (++ji == K) { ji = 0; ++ki; }
            }
        }
        float A[CPS][4], B[STATIC ? 1 : CPS][4];
#pragma unroll
        for (int c = 0; c < CPS; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                A[c][i] = 0.f;
                if constexpr (!STATIC) B[c][i] = 0.f;
            }
        for (int s0 = 0; s0 < n_src; s0 += slab) {
            const int ns = min(slab, n_src - s0);
            __syncthreads();                                                 // (the previous slab, or tile, is read)
            for (int i = threadIdx.x; i < n_sets * ns * CW; i += ENC_THREADS) {
                const int set = i / (ns * CW), r = i - set * (ns * CW);
                const int s = r / CW, c = r - s * CW;
                es[set * set_floats + s * CW + c] = w0 + c < C ? eg[(long)(k0 + set) * es_k + (long)(s0 + s) * C + w0 + c] : 0.f;
            }
            __syncthreads();
            if (!active) continue;
            for (int b0 = 0; b0 < ns; b0 += ENCODE_BLOCK) {
                const int nbk = min(ENCODE_BLOCK, ns - b0);
                const float *xrow = xg + (long)(s0 + b0) * xs_s;
                float a[CPS][4], b[STATIC ? 1 : CPS][4];
#pragma unroll
                for (int c = 0; c < CPS; ++c)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        a[c][i] = 0.f;
                        if constexpr (!STATIC) b[c][i] = 0.f;
                    }
                if (one_chunk) {
                    const float *pa = es + off[0] + b0 * CW + zl * CPS;
                    auto step = [&](const f32x4 xq, const float *p) {       // one source: 4 CPS (8 CPS) multiply-adds
                        const float xv[4] = {xq.x, xq.y, xq.z, xq.w};
#pragma unroll
                        for (int cq = 0; cq < CPS / 4; ++cq) {
                            const f32x4 qa = *reinterpret_cast<const f32x4 *>(p + 4 * cq);
                            const float ta[4] = {qa.x, qa.y, qa.z, qa.w};
#pragma unroll
                            for (int q = 0; q < 4; ++q)
#pragma unroll
                                for (int i = 0; i < 4; ++i) a[4 * cq + q][i] = fmaf(ta[q], xv[i], a[4 * cq + q][i]);
                            if constexpr (!STATIC) {
                                const f32x4 qb = *reinterpret_cast<const f32x4 *>(p + set_floats + 4 * cq);
                                const float tb[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                                for (int q = 0; q < 4; ++q)
#pragma unroll
                                    for (int i = 0; i < 4; ++i) b[4 * cq + q][i] = fmaf(tb[q], xv[i], b[4 * cq + q][i]);
                            }
                        }
                    };
#pragma unroll 4
                    for (int s = 0; s < nbk; ++s) step(enc_load4(xrow + (long)s * xs_s, tl, T), pa + s * CW);
                } else if (!STATIC) {                                        // a chunk boundary inside the quad
                    for (int s = 0; s < nbk; ++s) {
                        const f32x4 xq = enc_load4(xrow + (long)s * xs_s, tl, T);
                        const float xv[4] = {xq.x, xq.y, xq.z, xq.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float *pa = es + off[i] + (b0 + s) * CW + zl * CPS;
#pragma unroll
                            for (int cq = 0; cq < CPS / 4; ++cq) {
                                const f32x4 qa = *reinterpret_cast<const f32x4 *>(pa + 4 * cq);
                                const f32x4 qb = *reinterpret_cast<const f32x4 *>(pa + set_floats + 4 * cq);
                                const float ta[4] = {qa.x, qa.y, qa.z, qa.w}, tb[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    a[4 * cq + q][i] = fmaf(ta[q], xv[i], a[4 * cq + q][i]);
                                    b[(STATIC ? 0 : 4 * cq + q)][i] = fmaf(tb[q], xv[i], b[(STATIC ? 0 : 4 * cq + q)][i]);
                                }
                            }
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < CPS; ++c)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        A[c][i] = A[c][i] + a[c][i];
                        if constexpr (!STATIC) B[c][i] = B[c][i] + b[c][i];
                    }
            }
        }
        if (!active) continue;
        // ---- interpolation, base, store
        float w[4] = {0.f, 0.f, 0.f, 0.f};
        if (!STATIC) {
            int ji = j;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[i] = (float)ji * inv_K;
                if (++ji == K) ji = 0;
            }
        }
#pragma unroll
        for (int c = 0; c < CPS; ++c) {
            if (c0 + c < c1) {
                float o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) o[i] = STATIC ? A[c][i] : bas_crossfade(A[c][i], B[STATIC ? 0 : c][i], w[i]);
                if (bg) {
                    const f32x4 q = enc_load4(bg + (long)(c0 + c) * bs_c, tl, T);
                    o[0] = q.x + o[0]; o[1] = q.y + o[1]; o[2] = q.z + o[2]; o[3] = q.w + o[3];
                }
                float *out = yg + (long)(c0 + c) * ys_c;
                if ((reinterpret_cast<uintptr_t>(out) & 15) == 0 && tl + 3 < T) {
                    f32x4 q;
                    q.x = o[0]; q.y = o[1]; q.z = o[2]; q.w = o[3];
                    *reinterpret_cast<f32x4 *>(out + tl) = q;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (tl + i < T) out[tl + i] = o[i];
                }
            }
        }
    }
}

extern "C" int bas_ambi_encode_gains_f32(const double *elev, const double *azim, long as_g, long as_s, const double *gain,
                                         long gs_g, long gs_s, const double *scale, int order, int n_groups, int n_src,
                                         int nb, float *e, long es_g, long es_k, bas_stream_t stream) {
    BAS_REQUIRE(order >= 1 && order <= AMBI_MAX_ORDER, BAS_E_SHAPE, "bas_ambi_encode_gains_f32: order (%d) must be in 1..%d",
                order, AMBI_MAX_ORDER);
    BAS_REQUIRE(n_src >= 1 && n_src <= ENC_MAX_SRC, BAS_E_SHAPE, "bas_ambi_encode_gains_f32: n_src (%d) must be in 1..%d",
                n_src, ENC_MAX_SRC);
    BAS_REQUIRE(n_groups >= 0 && nb >= 0 && (long)n_groups * nb <= (1L << 30) &&
                    (long)n_groups * nb * n_src <= (1L << 30),
                BAS_E_SHAPE, "bas_ambi_encode_gains_f32: need n_groups, nb >= 0 and n_groups nb n_src <= 2^30");
    BAS_REQUIRE(bas_none_negative({as_g, as_s, gs_g, gs_s, es_g, es_k}), BAS_E_SHAPE,
                "bas_ambi_encode_gains_f32: strides must be >= 0");
    BAS_REQUIRE(bas_all_below(1L << 40, {as_g, as_s, gs_g, gs_s, es_g, es_k}), BAS_E_SHAPE,
                "bas_ambi_encode_gains_f32: strides must be below 2^40");
    if ((long)n_groups * nb == 0) return 0;
    const int C = (order + 1) * (order + 1);
    BAS_REQUIRE(bas_layout_one_to_one(n_groups, nb, (long)n_src * C, es_g, es_k), BAS_E_SHAPE,
                "bas_ambi_encode_gains_f32: the output's strides address an element twice");
    BAS_REQUIRE(elev && azim && scale && e, BAS_E_NULL, "bas_ambi_encode_gains_f32: null pointer");
    BAS_REQUIRE(bas_aligned(elev, 8) && bas_aligned(azim, 8) && bas_aligned(gain, 8) && bas_aligned(scale, 8) &&
                    bas_aligned(e, 4),
                BAS_E_ALIGN, "bas_ambi_encode_gains_f32: elev, azim, gain, scale must be 8-byte aligned, e 4-byte");
    ambi_scale_t sc;
    for (int l = 0; l <= AMBI_MAX_ORDER; ++l) sc.v[l] = l <= order ? scale[l] : 0.0;   // (scale is host memory)
    const long total = (long)n_groups * nb * n_src;
    hipLaunchKernelGGL(bas_ambi_encode_gains_kernel, dim3((unsigned)((total + AMBI_THREADS - 1) / AMBI_THREADS)),
                       dim3(AMBI_THREADS), 0, bas_stream(stream), elev, azim, as_g, as_s, gain, gs_g, gs_s, sc, order, total,
                       n_src, nb, e, es_g, es_k);
    return bas_check_launch("bas_ambi_encode_gains_f32");
}

// The launcher's rule (ambisonics.encode_plan states it again for the tests): the channels per slice, the tile, the slab.
static void ambi_encode_rule(int C, long T, int K, int n_groups, bool is_static, int *cps, int *split, int *tile, int *slab) {
    const int CP = (C + 3) & ~3, cap = is_static ? ENC_STATIC_SLICE : ENC_BOUNDARY_SLICE;
    int s = CP < cap ? CP : cap, sp = CP > cap ? 2 : 1, t = 0;              // two slices of 8 inside one workgroup
    for (int pass = 0; pass < 2; ++pass) {
        // a tile touches (tile - 1) / K + 3 boundaries at most, and a slab of one block must fit LDS with all of them
        const int cw = s * sp, tile_max = ENC_TILE / sp;
        const long fit = is_static ? tile_max : ((long)(ENC_LDS_FLOATS / (ENCODE_BLOCK * cw)) - 2) * K;
        t = fit >= tile_max ? tile_max : (int)(fit & ~3L);
        const long n_wg = ((T + t - 1) / t) * ((C + cw - 1) / cw) * n_groups;
        if (pass == 1 || (s == 4 && sp == 1) || 2 * n_wg >= ENC_FILL) break;
        s = 4;                                                               // few workgroups: slices of four channels
        sp = 1;
    }
    const int n_sets = is_static ? 1 : (t - 1) / K + 3;
    const int fill = (ENC_LDS_FLOATS / (n_sets * s * sp)) & ~(ENCODE_BLOCK - 1);
    *cps = s;
    *split = sp;
    *tile = t;
    *slab = fill < ENC_MAX_SLAB ? fill : ENC_MAX_SLAB;
}

template <int CPS, bool STATIC, int SPLIT>
static void ambi_launch_encode(dim3 grid, hipStream_t st, const float *x, long xs_g, long xs_s, const float *e, long es_g,
                               long es_k, int n_src, int C, int T, int K, int tile, int slab, int n_slices, const float *base,
                               long bs_g, long bs_c, float *y, long ys_g, long ys_c) {
    hipLaunchKernelGGL((bas_ambi_encode_kernel<CPS, STATIC, SPLIT>), grid, dim3(ENC_THREADS), 0, st, x, xs_g, xs_s, e, es_g, es_k,
                       n_src, C, T, K, tile, slab, n_slices, base, bs_g, bs_c, y, ys_g, ys_c);
}

extern "C" int bas_ambi_encode_f32(const float *x, long xs_g, long xs_s, const float *e, long es_g, long es_k, int n_src,
                                   int C, int n_groups, long T, int K, const float *base, long bs_g, long bs_c, float *y,
                                   long ys_g, long ys_c, bas_stream_t stream) {
    BAS_REQUIRE(C >= 1 && C <= AMBI_MAX_C, BAS_E_SHAPE, "bas_ambi_encode_f32: C (%d) must be in 1..%d", C, AMBI_MAX_C);
    BAS_REQUIRE(n_src >= 1 && n_src <= ENC_MAX_SRC, BAS_E_SHAPE, "bas_ambi_encode_f32: n_src (%d) must be in 1..%d", n_src,
                ENC_MAX_SRC);
    BAS_REQUIRE(n_groups >= 0 && n_groups <= 65535 && T >= 0 && K > 0, BAS_E_SHAPE,
                "bas_ambi_encode_f32: need 0 <= n_groups <= 65535, T >= 0 and K > 0");
    BAS_REQUIRE(T < (1L << 30), BAS_E_SHAPE, "bas_ambi_encode_f32: T (%ld) must be below 2^30", T);
    BAS_REQUIRE(bas_none_negative({xs_g, xs_s, es_g, es_k, bs_g, bs_c, ys_g, ys_c}), BAS_E_SHAPE,
                "bas_ambi_encode_f32: strides must be >= 0");
    BAS_REQUIRE(bas_all_below(1L << 40, {xs_g, xs_s, es_g, es_k, bs_g, bs_c, ys_g, ys_c}), BAS_E_SHAPE,
                "bas_ambi_encode_f32: strides must be below 2^40");
    BAS_REQUIRE(es_k == 0 || es_k >= (long)n_src * C, BAS_E_SHAPE,
                "bas_ambi_encode_f32: es_k must be 0 (static) or >= n_src C (the banks of two boundaries overlap)");
    if (n_groups == 0 || T == 0) return 0;
    BAS_REQUIRE(bas_layout_one_to_one(n_groups, C, T, ys_g, ys_c), BAS_E_SHAPE,
                "bas_ambi_encode_f32: the output's strides address an element twice");
    BAS_REQUIRE(x && e && y, BAS_E_NULL, "bas_ambi_encode_f32: null pointer");
    BAS_REQUIRE(bas_aligned(x, 4) && bas_aligned(e, 4) && bas_aligned(base, 4) && bas_aligned(y, 4), BAS_E_ALIGN,
                "bas_ambi_encode_f32: x, e, base, y must be 4-byte aligned");
    const long x_ext[3] = {n_groups, n_src, T}, x_str[3] = {xs_g, xs_s, 1};
    const long y_ext[3] = {n_groups, C, T}, y_str[3] = {ys_g, ys_c, 1};
    const size_t y_bytes = 4 * (size_t)bas_view_extent(3, y_ext, y_str);
    BAS_REQUIRE(!bas_ranges_meet(x, 4 * (size_t)bas_view_extent(3, x_ext, x_str), y, y_bytes), BAS_E_SHAPE,
                "bas_ambi_encode_f32: signals and output overlap");
    const long n_k = es_k == 0 ? 1 : (T - 1) / K + 2;
    BAS_REQUIRE(es_k <= (1L << 62) / n_k, BAS_E_SHAPE,
                "bas_ambi_encode_f32: the banks of the %ld boundaries at es_k = %ld span more than 2^62 elements", n_k, es_k);
    const long e_ext[3] = {n_groups, n_k, (long)n_src * C}, e_str[3] = {es_g, es_k, 1};
    BAS_REQUIRE(!bas_ranges_meet(e, 4 * (size_t)bas_view_extent(3, e_ext, e_str), y, y_bytes), BAS_E_SHAPE,
                "bas_ambi_encode_f32: banks and output overlap");
    if (base && !(base == y && bs_g == ys_g && bs_c == ys_c)) {              // (base == y with y's strides: in place)
        const long b_str[3] = {bs_g, bs_c, 1};
        BAS_REQUIRE(!bas_ranges_meet(base, 4 * (size_t)bas_view_extent(3, y_ext, b_str), y, y_bytes), BAS_E_SHAPE,
                    "bas_ambi_encode_f32: base and output overlap (in place takes base == y with the same strides)");
    }
    const bool is_static = es_k == 0;
    int cps, split, tile, slab;
    ambi_encode_rule(C, T, K, n_groups, is_static, &cps, &split, &tile, &slab);
    const int n_slices = (C + cps * split - 1) / (cps * split);             // slices of the grid: a workgroup's channels
    const long n_work = ((T + tile - 1) / tile) * n_slices;
    const dim3 grid((unsigned)(n_work < (1L << 20) ? n_work : (1L << 20)), (unsigned)n_groups);
    const hipStream_t st = bas_stream(stream);
#define ENC_ARGS grid, st, x, xs_g, xs_s, e, es_g, es_k, n_src, C, (int)T, K, tile, slab, n_slices, base, bs_g, bs_c, y, ys_g, ys_c
    if (is_static) {
        switch (cps) {
        case 4: ambi_launch_encode<4, true, 1>(ENC_ARGS); break;
        case 8: ambi_launch_encode<8, true, 1>(ENC_ARGS); break;
        case 12: ambi_launch_encode<12, true, 1>(ENC_ARGS); break;
        default: ambi_launch_encode<16, true, 1>(ENC_ARGS); break;
        }
    } else {
        if (split == 2) ambi_launch_encode<8, false, 2>(ENC_ARGS);
        else if (cps == 4) ambi_launch_encode<4, false, 1>(ENC_ARGS);
        else ambi_launch_encode<8, false, 1>(ENC_ARGS);
    }
#undef ENC_ARGS
    return bas_check_launch("bas_ambi_encode_f32");
}
