// What the four output-stationary FIR kernels share (bas_render.hip: bas_render_hd_kernel; bas_fused.hip: bas_render_fz_kernel;
// bas_fused_split.hip: bas_render_fs_kernel; bas_fused_quad.hip: bas_render_fq_kernel), defined once: the walk over
// (tile, source, tap segment) passes, the geometry of a pass's x window, the chunk slot / crossfade weight / live octets of a
// row step, the signal bounds and the clamped fetch of an x window, the address of a read-plan piece, and
// the flush (combine of the pinned accumulators, slab and direct stores).  Every helper takes the few scalars it needs, so
// RenderArgs (stored IRs) and FzArgs (fused) both call them.  The row steps themselves are bas_fir.h and bas_fir_asm.inc.
#pragma once
#include "bas_internal.h"
#include "bas_plan.h"
#include "bas_fir.h"

typedef float f32x32 __attribute__((ext_vector_type(32)));   // (as bas_fir_asm.inc declares it)

#define WIN_PL4 (2 * BAS_PLANS_WORDS / 4)                     // float4 per chunk IR's pair of read plans (18)

// ---- the walk: workgroup b owns the units [unit0, unit0 + units_per_wg) of the n_tiles * n_src (tile, source) units and
// makes one pass per (unit, 128-tap segment)
struct WinWalk {
    long unit0, n_pass;
    int nseg;
};
__device__ __forceinline__ WinWalk win_walk(long units_total, int units_per_wg, int Lp) {
    WinWalk W;
    W.unit0 = (long)blockIdx.x * units_per_wg;
    long unit1 = W.unit0 + units_per_wg;
    if (unit1 > units_total) unit1 = units_total;
    W.nseg = (Lp + RT_SEG - 1) / RT_SEG;
    W.n_pass = (unit1 - W.unit0) * W.nseg;
    return W;
}

// window geometry of a (tile, segment)
struct WinGeo {
    int seg0, Lseg, halo, nrows, c0, mo0;
    long xbase;
};
template <int TILE>
__device__ __forceinline__ WinGeo win_geo(long t, int g, int K, int Lp) {
    WinGeo G;
    G.seg0 = g * RT_SEG;
    G.Lseg = Lp - G.seg0 < RT_SEG ? Lp - G.seg0 : RT_SEG;    // multiple of 8
    G.halo = (G.Lseg + 31) >> 5;                             // input rows above the tile that matter
    G.xbase = t * TILE - G.seg0 - 32L * G.halo;              // first input sample in LDS (multiple of 32)
    G.nrows = TILE / 32 + G.halo;
    long cf = G.xbase / K;                                   // floor division, consistent across 0 (rows before the signal
    if (cf * K > G.xbase) --cf;                              // only meet x = 0, they just need finite IR values)
    G.c0 = (int)cf;
    G.mo0 = (int)(G.xbase - cf * K);
    return G;
}

// The walk's state (tile, source, segment) is advanced by counters, never re-divided
struct WinPos {
    long tile;
    int s, sg;
};
__device__ __forceinline__ WinPos win_next(long tile, int s, int sg, int nseg, int n_src) {
    WinPos N = {tile, s, sg + 1};
    if (N.sg == nseg) {
        N.sg = 0;
        if (++N.s == n_src) {
            N.s = 0;
            ++N.tile;
        }
    }
    return N;
}

// ---- a row step
// chunk slot of the window row at offset pos from the window's first chunk, and the row's offset inside its chunk
// (float estimate, corrected: no integer division)
__device__ __forceinline__ void win_row_slot(int pos, int K, float invK, int &sl, int &m_in) {
    sl = (int)((float)pos * invK);
    m_in = pos - sl * K;
    if (m_in < 0) { m_in += K; sl -= 1; }
    if (m_in >= K) { m_in -= K; sl += 1; }
}

// the next row up: 32 inputs earlier, in the chunk before where it wraps
__device__ __forceinline__ void win_row_up(int K, int &sl, int &m_in) {
    m_in -= 32;
    if (m_in < 0) {
        m_in += K;
        sl -= 1;
    }
}

// crossfade weight of the subchunk that holds offset m of its chunk (apply_hrtf.py:442-443)
__device__ __forceinline__ float win_weight(int m, int S, int s_pow2, float invK, float invS) {
    if (s_pow2) return (float)(m & ~(S - 1)) * invK;
    int q = (int)((float)m * invS);                          // any multiple of 32: m / S by float estimate, corrected
    const int r = m - q * S;
    if (r < 0) q -= 1;
    if (r >= S) q += 1;
    return (float)(q * S) * invK;
}

// octet i of row step rp holds taps t0 = 32 rp - 32 + 8 i .. + 7 of the segment and is live for 0 <= t0 < Lseg (a multiple of 8):
// i in [lo, hi).  (Closed form: eight compare-and-or chains per row step were 60 scalar instructions, which a wave that has
// its SIMD to itself pays ~6 clocks each for.)
__device__ __forceinline__ unsigned win_octet_mask(int rp, int Lseg) {
    const int oct_lo = 4 - 4 * rp > 0 ? 4 - 4 * rp : 0;
    int oct_hi = (Lseg + 32 - 32 * rp) >> 3;                 // >= 1 for rp <= halo
    oct_hi = oct_hi > 8 ? 8 : oct_hi;
    return ((1u << oct_hi) - 1u) & ~((1u << oct_lo) - 1u);
}

// ---- the x window
// offsets, from the window's first sample, of the signal's first sample / one past its last: the signal's ends as two scalar
// bounds on the per-thread window offsets
struct WinXBounds {
    int lo, hi;
};
__device__ __forceinline__ WinXBounds win_x_bounds(long xbase, long T_in) {
    const long lo_l = -xbase, hi_l = T_in - xbase;
    WinXBounds B;
    B.lo = lo_l < -(1 << 30) ? -(1 << 30) : (lo_l > (1 << 30) ? (1 << 30) : (int)lo_l);
    B.hi = hi_l < -(1 << 30) ? -(1 << 30) : (hi_l > (1 << 30) ? (1 << 30) : (int)hi_l);
    return B;
}
// the whole window of NX float4 per thread lies inside the signal
template <int NX, int THREADS>
__device__ __forceinline__ bool win_x_inside(const WinXBounds &B) { return B.lo <= 0 && B.hi >= 4 * NX * THREADS; }

// thread tid's NX float4 of the window, every address clamped into the row (T_in is a multiple of K >= 32).  The window is
// read once: non-temporal, so that L2 keeps the table (same speed, 13 % fewer bytes fetched past L2)
template <int NX, int THREADS>
__device__ __forceinline__ void win_fetch_x(f32x4 (&xv)[NX], const float *xwin, int tid, const WinXBounds &B) {
#pragma unroll
    for (int j = 0; j < NX; ++j) {
        int i = 4 * (tid + j * THREADS);
        i = i < B.lo ? B.lo : i;
        i = i > B.hi - 4 ? B.hi - 4 : i;
        xv[j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(xwin + i));
    }
}

// ---- chunk IRs
// 16-byte piece p = lane + 64 r of the read plans of a wave's n_ev chunk IRs, the first of them chunk c_first (clamped
// into the signal's chunks); pieces past the wave's share re-read piece 0
__device__ __forceinline__ const f32x4 *win_plan_piece(const f32x4 *pl_src, int lane, int r, int n_ev, int c_first, int n_chunks) {
    int p = lane + 64 * r;
    p = p < n_ev * WIN_PL4 ? p : 0;
    const int i = (p * 3641) >> 16;                          // p / 18 for p < 1000
    const int c = clampi(c_first + i, 0, n_chunks);
    return pl_src + (long)c * WIN_PL4 + (p - i * WIN_PL4);
}

// ---- the flush
// the assembly blocks' half-rate partial sums (three 32-float vectors + one pair, pinned to v[0:97]) into a row of 32
// outputs, both ears: y[2p] = A[p] + B[p-1];  y[2p+1] = P[p] - A[p] - B[p]   (ffa_combine of bas_fir.h on the pinned form)
__device__ __forceinline__ void win_combine_pinned(f32x2 (&acc)[32], const f32x32 &accA, const f32x32 &accB, const f32x2 &accB16,
                                                    const f32x32 &accP) {
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const f32x2 a = f32x2{accA[2 * p], accA[2 * p + 1]}, b0 = f32x2{accB[2 * p], accB[2 * p + 1]};
        const f32x2 b1 = p < 15 ? f32x2{accB[2 * p + 2], accB[2 * p + 3]} : accB16;
        const f32x2 pp = f32x2{accP[2 * p], accP[2 * p + 1]};
        acc[2 * p] = a + b0;
        acc[2 * p + 1] = (pp - a) - b1;
    }
}
__device__ __forceinline__ void win_zero_pinned(f32x32 &accA, f32x32 &accB, f32x2 &accB16, f32x32 &accP) {
#pragma unroll
    for (int i = 0; i < 32; ++i) accA[i] = accB[i] = accP[i] = 0.f;
    accB16 = f32x2{0.f, 0.f};
}

// a lane's row of 32 outputs into a slab part: left ear at dst, right ear one tile further.  Plain stores: non-temporal ones
// took WRITE_SIZE from 40 to 135 MB per launch
__device__ __forceinline__ void win_store_row_slab(const f32x2 (&acc)[32], float *dst, int tile_len) {
    f32x4 *l4 = reinterpret_cast<f32x4 *>(dst);
    f32x4 *r4 = reinterpret_cast<f32x4 *>(dst + tile_len);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        l4[i] = f32x4{acc[4 * i].x, acc[4 * i + 1].x, acc[4 * i + 2].x, acc[4 * i + 3].x};
        r4[i] = f32x4{acc[4 * i].y, acc[4 * i + 1].y, acc[4 * i + 2].y, acc[4 * i + 3].y};
    }
}

// Direct output (every tile finished by ONE workgroup): a lane's row of 32 outputs, both ears, into y itself (added to it
// when accumulate).  Plain stores: a lane writes 16 bytes per 128-byte line and instruction, which merge in the L2; as sc1
// stores - what a rescale by another workgroup in a kernel tail would need - they leave it one by one and the kernel doubles
// (DESIGN.md 3.6), so the peak rule stays a launch of its own behind these kernels.  Returns the largest |value| stored.
__device__ __forceinline__ float win_store_row_direct(const f32x2 (&acc)[32], float *__restrict__ y, long T_out, long n0,
                                                      int accumulate) {
    float lmax = 0.f;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        float *ye = y + (long)e * T_out + n0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            f32x4 v = e == 0 ? f32x4{acc[4 * i].x, acc[4 * i + 1].x, acc[4 * i + 2].x, acc[4 * i + 3].x}
                             : f32x4{acc[4 * i].y, acc[4 * i + 1].y, acc[4 * i + 2].y, acc[4 * i + 3].y};
            const long n = n0 + 4 * i;
            if (n + 3 < T_out) {
                f32x4_a4 *p = reinterpret_cast<f32x4_a4 *>(ye + 4 * i);   // (the right ear starts at 4 T_out bytes)
                if (accumulate) v += *p;
                *p = v;
                lmax = bas_peak_max4(lmax, v);
            } else {
                const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (n + j < T_out) {
                        const float r = accumulate ? vv[j] + ye[4 * i + j] : vv[j];
                        ye[4 * i + j] = r;
                        lmax = bas_peak_max(lmax, r);
                    }
                }
            }
        }
    }
    return lmax;
}

// max over the wave as the bits of a non-negative float, wave-uniform (kept in a scalar register across the row steps)
__device__ __forceinline__ unsigned win_wave_max_bits(float lmax) {
    lmax = bas_wave_peak(lmax);
    return (unsigned)__builtin_amdgcn_readfirstlane((int)__float_as_uint(lmax));
}

// the direct store of a flush.  Kernels that end in bas_tail (tail_mode) keep max|y| of what the wave has stored so far in a
// scalar register: the updated maximum is returned; otherwise the row's maximum goes into the peak word by atomicMax
__device__ __forceinline__ unsigned win_flush_row_direct(const f32x2 (&acc)[32], float *y, long T_out, long n0, int accumulate,
                                                          int tail_mode, unsigned int *peak_bits, unsigned wmax_bits) {
    const float lmax = win_store_row_direct(acc, y, T_out, n0, accumulate);
    if (tail_mode) {
        const unsigned b = win_wave_max_bits(lmax);
        wmax_bits = b > wmax_bits ? b : wmax_bits;
    } else if (peak_bits) {
        bas_wave_peak_max(lmax, peak_bits);
    }
    return wmax_bits;
}
