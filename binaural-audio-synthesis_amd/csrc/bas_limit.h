// The look-ahead limiter's sizes, and the stages that its two kernels share (bas_limit.hip: include/bas.h "look-ahead
// limiter"; bas_limit_tp.hip: include/bas_limit_tp.h): the sample fetch, the sliding
// minimum, the fixed-order sums, the epilogue with its meters, the carry of the ring, and the argument checks.
#pragma once
#include "bas_internal.h"
#include "bas_views.h"

#define LIM_THREADS 256
#define LIM_TILE 1024                              // output samples per workgroup (limiter.TILE)
#define LIM_PER_THREAD (LIM_TILE / LIM_THREADS)    // outputs a thread sums side by side
#define LIM_MAX_A BAS_LIMIT_MAX_LOOKAHEAD
#define LIM_MAX_HD BAS_LIMIT_MAX_HOLD
#define LIM_STATE_HEAD 4                           // floats in front of a session's ring: two positions, two spare

// context in front of an output: 2 A + Hd samples
static inline int lim_history(int A, int Hd) { return 2 * A + Hd; }
// floats of one of the kernel's two LDS arrays: history + tile, rounded up to whole quads
static inline int lim_span(int A, int Hd) { return (lim_history(A, Hd) + LIM_TILE + 3) & ~3; }
// dynamic LDS of the kernel: the two arrays (8 KiB .. 56 KiB: 56 KiB at A = 1024, Hd = 4096, so two workgroups share a
// CU's 160 KiB at the largest setting and eight at 5 ms / 20 ms)
static inline size_t lim_lds_bytes(int A, int Hd) { return 2 * (size_t)lim_span(A, Hd) * sizeof(float); }

static inline bool lim_params_ok(int A, int Hd) { return A >= 0 && A <= LIM_MAX_A && Hd >= 0 && Hd <= LIM_MAX_HD; }

// Every argument check of a limiter entry point `who` whose sessions carry `ring` samples per ear (the state's size is what
// `state_floats` returns), in the order bas.h gives.  Returns the error's code, or 0 with *c_out the ceiling as binary32 and
// *nothing set where there is nothing to do.
static inline int lim_check(const char *who, const float *y, long y_stride_g, long y_stride_t, long y_stride_e,
                            const float *out, long out_stride_g, long out_stride_t, long out_stride_e, int n_sessions,
                            long T_in, long T_out, double ceiling, int lookahead, int hold, const float *state,
                            long state_stride, const float *reduction, const float *peak, int ring, const char *state_floats,
                            float *c_out, bool *nothing) {
    *nothing = true;
    BAS_REQUIRE(lookahead >= 0 && lookahead <= LIM_MAX_A, BAS_E_SHAPE, "%s: lookahead (%d) must be in 0..%d", who,
                lookahead, LIM_MAX_A);
    BAS_REQUIRE(hold >= 0 && hold <= LIM_MAX_HD, BAS_E_SHAPE, "%s: hold (%d) must be in 0..%d", who, hold, LIM_MAX_HD);
    const float c = (float)ceiling;
    BAS_REQUIRE(ceiling > 0.0 && (double)c == ceiling && c >= 1.17549435e-38f && c <= 3.40282347e+38f, BAS_E_SHAPE,
                "%s: ceiling (%g) must be a normal binary32 value > 0", who, ceiling);
    BAS_REQUIRE(n_sessions >= 0 && n_sessions <= 65535, BAS_E_SHAPE, "%s: n_sessions (%d) must be in 0..65535", who,
                n_sessions);
    BAS_REQUIRE(T_in >= 0 && T_in < (1L << 30) && T_out >= 0 && T_out < (1L << 30), BAS_E_SHAPE,
                "%s: T_in and T_out must be in 0..2^30 - 1", who);
    BAS_REQUIRE(T_in == T_out || (state && T_in == 0), BAS_E_SHAPE,
                "%s: T_in (%ld) must equal T_out (%ld), or be 0 with a state (the stream's end)", who, T_in, T_out);
    BAS_REQUIRE(bas_none_negative({y_stride_g, y_stride_t, y_stride_e, out_stride_g, out_stride_t, out_stride_e,
                                   state_stride}),
                BAS_E_SHAPE, "%s: strides must be >= 0", who);
    BAS_REQUIRE(bas_all_below(1L << 40, {y_stride_g, y_stride_e, out_stride_g, out_stride_e, state_stride}) &&
                    bas_all_below(1L << 31, {y_stride_t, out_stride_t}),
                BAS_E_SHAPE, "%s: strides must be below 2^40 (session, ear) and 2^31 (sample)", who);
    BAS_REQUIRE(!state || (state_stride >= LIM_STATE_HEAD + 2L * ring && (state_stride & 3) == 0), BAS_E_SHAPE,
                "%s: state_stride (%ld) must be a multiple of 4 and >= %s (%ld)", who, state_stride, state_floats,
                LIM_STATE_HEAD + 2L * ring);
    *c_out = c;
    if (n_sessions == 0 || T_out == 0) return 0;
    BAS_REQUIRE(out && (y || T_in == 0), BAS_E_NULL, "%s: null pointer", who);
    BAS_REQUIRE(bas_aligned(y, 4) && bas_aligned(out, 4) && bas_aligned(reduction, 4) && bas_aligned(peak, 4) &&
                    bas_aligned(state, 16),
                BAS_E_ALIGN, "%s: y, out, reduction, peak must be 4-byte aligned, state 16-byte", who);
    const long in_extent[3] = {n_sessions, T_in, 2}, in_stride[3] = {y_stride_g, y_stride_t, y_stride_e};
    const long out_extent[3] = {n_sessions, T_out, 2}, out_stride[3] = {out_stride_g, out_stride_t, out_stride_e};
    BAS_REQUIRE(bas_layout_nested(3, out_extent, out_stride), BAS_E_SHAPE,
                "%s: the output's strides address an element twice", who);
    const size_t out_bytes = 4 * (size_t)bas_view_extent(3, out_extent, out_stride);
    BAS_REQUIRE(T_in == 0 || !bas_ranges_meet(y, 4 * (size_t)bas_view_extent(3, in_extent, in_stride), out, out_bytes),
                BAS_E_SHAPE, "%s: input and output overlap (the limiter does not run in place)", who);
    const long state_extent[2] = {n_sessions, LIM_STATE_HEAD + 2L * ring}, state_strides[2] = {state_stride, 1};
    BAS_REQUIRE(!bas_ranges_meet(state, 4 * (size_t)bas_view_extent(2, state_extent, state_strides), out, out_bytes),
                BAS_E_SHAPE, "%s: state and output overlap", who);
    *nothing = false;
    return 0;
}

// the required gain for a peak m >= 0: ONE binary32 division (m NaN: r = 1)
__device__ __forceinline__ float lim_required_of(float m, float c) { return m > c ? c / m : 1.0f; }

// The stereo sample at position p of the block (p >= -H): the block itself at 0 .. T_in - 1, the carried ring in front of
// it (slot of position p: (w + p) mod H), zero anywhere else.
__device__ __forceinline__ f32x2 lim_sample(const float *__restrict__ y, long y_t, long y_e, long T_in,
                                            const f32x2 *__restrict__ ring, int H, int w, long p) {
    f32x2 v;
    v.x = v.y = 0.f;
    if (p >= 0) {
        if (p < T_in) {
            v.x = y[p * y_t];
            v.y = y[p * y_t + y_e];
        }
    } else if (ring) {
        int i = w + (int)p + H;
        if (i >= H) i -= H;
        v = ring[i];
    }
    return v;
}

// The ring and its position of session g for a kernel whose ring holds H samples (state null: none, position 0).  With a
// carry launch behind this one (advance == 1) the session's first workgroup leaves the position in the word that launch
// reads: the carry launch reads the position from a word nobody reads here, and writes the new one to the word nobody
// reads there, so no launch reads a word that it writes.
__device__ __forceinline__ const f32x2 *lim_ring(float *state, long state_stride, int g, int H, int advance, int *w) {
    *w = 0;
    if (!state) return nullptr;
    float *sg = state + g * state_stride;
    int pos = reinterpret_cast<const int *>(sg)[0];
    if ((unsigned)pos >= (unsigned)H) pos = 0;                           // (a state that was never zeroed: stay inside the ring)
    if (advance == 1 && blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<int *>(sg)[1] = pos;
    *w = pos;
    return reinterpret_cast<const f32x2 *>(sg + LIM_STATE_HEAD);
}

// The meters of a workgroup of 256 threads (every thread must call it): min of the gains (positive floats: bit order =
// float order) into *gain_bits, max |out| into *peak_bits.  The waves meet in LDS once; one thread of wave 0 and one of
// wave 1 each read the published value and send an atomic only when it would change it (bas_block_peak_max's
// read-before-send; the two round trips run side by side).  Either pointer may be null.
__device__ __forceinline__ void lim_block_meters(float lmin, float lmax, unsigned int *gain_bits, unsigned int *peak_bits) {
    __shared__ float wave_min[4], wave_max[4];
    for (int o = 32; o > 0; o >>= 1) {
        lmin = fminf(lmin, __shfl_xor(lmin, o));
        lmax = bas_peak_max(lmax, __shfl_xor(lmax, o));
    }
    if ((threadIdx.x & 63) == 0) {
        wave_min[(threadIdx.x >> 6) & 3] = lmin;
        wave_max[(threadIdx.x >> 6) & 3] = lmax;
    }
    __syncthreads();
    if (threadIdx.x == 0 && gain_bits) {
        const unsigned int mine = __float_as_uint(fminf(fminf(wave_min[0], wave_min[1]), fminf(wave_min[2], wave_min[3])));
        if (mine < __hip_atomic_load(gain_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(gain_bits, mine);
    }
    if (threadIdx.x == 64 && peak_bits) {
        const unsigned int mine = __float_as_uint(bas_peak_max(bas_peak_max(wave_max[0], wave_max[1]), bas_peak_max(wave_max[2], wave_max[3])));
        if (mine > __hip_atomic_load(peak_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(peak_bits, mine);
    }
}

// The A + 1-term sums of NK outputs per thread (outputs tid + k 256): every chain adds its terms one by one in ascending
// order, in binary64 from +0 - eight terms per chain are read from LDS together, ahead of the adds that take them, so a
// lone workgroup does not wait for LDS once per term.
template <int NK>
__device__ __forceinline__ void lim_sums(const float *E, int tid, int A, double *acc) {
    double a[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k) a[k] = 0.0;
    int i = 0;
    for (; i + 8 <= A + 1; i += 8) {
        float e[NK][8];
#pragma unroll
        for (int k = 0; k < NK; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) e[k][j] = E[tid + k * LIM_THREADS + i + j];
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int k = 0; k < NK; ++k) a[k] += (double)e[k][j];
    }
    for (; i <= A; ++i) {
#pragma unroll
        for (int k = 0; k < NK; ++k) a[k] += (double)E[tid + k * LIM_THREADS + i];
    }
#pragma unroll
    for (int k = 0; k < NK; ++k) acc[k] = a[k];
}

// Steps 2 to 4 of the kernels' comment, for a tile of Tcur outputs: P holds r at its first lenq = (2 A + Hd + Tcur + 3) & ~3
// indices (every thread has passed a barrier behind the writes), Q is the second array; both are 16-byte aligned.  Leaves
// acc[k], the binary64 sum of output tid + k 256.  Every thread must call it.
__device__ __forceinline__ void lim_window_sums(float *P, float *Q, int lenq, int A, int Hd, int Tcur, double *acc) {
    const int tid = threadIdx.x;
    const int W = Hd + A + 1;
    int step = 1;
    const f32x4 ones = {1.0f, 1.0f, 1.0f, 1.0f};
    if (W >= 4) {                                                        // steps 1 and 2 in one pass
        for (int i = 4 * tid; i < lenq; i += 4 * LIM_THREADS) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(P + i);
            const f32x4 b = i + 4 < lenq ? *reinterpret_cast<const f32x4 *>(P + i + 4) : ones;
            f32x4 m;
            m.x = fminf(fminf(a.x, a.y), fminf(a.z, a.w));
            m.y = fminf(fminf(a.y, a.z), fminf(a.w, b.x));
            m.z = fminf(fminf(a.z, a.w), fminf(b.x, b.y));
            m.w = fminf(fminf(a.w, b.x), fminf(b.y, b.z));
            *reinterpret_cast<f32x4 *>(Q + i) = m;
        }
        __syncthreads();
        float *t = P;
        P = Q;
        Q = t;
        step = 4;
    }
    while (2 * step <= W) {
        if (step >= 4) {
            for (int i = 4 * tid; i < lenq; i += 4 * LIM_THREADS) {
                const f32x4 a = *reinterpret_cast<const f32x4 *>(P + i);
                const f32x4 b = i + step < lenq ? *reinterpret_cast<const f32x4 *>(P + i + step) : ones;
                f32x4 m;
                m.x = fminf(a.x, b.x);
                m.y = fminf(a.y, b.y);
                m.z = fminf(a.z, b.z);
                m.w = fminf(a.w, b.w);
                *reinterpret_cast<f32x4 *>(Q + i) = m;
            }
        } else {                                                         // (W < 4: at most one pass, step 1)
            for (int i = tid; i < lenq; i += LIM_THREADS) Q[i] = i + step < lenq ? fminf(P[i], P[i + step]) : P[i];
        }
        __syncthreads();
        float *t = P;
        P = Q;
        Q = t;
        step *= 2;
    }
    const int ne = Tcur + A;                                             // q + W - 1 <= len - 1: no window is cut
    for (int q = tid; q < ne; q += LIM_THREADS) Q[q] = fminf(P[q], P[q + W - step]);
    __syncthreads();
    if (Tcur <= LIM_THREADS) lim_sums<1>(Q, tid, A, acc);                // (every index read: <= LIM_TILE - 1 + A < span)
    else if (Tcur <= 2 * LIM_THREADS) lim_sums<2>(Q, tid, A, acc);
    else lim_sums<LIM_PER_THREAD>(Q, tid, A, acc);
}

// Step 5: output tid + k 256 of the tile is the sample v[k] under g = min(s, req[k]), s its sum over A + 1 rounded once,
// clamped to +-c and written to og + u o_t (+ o_e); then the meters of session g.  Every thread must call it.
__device__ __forceinline__ void lim_epilogue(const f32x2 *v, const float *req, const double *acc, int A, float c, int Tcur,
                                             float *og, long o_t, long o_e, float *reduction, float *peak, int g) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const double terms = (double)(A + 1);
    float lmin = 1.0f, lmax = 0.f;
#pragma unroll
    for (int k = 0; k < LIM_PER_THREAD; ++k) {
        const int u = tid + k * LIM_THREADS;
        if (u < Tcur) {
            const float s = (float)(acc[k] / terms);
            const float gain = fminf(s, req[k]);
            const float l = fminf(fmaxf(v[k].x * gain, -c), c), r = fminf(fmaxf(v[k].y * gain, -c), c);
            og[u * o_t] = l;
            og[u * o_t + o_e] = r;
            lmin = fminf(lmin, gain);
            lmax = bas_peak_max(bas_peak_max(lmax, l), r);
        }
    }
    if (reduction || peak)                                               // (uniform)
        lim_block_meters(lmin, lmax, reduction ? reinterpret_cast<unsigned int *>(reduction) + g : nullptr,
                         peak ? reinterpret_cast<unsigned int *>(peak) + g : nullptr);
}

// The state of one session moves forward: of the block's last cnt = min(T_in, H) samples, number i into its ring slot (slot
// of position j: (w + j) mod H, which held position j - H, no longer needed), and the new position by the thread with
// first set.  w is the position before the block.
__device__ __forceinline__ void lim_carry(const float *__restrict__ yg, long y_t, long y_e, long T_in, int H, int w,
                                          float *sg, long i, bool first) {
    f32x2 *ring = reinterpret_cast<f32x2 *>(sg + LIM_STATE_HEAD);
    const long cnt = T_in < H ? T_in : H;
    if (i < cnt) {
        const long j = T_in - cnt + i;
        f32x2 v;
        v.x = yg[j * y_t];
        v.y = yg[j * y_t + y_e];
        ring[(w + j) % H] = v;
    }
    if (first) reinterpret_cast<int *>(sg)[0] = (int)((w + T_in) % H);
}

// The body of a carry launch (a stream block of more than one tile): one thread per carried sample, as many workgroups as
// they fill; the position is the one the main launch left in the state's second word.
__device__ __forceinline__ void lim_carry_launch(const float *__restrict__ y, long y_g, long y_t, long y_e, long T_in, int H,
                                                 float *state, long state_stride) {
    const int g = blockIdx.y;
    float *sg = state + g * state_stride;
    int w = reinterpret_cast<const int *>(sg)[1];
    if ((unsigned)w >= (unsigned)H) w = 0;
    const long i = (long)blockIdx.x * LIM_THREADS + threadIdx.x;
    lim_carry(y + g * y_g, y_t, y_e, T_in, H, w, sg, i, i == 0);
}
