// Look-ahead peak limiter, one gain for both ears (include/bas.h "look-ahead limiter"):
//   bas_limit_f32          - a whole signal, or one block of a stream with its carried history in front
//   bas_limit_state_floats - the carried state of one session
// No recursion: output j of a block is a function of the inputs j - (2 A + Hd) .. j, so a stream block that finds those
// samples in its history gives the whole signal's bits.
#include "bas_limit.h"

// the required gain of one stereo sample: ONE binary32 division
__device__ __forceinline__ float lim_required(f32x2 v, float c) {
    const float m = bas_peak_max(bas_peak_max(0.f, v.x), v.y);      // (a NaN in either ear: m NaN, r = 1, as np.abs(y).max(-1))
    return m > c ? c / m : 1.0f;
}

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

// One workgroup per (tile of LIM_TILE outputs, session).  Output u of the tile sits at block position j = j0 + u and is
// the limited sample of position j - A.  In LDS, index i is position j0 - H + i:
//   1. r over positions j0 - H .. j0 + Tcur - 1 (eight samples per thread are in flight together);
//   2. minima over 2^k neighbours by doubling between the two arrays (a minimum has no rounding), 2^k <= W = Hd + A + 1:
//      four neighbours in the first pass, then a quad of entries per thread and pass (16-byte LDS accesses; entries past
//      the end read as 1, the largest r there is);
//   3. e[q] = min r over [q, q + W): two overlapping power-of-two windows; q = 0 .. Tcur + A - 1;
//   4. s[u] = (e[u] + e[u + 1] + ... + e[u + A]) / (A + 1): sequential binary64 adds from +0, one binary64 division, one
//      rounding; a thread carries one chain per 256 outputs of the tile side by side;
//   5. g = min(s, r), out = clamp(y g), the meters;
//   6. (advance == 2: the session's only workgroup) the state moves forward here, behind a barrier that every read of the
//      ring has passed; with more tiles per session (advance == 1) a second launch does it.
__global__ __launch_bounds__(LIM_THREADS) void bas_limit_kernel(const float *__restrict__ y, long y_g, long y_t, long y_e,
                                                                long T_in, float *__restrict__ out, long o_g, long o_t,
                                                                long o_e, long T_out, int lead, float c, int A, int Hd,
                                                                float *state, long state_stride, int advance,
                                                                float *reduction, float *peak) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lim_lds[];
    const int tid = threadIdx.x, g = blockIdx.y;
    const int H = 2 * A + Hd, span = (H + LIM_TILE + 3) & ~3;            // (lim_span)
    float *P = lim_lds, *Q = lim_lds + span;
    const long o0 = (long)blockIdx.x * LIM_TILE;
    const int Tcur = (int)(T_out - o0 < LIM_TILE ? T_out - o0 : LIM_TILE);
    const long j0 = o0 + lead;
    const float *yg = T_in > 0 ? y + g * y_g : nullptr;
    const f32x2 *ring = nullptr;
    int w = 0;
    if (state) {
        float *sg = state + g * state_stride;
        w = reinterpret_cast<const int *>(sg)[0];
        if ((unsigned)w >= (unsigned)H) w = 0;                           // (a state that was never zeroed: stay inside the ring)
        ring = reinterpret_cast<const f32x2 *>(sg + LIM_STATE_HEAD);
        // the carry launch behind this one reads the position from a word nobody reads here, and writes the new one to
        // the word nobody reads there: no launch reads a word that it writes
        if (advance == 1 && blockIdx.x == 0 && tid == 0) reinterpret_cast<int *>(sg)[1] = w;
    }
    const int len = H + Tcur, lenq = (len + 3) & ~3;
    for (int i0 = tid; i0 < lenq; i0 += 8 * LIM_THREADS) {
        f32x2 v[8];
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int i = i0 + b * LIM_THREADS;
            v[b].x = v[b].y = 0.f;
            if (i < len) v[b] = lim_sample(yg, y_t, y_e, T_in, ring, H, w, j0 - H + i);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int i = i0 + b * LIM_THREADS;
            if (i < lenq) P[i] = lim_required(v[b], c);                  // (zeros past len: r = 1)
        }
    }
    __syncthreads();
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
    double acc[LIM_PER_THREAD];                                          // (every index read: <= LIM_TILE - 1 + A < span)
    if (Tcur <= LIM_THREADS) lim_sums<1>(Q, tid, A, acc);
    else if (Tcur <= 2 * LIM_THREADS) lim_sums<2>(Q, tid, A, acc);
    else lim_sums<LIM_PER_THREAD>(Q, tid, A, acc);
    const double terms = (double)(A + 1);
    float lmin = 1.0f, lmax = 0.f;
    float *og = out + g * o_g;
    f32x2 v[LIM_PER_THREAD];
#pragma unroll
    for (int k = 0; k < LIM_PER_THREAD; ++k) {
        const int u = tid + k * LIM_THREADS;
        v[k].x = v[k].y = 0.f;
        if (u < Tcur) v[k] = lim_sample(yg, y_t, y_e, T_in, ring, H, w, j0 + u - A);
    }
#pragma unroll
    for (int k = 0; k < LIM_PER_THREAD; ++k) {
        const int u = tid + k * LIM_THREADS;
        if (u < Tcur) {
            const float s = (float)(acc[k] / terms);
            const float gain = fminf(s, lim_required(v[k], c));
            const float l = fminf(fmaxf(v[k].x * gain, -c), c), r = fminf(fmaxf(v[k].y * gain, -c), c);
            og[(o0 + u) * o_t] = l;
            og[(o0 + u) * o_t + o_e] = r;
            lmin = fminf(lmin, gain);
            lmax = bas_peak_max(bas_peak_max(lmax, l), r);
        }
    }
    if (reduction || peak)                                               // (uniform)
        lim_block_meters(lmin, lmax, reduction ? reinterpret_cast<unsigned int *>(reduction) + g : nullptr,
                         peak ? reinterpret_cast<unsigned int *>(peak) + g : nullptr);
    if (advance == 2) {                                                  // (uniform; this workgroup alone reads this state)
        __syncthreads();                                                 // every value read from the ring has been used
        float *sg = state + g * state_stride;
        f32x2 *slots = reinterpret_cast<f32x2 *>(sg + LIM_STATE_HEAD);
        const int cnt = (int)(T_in < H ? T_in : H);
        for (int i = tid; i < cnt; i += LIM_THREADS) {
            const long j = T_in - cnt + i;
            f32x2 s;
            s.x = yg[j * y_t];
            s.y = yg[j * y_t + y_e];
            slots[(w + j) % H] = s;
        }
        if (tid == 0) reinterpret_cast<int *>(sg)[0] = (int)((w + T_in) % H);
    }
}

// The state moves forward: the block's last min(T_in, H) samples into their ring slots (slot of position j: (w + j) mod H,
// which held position j - H, no longer needed), spread over as many workgroups as they fill; then the new position.
__global__ __launch_bounds__(LIM_THREADS) void bas_limit_carry_kernel(const float *__restrict__ y, long y_g, long y_t,
                                                                      long y_e, long T_in, int H, float *state,
                                                                      long state_stride) {
    const int g = blockIdx.y;
    float *sg = state + g * state_stride;
    int w = reinterpret_cast<const int *>(sg)[1];
    if ((unsigned)w >= (unsigned)H) w = 0;
    f32x2 *ring = reinterpret_cast<f32x2 *>(sg + LIM_STATE_HEAD);
    const float *yg = y + g * y_g;
    const long cnt = T_in < H ? T_in : H;
    const long i = (long)blockIdx.x * LIM_THREADS + threadIdx.x;
    if (i < cnt) {
        const long j = T_in - cnt + i;
        f32x2 v;
        v.x = yg[j * y_t];
        v.y = yg[j * y_t + y_e];
        ring[(w + j) % H] = v;
    }
    if (i == 0) reinterpret_cast<int *>(sg)[0] = (int)((w + T_in) % H);
}

static inline bool lim_params_ok(int A, int Hd) { return A >= 0 && A <= LIM_MAX_A && Hd >= 0 && Hd <= LIM_MAX_HD; }

extern "C" size_t bas_limit_state_floats(int lookahead, int hold) {
    if (!lim_params_ok(lookahead, hold)) return 0;
    return (size_t)LIM_STATE_HEAD + 2 * (size_t)lim_history(lookahead, hold);
}

extern "C" int bas_limit_f32(const float *y, long y_stride_g, long y_stride_t, long y_stride_e, float *out,
                             long out_stride_g, long out_stride_t, long out_stride_e, int n_sessions, long T_in, long T_out,
                             double ceiling, int lookahead, int hold, float *state, long state_stride, float *reduction,
                             float *peak, bas_stream_t stream) {
    BAS_REQUIRE(lookahead >= 0 && lookahead <= LIM_MAX_A, BAS_E_SHAPE, "bas_limit_f32: lookahead (%d) must be in 0..%d",
                lookahead, LIM_MAX_A);
    BAS_REQUIRE(hold >= 0 && hold <= LIM_MAX_HD, BAS_E_SHAPE, "bas_limit_f32: hold (%d) must be in 0..%d", hold, LIM_MAX_HD);
    const float c = (float)ceiling;
    BAS_REQUIRE(ceiling > 0.0 && (double)c == ceiling && c >= 1.17549435e-38f && c <= 3.40282347e+38f, BAS_E_SHAPE,
                "bas_limit_f32: ceiling (%g) must be a normal binary32 value > 0", ceiling);
    BAS_REQUIRE(n_sessions >= 0 && n_sessions <= 65535, BAS_E_SHAPE, "bas_limit_f32: n_sessions (%d) must be in 0..65535",
                n_sessions);
    BAS_REQUIRE(T_in >= 0 && T_in < (1L << 30) && T_out >= 0 && T_out < (1L << 30), BAS_E_SHAPE,
                "bas_limit_f32: T_in and T_out must be in 0..2^30 - 1");
    BAS_REQUIRE(T_in == T_out || (state && T_in == 0), BAS_E_SHAPE,
                "bas_limit_f32: T_in (%ld) must equal T_out (%ld), or be 0 with a state (the stream's end)", T_in, T_out);
    BAS_REQUIRE(bas_none_negative({y_stride_g, y_stride_t, y_stride_e, out_stride_g, out_stride_t, out_stride_e,
                                   state_stride}),
                BAS_E_SHAPE, "bas_limit_f32: strides must be >= 0");
    BAS_REQUIRE(bas_all_below(1L << 40, {y_stride_g, y_stride_e, out_stride_g, out_stride_e, state_stride}) &&
                    bas_all_below(1L << 31, {y_stride_t, out_stride_t}),
                BAS_E_SHAPE, "bas_limit_f32: strides must be below 2^40 (session, ear) and 2^31 (sample)");
    const int H = lim_history(lookahead, hold);
    BAS_REQUIRE(!state || (state_stride >= LIM_STATE_HEAD + 2L * H && (state_stride & 3) == 0), BAS_E_SHAPE,
                "bas_limit_f32: state_stride (%ld) must be a multiple of 4 and >= bas_limit_state_floats (%ld)",
                state_stride, LIM_STATE_HEAD + 2L * H);
    if (n_sessions == 0 || T_out == 0) return 0;
    BAS_REQUIRE(out && (y || T_in == 0), BAS_E_NULL, "bas_limit_f32: null pointer");
    BAS_REQUIRE(bas_aligned(y, 4) && bas_aligned(out, 4) && bas_aligned(reduction, 4) && bas_aligned(peak, 4) &&
                    bas_aligned(state, 16),
                BAS_E_ALIGN, "bas_limit_f32: y, out, reduction, peak must be 4-byte aligned, state 16-byte");
    const long in_extent[3] = {n_sessions, T_in, 2}, in_stride[3] = {y_stride_g, y_stride_t, y_stride_e};
    const long out_extent[3] = {n_sessions, T_out, 2}, out_stride[3] = {out_stride_g, out_stride_t, out_stride_e};
    BAS_REQUIRE(bas_layout_nested(3, out_extent, out_stride), BAS_E_SHAPE,
                "bas_limit_f32: the output's strides address an element twice");
    const size_t out_bytes = 4 * (size_t)bas_view_extent(3, out_extent, out_stride);
    BAS_REQUIRE(T_in == 0 || !bas_ranges_meet(y, 4 * (size_t)bas_view_extent(3, in_extent, in_stride), out, out_bytes),
                BAS_E_SHAPE, "bas_limit_f32: input and output overlap (the limiter does not run in place)");
    const long state_extent[2] = {n_sessions, LIM_STATE_HEAD + 2L * H}, state_strides[2] = {state_stride, 1};
    BAS_REQUIRE(!bas_ranges_meet(state, 4 * (size_t)bas_view_extent(2, state_extent, state_strides), out, out_bytes),
                BAS_E_SHAPE, "bas_limit_f32: state and output overlap");
    const hipStream_t st = bas_stream(stream);
    const unsigned tiles = (unsigned)((T_out + LIM_TILE - 1) / LIM_TILE);
    // a block of one tile per session moves its state forward itself; longer blocks leave it to a second launch
    const int advance = !(state && T_in > 0 && H > 0) ? 0 : tiles == 1 ? 2 : 1;
    hipLaunchKernelGGL(bas_limit_kernel, dim3(tiles, (unsigned)n_sessions), dim3(LIM_THREADS), lim_lds_bytes(lookahead, hold),
                       st, y, y_stride_g, y_stride_t, y_stride_e, T_in, out, out_stride_g, out_stride_t, out_stride_e, T_out,
                       state ? 0 : lookahead, c, lookahead, hold, state, state_stride, advance, reduction, peak);
    if (advance == 1) {
        const long cnt = T_in < H ? T_in : H;
        hipLaunchKernelGGL(bas_limit_carry_kernel, dim3((unsigned)((cnt + LIM_THREADS - 1) / LIM_THREADS), (unsigned)n_sessions),
                           dim3(LIM_THREADS), 0, st, y, y_stride_g, y_stride_t, y_stride_e, T_in, H, state, state_stride);
    }
    return bas_check_launch("bas_limit_f32");
}
