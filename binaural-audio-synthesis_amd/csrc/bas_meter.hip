// BS.1770 loudness and true-peak meter (include/bas.h "loudness meter"):
//   bas_meter_state_doubles   - the carried state of one session
//   bas_meter_workspace_bytes - scratch of a call of more than hop + 1 samples
//   bas_meter_f32             - hop energies of the K-weighted signal and the 4x oversampled peak of a whole signal, or of
//                               one block of a stream
// K-weighting is a recursion, the one stage here that has one.  The unit of work is one (session, ear, hop) - or the part
// of a hop that a block covers - and inside a unit the recursion is cut into 256 runs: every thread filters its run from
// rest, a scan in LDS with the powers of the cascade's 4 x 4 transition matrix turns the 256 end states into the 256 entry
// states, and every thread filters its run again, now squaring and summing.  Across the units of one (session, ear) the
// state is a chain: one launch for every unit's end state from rest, one for the chain, one for the energies - or, for a
// block of at most hop + 1 samples (it touches two hops at the most), ONE launch in which the session's workgroup does its
// one or two units in order.
#include "bas_internal.h"
#include "bas_meter.h"

struct MeterIo {
    const float *y;
    long y_g, y_t, y_e, T;
    double *energy;
    long e_g, e_e, max_hops;
    double *state;
    long state_stride;
    float *peak;                                   // whole signals: [G][2]
    double *ws;
    long n_units;                                  // units per (session, ear) the workspace and the grid provide for
};

// one sample through the cascade (transposed direct form II, binary64); returns the K-weighted sample
__device__ __forceinline__ double met_step(const MeterParams &F, double x, double &s1, double &s2, double &t1, double &t2) {
    const double y1 = F.b[0] * x + s1;
    s1 = F.b[1] * x - F.a[0] * y1 + s2;
    s2 = F.b[2] * x - F.a[1] * y1;
    const double y2 = F.c[0] * y1 + t1;
    t1 = F.c[1] * y1 - F.d[0] * y2 + t2;
    t2 = F.c[2] * y1 - F.d[1] * y2;
    return y2;
}

// The sample at position p of the call: the block at 0 .. T - 1, the carried 11 samples in front of it, zero elsewhere.
__device__ __forceinline__ float met_sample(const float *__restrict__ yg, long y_t, long T, const float *ctx, long p) {
    if (p >= 0) return p < T ? yg[p * y_t] : 0.f;
    return ctx && p >= -MET_CTX ? ctx[MET_CTX + p] : 0.f;
}

// max |.| over n samples and cnt interpolated positions.  xs[i] is the sample at u0 - 11 + i for a unit that starts at
// u0; position mi is time u0 - 6 + mi, its window the samples xs[mi .. mi + 11].  The 12 products of a phase are exact in
// binary64 and are added one by one from +0 with j ascending, then rounded to binary32 once.
__device__ __forceinline__ float met_peak(const float *xs, int n, int cnt, const MeterParams &F) {
    float lmax = 0.f;
    for (int i = threadIdx.x; i < n; i += MET_THREADS) lmax = bas_peak_max(lmax, xs[MET_CTX + i]);
    for (int mi = threadIdx.x; mi < cnt; mi += MET_THREADS) {
        double xv[MET_TAPS];
#pragma unroll
        for (int k = 0; k < MET_TAPS; ++k) xv[k] = (double)xs[mi + k];
#pragma unroll
        for (int p = 0; p < MET_PHASES; ++p) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < MET_TAPS; ++k) s += xv[k] * (double)F.taps[p * MET_TAPS + k];
            lmax = bas_peak_max(lmax, (float)s);
        }
    }
    return lmax;
}

// One unit: the n <= hop samples x[0 .. n - 1] (LDS) through the cascade from the entry state e[4] (uniform).  Every
// thread must call it, n >= 1.  Returns the sum of the squared outputs (want_energy; every thread gets it) and leaves
// the state behind the last sample in e.
//   1. thread t filters its run x[t R .. t R + R - 1] (cut at n) from rest: zs_t;
//   2. X_0 = e, X_{t+1} = zs_t; an inclusive scan Y_t = sum_{j <= t} A^(R (t - j)) X_j by doubling, step i with A^(R 2^i):
//      Y_t is the state in front of run t.  Every run in front of a run that is not empty is a whole one, so only powers of
//      A^R occur;
//   3. the runs again from Y_t, squaring and summing in run order; the 256 sums meet in a fixed tree.
__device__ __forceinline__ double met_unit(const float *x, int n, double *e, const MeterParams &F, bool want_energy) {
    __shared__ double S[2][4][MET_THREADS];
    __shared__ double red[MET_THREADS];
    __shared__ double last[4];
    const int tid = threadIdx.x, R = F.R;
    const int i0 = tid * R;
    const int len = n - i0 < 0 ? 0 : n - i0 < R ? n - i0 : R;
    double s1 = 0.0, s2 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int i = 0; i < len; ++i) (void)met_step(F, (double)x[i0 + i], s1, s2, t1, t2);
    {
        const bool head = tid == MET_THREADS - 1;              // (run 255's own end state enters no other run)
        const int slot = head ? 0 : tid + 1;
        S[0][0][slot] = head ? e[0] : s1;
        S[0][1][slot] = head ? e[1] : s2;
        S[0][2][slot] = head ? e[2] : t1;
        S[0][3][slot] = head ? e[3] : t2;
    }
    __syncthreads();
    int cur = 0;
#pragma unroll 1                                               // (a step's 16 matrix entries at a time in scalar registers)
    for (int i = 0; i < MET_SCAN_STEPS; ++i) {
        const int dist = 1 << i;
        double v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = S[cur][r][tid];
        if (tid >= dist) {
            double u[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) u[c] = S[cur][c][tid - dist];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                v[r] += F.P[i][4 * r] * u[0] + F.P[i][4 * r + 1] * u[1] + F.P[i][4 * r + 2] * u[2] + F.P[i][4 * r + 3] * u[3];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) S[cur ^ 1][r][tid] = v[r];
        __syncthreads();
        cur ^= 1;
    }
    const int t_last = (n - 1) / R;                            // the run that holds the unit's last sample
    double acc = 0.0;
    if (want_energy || tid == t_last) {
        s1 = S[cur][0][tid];
        s2 = S[cur][1][tid];
        t1 = S[cur][2][tid];
        t2 = S[cur][3][tid];
        for (int i = 0; i < len; ++i) {
            const double z = met_step(F, (double)x[i0 + i], s1, s2, t1, t2);
            acc += z * z;
        }
        if (tid == t_last) {
            last[0] = s1;
            last[1] = s2;
            last[2] = t1;
            last[3] = t2;
        }
    }
    red[tid] = acc;
    __syncthreads();
    for (int h = MET_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    const double sum = red[0];
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = last[r];
    __syncthreads();                                           // (the next unit writes these arrays again)
    return sum;
}

__device__ __forceinline__ double *met_ear_state(const MeterIo &io, int g, int ear) {
    return io.state ? io.state + g * io.state_stride + ear * MET_EAR_WORDS : nullptr;
}

__device__ __forceinline__ long long met_count(const double *se, int word) {
    if (!se) return 0;
    const long long c = reinterpret_cast<const long long *>(se)[word];
    return c < 0 ? 0 : c;                                      // (a state that was never zeroed: stay inside the buffers)
}

__device__ __forceinline__ unsigned int *met_peak_word(const MeterIo &io, double *se, int g, int ear) {
    if (se) return reinterpret_cast<unsigned int *>(se + MET_W_PEAK);
    return io.peak ? reinterpret_cast<unsigned int *>(io.peak) + 2 * g + ear : nullptr;
}

// the last 11 samples in front of position `end` of the staged array become the carried ones
__device__ __forceinline__ void met_store_ctx(double *se, const float *xs, int end) {
    if (threadIdx.x < MET_CTX) reinterpret_cast<float *>(se + MET_W_CTX)[threadIdx.x] = xs[end + threadIdx.x];
}

// A block of at most hop + 1 samples (or a whole signal that short, or a stream's end: T == 0), one workgroup per
// (ear, session), ONE launch: the block touches two hops at the most, so the workgroup filters its one or two units in
// order, closes the open hop where the block fills it, and moves the state forward itself behind a barrier that every
// read of the state has passed - nobody else reads or writes this ear's words.
__global__ __launch_bounds__(MET_THREADS) void bas_meter_block_kernel(MeterIo io, MeterParams F) {
    extern __shared__ __attribute__((aligned(16))) float met_xs[];
    const int tid = threadIdx.x, ear = blockIdx.x, g = blockIdx.y;
    const int T = (int)io.T, hop = F.hop;
    double *se = met_ear_state(io, g, ear);
    const long long count = met_count(se, MET_W_COUNT);
    const bool flush = !se || T == 0;                          // the positions whose windows reach past the end
    const float *yg = T > 0 ? io.y + g * io.y_g + ear * io.y_e : nullptr;
    const float *ctx = se ? reinterpret_cast<const float *>(se + MET_W_CTX) : nullptr;
    const int total = MET_CTX + T + (flush ? MET_CTX : 0);
    for (int i = tid; i < total; i += MET_THREADS) met_xs[i] = met_sample(yg, io.y_t, T, ctx, (long)i - MET_CTX);
    double e[4] = {0.0, 0.0, 0.0, 0.0}, open = 0.0;
    if (se) {
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = se[MET_W_FILT + r];
        open = se[MET_W_OPEN];
    }
    __syncthreads();
    const float lmax = met_peak(met_xs, T, T + (flush ? MET_CTX : 0), F);
    int fill = (int)(count % hop), done = 0;
    long long h = count / hop;
    while (done < T) {                                         // (uniform; at most two rounds)
        const int n = hop - fill < T - done ? hop - fill : T - done;
        open += met_unit(met_xs + MET_CTX + done, n, e, F, true);
        fill += n;
        done += n;
        if (fill == hop) {
            if (tid == 0 && h < io.max_hops) io.energy[g * io.e_g + ear * io.e_e + h] = open;
            open = 0.0;
            fill = 0;
            ++h;
        }
    }
    unsigned int *pw = met_peak_word(io, se, g, ear);
    if (pw) bas_block_peak_max(lmax, pw);                      // (uniform)
    if (se && T > 0) {
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) se[MET_W_FILT + r] = e[r];
            se[MET_W_OPEN] = open;
            reinterpret_cast<long long *>(se)[MET_W_COUNT] = count + T;
        }
        met_store_ctx(se, met_xs, T);
    }
}

// A call of more than hop + 1 samples, one workgroup per (unit, ear, session).  With the open hop holding `fill` samples,
// unit 0 is the hop - fill samples that close it and unit k > 0 the hop (or the last part of one) behind it.
//   PHASE 1: unit 0 knows its entry state - the carried one - and does everything: energy, peak, its true end state into
//            the workspace.  Every other unit leaves its end state FROM REST there.
//   (the chain kernel turns these into entry states)
//   PHASE 3: units k > 0 from their entry states: energy and peak; the last one moves the carried state forward.
// Phase 1 reads the state's count, filter, sum and samples and writes the copies of the count and the samples; phase 3
// reads the copies and writes the others: no launch reads a word that it writes.
template <int PHASE>
__global__ __launch_bounds__(MET_THREADS) void bas_meter_unit_kernel(MeterIo io, MeterParams F) {
    extern __shared__ __attribute__((aligned(16))) float met_xs[];
    const int tid = threadIdx.x, k = blockIdx.x, ear = blockIdx.y, g = blockIdx.z;
    const int hop = F.hop;
    if (PHASE == 3 && k == 0) return;
    double *se = met_ear_state(io, g, ear);
    const long long count = met_count(se, PHASE == 1 ? MET_W_COUNT : MET_W_SHADOW);
    const int fill = (int)(count % hop);
    const long u0 = k == 0 ? 0 : (long)(hop - fill) + (long)(k - 1) * hop;
    if (u0 >= io.T) return;                                    // (uniform: the grid provides for fill == hop - 1)
    const int n = k == 0 ? hop - fill : (int)(io.T - u0 < hop ? io.T - u0 : hop);
    const bool is_last = u0 + n == io.T, full = PHASE == 3 || k == 0;
    const bool flush = full && is_last && !se;
    // (a first unit of fewer than 11 samples: the windows of the second reach into the carried samples too)
    const float *ctx = se ? reinterpret_cast<const float *>(se + (PHASE == 1 ? MET_W_CTX : MET_W_CTX_SHADOW)) : nullptr;
    if (PHASE == 1 && k == 0 && se) {
        if (tid == 0) reinterpret_cast<long long *>(se)[MET_W_SHADOW] = count;
        if (tid < MET_CTX) reinterpret_cast<float *>(se + MET_W_CTX_SHADOW)[tid] = ctx[tid];
    }
    const float *yg = io.y + g * io.y_g + ear * io.y_e;
    const int total = MET_CTX + n + (flush ? MET_CTX : 0);
    for (int i = tid; i < total; i += MET_THREADS) met_xs[i] = met_sample(yg, io.y_t, io.T, ctx, u0 - MET_CTX + i);
    double *wsu = io.ws + (((long)g * 2 + ear) * io.n_units + k) * MET_WS_UNIT_WORDS;
    double e[4] = {0.0, 0.0, 0.0, 0.0}, open = 0.0;
    if (PHASE == 3) {
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = wsu[4 + r];
    } else if (k == 0 && se) {
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r] = se[MET_W_FILT + r];
        open = se[MET_W_OPEN];
    }
    __syncthreads();
    const float lmax = full ? met_peak(met_xs, n, n + (flush ? MET_CTX : 0), F) : 0.f;
    open += met_unit(met_xs + MET_CTX, n, e, F, full);
    if (PHASE == 1 && tid == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) wsu[r] = e[r];
    }
    if (!full) return;                                         // (uniform)
    const long long h = count / hop + k;
    const bool closes = (k == 0 ? fill : 0) + n == hop;
    if (closes && tid == 0 && h < io.max_hops) io.energy[g * io.e_g + ear * io.e_e + h] = open;
    unsigned int *pw = met_peak_word(io, se, g, ear);
    if (pw) bas_block_peak_max(lmax, pw);                      // (uniform)
    if (PHASE == 3 && is_last && se) {
        if (tid == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) se[MET_W_FILT + r] = e[r];
            se[MET_W_OPEN] = closes ? 0.0 : open;
            reinterpret_cast<long long *>(se)[MET_W_COUNT] = count + io.T;
        }
        met_store_ctx(se, met_xs, n);                          // (the 11 samples in front of the unit are staged too)
    }
}

// The chain: one thread per (session, ear).  Unit 0 left its true end state; s_{k+1} = A^hop s_k + zs_k over the whole
// hops behind it.  Eight units' end states are read together, ahead of the products that take them.
__global__ __launch_bounds__(64) void bas_meter_chain_kernel(MeterIo io, MeterParams F, int n_pairs) {
    const int pair = blockIdx.x * 64 + threadIdx.x;
    if (pair >= n_pairs) return;
    const int g = pair >> 1, ear = pair & 1, hop = F.hop;
    const long long count = met_count(met_ear_state(io, g, ear), MET_W_SHADOW);
    const int fill = (int)(count % hop);
    const long rest = io.T - (hop - fill);
    const long units = 1 + (rest + hop - 1) / hop;
    double *w = io.ws + (long)pair * io.n_units * MET_WS_UNIT_WORDS;
    double s[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) s[r] = w[r];
    for (long k0 = 1; k0 < units; k0 += 8) {
        double zs[8][4];
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) zs[b][r] = k0 + b < units ? w[(k0 + b) * MET_WS_UNIT_WORDS + r] : 0.0;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const long k = k0 + b;
            if (k < units) {
                double *wk = w + k * MET_WS_UNIT_WORDS;
                double t[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    wk[4 + r] = s[r];
                    t[r] = zs[b][r] + (F.Ahop[4 * r] * s[0] + F.Ahop[4 * r + 1] * s[1] + F.Ahop[4 * r + 2] * s[2] +
                                       F.Ahop[4 * r + 3] * s[3]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] = t[r];       // (behind the last unit: not used)
            }
        }
    }
}

extern "C" size_t bas_meter_state_doubles(void) { return MET_STATE_WORDS; }

extern "C" size_t bas_meter_workspace_bytes(int n_sessions, long T_in, int hop) {
    if (n_sessions <= 0 || n_sessions > 65535 || hop < MET_FS_MIN / 10 || hop > MET_FS_MAX / 10 || T_in <= (long)hop + 1 ||
        T_in >= (1L << 30))
        return 0;
    return (size_t)n_sessions * 2 * (size_t)meter_max_units(T_in, hop) * MET_WS_UNIT_WORDS * sizeof(double);
}

extern "C" int bas_meter_f32(const float *y, long y_stride_g, long y_stride_t, long y_stride_e, int n_sessions, long T_in,
                             int fs, int hop, const float *taps, double *energy, long e_stride_g, long e_stride_e,
                             long max_hops, long n_before, double *state, long state_stride, float *true_peak, void *ws,
                             size_t ws_bytes, bas_stream_t stream) {
    BAS_REQUIRE(meter_fs_ok(fs), BAS_E_SHAPE, "bas_meter_f32: fs (%d) must be a multiple of 10 in %d..%d", fs, MET_FS_MIN,
                MET_FS_MAX);
    BAS_REQUIRE(hop == fs / 10, BAS_E_SHAPE, "bas_meter_f32: hop (%d) must be fs / 10 (%d)", hop, fs / 10);
    BAS_REQUIRE(n_sessions >= 0 && n_sessions <= 65535, BAS_E_SHAPE, "bas_meter_f32: n_sessions (%d) must be in 0..65535",
                n_sessions);
    BAS_REQUIRE(T_in >= 0 && T_in < (1L << 30), BAS_E_SHAPE, "bas_meter_f32: T_in (%ld) must be in 0..2^30 - 1", T_in);
    BAS_REQUIRE(max_hops >= 0 && max_hops < (1L << 31), BAS_E_SHAPE, "bas_meter_f32: max_hops (%ld) must be in 0..2^31 - 1",
                max_hops);
    BAS_REQUIRE(bas_none_negative({y_stride_g, y_stride_t, y_stride_e, e_stride_g, e_stride_e, state_stride}), BAS_E_SHAPE,
                "bas_meter_f32: strides must be >= 0");
    BAS_REQUIRE(bas_all_below(1L << 40, {y_stride_g, y_stride_e, e_stride_g, e_stride_e, state_stride}) &&
                    y_stride_t < (1L << 31),
                BAS_E_SHAPE, "bas_meter_f32: strides must be below 2^40 (session, ear) and 2^31 (sample)");
    BAS_REQUIRE(!state || (state_stride >= MET_STATE_WORDS && (state_stride & 1) == 0), BAS_E_SHAPE,
                "bas_meter_f32: state_stride (%ld) must be even and >= bas_meter_state_doubles (%d)", state_stride,
                MET_STATE_WORDS);
    BAS_REQUIRE(n_before >= 0 && n_before < (1L << 62) && (state || n_before == 0), BAS_E_SHAPE,
                "bas_meter_f32: n_before (%ld) must be >= 0, and 0 for a whole signal", n_before);
    BAS_REQUIRE(!(state && true_peak), BAS_E_SHAPE,
                "bas_meter_f32: a stream's true peak lives in its state; true_peak belongs to a whole signal");
    BAS_REQUIRE((n_before + T_in) / hop <= max_hops, BAS_E_SHAPE,
                "bas_meter_f32: the energy buffer is full: %ld hops after this block, max_hops %ld", (n_before + T_in) / hop,
                max_hops);
    if (n_sessions == 0 || (T_in == 0 && !state)) return 0;
    BAS_REQUIRE(taps && (y || T_in == 0) && (energy || max_hops == 0), BAS_E_NULL, "bas_meter_f32: null pointer");
    BAS_REQUIRE(max_hops == 0 || bas_layout_one_to_one(n_sessions, 2, max_hops, e_stride_g, e_stride_e), BAS_E_SHAPE,
                "bas_meter_f32: the energy buffer's strides address an element twice");
    const bool chained = T_in > (long)hop + 1;
    const long n_units = chained ? meter_max_units(T_in, hop) : 0;
    const size_t ws_need = chained ? (size_t)n_sessions * 2 * (size_t)n_units * MET_WS_UNIT_WORDS * sizeof(double) : 0;
    BAS_REQUIRE(!chained || ws, BAS_E_NULL, "bas_meter_f32: null workspace for a call of more than hop + 1 samples");
    BAS_REQUIRE(ws_bytes >= ws_need, BAS_E_SHAPE, "bas_meter_f32: workspace of %zu bytes, bas_meter_workspace_bytes is %zu",
                ws_bytes, ws_need);
    BAS_REQUIRE(bas_aligned(y, 4) && bas_aligned(true_peak, 4) && bas_aligned(energy, 8) && bas_aligned(state, 16) &&
                    (!chained || bas_aligned(ws, 16)),
                BAS_E_ALIGN, "bas_meter_f32: y, true_peak must be 4-byte aligned, energy 8-byte, state and ws 16-byte");
    {
        const long y_ext[3] = {n_sessions, T_in, 2}, y_str[3] = {y_stride_g, y_stride_t, y_stride_e};
        const long e_ext[3] = {n_sessions, 2, max_hops}, e_str[3] = {e_stride_g, e_stride_e, 1};
        const long s_ext[2] = {n_sessions, MET_STATE_WORDS}, s_str[2] = {state_stride, 1};
        const size_t y_n = T_in > 0 ? 4 * (size_t)bas_view_extent(3, y_ext, y_str) : 0;
        const size_t e_n = max_hops > 0 ? 8 * (size_t)bas_view_extent(3, e_ext, e_str) : 0;
        const size_t s_n = state ? 8 * (size_t)bas_view_extent(2, s_ext, s_str) : 0;
        const size_t p_n = true_peak ? 8 * (size_t)n_sessions : 0;
        const void *buf[5] = {y, energy, state, true_peak, chained ? ws : nullptr};
        const size_t len[5] = {y_n, e_n, s_n, p_n, ws_need};
        for (int i = 0; i < 5; ++i)
            for (int j = i + 1; j < 5; ++j)
                BAS_REQUIRE(!bas_ranges_meet(buf[i], len[i], buf[j], len[j]), BAS_E_SHAPE,
                            "bas_meter_f32: input, energy buffer, state, true_peak and workspace overlap");
    }
    MeterParams F;
    meter_params(fs, taps, &F);
    const MeterIo io = {y, y_stride_g, y_stride_t, y_stride_e, T_in, energy, e_stride_g, e_stride_e, max_hops,
                        state, state_stride, true_peak, static_cast<double *>(ws), n_units};
    const hipStream_t st = bas_stream(stream);
    const size_t lds = meter_lds_bytes(hop);                   // with the static arrays: 22 KiB at 48 kHz, 96 KiB at 192 kHz
    if (!chained) {
        if (lds > 40 * 1024) {
            const hipError_t e = bas_allow_full_lds(reinterpret_cast<const void *>(bas_meter_block_kernel));
            if (e != hipSuccess) return bas_fail((int)e, "bas_meter_f32: hipFuncSetAttribute: %s", hipGetErrorString(e));
        }
        hipLaunchKernelGGL(bas_meter_block_kernel, dim3(2, (unsigned)n_sessions), dim3(MET_THREADS), lds, st, io, F);
        return bas_check_launch("bas_meter_f32");
    }
    if (lds > 40 * 1024) {
        hipError_t e = bas_allow_full_lds(reinterpret_cast<const void *>(bas_meter_unit_kernel<1>));
        if (e == hipSuccess) e = bas_allow_full_lds(reinterpret_cast<const void *>(bas_meter_unit_kernel<3>));
        if (e != hipSuccess) return bas_fail((int)e, "bas_meter_f32: hipFuncSetAttribute: %s", hipGetErrorString(e));
    }
    const dim3 grid((unsigned)n_units, 2, (unsigned)n_sessions);
    hipLaunchKernelGGL(bas_meter_unit_kernel<1>, grid, dim3(MET_THREADS), lds, st, io, F);
    hipLaunchKernelGGL(bas_meter_chain_kernel, dim3((unsigned)((2 * n_sessions + 63) / 64)), dim3(64), 0, st, io, F,
                       2 * n_sessions);
    hipLaunchKernelGGL(bas_meter_unit_kernel<3>, grid, dim3(MET_THREADS), lds, st, io, F);
    return bas_check_launch("bas_meter_f32");
}
