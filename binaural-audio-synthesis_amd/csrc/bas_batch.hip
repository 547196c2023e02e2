// Batched independent renders (include/bas.h "batches"): a batch of B items is rendered as ONE longer scene in which
// item b occupies the samples [off_b, off_b + T_in_b) of every source row, followed by a zero gap of G >= L-1 samples
// (G a multiple of K).  The render is causal and its crossfade depends only on the position inside a chunk, so item b's
// own render (apply_hrtf.py:356-459) is exactly the window [off_b, off_b + T_in_b + L - 1) of the long one.
// Two entry points around the unchanged render:
//   bas_batch_pack_f32   - scatter [B][n_src][N] signals and [B][n_src][n_q_max] angles into the concatenated layout
//                          (zero pad to K, zero gaps, filler angles), one launch;
//   bas_batch_finish_f32 - per-item m = max|y| over both ears of the item's window (apply_hrtf.py:462) and, with
//                          normalize, the rule per item (:463-464), in place or compacted to [B][2][T_out_max];
//                          two launches (maxima, then scale/compact), no inter-workgroup waiting.
#include "bas_internal.h"
#include "bas_delay.h"

#define BB_THREADS 256

// One row of workgroups per item (blockIdx.y = b): item b's segment [off_b, off_{b+1}) of every source row (the last one to
// x_stride), 4 samples per thread (16-byte store; rows 16-byte aligned, stride a multiple of 4 floats), then the segment's
// chunk boundaries [off_b/K, off_{b+1}/K) (the last one to n_q), one (elev, azim) pair per thread.  Every float of
// x[s][0 .. x_stride) is written: the pad and the gaps are 0.  No search: the item is the row's.  GAIN: gain [B][n_src]
// [n_q_max] is packed into gain_out like the angles.  DELAY: every sample of an item's segment is its
// delayed input, read from the item's own row and its own delay row delay[b][s][0 .. n_q_max) (no packed
// delay array), bounded by the item's valid length: reads outside [0, len_b) are 0, and so are the outputs at t >= len_b.
template <bool GAIN, bool DELAY>
__global__ __launch_bounds__(BB_THREADS) void bas_batch_pack_kernel(
    const float *__restrict__ sig, int n_items, int n_src, long N, const long *__restrict__ len, const long *__restrict__ off,
    const double *__restrict__ elev, const double *__restrict__ azim, long n_q_max, int K, long n_q,
    float *__restrict__ x, long x_stride, double *__restrict__ elev_out, double *__restrict__ azim_out,
    const double *__restrict__ gain, double *__restrict__ gain_out, const double *__restrict__ delay, int interp) {
    const int b0 = blockIdx.y;
    const bool last = b0 + 1 == n_items;
    const long start = off[b0], end = last ? x_stride : off[b0 + 1];
    const long q_lo = (start + 3) >> 2, q_hi = (end + 3) >> 2;               // quads whose first sample lies in the segment
    const long a_lo = start / K, a_hi = last ? n_q : off[b0 + 1] / K;
    const long nq = q_hi - q_lo, per_src = nq + (a_hi - a_lo);
    const long gstride = (long)gridDim.x * BB_THREADS;
    const bool sig_quads = (reinterpret_cast<uintptr_t>(sig) & 15) == 0 && (N & 3) == 0;
    const long n_own = min(len[b0], N);
    for (long i = blockIdx.x * (long)BB_THREADS + threadIdx.x; i < per_src * n_src; i += gstride) {
        const int s = (int)(i / per_src);
        const long r = i - (long)s * per_src;
        if (r < nq) {
            const long t0 = (q_lo + r) << 2;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            int b = b0;
            long o = start, n = n_own;
            const float *row = sig + ((long)b * n_src + s) * N;
            if constexpr (DELAY) {
                for (int k = 0; k < 4; ++k) {
                    const long t = t0 + k;
                    while (b + 1 < n_items && off[b + 1] <= t) {          // the quad crosses into the next segment
                        ++b;
                        o = off[b];
                        n = min(len[b], N);
                        row = sig + ((long)b * n_src + s) * N;
                    }
                    const long tl = t - o;                               // (o is a multiple of K: chunk-relative as alone)
                    if (tl < n) {
                        const long c = tl / K;
                        const double *drow = delay + ((long)b * n_src + s) * n_q_max;
                        v[k] = bas_delay_sample(row, 0, n, c * K, (int)(tl - c * K), K, drow[c], drow[c + 1],
                                                bas_delay_min(interp), (double)n + 4.0, interp);
                    }
                }
            } else if (t0 + 3 < o + n && sig_quads && ((t0 - o) & 3) == 0) {
                const f32x4 q = *reinterpret_cast<const f32x4 *>(row + (t0 - o));
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                for (int k = 0; k < 4; ++k) {
                    const long t = t0 + k;
                    while (b + 1 < n_items && off[b + 1] <= t) {          // the quad crosses into the next segment
                        ++b;
                        o = off[b];
                        n = min(len[b], N);
                        row = sig + ((long)b * n_src + s) * N;
                    }
                    if (t - o < n) v[k] = row[t - o];
                }
            }
            f32x4 q;
            q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
            *reinterpret_cast<f32x4 *>(x + (long)s * x_stride + t0) = q;
        } else {
            const long q = a_lo + (r - nq);
            const long n_chunks = (n_own + K - 1) / K;                     // the item's own boundaries: 0 .. n_chunks
            long c = q - a_lo;
            if (c > n_chunks) c = n_chunks;                              // filler: repeats the item's last angle (input is 0)
            if (c > n_q_max - 1) c = n_q_max - 1;
            const long src = ((long)b0 * n_src + s) * n_q_max + c;
            elev_out[(long)s * n_q + q] = elev[src];
            azim_out[(long)s * n_q + q] = azim[src];
            if constexpr (GAIN) gain_out[(long)s * n_q + q] = gain[src];        // (filler: the item's last gain)
        }
    }
}

// float4 when the window start is 16-byte aligned, else scalars (still coalesced across a wave)
__device__ __forceinline__ bool bas_aligned16(const float *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// launch 1: peak_bits[b] = max over the workgroups of item b of max|y[e][off_b .. off_b + n_b)|, e = 0, 1.  atomicMax on the
// bits of a non-negative float is exact and order-free: the result does not depend on which workgroup comes first.
__global__ __launch_bounds__(BB_THREADS) void bas_batch_peaks_kernel(const float *__restrict__ y, long y_stride,
                                                                     const long *__restrict__ off,
                                                                     const long *__restrict__ out_len,
                                                                     unsigned int *__restrict__ peak_bits) {
    const int b = blockIdx.y;
    const long n = out_len[b];
    const long gstride = (long)gridDim.x * BB_THREADS;
    float lmax = 0.f;
    for (int e = 0; e < 2; ++e) {
        const float *w = y + e * y_stride + off[b];
        const long head = bas_aligned16(w) ? 0 : min(n, (long)((16 - (reinterpret_cast<uintptr_t>(w) & 15)) >> 2));
        if (blockIdx.x == 0 && threadIdx.x < head) lmax = bas_peak_max(lmax, w[threadIdx.x]);
        const float *wa = w + head;
        const long nq = (n - head) >> 2;
        for (long i = blockIdx.x * (long)BB_THREADS + threadIdx.x; i < nq; i += gstride) {
            const f32x4 q = *reinterpret_cast<const f32x4 *>(wa + 4 * i);
            lmax = bas_peak_max4(lmax, q);
        }
        const long tail0 = head + 4 * nq;
        if (blockIdx.x == 0 && tail0 + threadIdx.x < n) lmax = bas_peak_max(lmax, w[tail0 + threadIdx.x]);
    }
    bas_block_peak_max(lmax, peak_bits + b);
}

// launch 2, in place: y[e][off_b + i] /= m_b when m_b > 1 (:463-464; a division, as the reference and bas_scale_by_peak_f32)
__global__ __launch_bounds__(BB_THREADS) void bas_batch_scale_kernel(float *__restrict__ y, long y_stride,
                                                                     const long *__restrict__ off,
                                                                     const long *__restrict__ out_len,
                                                                     const float *__restrict__ peaks) {
    const int b = blockIdx.y;
    const float m = peaks[b];
    if (!(m > 1.0f)) return;
    const long n = out_len[b];
    const long gstride = (long)gridDim.x * BB_THREADS;
    for (int e = 0; e < 2; ++e) {
        float *w = y + e * y_stride + off[b];
        const long head = bas_aligned16(w) ? 0 : min(n, (long)((16 - (reinterpret_cast<uintptr_t>(w) & 15)) >> 2));
        if (blockIdx.x == 0 && threadIdx.x < head) w[threadIdx.x] = w[threadIdx.x] / m;
        float *wa = w + head;
        const long nq = (n - head) >> 2;
        for (long i = blockIdx.x * (long)BB_THREADS + threadIdx.x; i < nq; i += gstride) {
            f32x4 q = *reinterpret_cast<f32x4 *>(wa + 4 * i);
            q.x = q.x / m; q.y = q.y / m; q.z = q.z / m; q.w = q.w / m;
            *reinterpret_cast<f32x4 *>(wa + 4 * i) = q;
        }
        const long tail0 = head + 4 * nq;
        if (blockIdx.x == 0 && tail0 + threadIdx.x < n) w[tail0 + threadIdx.x] = w[tail0 + threadIdx.x] / m;
    }
}

// launch 2, compacting: out[b][e][i] = y[e][off_b + i] (/ m_b when normalize and m_b > 1) for i < n_b, 0 up to out_len_max.
// Every float of out[b] is written.  4 consecutive samples per thread; 16-byte loads and stores when both ends are aligned.
__global__ __launch_bounds__(BB_THREADS) void bas_batch_compact_kernel(const float *__restrict__ y, long y_stride,
                                                                       const long *__restrict__ off,
                                                                       const long *__restrict__ out_len,
                                                                       const float *__restrict__ peaks, int normalize,
                                                                       float *__restrict__ out, long out_len_max) {
    const int b = blockIdx.y;
    const float m = peaks[b];
    const bool scale = normalize && m > 1.0f;
    const long n = out_len[b];
    const long nq = (out_len_max + 3) >> 2;
    const long gstride = (long)gridDim.x * BB_THREADS;
    for (int e = 0; e < 2; ++e) {
        const float *w = y + e * y_stride + off[b];
        float *d = out + ((long)b * 2 + e) * out_len_max;
        const bool quads = bas_aligned16(w) && bas_aligned16(d);
        for (long i = blockIdx.x * (long)BB_THREADS + threadIdx.x; i < nq; i += gstride) {
            const long t0 = 4 * i;
            if (quads && t0 + 3 < n && t0 + 3 < out_len_max) {
                f32x4 q = *reinterpret_cast<const f32x4 *>(w + t0);
                if (scale) { q.x = q.x / m; q.y = q.y / m; q.z = q.z / m; q.w = q.w / m; }
                *reinterpret_cast<f32x4 *>(d + t0) = q;
            } else {
                for (int k = 0; k < 4 && t0 + k < out_len_max; ++k) {
                    float v = t0 + k < n ? w[t0 + k] : 0.f;
                    d[t0 + k] = scale ? v / m : v;
                }
            }
        }
    }
}

// workgroups per item: about 8 per CU over the whole batch, at least one, at most one per 1024 samples of the longest window
static int batch_blocks_x(int n_items, long max_len) {
    long want = (8L * bas_device_cus() + n_items - 1) / n_items;
    const long cap = max_len / 1024 + (max_len % 1024 != 0);  // (ceil without max_len + 1023: any long)
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    if (want > 65535) want = 65535;
    return (int)want;
}

static int batch_pack(const char *who, const float *sig, int n_items, int n_src, long N, const long *lengths,
                      const long *offsets, const double *elev, const double *azim, const double *gain, bool need_gain,
                      const double *delay, bool need_delay, int interp, long n_q_max, int K, long T_in, float *x,
                      long x_stride, double *elev_out, double *azim_out, double *gain_out, bas_stream_t stream) {
    BAS_REQUIRE(n_items > 0 && n_src > 0 && N >= 0 && K > 0 && T_in > 0 && n_q_max > 0, BAS_E_SHAPE,
                "%s: need n_items, n_src, K, T_in, n_q_max > 0 and N >= 0", who);
    BAS_REQUIRE(T_in % K == 0, BAS_E_SHAPE, "%s: T_in (%ld) must be a multiple of K (%d)", who, T_in, K);
    BAS_REQUIRE(T_in <= BAS_MAX_T_IN && x_stride >= T_in && x_stride % 4 == 0, BAS_E_SHAPE,
                "%s: x_stride must be >= T_in and a multiple of 4, T_in <= 2^41", who);
    BAS_REQUIRE(lengths && offsets && elev && azim && x && elev_out && azim_out && (sig || N == 0) &&
                    (!need_gain || (gain && gain_out)) && (!need_delay || delay),
                BAS_E_NULL, "%s: null pointer", who);
    BAS_REQUIRE(!need_delay || interp == BAS_DELAY_LINEAR || interp == BAS_DELAY_CUBIC, BAS_E_SHAPE,
                "%s: interp must be 0 (linear) or 1 (cubic)", who);
    BAS_REQUIRE(reinterpret_cast<uintptr_t>(x) % 16 == 0, BAS_E_ALIGN, "%s: x must be 16-byte aligned", who);
    BAS_REQUIRE(n_items <= 65535, BAS_E_SHAPE, "%s: more than 65535 items in one call", who);
    const long n_q = T_in / K + 1;
    long per_item = x_stride / n_items + (x_stride % n_items != 0);   // ceil; capped: the product with n_src stays a long
    if (per_item > (1L << 31)) per_item = 1L << 31;
    const dim3 grid(batch_blocks_x(n_items, n_src * per_item), n_items);
    const double *g = need_gain ? gain : nullptr;
    double *go = need_gain ? gain_out : nullptr;
    if (need_delay && need_gain)
        hipLaunchKernelGGL((bas_batch_pack_kernel<true, true>), grid, dim3(BB_THREADS), 0, bas_stream(stream), sig, n_items,
                           n_src, N, lengths, offsets, elev, azim, n_q_max, K, n_q, x, x_stride, elev_out, azim_out, g, go,
                           delay, interp);
    else if (need_delay)
        hipLaunchKernelGGL((bas_batch_pack_kernel<false, true>), grid, dim3(BB_THREADS), 0, bas_stream(stream), sig, n_items,
                           n_src, N, lengths, offsets, elev, azim, n_q_max, K, n_q, x, x_stride, elev_out, azim_out, g, go,
                           delay, interp);
    else if (need_gain)
        hipLaunchKernelGGL((bas_batch_pack_kernel<true, false>), grid, dim3(BB_THREADS), 0, bas_stream(stream), sig, n_items,
                           n_src, N, lengths, offsets, elev, azim, n_q_max, K, n_q, x, x_stride, elev_out, azim_out, g, go,
                           nullptr, 0);
    else
        hipLaunchKernelGGL((bas_batch_pack_kernel<false, false>), grid, dim3(BB_THREADS), 0, bas_stream(stream), sig, n_items,
                           n_src, N, lengths, offsets, elev, azim, n_q_max, K, n_q, x, x_stride, elev_out, azim_out, nullptr,
                           nullptr, nullptr, 0);
    return bas_check_launch(who);
}

extern "C" int bas_batch_pack_f32(const float *sig, int n_items, int n_src, long N, const long *lengths,
                                  const long *offsets, const double *elev, const double *azim, long n_q_max, int K,
                                  long T_in, float *x, long x_stride, double *elev_out, double *azim_out,
                                  bas_stream_t stream) {
    return batch_pack("bas_batch_pack_f32", sig, n_items, n_src, N, lengths, offsets, elev, azim, nullptr, false, nullptr,
                      false, 0, n_q_max, K, T_in, x, x_stride, elev_out, azim_out, nullptr, stream);
}

// apply_hrtf.py:429-447 per item with per-boundary gains: gain [B][n_src][n_q_max] -> gain_out
// [n_src][T_in/K + 1], packed as the angles (the gap's inner boundaries repeat the item's last gain)
extern "C" int bas_batch_pack_gain_f32(const float *sig, int n_items, int n_src, long N, const long *lengths,
                                       const long *offsets, const double *elev, const double *azim, const double *gain,
                                       long n_q_max, int K, long T_in, float *x, long x_stride, double *elev_out,
                                       double *azim_out, double *gain_out, bas_stream_t stream) {
    return batch_pack("bas_batch_pack_gain_f32", sig, n_items, n_src, N, lengths, offsets, elev, azim, gain, true, nullptr,
                      false, 0, n_q_max, K, T_in, x, x_stride, elev_out, azim_out, gain_out, stream);
}

// apply_hrtf.py:405-406 per item with a per-source propagation delay: delay [B][n_src][n_q_max] is
// read where it is, item b's delayed input goes into its segment; gain may be NULL (then gain_out is ignored)
extern "C" int bas_batch_pack_delay_f32(const float *sig, int n_items, int n_src, long N, const long *lengths,
                                        const long *offsets, const double *elev, const double *azim, const double *gain,
                                        const double *delay, int interp, long n_q_max, int K, long T_in, float *x,
                                        long x_stride, double *elev_out, double *azim_out, double *gain_out,
                                        bas_stream_t stream) {
    return batch_pack("bas_batch_pack_delay_f32", sig, n_items, n_src, N, lengths, offsets, elev, azim, gain, gain != nullptr,
                      delay, true, interp, n_q_max, K, T_in, x, x_stride, elev_out, azim_out, gain_out, stream);
}

extern "C" int bas_batch_finish_f32(float *y, long y_stride, int n_items, const long *offsets, const long *out_lengths,
                                    long out_len_max, int normalize, float *out, float *peaks, bas_stream_t stream) {
    BAS_REQUIRE(n_items > 0 && n_items <= 65535 && out_len_max >= 0 && y_stride >= 0, BAS_E_SHAPE,
                "bas_batch_finish_f32: need 0 < n_items <= 65535, out_len_max >= 0, y_stride >= 0");
    BAS_REQUIRE(y && offsets && out_lengths && peaks, BAS_E_NULL, "bas_batch_finish_f32: null pointer");
    hipStream_t st = bas_stream(stream);
    hipError_t e = hipMemsetAsync(peaks, 0, (size_t)n_items * sizeof(float), st);
    if (e != hipSuccess) return bas_fail((int)e, "bas_batch_finish_f32: hipMemsetAsync: %s", hipGetErrorString(e));
    const dim3 grid(batch_blocks_x(n_items, out_len_max), n_items);
    hipLaunchKernelGGL(bas_batch_peaks_kernel, grid, dim3(BB_THREADS), 0, st, y, y_stride, offsets, out_lengths,
                       reinterpret_cast<unsigned int *>(peaks));
    int rc = bas_check_launch("bas_batch_finish_f32(peaks)");
    if (rc) return rc;
    if (out) {
        hipLaunchKernelGGL(bas_batch_compact_kernel, grid, dim3(BB_THREADS), 0, st, y, y_stride, offsets, out_lengths,
                           peaks, normalize, out, out_len_max);
        return bas_check_launch("bas_batch_finish_f32(compact)");
    }
    if (!normalize) return 0;
    hipLaunchKernelGGL(bas_batch_scale_kernel, grid, dim3(BB_THREADS), 0, st, y, y_stride, offsets, out_lengths, peaks);
    return bas_check_launch("bas_batch_finish_f32(scale)");
}
