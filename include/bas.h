/* bas.h - C ABI of the MI355X (gfx950) binaural render library, libbas_hip.so.
 *
 * The reference (mbjd/binaural-audio-synthesis) is pure Python and has no FFI
 * boundary of its own: its boundary for the moving-source render path is three
 * Python functions in apply_hrtf.py.  This header is the native boundary this
 * build puts BEHIND those functions; every entry point names the reference
 * interface it replaces (file:line into the reference tree).  The ctypes stub a
 * reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     marked "host"; nothing here allocates, frees or retains caller memory.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream) and returns without synchronising, so calls can be
 *     captured into a hipGraph.
 *   - return value: 0 = ok, negative = BAS_E_* argument/shape error (nothing
 *     was enqueued), positive = hipError_t reported by the launch.
 *     bas_last_error() returns a thread-local description of the last failure.
 *   - re-entrant; no mutable global state besides that thread-local string.
 *   - float data is IEEE binary32, computed in binary32 on the device ("f32");
 *     delay bookkeeping (shift amounts) is computed in binary64.
 */
#ifndef BAS_H
#define BAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BAS_ABI_VERSION 7

#define BAS_E_NULL      (-1)   /* a required pointer is NULL                    */
#define BAS_E_SHAPE     (-2)   /* inconsistent or unsupported sizes             */
#define BAS_E_ALIGN     (-3)   /* pointer/stride alignment requirement violated */
#define BAS_E_WORKSPACE (-4)   /* workspace too small                           */

#define BAS_WS_CONTROL_BYTES 2048   /* head of every workspace: the library's control block (see bas_render_mix_fused_f32) */

/* Ceilings of the render sizes (n_src, T_in, K, S, L).  Inside them every size and plan query is computed without
 * overflow and in bounded time; beyond any of them bas_render_fused_supported answers 0 (kernel name "", workspace
 * of the head alone), bas_render_kernel_name answers the generic kernel, bas_render_workspace_bytes the head alone,
 * and the render entry points (bas_render_mix_f32, bas_render_mix_fused_f32, their _profiled, _fir_, _reduce_ and
 * stream-block siblings) return BAS_E_SHAPE.  Each comes from what the kernels can address:
 *   BAS_MAX_K      2^24: the crossfade weight of an input sample is (float)(m % K) / K (apply_hrtf.py:442-443 in
 *                  binary32), and binary32 holds the integers up to 2^24 exactly;
 *   BAS_MAX_L      2^18: the fused kernels read the packed table through 32-bit byte offsets, so
 *                  2 ears x ndir x U x (L + 4) x 4 bytes < 2^31; with the table's 187 directions and the smallest
 *                  planned factor U = 4 that is L < 358 836, and 2^18 is the power of two below;
 *   BAS_MAX_N_SRC  2^30 - 1: the n_src x (T_in / K + 1) chunk-boundary queries of a render are counted in an int
 *                  and every source has at least two boundaries;
 *   BAS_MAX_T_IN   2^41: (tile, source) work units are int indices, and the smallest tile has 2048 outputs, so
 *                  T_in + L - 1 < 2^31 x 2^11 = 2^42; 2^41 leaves room for any L.  (T_in / K < 2^30 still holds
 *                  on top: the chunk index is an int.)
 * A shape inside the ceilings whose (tile, source) units reach 2^31 - 65536 gets a workspace size of the head alone and
 * BAS_E_SHAPE ("render in blocks") from the render entry points that would run a fast kernel. */
#define BAS_MAX_K     (1 << 24)
#define BAS_MAX_L     (1 << 18)
#define BAS_MAX_N_SRC ((1 << 30) - 1)
#define BAS_MAX_T_IN  (1L << 41)

typedef void *bas_stream_t;    /* hipStream_t */

/* Library / ABI version (BAS_ABI_VERSION). */
int bas_version(void);

/* Thread-local text for the last non-zero return on this thread ("" if none). */
const char *bas_last_error(void);

/* ---- a1: table layout ----------------------------------------------------
 * Replaces the in-memory table produced by load_irs_and_delaydiffs
 * (apply_hrtf.py:23-46): irs_left/irs_right truncated to M = samples_to_keep*U
 * columns (:43-44).  Re-lays the row-major table
 *     irs   [2 ears][ndir][M]            (ear 0 = left)
 * as phase planes with guard floats at both ends of every plane
 *     packed[2 ears][ndir][U][L + 4],  packed[e][p][i % U][1 + i / U] = irs[e][p][i],
 *     packed[e][p][ph][0] = sample L-1 of the plane, packed[e][p][ph][L+1 .. L+3] = samples 0..2
 * (circular neighbours), L = M / U, so that the stride-U reads of a fractional
 * shift followed by decimation (apply_hrtf.py:156-165) are contiguous across
 * lanes and neither "one sample earlier" nor "the next three taps" need a wrap test.  bas_table_packed_floats() gives
 * the size of `packed` in floats (0 for invalid shapes); the layout belongs to the library build that packed it
 * (a build with -DBAS_PLANE_DOUBLE=1 keeps every plane's samples twice).  Every entry point that takes a table,
 * bas_table_pack_f32 included, refuses one of 2^31 floats or more (BAS_E_SHAPE: the kernels use 32-bit offsets). */
size_t bas_table_packed_floats(int ndir, int M, int U);
int bas_table_pack_f32(const float *irs, int ndir, int M, int U, float *packed,
                       bas_stream_t stream);

/* ---- a4: delay_signal_float (apply_hrtf.py:127-165) ------------------------
 * y[i][j] = (1-f) x[i][(j*down - floor s_i) mod M] + f x[i][(j*down - ceil s_i) mod M],
 * f = s_i - floor s_i, j = 0..ceil(M/down)-1; circular like np.roll (:156-157);
 * decimation before the blend (:160-163).
 *   x [n][M] f32, shifts [n] f64 (samples), y [n][ceil(M/down)] f32. */
int bas_delay_signal_f32(const float *x, const double *shifts, int n, int M, int down,
                         float *y, bas_stream_t stream);

/* ---- a5: delay_compensated_interpolation_with_delaydiff (apply_hrtf.py:53-106)
 *   packed  table from bas_table_pack_f32
 *   diffs   [2 ears][ndir][ndir] f64   (diffs_left, diffs_right; :40-41)
 *   pq      [n][2] int32   (before, after)
 *   alpha   [n] f64
 *   out     [n][2 ears][return_upsampled ? M : L] f32   (:97-104)
 *   delays  [n][2 ears] f64, in non-upsampled samples (:106); may be NULL. */
int bas_ring_interp_f32(const float *packed, const double *diffs, const int32_t *pq,
                        const double *alpha, int n, int ndir, int L, int U,
                        int return_upsampled, float *out, double *delays,
                        bas_stream_t stream);

/* ---- a3 + elevation bracket on the device --------------------------------------
 * (elev, azim) radians -> the (idx, w) inputs of bas_interp2d_f32, float64 branch of
 * sphere.azim_to_interpolation_params (sphere.py:78-121) plus interpolate_2d's elevation
 * bracket and vertical weight (apply_hrtf.py:199-215, :261-266); azimuth wrapped,
 * elevation clamped like the reference.  Same arithmetic as the host's
 * sphere.interpolation_params_batch (bit-identical on finite inputs; tested).
 *   elev, azim [n] f64 (device); idx [n][4] int32, w [n][3] f64 (device)
 *   ring_elev[10] f64, ring_start[10], ring_count[10] int32: HOST arrays (the ten rings:
 *   deg2rad(-45..90), first direction index, number of azimuths); node_az [187] f32
 *   DEVICE array of the table's node azimuths (sphere.py:318 float32 values), ascending
 *   inside every ring with the ring's first node at azimuth 0, as sphere.py:124-319 lists
 *   them: the search for "the last node <= azim" (sphere.py:103) starts from azim's
 *   position on an evenly spaced ring and walks to the exact node. */
int bas_traj_params_f64(const double *elev, const double *azim, long n, const double *ring_elev,
                        const int32_t *ring_start, const int32_t *ring_count, const float *node_az,
                        int32_t *idx, double *w, bas_stream_t stream);

/* The same with the reference's OTHER numeric branch selectable.  Which one the reference takes
 * depends on the scalar type its trajectory function returns (NumPy >= 2 promotion rules):
 *   BAS_BRANCH_F64      azimuth is an np.float64: node comparisons (sphere.py:103-104) and the weight
 *                       a = (azim - az_b) / (az_a - az_b) (:119) in binary64 against the float32 node
 *                       values (= bas_traj_params_f64);
 *   BAS_BRANCH_PYFLOAT  azimuth is a Python float (what the reference's own presets circle_horizontal,
 *                       circle_askew and spiral return, apply_hrtf.py:585-586, :593): the azimuth is
 *                       wrapped in binary64 (:86), then rounded to binary32; comparisons and the weight
 *                       are binary32 (the weight is returned widened to f64).
 * The elevation bracket and the vertical weight (apply_hrtf.py:199-215, :261-266) are binary64 in
 * both branches, as in the reference. */
#define BAS_BRANCH_F64     0
#define BAS_BRANCH_PYFLOAT 1
int bas_traj_params_branch_f64(const double *elev, const double *azim, long n,
                               const double *ring_elev, const int32_t *ring_start,
                               const int32_t *ring_count, const float *node_az, int32_t *idx,
                               double *w, int branch, bas_stream_t stream);

/* ---- a6: interpolate_2d (apply_hrtf.py:171-281), batched --------------------
 * The angle -> (indices, weights) step (sphere.py:78-121 and the elevation
 * bracket apply_hrtf.py:199-215, :261-266) is host logic; this entry point does
 * all table arithmetic (:219-279).
 *   idx [n][4] int32 = (top_before, top_after, bot_before, bot_after)
 *   w   [n][3] f64   = (top_alpha, bot_alpha, a)
 *   H   [n][2 ears][L] f32
 *   ws / ws_bytes: 16-byte aligned scratch of bas_interp2d_workspace_bytes(n) bytes
 *      (per-(query, ear) read plans handed from the plan kernel to the eval kernel).  BAS_E_WORKSPACE when it is NULL,
 *      too small or not 16-byte aligned - here and for the `plans` buffer of the bas_interp2d_plan_* entry points. */
size_t bas_interp2d_workspace_bytes(int n);
int bas_interp2d_f32(const float *packed, const double *diffs, const int32_t *idx,
                     const double *w, int n, int ndir, int L, int U, float *H, void *ws,
                     size_t ws_bytes, bas_stream_t stream);

/* ---- a7/a8: make_signal_move_2d inner loops (apply_hrtf.py:431-453) ---------
 * For every source s, input sample m and tap k:
 *   y[e][m+k] += x[s][m] * ((1-al) H[s][c][e][k] + al H[s][c+1][e][k]),
 *   c = m / K,  al = ((m % K) / S) * S / K            (:442-443, :445-446, :450-453)
 * i.e. per-subchunk crossfaded IR, direct-form FIR (what scipy.signal.convolve
 * resolves to at these sizes), overlap-add, summed over sources.
 *   x  [n_src] rows of T_in floats, row stride x_stride floats; T_in % K == 0
 *      (the caller zero-pads as apply_hrtf.py:405-406 does).  The fast kernels need x 16-byte
 *      aligned and x_stride % 4 == 0 (else the plain kernel runs); when T_in % 4 != 0 they read
 *      every row up to the next multiple of 4 floats, which x_stride then covers - also for
 *      the last row, so allocate n_src * x_stride floats.
 *   H  [n_src][T_in/K + 1][2][L] f32 (bas_interp2d_f32 output, chunk IRs at
 *      t = 0, K, .., T_in; :429, :435)
 *   y  [2][T_in + L - 1] f32; overwritten, or added to when accumulate != 0
 *   peak (may be NULL): device float receiving max|y| of the result (:462),
 *      fused into the final pass
 *   ws / ws_bytes: scratch of at least bas_render_workspace_bytes(...) bytes; its first BAS_WS_CONTROL_BYTES are the library's
 *      control block (see bas_render_mix_fused_f32: zero them once after allocating), which this entry point leaves alone. */
size_t bas_render_workspace_bytes(int n_src, long T_in, int K, int S, int L);

/* Name of the FIR kernel bas_render_mix_f32 launches for these sizes with aligned
 * operands ("bas_render_hd_kernel", "bas_render_rows32_kernel" or
 * "bas_render_generic_kernel"); for profiling tools.  The hd kernel (fast path) serves
 * chunk sizes from about 72 samples up with any subchunk size >= 4: multiples of 32 (and
 * 16 / 8 / 4 with K % 32 == 0) at full speed, other sizes through a multi-part row step
 * (2 to 5 times the arithmetic); rows32 serves smaller chunks with subchunks that are
 * multiples of 32; everything else runs the plain generic kernel. */
const char *bas_render_kernel_name(int n_src, long T_in, int K, int S, int L);

int bas_render_mix_f32(const float *x, long x_stride, const float *H, int n_src, long T_in,
                       int K, int S, int L, float *y, int accumulate, float *peak,
                       void *ws, size_t ws_bytes, bas_stream_t stream);

/* Same call; additionally records the caller's hipEvent_t pair (passed as void*, either
 * may be NULL) on `stream` immediately before and after the FIR kernel, so a
 * benchmark can time the dominant kernel live with HIP events. */
int bas_render_mix_profiled_f32(const float *x, long x_stride, const float *H, int n_src,
                                long T_in, int K, int S, int L, float *y, int accumulate,
                                float *peak, void *ws, size_t ws_bytes, bas_stream_t stream,
                                void *ev_begin, void *ev_end);

/* ---- a6 + a7 fused: chunk IRs evaluated inside the FIR kernel ------------------
 * bas_interp2d_plan_f32 runs only the per-(query, ear) plan step of bas_interp2d_f32
 * (delays, shift splits, the 16 folded blend weights; apply_hrtf.py:219-279) and
 * leaves n*2 read plans of 144 bytes in `plans` (bas_interp2d_workspace_bytes(n) bytes,
 * 16-byte aligned; query order [n_src][T_in/K + 1]; needs U >= 4).
 * bas_render_mix_fused_f32 is bas_render_mix_f32 with H replaced by (packed table, plans):
 * the workgroups evaluate the chunk IRs they need while staging (plans staged in LDS,
 * table samples by buffer loads), so the [n][2][L] IR array never exists in HBM.
 * Served for chunk sizes K >= 448 or so (K % 32 == 0) with subchunks that are multiples
 * of 32, for K >= 256 when the scene has at least two workgroups' worth of
 * (8192-output tile, source) units per CU, and for subchunks of 16 and 8 samples (the reference accepts any
 * divisor of the chunk, apply_hrtf.py:401-402) in scenes with more than one such unit per CU and
 * L = 97 .. 104 or 121 .. 128: check bas_render_fused_supported (1 = yes) and
 * otherwise use bas_interp2d_f32 + bas_render_mix_f32.  Scenes with few sources get
 * smaller tiles (2048 outputs) and more workgroups.  ndir = directions in the table (187).
 * ws / ws_bytes: scratch of bas_render_fused_workspace_bytes(...) bytes, 16-byte aligned.  Its first BAS_WS_CONTROL_BYTES (2048) are the
 *    library's control block (arrival counters of the kernel tails, the device-side error record): zero them ONCE after
 *    allocating the workspace (hipMemset); every call leaves the counters zero, so the workspace can be reused call after
 *    call and inside hipGraph replays.  One workspace serves one stream at a time.
 * x must be 16-byte aligned with x_stride % 4 == 0 (BAS_E_ALIGN otherwise).
 * normalize != 0: the peak rule of make_signal_move_2d (apply_hrtf.py:462-464: m = max|y|; if m > 1: y /= m) is applied
 *    to y before the call's work on `stream` ends - inside the tail of the last kernel (no launch of its own; the workgroups
 *    that finish last share the rescale) whenever y is 16-byte aligned, else by bas_scale_by_peak_f32.  `peak` (may be NULL)
 *    receives max|y| BEFORE the rule either way.
 *    Every max|.| of this library (here, the batch's and the streams' peaks, the late tail's, the meters') is taken on the
 *    bit patterns of |y|: a NaN among the samples makes it NaN - and it stays NaN - and +-Inf without
 *    a NaN makes it +Inf.  The rule acts on that value as the reference's `if m > 1` does: a NaN peak leaves y as it is,
 *    a +Inf peak divides by it.
 * n == 0 (no queries / no sources) is served by every entry point: the per-query arrays may then be NULL. */
int bas_interp2d_plan_f32(const double *diffs, const int32_t *idx, const double *w, int n,
                          int ndir, int L, int U, void *plans, size_t plans_bytes,
                          bas_stream_t stream);
/* bas_traj_params_branch_f64 + bas_interp2d_plan_f32 in ONE launch (a3 and the plan step of a6: sphere.py:78-121,
 * apply_hrtf.py:199-279): the first two waves of a block do the angle arithmetic of its 128 queries, the (query, ear)
 * threads of all four take the parameters from LDS - no (idx, w) round trip through HBM, one launch less (what every
 * render from angles runs since round 4; one source x 10 s is 863 queries, the headline scene 221 k).
 * Same plans, bit for bit, as the two calls.  elev / azim [n] f64 device; ring_* host, node_az device, branch as in
 * bas_traj_params_branch_f64. */
int bas_interp2d_plan_angles_f32(const double *diffs, const double *elev, const double *azim, int n,
                                 const double *ring_elev, const int32_t *ring_start,
                                 const int32_t *ring_count, const float *node_az, int branch, int ndir,
                                 int L, int U, void *plans, size_t plans_bytes, bas_stream_t stream);
int bas_render_fused_supported(int n_src, long T_in, int K, int S, int L);
/* Name of the kernel bas_render_mix_fused_f32 launches for these operands, for profiling tools ("" when the sizes are
 * not served): "bas_render_fs_kernel<128>" / "<104>" / "<0>" - one workgroup of four filter and four stager waves per
 * CU, two LDS buffers (scenes with more than one (tile of 8192, source) unit per CU; <128>: L = 121 .. 128 and the lengths of
 * several whole 128-tap segments - 249 .. 256, 377 .. 384, 505 .. 512, .. -, <104>: L = 97 .. 104: the five row steps of
 * a (unit, segment) pass as one assembly block; "<128,2>" / "<104,2>", "<128,4>" / "<104,4>": the same
 * for subchunks of 16 / 8 samples - two / four crossfaded tap sets per row of 32 inputs); "bas_render_fq_kernel" - four waves per tile of 2048
 * outputs, staging and row steps dealt over them (small scenes: one source, a handful, real-time blocks) - or
 * "bas_render_fz_kernel<4,0>" / "<1,0>" / "<4,1>": every wave stages and filters (two workgroups of four waves per CU on
 * tiles of 8192 outputs / eight one-wave workgroups on tiles of 2048; <4,1>: chunk sizes below ~448, h-only LDS rows). */
const char *bas_render_fused_kernel_name(int n_src, long T_in, int K, int S, int L);
size_t bas_render_fused_workspace_bytes(int n_src, long T_in, int K, int S, int L);
int bas_render_mix_fused_f32(const float *x, long x_stride, const float *packed,
                             const void *plans, int n_src, long T_in, int K, int S, int L,
                             int U, int ndir, float *y, int accumulate, float *peak, int normalize,
                             void *ws, size_t ws_bytes, bas_stream_t stream);

/* Same call; additionally records the caller's hipEvent_t pair (void*, either may be NULL) on `stream` immediately
 * before and after the FIR kernel (benchmarks time the dominant kernel live with HIP events). */
int bas_render_mix_fused_profiled_f32(const float *x, long x_stride, const float *packed,
                                      const void *plans, int n_src, long T_in, int K, int S, int L,
                                      int U, int ndir, float *y, int accumulate, float *peak,
                                      int normalize, void *ws, size_t ws_bytes, bas_stream_t stream,
                                      void *ev_begin, void *ev_end);

/* The two halves of bas_render_mix_fused_f32 as entry points of their own, same arguments: _fir_ launches the FIR kernel
 * (partial tiles into the workspace - or y itself, complete with peak and rule, for scenes whose tiles are each finished
 * by one workgroup, e.g. a single source), _reduce_ the fixed-order sum of the partial tiles into y with max|y| and the
 * peak rule.  Called back to back on one stream they ARE bas_render_mix_fused_f32; apart, a caller can put other work
 * of its own between them or on a second stream beside either (the read plans of its next block, the carry of its
 * previous one).  _reduce_ reads only the sizes, y, accumulate, peak, normalize and the workspace. */
int bas_render_fused_fir_f32(const float *x, long x_stride, const float *packed, const void *plans,
                             int n_src, long T_in, int K, int S, int L, int U, int ndir, float *y,
                             int accumulate, float *peak, int normalize, void *ws, size_t ws_bytes,
                             bas_stream_t stream);
int bas_render_fused_reduce_f32(const float *x, long x_stride, const float *packed, const void *plans,
                                int n_src, long T_in, int K, int S, int L, int U, int ndir, float *y,
                                int accumulate, float *peak, int normalize, void *ws, size_t ws_bytes,
                                bas_stream_t stream);

/* Device-side error record of a workspace (its control block): synchronises `stream`, returns 0 when no kernel that
 * used this workspace has reported anything since the last call, else a positive code (hipErrorLaunchTimeOut; text in
 * bas_last_error) and clears the record.  What can be reported: a stager wave that never received its neighbour's
 * boundary chunk IR inside a fused kernel (the affected outputs then hold NaN, never plausible audio), a kernel tail
 * whose late workgroups never saw the others arrive (peak rule not applied).  Neither has ever been observed; both used
 * to fall through silently.  Costs a stream synchronisation: call it where the caller synchronises anyway. */
int bas_render_status(void *ws, size_t ws_bytes, bas_stream_t stream);

/* ---- a7 (vii): peak normalisation (apply_hrtf.py:462-464) -------------------
 * m = max|y| over n floats; *peak = m (device float, may be NULL when apply);
 * if apply and m > 1: y /= m. */
int bas_peak_normalize_f32(float *y, long n, float *peak, int apply, bas_stream_t stream);

/* y /= *peak if *peak > 1 (second half of the rule, for a peak already known,
 * e.g. reduced across GPUs). */
int bas_scale_by_peak_f32(float *y, long n, const float *peak, bas_stream_t stream);

/* ---- multi-GPU combine (no reference counterpart; DESIGN.md "Multi-GPU") ------
 * y[i] = parts[0][i] + parts[1][i] + ... in that fixed order (deterministic),
 * parts[p] at parts + p*part_stride, n floats each; *peak = max|y| (may be NULL).
 * Used on the root rank after the RCCL gather of the per-GPU partial mixes. */
int bas_mix_partials_f32(const float *parts, int n_parts, long part_stride, long n, float *y,
                         float *peak, bas_stream_t stream);

/* The same sum, max|y| and - with normalize != 0 - the peak rule (apply_hrtf.py:462-464) in ONE launch: what the root
 * rank runs on the gathered partial mixes (bas_mix_partials_f32 + bas_scale_by_peak_f32 are a memset and two launches).
 * y and ws 16-byte aligned; ws: bas_mix_workspace_bytes() bytes whose first BAS_WS_CONTROL_BYTES are zero when first
 * used (the control block, as for bas_render_mix_fused_f32; a fused-render workspace may be passed). */
size_t bas_mix_workspace_bytes(void);
int bas_mix_finish_f32(const float *parts, int n_parts, long part_stride, long n, float *y, float *peak,
                       int normalize, void *ws, size_t ws_bytes, bas_stream_t stream);

/* ---- streaming: carried state of block-wise rendering -------
 * No reference counterpart: the reference renders one whole signal held in RAM
 * (apply_hrtf.py:405-414); its chunk loop is causal (:431-453), so a stream is rendered
 * as windows [halo | block] with halo = (L-1) rounded up to chunks.  After a window's
 * render this ONE launch moves everything that crosses the block boundary:
 *   running_peak = max(running_peak, max|y[e][halo .. halo+B)|)   (the peak of
 *       apply_hrtf.py:462 over the samples EMITTED so far; may be NULL)
 *   x[s][0 .. halo)  = x[s][B .. B+halo)           (input halo, every source)
 *   last[0][s], last[1][s] = elev/azim[s][nh+nb-1] (the angles at the block's end)
 *   elev/azim[s][0 .. nh) = elev/azim[s][nb-1 .. nb-1+nh)   (halo chunk boundaries)
 * x [n_src] rows, stride x_stride >= halo+B; elev/azim f64 [n_src] rows of nh+nb angles,
 * stride ang_stride; last f64 [2][n_src]; y [2] rows of the window's output, stride
 * y_stride; nh = halo / K, nb = B / K + 1. */
int bas_stream_epilogue_f32(float *x, long x_stride, int n_src, int halo, long B, double *elev,
                            double *azim, long ang_stride, int nh, int nb, double *last,
                            const float *y, long y_stride, float *running_peak,
                            bas_stream_t stream);

/* One block of a stream in one call (behind read plans of the window's chunk boundaries,
 * bas_interp2d_plan_angles_f32 over elev/azim [n_src][nh+nb]): the fused render of the
 * window x[s][0 .. T_in), T_in = halo + B, into y [2][T_in+L-1] - overwritten, no peak of
 * the window, no peak rule: a stream's samples leave before apply_hrtf.py:462-464 could
 * know its peak - followed by everything bas_stream_epilogue_f32 does (same arguments,
 * y_stride = T_in+L-1).  Where the scene's FIR kernel leaves slabs, the carried state and
 * the running peak ride in the reduce kernel (no launch of their own: 4.4 us of a
 * 256 x 512 real-time block's 30); where it writes y itself, the epilogue kernel is
 * launched.  Same results either way.  Sizes must be served by the fused kernels
 * (bas_render_fused_supported(n_src, T_in, K, S, L)); workspace as for
 * bas_render_mix_fused_f32.  x is WRITTEN (its first halo samples).
 * _profiled: HIP events around the FIR kernel (bench.py). */
int bas_render_stream_block_f32(float *x, long x_stride, const float *packed, const void *plans,
                                int n_src, long T_in, int K, int S, int L, int U, int ndir,
                                float *y, void *ws, size_t ws_bytes, int halo, double *elev,
                                double *azim, long ang_stride, int nh, int nb, double *last,
                                float *running_peak, bas_stream_t stream);
int bas_render_stream_block_profiled_f32(float *x, long x_stride, const float *packed,
                                         const void *plans, int n_src, long T_in, int K, int S,
                                         int L, int U, int ndir, float *y, void *ws,
                                         size_t ws_bytes, int halo, double *elev, double *azim,
                                         long ang_stride, int nh, int nb, double *last,
                                         float *running_peak, bas_stream_t stream,
                                         void *ev_begin, void *ev_end);

/* ---- batches of independent renders (no reference counterpart as a batch; DESIGN.md "Batches") ----------
 * B items, each rendered as if by make_signal_move_2d alone (apply_hrtf.py:356-466), in ONE render: item b occupies
 * [off_b, off_b + T_in_b) of every source row (T_in_b = len_b rounded up to K, :405-406), followed by a zero gap of G
 * samples (G >= L-1, a multiple of K) before off_{b+1}; its output is the window [off_b, off_b + T_in_b + L - 1) of the
 * long render.  offsets [B] and lengths [B] are int64 DEVICE arrays; off_0 = 0, strictly increasing.
 *
 * bas_batch_pack_f32: sig [B][n_src][N] float32 (len_b <= N valid samples per item) -> x [n_src] rows of x_stride
 *   floats (16-byte aligned, x_stride % 4 == 0; every float of a row written: the zero pad of :406 and the gaps);
 *   elev/azim [B][n_src][n_q_max] float64 (the item's angles at t = 0, K, .., T_in_b: :429, :435) -> elev_out/azim_out
 *   [n_src][T_in/K + 1]; the gap's inner boundaries repeat the item's last angle (their chunks' input is zero).  One launch.
 * bas_batch_finish_f32: y [2] rows of y_stride floats (the long render); out_lengths [B] = T_in_b + L - 1 (:410).
 *   peaks[b] = m_b = max|y| over both ears of item b's window (:462, device float [B], overwritten); with normalize != 0
 *   the rule per item: if m_b > 1 the window is divided by m_b (:463-464).  out == NULL: in place; else out [B][2]
 *   [out_len_max] is written whole (the window, then zeros).  A memset and two launches (maxima, then scale or compact);
 *   bitwise deterministic (max is exact; atomicMax on the bits of non-negative floats); B <= 65535.
 * Codes of the packs: x_stride < T_in, x_stride % 4 != 0 or T_in > BAS_MAX_T_IN: BAS_E_SHAPE; x not 16-byte aligned: BAS_E_ALIGN. */
int bas_batch_pack_f32(const float *sig, int n_items, int n_src, long N, const long *lengths, const long *offsets,
                       const double *elev, const double *azim, long n_q_max, int K, long T_in, float *x,
                       long x_stride, double *elev_out, double *azim_out, bas_stream_t stream);
int bas_batch_finish_f32(float *y, long y_stride, int n_items, const long *offsets, const long *out_lengths,
                         long out_len_max, int normalize, float *out, float *peaks, bas_stream_t stream);

/* ---- batched streams (no reference counterpart) ----------------------------------------------------
 * G independent streams (sessions) of n_src sources advance by one block of B samples in ONE render.  Session g's window
 * [halo | block] (halo = L-1 rounded up to chunks, as for bas_stream_epilogue_f32) starts at g W of every source row,
 * W = halo + B + K: one zero chunk follows each window, T_in = G W - K.  The chunk crossfade (apply_hrtf.py:431-442)
 * mixes the IRs of a chunk's two boundaries, so a window's first boundary cannot be the previous window's last one: the
 * gap chunk's boundaries are both, and its input is zero.  The FIR needs no gap (an emitted sample, at >= halo >= L-1
 * into its window, reads only inputs of that window: apply_hrtf.py:444-453).  Angle rows: nh + nb boundaries per session
 * (nh = halo / K, nb = B / K + 1), session g's from g (nh + nb); T_in / K + 1 = G (nh + nb).  K divides B and halo;
 * x_stride >= T_in, ang_stride >= G (nh + nb); G <= 65535 (one row of workgroups per session); B <= BAS_MAX_T_IN.
 *
 * bas_stream_batch_pack_f32: blocks [G][n_src][B] float32 -> x[s][g W + halo + j]; elev/azim [G][n_src][nb] float64 (the
 *   block's boundaries t0, t0 + K, .., t0 + B: :429, :435) -> elev_out/azim_out[s][g (nh + nb) + nh + c].  The halo
 *   columns, the halo angles and the gaps are not written.  One launch; 16-byte accesses where the rows are aligned.
 * bas_stream_batch_epilogue_f32: after the window render into y [2] rows of y_stride >= T_in floats, per session g what
 *   bas_stream_epilogue_f32 does for one stream, on session g's offset pointers: peaks[g] = max(peaks[g], max|y[e][g W +
 *   halo .. g W + halo + B)|) over both ears (:462 over the emitted samples; atomicMax on the bits of non-negative floats:
 *   exact, order-free); the input halo, the halo's boundaries and the angles at the block's end (last [G][2][n_src]) move
 *   as for one stream.  One launch.
 * bas_stream_batch_pack_head_f32: bas_stream_batch_pack_f32 with world-frame elev/azim and head [G][nb][4] (dense; session
 *   g's orientation (w, x, y, z) at each of the block's boundaries, see "head tracking" below): the angle slots receive
 *   the head-relative angles bas_head_relative_f64 computes, bit for bit.  Same checks, same launch count (one). */
int bas_stream_batch_pack_f32(const float *blocks, const double *elev, const double *azim, int n_sessions, int n_src,
                              long B, int K, int halo, float *x, long x_stride, double *elev_out, double *azim_out,
                              long ang_stride, bas_stream_t stream);
int bas_stream_batch_pack_head_f32(const float *blocks, const double *elev, const double *azim, const double *head,
                                   int n_sessions, int n_src, long B, int K, int halo, float *x, long x_stride,
                                   double *elev_out, double *azim_out, long ang_stride, bas_stream_t stream);
int bas_stream_batch_epilogue_f32(float *x, long x_stride, int n_sessions, int n_src, int halo, long B, int K,
                                  double *elev, double *azim, long ang_stride, double *last, const float *y,
                                  long y_stride, float *peaks, bas_stream_t stream);

/* ---- head tracking (no reference counterpart) -------------------------------------------------------
 * Sources given in the world frame, the listener's head orientation per chunk boundary.  Directions follow the
 * reference's convention (sphere.py:51-56): d = (-sin az cos el, cos az cos el, sin el), +y front, +z up, +x right.
 * head = unit quaternion (w, x, y, z), float64 (any non-zero norm: it is normalised), rotating head coordinates into
 * world ones: d_world = R(q) d_head, so d_head = R(q)^T d_world.  q is negated first when w < 0.  A pure yaw (x == y == 0
 * after that) keeps the elevation bit for bit and gives az - 2 atan2(z, w) (az itself when z == 0: the identity changes
 * neither angle); otherwise el_h = atan2(z_h, hypot(x_h, y_h)), az_h = atan2(-x_h, y_h), not wrapped.  Nothing is
 * validated on the device: a non-finite head gives non-finite angles, a zero quaternion the identity.
 *
 * bas_head_relative_f64: elev/azim [G][n_src][nb] at elev[g in_stride_g + s in_stride_s + c] (world frame), head [G][nb][4]
 *   at head[g head_stride_g + c head_stride_c + k] -> elev_out/azim_out[g out_stride_g + s out_stride_s + c] (head
 *   relative).  The output strides must address every element once (BAS_E_SHAPE otherwise), head_stride_c >= 4, all
 *   strides >= 0, all pointers 8-byte aligned (BAS_E_ALIGN).  In place: elev_out == elev and azim_out == azim with the
 *   input strides on the output.  One launch. */
int bas_head_relative_f64(const double *elev, const double *azim, long in_stride_g, long in_stride_s, const double *head,
                          long head_stride_g, long head_stride_c, int n_groups, int n_src, int nb, double *elev_out,
                          double *azim_out, long out_stride_g, long out_stride_s, bas_stream_t stream);

/* ---- per-source gain at chunk boundaries (no reference counterpart) -------------------------------
 * gain [..] f64 (device) holds one value per chunk boundary, laid out exactly as the angles of the same call (one per
 * query: source s at boundary k sits where elev[s][k] / azim[s][k] sit).  The chunk IR at a boundary becomes
 * g_k interpolate_2d(el_k, az_k); the reference's subchunk crossfade (apply_hrtf.py:435, :443) then runs unchanged between
 * g_k H_k and g_{k+1} H_{k+1}.  Any finite real gain is allowed (negative: polarity inverted, zero: silence); nothing is
 * validated on the device.  The peak rules (make_signal_move_2d's :462-464, the batch's per item, the streams' running
 * peaks) see the gained output.  Every entry point below is its gain-less namesake with the gain added (a required
 * pointer: BAS_E_NULL when it is NULL and there is work); the namesakes are these calls with no gain and keep their code.
 *   plans (bas_interp2d_plan_gain_f32, _plan_angles_gain_f32): every one of the 16 folded weights is multiplied by
 *     gain[q] in binary64 and rounded to binary32 once, so the fused FIR kernels gain it without a change;
 *   bas_interp2d_gain_f32: the stored chunk IRs H[q] = gain[q] interpolate_2d(q) (planned tables as above; U < 4 tables
 *     scale every tap by gain[q] in binary64, rounded once);
 *   carried stream state (bas_render_stream_block_gain_f32, bas_stream_epilogue_gain_f32, bas_stream_batch_epilogue_gain_f32):
 *     gain rows at the angles' stride move as the angles do, gain_last [n_src] (one stream) / [G][n_src] (batched
 *     streams) receives the gain at the block's end, as last[] receives the angles;
 *   bas_stream_batch_pack_gain_f32: gain [G][n_src][nb] -> gain_out's slots beside the angles, in the same launch; head
 *     may be NULL (head-relative angles) or as for bas_stream_batch_pack_head_f32;
 *   bas_batch_pack_gain_f32: gain [B][n_src][n_q_max] -> gain_out [n_src][T_in/K + 1] as the angles (the gap's inner
 *     boundaries repeat the item's last gain). */
int bas_interp2d_plan_gain_f32(const double *diffs, const int32_t *idx, const double *w, const double *gain, int n,
                               int ndir, int L, int U, void *plans, size_t plans_bytes, bas_stream_t stream);
int bas_interp2d_plan_angles_gain_f32(const double *diffs, const double *elev, const double *azim, const double *gain,
                                      int n, const double *ring_elev, const int32_t *ring_start,
                                      const int32_t *ring_count, const float *node_az, int branch, int ndir, int L,
                                      int U, void *plans, size_t plans_bytes, bas_stream_t stream);
int bas_interp2d_gain_f32(const float *packed, const double *diffs, const int32_t *idx, const double *w,
                          const double *gain, int n, int ndir, int L, int U, float *H, void *ws, size_t ws_bytes,
                          bas_stream_t stream);
int bas_render_stream_block_gain_f32(float *x, long x_stride, const float *packed, const void *plans, int n_src,
                                     long T_in, int K, int S, int L, int U, int ndir, float *y, void *ws,
                                     size_t ws_bytes, int halo, double *elev, double *azim, double *gain,
                                     long ang_stride, int nh, int nb, double *last, double *gain_last,
                                     float *running_peak, bas_stream_t stream);
int bas_stream_epilogue_gain_f32(float *x, long x_stride, int n_src, int halo, long B, double *elev, double *azim,
                                 double *gain, long ang_stride, int nh, int nb, double *last, double *gain_last,
                                 const float *y, long y_stride, float *running_peak, bas_stream_t stream);
int bas_stream_batch_pack_gain_f32(const float *blocks, const double *elev, const double *azim, const double *head,
                                   const double *gain, int n_sessions, int n_src, long B, int K, int halo, float *x,
                                   long x_stride, double *elev_out, double *azim_out, double *gain_out,
                                   long ang_stride, bas_stream_t stream);
int bas_stream_batch_epilogue_gain_f32(float *x, long x_stride, int n_sessions, int n_src, int halo, long B, int K,
                                       double *elev, double *azim, double *gain, long ang_stride, double *last,
                                       double *gain_last, const float *y, long y_stride, float *peaks,
                                       bas_stream_t stream);
int bas_batch_pack_gain_f32(const float *sig, int n_items, int n_src, long N, const long *lengths, const long *offsets,
                            const double *elev, const double *azim, const double *gain, long n_q_max, int K,
                            long T_in, float *x, long x_stride, double *elev_out, double *azim_out, double *gain_out,
                            bas_stream_t stream);

/* ---- per-source propagation delay (no reference counterpart) --------------------------------------
 * delay [..] f64 (device), in SAMPLES, one value per chunk boundary laid out as the angles of the same call.  A source's
 * delayed input x' replaces its input x; everything after that (chunk IRs, crossfade, FIR, mix, peak rules) is unchanged.
 * For t = kK + j, 0 <= j < K:  d = d_k + (j / K)(d_{k+1} - d_k), clamped to [d_min, d_max] with fmax(fmin(.)) (a NaN
 * reads as d_max);  u = j - d,  n = floor(u),  f = u - n,  i = kK + n  (binary64, relative to the chunk start: the bits do
 * not depend on the absolute time);  x'(t) = sum_m c_m(f) x(i + m) in binary64, rounded to binary32 once:
 *   interp 1 (cubic): m = -1..2, 4-point Lagrange in product form, c_-1 = -f(f-1)(f-2)/6, c_0 = (f+1)(f-1)(f-2)/2,
 *     c_1 = -(f+1)f(f-2)/2, c_2 = (f+1)f(f-1)/6 (f = 0: exactly (0, 1, 0, 0)); d_min = 2;
 *   interp 0 (linear): m = 0..1, (1 - f, f) (apply_hrtf.py:178-199's fractional delay, per sample); d_min = 1.
 * Neither reads a sample later than t.  Samples outside the readable range are 0.  Nothing is validated on the device.
 *   bas_delay_rows_f32: rows (g, s), g < n_groups, s < n_src: input x + g x_stride_g + s x_stride_s (sample 0; samples
 *     -H .. -1 in front are readable history, H may be 0), delay + g d_stride_g + s d_stride_s ((T-1)/K + 2 boundaries),
 *     output y + g y_stride_g + s y_stride_s, T samples (16-byte stores where the output row is 16-byte aligned).
 *     lengths [n_groups n_src] (NULL: T each): the row's valid samples; reads at or past it are 0, and so are the
 *     outputs.  max_delay: the upper clamp, which must leave the reads inside the history (d_min <= max_delay <= H - 2),
 *     or 0 offline: the row's valid length + 4 (no output changes: every read past it lands before sample 0).  One launch;
 *     T < 2^30, n_groups n_src <= 65535.  y must not overlap x's readable range.
 *   bas_delay_carry_f32: the raw history of a stream block: row[0 .. H) = row[B .. B + H) for every (g, s) row (row =
 *     x + g x_stride_g + s x_stride_s at the history's start), B < H (overlapping) included.  One launch; n_groups n_src
 *     < 2^31 (one workgroup per row).
 *   bas_batch_pack_delay_f32: bas_batch_pack_gain_f32 (gain NULL: bas_batch_pack_f32) with item b's DELAYED input in its
 *     segment: delay [B][n_src][n_q_max] is read where it is (no packed delay array), item b's reads are bounded by its
 *     own valid length (the offline rule above), the gaps stay zeros.  Still one launch.
 *   bas_stream_batch_pack_delay_f32: bas_stream_batch_pack_gain_f32 (gain NULL: no gain, gain_out ignored; head NULL:
 *     head-relative angles) with session g's DELAYED block in its window slots [halo, halo + B): raw + g raw_stride_g +
 *     s raw_stride_s holds the H carried raw samples of (g, s) (raw_stride_s >= H + B); the delayed samples read them
 *     and the dense block (the same bits as bas_delay_rows_f32 on [history | block]), with delay [G][n_src][nb] clamped
 *     to [d_min, max_delay] (d_min <= max_delay <= H - 2), and the raw block is copied behind the history, where
 *     bas_delay_carry_f32 moves the last H raw samples to the front after the block.  Still one launch. */
int bas_delay_rows_f32(const float *x, long x_stride_g, long x_stride_s, int H, const long *lengths, const double *delay,
                       long d_stride_g, long d_stride_s, int n_groups, int n_src, long T, int K, int interp,
                       double max_delay, float *y, long y_stride_g, long y_stride_s, bas_stream_t stream);
int bas_delay_carry_f32(float *x, long x_stride_g, long x_stride_s, int n_groups, int n_src, int H, long B,
                        bas_stream_t stream);
int bas_stream_batch_pack_delay_f32(const float *blocks, const double *elev, const double *azim, const double *head,
                                    const double *gain, const double *delay, int interp, double max_delay, float *raw,
                                    long raw_stride_g, long raw_stride_s, int H, int n_sessions, int n_src, long B, int K,
                                    int halo, float *x, long x_stride, double *elev_out, double *azim_out,
                                    double *gain_out, long ang_stride, bas_stream_t stream);
int bas_batch_pack_delay_f32(const float *sig, int n_items, int n_src, long N, const long *lengths, const long *offsets,
                             const double *elev, const double *azim, const double *gain, const double *delay, int interp,
                             long n_q_max, int K, long T_in, float *x, long x_stride, double *elev_out, double *azim_out,
                             double *gain_out, bas_stream_t stream);

/* ---- per-source colour (no reference counterpart) ----------------------------------------------------
 * color [..] f32 (device): M coefficients (1 <= M <= 64) of a short FIR per source row and chunk boundary, boundaries laid
 * out in time as the angles, gains and delays of the same call.  A source's coloured input x'' replaces its (delayed) input
 * x'; everything after that (chunk IRs, crossfade, FIR, mix, gains, peak rules) is unchanged.  For t = kK + j, 0 <= j < K:
 *   A = sum_{m < M} c_k[m] x'(t - m),  B = sum_{m < M} c_{k+1}[m] x'(t - m),  x''(t) = A + (j / K)(B - A).
 * Precision: A and B are accumulated in binary32 by fused multiply-adds, acc = fma(c[m], x'(t - m), acc) from acc = 0 with
 * m ascending (M is padded to a multiple of 4 with zero taps, which add exact zeros); w = (float)j * (1.0f / (float)K);
 * x'' = A if A == B, else fma(w, B, fma(-w, A, A)).  The bits of an output depend on (j, K, c_k, c_{k+1}) and its M inputs alone - not on the absolute
 * time nor on where a tile starts - so a stream's coloured block is the offline one bit for bit; (1, 0, .., 0) returns its
 * input bit for bit; B == A returns A.  Samples outside the readable range are 0.  Nothing is validated on the device.
 *   bas_color_rows_f32: rows (g, s), g < n_groups, s < n_src: input x + g x_stride_g + s x_stride_s (sample 0; samples
 *     -Hc .. -1 in front are readable, Hc may be 0: the missing samples are zeros; an input stride of 0 repeats a signal),
 *     coefficients at color + g c_stride_g + s c_stride_s + k c_stride_k, M contiguous floats for each of the (T-1)/K + 2
 *     boundaries k; any coefficient stride may be 0: c_stride_k == 0 is the static form (one set per row, B is skipped: the
 *     bits of the per-boundary form fed repeated sets), c_stride_g == 0 shares one bank over the groups; otherwise
 *     c_stride_k >= M.  Output y + g y_stride_g + s y_stride_s, T samples (16-byte loads and stores where a row is
 *     16-byte aligned).  lengths [n_groups n_src] (NULL: T each): the row's valid samples; reads at or past it are 0, and
 *     so are the outputs.  One launch, no allocation, no synchronisation (capturable); T < 2^30, n_groups n_src <= 65535,
 *     strides >= 0, K > 0 (BAS_E_SHAPE); x, color, y required (BAS_E_NULL) and 4-byte aligned, lengths 8-byte
 *     (BAS_E_ALIGN).  y must not overlap x's readable range. */
int bas_color_rows_f32(const float *x, long x_stride_g, long x_stride_s, int Hc, const long *lengths, const float *color,
                       long c_stride_g, long c_stride_s, long c_stride_k, int M, int n_groups, int n_src, long T, int K,
                       float *y, long y_stride_g, long y_stride_s, bas_stream_t stream);

/* ---- Cartesian scenes (no reference counterpart) -----------------------------------------------------
 * Source positions, the listener's pose and an optional axis-aligned shoebox room -> the angles, gains and delays of every
 * image source at every chunk boundary: what the three sections above consume.  All float64 on the device unless stated,
 * all strides in elements and >= 0 (0 repeats), metres in the world frame (+y front, +z up, +x right: sphere.py:51-56).
 *   pos [G][n_src][nb][3] at pos[g pos_stride_g + s pos_stride_s + c pos_stride_c + k];
 *   lpos [G][nb][3] at lpos[g lpos_stride_g + c lpos_stride_c + k]: the listener's position; NULL: the origin;
 *   head [G][nb][4] at head[g head_stride_g + c head_stride_c + k]: (w, x, y, z) as in "head tracking" (rotates head into
 *     world coordinates, any non-zero norm, normalised here); NULL: the identity;
 *   src_gain [G][n_src][nb] at src_gain[g sg_stride_g + s sg_stride_s + c]: a multiplier (volume, fades); NULL: 1;
 *   room_size [3] (metres; the room occupies [0, L_a] on axis a), images int32 [n_img][3], img_gain [n_img].
 *     room_size NULL: free field, n_img must be 1 (the one image is the source itself; images, img_gain are not read).
 * For group g, source s, image i, boundary c, in binary64 without contraction, in this order:
 *   1. q_a = m L_a + (m even ? p_a : L_a - p_a) for m = images[i][a] (m = 0: the source; 1: mirrored at the wall a = L_a;
 *      -1: at the wall a = 0); free field: q = p;
 *   1b. (samples_per_chunk > 0 only) a moving source is heard where it was when the sound left it.  The image's velocity
 *      per sample is u = (q(b) - q(a)) / samples_per_chunk for the source's positions (a, b) = (c - 1, c); at c = 0,
 *      (pos_prev, 0) when pos_prev [G][n_src][3] (at [g prev_stride_g + s prev_stride_s + k]: the boundary before this
 *      call's first, a stream's carry) is given, else (0, 1), else (nb == 1) u = 0.  With w = q - listener and
 *      A = 1 / samples_per_metre^2 - |u|^2 > 0 (subsonic; otherwise no correction), the time of flight in samples is
 *      d = (sqrt((w.u)^2 + A |w|^2) - w.u) / A, the root of |w - u d| = d / samples_per_metre, and q becomes q - u d.
 *      A source at rest keeps q bit for bit.  samples_per_chunk == 0: no correction (the distance at reception);
 *   2. v = q - listener;  r = sqrt(vx^2 + vy^2 + vz^2);
 *   3. v_h = R(head / |head|)^T v (the matrix of "head tracking"; skipped when head is NULL);
 *   4. el = atan2(v_hz, hypot(v_hx, v_hy)),  az = atan2(-v_hx, v_hy), not wrapped;  v == 0 exactly: el = az = 0;
 *   5. gain = src_gain img_gain[i] r_ref / fmax(r, r_ref);
 *   6. delay = fmax(fmin(r samples_per_metre, d_max), d_min)   (samples; samples_per_metre = fs / c).
 * Outputs, row = s n_img + i: elev, azim, gain at [g a_stride_g + row a_stride_s + c], delay at [g d_stride_g +
 * row d_stride_s + c]; gain and delay may each be NULL (not written).  Each output layout must address every element once
 * and the outputs must be distinct buffers (BAS_E_SHAPE); samples_per_chunk finite and >= 0, > 0 with pos_prev; n_groups, n_src, nb, n_img > 0, samples_per_metre and r_ref
 * finite and > 0, 0 <= d_min <= d_max (d_max may be +inf) (BAS_E_SHAPE); pos, elev, azim and, with a room, images and
 * img_gain are required (BAS_E_NULL); float64 pointers 8-byte aligned, images 4-byte (BAS_E_ALIGN).  Nothing is validated
 * on the device.  One launch. */
int bas_scene_params_f64(const double *pos, long pos_stride_g, long pos_stride_s, long pos_stride_c,
                         const double *pos_prev, long prev_stride_g, long prev_stride_s, double samples_per_chunk,
                         const double *lpos, long lpos_stride_g, long lpos_stride_c, const double *head, long head_stride_g,
                         long head_stride_c, const double *src_gain, long sg_stride_g, long sg_stride_s,
                         const double *room_size, const int32_t *images, const double *img_gain, int n_img,
                         double samples_per_metre, double r_ref, double d_min, double d_max, int n_groups, int n_src,
                         int nb, double *elev, double *azim, double *gain, long a_stride_g, long a_stride_s,
                         double *delay, long d_stride_g, long d_stride_s, bas_stream_t stream);

/* ---- scene colour: air absorption and source directivity (no reference counterpart) -------------------
 * Per (row, boundary) of a Cartesian scene, the natural log-magnitude in each of n_bands frequency bands of what the
 * path does to the sound - the walls the image met, the air it crossed, the source's pattern towards the listener - and,
 * from such log-magnitudes, the taps of a minimum-phase FIR per (row, boundary), laid out as "per-source colour" reads them.
 *   bas_scene_params_bands_f64: bas_scene_params_f64 (same arguments, same four outputs bit for bit, same checks) plus
 *     orient [G][n_src][nb][4] at orient[g orient_stride_g + s orient_stride_s + c orient_stride_c + k]: (w, x, y, z)
 *       turning the source's frame into the world frame, any non-zero norm, normalised here; NULL: the identity.  A source
 *       radiates along its local +y: f = R(orient) (0, 1, 0) = (2(xy - wz), 1 - 2(x^2 + z^2), 2(yz + wx));
 *     pattern [n_src][n_bands] at pattern[s pattern_stride_s + b]: first-order coefficients a in [0, 1] (1 omni, 0.5
 *       cardioid, 0 figure-of-eight); pattern_stride_s 0 shares one row over the sources, else >= n_bands; NULL: omni;
 *     air [n_bands]: absorption in nepers per metre (dB per metre times ln 10 / 20), >= 0; NULL: none;
 *     img_logmag [n_img][n_bands]: ln of the images' wall magnitudes (floored by the caller); NULL: 0;
 *     n_bands in 1..16; floor in (0, 1]: the magnitude below which the pattern term and the sum are floored.
 *   With q the image's position of steps 1-1b, v = q - listener and r of step 2 (unclamped), in binary64 without
 *   contraction: f_a is negated where images[i][a] is odd (the mirror turns the source);
 *     cos = -(fx vx + fy vy + fz vz) / r  (r == 0: 1);   D_b = |a_b + (1 - a_b) cos|;
 *     L[b] = fmax(((img_logmag[i][b] - air[b] r) + log(fmax(D_b, floor))), log(floor))
 *   (a NULL term is skipped), written at logmag[g l_stride_g + row l_stride_s + c l_stride_c + b], row = s n_img + i.
 *   l_stride_c >= n_bands and [G][rows][(nb - 1) l_stride_c + n_bands] with strides (l_stride_g, l_stride_s, 1) must
 *   address no element twice; logmag distinct from the other outputs; input strides >= 0 (BAS_E_SHAPE); logmag required
 *   (BAS_E_NULL); the new float64 pointers 8-byte aligned (BAS_E_ALIGN).  Still one launch, capturable.
 *   bas_color_design_f32: logmag float64 at logmag[g l_stride_g + s l_stride_s + k l_stride_k + b] (strides in 0..2^40,
 *     0 repeats), g < n_groups, s < n_src, k < nb; basis float64 [n_bands][M] (device): row b holds the first M folded
 *     cepstrum coefficients of band b's interpolation weight (propagation.cepstral_basis).  Per filter, in binary64:
 *       L[b] = fmax(logmag[b], logmag_floor);  c[m] = sum_b L[b] basis[b][m]  (fma from 0, b ascending);
 *       h[0] = exp(c[0]);  h[n] = (sum_{k=1..n} (k c[k]) h[n - k]) / n  (fma from 0, k ascending),  1 <= n < M;
 *     the first M taps of the minimum-phase response whose log-magnitude has those band values.  Output: (float)h[m] at
 *     color[g c_stride_g + s c_stride_s + k c_stride_k + m], M contiguous floats.  A filter's bits depend on its n_bands
 *     inputs, the basis and the floor alone, not on the grid nor on its place in it.  M in 1..64, n_bands in 1..16,
 *     logmag_floor finite and <= 0, n_groups n_src nb < 2^40, c_stride_k >= M and [G][n_src][(nb - 1) c_stride_k + M] with
 *     strides (c_stride_g, c_stride_s, 1) must address no element twice (BAS_E_SHAPE; a StreamRenderer's color_view(B)
 *     passes); any count 0: nothing to do; logmag, basis, color required (BAS_E_NULL), 8-, 8- and 4-byte aligned
 *     (BAS_E_ALIGN).  color must not overlap logmag or basis.  One launch, no allocation, no synchronisation
 *     (capturable once the first call on a device has been made).  Nothing is validated on the device. */
int bas_scene_params_bands_f64(const double *pos, long pos_stride_g, long pos_stride_s, long pos_stride_c,
                               const double *pos_prev, long prev_stride_g, long prev_stride_s, double samples_per_chunk,
                               const double *lpos, long lpos_stride_g, long lpos_stride_c, const double *head,
                               long head_stride_g, long head_stride_c, const double *src_gain, long sg_stride_g,
                               long sg_stride_s, const double *room_size, const int32_t *images, const double *img_gain,
                               int n_img, double samples_per_metre, double r_ref, double d_min, double d_max, int n_groups,
                               int n_src, int nb, const double *orient, long orient_stride_g, long orient_stride_s,
                               long orient_stride_c, const double *pattern, long pattern_stride_s, const double *air,
                               const double *img_logmag, int n_bands, double floor, double *elev, double *azim,
                               double *gain, long a_stride_g, long a_stride_s, double *delay, long d_stride_g,
                               long d_stride_s, double *logmag, long l_stride_g, long l_stride_s, long l_stride_c,
                               bas_stream_t stream);
int bas_color_design_f32(const double *logmag, long l_stride_g, long l_stride_s, long l_stride_k, const double *basis,
                         int n_bands, int M, double logmag_floor, int n_groups, int n_src, int nb, float *color,
                         long c_stride_g, long c_stride_s, long c_stride_k, bas_stream_t stream);

/* ---- screens: occlusion and edge diffraction (no reference counterpart) ------------------------------
 * Static thin rectangles between the image sources and the listener, as one more term of "scene colour"'s L[b].
 *   bas_scene_params_occluded_f64: bas_scene_params_bands_f64 (same arguments, same checks, the four outputs bit for bit)
 *   plus
 *     screens [n_screens][9]: centre c, half-edge vectors e1, e2 (metres, world frame; e1, e2 non-zero and orthogonal: the
 *       caller's to check), n_screens in 1..32;
 *     transmission [n_screens][n_bands] at transmission[k transmission_stride_s + b]: magnitudes T in [0, 1];
 *       transmission_stride_s 0 shares one row over the screens, else >= n_bands; NULL: opaque (T = 0);
 *     fresnel [n_bands]: 2 f_b / c per band centre f_b (1/metres).
 *   For the straight path from q (the image's position of steps 1-1b) to the listener l and one screen copy, in binary64
 *   without contraction (bas_occlude.h holds the expressions and their order):
 *     n = e1 x e2, s_q = n.(q - c), s_l = n.(l - c); unless s_q s_l < 0 the copy contributes exactly 0 to every band;
 *     h = q + (s_q / (s_q - s_l)) (l - q), a = (h - c).e1 / |e1|^2, b = (h - c).e2 / |e2|^2, blocked: |a| <= 1 and |b| <= 1;
 *     delta = max(min over the four edges A-B of [min over P in AB of |q - P| + |P - l|] - |q - l|, 0)   (closed form);
 *     N_b = +- fresnel[b] delta (+ blocked, - lit), x = sqrt(2 pi |N_b|),
 *     A = min(5 + 20 log10(x / tanh x), 24) for N >= 0, max(5 + 20 log10(x / tan x), 0) for -0.2 < N < 0, else 0 (dB);
 *     M_b = T_b + (1 - T_b) exp(-A ln 10 / 20).
 *   With a room, image m = images[i] meets the copies of every screen in the cells (i, j, k), each index between 0 and
 *   m_a inclusive: c'_a = i_a L_a + (i_a odd ? L_a - c_a : c_a), component a of e1, e2 negated where i_a is odd.  The sum
 *   of ln M_b over screens (ascending) and cells (x outermost, each index from 0 towards m_a), from 0, is added to the
 *   sum of "scene colour" before its final fmax(., log(floor)).  n_screens out of range, a transmission stride in
 *   (0, n_bands) or negative (BAS_E_SHAPE); screens, fresnel required (BAS_E_NULL); the new pointers 8-byte aligned
 *   (BAS_E_ALIGN).  room_size may be NULL (screens in the free field: one copy each).  Still one launch, capturable. */
int bas_scene_params_occluded_f64(const double *pos, long pos_stride_g, long pos_stride_s, long pos_stride_c,
                                  const double *pos_prev, long prev_stride_g, long prev_stride_s, double samples_per_chunk,
                                  const double *lpos, long lpos_stride_g, long lpos_stride_c, const double *head,
                                  long head_stride_g, long head_stride_c, const double *src_gain, long sg_stride_g,
                                  long sg_stride_s, const double *room_size, const int32_t *images, const double *img_gain,
                                  int n_img, double samples_per_metre, double r_ref, double d_min, double d_max,
                                  int n_groups, int n_src, int nb, const double *orient, long orient_stride_g,
                                  long orient_stride_s, long orient_stride_c, const double *pattern, long pattern_stride_s,
                                  const double *air, const double *img_logmag, int n_bands, double floor,
                                  const double *screens, const double *transmission, long transmission_stride_s,
                                  const double *fresnel, int n_screens, double *elev, double *azim, double *gain,
                                  long a_stride_g, long a_stride_s, double *delay, long d_stride_g, long d_stride_s,
                                  double *logmag, long l_stride_g, long l_stride_s, long l_stride_c, bas_stream_t stream);

/* ---- late reverberation (no reference counterpart) ---------------------------------------------------
 * One send bus per group - a weighted mono mix of the group's source rows - through one long static stereo tail, added to
 * the binaural mix.  All entries: one stream, no allocation, no synchronisation (capturable); every argument check runs
 * before any launch.
 *   bas_bus_mix_f32: bus[g][t] = sum_s w_s(t) x_{g,s}(t), t < T, for the rows x + g x_stride_g + s x_stride_s and the
 *     weights send + g s_stride_g + s s_stride_s + k s_stride_k (float64, one per chunk boundary k <= (T-1)/K + 1):
 *     for t = kK + j, w_s(t) = g_k + (j / K)(g_{k+1} - g_k), formed in binary64 without contraction (j / K one division)
 *     and rounded ONCE to binary32; acc = fmaf(w, x, acc) from acc = +0 with s ascending.  s_stride_k == 0 is the static
 *     form, w = (float)g_0: the bits of the per-boundary form fed repeated weights.  The bits do not depend on tiling.
 *     Output bus + g bus_stride.  16-byte loads and stores where a row is 16-byte aligned.  One launch.  T < 2^30,
 *     n_groups <= 65535, strides >= 0, bus_stride >= T with more than one group, K > 0 (BAS_E_SHAPE); x, send, bus
 *     required (BAS_E_NULL); x, bus 4-byte aligned, send 8-byte (BAS_E_ALIGN).
 *   bas_long_fir_tail_floats / bas_long_fir_tail_f32: h [2][Lr] (ear e at h + e h_stride) -> `tail`, an opaque array of
 *     bas_long_fir_tail_floats(Lr, Np) floats (0 for sizes out of range), 16-byte aligned: the twiddle table of the
 *     transforms of size 2 Np (binary32 roundings of binary64 sincospi values) and the spectra of the P = ceil(Lr / Np)
 *     partitions [h_p | Np zeros] under a DFT of size 2 Np, bins 0 .. Np.  Once per tail and Np.  One launch.
 *   bas_long_fir_workspace_bytes / bas_long_fir_f32: r[g][e][n] = sum_{k < Lr} h[e][k] b_g(n - lag - k), n < T_out, by
 *     uniformly partitioned overlap-save.  Bus g is bus + g bus_stride: samples [-Hb, T_bus) are readable (Hb: a stream's
 *     carried history, may be 0), everything else reads as zero.  Output frame f covers outputs [f Np, (f + 1) Np); X_f is
 *     the DFT of size 2 Np of b[(f - 1) Np - lag, (f + 1) Np - lag) (lag only shifts the window: exact, free);
 *     Y_e[k] = sum_{p < P} X_{f - p}[k] H_{e,p}[k], accumulated by ONE thread per bin from +0 with p ascending, the four
 *     fused multiply-adds of a complex product in a fixed order; both ears go through one complex inverse transform, whose
 *     second half is r.  out[g][e][n] = y_in[g][e][n] + r (one binary32 add; y_in is zero at n >= T_y; NULL: zero
 *     everywhere; out may be y_in with the same strides: in place) at out + g out_stride_g + e out_stride_e + n;
 *     peak[g] = max(peak[g], max|out|) (float; an atomic max on the bits of non-negative floats, as
 *     bas_batch_finish_f32 takes it; NULL: not taken).  An output's bits depend on the bus, h, lag and Np only - not on
 *     T_out or T_bus, not on how frames and bins are dealt to workgroups, not on whether the call is a whole signal or a
 *     stream block with its history in front.  A zero bus or a zero h adds +0.  Three launches (frame spectra, the sums
 *     over partitions, inverse + add + peak).  ws: bas_long_fir_workspace_bytes(n_bus, T_out, Lr, Np) bytes, 16-byte
 *     aligned, uninitialised (BAS_E_WORKSPACE when smaller).  Np in {32, 64, 128, 256, 512}, 1 <= Lr <= 2^17,
 *     0 <= lag <= 2^20, T_bus, T_out, T_y, Hb < 2^30, n_bus <= 65535, strides >= 0, out_stride_e >= T_out and, with more
 *     than one bus, out_stride_g >= out_stride_e + T_out (BAS_E_SHAPE); tail, out, ws and (with anything to read) bus
 *     required (BAS_E_NULL); bus, y_in, out, peak 4-byte aligned, tail and ws 16-byte (BAS_E_ALIGN). */
int bas_bus_mix_f32(const float *x, long x_stride_g, long x_stride_s, const double *send, long s_stride_g,
                    long s_stride_s, long s_stride_k, int n_groups, int n_src, long T, int K, float *bus, long bus_stride,
                    bas_stream_t stream);
size_t bas_long_fir_tail_floats(int Lr, int Np);
int bas_long_fir_tail_f32(const float *h, long h_stride, int Lr, int Np, float *tail, bas_stream_t stream);
size_t bas_long_fir_workspace_bytes(int n_bus, long T_out, int Lr, int Np);
int bas_long_fir_f32(const float *bus, long bus_stride, long Hb, long T_bus, int n_bus, const float *tail, int Lr, int Np,
                     int lag, const float *y_in, long y_stride_g, long y_stride_e, long T_y, float *out, long out_stride_g,
                     long out_stride_e, long T_out, float *peak, void *ws, size_t ws_bytes, bas_stream_t stream);

/* ---- look-ahead limiter -----------------------------------------------------------------------------
 * The reference ends a render with its peak rule (apply_hrtf.py:462-464: if max|y| > 1, divide the whole signal by it).  A
 * stream cannot apply that rule - the maximum is known when the stream is over - so the streamed paths hand out raw sums.
 * This stage makes them safe to play: a peak limiter with look-ahead, ONE gain for both ears (the interaural level
 * difference is kept), no recursion.  For a ceiling c > 0 (a normal binary32 value, carried in a double), a look-ahead of
 * A samples and a hold of Hd samples, with zeros before the start and after the end of a signal:
 *   1. m[n] = max(|yL[n]|, |yR[n]|);
 *   2. r[n] = m[n] > c ? c / m[n] : 1                          (one binary32 division);
 *   3. e[k] = min r[j] over j in [k - Hd, k + A]               (exact);
 *   4. s[n] = (e[n - A] + ... + e[n]) / (A + 1): binary64 adds from +0 with k ascending, one binary64 division, rounded
 *      ONCE to binary32;
 *   5. g[n] = min(s[n], r[n]);
 *   6. out[n] = min(max(y[n] g[n], -c), c) per ear             (one binary32 multiplication; the sign is kept).
 * The gain falls linearly over the A samples before a peak, meets the required gain at the peak, stays for Hd samples and
 * returns linearly over A samples; |out| <= c always; a signal whose peak is at most c keeps its bits.  The bits are
 * specified for |y| <= 2^20 c (no r subnormal).
 * Non-finite inputs: for ANY input bits every output is finite and |out| <= c.  In step 1 a NaN in
 * either ear makes m NaN (the maximum is taken on the bit patterns: bas_peak_max), so step 2 gives r = 1, as for a zeroed
 * frame; an infinite sample gives r = 0.  A non-finite product in step 6 leaves as -c (min(max(NaN, -c), c)): what the bad
 * frame itself becomes is not part of the contract.  The other outputs of the session are those of limit_f32_ref
 * (limiter.py) on the same input; they are the bits of the run with that frame zeroed once 2 A + Hd samples have passed
 * it.  No other session's outputs, meters or state change.
 *   y at y + g y_stride_g + t y_stride_t + e y_stride_e, out likewise: any strides >= 0 (the stream renderers' [B, 2]
 *   views of planar buffers, interleaved frames); the output's strides must address every element once, and input, output
 *   and state must not overlap (BAS_E_SHAPE: the limiter does not run in place).
 *   state == NULL: a whole signal.  T_in == T_out; out[n] belongs to y[n].
 *   state != NULL: a block of a stream.  state + g state_stride holds bas_limit_state_floats(A, Hd) floats per session
 *     (0 for parameters out of range), zeroed before a stream's first block: two ring positions and the session's last
 *     2 A + Hd input samples - samples only, r is recomputed.  out[j] is the limited sample of time t0 + j - A for a block
 *     that starts at t0: the stream is delayed by A samples and begins with A zeros.  T_in == T_out: a block, whose last
 *     min(T_in, 2 A + Hd) samples then go into the ring - by the session's own workgroup where the block is one tile (1024
 *     samples) or less, by a second launch where it is longer.  T_in == 0: the stream's end - T_out (usually A) more
 *     samples with zeros behind the history; the state is left as it is, y is not read.
 *     Any block length >= 1.  An output's bits depend on the samples at times [n - A - Hd, n + A] alone: not on the block
 *     boundaries, not on how samples are dealt to workgroups.
 *   reduction[g] = min(reduction[g], min g) over the outputs written (the gain-reduction meter; set to 1 by the caller
 *   before a stream), peak[g] = max(peak[g], max|out|): atomics on the bits of positive floats, sent only when they would
 *   change the value; each may be NULL.
 * One stream, no allocation, no synchronisation (capturable); one launch, two for a stream block of more than 1024 samples.
 * Every argument check runs before any launch: 0 <= lookahead <= 1024, 0 <= hold <= 4096, ceiling a normal binary32 value
 * > 0, n_sessions <= 65535, T_in, T_out < 2^30, strides >= 0, state_stride a multiple of 4 and >= the state's size
 * (BAS_E_SHAPE); out, and y with T_in > 0, required (BAS_E_NULL); y, out, reduction, peak 4-byte aligned, state 16-byte
 * (BAS_E_ALIGN). */
#define BAS_LIMIT_MAX_LOOKAHEAD 1024
#define BAS_LIMIT_MAX_HOLD 4096
size_t bas_limit_state_floats(int lookahead, int hold);
int bas_limit_f32(const float *y, long y_stride_g, long y_stride_t, long y_stride_e, float *out, long out_stride_g,
                  long out_stride_t, long out_stride_e, int n_sessions, long T_in, long T_out, double ceiling,
                  int lookahead, int hold, float *state, long state_stride, float *reduction, float *peak,
                  bas_stream_t stream);

/* ---- loudness meter (no reference counterpart) --------------------------------------------------------------
 * How loud a stereo signal is, after ITU-R BS.1770 / EBU R128: the energies of the K-weighted signal per hop of 100 ms, from
 * which the caller forms momentary, short-term and gated integrated loudness (loudness.py: readings), and the true peak, 4x
 * oversampled.  A stage of its own behind a render, a stream or the limiter; it writes no audio.
 *   K-weighting at fs (a multiple of 10 in 8000..192000; hop = fs / 10): two biquads per ear in binary64, transposed direct
 *   form II, from rest at a signal's first sample and never reset.  With K = tan(pi f0 / fs), a0 = 1 + K/Q + K^2:
 *     shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20),
 *                Vb = Vh^0.4996667741545416:  b = (Vh + Vb K/Q + K^2, 2 (K^2 - Vh), Vh - Vb K/Q + K^2) / a0,
 *                a1 = 2 (K^2 - 1) / a0, a2 = (1 - K/Q + K^2) / a0;
 *     high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773:  b = (1, -2, 1), a1 and a2 as above
 *   (at 48 kHz the coefficients tabulated in BS.1770-4).  E[g][ear][h] = sum of z^2 over samples h hop .. (h + 1) hop - 1 of
 *   the K-weighted signal z; a last partial hop is not counted.  The recursion is evaluated in parallel (runs from rest, a
 *   scan with powers of the transition matrix, the runs again), so an energy is the definition's within rounding - 1e-9
 *   relative is the tested bar - and the same call gives the same bits twice: fixed orders, no floating-point atomics.
 *   True peak: phase 0 is the samples; phases p = 1..3 at time m + p/4 are sum_j x[m + j] taps[(p - 1) 12 + j + 5],
 *   j = -5 .. 6: 36 binary32 taps in HOST memory, read before the launch.  The 12 products (exact in binary64) are added
 *   one by one from +0 with j ascending and rounded to binary32 once; then |.| and the maximum, per ear, over every m whose
 *   window touches the signal (zeros outside it).  Being a maximum it is exact whatever the order: bits do not depend on
 *   blocks.  It travels as the bits of a binary32 value >= 0 through atomics that are sent only when they would raise it.
 *   y at y + g y_stride_g + t y_stride_t + e y_stride_e: any strides >= 0, read without a copy.
 *   energy at energy + g e_stride_g + e e_stride_e + h, h < max_hops, caller-owned; nothing is written at h >= max_hops.
 *   state == NULL: a whole signal from rest; n_before must be 0; true_peak [n_sessions][2] (set to 0 by the caller; may be
 *     NULL) takes the peak, the positions behind the end whose windows still touch the signal included.
 *   state != NULL: a block of a stream.  state + g state_stride holds bas_meter_state_doubles() doubles per session, zeroed
 *     before a stream's first block: per ear the sample count (on the device: a captured call replays correctly) and a copy
 *     of it, the cascade's four states, the open hop's running sum, the last 11 input samples and a copy, the running true
 *     peak (binary32 bits in the low half of word 13 and 33).  true_peak must be NULL.  n_before: the caller's own count of
 *     the samples metered before this block, the largest over the sessions - used for the capacity check alone:
 *     (n_before + T_in) / hop > max_hops is refused (BAS_E_SHAPE) before any launch.  T_in == 0 is the stream's end: the
 *     true peak's last 11 positions; the state is not moved and the open hop is dropped.
 *   T_in <= hop + 1 (every real-time block; it touches two hops at the most): ONE launch, one workgroup per (ear, session),
 *     which moves the state itself.  Longer: three launches - every unit's end state from rest, the chain of the states,
 *     the energies - with a workspace of bas_meter_workspace_bytes (0 for T_in <= hop + 1 or arguments out of range) that
 *     need not be initialised.  No launch reads a word of the state that it writes.
 * One stream, no allocation, no synchronisation (capturable).  Every check runs before any launch: fs, hop == fs / 10,
 * n_sessions <= 65535, T_in < 2^30, max_hops < 2^31, strides >= 0, state_stride even and >= the state's size, the energy
 * buffer's strides address no element twice, capacity, ws_bytes, and no two of input, energy buffer, state, true_peak and
 * workspace overlap (BAS_E_SHAPE); taps, y (T_in > 0), energy (max_hops > 0), ws (T_in > hop + 1) required (BAS_E_NULL);
 * y, true_peak 4-byte aligned, energy 8-byte, state and ws 16-byte (BAS_E_ALIGN). */
size_t bas_meter_state_doubles(void);
size_t bas_meter_workspace_bytes(int n_sessions, long T_in, int hop);
int bas_meter_f32(const float *y, long y_stride_g, long y_stride_t, long y_stride_e, int n_sessions, long T_in, int fs,
                  int hop, const float *taps, double *energy, long e_stride_g, long e_stride_e, long max_hops,
                  long n_before, double *state, long state_stride, float *true_peak, void *ws, size_t ws_bytes,
                  bas_stream_t stream);

/* ---- ambisonic beds (no reference counterpart) --------------------------------------------------------
 * A bed is a sound field in real spherical harmonics: orders N = 1..3, C = (N + 1)^2 channels in ACN order, N3D inside
 * ((1 / 4 pi) int Y_a Y_b = delta_ab; no Condon-Shortley phase; SN3D input is a diagonal folded into the decoder by the
 * host).  In the frame of "head tracking" (d = (-sin az cos el, cos az cos el, sin el)) and (x, y, z) = (d_y, -d_x, d_z):
 *   Y_0 = 1;  Y_1..3 = r3 y, r3 z, r3 x;  Y_4..8 = r15 xy, r15 yz, (r5/2)(3 z^2 - 1), r15 xz, (r15/2)(x^2 - y^2);
 *   Y_9..15 = r(35/8) y (3 x^2 - y^2), r105 xyz, r(21/8) y (5 z^2 - 1), (r7/2) z (5 z^2 - 3), r(21/8) x (5 z^2 - 1),
 *   (r105/2) z (x^2 - y^2), r(35/8) x (x^2 - 3 y^2)        (r: the correctly rounded binary64 square root).
 * The bed is decoded to V <= 64 virtual loudspeakers fixed to the head; the FIELD is turned by the head orientation:
 * feeds = M bed with M = D Rot(q), D [V][C] the static decoder and Rot the C x C matrix, block diagonal per order, with
 * Y(R(q)^T s) = Rot Y(s) for every direction s (R(q): the matrix of "head tracking").  The feeds are V more source rows of a
 * render.  Both entries: one stream, no allocation, no synchronisation (capturable), one launch; every argument check runs
 * before the launch; all strides in elements, >= 0.
 *   bas_ambi_matrices_f32: head [n_groups][nb][4] (float64 (w, x, y, z) at head + g hs_g + k hs_c, hs_c >= 4) -> M
 *     (float32 at m + g ms_g + k ms_k + v C + c).  Rot is defined by sample points: S [J][3] unit vectors and Q [J][C]
 *     whose columns of order l are pinv(Y_l(S)^T) (the host makes both once; J <= 64);
 *       q is negated when w < 0; x == y == z == 0 after that (a zero quaternion included) is the identity: M = (float)D,
 *         exactly; otherwise q is normalised and h_j = R(q)^T s_j by the expressions of "head tracking";
 *       Rot[a][b] = sum_{j < J} Y_a(h_j) Q[j][b] for a, b of the same order, from +0 with j ascending, 0 elsewhere;
 *       M[v][c] = sum_b D[v][b] Rot[b][c], from +0 with b ascending over c's order block;
 *     all in binary64 without contraction, rounded to binary32 once.  Nothing is validated on the device (a non-finite
 *     head gives non-finite matrices).  order in 1..3, V in 1..64, J in 1..64, n_groups nb <= 2^30, hs_c >= 4, and the
 *     output's strides must address every element once (BAS_E_SHAPE); all pointers required (BAS_E_NULL); float64
 *     pointers 8-byte aligned, m 4-byte (BAS_E_ALIGN).
 *   bas_matrix_mix_f32: the hot path.  Input rows x + g xs_g + c xs_c (C <= 16 rows of T samples), matrices
 *     m + g ms_g + k ms_k + v C + c for the (T - 1) / K + 2 chunk boundaries, output rows y + g ys_g + v ys_v (V <= 64).
 *     For t = k K + j:  A = fmaf(M_k[v][c], x_c(t), A) from +0 with c ascending, B likewise with M_{k+1},
 *     w = (float)j * (1.0f / (float)K),  y_v(t) = A == B ? A : fmaf(w, B, fmaf(-w, A, A)) - the form of bas_color_rows_f32: an output's bits
 *     depend on (j, K, M_k, M_{k+1}) and the C inputs at t alone, not on tiles, block boundaries or alignment.
 *     ms_k == 0 is the static form, y = A (B skipped): the bits of the per-boundary form fed repeated matrices.
 *     ms_g == 0 shares one matrix bank, xs_g == 0 one bed over all groups.  16-byte loads and stores where a row is
 *     16-byte aligned, 4-byte ones elsewhere.  C in 1..16, V in 1..64, T < 2^30, n_groups <= 65535, K > 0, ms_k == 0 or
 *     >= V C, the output's strides must address every element once, and the output must overlap neither x nor the
 *     matrices (BAS_E_SHAPE); x, m, y required (BAS_E_NULL) and 4-byte aligned (BAS_E_ALIGN). */
#define BAS_AMBI_MAX_ORDER 3
#define BAS_AMBI_MAX_CHANNELS 16
#define BAS_AMBI_MAX_SPEAKERS 64
#define BAS_AMBI_MAX_POINTS 64
int bas_ambi_matrices_f32(const double *head, long hs_g, long hs_c, const double *D, const double *Q, const double *S,
                          int J, int order, int V, int n_groups, int nb, float *m, long ms_g, long ms_k,
                          bas_stream_t stream);
int bas_matrix_mix_f32(const float *x, long xs_g, long xs_c, const float *m, long ms_g, long ms_k, int C, int V,
                       int n_groups, long T, int K, float *y, long ys_g, long ys_v, bas_stream_t stream);

/* ---- ambisonic encoder (no reference counterpart) -------------------------------------------------------
 * The stage in front of a bed: n_src point sources with directions (and gains) at chunk boundaries are summed into one bed
 * of order N = 1..3 in world coordinates, conventions as above.  Both entries: one stream, no allocation, no synchronisation
 * (capturable), one launch; every argument check runs before the launch; all strides in elements, >= 0 and below 2^40.
 *   bas_ambi_encode_gains_f32: angles (float64 radians, world frame) at elev + g as_g + s as_s + k and azim likewise (the
 *     layout of a renderer's trajectory views), gain likewise with its own strides (NULL: 1) -> banks E (float32 at
 *     e + g es_g + k es_k + s C + c, the [n_src][C] banks dense):
 *       d = (-sin az cos el, cos az cos el, sin el);  E[s][c] = (gain * scale[l(c)]) * Y_c(d),  l(c) the order of channel c;
 *     scale: order + 1 doubles in HOST memory, read before the launch (1 for N3D output, 1 / sqrt(2 l + 1) for SN3D: the
 *     host's choice).  Binary64 without contraction, the product order as written, rounded to binary32 once.  Nothing is
 *     validated on the device.  order in 1..3, n_src in 1..65536, n_groups nb n_src <= 2^30, and the output's strides must
 *     address every element once (BAS_E_SHAPE); elev, azim, scale, e required (BAS_E_NULL); float64 pointers 8-byte
 *     aligned, e 4-byte (BAS_E_ALIGN).  n_groups == 0 or nb == 0: nothing to do.
 *   bas_ambi_encode_f32: the hot path.  Signals x + g xs_g + s xs_s (n_src rows of T samples), banks
 *     e + g es_g + k es_k + s C + c for the (T - 1) / K + 2 chunk boundaries, output rows y + g ys_g + c ys_c (C <= 16, any
 *     value).  The reduction over the sources has two levels; sources form blocks of BAS_AMBI_ENCODE_BLOCK = 32
 *     consecutive rows.  For t = k K + j:
 *       per block b:   A_b = fmaf(E_k[s][c], x_s(t), A_b) from +0 with s ascending inside the block, B_b likewise with E_{k+1};
 *       across blocks: A = A_0, then A = A + A_b for b = 1, 2, .. ascending (binary32 additions), B likewise;
 *       w = (float)j * (1.0f / (float)K),  y = A == B ? A : fmaf(w, B, fmaf(-w, A, A));   with base:  y = base_c(t) + y  (one addition).
 *     es_k == 0 is the static form, y = A (B skipped): the bits of the per-boundary form fed repeated banks.  An output's
 *     bits depend on (j, K, n_src, E_k[:, c], E_{k+1}[:, c]), the n_src inputs at t and base_c(t) alone - not on tiles, T,
 *     block boundaries of a stream, alignment, grid, slab sizes or groups.  With n_src <= 32 this is the chain of
 *     bas_matrix_mix_f32 fed the transposed bank.  xs_g == 0 shares the signals, es_g == 0 the banks over all groups.
 *     base: NULL, or rows base + g bs_g + c bs_c; base may be y itself with y's strides (in place: every output is read and
 *     written by the one lane that owns it), otherwise it must not overlap y.  16-byte loads and stores where a row is
 *     16-byte aligned, 4-byte ones elsewhere.  C in 1..16, n_src in 1..65536, T < 2^30, n_groups <= 65535, K > 0,
 *     es_k == 0 or >= n_src C with ((T - 1) / K + 2) es_k <= 2^62, the output's strides must address every element once,
 *     and the output must overlap neither x nor the banks (BAS_E_SHAPE); x, e, y required (BAS_E_NULL); x, e, base, y 4-byte aligned (BAS_E_ALIGN).
 *     n_groups == 0 or T == 0: nothing to do. */
#define BAS_AMBI_ENCODE_BLOCK 32
#define BAS_AMBI_ENCODE_MAX_SOURCES 65536
int bas_ambi_encode_gains_f32(const double *elev, const double *azim, long as_g, long as_s, const double *gain, long gs_g,
                              long gs_s, const double *scale, int order, int n_groups, int n_src, int nb, float *e,
                              long es_g, long es_k, bas_stream_t stream);
int bas_ambi_encode_f32(const float *x, long xs_g, long xs_s, const float *e, long es_g, long es_k, int n_src, int C,
                        int n_groups, long T, int K, const float *base, long bs_g, long bs_c, float *y, long ys_g,
                        long ys_c, bas_stream_t stream);

/* ---- table builder: the heavy parts of upsample_irs.m ---------
 * PARITY UNPINNED (no Octave, no IRCAM data in the build: upsample_irs.py's header).  All
 * arrays float64 on the device; h = the 2 Lh + 1 taps of the resampling filter Octave's
 * resample(x, p, 1) designs (upsample_irs.py: octave_resample_filter), made on the host.
 *
 * bas_resample_up_f64: y[r][j] = sum_k h[j + Lh - p k] x[r][k], j < lx p: `rows` signals
 *   of lx samples resampled by p (upsample_irs.m:37-44: the 2 x 187 HRIRs).
 * bas_delaydiffs_f64: diffs [n_dir][n_dir] (overwritten) = the antisymmetric matrix of
 *   delay differences (upsample_irs.m:15-32, :58-101): for every pair i < j the
 *   cross-correlation of irs[i], irs[j] ([n_dir][n_taps]), resampled by p, its FIRST
 *   maximum refined by a parabola; diffs[i][j] = peak / p - (n_taps - 1), diffs[j][i] =
 *   -diffs[i][j], zero diagonal.  status: ONE 64-bit word on the device (overwritten,
 *   8-byte aligned): 0, or - where a pair hit one of the reference's preconditions -
 *   ((n_dir^2 - (i n_dir + j)) << 2) | code for the failing pair with the smallest (i, j)
 *   (the same one whichever workgroup ran first); code 1: peak at the edge of the
 *   correlation's support (:70), 2: the middle point is not the first maximum (:92-93),
 *   3: three collinear points (:98).  Failing pairs' entries stay zero.  One ear per call. */
int bas_resample_up_f64(const double *x, int rows, int lx, const double *h, int Lh, int p,
                        double *y, bas_stream_t stream);
int bas_delaydiffs_f64(const double *irs, int n_dir, int n_taps, const double *h, int Lh, int p,
                       double *diffs, unsigned long long *status, bas_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BAS_H */
