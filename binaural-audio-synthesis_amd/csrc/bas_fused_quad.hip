// a6 + a7 + a8 in one kernel (gfx950) for SMALL scenes - one source (BASELINE configs 2 and 3), a handful of sources, the
// real-time blocks of a stream: at most a few (tile of 2048, source) units per CU, where what counts is how long ONE unit
// takes.  Same arithmetic as bas_render_fz_kernel<1, false> (bas_fused.hip; interpolate_2d apply_hrtf.py:219-279, crossfade
// :442-443, FIR :445-446, overlap-add and mix :450-453) on the same tiles, but FOUR waves per tile instead of one:
//
//   staging   all four waves fetch the x window (3 float4 per lane instead of 9) and evaluate the tile's 6-7 chunk IRs, two
//             each instead of all of them in a chain (dealt and handed over as in the four-wave kernels);
//   FIR       lane = one of the tile's 64 rows in EVERY wave; wave w runs the row steps rp = w (mod 4) - a 128-tap segment
//             has rp = 0 .. 4 with half of the taps live in steps 0 and 4, so the four waves get one full step each - into
//             its own 98 accumulators (the FIR is linear in the taps: partial sums over disjoint tap ranges add up);
//   flush     when the tile is finished the waves' 32 x 2 outputs per row meet in LDS and wave 0 adds them in the fixed
//             order 0, 1, 2, 3 (deterministic) and writes the tile (y itself for one source, a slab part otherwise).
//
// One wave per SIMD runs this instruction stream at ~5 clocks per vector instruction, so a unit takes about a
// quarter of the one-wave kernel's 19 us plus two barriers.  The walk, the window geometry, the row-step setup and the flush's
// combine and stores are bas_window.h, shared with the other FIR kernels.  No MFMA: this is a 1-D FIR (BASELINE.json north_star).
#include "bas_fused.h"

#if FZ_ASM
__global__ __launch_bounds__(256, 2) void bas_render_fq_kernel(
    FzArgs A, const float *__restrict__ x,                   // [n_src] rows of T_in floats, stride A.x_stride
    float *__restrict__ slab,                                // [n_wg][parts_per_wg][2][tile]
    const float *__restrict__ packed,                        // table in phase-plane layout
    const unsigned *__restrict__ plans,                      // [n_src][n_chunks+1][2 ears][BAS_PLANS_WORDS]
    float *__restrict__ y, unsigned int *__restrict__ peak_bits) {   // direct output only: [2][T_out], max|y| bits
    constexpr int NW = 4;
    constexpr int THREADS = 64 * NW;
    constexpr int TILE = 2048;
    constexpr int ROWS = TILE / 32 + HD_HALO;                // rows of 32 inputs in the x window (68)
    constexpr int XR = ROWS + 1;                             // odd: conflict-free column-major image
    constexpr int NX = (ROWS * 8 + THREADS - 1) / THREADS;   // float4 of x per thread (3)
    constexpr int XFLOATS = 8 * XR * 4;
    constexpr int MAXEV = BAS_FQ_MAXEV;                      // chunk IRs one wave evaluates per unit
    constexpr int PL4 = WIN_PL4;
    constexpr int NPV = (MAXEV * PL4 + 63) / 64;             // 16-byte plan pieces per lane
    static_assert(XR == 69, "bas_fir_asm.inc holds the row step for this x-image stride");
    extern __shared__ f32x4 lds4[];
    // LDS: [8][XR] float4 x image | [nslots][HD_SLOT] taps (h0_L, h0_R, d_L, d_R) | [NW][MAXEV * PL4] plans |
    //      [NW][64] float4 boundary IRs | [NW] flags | [3][32][64] float2 outputs of waves 1-3 at a flush
    f32x4 *xs4 = lds4;
    float *hd = reinterpret_cast<float *>(lds4) + XFLOATS;
    f32x4 *pl_base = reinterpret_cast<f32x4 *>(hd + ((A.nslots * HD_SLOT + 3) & ~3));
    f32x4 *bnd = pl_base + NW * (MAXEV * PL4);
    volatile unsigned *flags = reinterpret_cast<volatile unsigned *>(bnd + NW * 64);
    f32x2 *comb = reinterpret_cast<f32x2 *>(bnd + NW * 64 + 1);

    const int tid0 = threadIdx.x;
    const int lane0 = tid0 & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid0 >> 6);

    const WinWalk W = win_walk(A.units_total, A.units_per_wg, A.Lp);
    const long n_pass = W.n_pass;
    if (!A.direct && peak_bits && blockIdx.x == 0 && tid0 == 0) *peak_bits = 0u;   // the reduce kernel maxes into it later
    if (n_pass <= 0) {
        if (A.direct && A.tail_mode) bas_tail<THREADS>(fz_tail(A, y, peak_bits), 0.f);
        return;
    }
    unsigned wmax_bits = 0u;                                 // direct output with a tail: max|y| wave 0 has stored (uniform)
    if (tid0 < NW) flags[tid0] = 0u;                         // hand-over flags of the boundary IRs: no pass has id 0
                                                             // (ordered before their first use by the first pass's barrier)
    f32x32 accA, accB, accP;                                 // half-rate partial sums (bas_fir.h), pinned to v[0:97] by the block
    f32x2 accB16 = f32x2{0.f, 0.f};
    win_zero_pinned(accA, accB, accB16, accP);

    const long first_tile = W.unit0 / A.n_src;
    float *slab_wg = slab + (long)blockIdx.x * A.parts_per_wg * 2 * TILE;
    const __amdgpu_buffer_rsrc_t tab =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(packed), 0, (int)A.packed_bytes, 0x00020000);
    const unsigned L4 = 4u * (unsigned)A.L;

    // every wave holds a share of the tile's outputs (its row steps' taps): they meet in LDS, wave 0 writes the tile
    auto flush = [&](long t) {
        f32x2 acc[32];
        win_combine_pinned(acc, accA, accB, accB16, accP);
        win_zero_pinned(accA, accB, accB16, accP);
        if (wv > 0) {
            f32x2 *c = comb + (wv - 1) * 32 * 64 + lane0;
#pragma unroll
            for (int i = 0; i < 32; ++i) c[i * 64] = acc[i];
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int w = 0; w < 3; ++w) {
                const f32x2 *c = comb + w * 32 * 64 + lane0;
#pragma unroll
                for (int i = 0; i < 32; ++i) acc[i] += c[i * 64];
            }
            if (A.direct) {                                  // uniform
                const long n0 = t * TILE + 32 * lane0;       // this lane's first output
                wmax_bits = win_flush_row_direct(acc, y, A.T_out, n0, A.accumulate, A.tail_mode, peak_bits, wmax_bits);
            } else {
                win_store_row_slab(acc, slab_wg + (t - first_tile) * 2 * TILE + 32 * lane0, TILE);
            }
        }
        __syncthreads();                                     // (the next flush may write the meeting place again)
    };

    // scalar state of the walk over (tile, source, tap segment)
    long tile = first_tile;
    int s = (int)(W.unit0 - first_tile * A.n_src);
    int sg = 0;
    WinGeo G = win_geo<TILE>(tile, sg, A.K, A.Lp);
    long open_tile = -1;                                     // tile whose partial sums the accumulators hold
    // this wave's share of the nslots + 1 chunk IRs: balanced contiguous ranges [slot_a, slot_b); it writes the slots
    // [slot_a, slot_b): slot i holds (IR i, IR i+1 - IR i), so its LAST slot needs the FIRST IR of the next wave, which that
    // wave leaves in LDS as soon as it has it (bnd / flags).  (A copy of bas_render_fz_kernel's deal: that kernel cannot take a
    // shared helper - its scratch size changes - and the split-role stagers' copy differs on purpose.)
    const int n_ir = A.nslots + 1, base = n_ir / NW, rem = n_ir - base * NW;
    const int slot_a = wv * base + (wv < rem ? wv : rem);
    const int slot_b = slot_a + base + (wv < rem ? 1 : 0);
    const int n_ev = slot_a < slot_b ? slot_b - slot_a : 0;
    const bool need_next = n_ev > 0 && slot_b <= A.nslots;  // slot slot_b - 1 exists: it needs IR slot_b
    f32x4 *plw = pl_base + wv * (MAXEV * PL4);

    for (long pid = 0; pid < n_pass; ++pid) {
        // the thread index is made opaque once per pass: what derives from it is recomputed per pass instead of being held in
        // (or spilled from) registers across the row steps
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const int lane = tid & 63;
        if (tile != open_tile) {                             // the accumulators belong to another tile: hand them over
            if (open_tile >= 0) flush(open_tile);
            open_tile = tile;
        }
        const int seg0 = G.seg0, Lseg = G.Lseg, halo = G.halo, nrows = G.nrows;
        __builtin_amdgcn_s_setprio(3);                       // staging is latency bound: its few instructions go first
        // ---- global -> registers: read plans of this wave's chunk IRs (both ears) and the x window
        f32x4 pv[NPV], xv[NX];
        const f32x4 *pl_src = reinterpret_cast<const f32x4 *>(plans) + (long)s * (A.n_chunks + 1) * PL4;
#pragma unroll
        for (int r = 0; r < NPV; ++r)                        // (read once, as the x window is: non-temporal)
            pv[r] = __builtin_nontemporal_load(win_plan_piece(pl_src, lane, r, n_ev, G.c0 + slot_a, A.n_chunks));
        const WinXBounds XB = win_x_bounds(G.xbase, A.T_in);
        const bool x_inside = win_x_inside<NX, THREADS>(XB);
        win_fetch_x<NX, THREADS>(xv, x + (long)s * A.x_stride + G.xbase, tid, XB);
        __syncthreads();                                     // previous pass has finished reading LDS
        // ---- registers -> LDS: plans into this wave's own region, the x window as a column-major image
        const unsigned pass_id = (unsigned)pid + 1u;
#pragma unroll
        for (int r = 0; r < NPV; ++r)
            if (lane + 64 * r < n_ev * PL4) plw[lane + 64 * r] = pv[r];
#pragma unroll
        for (int j = 0; j < NX; ++j) {                       // (as in bas_render_fz_kernel; a shared helper changed both kernels' branches)
            const int i4 = tid + j * THREADS;
            f32x4 v = xv[j];
            if (!x_inside) {                                 // uniform: only windows that overlap an end of the signal
                const int e = 4 * i4;                        // the bounds are multiples of 4: all four in or out
                if (!(e >= XB.lo && e < XB.hi)) v = f32x4{0.f, 0.f, 0.f, 0.f};
            }
            if (i4 < nrows * 8) xs4[(i4 & 7) * XR + (i4 >> 3)] = v;
        }
        __builtin_amdgcn_wave_barrier();                     // other lanes of this wave read the plan words below

        // ---- chunk IRs from the table: lanes 0-31 four adjacent taps of the left ear, lanes 32-63 of the right.
        // Two halves of 8 reads are in flight at any time; slot i - 1 = (IR i-1, IR i - IR i-1) is stored as soon
        // as IR i is known: both ears of two taps per 16-byte LDS write.  (A copy of the (h0, d) form of bas_render_fz_kernel's
        // loop, which carries its h-only rows as a branch inside the same body and so stays whole.)
        {
            const int half = lane >> 5;
            const int m = seg0 + 4 * (lane & 31);
            const int m_c = m < A.L ? m : A.L - 1;           // idle lanes evaluate a valid tap and drop it
            const unsigned m4 = 4u * (unsigned)m_c;
            const f32x4 live = f32x4{m < A.L ? 1.f : 0.f, m + 1 < A.L ? 1.f : 0.f, m + 2 < A.L ? 1.f : 0.f,
                                     m + 3 < A.L ? 1.f : 0.f};                 // taps >= L read as zero
            const f32x4 *pl = plw + half * (BAS_PLANS_WORDS / 4);
            const int tq = 4 * (lane & 31) + (lane < 32 ? 2 : 0);          // first of the two taps this lane stores
            f32x4 *dst = reinterpret_cast<f32x4 *>(hd) + slot_a * (HD_SLOT / 4) + tq;
            FzHalf ha, hb;
            f32x4 prev = f32x4{0.f, 0.f, 0.f, 0.f};
            const f32x4 *pl_last = pl + (n_ev > 0 ? n_ev - 1 : 0) * PL4;
            if (n_ev > 0) fz_issue<0>(tab, pl, m4, L4, ha);  // (a wave without slots - few, long chunks - skips it all)
            for (int i = 0; i < n_ev; ++i) {
                const f32x4 *pl_next = pl + PL4 < pl_last ? pl + PL4 : pl_last;
                fz_issue<1>(tab, pl, m4, L4, hb);
                f32x4 h = fz_finish<0>(pl, ha, f32x4{0.f, 0.f, 0.f, 0.f});
                fz_issue<0>(tab, pl_next, m4, L4, ha);
                h = fz_finish<1>(pl, hb, h) * live;
                if (i == 0 && wv > 0) {                      // (uniform) the previous wave's last slot needs this IR
                    bnd[wv * 64 + lane] = h;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0 && !fz_inject(A)) flags[wv] = pass_id;
                }
                if (i > 0) {                                 // slot slot_a + i - 1, written once IR i is known
                    f32x2 h0a, h0b, da, db;
                    fz_pair_ears(prev, h0a, h0b);
                    fz_pair_ears(h - prev, da, db);
                    if (tq < Lseg) {
                        dst[0] = f32x4{h0a.x, h0a.y, da.x, da.y};
                        dst[1] = f32x4{h0b.x, h0b.y, db.x, db.y};
                    }
                    dst += HD_SLOT / 4;
                }
                prev = h;
                pl = pl_next;
            }
            if (need_next) {                                 // (uniform) IR slot_b comes from the next wave's LDS copy
                const bool got = fz_wait_handover(flags + wv + 1, pass_id, A);   // it stored that IR first thing
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                f32x4 nx = bnd[(wv + 1) * 64 + lane];
                if (!got) nx = f32x4{__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
                f32x2 h0a, h0b, da, db;
                fz_pair_ears(prev, h0a, h0b);
                fz_pair_ears(nx - prev, da, db);
                if (tq < Lseg) {
                    dst[0] = f32x4{h0a.x, h0a.y, da.x, da.y};
                    dst[1] = f32x4{h0b.x, h0b.y, db.x, db.y};
                }
            }
        }
        __syncthreads();
        __builtin_amdgcn_s_setprio(0);

        // ---- FIR: the lane's row in every wave; this wave's share of the input rows rho' = 0..halo above/at it
        const int row_out = lane + halo;                     // window row holding the lane's outputs
        int sl, m_in;                                        // chunk slot of that row, its offset inside the chunk
        win_row_slot(G.mo0 + 32 * row_out, A.K, A.invK, sl, m_in);
        const f32x4 *xrow = xs4 + row_out;
#pragma unroll 1
        for (int rp = 0; rp <= halo; ++rp) {
            if ((rp & (NW - 1)) == wv) {                     // (uniform)
                const float al = win_weight(m_in, A.S, A.s_pow2, A.invK, A.invS);
                const unsigned mk = win_octet_mask(rp, Lseg);
                ffa_row_step_asm<XR>(accA, accB, accB16, accP, (unsigned)reinterpret_cast<uintptr_t>(xrow),
                                     (unsigned)reinterpret_cast<uintptr_t>(hd + sl * HD_SLOT + (32 * rp - 32) * 4), al, mk);
            }
            xrow -= 1;
            win_row_up(A.K, sl, m_in);
        }

        // ---- next (tile, source, segment)
        const WinPos N = win_next(tile, s, sg, W.nseg, A.n_src);
        if (N.tile != tile || N.sg != sg) G = win_geo<TILE>(N.tile, N.sg, A.K, A.Lp);
        tile = N.tile, s = N.s, sg = N.sg;
    }
    flush(open_tile);
    if (A.direct && A.tail_mode) bas_tail<THREADS>(fz_tail(A, y, peak_bits), __uint_as_float(wmax_bits));
}

#endif  // FZ_ASM

size_t bas_fq_lds_bytes(int nslots) {
    const int rows = 2048 / 32 + HD_HALO;
    return (size_t)(8 * (rows + 1) * 4 + ((nslots * HD_SLOT + 3) & ~3) + 4 * BAS_FQ_MAXEV * 2 * BAS_PLANS_WORDS + 4 * 64 * 4 + 4) * sizeof(float) +
           (size_t)3 * 32 * 64 * sizeof(f32x2);
}

const BasKernelRow *bas_fq_row() {
#if FZ_ASM
    static const BasKernelRow row = {"bas_render_fq_kernel", "bas_render_fq_kernel", reinterpret_cast<const void *>(bas_render_fq_kernel),
                                     256, 0, 1 | (1 << 6)};
    return &row;
#else
    return nullptr;                                          // (make cppstep: the kernel exists only around the assembly blocks)
#endif
}
