// Cartesian scenes (include/bas.h "Cartesian scenes"): source positions [G][n_src][nb][3], the listener's
// position and head orientation per boundary and an optional shoebox room's image list -> the angles, gains and delays
// of every image source, [G][n_src n_img][nb], strided on both sides so that a stream renderer's views take them in
// place.  One launch.
#include "bas_internal.h"
#include "bas_scene.h"
#include "bas_occlude.h"

#include <string.h>

#define SC_THREADS 256
#define SC_MAX_BANDS 16

struct BasSceneArgs {
    const double *pos; long ps_g, ps_s, ps_c;
    const double *prev; long pp_g, pp_s;
    double spc;
    const double *lpos; long lp_g, lp_c;
    const double *head; long h_g, h_c;
    const double *src_gain; long sg_g, sg_s;
    const double *room_size; const int32_t *images; const double *img_gain;
    double spm, r_ref, dmin, dmax;
    int n_src, n_img, nb;
    double *elev, *azim, *gain; long a_g, a_s;
    double *delay; long d_g, d_s;
    // bas_scene_params_bands_f64 only: the per-band log-magnitudes of every (row, boundary)
    const double *orient; long o_g, o_s, o_c;
    const double *pattern; long pt_s;
    const double *air, *img_logmag;
    int n_bands; double floor;
    double *logmag; long l_g, l_s, l_c;
};

// bas_scene_params_occluded_f64's kernel also takes the screens every path is held against; the other two
// keep the argument block they had
struct BasSceneOccArgs : BasSceneArgs {
    BasOccludeScreens scr;
};

// one thread per (g, s, i, c) item, c fastest (the stores of a wave are consecutive along c), grid-stride.  BANDS: the
// item's n_bands log-magnitudes follow, L[b] = ln W_i[b] - air[b] r + ln max(|a_b + (1 - a_b) cos theta|, floor), floored
// at ln floor, n_bands consecutive doubles per thread (the threads of a wave tile a consecutive range where l_c = n_bands)
// MODE: SC_PLAIN (no bands), SC_BANDS, SC_SCREENS (the bands, and the screens' term in them: + bas_occlude_sum before the
// floor).  The first two are the kernels they were before the third existed: what SC_SCREENS adds is compiled out of them.
enum { SC_PLAIN = 0, SC_BANDS = 1, SC_SCREENS = 2 };
template <int MODE> struct ScArgs { typedef BasSceneArgs type; };
template <> struct ScArgs<SC_SCREENS> { typedef BasSceneOccArgs type; };

template <int MODE>
__global__ __launch_bounds__(SC_THREADS) void bas_scene_params_kernel(typename ScArgs<MODE>::type A, long n_items) {
    constexpr bool BANDS = MODE != SC_PLAIN;
    const long per_s = (long)A.n_img * A.nb, per_g = per_s * A.n_src;
    const bool room = A.room_size != nullptr;
    double Lx = 0.0, Ly = 0.0, Lz = 0.0;
    if (room) {
        Lx = A.room_size[0]; Ly = A.room_size[1]; Lz = A.room_size[2];
    }
    for (long it = blockIdx.x * (long)SC_THREADS + threadIdx.x; it < n_items; it += (long)gridDim.x * SC_THREADS) {
        const long g = it / per_g, r0 = it - g * per_g;
        const long s = r0 / per_s, r1 = r0 - s * per_s;
        const long i = r1 / A.nb, c = r1 - i * A.nb;
        const double *p = A.pos + g * A.ps_g + s * A.ps_s + c * A.ps_c;
        double lx = 0.0, ly = 0.0, lz = 0.0, w = 1.0, x = 0.0, y = 0.0, z = 0.0;
        if (A.lpos) {
            const double *l = A.lpos + g * A.lp_g + c * A.lp_c;
            lx = l[0]; ly = l[1]; lz = l[2];
        }
        if (A.head) {
            const double *q = A.head + g * A.h_g + c * A.h_c;
            w = q[0]; x = q[1]; y = q[2]; z = q[3];
        }
        int mx = 0, my = 0, mz = 0;
        double ig = 1.0;
        if (room) {
            mx = A.images[3 * i]; my = A.images[3 * i + 1]; mz = A.images[3 * i + 2];
            ig = A.img_gain[i];
        }
        // the two positions a chunk apart that give the source's velocity at this boundary: (c - 1, c); at c = 0 the
        // caller's previous boundary, else (0, 1)
        const bool moving = A.spc > 0.0 && (c > 0 || A.prev || A.nb > 1);
        const double *a = p, *b = p;
        if (moving) {
            if (c > 0) a = p - A.ps_c;
            else if (A.prev) a = A.prev + g * A.pp_g + s * A.pp_s;
            else b = p + A.ps_c;
        }
        const double sg = A.src_gain ? A.src_gain[g * A.sg_g + s * A.sg_s + c] : 1.0;
        double ow = 1.0, ox = 0.0, oy = 0.0, oz = 0.0;
        if (BANDS && A.orient) {
            const double *q = A.orient + g * A.o_g + s * A.o_s + c * A.o_c;
            ow = q[0]; ox = q[1]; oy = q[2]; oz = q[3];
        }
        const BasScenePoint o = bas_scene_point(p[0], p[1], p[2], lx, ly, lz, moving, a[0], a[1], a[2], b[0], b[1],
                                                b[2], A.spc, room, Lx, Ly, Lz, mx, my, mz, A.head != nullptr,
                                                w, x, y, z, sg, ig, A.spm, A.r_ref, A.dmin, A.dmax, BANDS, ow, ox, oy, oz);
        const long row = s * A.n_img + i;
        if constexpr (MODE == SC_SCREENS) {
#pragma clang fp contract(off)
            // (the four results first: they need not stay in registers through the screens)
            const long to = g * A.a_g + row * A.a_s + c;
            A.elev[to] = o.el;
            A.azim[to] = o.az;
            if (A.gain) A.gain[to] = o.gain;
            if (A.delay) A.delay[g * A.d_g + row * A.d_s + c] = o.delay;
            double occ[SC_MAX_BANDS];
#pragma unroll
            for (int k = 0; k < SC_MAX_BANDS; ++k) occ[k] = 0.0;
            bas_occlude_sum(A.scr, o.qx, o.qy, o.qz, lx, ly, lz, room, Lx, Ly, Lz, mx, my, mz, occ);
            double *L = A.logmag + g * A.l_g + row * A.l_s + c * A.l_c;
            const double ln_floor = log(A.floor);
            for (int bd = 0; bd < A.n_bands; ++bd) {
                double v = A.img_logmag ? A.img_logmag[i * A.n_bands + bd] : 0.0;
                if (A.air) v = v - A.air[bd] * o.r;
                if (A.pattern) {
                    const double al = A.pattern[s * A.pt_s + bd];
                    v = v + log(fmax(fabs(al + (1.0 - al) * o.cos_theta), A.floor));
                }
                double ob = 0.0;
#pragma unroll
                for (int k = 0; k < SC_MAX_BANDS; ++k) ob = k == bd ? occ[k] : ob;
                L[bd] = fmax(v + ob, ln_floor);
            }
        } else if (BANDS) {
#pragma clang fp contract(off)
            double *L = A.logmag + g * A.l_g + row * A.l_s + c * A.l_c;
            const double ln_floor = log(A.floor);
            for (int bd = 0; bd < A.n_bands; ++bd) {
                double v = A.img_logmag ? A.img_logmag[i * A.n_bands + bd] : 0.0;
                if (A.air) v = v - A.air[bd] * o.r;
                if (A.pattern) {
                    const double al = A.pattern[s * A.pt_s + bd];
                    v = v + log(fmax(fabs(al + (1.0 - al) * o.cos_theta), A.floor));
                }
                L[bd] = fmax(v, ln_floor);
            }
        }
        if (MODE == SC_SCREENS) continue;
        const long to = g * A.a_g + row * A.a_s + c;
        A.elev[to] = o.el;
        A.azim[to] = o.az;
        if (A.gain) A.gain[to] = o.gain;
        if (A.delay) A.delay[g * A.d_g + row * A.d_s + c] = o.delay;
    }
}

// the written layout [G][rows][nb] with strides (sg, ss, 1) addresses no element twice (bas_internal.h)
static bool sc_one_to_one(long G, long rows, long nb, long sg, long ss) { return bas_layout_one_to_one(G, rows, nb, sg, ss); }


// what bas_scene_params_bands_f64 adds to the argument list
struct BasSceneBands {
    const double *orient; long o_g, o_s, o_c;
    const double *pattern; long pt_s;
    const double *air, *img_logmag;
    int n_bands; double floor;
    double *logmag; long l_g, l_s, l_c;
    // bas_scene_params_occluded_f64 only (fn names it: occluded)
    bool occluded;
    const double *screens, *transmission; long t_s;
    const double *fresnel; int n_screens;
};

// The launcher the three entry points share (B == nullptr: bas_scene_params_f64, the kernel without the bands;
// B->occluded: bas_scene_params_occluded_f64, the bands with the screens): every check, then one launch.
static int sc_launch(const char *fn, const double *pos, long pos_stride_g, long pos_stride_s, long pos_stride_c,
                     const double *pos_prev, long prev_stride_g, long prev_stride_s, double samples_per_chunk,
                     const double *lpos, long lpos_stride_g, long lpos_stride_c, const double *head, long head_stride_g,
                     long head_stride_c, const double *src_gain, long sg_stride_g, long sg_stride_s,
                     const double *room_size, const int32_t *images, const double *img_gain, int n_img,
                     double samples_per_metre, double r_ref, double d_min, double d_max, int n_groups, int n_src, int nb,
                     double *elev, double *azim, double *gain, long a_stride_g, long a_stride_s, double *delay,
                     long d_stride_g, long d_stride_s, const BasSceneBands *B, bas_stream_t stream) {
    BAS_REQUIRE(n_groups > 0 && n_src > 0 && nb > 0 && n_img > 0, BAS_E_SHAPE,
                "%s: need n_groups, n_src, nb, n_img > 0 (G=%d n_src=%d nb=%d n_img=%d)", fn, n_groups, n_src, nb, n_img);
    BAS_REQUIRE((long)n_src * n_img <= 0x7fffffffL, BAS_E_SHAPE, "%s: n_src n_img must be below 2^31", fn);
    BAS_REQUIRE(room_size || n_img == 1, BAS_E_SHAPE, "%s: free field (room_size NULL) has one image, not %d", fn, n_img);
    BAS_REQUIRE(samples_per_chunk >= 0.0 && samples_per_chunk < HUGE_VAL && prev_stride_g >= 0 && prev_stride_s >= 0 &&
                (!pos_prev || samples_per_chunk > 0.0), BAS_E_SHAPE,
                "%s: need finite samples_per_chunk >= 0 (> 0 with pos_prev) and non-negative pos_prev strides", fn);
    BAS_REQUIRE(pos_stride_g >= 0 && pos_stride_s >= 0 && pos_stride_c >= 0 && lpos_stride_g >= 0 && lpos_stride_c >= 0 &&
                head_stride_g >= 0 && head_stride_c >= 0 && sg_stride_g >= 0 && sg_stride_s >= 0, BAS_E_SHAPE,
                "%s: input strides must be non-negative", fn);
    BAS_REQUIRE(samples_per_metre > 0.0 && samples_per_metre < HUGE_VAL && r_ref > 0.0 && r_ref < HUGE_VAL && d_min >= 0.0 &&
                d_max >= d_min, BAS_E_SHAPE,
                "%s: need finite samples_per_metre, r_ref > 0 and 0 <= d_min <= d_max (%g, %g, %g, %g)", fn, samples_per_metre,
                r_ref, d_min, d_max);
    const long rows = (long)n_src * n_img;
    BAS_REQUIRE(a_stride_g >= 0 && a_stride_s >= 0 && sc_one_to_one(n_groups, rows, nb, a_stride_g, a_stride_s), BAS_E_SHAPE,
                "%s: angle/gain output strides (%ld, %ld, 1) overlap for [%d][%ld][%d]", fn, a_stride_g, a_stride_s, n_groups,
                rows, nb);
    BAS_REQUIRE(!delay || (d_stride_g >= 0 && d_stride_s >= 0 && sc_one_to_one(n_groups, rows, nb, d_stride_g, d_stride_s)),
                BAS_E_SHAPE, "%s: delay output strides (%ld, %ld, 1) overlap for [%d][%ld][%d]", fn, d_stride_g, d_stride_s,
                n_groups, rows, nb);
    BAS_REQUIRE(pos && elev && azim && (!room_size || (images && img_gain)), BAS_E_NULL, "%s: null pointer", fn);
    BAS_REQUIRE(elev != azim && (!gain || (gain != elev && gain != azim)) &&
                (!delay || (delay != elev && delay != azim && delay != gain)), BAS_E_SHAPE,
                "%s: two outputs are one buffer", fn);
    BAS_REQUIRE(bas_aligned(pos, 8) && bas_aligned(pos_prev, 8) && bas_aligned(lpos, 8) && bas_aligned(head, 8) &&
                bas_aligned(src_gain, 8) && bas_aligned(room_size, 8) && bas_aligned(img_gain, 8) &&
                bas_aligned(images, 4) && bas_aligned(elev, 8) && bas_aligned(azim, 8) && bas_aligned(gain, 8) &&
                bas_aligned(delay, 8), BAS_E_ALIGN,
                "%s: float64 arrays must be 8-byte aligned (images: 4-byte)", fn);
    BasSceneOccArgs AO;
    memset(&AO, 0, sizeof AO);
    BasSceneArgs &A = AO;
    if (B) {
        BAS_REQUIRE(B->n_bands >= 1 && B->n_bands <= SC_MAX_BANDS, BAS_E_SHAPE, "%s: n_bands (%d) must be in 1..%d", fn,
                    B->n_bands, SC_MAX_BANDS);
        BAS_REQUIRE(B->floor > 0.0 && B->floor <= 1.0, BAS_E_SHAPE, "%s: the floor (%g) must be in (0, 1]", fn, B->floor);
        BAS_REQUIRE(B->o_g >= 0 && B->o_s >= 0 && B->o_c >= 0 && B->pt_s >= 0, BAS_E_SHAPE,
                    "%s: input strides must be non-negative", fn);
        BAS_REQUIRE(B->pt_s == 0 || B->pt_s >= B->n_bands, BAS_E_SHAPE,
                    "%s: the pattern's source stride must be 0 (shared) or >= n_bands", fn);
        // [G][rows][nb][n_bands] with strides (l_g, l_s, l_c, 1): a boundary's bands must not meet the next one's, and the
        // rows' extents (nb - 1) l_c + n_bands are held to the rule of the other outputs
        long extent = 0;
        BAS_REQUIRE(B->l_g >= 0 && B->l_s >= 0 && B->l_c >= B->n_bands &&
                    !__builtin_mul_overflow((long)(nb - 1), B->l_c, &extent) &&
                    !__builtin_add_overflow(extent, (long)B->n_bands, &extent) &&
                    sc_one_to_one(n_groups, rows, extent, B->l_g, B->l_s), BAS_E_SHAPE,
                    "%s: logmag output strides (%ld, %ld, %ld, 1) overlap for [%d][%ld][%d][%d]", fn, B->l_g, B->l_s, B->l_c,
                    n_groups, rows, nb, B->n_bands);
        BAS_REQUIRE(B->logmag, BAS_E_NULL, "%s: null pointer", fn);
        BAS_REQUIRE((void *)B->logmag != elev && (void *)B->logmag != azim && (void *)B->logmag != gain &&
                    (void *)B->logmag != delay, BAS_E_SHAPE, "%s: two outputs are one buffer", fn);
        BAS_REQUIRE(bas_aligned(B->orient, 8) && bas_aligned(B->pattern, 8) && bas_aligned(B->air, 8) &&
                    bas_aligned(B->img_logmag, 8) && bas_aligned(B->logmag, 8), BAS_E_ALIGN,
                    "%s: float64 arrays must be 8-byte aligned (images: 4-byte)", fn);
        A.orient = B->orient; A.o_g = B->o_g; A.o_s = B->o_s; A.o_c = B->o_c;
        A.pattern = B->pattern; A.pt_s = B->pt_s; A.air = B->air; A.img_logmag = B->img_logmag;
        A.n_bands = B->n_bands; A.floor = B->floor;
        A.logmag = B->logmag; A.l_g = B->l_g; A.l_s = B->l_s; A.l_c = B->l_c;
        if (B->occluded) {
            BAS_REQUIRE(B->n_screens >= 1 && B->n_screens <= BAS_OCCLUDE_MAX_SCREENS, BAS_E_SHAPE,
                        "%s: n_screens (%d) must be in 1..%d", fn, B->n_screens, BAS_OCCLUDE_MAX_SCREENS);
            BAS_REQUIRE(B->t_s == 0 || B->t_s >= B->n_bands, BAS_E_SHAPE,
                        "%s: the transmission's screen stride (%ld) must be 0 (shared) or >= n_bands", fn, B->t_s);
            BAS_REQUIRE(B->screens && B->fresnel, BAS_E_NULL, "%s: null pointer (screens, fresnel)", fn);
            BAS_REQUIRE(bas_aligned(B->screens, 8) && bas_aligned(B->transmission, 8) && bas_aligned(B->fresnel, 8),
                        BAS_E_ALIGN,
                        "%s: float64 arrays must be 8-byte aligned (images: 4-byte)", fn);
            AO.scr.screens = B->screens; AO.scr.transmission = B->transmission; AO.scr.fresnel = B->fresnel;
            AO.scr.t_s = B->t_s; AO.scr.n_screens = B->n_screens; AO.scr.n_bands = B->n_bands;
        }
    }
    A.pos = pos; A.ps_g = pos_stride_g; A.ps_s = pos_stride_s; A.ps_c = pos_stride_c;
    A.prev = pos_prev; A.pp_g = prev_stride_g; A.pp_s = prev_stride_s; A.spc = samples_per_chunk;
    A.lpos = lpos; A.lp_g = lpos_stride_g; A.lp_c = lpos_stride_c;
    A.head = head; A.h_g = head_stride_g; A.h_c = head_stride_c;
    A.src_gain = src_gain; A.sg_g = sg_stride_g; A.sg_s = sg_stride_s;
    A.room_size = room_size; A.images = images; A.img_gain = img_gain;
    A.spm = samples_per_metre; A.r_ref = r_ref; A.dmin = d_min; A.dmax = d_max;
    A.n_src = n_src; A.n_img = n_img; A.nb = nb;
    A.elev = elev; A.azim = azim; A.gain = gain; A.a_g = a_stride_g; A.a_s = a_stride_s;
    A.delay = delay; A.d_g = d_stride_g; A.d_s = d_stride_s;
    const long n_items = (long)n_groups * rows * nb;
    const int blocks = bas_grid_for(n_items, 8 * bas_device_cus());
    if (B && B->occluded)
        hipLaunchKernelGGL(bas_scene_params_kernel<SC_SCREENS>, dim3(blocks), dim3(SC_THREADS), 0, bas_stream(stream), AO, n_items);
    else if (B)
        hipLaunchKernelGGL(bas_scene_params_kernel<SC_BANDS>, dim3(blocks), dim3(SC_THREADS), 0, bas_stream(stream), A, n_items);
    else
        hipLaunchKernelGGL(bas_scene_params_kernel<SC_PLAIN>, dim3(blocks), dim3(SC_THREADS), 0, bas_stream(stream), A, n_items);
    return bas_check_launch(fn);
}

extern "C" int bas_scene_params_f64(const double *pos, long pos_stride_g, long pos_stride_s, long pos_stride_c,
                                    const double *pos_prev, long prev_stride_g, long prev_stride_s,
                                    double samples_per_chunk, const double *lpos, long lpos_stride_g,
                                    long lpos_stride_c, const double *head,
                                    long head_stride_g, long head_stride_c, const double *src_gain, long sg_stride_g,
                                    long sg_stride_s, const double *room_size, const int32_t *images,
                                    const double *img_gain, int n_img, double samples_per_metre, double r_ref,
                                    double d_min, double d_max, int n_groups, int n_src, int nb, double *elev,
                                    double *azim, double *gain, long a_stride_g, long a_stride_s, double *delay,
                                    long d_stride_g, long d_stride_s, bas_stream_t stream) {
    return sc_launch("bas_scene_params_f64", pos, pos_stride_g, pos_stride_s, pos_stride_c, pos_prev, prev_stride_g,
                     prev_stride_s, samples_per_chunk, lpos, lpos_stride_g, lpos_stride_c, head, head_stride_g,
                     head_stride_c, src_gain, sg_stride_g, sg_stride_s, room_size, images, img_gain, n_img,
                     samples_per_metre, r_ref, d_min, d_max, n_groups, n_src, nb, elev, azim, gain, a_stride_g, a_stride_s,
                     delay, d_stride_g, d_stride_s, nullptr, stream);
}

extern "C" int bas_scene_params_bands_f64(const double *pos, long pos_stride_g, long pos_stride_s, long pos_stride_c,
                                          const double *pos_prev, long prev_stride_g, long prev_stride_s,
                                          double samples_per_chunk, const double *lpos, long lpos_stride_g,
                                          long lpos_stride_c, const double *head, long head_stride_g, long head_stride_c,
                                          const double *src_gain, long sg_stride_g, long sg_stride_s,
                                          const double *room_size, const int32_t *images, const double *img_gain,
                                          int n_img, double samples_per_metre, double r_ref, double d_min, double d_max,
                                          int n_groups, int n_src, int nb, const double *orient, long orient_stride_g,
                                          long orient_stride_s, long orient_stride_c, const double *pattern,
                                          long pattern_stride_s, const double *air, const double *img_logmag, int n_bands,
                                          double floor, double *elev, double *azim, double *gain, long a_stride_g,
                                          long a_stride_s, double *delay, long d_stride_g, long d_stride_s, double *logmag,
                                          long l_stride_g, long l_stride_s, long l_stride_c, bas_stream_t stream) {
    const BasSceneBands B = {orient, orient_stride_g, orient_stride_s, orient_stride_c, pattern, pattern_stride_s, air,
                             img_logmag, n_bands, floor, logmag, l_stride_g, l_stride_s, l_stride_c, false, nullptr, nullptr,
                             0, nullptr, 0};
    return sc_launch("bas_scene_params_bands_f64", pos, pos_stride_g, pos_stride_s, pos_stride_c, pos_prev, prev_stride_g,
                     prev_stride_s, samples_per_chunk, lpos, lpos_stride_g, lpos_stride_c, head, head_stride_g,
                     head_stride_c, src_gain, sg_stride_g, sg_stride_s, room_size, images, img_gain, n_img,
                     samples_per_metre, r_ref, d_min, d_max, n_groups, n_src, nb, elev, azim, gain, a_stride_g, a_stride_s,
                     delay, d_stride_g, d_stride_s, &B, stream);
}

extern "C" int bas_scene_params_occluded_f64(const double *pos, long pos_stride_g, long pos_stride_s, long pos_stride_c,
                                             const double *pos_prev, long prev_stride_g, long prev_stride_s,
                                             double samples_per_chunk, const double *lpos, long lpos_stride_g,
                                             long lpos_stride_c, const double *head, long head_stride_g, long head_stride_c,
                                             const double *src_gain, long sg_stride_g, long sg_stride_s,
                                             const double *room_size, const int32_t *images, const double *img_gain,
                                             int n_img, double samples_per_metre, double r_ref, double d_min, double d_max,
                                             int n_groups, int n_src, int nb, const double *orient, long orient_stride_g,
                                             long orient_stride_s, long orient_stride_c, const double *pattern,
                                             long pattern_stride_s, const double *air, const double *img_logmag, int n_bands,
                                             double floor, const double *screens, const double *transmission,
                                             long transmission_stride_s, const double *fresnel, int n_screens, double *elev,
                                             double *azim, double *gain, long a_stride_g, long a_stride_s, double *delay,
                                             long d_stride_g, long d_stride_s, double *logmag, long l_stride_g,
                                             long l_stride_s, long l_stride_c, bas_stream_t stream) {
    const BasSceneBands B = {orient, orient_stride_g, orient_stride_s, orient_stride_c, pattern, pattern_stride_s, air,
                             img_logmag, n_bands, floor, logmag, l_stride_g, l_stride_s, l_stride_c, true, screens,
                             transmission, transmission_stride_s, fresnel, n_screens};
    return sc_launch("bas_scene_params_occluded_f64", pos, pos_stride_g, pos_stride_s, pos_stride_c, pos_prev, prev_stride_g,
                     prev_stride_s, samples_per_chunk, lpos, lpos_stride_g, lpos_stride_c, head, head_stride_g,
                     head_stride_c, src_gain, sg_stride_g, sg_stride_s, room_size, images, img_gain, n_img,
                     samples_per_metre, r_ref, d_min, d_max, n_groups, n_src, nb, elev, azim, gain, a_stride_g, a_stride_s,
                     delay, d_stride_g, d_stride_s, &B, stream);
}
