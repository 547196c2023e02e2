// The host half of screens (include/bas.h "screens") under AddressSanitizer and
// UndefinedBehaviorSanitizer, stand-alone: `make -C binaural-audio-synthesis_amd/csrc hostsan_occlude` links this file with
// the library's objects (host code sanitized, device code as shipped).  Three parts:
//   1. bas_scene_params_occluded_f64: valid argument lists, which with no device to run on return a positive hipError_t,
//      and the violations, each of which returns the code bas.h documents and leaves a text naming the entry point.  The
//      pointers are never dereferenced by the host code.
//   2. the host build of bas_occlude.h (the edge minimiser, the signed detour, the band term, the sum over screens and
//      mirrored cells) against a restatement in long double: the edge by a golden-section search instead of the closed form,
//      the copies placed by reflecting the screen cell by cell instead of by the parity rule.
//   3. `hostsan_occlude paths IN OUT`: the same host build for the Python tests - IN holds int32 n_bands, n_screens, n_paths,
//      has_room, has_transmission, then float64 room [3], fresnel [n_bands], screens [n_screens][9], transmission
//      [n_screens][n_bands] (if any), q [n_paths][3], l [n_paths][3], then int32 images [n_paths][3]; OUT receives float64
//      sums [n_paths][n_bands] and signed detours of the first screen's copy in cell 0 [n_paths] (NaN: not crossed).
// Exits 77 where a GPU is visible.
#include <cmath>
#include <vector>

#define HOSTSAN_NAME "hostsan_occlude"
#include "hostsan_common.h"
#include "../../binaural-audio-synthesis_amd/csrc/bas_occlude.h"

struct Occluded {
    const double *pos;
    long ps_g, ps_s, ps_c;
    const double *room_size;
    const int32_t *images;
    const double *img_gain;
    int n_img, G, n_src, nb;
    const double *orient;
    long o_g, o_s, o_c;
    const double *pattern;
    long pt_s;
    const double *air, *lnw;
    int n_bands;
    double floor;
    const double *screens, *transmission;
    long t_s;
    const double *fresnel;
    int n_screens;
    double *elev, *azim, *gain;
    long a_g, a_s;
    double *delay;
    long d_g, d_s;
    double *logmag;
    long l_g, l_s, l_c;
    int call() const {
        return bas_scene_params_occluded_f64(pos, ps_g, ps_s, ps_c, nullptr, 0, 0, 0.0, nullptr, 0, 0, nullptr, 0, 0, nullptr, 0,
                                             0, room_size, images, img_gain, n_img, 128.0, 1.0, 2.0, 1e4, G, n_src, nb, orient,
                                             o_g, o_s, o_c, pattern, pt_s, air, lnw, n_bands, floor, screens, transmission, t_s,
                                             fresnel, n_screens, elev, azim, gain, a_g, a_s, delay, d_g, d_s, logmag, l_g, l_s,
                                             l_c, nullptr);
    }
};

static void entry_section() {
    static const char *N = "bas_scene_params_occluded_f64";
    const uintptr_t p = uintptr_t(1) << 32;                                  // made-up device addresses, 64-byte aligned
    const int G = 2, n_src = 5, n_img = 7, nb = 9, n_bands = 6, n_screens = 3;
    const long rows = (long)n_src * n_img;
    const Occluded ok = {at<const double>(p, 0), (long)n_src * nb * 3, (long)nb * 3, 3, at<const double>(p, 1 << 20),
                         at<const int32_t>(p, 2 << 20), at<const double>(p, 3 << 20), n_img, G, n_src, nb,
                         at<const double>(p, 4 << 20), (long)n_src * nb * 4, (long)nb * 4, 4, at<const double>(p, 5 << 20),
                         n_bands, at<const double>(p, 6 << 20), at<const double>(p, 7 << 20), n_bands, 1e-6,
                         at<const double>(p, 13 << 20), at<const double>(p, 14 << 20), n_bands, at<const double>(p, 15 << 20),
                         n_screens, at<double>(p, 8 << 20), at<double>(p, 9 << 20), at<double>(p, 10 << 20), rows * nb, nb,
                         at<double>(p, 11 << 20), rows * nb, nb, at<double>(p, 12 << 20), rows * nb * n_bands,
                         (long)nb * n_bands, n_bands};
    Occluded a;
    EXPECT("valid arguments, no device", ok.call(), NO_DEVICE, N);
    a = ok; a.transmission = nullptr; a.t_s = 0;
    EXPECT("opaque screens, no device", a.call(), NO_DEVICE, N);
    a = ok; a.t_s = 0;
    EXPECT("one transmission for all screens, no device", a.call(), NO_DEVICE, N);
    a = ok; a.t_s = n_bands + 3;
    EXPECT("padded transmission rows, no device", a.call(), NO_DEVICE, N);
    a = ok; a.n_screens = 32;
    EXPECT("the most screens, no device", a.call(), NO_DEVICE, N);
    a = ok; a.n_screens = 1;
    EXPECT("one screen, no device", a.call(), NO_DEVICE, N);
    a = ok; a.room_size = nullptr; a.images = nullptr; a.img_gain = nullptr; a.n_img = 1; a.lnw = nullptr;
    a.a_g = (long)n_src * nb; a.d_g = a.a_g; a.l_g = (long)n_src * nb * n_bands;
    EXPECT("screens in the free field, no device", a.call(), NO_DEVICE, N);
    a = ok; a.orient = nullptr; a.pattern = nullptr; a.air = nullptr; a.lnw = nullptr; a.o_g = a.o_s = a.o_c = a.pt_s = 0;
    EXPECT("screens alone, no device", a.call(), NO_DEVICE, N);
    // ---- what the launcher of the three entries refuses holds here too (a sample)
    a = ok; a.pos = nullptr; EXPECT("pos null", a.call(), E_NULL, N);
    a = ok; a.elev = nullptr; EXPECT("elev null", a.call(), E_NULL, N);
    a = ok; a.logmag = nullptr; EXPECT("logmag null", a.call(), E_NULL, N);
    a = ok; a.images = nullptr; EXPECT("a room without images", a.call(), E_NULL, N);
    a = ok; a.nb = 0; EXPECT("nb 0", a.call(), E_SHAPE, N);
    a = ok; a.room_size = nullptr; EXPECT("free field with 7 images", a.call(), E_SHAPE, N);
    a = ok; a.a_s = nb - 1; EXPECT("angle rows overlap", a.call(), E_SHAPE, N);
    a = ok; a.azim = a.elev; EXPECT("azim == elev", a.call(), E_SHAPE, N);
    a = ok; a.logmag = a.gain; EXPECT("logmag == gain", a.call(), E_SHAPE, N);
    a = ok; a.pos = at<const double>(p, 4); EXPECT("pos misaligned", a.call(), E_ALIGN, N);
    for (int n : {0, -1, 17}) { a = ok; a.n_bands = n; EXPECT("n_bands", a.call(), E_SHAPE, N); }
    for (double f : {0.0, -1e-6, 1.5, (double)NAN}) { a = ok; a.floor = f; EXPECT("floor", a.call(), E_SHAPE, N); }
    a = ok; a.pt_s = n_bands - 1; EXPECT("pattern rows overlap", a.call(), E_SHAPE, N);
    a = ok; a.l_c = n_bands - 1; EXPECT("boundaries' bands overlap", a.call(), E_SHAPE, N);
    for (int i = 0; i < 7; ++i) {
        a = ok;
        long *f[7] = {&a.o_g, &a.o_s, &a.o_c, &a.pt_s, &a.l_g, &a.l_s, &a.l_c};
        *f[i] = -1;
        EXPECT("negative stride", a.call(), E_SHAPE, N);
    }
    // ---- the new arguments
    a = ok; a.screens = nullptr; EXPECT("screens null", a.call(), E_NULL, N);
    a = ok; a.fresnel = nullptr; EXPECT("fresnel null", a.call(), E_NULL, N);
    for (int n : {0, -1, 33, 1 << 30}) { a = ok; a.n_screens = n; EXPECT("n_screens", a.call(), E_SHAPE, N); }
    for (long t : {-1L, 1L, (long)n_bands - 1, -(long)n_bands}) {
        a = ok; a.t_s = t; EXPECT("transmission stride", a.call(), E_SHAPE, N);
    }
    a = ok; a.screens = at<const double>(p, (13 << 20) + 4); EXPECT("screens misaligned", a.call(), E_ALIGN, N);
    a = ok; a.transmission = at<const double>(p, (14 << 20) + 2); EXPECT("transmission misaligned", a.call(), E_ALIGN, N);
    a = ok; a.fresnel = at<const double>(p, (15 << 20) + 1); EXPECT("fresnel misaligned", a.call(), E_ALIGN, N);
}

// ---- part 2: bas_occlude.h's host build against a restatement ------------------------------------------------------------
typedef long double ld;
struct V3 { ld x, y, z; };
static V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V3 mul(V3 a, ld s) { return {a.x * s, a.y * s, a.z * s}; }
static ld dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static ld norm(V3 a) { return sqrtl(dot(a, a)); }
static V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// min over t in [0, 1] of |q - P(t)| + |P(t) - l| by golden-section search (the sum is convex in t)
static ld edge_search(V3 q, V3 l, V3 A, V3 B) {
    const ld g = (sqrtl(5.0L) - 1) / 2;
    ld lo = 0, hi = 1;
    auto f = [&](ld t) { const V3 P = add(A, mul(sub(B, A), t)); return norm(sub(q, P)) + norm(sub(P, l)); };
    ld x1 = hi - g * (hi - lo), x2 = lo + g * (hi - lo), f1 = f(x1), f2 = f(x2);
    for (int it = 0; it < 200; ++it) {
        if (f1 < f2) { hi = x2; x2 = x1; f2 = f1; x1 = hi - g * (hi - lo); f1 = f(x1); }
        else { lo = x1; x1 = x2; f1 = f2; x2 = lo + g * (hi - lo); f2 = f(x2); }
    }
    return fminl(fminl(f1, f2), fminl(f(0), f(1)));
}

// the signed detour of one screen copy; returns false where the ends do not lie on opposite sides
static bool detour_restated(V3 q, V3 l, V3 c, V3 e1, V3 e2, ld *sd, ld *margin) {
    const V3 n = cross(e1, e2);
    const ld sq = dot(n, sub(q, c)), sl = dot(n, sub(l, c));
    *margin = fminl(fabsl(sq), fabsl(sl)) / norm(n);
    if (!(sq * sl < 0)) return false;
    const V3 h = sub(add(q, mul(sub(l, q), sq / (sq - sl))), c);
    const ld a = dot(h, e1) / dot(e1, e1), b = dot(h, e2) / dot(e2, e2);
    const V3 mm = sub(sub(c, e1), e2), pm = sub(add(c, e1), e2), mp = add(sub(c, e1), e2), pp = add(add(c, e1), e2);
    ld best = edge_search(q, l, mm, pm);
    best = fminl(best, edge_search(q, l, mp, pp));
    best = fminl(best, edge_search(q, l, mm, mp));
    best = fminl(best, edge_search(q, l, pm, pp));
    const ld delta = fmaxl(best - norm(sub(q, l)), 0);
    *sd = fabsl(a) <= 1 && fabsl(b) <= 1 ? delta : -delta;
    *margin = fminl(*margin, fminl(fabsl(fabsl(a) - 1), fabsl(fabsl(b) - 1)));    // (distance to a switch of the sign)
    return true;
}

static ld logmag_restated(ld sd, ld fresnel, ld T) {
    const ld N = fresnel * sd, two_pi = 2 * acosl(-1.0L);
    ld A = 0;
    if (N >= 0) {
        const ld x = sqrtl(two_pi * N);
        A = fminl(5 + 20 * log10l(x == 0 ? 1 : x / tanhl(x)), 24);
    } else if (N > -0.2L) {
        const ld x = sqrtl(two_pi * -N);
        A = fmaxl(5 + 20 * log10l(x / tanl(x)), 0);
    }
    return logl(T + (1 - T) * powl(10, -A / 20));
}

// the screen reflected in the walls between cell 0 and cell i of one axis, one wall at a time
static void reflect_axis(ld L, int i, ld *c, ld *e1, ld *e2) {
    const int step = i < 0 ? -1 : 1;
    for (int k = 0; k != i; k += step) {
        const ld wall = step > 0 ? (k + 1) * L : k * L;                      // the wall between cell k and cell k + step
        *c = 2 * wall - *c;
        *e1 = -*e1;
        *e2 = -*e2;
    }
}


static void note(bool ok, const char *what, int i, double got, double want) {
    ++g_checks;
    if (!ok && ++g_fail <= 40) fprintf(stderr, "hostsan_occlude: FAIL %s case %d: got %.17g, want %.17g\n", what, i, got, want);
}

static double edge_section() {
    double worst = 0.0;
    for (int i = 0; i < 2000; ++i) {
        double v[12];
        for (double &x : v) x = between(-5.0, 5.0);
        if (i % 7 == 0) { v[0] = v[6] + 0.3 * (v[9] - v[6]); v[1] = v[7] + 0.3 * (v[10] - v[7]); v[2] = v[8] + 0.3 * (v[11] - v[8]); }
        const double got = bas_occlude_edge(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]);
        const ld want = edge_search({v[0], v[1], v[2]}, {v[3], v[4], v[5]}, {v[6], v[7], v[8]}, {v[9], v[10], v[11]});
        const double err = (double)fabsl(got - want);
        if (err > worst) worst = err;
        note(err <= 1e-9, "edge", i, got, (double)want);                     // (the search resolves t to 1e-9 of the edge or so)
    }
    // both ends on the edge's line: the midpoint rule (d_q + d_l == 0), inside and clamped
    note(bas_occlude_edge(-1, 0, 0, 3, 0, 0, 0, 0, 0, 2, 0, 0) == 4.0, "edge on the line", 0, 0, 4);
    note(bas_occlude_edge(5, 0, 0, 7, 0, 0, 0, 0, 0, 2, 0, 0) == 8.0, "edge on the line, clamped", 1, 0, 8);
    // t* beyond a corner: the corner is the point
    note(std::fabs(bas_occlude_edge(5, 1, 0, 6, -1, 0, 0, 0, 0, 2, 0, 0) - (std::hypot(3.0, 1.0) + std::hypot(4.0, 1.0))) <= 1e-15,
         "edge clamped at a corner", 2, 0, 0);
    return worst;
}

static double sum_section(double *worst_sd) {
    double worst = 0.0;
    *worst_sd = 0.0;
    const double room[3] = {6.0, 5.0, 4.0};
    for (int i = 0; i < 600; ++i) {
        const int n_bands = 1 + (int)(uniform() * 16) % 16, n_screens = 1 + (int)(uniform() * 4);
        const bool in_room = i % 3 != 0, has_T = i % 4 != 0;
        std::vector<double> scr(9 * n_screens), T((size_t)n_screens * n_bands), fres(n_bands);
        for (int b = 0; b < n_bands; ++b) fres[b] = 2.0 * 62.5 * std::pow(2.0, 0.5 * b) / 343.0;
        for (int k = 0; k < n_screens; ++k) {
            double *s = &scr[9 * k];
            for (int a = 0; a < 3; ++a) s[a] = between(0.3 * room[a], 0.7 * room[a]);
            // two orthogonal half-edges that keep the rectangle inside the room
            const double th = between(0.0, 6.28), ph = between(-1.0, 1.0), u = between(0.2, 0.6), w = between(0.2, 0.6);
            const double e1[3] = {std::cos(th) * std::cos(ph), std::sin(th) * std::cos(ph), std::sin(ph)};
            const double e2[3] = {-std::sin(th), std::cos(th), 0.0};
            for (int a = 0; a < 3; ++a) { s[3 + a] = u * e1[a]; s[6 + a] = w * e2[a]; }
            for (int b = 0; b < n_bands; ++b) T[(size_t)k * n_bands + b] = (i % 8 == 1) ? 1.0 : between(0.0, 1.0);
        }
        int m[3] = {0, 0, 0};
        if (in_room) {
            const int order = 1 + i % 3;
            do { for (int &v : m) v = (int)(uniform() * 7) - 3; } while (std::abs(m[0]) + std::abs(m[1]) + std::abs(m[2]) > order);
        }
        double p[3], l[3], q[3];
        for (int a = 0; a < 3; ++a) {
            p[a] = between(0.05 * room[a], 0.95 * room[a]);
            l[a] = between(0.05 * room[a], 0.95 * room[a]);
            q[a] = in_room ? m[a] * room[a] + ((m[a] & 1) ? room[a] - p[a] : p[a]) : p[a] + (i % 2 ? 7.0 : 0.0);
        }
        double acc[BAS_OCCLUDE_MAX_BANDS];
        for (double &v : acc) v = 0.0;
        const BasOccludeScreens W = {scr.data(), has_T ? T.data() : nullptr, fres.data(), n_bands, n_screens, n_bands};
        bas_occlude_sum(W, q[0], q[1], q[2], l[0], l[1], l[2], in_room, room[0], room[1], room[2], m[0], m[1], m[2], acc);
        // the restatement: reflect, test, search
        std::vector<ld> want(n_bands, 0);
        ld margin = 1;
        for (int k = 0; k < n_screens; ++k)
            for (int ia = 0; ia <= std::abs(m[0]); ++ia)
                for (int ja = 0; ja <= std::abs(m[1]); ++ja)
                    for (int ka = 0; ka <= std::abs(m[2]); ++ka) {
                        const int cell[3] = {m[0] < 0 ? -ia : ia, m[1] < 0 ? -ja : ja, m[2] < 0 ? -ka : ka};
                        ld c[3], e1[3], e2[3];
                        for (int a = 0; a < 3; ++a) {
                            c[a] = scr[9 * k + a]; e1[a] = scr[9 * k + 3 + a]; e2[a] = scr[9 * k + 6 + a];
                            reflect_axis(room[a], cell[a], &c[a], &e1[a], &e2[a]);
                        }
                        ld sd, mg;
                        const bool crossed = detour_restated({q[0], q[1], q[2]}, {l[0], l[1], l[2]}, {c[0], c[1], c[2]},
                                                             {e1[0], e1[1], e1[2]}, {e2[0], e2[1], e2[2]}, &sd, &mg);
                        margin = fminl(margin, mg);
                        if (!crossed) continue;
                        if (k == 0 && ia + ja + ka == 0) {
                            double got_sd = 0.0;
                            const double *s = &scr[0];
                            if (bas_occlude_detour(q[0], q[1], q[2], l[0], l[1], l[2], s[0], s[1], s[2], s[3], s[4], s[5], s[6],
                                                   s[7], s[8], &got_sd) && mg > 1e-6) {
                                const double e = (double)fabsl(got_sd - sd);
                                if (e > *worst_sd) *worst_sd = e;
                                note(e <= 1e-9, "signed detour", i, got_sd, (double)sd);
                            }
                        }
                        for (int b = 0; b < n_bands; ++b)
                            want[b] += logmag_restated(sd, fres[b], has_T ? (ld)T[(size_t)k * n_bands + b] : 0);
                    }
        if (margin <= 1e-6) continue;                                        // (within rounding of a discontinuity: not compared)
        for (int b = 0; b < n_bands; ++b) {
            const double e = (double)fabsl(acc[b] - want[b]);
            if (e > worst) worst = e;
            // dL/d delta <= (4 pi / 3) fresnel / 2 .. per copy; the search leaves 1e-9 m in delta at most: 1e-7 is ample
            note(e <= 1e-7, "sum of ln M", i, acc[b], (double)want[b]);
            if (i % 8 == 1 && has_T) note(acc[b] == 0.0, "T == 1 gives exactly 0", i, acc[b], 0.0);
        }
        for (int b = n_bands; b < BAS_OCCLUDE_MAX_BANDS; ++b) note(acc[b] == 0.0, "bands past n_bands stay 0", i, acc[b], 0.0);
    }
    // the curve's fixed points
    note(std::fabs(bas_occlude_logmag(0.0, 5.83, 0.0) * (-20.0 / std::log(10.0)) - 5.0) <= 1e-14, "A(0)", 0, 0, 5);
    note(bas_occlude_logmag(-0.2, 1.0, 0.0) == 0.0, "A(-0.2)", 0, bas_occlude_logmag(-0.2, 1.0, 0.0), 0);
    note(bas_occlude_logmag(-5.0, 1.0, 0.0) == 0.0, "A(-5)", 0, 0, 0);
    note(std::fabs(bas_occlude_logmag(50.0, 1.0, 0.0) * (-20.0 / std::log(10.0)) - 24.0) <= 1e-13, "A(50)", 0, 0, 24);
    note(bas_occlude_logmag(3.0, 1.0, 1.0) == 0.0, "T = 1", 0, 0, 0);
    return worst;
}

// ---- part 3: the host build for the Python tests ------------------------------------------------------------------------
static int paths_file(const char *in_path, const char *out_path) {
    FILE *in = fopen(in_path, "rb");
    if (!in) return 2;
    int32_t dims[5];
    if (fread(dims, sizeof(int32_t), 5, in) != 5) { fclose(in); return 2; }
    const int n_bands = dims[0], n_screens = dims[1], n = dims[2];
    const bool has_room = dims[3] != 0, has_T = dims[4] != 0;
    if (n_bands < 1 || n_bands > BAS_OCCLUDE_MAX_BANDS || n_screens < 1 || n_screens > BAS_OCCLUDE_MAX_SCREENS || n < 0 ||
        n > (1 << 22)) {
        fclose(in);
        return 2;
    }
    double room[3];
    std::vector<double> fres(n_bands), scr((size_t)9 * n_screens), T(has_T ? (size_t)n_screens * n_bands : 0), q((size_t)3 * n),
        l((size_t)3 * n);
    std::vector<int32_t> m((size_t)3 * n);
    const bool read = fread(room, sizeof(double), 3, in) == 3 && fread(fres.data(), sizeof(double), fres.size(), in) == fres.size() &&
                      fread(scr.data(), sizeof(double), scr.size(), in) == scr.size() &&
                      fread(T.data(), sizeof(double), T.size(), in) == T.size() &&
                      fread(q.data(), sizeof(double), q.size(), in) == q.size() &&
                      fread(l.data(), sizeof(double), l.size(), in) == l.size() &&
                      fread(m.data(), sizeof(int32_t), m.size(), in) == m.size();
    fclose(in);
    if (!read) return 2;
    for (int i = 0; i < 3 * n; ++i)
        if (m[i] < -3 || m[i] > 3) return 2;
    std::vector<double> sums((size_t)n * n_bands), sds(n);
    const BasOccludeScreens W = {scr.data(), has_T ? T.data() : nullptr, fres.data(), n_bands, n_screens, n_bands};
    for (int i = 0; i < n; ++i) {
        double acc[BAS_OCCLUDE_MAX_BANDS];
        for (double &v : acc) v = 0.0;
        const double *qi = &q[(size_t)3 * i], *li = &l[(size_t)3 * i];
        bas_occlude_sum(W, qi[0], qi[1], qi[2], li[0], li[1], li[2], has_room, room[0], room[1], room[2], m[3 * i], m[3 * i + 1],
                        m[3 * i + 2], acc);
        for (int b = 0; b < n_bands; ++b) sums[(size_t)i * n_bands + b] = acc[b];
        double sd = 0.0;
        sds[i] = bas_occlude_detour(qi[0], qi[1], qi[2], li[0], li[1], li[2], scr[0], scr[1], scr[2], scr[3], scr[4], scr[5], scr[6],
                                    scr[7], scr[8], &sd) ? sd : (double)NAN;
    }
    FILE *out = fopen(out_path, "wb");
    if (!out) return 2;
    const bool wrote = fwrite(sums.data(), sizeof(double), sums.size(), out) == sums.size() &&
                       fwrite(sds.data(), sizeof(double), sds.size(), out) == sds.size();
    return fclose(out) == 0 && wrote ? 0 : 2;
}

int main(int argc, char **argv) {
    if (hostsan_gpu_visible("hostsan_occlude")) return 77;
    if (argc == 4 && strcmp(argv[1], "paths") == 0) return paths_file(argv[2], argv[3]);
    entry_section();
    const int after_entry = g_checks;
    const double worst_edge = edge_section();
    const int after_edge = g_checks;
    double worst_sd = 0.0;
    const double worst_sum = sum_section(&worst_sd);
    printf("hostsan_occlude: bas_scene_params_occluded_f64 %d checks, bas_occlude_edge %d checks (worst %.3e m), "
           "bas_occlude_sum %d checks (worst detour %.3e m, worst ln M sum %.3e), %d failed\n", after_entry,
           after_edge - after_entry, worst_edge, g_checks - after_edge, worst_sd, worst_sum, g_fail);
    printf("hostsan_occlude: %s\n", g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}
