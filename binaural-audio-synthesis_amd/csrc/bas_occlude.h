// Occlusion and edge diffraction by screens (include/bas.h "screens"): the arithmetic of one straight path
// q -> l against one copy of one screen (a thin rectangle: centre c, half-edge vectors e1, e2), in binary64 with
// floating-point contraction off.  One set of functions for the scene kernel (bas_scene.hip) and for a host build
// (tests/hostsan), so that the arithmetic can be checked on a machine without a GPU; scene.occlusion_logmag is the numpy
// statement of the same expressions in the same order.
//
//   bas_occlude_mirror   the copy of a screen in the cell of index i along one axis (bas_scene_point's mirror rule)
//   bas_occlude_edge     the shortest path q -> P -> l over the points P of one edge segment
//   bas_occlude_detour   the side test, the hit point and, only where the ends lie on opposite sides, the four edges:
//                        the signed detour, + delta where the path is blocked, - delta where it is lit
//   bas_occlude_logmag   one band's ln M from the signed detour (Kurze-Anderson, continued into the lit zone)
//   bas_occlude_sum      one path against every screen and, in a room, every copy: the sum of ln M per band
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define BAS_OCCLUDE_MAX_SCREENS 32
#define BAS_OCCLUDE_MAX_BANDS 16
#define BAS_OCCLUDE_TWO_PI 6.283185307179586
#define BAS_OCCLUDE_NEPERS_PER_DB 0.11512925464970229                      // ln 10 / 20

// Component a of a screen's copy in the cell i along that axis of a room of size L: c' = i L + (i odd ? L - c : c), and
// the half-edges' components change sign where i is odd.  i == 0 keeps every bit.
__host__ __device__ inline void bas_occlude_mirror(double L, int i, double *c, double *e1, double *e2) {
#pragma clang fp contract(off)
    if (i & 1) {
        *c = (double)i * L + (L - *c);
        *e1 = -*e1;
        *e2 = -*e2;
    } else {
        *c = (double)i * L + *c;
    }
}

// The least of |q - P| + |P - l| over the points P of the segment from A to B (A != B).  With u the edge's direction,
// t the coordinate along it and d the distance from its line: the sum hypot(d_q, t - t_q) + hypot(d_l, t - t_l) is convex
// in t, least at t* = t_q + (t_l - t_q) d_q / (d_q + d_l) (the midpoint where both ends lie on the line), and the clamp
// of t* to the segment is therefore exact.
__host__ __device__ inline double bas_occlude_edge(double qx, double qy, double qz, double lx, double ly, double lz,
                                                   double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = bx - ax, dy = by - ay, dz = bz - az;
    const double len = sqrt(dx * dx + dy * dy + dz * dz);
    const double ux = dx / len, uy = dy / len, uz = dz / len;
    const double qax = qx - ax, qay = qy - ay, qaz = qz - az;
    const double lax = lx - ax, lay = ly - ay, laz = lz - az;
    const double tq = qax * ux + qay * uy + qaz * uz;
    const double tl = lax * ux + lay * uy + laz * uz;
    const double wqx = qax - tq * ux, wqy = qay - tq * uy, wqz = qaz - tq * uz;
    const double wlx = lax - tl * ux, wly = lay - tl * uy, wlz = laz - tl * uz;
    const double dq = sqrt(wqx * wqx + wqy * wqy + wqz * wqz);
    const double dl = sqrt(wlx * wlx + wly * wly + wlz * wlz);
    const double ds = dq + dl;
    double ts = ds == 0.0 ? 0.5 * (tq + tl) : tq + (tl - tq) * dq / ds;
    ts = fmin(fmax(ts, 0.0), len);
    return hypot(dq, ts - tq) + hypot(dl, ts - tl);
}

// One path against one screen copy.  n = e1 x e2, s_q = n.(q - c), s_l = n.(l - c).  Unless s_q s_l < 0 the ends lie on
// one side or in the plane: returns false (the screen contributes exactly 0) and leaves *sd alone.  Otherwise the hit
// point h = q + (s_q / (s_q - s_l)) (l - q), its coordinates a = (h - c).e1 / |e1|^2, b = (h - c).e2 / |e2|^2, blocked
// where |a| <= 1 and |b| <= 1; delta = max(min over the four edges of bas_occlude_edge - |q - l|, 0); *sd = + delta where
// blocked, - delta where lit; returns true.
__host__ __device__ inline bool bas_occlude_detour(double qx, double qy, double qz, double lx, double ly, double lz,
                                                   double cx, double cy, double cz, double e1x, double e1y, double e1z,
                                                   double e2x, double e2y, double e2z, double *sd) {
#pragma clang fp contract(off)
    const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
    const double sq = nx * (qx - cx) + ny * (qy - cy) + nz * (qz - cz);
    const double sl = nx * (lx - cx) + ny * (ly - cy) + nz * (lz - cz);
    if (!(sq * sl < 0.0)) return false;
    const double vx = lx - qx, vy = ly - qy, vz = lz - qz;
    const double t = sq / (sq - sl);
    const double hx = (qx + t * vx) - cx, hy = (qy + t * vy) - cy, hz = (qz + t * vz) - cz;
    const double a = (hx * e1x + hy * e1y + hz * e1z) / (e1x * e1x + e1y * e1y + e1z * e1z);
    const double b = (hx * e2x + hy * e2y + hz * e2z) / (e2x * e2x + e2y * e2y + e2z * e2z);
    const bool blocked = fabs(a) <= 1.0 && fabs(b) <= 1.0;
    // the corners c -+ e1 -+ e2: mm, pm, mp, pp (the sign of e1, then of e2)
    const double mmx = (cx - e1x) - e2x, mmy = (cy - e1y) - e2y, mmz = (cz - e1z) - e2z;
    const double pmx = (cx + e1x) - e2x, pmy = (cy + e1y) - e2y, pmz = (cz + e1z) - e2z;
    const double mpx = (cx - e1x) + e2x, mpy = (cy - e1y) + e2y, mpz = (cz - e1z) + e2z;
    const double ppx = (cx + e1x) + e2x, ppy = (cy + e1y) + e2y, ppz = (cz + e1z) + e2z;
    // the edges mm-pm, mp-pp (along e1), mm-mp, pm-pp (along e2), one after the other through one copy of the code: the
    // ends are picked by compares, so nothing is indexed at run time
    double best = HUGE_VAL;
#pragma unroll 1
    for (int e = 0; e < 4; ++e) {
        const bool a_mm = e == 0 || e == 2, b_pp = e == 1 || e == 3;
        const double ax = a_mm ? mmx : e == 1 ? mpx : pmx, ay = a_mm ? mmy : e == 1 ? mpy : pmy, az = a_mm ? mmz : e == 1 ? mpz : pmz;
        const double bx = b_pp ? ppx : e == 0 ? pmx : mpx, by = b_pp ? ppy : e == 0 ? pmy : mpy, bz = b_pp ? ppz : e == 0 ? pmz : mpz;
        best = fmin(best, bas_occlude_edge(qx, qy, qz, lx, ly, lz, ax, ay, az, bx, by, bz));
    }
    const double delta = fmax(best - sqrt(vx * vx + vy * vy + vz * vz), 0.0);
    *sd = blocked ? delta : -delta;
    return true;
}

// One band of one crossed copy: N = fresnel sd (fresnel = 2 f / c: the Fresnel number, signed as sd is), x = sqrt(2 pi |N|),
//   N >= 0:         A = min(5 + 20 log10(x / tanh x), 24)   (ratio 1 at x == 0)
//   -0.2 < N < 0:   A = max(5 + 20 log10(x / tan x), 0)
//   N <= -0.2:      A = 0
// D = 10^(-A / 20) = exp(-A ln 10 / 20), M = T + (1 - T) D for the screen's transmission T in [0, 1]; returns ln M (exactly 0 for T == 1).
__host__ __device__ inline double bas_occlude_logmag(double sd, double fresnel, double T) {
#pragma clang fp contract(off)
    const double N = fresnel * sd;
    double A = 0.0;
    if (N >= 0.0) {
        const double x = sqrt(BAS_OCCLUDE_TWO_PI * N);
        const double ratio = x == 0.0 ? 1.0 : x / tanh(x);
        A = fmin(5.0 + 20.0 * log10(ratio), 24.0);
    } else if (N > -0.2) {
        const double x = sqrt(BAS_OCCLUDE_TWO_PI * -N);
        A = fmax(5.0 + 20.0 * log10(x / tan(x)), 0.0);
    }
    const double D = exp(-A * BAS_OCCLUDE_NEPERS_PER_DB);
    return log(T + (1.0 - T) * D);
}

// The screens' term of one path's log-magnitudes: the sum over screens (ascending) and, in a room, over the copies of each in
// the cells between the listener's (0) and the image's (m) - x outermost, every index from 0 towards m_a - of ln M[b], added
// to acc[b] in that order.  W: screens [n_screens][9]: c, e1, e2; transmission at [k t_s + b] (NULL: opaque, T = 0);
// fresnel [n_bands].  The geometry of a copy is done once, the bands follow only where the path's ends lie on opposite sides of it.
// On the device acc stays in registers: the band loop is a run-time one (one copy of the transcendentals in the code, not
// sixteen) and the accumulator it adds to is picked by an unrolled compare, so every index into acc is static.  The table,
// the transmissions and the Fresnel factors are read at addresses that do not depend on the path (wave-uniform).
struct BasOccludeScreens {
    const double *screens, *transmission, *fresnel;
    long t_s;
    int n_screens, n_bands;
};

__host__ __device__ __forceinline__ void bas_occlude_sum(const BasOccludeScreens &W, double qx, double qy, double qz,
                                                         double lx, double ly, double lz, bool room, double Lx, double Ly,
                                                         double Lz, int mx, int my, int mz,
                                                         double (&acc)[BAS_OCCLUDE_MAX_BANDS]) {
#pragma clang fp contract(off)
    const int nx = mx < 0 ? -mx : mx, ny = my < 0 ? -my : my, nz = mz < 0 ? -mz : mz;
#pragma unroll 1
    for (int sn = 0; sn < W.n_screens; ++sn) {
        const double *S = W.screens + 9 * sn;
        const double *T = W.transmission ? W.transmission + sn * W.t_s : nullptr;
#pragma unroll 1
        for (int ia = 0; ia <= nx; ++ia)
#pragma unroll 1
            for (int ja = 0; ja <= ny; ++ja)
#pragma unroll 1
                for (int ka = 0; ka <= nz; ++ka) {
                    double cx = S[0], cy = S[1], cz = S[2], e1x = S[3], e1y = S[4], e1z = S[5], e2x = S[6], e2y = S[7],
                           e2z = S[8];
                    if (room) {
                        bas_occlude_mirror(Lx, mx < 0 ? -ia : ia, &cx, &e1x, &e2x);
                        bas_occlude_mirror(Ly, my < 0 ? -ja : ja, &cy, &e1y, &e2y);
                        bas_occlude_mirror(Lz, mz < 0 ? -ka : ka, &cz, &e1z, &e2z);
                    }
                    double sd;
                    if (!bas_occlude_detour(qx, qy, qz, lx, ly, lz, cx, cy, cz, e1x, e1y, e1z, e2x, e2y, e2z, &sd)) continue;
#pragma unroll 1
                    for (int bd = 0; bd < W.n_bands; ++bd) {
                        const double t = bas_occlude_logmag(sd, W.fresnel[bd], T ? T[bd] : 0.0);
#pragma unroll
                        for (int k = 0; k < BAS_OCCLUDE_MAX_BANDS; ++k) acc[k] = k == bd ? acc[k] + t : acc[k];
                    }
                }
    }
}
