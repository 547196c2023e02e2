// Sections b and c of the host-sanitizer harness (hostsan_main.cpp): every compute entry point of include/bas.h, driven
// from one table - a valid argument list and its violations (null, negative, zero, over the limit, misaligned, stride too
// small, overlapping outputs), each with the BAS_E_* code bas.h documents for it.
//   b: every violation returns its code and leaves a text in bas_last_error;
//   c: the valid list itself, with no device to run on, returns a positive hipError_t and a text - no crash, no report.
// Pointers are host buffers standing in for device memory: the library hands them on without reading them.  The ring
// tables of the angle entry points are host arrays by contract and are real.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../include/bas.h"

void hostsan_fail(int line, const char *text);
int hostsan_failures();

namespace {

struct Arg {
    long i = 0;
    double f = 0.0;
    void *p = nullptr;
    Arg(int v) : i(v) {}
    Arg(long v) : i(v) {}
    Arg(unsigned long v) : i((long)v) {}
    Arg(double v) : f(v) {}
    Arg(void *v) : p(v) {}
    Arg(std::nullptr_t) {}
};
typedef std::vector<Arg> Args;

const int ANY = 1000;        // "no documented limit": any answer but success (without a device) - and no sanitizer report
struct Viol {
    int at;                  // argument index
    Arg value;
    int want;                // BAS_E_* or ANY
    int at2 = -1;            // a second argument changed with it (-1: none)
    Arg value2 = 0;
    Viol(int a, Arg v, int w) : at(a), value(v), want(w) {}
    Viol(int a, Arg v, int a2, Arg v2, int w) : at(a), value(v), want(w), at2(a2), value2(v2) {}
};
struct Entry {
    const char *name;
    Args valid;
    std::function<int(const Args &)> call;
    std::vector<Viol> viol;
};

alignas(64) unsigned char g_mem[12][4096];
void *B(int k, int offset = 0) { return g_mem[k] + offset; }
void *const NUL = nullptr;

// the ring tables of the angle entry points (host arrays): ten rings of 18 directions, and broken ones
double RE[10] = {-0.785, -0.524, -0.262, 0.0, 0.262, 0.524, 0.785, 1.047, 1.309, 1.571};
int32_t RS[10] = {0, 18, 36, 54, 72, 90, 108, 126, 144, 162}, RC[10] = {18, 18, 18, 18, 18, 18, 18, 18, 18, 18};
int32_t RC_ZERO[10] = {18, 18, 18, 0, 18, 18, 18, 18, 18, 18}, RS_PAST[10] = {0, 18, 36, 54, 72, 90, 108, 126, 144, 170};
int32_t RS_MAX[10] = {0, 18, 36, 54, 72, 90, 108, 126, 144, INT_MAX}, RC_MAX[10] = {18, 18, 18, 18, 18, 18, 18, 18, 18, INT_MAX};
int32_t RS_NEG[10] = {-1, 18, 36, 54, 72, 90, 108, 126, 144, 162};

#define I(k) ((int)a[k].i)
#define L(k) (a[k].i)
#define Z(k) ((size_t)a[k].i)
#define D(k) (a[k].f)
#define P(T, k) ((T *)a[k].p)

const long BIG_WS = 1L << 30;                               // (a size only: nothing is read or written behind the pointers)
const long T_LIMIT = BAS_MAX_T_IN + 512;                     // a multiple of 512 beyond the ceiling
const int K_LIMIT = BAS_MAX_K + 32;

std::vector<Entry> build_table() {
    std::vector<Entry> t;
    const long plans10 = (long)bas_interp2d_workspace_bytes(10);

    t.push_back({"bas_table_pack_f32", {B(0), 187, 1024, 8, B(1), NUL},
                 [](const Args &a) { return bas_table_pack_f32(P(float, 0), I(1), I(2), I(3), P(float, 4), a[5].p); },
                 {{0, NUL, BAS_E_NULL}, {4, NUL, BAS_E_NULL}, {1, 0, BAS_E_SHAPE}, {1, -1, BAS_E_SHAPE}, {2, 0, BAS_E_SHAPE}, {2, 1001, BAS_E_SHAPE},
                  {3, 0, BAS_E_SHAPE}, {3, -8, BAS_E_SHAPE}, {1, INT_MAX, 2, INT_MAX - 7, BAS_E_SHAPE}, {2, INT_MIN, BAS_E_SHAPE}}});
    t.push_back({"bas_delay_signal_f32", {B(0), B(1), 4, 1024, 8, B(2), NUL},
                 [](const Args &a) { return bas_delay_signal_f32(P(float, 0), P(double, 1), I(2), I(3), I(4), P(float, 5), a[6].p); },
                 {{0, NUL, BAS_E_NULL}, {1, NUL, BAS_E_NULL}, {5, NUL, BAS_E_NULL}, {2, -1, BAS_E_SHAPE}, {3, 0, BAS_E_SHAPE}, {4, 0, BAS_E_SHAPE},
                  {4, -1, BAS_E_SHAPE}, {3, INT_MAX, 4, INT_MAX, ANY}, {2, INT_MAX, 3, INT_MAX, ANY}}});
    t.push_back({"bas_ring_interp_f32", {B(0), B(1), B(2), B(3), 4, 187, 128, 8, 0, B(4), B(5), NUL},
                 [](const Args &a) {
                     return bas_ring_interp_f32(P(float, 0), P(double, 1), P(int32_t, 2), P(double, 3), I(4), I(5), I(6), I(7), I(8), P(float, 9),
                                                P(double, 10), a[11].p);
                 },
                 {{0, NUL, BAS_E_NULL}, {1, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL}, {3, NUL, BAS_E_NULL}, {9, NUL, BAS_E_NULL}, {10, NUL, ANY},
                  {4, -1, BAS_E_SHAPE}, {5, 0, BAS_E_SHAPE}, {6, 0, BAS_E_SHAPE}, {7, 0, BAS_E_SHAPE}, {6, INT_MAX, BAS_E_SHAPE},
                  {5, INT_MAX, 7, INT_MAX, BAS_E_SHAPE}, {8, 1, ANY}}});
    for (int branch = 0; branch < 2; ++branch) {
        Entry e;
        e.name = branch ? "bas_traj_params_branch_f64" : "bas_traj_params_f64";
        e.valid = {B(0), B(1), 100L, (void *)RE, (void *)RS, (void *)RC, B(2), B(3), B(4), 1, NUL};
        if (branch)
            e.call = [](const Args &a) {
                return bas_traj_params_branch_f64(P(double, 0), P(double, 1), L(2), P(double, 3), P(int32_t, 4), P(int32_t, 5), P(float, 6),
                                                  P(int32_t, 7), P(double, 8), I(9), a[10].p);
            };
        else
            e.call = [](const Args &a) {
                return bas_traj_params_f64(P(double, 0), P(double, 1), L(2), P(double, 3), P(int32_t, 4), P(int32_t, 5), P(float, 6), P(int32_t, 7),
                                           P(double, 8), a[10].p);
            };
        e.viol = {{0, NUL, BAS_E_NULL}, {1, NUL, BAS_E_NULL}, {3, NUL, BAS_E_NULL}, {4, NUL, BAS_E_NULL}, {5, NUL, BAS_E_NULL}, {6, NUL, BAS_E_NULL},
                  {7, NUL, BAS_E_NULL}, {8, NUL, BAS_E_NULL}, {2, -1L, BAS_E_SHAPE}, {2, LONG_MIN, BAS_E_SHAPE}, {2, LONG_MAX, ANY},
                  {5, (void *)RC_ZERO, BAS_E_SHAPE}, {4, (void *)RS_PAST, BAS_E_SHAPE}, {4, (void *)RS_NEG, BAS_E_SHAPE},
                  {4, (void *)RS_MAX, 5, (void *)RC_MAX, BAS_E_SHAPE}};
        if (branch) {
            e.viol.push_back({9, 2, BAS_E_SHAPE});
            e.viol.push_back({9, -1, BAS_E_SHAPE});
        }
        t.push_back(e);
    }
    for (int gain = 0; gain < 2; ++gain) {
        Entry e;
        e.name = gain ? "bas_interp2d_gain_f32" : "bas_interp2d_f32";
        e.valid = {B(0), B(1), B(2), B(3), B(6), 10, 187, 128, 8, B(4), B(5), plans10, NUL};
        if (gain)
            e.call = [](const Args &a) {
                return bas_interp2d_gain_f32(P(float, 0), P(double, 1), P(int32_t, 2), P(double, 3), P(double, 4), I(5), I(6), I(7), I(8), P(float, 9),
                                             a[10].p, Z(11), a[12].p);
            };
        else
            e.call = [](const Args &a) {
                return bas_interp2d_f32(P(float, 0), P(double, 1), P(int32_t, 2), P(double, 3), I(5), I(6), I(7), I(8), P(float, 9), a[10].p, Z(11),
                                        a[12].p);
            };
        e.viol = {{0, NUL, BAS_E_NULL}, {1, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL}, {3, NUL, BAS_E_NULL}, {9, NUL, BAS_E_NULL}, {5, -1, BAS_E_SHAPE},
                  {6, 0, BAS_E_SHAPE}, {7, 0, BAS_E_SHAPE}, {8, 0, BAS_E_SHAPE}, {7, INT_MAX, BAS_E_SHAPE}, {6, INT_MAX, 8, INT_MAX, BAS_E_SHAPE},
                  {10, NUL, BAS_E_WORKSPACE}, {11, plans10 - 1, BAS_E_WORKSPACE}, {11, 0L, BAS_E_WORKSPACE}, {10, B(5, 8), BAS_E_WORKSPACE}, {8, 2, ANY},
                  {5, INT_MAX, 11, LONG_MAX, ANY}};
        if (gain) e.viol.push_back({4, NUL, BAS_E_NULL});
        t.push_back(e);
    }
    for (int gain = 0; gain < 2; ++gain) {
        Entry e;
        e.name = gain ? "bas_interp2d_plan_gain_f32" : "bas_interp2d_plan_f32";
        e.valid = {B(0), B(1), B(2), B(6), 10, 187, 128, 8, B(3), plans10, NUL};
        if (gain)
            e.call = [](const Args &a) {
                return bas_interp2d_plan_gain_f32(P(double, 0), P(int32_t, 1), P(double, 2), P(double, 3), I(4), I(5), I(6), I(7), a[8].p, Z(9), a[10].p);
            };
        else
            e.call = [](const Args &a) {
                return bas_interp2d_plan_f32(P(double, 0), P(int32_t, 1), P(double, 2), I(4), I(5), I(6), I(7), a[8].p, Z(9), a[10].p);
            };
        e.viol = {{0, NUL, BAS_E_NULL}, {1, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL}, {4, -1, BAS_E_SHAPE}, {5, 0, BAS_E_SHAPE}, {6, 0, BAS_E_SHAPE},
                  {7, 0, BAS_E_SHAPE}, {7, 3, BAS_E_SHAPE}, {6, INT_MAX, BAS_E_SHAPE}, {5, INT_MAX, 7, INT_MAX, BAS_E_SHAPE}, {8, NUL, BAS_E_WORKSPACE},
                  {9, plans10 - 1, BAS_E_WORKSPACE}, {8, B(3, 8), BAS_E_WORKSPACE}, {4, INT_MAX, 9, LONG_MAX, ANY}};
        if (gain) e.viol.push_back({3, NUL, BAS_E_NULL});
        t.push_back(e);
    }
    for (int gain = 0; gain < 2; ++gain) {
        Entry e;
        e.name = gain ? "bas_interp2d_plan_angles_gain_f32" : "bas_interp2d_plan_angles_f32";
        e.valid = {B(0), B(1), B(2), B(6), 10, (void *)RE, (void *)RS, (void *)RC, B(3), 1, 187, 128, 8, B(4), plans10, NUL};
        if (gain)
            e.call = [](const Args &a) {
                return bas_interp2d_plan_angles_gain_f32(P(double, 0), P(double, 1), P(double, 2), P(double, 3), I(4), P(double, 5), P(int32_t, 6),
                                                         P(int32_t, 7), P(float, 8), I(9), I(10), I(11), I(12), a[13].p, Z(14), a[15].p);
            };
        else
            e.call = [](const Args &a) {
                return bas_interp2d_plan_angles_f32(P(double, 0), P(double, 1), P(double, 2), I(4), P(double, 5), P(int32_t, 6), P(int32_t, 7),
                                                    P(float, 8), I(9), I(10), I(11), I(12), a[13].p, Z(14), a[15].p);
            };
        e.viol = {{0, NUL, BAS_E_NULL}, {1, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL}, {5, NUL, BAS_E_NULL}, {6, NUL, BAS_E_NULL}, {7, NUL, BAS_E_NULL},
                  {8, NUL, BAS_E_NULL}, {4, -1, BAS_E_SHAPE}, {10, 0, BAS_E_SHAPE}, {11, 0, BAS_E_SHAPE}, {12, 3, BAS_E_SHAPE}, {12, 0, BAS_E_SHAPE},
                  {9, 2, BAS_E_SHAPE}, {9, -1, BAS_E_SHAPE}, {11, INT_MAX, BAS_E_SHAPE}, {10, INT_MAX, 12, INT_MAX, BAS_E_SHAPE},
                  {13, NUL, BAS_E_WORKSPACE}, {14, plans10 - 1, BAS_E_WORKSPACE}, {13, B(4, 8), BAS_E_WORKSPACE}, {10, 100, BAS_E_SHAPE},
                  {7, (void *)RC_ZERO, BAS_E_SHAPE}, {6, (void *)RS_NEG, BAS_E_SHAPE}, {6, (void *)RS_MAX, 7, (void *)RC_MAX, BAS_E_SHAPE}};
        if (gain) e.viol.push_back({3, NUL, BAS_E_NULL});
        t.push_back(e);
    }
    for (int prof = 0; prof < 2; ++prof) {
        Entry e;
        e.name = prof ? "bas_render_mix_profiled_f32" : "bas_render_mix_f32";
        e.valid = {B(0), 1024L, B(1), 2, 1024L, 512, 32, 128, B(2), 0, B(3), B(4), BIG_WS, NUL, NUL, NUL};
        if (prof)
            e.call = [](const Args &a) {
                return bas_render_mix_profiled_f32(P(float, 0), L(1), P(float, 2), I(3), L(4), I(5), I(6), I(7), P(float, 8), I(9), P(float, 10), a[11].p,
                                                   Z(12), a[13].p, a[14].p, a[15].p);
            };
        else
            e.call = [](const Args &a) {
                return bas_render_mix_f32(P(float, 0), L(1), P(float, 2), I(3), L(4), I(5), I(6), I(7), P(float, 8), I(9), P(float, 10), a[11].p, Z(12),
                                          a[13].p);
            };
        e.viol = {{8, NUL, BAS_E_NULL}, {0, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL}, {3, -1, BAS_E_SHAPE}, {4, -512L, BAS_E_SHAPE}, {5, 0, BAS_E_SHAPE},
                  {5, -512, BAS_E_SHAPE}, {6, 0, BAS_E_SHAPE}, {6, -32, BAS_E_SHAPE}, {7, 0, BAS_E_SHAPE}, {7, INT_MIN, BAS_E_SHAPE}, {6, 48, BAS_E_SHAPE},
                  {4, 1000L, BAS_E_SHAPE}, {1, 512L, BAS_E_SHAPE}, {1, -1L, BAS_E_SHAPE}, {5, K_LIMIT, 4, (long)K_LIMIT, BAS_E_SHAPE},
                  {7, BAS_MAX_L + 1, BAS_E_SHAPE}, {7, INT_MAX, BAS_E_SHAPE}, {3, BAS_MAX_N_SRC + 1, BAS_E_SHAPE}, {3, INT_MAX, BAS_E_SHAPE},
                  {4, T_LIMIT, 1, T_LIMIT, BAS_E_SHAPE}, {4, LONG_MAX / 512 * 512, 1, LONG_MAX, BAS_E_SHAPE}, {4, 1L << 35, 5, 32, BAS_E_SHAPE},
                  {10, NUL, 12, 64L, BAS_E_WORKSPACE}, {10, NUL, 11, NUL, BAS_E_WORKSPACE}};
        t.push_back(e);
    }
    for (int which = 0; which < 4; ++which) {
        Entry e;
        static const char *names[4] = {"bas_render_mix_fused_f32", "bas_render_mix_fused_profiled_f32", "bas_render_fused_fir_f32", "bas_render_fused_reduce_f32"};
        e.name = names[which];
        e.valid = {B(0), 1024L, B(1), B(2), 256, 1024L, 512, 32, 128, 8, 187, B(3), 0, B(5), 1, B(4), BIG_WS, NUL, NUL, NUL};
        e.call = [which](const Args &a) {
            typedef int (*fn_t)(const float *, long, const float *, const void *, int, long, int, int, int, int, int, float *, int, float *, int, void *,
                                size_t, bas_stream_t);
            if (which == 1)
                return bas_render_mix_fused_profiled_f32(P(float, 0), L(1), P(float, 2), a[3].p, I(4), L(5), I(6), I(7), I(8), I(9), I(10), P(float, 11),
                                                         I(12), P(float, 13), I(14), a[15].p, Z(16), a[17].p, a[18].p, a[19].p);
            const fn_t fn = which == 0 ? bas_render_mix_fused_f32 : which == 2 ? bas_render_fused_fir_f32 : bas_render_fused_reduce_f32;
            return fn(P(float, 0), L(1), P(float, 2), a[3].p, I(4), L(5), I(6), I(7), I(8), I(9), I(10), P(float, 11), I(12), P(float, 13), I(14), a[15].p,
                      Z(16), a[17].p);
        };
        e.viol = {{11, NUL, BAS_E_NULL}, {0, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL}, {3, NUL, BAS_E_NULL}, {4, -1, BAS_E_SHAPE}, {5, -512L, BAS_E_SHAPE},
                  {6, 0, BAS_E_SHAPE}, {7, 0, BAS_E_SHAPE}, {7, -32, BAS_E_SHAPE}, {8, 0, BAS_E_SHAPE}, {10, 0, BAS_E_SHAPE}, {9, 3, BAS_E_SHAPE},
                  {9, 0, BAS_E_SHAPE}, {7, 48, BAS_E_SHAPE}, {5, 1000L, BAS_E_SHAPE}, {1, 512L, BAS_E_SHAPE}, {0, B(0, 4), BAS_E_ALIGN},
                  {1, 1026L, BAS_E_ALIGN}, {3, B(2, 8), BAS_E_ALIGN}, {15, B(4, 8), BAS_E_ALIGN}, {6, 64, 5, 1024L, BAS_E_SHAPE}, {7, 4, BAS_E_SHAPE},
                  {15, NUL, BAS_E_WORKSPACE}, {16, 16L, BAS_E_WORKSPACE}, {6, K_LIMIT, 5, (long)K_LIMIT, BAS_E_SHAPE}, {8, BAS_MAX_L + 1, BAS_E_SHAPE},
                  {8, BAS_MAX_L, BAS_E_SHAPE}, {4, BAS_MAX_N_SRC + 1, BAS_E_SHAPE}, {5, T_LIMIT, 1, T_LIMIT, BAS_E_SHAPE}, {5, 1L << 35, 6, 32, BAS_E_SHAPE},
                  {10, INT_MAX, 9, INT_MAX, BAS_E_SHAPE}};
        t.push_back(e);
    }
    for (int which = 0; which < 3; ++which) {
        Entry e;
        static const char *names[3] = {"bas_render_stream_block_f32", "bas_render_stream_block_profiled_f32", "bas_render_stream_block_gain_f32"};
        e.name = names[which];
        //          0     1      2     3     4    5      6    7   8    9  10   11    12    13      14   15    16    17    18  19 20 21    22    23    24
        e.valid = {B(0), 1024L, B(1), B(2), 256, 1024L, 512, 32, 128, 8, 187, B(3), B(4), BIG_WS, 512, B(5), B(6), B(7), 3L, 1, 2, B(8), B(9), B(10), NUL};
        e.call = [which](const Args &a) {
            if (which == 0)
                return bas_render_stream_block_f32(P(float, 0), L(1), P(float, 2), a[3].p, I(4), L(5), I(6), I(7), I(8), I(9), I(10), P(float, 11), a[12].p,
                                                   Z(13), I(14), P(double, 15), P(double, 16), L(18), I(19), I(20), P(double, 21), P(float, 23), a[24].p);
            if (which == 1)
                return bas_render_stream_block_profiled_f32(P(float, 0), L(1), P(float, 2), a[3].p, I(4), L(5), I(6), I(7), I(8), I(9), I(10), P(float, 11),
                                                            a[12].p, Z(13), I(14), P(double, 15), P(double, 16), L(18), I(19), I(20), P(double, 21),
                                                            P(float, 23), a[24].p, nullptr, nullptr);
            return bas_render_stream_block_gain_f32(P(float, 0), L(1), P(float, 2), a[3].p, I(4), L(5), I(6), I(7), I(8), I(9), I(10), P(float, 11), a[12].p,
                                                    Z(13), I(14), P(double, 15), P(double, 16), P(double, 17), L(18), I(19), I(20), P(double, 21),
                                                    P(double, 22), P(float, 23), a[24].p);
        };
        e.viol = {{4, 0, BAS_E_SHAPE}, {4, -1, BAS_E_SHAPE}, {14, -512, BAS_E_SHAPE}, {14, 1024, BAS_E_SHAPE}, {14, INT_MIN, 5, LONG_MAX, BAS_E_SHAPE},
                  {5, LONG_MIN, BAS_E_SHAPE}, {20, 1, BAS_E_SHAPE}, {19, -1, BAS_E_SHAPE}, {18, 2L, BAS_E_SHAPE}, {19, INT_MAX, 20, INT_MAX, BAS_E_SHAPE},
                  {0, NUL, BAS_E_NULL}, {15, NUL, BAS_E_NULL}, {16, NUL, BAS_E_NULL}, {21, NUL, BAS_E_NULL}, {11, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL},
                  {3, NUL, BAS_E_NULL}, {9, 3, BAS_E_SHAPE}, {7, 48, BAS_E_SHAPE}, {6, 64, BAS_E_SHAPE}, {12, NUL, BAS_E_WORKSPACE}, {13, 16L, BAS_E_WORKSPACE},
                  {0, B(0, 4), BAS_E_ALIGN}, {1, 1026L, BAS_E_ALIGN}, {8, BAS_MAX_L + 1, BAS_E_SHAPE}, {23, NUL, ANY}};
        if (which == 2) {
            e.viol.push_back({17, NUL, BAS_E_NULL});
            e.viol.push_back({22, NUL, BAS_E_NULL});
        }
        t.push_back(e);
    }
    t.push_back({"bas_render_status", {B(0), 1L << 20, NUL},
                 [](const Args &a) { return bas_render_status(a[0].p, Z(1), a[2].p); },
                 {{0, NUL, BAS_E_WORKSPACE}, {1, 16L, BAS_E_WORKSPACE}, {1, 0L, BAS_E_WORKSPACE}}});
    t.push_back({"bas_peak_normalize_f32", {B(0), 1000L, B(1), 1, NUL},
                 [](const Args &a) { return bas_peak_normalize_f32(P(float, 0), L(1), P(float, 2), I(3), a[4].p); },
                 {{0, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL}, {1, -1L, BAS_E_SHAPE}, {1, LONG_MIN, BAS_E_SHAPE}, {1, LONG_MAX, ANY}}});
    t.push_back({"bas_scale_by_peak_f32", {B(0), 1000L, B(1), NUL},
                 [](const Args &a) { return bas_scale_by_peak_f32(P(float, 0), L(1), P(float, 2), a[3].p); },
                 {{0, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL}, {1, -1L, BAS_E_SHAPE}, {1, LONG_MAX, ANY}}});
    t.push_back({"bas_mix_partials_f32", {B(0), 4, 1024L, 1000L, B(1), B(2), NUL},
                 [](const Args &a) { return bas_mix_partials_f32(P(float, 0), I(1), L(2), L(3), P(float, 4), P(float, 5), a[6].p); },
                 {{0, NUL, BAS_E_NULL}, {4, NUL, BAS_E_NULL}, {3, -1L, BAS_E_SHAPE}, {1, -1, BAS_E_SHAPE}, {2, 999L, BAS_E_SHAPE}, {2, -1L, BAS_E_SHAPE},
                  {5, NUL, ANY}, {3, LONG_MAX, 2, LONG_MAX, ANY}}});
    t.push_back({"bas_mix_finish_f32", {B(0), 4, 1024L, 1000L, B(1), B(2), 1, B(3), 1L << 20, NUL},
                 [](const Args &a) { return bas_mix_finish_f32(P(float, 0), I(1), L(2), L(3), P(float, 4), P(float, 5), I(6), a[7].p, Z(8), a[9].p); },
                 {{0, NUL, BAS_E_NULL}, {4, NUL, BAS_E_NULL}, {3, -1L, BAS_E_SHAPE}, {1, -1, BAS_E_SHAPE}, {2, 999L, BAS_E_SHAPE}, {7, NUL, BAS_E_WORKSPACE},
                  {8, 2048L, BAS_E_WORKSPACE}, {7, B(3, 8), BAS_E_ALIGN}, {4, B(1, 4), BAS_E_ALIGN}, {5, NUL, ANY}, {3, LONG_MAX, 2, LONG_MAX, ANY}}});
    for (int gain = 0; gain < 2; ++gain) {
        Entry e;
        e.name = gain ? "bas_stream_epilogue_gain_f32" : "bas_stream_epilogue_f32";
        //          0     1      2  3    4     5     6     7     8   9  10 11    12    13    14     15    16
        e.valid = {B(0), 1024L, 4, 512, 512L, B(1), B(2), B(6), 3L, 1, 2, B(3), B(7), B(4), 1200L, B(5), NUL};
        if (gain)
            e.call = [](const Args &a) {
                return bas_stream_epilogue_gain_f32(P(float, 0), L(1), I(2), I(3), L(4), P(double, 5), P(double, 6), P(double, 7), L(8), I(9), I(10),
                                                    P(double, 11), P(double, 12), P(float, 13), L(14), P(float, 15), a[16].p);
            };
        else
            e.call = [](const Args &a) {
                return bas_stream_epilogue_f32(P(float, 0), L(1), I(2), I(3), L(4), P(double, 5), P(double, 6), L(8), I(9), I(10), P(double, 11),
                                               P(float, 13), L(14), P(float, 15), a[16].p);
            };
        e.viol = {{2, -1, BAS_E_SHAPE}, {3, -1, BAS_E_SHAPE}, {4, 0L, BAS_E_SHAPE}, {4, -512L, BAS_E_SHAPE}, {9, -1, BAS_E_SHAPE}, {10, 1, BAS_E_SHAPE},
                  {1, 1023L, BAS_E_SHAPE}, {8, 2L, BAS_E_SHAPE}, {14, 1023L, BAS_E_SHAPE}, {13, NUL, BAS_E_NULL}, {0, NUL, BAS_E_NULL}, {5, NUL, BAS_E_NULL},
                  {6, NUL, BAS_E_NULL}, {11, NUL, BAS_E_NULL}, {4, LONG_MAX, 1, LONG_MAX, BAS_E_SHAPE}, {9, INT_MAX, 10, INT_MAX, BAS_E_SHAPE},
                  {3, INT_MAX, 4, LONG_MAX - 7, BAS_E_SHAPE}, {15, NUL, ANY}};
        if (gain) {
            e.viol.push_back({7, NUL, BAS_E_NULL});
            e.viol.push_back({12, NUL, BAS_E_NULL});
        }
        t.push_back(e);
    }
    for (int which = 0; which < 3; ++which) {
        Entry e;
        static const char *names[3] = {"bas_batch_pack_f32", "bas_batch_pack_gain_f32", "bas_batch_pack_delay_f32"};
        e.name = names[which];
        //          0     1  2  3      4     5     6     7     8     9     10 11  12   13     14    15     16    17    18     19
        e.valid = {B(0), 3, 2, 1000L, B(1), B(2), B(3), B(4), B(8), B(9), 1, 3L, 512, 4096L, B(5), 4096L, B(6), B(7), B(10), NUL};
        e.call = [which](const Args &a) {
            if (which == 0)
                return bas_batch_pack_f32(P(float, 0), I(1), I(2), L(3), P(long, 4), P(long, 5), P(double, 6), P(double, 7), L(11), I(12), L(13),
                                          P(float, 14), L(15), P(double, 16), P(double, 17), a[19].p);
            if (which == 1)
                return bas_batch_pack_gain_f32(P(float, 0), I(1), I(2), L(3), P(long, 4), P(long, 5), P(double, 6), P(double, 7), P(double, 8), L(11), I(12),
                                               L(13), P(float, 14), L(15), P(double, 16), P(double, 17), P(double, 18), a[19].p);
            return bas_batch_pack_delay_f32(P(float, 0), I(1), I(2), L(3), P(long, 4), P(long, 5), P(double, 6), P(double, 7), P(double, 8), P(double, 9),
                                            I(10), L(11), I(12), L(13), P(float, 14), L(15), P(double, 16), P(double, 17), P(double, 18), a[19].p);
        };
        e.viol = {{1, 0, BAS_E_SHAPE}, {1, -1, BAS_E_SHAPE}, {2, 0, BAS_E_SHAPE}, {3, -1L, BAS_E_SHAPE}, {12, 0, BAS_E_SHAPE}, {13, 0L, BAS_E_SHAPE},
                  {11, 0L, BAS_E_SHAPE}, {13, 4000L, BAS_E_SHAPE}, {15, 4000L, BAS_E_SHAPE}, {15, 4098L, BAS_E_SHAPE}, {0, NUL, BAS_E_NULL},
                  {4, NUL, BAS_E_NULL}, {5, NUL, BAS_E_NULL}, {6, NUL, BAS_E_NULL}, {7, NUL, BAS_E_NULL}, {14, NUL, BAS_E_NULL}, {16, NUL, BAS_E_NULL},
                  {17, NUL, BAS_E_NULL}, {14, B(5, 4), BAS_E_ALIGN}, {1, 65536, BAS_E_SHAPE}, {1, INT_MAX, BAS_E_SHAPE},
                  {15, LONG_MAX - 3, 2, INT_MAX, ANY}, {13, LONG_MAX / 512 * 512, 15, LONG_MAX - 3, ANY}, {0, NUL, 3, 0L, ANY}};
        if (which == 1) {
            e.viol.push_back({8, NUL, BAS_E_NULL});
            e.viol.push_back({18, NUL, BAS_E_NULL});
        }
        if (which == 2) {
            e.viol.push_back({9, NUL, BAS_E_NULL});
            e.viol.push_back({18, NUL, BAS_E_NULL});
            e.viol.push_back({8, NUL, 18, NUL, ANY});        // no gain: gain_out is not looked at
            e.viol.push_back({10, 2, BAS_E_SHAPE});
            e.viol.push_back({10, -1, BAS_E_SHAPE});
        }
        t.push_back(e);
    }
    t.push_back({"bas_batch_finish_f32", {B(0), 5000L, 3, B(1), B(2), 1200L, 1, B(3), B(4), NUL},
                 [](const Args &a) {
                     return bas_batch_finish_f32(P(float, 0), L(1), I(2), P(long, 3), P(long, 4), L(5), I(6), P(float, 7), P(float, 8), a[9].p);
                 },
                 {{2, 0, BAS_E_SHAPE}, {2, -1, BAS_E_SHAPE}, {2, 65536, BAS_E_SHAPE}, {5, -1L, BAS_E_SHAPE}, {1, -1L, BAS_E_SHAPE}, {0, NUL, BAS_E_NULL},
                  {3, NUL, BAS_E_NULL}, {4, NUL, BAS_E_NULL}, {8, NUL, BAS_E_NULL}, {7, NUL, ANY}, {5, LONG_MAX, 1, LONG_MAX, ANY}}});
    for (int which = 0; which < 4; ++which) {
        Entry e;
        static const char *names[4] = {"bas_stream_batch_pack_f32", "bas_stream_batch_pack_head_f32", "bas_stream_batch_pack_gain_f32",
                                       "bas_stream_batch_pack_delay_f32"};
        e.name = names[which];
        //          0     1     2     3     4     5     6  7     8     9      10     11  12 13 14    15   16   17    18     19    20    21     22   23
        e.valid = {B(0), B(1), B(2), B(6), B(7), B(8), 1, 30.0, B(9), 3072L, 1024L, 64, 4, 3, 512L, 512, 512, B(3), 8192L, B(4), B(5), B(10), 16L, NUL};
        e.call = [which](const Args &a) {
            if (which == 0)
                return bas_stream_batch_pack_f32(P(float, 0), P(double, 1), P(double, 2), I(12), I(13), L(14), I(15), I(16), P(float, 17), L(18),
                                                 P(double, 19), P(double, 20), L(22), a[23].p);
            if (which == 1)
                return bas_stream_batch_pack_head_f32(P(float, 0), P(double, 1), P(double, 2), P(double, 3), I(12), I(13), L(14), I(15), I(16), P(float, 17),
                                                      L(18), P(double, 19), P(double, 20), L(22), a[23].p);
            if (which == 2)
                return bas_stream_batch_pack_gain_f32(P(float, 0), P(double, 1), P(double, 2), P(double, 3), P(double, 4), I(12), I(13), L(14), I(15), I(16),
                                                      P(float, 17), L(18), P(double, 19), P(double, 20), P(double, 21), L(22), a[23].p);
            return bas_stream_batch_pack_delay_f32(P(float, 0), P(double, 1), P(double, 2), P(double, 3), P(double, 4), P(double, 5), I(6), D(7), P(float, 8),
                                                   L(9), L(10), I(11), I(12), I(13), L(14), I(15), I(16), P(float, 17), L(18), P(double, 19), P(double, 20),
                                                   P(double, 21), L(22), a[23].p);
        };
        e.viol = {{12, 0, BAS_E_SHAPE}, {12, 65536, BAS_E_SHAPE}, {12, -1, BAS_E_SHAPE}, {13, 0, BAS_E_SHAPE}, {15, 0, BAS_E_SHAPE}, {14, 0L, BAS_E_SHAPE},
                  {16, -512, BAS_E_SHAPE}, {14, 500L, BAS_E_SHAPE}, {16, 100, BAS_E_SHAPE}, {18, 5631L, BAS_E_SHAPE}, {22, 11L, BAS_E_SHAPE},
                  {0, NUL, BAS_E_NULL}, {1, NUL, BAS_E_NULL}, {2, NUL, BAS_E_NULL}, {17, NUL, BAS_E_NULL}, {19, NUL, BAS_E_NULL}, {20, NUL, BAS_E_NULL},
                  {14, LONG_MAX / 512 * 512, 18, LONG_MAX, BAS_E_SHAPE}, {14, LONG_MAX / 512 * 512, 22, LONG_MAX, BAS_E_SHAPE},
                  {16, INT_MAX / 512 * 512, 18, LONG_MAX, ANY}};
        if (which == 1) e.viol.push_back({3, NUL, BAS_E_NULL});
        if (which == 2) {
            e.viol.push_back({4, NUL, BAS_E_NULL});
            e.viol.push_back({21, NUL, BAS_E_NULL});
            e.viol.push_back({3, NUL, ANY});
        }
        if (which == 3) {
            const std::vector<Viol> more = {{5, NUL, BAS_E_NULL}, {8, NUL, BAS_E_NULL}, {6, 2, BAS_E_SHAPE}, {7, 1.0, BAS_E_SHAPE}, {7, 63.0, BAS_E_SHAPE},
                                            {7, 0.0, BAS_E_SHAPE}, {7, (double)NAN, BAS_E_SHAPE}, {10, 500L, BAS_E_SHAPE}, {9, 1024L, BAS_E_SHAPE},
                                            {11, 3, BAS_E_SHAPE}, {3, NUL, 4, NUL, ANY}, {11, INT_MAX, 10, LONG_MAX, ANY}};
            e.viol.insert(e.viol.end(), more.begin(), more.end());
        }
        t.push_back(e);
    }
    for (int gain = 0; gain < 2; ++gain) {
        Entry e;
        e.name = gain ? "bas_stream_batch_epilogue_gain_f32" : "bas_stream_batch_epilogue_f32";
        //          0     1      2  3  4    5     6    7     8     9     10   11    12    13    14     15    16
        e.valid = {B(0), 8192L, 4, 3, 512, 512L, 512, B(1), B(2), B(6), 16L, B(3), B(7), B(4), 8192L, B(5), NUL};
        if (gain)
            e.call = [](const Args &a) {
                return bas_stream_batch_epilogue_gain_f32(P(float, 0), L(1), I(2), I(3), I(4), L(5), I(6), P(double, 7), P(double, 8), P(double, 9), L(10),
                                                          P(double, 11), P(double, 12), P(float, 13), L(14), P(float, 15), a[16].p);
            };
        else
            e.call = [](const Args &a) {
                return bas_stream_batch_epilogue_f32(P(float, 0), L(1), I(2), I(3), I(4), L(5), I(6), P(double, 7), P(double, 8), L(10), P(double, 11),
                                                     P(float, 13), L(14), P(float, 15), a[16].p);
            };
        e.viol = {{2, 0, BAS_E_SHAPE}, {2, 65536, BAS_E_SHAPE}, {3, 0, BAS_E_SHAPE}, {6, 0, BAS_E_SHAPE}, {5, 0L, BAS_E_SHAPE}, {4, -512, BAS_E_SHAPE},
                  {5, 500L, BAS_E_SHAPE}, {4, 100, BAS_E_SHAPE}, {1, 5631L, BAS_E_SHAPE}, {10, 11L, BAS_E_SHAPE}, {14, 5631L, BAS_E_SHAPE},
                  {0, NUL, BAS_E_NULL}, {7, NUL, BAS_E_NULL}, {8, NUL, BAS_E_NULL}, {11, NUL, BAS_E_NULL}, {13, NUL, BAS_E_NULL}, {15, NUL, BAS_E_NULL},
                  {5, LONG_MAX / 512 * 512, 1, LONG_MAX, BAS_E_SHAPE}};
        if (gain) {
            e.viol.push_back({9, NUL, BAS_E_NULL});
            e.viol.push_back({12, NUL, BAS_E_NULL});
        }
        t.push_back(e);
    }
    t.push_back({"bas_head_relative_f64", {B(0), B(1), 64L, 8L, B(2), 64L, 4L, 2, 3, 4, B(3), B(4), 12L, 4L, NUL},
                 [](const Args &a) {
                     return bas_head_relative_f64(P(double, 0), P(double, 1), L(2), L(3), P(double, 4), L(5), L(6), I(7), I(8), I(9), P(double, 10),
                                                  P(double, 11), L(12), L(13), a[14].p);
                 },
                 {{0, NUL, BAS_E_NULL}, {1, NUL, BAS_E_NULL}, {4, NUL, BAS_E_NULL}, {10, NUL, BAS_E_NULL}, {11, NUL, BAS_E_NULL}, {7, 0, BAS_E_SHAPE},
                  {8, 0, BAS_E_SHAPE}, {9, 0, BAS_E_SHAPE}, {9, -1, BAS_E_SHAPE}, {2, -1L, BAS_E_SHAPE}, {3, -1L, BAS_E_SHAPE}, {5, -1L, BAS_E_SHAPE},
                  {6, 3L, BAS_E_SHAPE}, {12, -1L, BAS_E_SHAPE}, {13, -1L, BAS_E_SHAPE}, {13, 3L, BAS_E_SHAPE}, {12, 11L, BAS_E_SHAPE},
                  {11, B(3), BAS_E_SHAPE}, {0, B(0, 4), BAS_E_ALIGN}, {4, B(2, 4), BAS_E_ALIGN}, {10, B(3, 4), BAS_E_ALIGN},
                  {7, INT_MAX, 12, LONG_MAX, ANY}, {7, 65535, 8, 65535, ANY}}});
    t.push_back({"bas_delay_rows_f32", {B(0, 64), 0L, 1024L, 8, B(3), B(1), 0L, 16L, 1, 2, 256L, 64, 1, 0.0, B(2), 0L, 1024L, NUL},
                 [](const Args &a) {
                     return bas_delay_rows_f32(P(float, 0), L(1), L(2), I(3), P(long, 4), P(double, 5), L(6), L(7), I(8), I(9), L(10), I(11), I(12), D(13),
                                               P(float, 14), L(15), L(16), a[17].p);
                 },
                 {{8, -1, BAS_E_SHAPE}, {9, -1, BAS_E_SHAPE}, {10, -1L, BAS_E_SHAPE}, {11, 0, BAS_E_SHAPE}, {3, -1, BAS_E_SHAPE}, {12, 2, BAS_E_SHAPE},
                  {10, 1L << 30, BAS_E_SHAPE}, {10, LONG_MAX, BAS_E_SHAPE}, {8, 65536, BAS_E_SHAPE}, {8, INT_MAX, 9, INT_MAX, BAS_E_SHAPE},
                  {13, 7.0, BAS_E_SHAPE}, {13, 1.5, BAS_E_SHAPE}, {0, NUL, BAS_E_NULL}, {5, NUL, BAS_E_NULL}, {14, NUL, BAS_E_NULL}, {4, NUL, ANY}}});
    t.push_back({"bas_delay_carry_f32", {B(0), 0L, 1024L, 1, 2, 64, 512L, NUL},
                 [](const Args &a) { return bas_delay_carry_f32(P(float, 0), L(1), L(2), I(3), I(4), I(5), L(6), a[7].p); },
                 {{3, -1, BAS_E_SHAPE}, {4, -1, BAS_E_SHAPE}, {5, -1, BAS_E_SHAPE}, {6, 0L, BAS_E_SHAPE}, {6, -1L, BAS_E_SHAPE}, {0, NUL, BAS_E_NULL},
                  {3, 65536, 4, 65536, BAS_E_SHAPE}, {3, INT_MAX, 4, INT_MAX, BAS_E_SHAPE}}});
    t.push_back({"bas_color_rows_f32", {B(0), 0L, 1024L, 0, B(3), B(1), 0L, 0L, 8L, 5, 1, 2, 256L, 64, B(2), 0L, 1024L, NUL},
                 [](const Args &a) {
                     return bas_color_rows_f32(P(float, 0), L(1), L(2), I(3), P(long, 4), P(float, 5), L(6), L(7), L(8), I(9), I(10), I(11), L(12), I(13),
                                               P(float, 14), L(15), L(16), a[17].p);
                 },
                 {{10, -1, BAS_E_SHAPE}, {11, -1, BAS_E_SHAPE}, {12, -1L, BAS_E_SHAPE}, {13, 0, BAS_E_SHAPE}, {3, -1, BAS_E_SHAPE}, {9, 0, BAS_E_SHAPE},
                  {9, 65, BAS_E_SHAPE}, {12, 1L << 30, BAS_E_SHAPE}, {10, 65536, BAS_E_SHAPE}, {10, INT_MAX, 11, INT_MAX, BAS_E_SHAPE}, {1, -1L, BAS_E_SHAPE},
                  {2, -1L, BAS_E_SHAPE}, {6, -1L, BAS_E_SHAPE}, {7, -1L, BAS_E_SHAPE}, {8, -1L, BAS_E_SHAPE}, {15, -1L, BAS_E_SHAPE}, {16, -1L, BAS_E_SHAPE},
                  {8, 4L, BAS_E_SHAPE}, {0, NUL, BAS_E_NULL}, {5, NUL, BAS_E_NULL}, {14, NUL, BAS_E_NULL}, {0, B(0, 2), BAS_E_ALIGN}, {5, B(1, 1), BAS_E_ALIGN},
                  {14, B(2, 2), BAS_E_ALIGN}, {4, B(3, 4), BAS_E_ALIGN}, {4, NUL, ANY}, {13, INT_MAX, ANY}, {13, 1 << 26, ANY}}});
    {
        Entry e;
        e.name = "bas_scene_params_f64";
        //          0     1    2    3   4    5   6   7    8    9   10  11   12  13  14   15  16  17   18   19   20 21     22   23   24     25 26 27 28    29    30    31   32  33    34   35  36
        e.valid = {B(0), 64L, 16L, 3L, NUL, 0L, 0L, 0.0, NUL, 0L, 0L, NUL, 0L, 0L, NUL, 0L, 0L, NUL, NUL, NUL, 1, 128.0, 1.0, 0.0, 100.0, 2, 2, 3, B(3), B(4), B(5), 6L, 3L, B(6), 6L, 3L, NUL};
        e.call = [](const Args &a) {
            return bas_scene_params_f64(P(double, 0), L(1), L(2), L(3), P(double, 4), L(5), L(6), D(7), P(double, 8), L(9), L(10), P(double, 11), L(12), L(13),
                                        P(double, 14), L(15), L(16), P(double, 17), P(int32_t, 18), P(double, 19), I(20), D(21), D(22), D(23), D(24), I(25),
                                        I(26), I(27), P(double, 28), P(double, 29), P(double, 30), L(31), L(32), P(double, 33), L(34), L(35), a[36].p);
        };
        e.viol = {{0, NUL, BAS_E_NULL}, {28, NUL, BAS_E_NULL}, {29, NUL, BAS_E_NULL}, {25, 0, BAS_E_SHAPE}, {26, 0, BAS_E_SHAPE}, {27, 0, BAS_E_SHAPE},
                  {20, 0, BAS_E_SHAPE}, {20, 2, BAS_E_SHAPE}, {17, B(7), 18, NUL, BAS_E_NULL}, {17, B(7), 18, B(8), BAS_E_NULL},
                  {1, -1L, BAS_E_SHAPE}, {2, -1L, BAS_E_SHAPE}, {3, -1L, BAS_E_SHAPE}, {5, -1L, BAS_E_SHAPE}, {9, -1L, BAS_E_SHAPE}, {12, -1L, BAS_E_SHAPE},
                  {16, -1L, BAS_E_SHAPE}, {31, -1L, BAS_E_SHAPE}, {32, 2L, BAS_E_SHAPE}, {35, 2L, BAS_E_SHAPE}, {34, -1L, BAS_E_SHAPE},
                  {21, 0.0, BAS_E_SHAPE}, {21, (double)NAN, BAS_E_SHAPE}, {21, (double)INFINITY, BAS_E_SHAPE}, {22, 0.0, BAS_E_SHAPE}, {22, -1.0, BAS_E_SHAPE},
                  {23, -1.0, BAS_E_SHAPE}, {24, -1.0, BAS_E_SHAPE}, {23, (double)NAN, BAS_E_SHAPE}, {7, -1.0, BAS_E_SHAPE}, {7, (double)NAN, BAS_E_SHAPE},
                  {7, (double)INFINITY, BAS_E_SHAPE}, {4, B(9), BAS_E_SHAPE}, {29, B(3), BAS_E_SHAPE}, {30, B(4), BAS_E_SHAPE}, {33, B(5), BAS_E_SHAPE},
                  {0, B(0, 4), BAS_E_ALIGN}, {28, B(3, 4), BAS_E_ALIGN}, {33, B(6, 4), BAS_E_ALIGN}, {8, B(9, 4), BAS_E_ALIGN},
                  {26, 65536, 20, 65536, BAS_E_SHAPE}, {30, NUL, ANY}, {33, NUL, ANY}, {24, (double)INFINITY, ANY},
                  {25, INT_MAX, 31, LONG_MAX, ANY}, {27, INT_MAX, 32, LONG_MAX / 4, ANY}};
        t.push_back(e);
    }
    t.push_back({"bas_resample_up_f64", {B(0), 4, 128, B(1), 40, 8, B(2), NUL},
                 [](const Args &a) { return bas_resample_up_f64(P(double, 0), I(1), I(2), P(double, 3), I(4), I(5), P(double, 6), a[7].p); },
                 {{0, NUL, BAS_E_NULL}, {3, NUL, BAS_E_NULL}, {6, NUL, BAS_E_NULL}, {1, 0, BAS_E_SHAPE}, {2, 0, BAS_E_SHAPE}, {4, 0, BAS_E_SHAPE},
                  {5, 0, BAS_E_SHAPE}, {5, -1, BAS_E_SHAPE}, {2, 1 << 20, 5, 1 << 10, BAS_E_SHAPE}, {2, INT_MAX, 5, INT_MAX, BAS_E_SHAPE},
                  {4, 1 << 20, BAS_E_SHAPE}, {4, INT_MAX, BAS_E_SHAPE}, {2, 8200, BAS_E_SHAPE}, {1, INT_MAX, ANY}}});
    t.push_back({"bas_delaydiffs_f64", {B(0), 187, 128, B(1), 40, 8, B(2), B(3), NUL},
                 [](const Args &a) {
                     return bas_delaydiffs_f64(P(double, 0), I(1), I(2), P(double, 3), I(4), I(5), P(double, 6), P(unsigned long long, 7), a[8].p);
                 },
                 {{0, NUL, BAS_E_NULL}, {3, NUL, BAS_E_NULL}, {6, NUL, BAS_E_NULL}, {7, NUL, BAS_E_NULL}, {7, B(3, 4), BAS_E_ALIGN}, {1, 0, BAS_E_SHAPE},
                  {2, 0, BAS_E_SHAPE}, {4, 0, BAS_E_SHAPE}, {5, 0, BAS_E_SHAPE}, {1, 65536, BAS_E_SHAPE}, {2, 4100, BAS_E_SHAPE},
                  {2, 1 << 29, 5, 1, BAS_E_SHAPE}, {2, (1 << 30) - 1, 5, 1, BAS_E_SHAPE}, {4, (1 << 20) - 1, BAS_E_SHAPE}}});
    return t;
}

#define TFAIL(...)                                   \
    do {                                             \
        char text_[600];                             \
        snprintf(text_, sizeof(text_), __VA_ARGS__); \
        hostsan_fail(__LINE__, text_);               \
    } while (0)

const char *last_error() {
    const char *e = bas_last_error();
    return e ? e : "";
}

}  // namespace

int section_b() {
    const std::vector<Entry> table = build_table();
    long n = 0;
    for (const Entry &e : table)
        for (size_t v = 0; v < e.viol.size(); ++v) {
            const Viol &vi = e.viol[v];
            Args a = e.valid;
            a[vi.at] = vi.value;
            if (vi.at2 >= 0) a[vi.at2] = vi.value2;
            const int rc = e.call(a);
            ++n;
            if (vi.want == ANY) {
                if (rc == 0) TFAIL("%s violation %zu (argument %d): returned 0 without a device", e.name, v, vi.at);
            } else if (rc != vi.want) {
                TFAIL("%s violation %zu (argument %d): returned %d, bas.h documents %d (\"%s\")", e.name, v, vi.at, rc, vi.want, last_error());
            }
            if (rc != 0 && !last_error()[0]) TFAIL("%s violation %zu (argument %d): code %d without a text", e.name, v, vi.at, rc);
            if (vi.want != ANY && rc == vi.want && !strstr(last_error(), "bas_") && !strstr(last_error(), e.name))
                TFAIL("%s violation %zu: the text \"%s\" does not name the entry point", e.name, v, last_error());
        }
    printf("hostsan: section b: %zu entry points, %ld violations\n", table.size(), n);
    return hostsan_failures();
}

int section_c() {
    const std::vector<Entry> table = build_table();
    for (const Entry &e : table) {
        const int rc = e.call(e.valid);
        if (rc <= 0) TFAIL("%s with valid arguments and no device returned %d (\"%s\"): a positive hipError_t is due", e.name, rc, last_error());
        else if (!last_error()[0]) TFAIL("%s: hipError_t %d without a text", e.name, rc);
    }
    printf("hostsan: section c: %zu entry points\n", table.size());
    return hostsan_failures();
}
