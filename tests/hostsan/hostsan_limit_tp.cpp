// The host half of the true-peak limiter (include/bas_limit_tp.h) under AddressSanitizer and
// UndefinedBehaviorSanitizer, stand-alone: `make -C binaural-audio-synthesis_amd/csrc hostsan_limit_tp` links this file with
// the library's objects (host code sanitized, device code as shipped).  Two parts:
//   1. bas_limit_tp_f32: valid argument lists - a whole signal, a stream block of one tile and of several, a stream's end, the
//      smallest and the largest setting, planar layouts, the far end of the index range - which with no device to run on
//      return a positive hipError_t, and the violations, each of which returns the code bas_limit_tp.h documents and leaves a
//      text naming the entry point.  No pointer is dereferenced by the host code.
//   2. the state size and the launch plan of bas_limit_tp.h for every (A, Hd) on a grid that holds the extremes: the ring two
//      reaches longer than the look-ahead limiter's, the two LDS arrays on 16-byte boundaries, inside 64 KiB, with room for
//      every raw sample and every sum a full tile reads; one launch up to a tile, two beyond.
// Exits 77 where a GPU is visible.
#include <climits>
#include <cmath>

#define HOSTSAN_NAME "hostsan_limit_tp"
#include "hostsan_common.h"
#include "../../binaural-audio-synthesis_amd/csrc/bas_limit_tp.h"

struct Lim {
    const float *y;
    long y_g, y_t, y_e;
    float *out;
    long o_g, o_t, o_e;
    int G;
    long T_in, T_out;
    double c;
    int A, Hd;
    float *state;
    long ss;
    float *red, *peak;
    int call() const {
        return bas_limit_tp_f32(y, y_g, y_t, y_e, out, o_g, o_t, o_e, G, T_in, T_out, c, A, Hd, state, ss, red, peak, nullptr);
    }
};

static void entry_section() {
    static const char *E = "bas_limit_tp_f32";
    const uintptr_t b = uintptr_t(1) << 32;                                  // made-up device addresses
    const long need = 4 + 2 * (2 * 16 + 32 + 12);                            // 156 floats
    const Lim ok = {at<const float>(b, 0), 1024, 2, 1, at<float>(b, 1 << 20), 1024, 2, 1, 3, 512, 512, 0.5, 16, 32,
                    at<float>(b, 1 << 22), need, at<float>(b, 1 << 24), at<float>(b, (1 << 24) + 64)};
    Lim a;
    EXPECT("a stream block, no device", ok.call(), NO_DEVICE, E);
    a = ok; a.state = nullptr; a.ss = 0;
    EXPECT("a whole signal, no device", a.call(), NO_DEVICE, E);
    a = ok; a.T_in = a.T_out = 5000; a.y_g = a.o_g = 10000;
    EXPECT("a block of several tiles, no device", a.call(), NO_DEVICE, E);
    a = ok; a.T_in = 0; a.T_out = 16 + 6; a.y = nullptr;
    EXPECT("a stream's end, no device", a.call(), NO_DEVICE, E);
    a = ok; a.T_in = a.T_out = 1;
    EXPECT("a block of one sample, no device", a.call(), NO_DEVICE, E);
    a = ok; a.A = 0; a.Hd = 0; a.ss = 28;
    EXPECT("the smallest setting, no device", a.call(), NO_DEVICE, E);
    a = ok; a.A = 1024; a.Hd = 4096; a.ss = 4 + 2 * 6156;
    EXPECT("the largest setting, no device", a.call(), NO_DEVICE, E);
    a = ok; a.red = a.peak = nullptr;
    EXPECT("no meters, no device", a.call(), NO_DEVICE, E);
    a = ok; a.y_g = 2 * 600; a.y_t = 1; a.y_e = 600; a.o_g = 2 * 600; a.o_t = 1; a.o_e = 600;
    EXPECT("planar in and out, no device", a.call(), NO_DEVICE, E);
    a = ok; a.G = 1; a.state = nullptr; a.ss = 0; a.T_in = a.T_out = (1L << 30) - 1; a.out = at<float>(b, 1L << 36);
    EXPECT("the far end of the index range, no device", a.call(), NO_DEVICE, E);
    a = ok; a.T_in = a.T_out = 0; a.y = nullptr; a.out = nullptr; EXPECT("no samples", a.call(), 0, E);
    a = ok; a.G = 0; a.y = nullptr; a.out = nullptr; EXPECT("no sessions", a.call(), 0, E);
    // ---- shapes
    for (int v : {-1, 1025, INT_MAX, INT_MIN}) { a = ok; a.A = v; EXPECT("lookahead", a.call(), E_SHAPE, E); }
    for (int v : {-1, 4097, INT_MAX, INT_MIN}) { a = ok; a.Hd = v; EXPECT("hold", a.call(), E_SHAPE, E); }
    for (double v : {0.0, -0.5, 0.1, 1e39, 1e-42, (double)NAN, (double)INFINITY}) { a = ok; a.c = v; EXPECT("ceiling", a.call(), E_SHAPE, E); }
    for (int v : {-1, 65536, INT_MAX}) { a = ok; a.G = v; EXPECT("n_sessions", a.call(), E_SHAPE, E); }
    for (long v : {-1L, 1L << 30, LONG_MAX, LONG_MIN}) { a = ok; a.T_in = a.T_out = v; EXPECT("T", a.call(), E_SHAPE, E); }
    a = ok; a.T_out = 513; EXPECT("T_out beside T_in", a.call(), E_SHAPE, E);
    a = ok; a.T_in = 0; a.state = nullptr; EXPECT("an end without a state", a.call(), E_SHAPE, E);
    for (int i = 0; i < 7; ++i) {
        a = ok;
        long *f[7] = {&a.y_g, &a.y_t, &a.y_e, &a.o_g, &a.o_t, &a.o_e, &a.ss};
        *f[i] = -4;
        EXPECT("negative stride", a.call(), E_SHAPE, E);
        a = ok;
        *f[i] = LONG_MIN;
        EXPECT("most negative stride", a.call(), E_SHAPE, E);
        a = ok;
        *f[i] = (i == 1 || i == 4) ? 1L << 31 : 1L << 40;
        EXPECT("stride too large", a.call(), E_SHAPE, E);
        a = ok;
        *f[i] = LONG_MAX;
        EXPECT("largest stride", a.call(), E_SHAPE, E);
    }
    a = ok; a.ss = need - 4; EXPECT("a state too small", a.call(), E_SHAPE, E);
    a = ok; a.ss = 4 + 2 * (2 * 16 + 32); EXPECT("the look-ahead limiter's state", a.call(), E_SHAPE, E);
    a = ok; a.ss = need + 2; EXPECT("a state stride that is no multiple of 4", a.call(), E_SHAPE, E);
    a = ok; a.o_g = 1023; EXPECT("output sessions overlap", a.call(), E_SHAPE, E);
    a = ok; a.o_g = 0; EXPECT("output sessions on each other", a.call(), E_SHAPE, E);
    a = ok; a.o_t = 1; EXPECT("output ears on the next sample", a.call(), E_SHAPE, E);
    a = ok; a.o_e = 0; EXPECT("output ears on each other", a.call(), E_SHAPE, E);
    a = ok; a.out = at<float>(b, 4 * 500); EXPECT("output inside the input", a.call(), E_SHAPE, E);
    a = ok; a.y = at<const float>(b, (1 << 20) + 64); EXPECT("input inside the output", a.call(), E_SHAPE, E);
    a = ok; a.state = at<float>(b, (1 << 20) + 1024); EXPECT("state inside the output", a.call(), E_SHAPE, E);
    a = ok; a.out = at<float>(b, (1 << 22) + 4 * (3 * need - 20)); EXPECT("output on the ring's last frames", a.call(), E_SHAPE, E);
    // ---- NULLs and alignment
    a = ok; a.y = nullptr; EXPECT("y null", a.call(), E_NULL, E);
    a = ok; a.out = nullptr; EXPECT("out null", a.call(), E_NULL, E);
    a = ok; a.T_in = 0; a.T_out = 22; a.y = nullptr; a.out = nullptr; EXPECT("out null at the end", a.call(), E_NULL, E);
    a = ok; a.y = at<const float>(b, 2); EXPECT("y misaligned", a.call(), E_ALIGN, E);
    a = ok; a.out = at<float>(b, (1 << 20) + 1); EXPECT("out misaligned", a.call(), E_ALIGN, E);
    a = ok; a.red = at<float>(b, (1 << 24) + 2); EXPECT("reduction misaligned", a.call(), E_ALIGN, E);
    a = ok; a.peak = at<float>(b, (1 << 24) + 67); EXPECT("peak misaligned", a.call(), E_ALIGN, E);
    a = ok; a.state = at<float>(b, (1 << 22) + 8); EXPECT("state misaligned", a.call(), E_ALIGN, E);
    a = ok; a.A = -1; a.out = nullptr; EXPECT("the sizes are checked first", a.call(), E_SHAPE, E);
}

// ---- part 2: the state and the plan -----------------------------------------------------------------------------------------------
static void note(bool ok, const char *what, int A, int Hd) {
    ++g_checks;
    if (!ok && ++g_fail <= 40) fprintf(stderr, "hostsan_limit_tp: FAIL %s at A %d Hd %d\n", what, A, Hd);
}

static void plans_section() {
    const int As[] = {0, 1, 2, 5, 6, 7, 63, 64, 240, 511, 1000, 1023, 1024};
    const int Hds[] = {0, 1, 2, 3, 5, 100, 960, 2047, 4000, 4095, 4096};
    for (int A : As) {
        for (int Hd : Hds) {
            const int H = lim_history(A, Hd), HT = lim_tp_history(A, Hd);
            note(HT == 2 * A + Hd + 12 && HT == H + 2 * LIM_TP_REACH && HT > 0, "history", A, Hd);
            note(bas_limit_tp_state_floats(A, Hd) == (size_t)(4 + 2 * HT), "state floats", A, Hd);
            note(bas_limit_tp_state_floats(A, Hd) == bas_limit_state_floats(A, Hd) + 24, "state beside the limiter's", A, Hd);
            note(lim_tp_latency(A) == A + 6, "latency", A, Hd);
            const int span = lim_tp_span(A, Hd);
            // a full tile: lenq r values, 12 raw samples more, read in quads of 16 from index lenq - 4; the sums read E up
            // to index LIM_TILE - 1 + A
            const int lenq = (H + LIM_TILE + 3) & ~3;
            note(span % 4 == 0 && span >= lenq + 2 * LIM_TP_REACH && span >= lenq - 4 + 16, "raw samples", A, Hd);
            note(span > LIM_TILE - 1 + A, "sums", A, Hd);
            note(lim_tp_lds_bytes(A, Hd) == 8 * (size_t)span && lim_tp_lds_bytes(A, Hd) == lim_lds_bytes(A, Hd) + 96 &&
                     lim_tp_lds_bytes(A, Hd) <= 64 * 1024,
                 "LDS", A, Hd);
            for (long T : {1L, 5L, 1023L, 1024L, 1025L, 5000L, (1L << 30) - 1}) {
                note(lim_tp_advance(true, T, T) == (T <= LIM_TILE ? 2 : 1), "a block's carry", A, Hd);
                note(lim_tp_advance(false, T, T) == 0 && lim_tp_advance(true, 0, T) == 0, "no carry", A, Hd);
            }
        }
    }
    for (int v : {-1, 1025, 4097, INT_MIN, INT_MAX})
        note((v == 4097 || bas_limit_tp_state_floats(v, 0) == 0) && (v == 1025 || bas_limit_tp_state_floats(0, v) == 0),
             "out of range", v, v);
    note(LIM_TP_QUAD_WINDOWS == 5 && LIM_TP_TAPS == 2 * LIM_TP_REACH && LIM_TILE % (4 * LIM_THREADS) == 0, "the quads", 0, 0);
    const float taps[] = LIM_TP_TAP_VALUES;
    note(sizeof(taps) == 4 * LIM_TP_PHASES * LIM_TP_TAPS, "36 taps", 0, 0);
    for (int k = 0; k < LIM_TP_TAPS; ++k) {                                  // phase 3 is phase 1 mirrored, phase 2 symmetric
        note(taps[k] == taps[2 * LIM_TP_TAPS + LIM_TP_TAPS - 1 - k], "mirrored phases", k, 0);
        note(taps[LIM_TP_TAPS + k] == taps[LIM_TP_TAPS + LIM_TP_TAPS - 1 - k], "the middle phase", k, 0);
    }
}

int main() {
    if (hostsan_gpu_visible("hostsan_limit_tp")) return 77;
    entry_section();
    const int after_entry = g_checks;
    plans_section();
    printf("hostsan_limit_tp: bas_limit_tp_f32 %d checks, plans %d checks, %d failed\n", after_entry, g_checks - after_entry,
           g_fail);
    printf("hostsan_limit_tp: %s\n", g_fail ? "FAILED" : "ok");
    return g_fail ? 1 : 0;
}
