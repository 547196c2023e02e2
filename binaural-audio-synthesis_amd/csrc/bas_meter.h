// The loudness and true-peak meter's sizes and its host arithmetic (bas_meter.hip; include/bas.h "loudness meter";
// DESIGN.md §3.20).  Plain C++ with no HIP in it: tests/hostsan/hostsan_meter.cpp builds this file for the host alone.
#pragma once
#include <math.h>
#include <stddef.h>

#define MET_THREADS 256
#define MET_SCAN_STEPS 8                           // log2(MET_THREADS): doubling steps of the scan over the runs
#define MET_TAPS 12                                // taps of one true-peak phase: j = -5 .. 6
#define MET_CTX (MET_TAPS - 1)                     // input samples in front of a block that its first windows read
#define MET_PHASES 3                               // the interpolated phases 1/4, 2/4, 3/4 (phase 0: the samples)
#define MET_FS_MIN 8000
#define MET_FS_MAX 192000
// One session's carried state, in 8-byte words: two ears of MET_EAR_WORDS each.  An ear's words:
//   0 the sample count, 1 its copy for the launches behind the first (no launch reads a word that it writes),
//   2..5 the cascade's four states, 6 the open hop's running sum, 7..12 the last 11 input samples (binary32, one spare),
//   13 the running true peak (the bits of a binary32 value >= 0 in the low half), 14..19 the samples' copy for the launches
//   behind the first
#define MET_W_COUNT 0
#define MET_W_SHADOW 1
#define MET_W_FILT 2
#define MET_W_OPEN 6
#define MET_W_CTX 7
#define MET_W_PEAK 13
#define MET_W_CTX_SHADOW 14
#define MET_EAR_WORDS 20
#define MET_STATE_WORDS (2 * MET_EAR_WORDS)
// a unit's words in the workspace: its zero-state end state (unit 0: its true end state), then its entry state
#define MET_WS_UNIT_WORDS 8

// What the kernels take by value: the cascade, the transition matrix's powers and the true-peak taps.
struct MeterParams {
    double b[3], a[2];                             // stage 1 (shelf), a0 = 1
    double c[3], d[2];                             // stage 2 (high-pass), numerator (1, -2, 1)
    double P[MET_SCAN_STEPS][16];                  // A^(R 2^i), row-major: the scan's step i
    double Ahop[16];                               // A^hop: the chain over whole hops
    float taps[MET_PHASES * MET_TAPS];             // g_p[j] at (p - 1) 12 + j + 5
    int R, hop;                                    // run length of a thread: ceil(hop / 256)
};

// K-weighting at fs (include/bas.h): K = tan(pi f0 / fs), a0 = 1 + K/Q + K^2
static inline void meter_kweighting(double fs, double *b, double *a, double *c, double *d) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        b[0] = (Vh + Vb * K / Q + K * K) / a0;
        b[1] = 2.0 * (K * K - Vh) / a0;
        b[2] = (Vh - Vb * K / Q + K * K) / a0;
        a[0] = 2.0 * (K * K - 1.0) / a0;
        a[1] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        c[0] = 1.0;
        c[1] = -2.0;
        c[2] = 1.0;
        d[0] = 2.0 * (K * K - 1.0) / a0;
        d[1] = (1.0 - K / Q + K * K) / a0;
    }
}

// The transition matrix of the two transposed-direct-form-II biquads as ONE system on (s1, s2, t1, t2):
//   y1 = b0 x + s1;  s1' = b1 x - a1 y1 + s2;  s2' = b2 x - a2 y1;  y2 = c0 y1 + t1;  t1' = c1 y1 - d1 y2 + t2;  t2' = c2 y1 - d2 y2
static inline void meter_transition(const double *a, const double *c, const double *d, double *A) {
    for (int i = 0; i < 16; ++i) A[i] = 0.0;
    A[0] = -a[0];  A[1] = 1.0;
    A[4] = -a[1];
    A[8] = c[1] - d[0] * c[0];   A[10] = -d[0];  A[11] = 1.0;
    A[12] = c[2] - d[1] * c[0];  A[14] = -d[1];
}

// The powers are formed in the host's long double and rounded to binary64 once.  The high-pass has two poles within
// eps = (pi f0 / fs) / Q of 1, so A^n reacts to a relative error u in a factor as up to 16 n u / eps^2: binary64 squaring
// was seen 5e-8 of the power's largest entry off at n = 8832 (176.4 kHz), the x87 format (u = 2^-64) 3e-11.
typedef long double meter_wide;

static inline void meter_matmul(const meter_wide *X, const meter_wide *Y, meter_wide *Z) {   // Z = X Y (Z apart from X, Y)
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            meter_wide s = 0;
            for (int k = 0; k < 4; ++k) s += X[4 * i + k] * Y[4 * k + j];
            Z[4 * i + j] = s;
        }
}

// A^n by squaring, n >= 0
static inline void meter_matpow(const meter_wide *A, long n, meter_wide *out) {
    meter_wide acc[16], sq[16], t[16];
    for (int i = 0; i < 16; ++i) {
        acc[i] = (i % 5 == 0) ? 1 : 0;
        sq[i] = A[i];
    }
    for (; n > 0; n >>= 1) {
        if (n & 1) {
            meter_matmul(acc, sq, t);
            for (int i = 0; i < 16; ++i) acc[i] = t[i];
        }
        meter_matmul(sq, sq, t);
        for (int i = 0; i < 16; ++i) sq[i] = t[i];
    }
    for (int i = 0; i < 16; ++i) out[i] = acc[i];
}

static inline bool meter_fs_ok(int fs) { return fs >= MET_FS_MIN && fs <= MET_FS_MAX && fs % 10 == 0; }

// Everything a launch takes by value, for a valid fs: the cascade, A^(R 2^i) by repeated squaring of A^R, A^hop, the taps.
static inline void meter_params(int fs, const float *taps, MeterParams *F) {
    meter_kweighting((double)fs, F->b, F->a, F->c, F->d);
    F->hop = fs / 10;
    F->R = (F->hop + MET_THREADS - 1) / MET_THREADS;
    double Ad[16];
    meter_wide A[16], P[16], t[16];
    meter_transition(F->a, F->c, F->d, Ad);
    for (int k = 0; k < 16; ++k) A[k] = Ad[k];
    meter_matpow(A, F->R, P);
    for (int i = 0; i < MET_SCAN_STEPS; ++i) {
        for (int k = 0; k < 16; ++k) F->P[i][k] = (double)P[k];
        meter_matmul(P, P, t);
        for (int k = 0; k < 16; ++k) P[k] = t[k];
    }
    meter_matpow(A, F->hop, P);
    for (int k = 0; k < 16; ++k) F->Ahop[k] = (double)P[k];
    for (int i = 0; i < MET_PHASES * MET_TAPS; ++i) F->taps[i] = taps[i];
}

// units of one (session, ear) in a call of more than hop + 1 samples, whatever the open hop holds: the first closes the
// open hop (1 .. hop samples), the others are whole hops and a last part
static inline long meter_max_units(long T, int hop) { return T <= 0 ? 0 : 1 + (T - 1 + hop - 1) / hop; }
// floats of the kernels' sample array in LDS: a unit (or a block of hop + 1), 11 samples in front, 11 zeros behind
static inline size_t meter_lds_bytes(int hop) {
    return (((size_t)hop + 1 + 2 * MET_CTX + 3) & ~(size_t)3) * sizeof(float);
}
