// What the single-file sanitizer programs share (hostsan_encode, hostsan_design, hostsan_occlude, hostsan_meter).  A program
// defines HOSTSAN_NAME (the name its lines start with) before it includes this, and keeps its own main.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/bas.h"

#ifndef HOSTSAN_NAME
#error "define HOSTSAN_NAME before including hostsan_common.h"
#endif

static int g_fail = 0, g_checks = 0;

// rc against the code bas.h documents (want > 0: any positive hipError_t - there is no device to run on)
static inline void expect(int line, const char *what, int rc, int want, const char *entry) {
    ++g_checks;
    const char *text = bas_last_error();
    bool ok = want > 0 ? rc > 0 : rc == want;
    if (ok && want != 0) ok = text && strstr(text, entry) != nullptr;      // every failure leaves a text naming the entry
    if (!ok && ++g_fail <= 40)
        fprintf(stderr, HOSTSAN_NAME ": FAIL line %d: %s: returned %d, want %s%d, text \"%s\"\n", line, what, rc,
                want > 0 ? "> " : "", want > 0 ? 0 : want, text ? text : "(null)");
}
#define EXPECT(what, call, want, entry) expect(__LINE__, what, (call), (want), entry)

static const int E_NULL = -1, E_SHAPE = -2, E_ALIGN = -3, NO_DEVICE = 1;

// a made-up device address: the host code never dereferences it
template <class T>
static inline T *at(uintptr_t base, long bytes) {
    return reinterpret_cast<T *>(base + bytes);
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static inline double uniform() {                                            // xorshift64*, in [0, 1)
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return (double)((g_rng * 0x2545f4914f6cdd1dull) >> 11) / 9007199254740992.0;
}
static inline double between(double a, double b) { return a + (b - a) * uniform(); }

// True, with the refusal line printed, where a GPU is visible: main then returns 77.
static inline bool hostsan_gpu_visible(const char *name) {
    int n_dev = 0;
    const hipError_t e = hipGetDeviceCount(&n_dev);
    if (e == hipSuccess && n_dev > 0) {
        printf("%s: refused: %d GPU device(s) visible - sanitized host code never drives a GPU; hide them "
               "(HIP_VISIBLE_DEVICES=-1)\n", name, n_dev);
        return true;
    }
    (void)hipGetLastError();
    return false;
}
