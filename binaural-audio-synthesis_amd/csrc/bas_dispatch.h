// Host dispatch of the FIR kernels: ONE record, BasPlan, says which kernel renders a shape, with what launch geometry and
// what follows it.  The planners (plan_render in bas_render.hip, fz_plan in bas_fused.hip) fill it; its kernel is a row of the
// kernel table, defined beside each kernel; the public name functions, the launches and the diagnostic exports read both.
#pragma once
#include "bas_internal.h"
#include <limits.h>

// What the diagnostic build (-DBAS_DIAG) takes from the environment; the shipped build never reads it.
#define BAS_DIAG_UNSET INT_MIN
enum { BAS_FORCE_NONE = 0, BAS_FORCE_GENERIC, BAS_FORCE_ROWS32, BAS_FORCE_HD, BAS_FORCE_OTHER };
struct BasDiag {
    int force_kernel = BAS_FORCE_NONE;      // BAS_FORCE_KERNEL: the stored-IR kernel (tests force the fallback kernels)
    int fz_nw = BAS_DIAG_UNSET;             // BAS_FZ_NW: waves per tile of 2048 x nw
    int fz_split = BAS_DIAG_UNSET;          // BAS_FZ_SPLIT: the split-role kernel wherever it fits (1) or nowhere (0)
    int fz_quad = BAS_DIAG_UNSET;           // BAS_FZ_QUAD: the four-wave kernel of small scenes likewise
    int fz_wg_per_cu = BAS_DIAG_UNSET;      // BAS_FZ_WG_PER_CU: e.g. a workgroup alone on its CU
    int fs_taps_once = BAS_DIAG_UNSET;      // BAS_FS_TAPS_ONCE=0: the unit block that reads every tap twice
    int debug_flags = 0;                    // BAS_DEBUG_FLAGS (RenderArgs.dbg; & 256: FzArgs.inject)
};
BasDiag bas_diag();                         // (bas_render.hip) shipped build: the defaults; diagnostic build: read on every call

// A row of the kernel table.  key: the template arguments as one number, unique within the kernel's rows; code: the row's
// bits of bas_debug_fused_plan.
struct BasKernelRow {
    const char *instance;                   // the kernel with all its template arguments
    const char *public_name;                // what bas_render_kernel_name / bas_render_fused_kernel_name return
    const void *fn;
    int threads;                            // per workgroup
    int key, code;
};
template <int N> static inline const BasKernelRow *bas_find_row(const BasKernelRow (&rows)[N], int key) {
    for (const BasKernelRow &r : rows)
        if (r.key == key) return &r;
    return nullptr;                         // (this build holds no such instance)
}
const BasKernelRow *bas_fs_row(int Lp, int S, const BasDiag &D);   // bas_fused_split.hip
const BasKernelRow *bas_fq_row();                                  // bas_fused_quad.hip

enum { BAS_REDUCE_NONE = 0, BAS_REDUCE_PLAIN = 1, BAS_REDUCE_WIDE = 2 };
#define BAS_PLAN_FIELDS 12                  // what bas_plan_fields writes
struct BasPlan {
    const BasKernelRow *row;                // null: shape not served (fused path)
    int tile;                               // outputs per tile (0: the generic kernel, no tiles)
    long n_tiles, units_total;
    int n_wg, units_per_wg, parts_per_wg;
    int nslots, spw;                        // chunk slots per pass, per wave (h-only fz rows)
    size_t lds_bytes, slab_bytes;
    int direct;                             // the FIR kernel writes y itself: every tile is finished by ONE workgroup
    int reduce;                             // what follows it: BAS_REDUCE_*
};

// The tail of every plan: tiles, the deal of the (tile, source) units over `slots` workgroups, and what follows the kernel.
// Many sources on a short signal - more than 24 workgroups can share a tile - sum the parts in parallel (the wide reduce).
static inline void bas_plan_deal(BasPlan &p, int tile, long T_out, int n_src, long slots, bool may_direct) {
    p.tile = tile;
    p.n_tiles = (T_out + tile - 1) / tile;
    p.units_total = p.n_tiles * n_src;
    bas_deal_units(p.units_total, slots, n_src, tile, &p.units_per_wg, &p.n_wg, &p.parts_per_wg, &p.slab_bytes);
    p.direct = may_direct && p.units_per_wg % n_src == 0;
    const int parts = p.units_per_wg ? (n_src + p.units_per_wg - 1) / p.units_per_wg + 1 : 0;
    p.reduce = p.direct ? BAS_REDUCE_NONE : parts > 24 ? BAS_REDUCE_WIDE : BAS_REDUCE_PLAIN;
}

// every field, in declaration order, for the diagnostic exports
static inline void bas_plan_fields(const BasPlan &p, long *out) {
    const long f[BAS_PLAN_FIELDS] = {p.tile, p.n_tiles, p.units_total, p.n_wg, p.units_per_wg, p.parts_per_wg, p.nslots, p.spw,
                                     (long)p.lds_bytes, (long)p.slab_bytes, p.direct, p.reduce};
    for (int i = 0; i < BAS_PLAN_FIELDS; ++i) out[i] = f[i];
}

BasPlan plan_render(int n_src, long T_in, int K, int S, int L, bool aligned, const BasDiag &D);   // the stored-IR path's
// slabs of partial tiles -> y by the plan's reduce kernel (bas_render.hip)
int bas_launch_slab_reduce(const float *slab, const BasPlan &p, int n_src, long T_out, float *y, int accumulate,
                           unsigned int *peak_bits, const BasTail *tail, int *tail_skipped, const BasCarry *carry,
                           hipStream_t st, const char *what);
