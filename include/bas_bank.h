/* bas_bank.h - HRTF table banks of libbas_hip.so, beside the ABI of bas.h: the same conventions (device
 * pointers, one stream, no allocation, no synchronisation, 0 / BAS_E_* / hipError_t, the text of bas_last_error), the same
 * library, BAS_ABI_VERSION untouched.  The reference has no counterpart: it renders through one HRIR set.
 *
 * ---- the bank ---------------------------------------------------------------------------------------------------------
 * A bank is n_tables tables of the SAME ndir, L and U (U >= 4: the read plans' form) side by side in two allocations:
 *     packed [n_tables][2][ndir][U][L + 4] f32     each slice exactly what bas_table_pack_f32 writes (guards included),
 *     diffs  [n_tables][2][ndir][ndir]     f64     each slice a table's two delay-difference matrices.
 * The whole of `packed` must stay below 2^31 bytes: n_tables 2 ndir U (L + 4) 4 < 2^31 (the kernels address it through
 * 32-bit byte offsets off one buffer resource); a larger bank is BAS_E_SHAPE.
 * table_of [cols] i32 holds one table index per chunk-boundary COLUMN: the n queries of a call are rows of `cols`
 * boundaries (n % cols == 0; the angle rows [n_src][cols] of a render), and query q is planned with table
 * table_of[q % cols].  An index outside [0, n_tables) is clamped into it on the device (memory safety, as direction
 * indices are clamped; nothing is validated there).
 * A read plan of a bank differs from the plan of table t alone in its 16 byte offsets only: each is the single-table offset
 * plus t 2 ndir U (L + 4) 4.  Weights and o4 are the same bits.  So the FIR entry points of bas.h that take (packed, plans,
 * ndir) serve a bank unchanged when they are given the bank's `packed` and n_tables ndir as ndir (there ndir only sizes the
 * table resource).
 *
 *   bas_interp2d_plan_angles_bank_f32: bas_interp2d_plan_angles_gain_f32 over a bank.  gain may be NULL (no gain: the
 *     weights of bas_interp2d_plan_angles_f32).  ndir is per table.
 *   bas_interp2d_bank_f32: bas_interp2d_gain_f32 over a bank (the stored-IR path: plans into ws, then H [n][2][L]).  gain may
 *     be NULL.  `packed` and `diffs` are the bank's.
 *   Both: every argument check runs before the launch - BAS_E_NULL (a required pointer with n > 0; table_of included),
 *   BAS_E_SHAPE (n < 0, ndir, L <= 0, U < 4, n_tables <= 0, cols <= 0, n % cols != 0, a branch that is neither, a ring outside
 *   the ndir directions, a bank of 2^31 bytes or more), BAS_E_WORKSPACE (plans / ws smaller than
 *   bas_interp2d_workspace_bytes(n) or not 16-byte aligned).  n = 0: nothing to do. */
#ifndef BAS_BANK_H
#define BAS_BANK_H

#include "bas.h"

#ifdef __cplusplus
extern "C" {
#endif

int bas_interp2d_plan_angles_bank_f32(const double *diffs, const double *elev, const double *azim, const double *gain,
                                      int n, const double *ring_elev, const int32_t *ring_start,
                                      const int32_t *ring_count, const float *node_az, int branch, int ndir, int L,
                                      int U, void *plans, size_t plans_bytes, const int32_t *table_of, int cols,
                                      int n_tables, bas_stream_t stream);
int bas_interp2d_bank_f32(const float *packed, const double *diffs, const int32_t *idx, const double *w,
                          const double *gain, int n, int ndir, int L, int U, float *H, void *ws, size_t ws_bytes,
                          const int32_t *table_of, int cols, int n_tables, bas_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
