// The stereo output filter: sizes, the launch plan and the argument checks (bas_output.hip; include/bas_output.h; DESIGN.md
// §3.25).  The functions here are host code (no kernel calls them); tests/hostsan/hostsan_output.cpp includes this header
// for them.
#pragma once
#include "bas_internal.h"
#include "bas_views.h"
#include "../../include/bas_output.h"

#define OUT_U 3                                   // consecutive frames a thread owns: 2 U (full) or U (diagonal) binary64 chains per pass
#define OUT_THREADS 192                           // three waves; a lane's frames are 3 doubles apart in LDS: no bank is hit twice
#define OUT_TILE BAS_OUTPUT_TILE                  // output frames per workgroup (output.TILE)
#define OUT_KB 12                                 // steps of k whose taps and samples are read ahead together
static_assert(OUT_TILE == OUT_U * OUT_THREADS, "a tile is U frames of every thread");

// What a launch keeps in LDS, as binary64: the session's taps ([2][M][2] = [i][k][o] full, [2][M] = [o][k] diagonal), then
// the window's part of the tile, channel after channel: OUT_TILE + M - 1 frames each.
struct OutputPlan {
    int taps_doubles, window_doubles;             // the window's frames per channel
    size_t lds_bytes;
};
static inline OutputPlan output_plan(int M, int full) {
    OutputPlan P;
    P.taps_doubles = (full ? 4 : 2) * M;
    P.window_doubles = OUT_TILE + M - 1;
    P.lds_bytes = sizeof(double) * ((size_t)P.taps_doubles + 2 * (size_t)P.window_doubles);
    return P;
}

// Every check of bas_output_filter_f32, before any launch: 0, or the BAS_E_* code with the text set.  *nothing is set where
// the call is a legal no-op (no pointer is looked at).
static inline int output_check(const float *y, long y_g, long y_t, long y_c, int G, long T_win, long first, const float *taps,
                               long taps_g, int M, int full, const float *out, long o_g, long o_t, long o_c, long T_out,
                               bool *nothing) {
    *nothing = false;
    BAS_REQUIRE(M >= 1 && M <= BAS_OUTPUT_MAX_TAPS, BAS_E_SHAPE, "bas_output_filter_f32: M (%d) must be in 1..%d", M,
                BAS_OUTPUT_MAX_TAPS);
    BAS_REQUIRE(G >= 0 && G <= 65535, BAS_E_SHAPE, "bas_output_filter_f32: n_sessions (%d) must be in 0..65535", G);
    BAS_REQUIRE(T_win >= 0 && T_win < (1L << 31), BAS_E_SHAPE, "bas_output_filter_f32: T_win (%ld) must be in 0..2^31 - 1", T_win);
    BAS_REQUIRE(first >= 0 && first < (1L << 31), BAS_E_SHAPE, "bas_output_filter_f32: first (%ld) must be in 0..2^31 - 1", first);
    BAS_REQUIRE(T_out >= 0 && T_out < (1L << 30), BAS_E_SHAPE, "bas_output_filter_f32: T_out (%ld) must be in 0..2^30 - 1", T_out);
    BAS_REQUIRE(bas_none_negative({y_g, y_t, y_c, taps_g, o_g, o_t, o_c}), BAS_E_SHAPE,
                "bas_output_filter_f32: strides must be >= 0");
    BAS_REQUIRE(bas_all_below(1L << 40, {y_g, taps_g, o_g}) && bas_all_below(1L << 31, {y_t, y_c, o_t, o_c}), BAS_E_SHAPE,
                "bas_output_filter_f32: strides must be below 2^40 (session) and 2^31 (frame, channel)");
    const long set = (long)(full ? 4 : 2) * M;
    BAS_REQUIRE(taps_g == 0 || taps_g >= set, BAS_E_SHAPE,
                "bas_output_filter_f32: taps_stride_g (%ld) must be 0 (one set for all) or >= the set's %ld floats", taps_g, set);
    if (G == 0 || T_out == 0) {
        *nothing = true;
        return 0;
    }
    BAS_REQUIRE(out && taps && (y || T_win == 0), BAS_E_NULL, "bas_output_filter_f32: null pointer");
    BAS_REQUIRE(bas_aligned(y, 4) && bas_aligned(taps, 4) && bas_aligned(out, 4), BAS_E_ALIGN,
                "bas_output_filter_f32: y, taps and out must be 4-byte aligned");
    const long in_extent[3] = {G, T_win, 2}, in_stride[3] = {y_g, y_t, y_c};
    const long out_extent[3] = {G, T_out, 2}, out_stride[3] = {o_g, o_t, o_c};
    BAS_REQUIRE(bas_layout_nested(3, out_extent, out_stride), BAS_E_SHAPE,
                "bas_output_filter_f32: the output's strides address an element twice");
    const size_t out_bytes = 4 * (size_t)bas_view_extent(3, out_extent, out_stride);
    BAS_REQUIRE(T_win == 0 || !bas_ranges_meet(y, 4 * (size_t)bas_view_extent(3, in_extent, in_stride), out, out_bytes),
                BAS_E_SHAPE, "bas_output_filter_f32: input and output overlap");
    BAS_REQUIRE(!bas_ranges_meet(taps, 4 * (size_t)((G - 1) * taps_g + set), out, out_bytes), BAS_E_SHAPE,
                "bas_output_filter_f32: taps and output overlap");
    return 0;
}
