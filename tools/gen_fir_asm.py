#!/usr/bin/env python3
"""Generator of binaural-audio-synthesis_amd/csrc/bas_fir_asm.inc and bas_fir_once_asm.inc: the FIR of the fused kernels
(bas_fir.h: ffa_row_step_x, the 2-parallel fast FIR on a 32 x 32 Toeplitz block of packed FMAs) as hand-scheduled gfx950
assembly blocks with explicit VGPR numbers.

Why assembly: a wave that has its SIMD to itself - its CU partner is staging - waits
for the 8 tap reads of every octet before the octet's 98 FMAs (~25 % of its cycles), and hipcc cannot be made to issue
the reads of octet I + 1 under the FMAs of octet I without spilling hundreds of registers.  Here the taps are buffered in
fixed registers, and every 64-bit instruction starts at an address = 0 mod 8 (an instruction at = 4 mod 8 costs one more
issue cycle: profiles/r03_ubench_bank_placement.txt).

The core, each part once:
    Block       the typed line list of one assembly block, its .p2align placement and the in-order LDS return queue
                (issue / wait_for / landed).  Every line has a kind (KINDS); the leave-out switches remove lines BY KIND in
                Block.filtered and nowhere else: a variant block is the default block with lines taken out, nothing
                reordered, nothing added.
    fir_fmas    the fast-FIR index loop: the FMAs of half octet (i, h) as (text, x quad, tap set).
    form_taps   the crossfaded taps of a half octet: g_e, g_o, their sums, and the sum of the sums where P is split.
    Regs        a block's register map, passed as a value.
    render      the C++ wrapper around a block; what differs between the wrappers is data (Wrapper).
    parse_args  the options, parsed once and passed down; no module state.
The schedules on top of it: row_step_block (half octets by the mask), unit3_block (round 3: two x buffers), roll_block
(rolling x row; nbuf tap buffers, nsub tap sets per row, P split) and once_block (merged half octets: every tap read
once).  block_table lists what is emitted, one row per function:
    ffa_row_step_asm<XR>            row_step_block   per column stride XR of the x image          bas_fir_asm.inc
    ffa_unit_asm<261, LSEG>         roll_block(nbuf = --roll) or, with --roll=0, unit3_block      (each unit block per
    ffa_unitp_asm<261, LSEG>        roll_block(P split, PSPLIT_NBUF buffers)                       LSEG of U_LSEGS)
    ffa_unit2_asm<261, LSEG>        roll_block(two tap sets per row)
    ffa_unit4_asm<261, LSEG>        roll_block(four tap sets per row, two buffers)
    ffa_unitp1_asm<261, LSEG>       once_block: what the shipped split-role kernel runs           bas_fir_once_asm.inc

Register map of the row step (per lane; the accumulators are C++ variables pinned to these registers by "+{v[a:b]}"
constraints; the unit blocks keep the accumulators and move the operands: ROW, UNIT3, roll_regs, ONCE_N / ONCE_O):
    v[0:31]    A[p] = g_e * x_e       16 pairs (left, right)         v[98:129]   x row: 32 inputs
    v[32:63]   B[p-1] = g_o * x_o     entries 0..15                  v[130:145]  x_e + x_o: 16 sums
    v[64:95]   P[p] = (g_e+g_o)*(x_e+x_o)                            v[146:161]  taps: 4 x (h0_L, h0_R, d_L, d_R)
    v[96:97]   B entry 16                                            v[162:165] g_e[2]  v[166:169] g_o[2]  v[170:173] g_e + g_o
                                                                     v[174:175]  crossfade weight (low half)
Inputs: LDS byte address of the lane's x row, of its tap row (tap - 32 of the row distance), the weight, and the mask of
live octets (SGPR).  Arithmetic, order of accumulation per accumulator and results are those of ffa_octet_fma.

    python3 tools/gen_fir_asm.py [XR ...]    (XR = column stride of the x image in float4 units = rows + 1; default: 261 69,
                                              the tiles of 8192 and 2048 outputs)
    --check      compare with the files that are there instead of writing them;  --out=FILE  write a variant (and FILE_once)
    A/B schedules: --generic (row step without the straight-line variants, no unit blocks), --roll=N (tap buffers of
    ffa_unit_asm; 0: round 3's block), --two-waits (a wait per half octet), --spread=N (with --roll=0 only: LDS reads dealt
    over the first N/8 of the FMA run behind them), --nobranch (row step: all octets live, no mask tests),
    --taps-once-probe (ffa_unitp_asm without the second read of every tap: the ceiling of once_block).
    Leave-out variants of EVERY block (wrong results; tools/ubench_lone_wave.hip, tools/build_fir_variants.sh): --nowait
    (but a block's entry wait), --notaps, --nox, --noalign, --noform (no tap forming), --fma-keep=K (K of every 8 FIR FMAs).
"""
import argparse
import os
import sys
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "binaural-audio-synthesis_amd", "csrc", "bas_fir_asm.inc")

KINDS = ("fir", "form", "formsum", "xsum", "weight", "tapread", "xread", "wait", "align", "scalar", "label")
# leave-out switch -> the kinds it removes (--nobranch is a schedule of the row step as well: row_step_block)
LEAVE_OUT = {"nowait": ("wait",), "notaps": ("tapread",), "nox": ("xread",), "noalign": ("align",), "noform": ("form", "formsum"),
             "nobranch": ("scalar",)}
U_LSEGS = (128, 104)            # segment lengths with a unit block: L = 121 .. 128, and 97 .. 104 (the reference's default is 100)
PSPLIT_NBUF = 2

# accumulators, the same in every block: A, B (entry 16: Regs.b16), and P or, where P is split once more, PA, PB, PP
A0, B0, P0 = 0, 32, 64
PA0, PB0, PP0 = 64, 80, 98
# operand registers of a block: x row, x_e + x_o, their sums (P split), tap buffers, formed sets (12 registers each: g_e[2],
# g_o[2], g_e + g_o [2]), gs_even + gs_odd (P split), crossfade weights, B entry 16, the last register the block writes
Regs = namedtuple("Regs", "x xs xss tap g gss w b16 last")
ROW = Regs(x=98, xs=130, xss=None, tap=146, g=162, gss=None, w=174, b16=96, last=175)      # ONE tap buffer: dead once formed
UNIT3 = Regs(x=98, xs=162, xss=None, tap=178, g=210, gss=None, w=222, b16=96, last=223)    # x buffers at x, x + 32; taps at tap, tap + 16
ONCE_N = Regs(x=116, xs=148, xss=164, tap=172, g=188, gss=200, w=216, b16=114, last=217)   # the set formed for the newer row
ONCE_O = ONCE_N._replace(g=202, gss=214)                                                   # ... and for the older row


def roll_regs(nsub, nbuf, psplit):
    """P split: 18 more accumulators (PA v[64:79], PB v[80:97] (r = -1 .. 7), PP v[98:113], B entry 16 v[114:115]), the
    operands start at v116"""
    x = 116 if psplit else 98
    tap = x + 48 + (8 if psplit else 0)
    g = tap + 16 * nbuf
    gss = g + 12 * nsub
    w = gss + (2 if psplit else 0)                               # the weights of the row's nsub subchunks, two per pair
    return Regs(x=x, xs=x + 32, xss=x + 48, tap=tap, g=g, gss=gss, w=w, b16=114 if psplit else 96, last=w + (3 if nsub == 4 else 1))


def parse_args(argv):
    ap = argparse.ArgumentParser(description="writes bas_fir_asm.inc and bas_fir_once_asm.inc (see the head of this file)")
    ap.add_argument("xrs", nargs="*", type=int, metavar="XR")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--generic", action="store_true")
    ap.add_argument("--roll", type=int, default=3)
    ap.add_argument("--two-waits", action="store_true")
    ap.add_argument("--spread", type=int, default=0)
    ap.add_argument("--taps-once-probe", action="store_true")
    ap.add_argument("--fma-keep", type=int, default=8)
    for k in LEAVE_OUT:
        ap.add_argument("--" + k, action="store_true")
    o = ap.parse_args(argv)
    o.xrs = o.xrs or [261, 69]                                  # tiles of 8192 (4 waves) and 2048 (1 wave): 260 / 68 rows + 1
    o.drop = frozenset(kind for k, kinds in LEAVE_OUT.items() if getattr(o, k) for kind in kinds)
    return o


DEFAULT = parse_args([])


def pr(r):
    return f"v[{r}:{r + 1}]"


def quad(r):
    return f"v[{r}:{r + 3}]"


class Block:
    """The lines of one assembly block, each with its kind, and the LDS reads in flight (they return in order)."""

    def __init__(self, regs):
        self.regs = regs
        self.typed = []                                         # (kind, text): the WHOLE block, whatever the switches leave out
        self.queue = []                                         # tags of the reads in flight, oldest first
        self.landed = set()                                     # tags of the reads a wait has covered

    def emit(self, kind, text):
        assert kind in KINDS
        self.typed.append((kind, text))

    def align(self):
        self.emit("align", ".p2align 3")

    def issue(self, tag, kind, text):
        self.emit(kind, text)
        self.queue.append(tag)

    def wait(self, n):
        self.emit("wait", f"s_waitcnt lgkmcnt({n})")
        self.align()

    def wait_for(self, tags):
        """wait until no read with one of these tags is in flight"""
        if not any(t in tags for t in self.queue):
            return
        last = max(k for k, t in enumerate(self.queue) if t in tags)
        n = len(self.queue) - 1 - last
        assert n <= 15, n
        self.landed.update(self.queue[:last + 1])
        del self.queue[:last + 1]
        self.wait(n)

    def done(self):
        assert not self.queue, self.queue
        return self

    def filtered(self, o):
        """what the leave-out switches keep (sensitivity runs, wrong results).  A wait that opens a block stays: it is the one
        for the scalar loads of the code around the block."""
        out, n = [], 0
        for k, (kind, text) in enumerate(self.typed):
            if kind in o.drop and not (kind == "wait" and k == 0):
                continue
            if kind == "fir":
                n += 1
                if n % 8 >= o.fma_keep:
                    continue
            out.append((kind, text))
        return out

    def lines(self, o):
        return [text for _, text in self.filtered(o)]


def fir_fmas(m, i, h, nsub=1, psplit=False):
    """The FMAs of half octet (i, h) of a row step as (text, x quad read, tap set): its two half-rate taps k against the 16
    input pairs q, on the formed set of the subchunk q falls into (nsub sets per row).  psplit: the half-rate product
    P = (g_e + g_o) * (x_e + x_o) is split ONCE MORE the same way (a second fast-FIR level for one of the three products: what
    the registers of the rolling x row allow; profiles/r04_ubench_fast_fir_level2.txt): with xs = x_e + x_o, gs = g_e + g_o at
    half rate,  P[2r] = PA[r] + PB[r-1],  P[2r+1] = PP[r] - PA[r] - PB[r],  PA = gs_even * xs_even, PB = gs_odd * xs_odd,
    PP = (gs_even + gs_odd) * (xs_even + xs_odd) at quarter rate: a half octet carries ONE quarter-rate tap (its two half-rate
    taps are the even and the odd one), so its 2 x 16 P FMAs become 8 + 9 + 8 at the most."""
    for k in range(2):
        dk = 4 * i + 2 * h + k - 16
        for p in range(-1, 16):
            q = p - dk
            if not (0 <= q < 16):
                continue
            u = q // (16 // nsub)                               # subchunk of the row that inputs 2 q, 2 q + 1 fall into
            ge, go, gs = m.g + 12 * u, m.g + 12 * u + 4, m.g + 12 * u + 8
            xp = pr(m.x + 2 * q)                                # (x_e[q], x_o[q]) = inputs 2q, 2q + 1
            if p >= 0:
                yield f"v_pk_fma_f32 {pr(A0 + 2 * p)}, {pr(ge + 2 * k)}, {xp}, {pr(A0 + 2 * p)} op_sel_hi:[1,0,1]", q >> 1, u
                if not psplit:
                    sel = "op_sel:[0,1,0]" if q & 1 else "op_sel_hi:[1,0,1]"
                    yield f"v_pk_fma_f32 {pr(P0 + 2 * p)}, {pr(gs + 2 * k)}, {pr(m.xs + 2 * (q >> 1))}, {pr(P0 + 2 * p)} {sel}", q >> 1, u
            breg = m.b16 if p + 1 == 16 else B0 + 2 * (p + 1)
            yield f"v_pk_fma_f32 {pr(breg)}, {pr(go + 2 * k)}, {xp}, {pr(breg)} op_sel:[0,1,0]", q >> 1, u
    if psplit:                                                  # the quarter-rate tap j of this half octet against xs_even / xs_odd / their sum
        j = 2 * i + h - 8
        for r in range(-1, 8):
            t = r - j
            if not (0 <= t < 8):
                continue
            xs_pair = pr(m.xs + 2 * t)                          # (xs[2t], xs[2t+1]) = (xs_even[t], xs_odd[t])
            if r >= 0:
                yield f"v_pk_fma_f32 {pr(PA0 + 2 * r)}, {pr(m.g + 8)}, {xs_pair}, {pr(PA0 + 2 * r)} op_sel_hi:[1,0,1]", t, 0
                sel = "op_sel:[0,1,0]" if t & 1 else "op_sel_hi:[1,0,1]"
                yield f"v_pk_fma_f32 {pr(PP0 + 2 * r)}, {pr(m.gss)}, {pr(m.xss + 2 * (t >> 1))}, {pr(PP0 + 2 * r)} {sel}", t, 0
            yield f"v_pk_fma_f32 {pr(PB0 + 2 * (r + 1))}, {pr(m.g + 10)}, {xs_pair}, {pr(PB0 + 2 * (r + 1))} op_sel:[0,1,0]", t, 0


W_LOW, W_HIGH = "op_sel_hi:[1,0,1]", "op_sel:[0,1,0] op_sel_hi:[1,1,1]"      # the low / high half of a weight pair, for both lanes


def form_taps(b, tb, g, wp, wsel, gss=None):
    """crossfaded taps of the half octet in tap buffer tb: g = h0 + w d with the weight in half wsel of pair wp; even
    full-rate taps -> g_e, odd -> g_o, their sums, and (gss) the sum of the two sums"""
    for k in range(2):
        te, to = tb + 4 * (2 * k), tb + 4 * (2 * k + 1)
        b.emit("form", f"v_pk_fma_f32 {pr(g + 2 * k)}, {pr(te + 2)}, {wp}, {pr(te)} {wsel}")
        b.emit("form", f"v_pk_fma_f32 {pr(g + 4 + 2 * k)}, {pr(to + 2)}, {wp}, {pr(to)} {wsel}")
    for k in range(2):
        b.emit("formsum", f"v_pk_add_f32 {pr(g + 8 + 2 * k)}, {pr(g + 2 * k)}, {pr(g + 4 + 2 * k)}")
    if gss is not None:
        b.emit("formsum", f"v_pk_add_f32 {pr(gss)}, {pr(g + 8)}, {pr(g + 10)}")


def x_sums(b, m, c, psplit=False):
    """x_e + x_o of x quad c (and xs_even + xs_odd)"""
    for q in (2 * c, 2 * c + 1):
        b.emit("xsum", f"v_add_f32_e64 v{m.xs + q}, v{m.x + 2 * q}, v{m.x + 2 * q + 1}")
    if psplit:
        b.emit("xsum", f"v_add_f32_e64 v{m.xss + c}, v{m.xs + 2 * c}, v{m.xs + 2 * c + 1}")


def row_step_block(xr_stride, o):
    """The schedule works in HALF octets (4 taps = 16 registers): forming the crossfaded taps consumes the tap buffer, so
    the reads of half u + 1 go out into the SAME buffer right behind the forming of half u and land under its ~49 FMAs.
    (A whole-octet double buffer needs 60 more registers per lane; those came back as scratch traffic in the staging code
    around the block: 16 % slower than hipcc's schedule.  Two half-octet buffers: 4 % slower.)"""
    m = ROW
    b = Block(m)

    def load_taps(u):
        for j in range(4):
            b.emit("tapread", f"ds_read_b128 {quad(m.tap + 4 * j)}, %[tap] offset:{(4 * u + j) * 16}")

    def form():
        form_taps(b, m.tap, m.g, pr(m.w), W_LOW)

    def fmas(u):
        for text, _, _ in fir_fmas(m, u >> 1, u & 1):
            b.emit("fir", text)

    def prologue(first_live):
        """weight into its pair, the x row, taps of the first half octet; first_live: None = by the mask (octet 0), else the
        number of the first live octet (straight-line variants)"""
        b.align()
        b.emit("weight", f"v_mov_b32_e64 v{m.w}, %[al]")
        for c in range(8):
            b.emit("xread", f"ds_read_b128 {quad(m.x + 4 * c)}, %[xrow] offset:{c * xr_stride * 16}")
        if first_live is None:
            b.emit("scalar", "s_bitcmp1_b32 %[mask], 0")
            b.emit("scalar", "s_cbranch_scc0 L_x_only_%=")
            load_taps(0)
            b.emit("label", "L_x_only_%=:")
        else:
            load_taps(2 * first_live)
        b.wait(0)
        for c in range(8):
            x_sums(b, m, c)

    def straight(lo, hi, tag):
        """octets lo .. hi - 1 live, known at assembly time: no mask tests, no branches"""
        b.emit("label", f"L_{tag}_%=:")
        prologue(lo)
        for i in range(lo, hi):
            b.wait(0)
            form()
            load_taps(2 * i + 1)
            fmas(2 * i)
            b.wait(0)
            form()
            if i + 1 < hi:
                load_taps(2 * i + 2)
            fmas(2 * i + 1)

    # ---- the masks of a 128-tap segment (0xff: rows 1-3, 0xf0: row 0, 0x0f: row 4) run straight-line code; any other
    # mask (shorter segments) takes the general block below.  A wave that has its SIMD to itself pays ~6 clocks for every
    # scalar instruction (profiles/r03_ubench_lone_wave.txt): the mask tests and branches were 9 % of a row step.
    variants = not o.nobranch and not o.generic
    if variants:
        for mask, tag in ((0xff, "ff"), (0xf0, "f0"), (0x0f, "0f")):
            b.emit("scalar", f"s_cmp_eq_u32 %[mask], {mask}")
            b.emit("scalar", f"s_cbranch_scc1 L_{tag}_%=")
    # ---- general block: octets by the mask (both halves of an octet are live or dead together); --nobranch: all of them
    # live, the scalar lines left out (their labels stay)
    prologue(None)
    for i in range(8):
        b.emit("scalar", f"s_bitcmp1_b32 %[mask], {i}")
        b.emit("scalar", f"s_cbranch_scc0 L_dead{i}_%=")
        b.wait(0)                                               # (its reads went out under the previous half's FMAs)
        form()
        load_taps(2 * i + 1)
        fmas(2 * i)
        b.wait(0)
        form()
        if i < 7:
            b.emit("scalar", f"s_bitcmp1_b32 %[mask], {i + 1}")
            b.emit("scalar", f"s_cbranch_scc0 L_last{i}_%=")
            load_taps(2 * i + 2)
            b.emit("label", f"L_last{i}_%=:")
            b.align()
        fmas(2 * i + 1)
        if o.nobranch:
            continue
        if i < 7:
            b.emit("scalar", f"s_branch L_end{i}_%=")
            b.emit("label", f"L_dead{i}_%=:")
            b.emit("scalar", f"s_bitcmp1_b32 %[mask], {i + 1}")
            b.emit("scalar", f"s_cbranch_scc0 L_end{i}_%=")
            load_taps(2 * i + 2)
            b.emit("label", f"L_end{i}_%=:")
        else:
            b.emit("label", f"L_dead{i}_%=:")
    if variants:
        for lo, hi, tag in ((0, 8, "ff"), (4, 8, "f0"), (0, 4, "0f")):
            b.emit("scalar", "s_branch L_done_%=")
            straight(lo, hi, tag)
        b.emit("label", "L_done_%=:")
    return b.done()


def unit_steps(lseg):
    """live octets [lo, hi) of the row steps rp = 0 .. halo of a segment of lseg taps (a multiple of 8): octet i of step rp
    holds taps 32 rp - 32 + 8 i .. + 7"""
    halo = (lseg + 31) >> 5
    return tuple((max(0, 4 - 4 * r), min(8, (lseg + 32 - 32 * r) >> 3)) for r in range(halo + 1))


# ---------------------------------------------------------------------------------------------------------------------------
# The whole (tile, source) unit of a 128-tap segment as ONE block (split-role kernel, bas_fused_split.hip: the filter waves
# have no staging state to keep, so the block may hold 126 operand registers).  Five row steps rp = 0..4 with the octets
# 4-7 | 0-7 | 0-7 | 0-7 | 0-3 live = 32 octets in a row, and what the per-step block cannot do:
#   * the x row of step r + 1 is read into the OTHER x buffer under the last octet of step r, its first taps likewise: no
#     exposed LDS latency at a step's start (5 x ~200 clocks per unit for a wave that has its SIMD to itself);
#   * taps are read one whole octet ahead into two half-octet buffers, so every wait is an lgkmcnt(N > 0) that is met;
#   * no mask tests, no branches, no per-step address arithmetic between the steps (tap address and weight of every step are
#     operands).
def unit3_block(xr_stride, lseg, o):
    steps = unit_steps(lseg)
    halo = len(steps) - 1
    m = UNIT3
    b = Block(m)

    def x_reads(r):
        xb = m.x + 32 * (r % 2)
        return [(f"x{r}", "xread", f"ds_read_b128 {quad(xb + 4 * c)}, %[xrow] offset:{(halo - r) * 16 + c * xr_stride * 16}")
                for c in range(8)]

    def tap_reads(r, i, h):
        return [(f"t{r}.{i}.{h}", "tapread", f"ds_read_b128 {quad(m.tap + 16 * h + 4 * j)}, %[tap{r}] offset:{(8 * i + 4 * h + j) * 16}")
                for j in range(4)]

    def fmas(xb, i, h, reads):
        """the FMAs of half octet (i, h); `reads` go out in front of them (--spread=0) or one by one between them"""
        lines = [text for text, _, _ in fir_fmas(m._replace(x=xb), i, h)]
        reads = list(reads)
        if not o.spread or not reads:
            for rd in reads:
                b.issue(*rd)
            for ln in lines:
                b.emit("fir", ln)
            return
        span = max(len(lines) * o.spread // 8, len(reads))     # FMAs the reads are dealt over
        at = {(k * span) // len(reads) for k in range(len(reads))}
        for n_, ln in enumerate(lines):
            if n_ in at and reads:
                b.issue(*reads.pop(0))
            b.emit("fir", ln)
        for rd in reads:
            b.issue(*rd)

    octets = [(r, i) for r, (lo, hi) in enumerate(steps) for i in range(lo, hi)]
    b.wait(0)                                                   # (scalar loads of the code around the block return out of order)
    for rd in x_reads(0) + tap_reads(*octets[0], 0) + tap_reads(*octets[0], 1):
        b.issue(*rd)
    for n, (r, i) in enumerate(octets):
        xb = m.x + 32 * (r % 2)
        nxt = octets[n + 1] if n + 1 < len(octets) else None
        if i == steps[r][0]:                                    # first octet of a step: its x row, the sums, the weight
            b.wait_for([f"x{r}"])
            for c in range(8):
                x_sums(b, m._replace(x=xb), c)
            b.emit("weight", f"v_mov_b32_e64 v{m.w}, %[al{r}]")
        last_of_step = i == steps[r][1] - 1
        for h in range(2):
            if not o.two_waits:
                # ONE wait per octet, in its middle: for the octet's second half (read a whole octet ago) and the NEXT octet's
                # first half (read half an octet ago, behind the forming of this octet's first half)
                if h == 1:
                    b.wait_for([f"t{r}.{i}.1"] + ([f"t{nxt[0]}.{nxt[1]}.0"] if nxt else []))
                elif n == 0:
                    b.wait_for([f"t{r}.{i}.0"])
            else:
                b.wait_for([f"t{r}.{i}.{h}"])
            form_taps(b, m.tap + 16 * h, m.g, pr(m.w), W_LOW)
            reads = []
            if h == 0 and last_of_step and r + 1 < len(steps):
                reads += x_reads(r + 1)                         # (in front of the next octet's taps: it is needed first)
            if nxt:
                reads += tap_reads(*nxt, h)
            fmas(xb, i, h, reads)
    return b.done()


# ---------------------------------------------------------------------------------------------------------------------------
# The unit block with a ROLLING x row (round 4): the 8 quads of an x row are not used evenly - octet i of a row step
# meets inputs q in [12 - 4 i, 31 - 4 i] - so quad c of the NEXT row is read into the same registers as soon as the last
# octet that needs quad c of this row has gone out (quads 7, 6 behind octet 4, .. quads 1, 0 behind octet 7), three octets
# before its first use.  One x buffer instead of two: 32 registers free for
#   * nsub = 2: subchunks of 16 samples - a row of 32 inputs then meets TWO crossfaded tap sets (inputs 0-15 with the
#     weight al, 16-31 with al + S / K; apply_hrtf.py:442-443), 12 more formed-tap registers; a half octet forms only the
#     sets its inputs fall into;
#   * nbuf = 3 or 4 half-octet tap buffers (reads one and a half or two octets ahead);
#   * psplit: P split once more (fir_fmas), 18 more accumulators.
# Same arithmetic and order of accumulation per accumulator as unit3_block (bit-identical output for nsub = 1).
def roll_block(xr_stride, lseg, nsub, nbuf, psplit, o):
    assert not (psplit and nsub != 1)
    steps = unit_steps(lseg)
    halo = len(steps) - 1
    m = roll_regs(nsub, nbuf, psplit)
    b = Block(m)
    halves = [(r, i, h) for r, (lo, hi) in enumerate(steps) for i in range(lo, hi) for h in range(2)]

    def plan_of(i, h):
        """(lines, quads read, tap sets used) of half octet (i, h)"""
        f = list(fir_fmas(m, i, h, nsub, psplit))
        return [text for text, _, _ in f], {c for _, c, _ in f}, {u for _, _, u in f}

    plan = [plan_of(i, h) for _, i, h in halves]
    first_use, last_use = {}, {}
    for n, ((r, i, h), (_, quads, _)) in enumerate(zip(halves, plan)):
        for c in quads:
            first_use.setdefault((r, c), n)
            last_use[(r, c)] = n

    def x_read(r, c):
        return (f"x{r}.{c}", "xread", f"ds_read_b128 {quad(m.x + 4 * c)}, %[xrow] offset:{(halo - r) * 16 + c * xr_stride * 16}")

    def tap_reads(n):
        r, i, h = halves[n]
        tb = m.tap + 16 * (n % nbuf)
        if o.taps_once_probe and psplit and r >= 1 and i < 4:  # (probe: this half forms whatever its buffer holds)
            b.landed.add(f"t{n}")
            return []
        return [(f"t{n}", "tapread", f"ds_read_b128 {quad(tb + 4 * j)}, %[tap{r}] offset:{(8 * i + 4 * h + j) * 16}") for j in range(4)]

    # x quads of step r + 1 go out right behind the half octet that uses quad c of step r for the last time
    x_after = {}                                                # half index n -> reads issued in front of the FMAs of half n
    for (r, c), n_first in sorted(first_use.items()):
        if r == 0:
            continue
        prev = [last_use[(rr, c)] for rr in range(r) if (rr, c) in last_use]
        x_after.setdefault((max(prev) + 1) if prev else 0, []).append(x_read(r, c))
    wait_points = list(range(len(halves))) if o.two_waits else [n for n, (r, i, h) in enumerate(halves) if n == 0 or h == 1]

    b.wait(0)                                                   # (scalar loads of the code around the block return out of order)
    for c in sorted(c for (r, c) in first_use if r == 0):
        b.issue(*x_read(0, c))
    for n in range(min(nbuf, len(halves))):
        for rd in tap_reads(n):
            b.issue(*rd)
    xs_done = set()

    def needs(k):
        rk = halves[k][0]
        return [f"t{k}"] + [f"x{rk}.{c}" for c in sorted(plan[k][1]) if first_use[(rk, c)] == k]

    def sums_of(k):
        """x_e + x_o of the quads half k is the first to use, once they have landed"""
        rk = halves[k][0]
        for c in sorted(plan[k][1]):
            if first_use[(rk, c)] == k and f"x{rk}.{c}" in b.landed and (rk, c) not in xs_done:
                xs_done.add((rk, c))
                x_sums(b, m, c, psplit)

    for n, ((r, i, h), (lines, quads, sets)) in enumerate(zip(halves, plan)):
        nxt = min([k for k in wait_points if k > n], default=len(halves))
        if n in wait_points:                                    # what the halves up to the next wait point need, as far as it is on its way
            b.wait_for([t for k in range(n, nxt) for t in needs(k) if t in b.queue])
        missing = [t for t in needs(n) if t not in b.landed]
        if missing:                                             # (read too late for the wait point in front: a wait of its own)
            assert all(t in b.queue for t in missing), (n, missing)
            b.wait_for(missing)
        for k in range(n, nxt if n in wait_points else n + 1):
            sums_of(k)
        assert all(f"x{r}.{c}" in b.landed and (r, c) in xs_done for c in quads), (n, quads)
        if (i, h) == (steps[r][0], 0):                          # first half octet of a step: its weights
            b.emit("weight", f"v_mov_b32_e64 v{m.w}, %[al{r}]")
            if nsub == 2:
                b.emit("weight", f"v_mov_b32_e64 v{m.w + 1}, %[bl{r}]")
            if nsub == 4:                                       # al + u S / K for the row's subchunks u = 1, 2, 3
                b.emit("weight", f"v_add_f32_e64 v{m.w + 1}, v{m.w}, %[dl]")
                b.emit("weight", f"v_fma_f32 v{m.w + 2}, 2.0, %[dl], v{m.w}")
                b.emit("weight", f"v_add_f32_e64 v{m.w + 3}, v{m.w + 2}, %[dl]")
        for u in sorted(sets):                                  # (P split: one set, and the sum of its sums)
            form_taps(b, m.tap + 16 * (n % nbuf), m.g + 12 * u, pr(m.w + 2 * (u >> 1)), W_HIGH if u % 2 else W_LOW,
                      m.gss if psplit else None)
        if n == 0:
            for rd in x_after.get(0, []):
                b.issue(*rd)
        for rd in tap_reads(n + nbuf) if n + nbuf < len(halves) else []:
            b.issue(*rd)
        for ln in lines:
            b.emit("fir", ln)
        for rd in x_after.get(n + 1, []):                       # (quads whose last use is THIS half: behind its FMAs = in front of the next)
            b.issue(*rd)
    return b.done()


# ---------------------------------------------------------------------------------------------------------------------------
# The P-split unit block with every tap read ONCE (ffa_unitp1_asm, bas_fir_once_asm.inc).  Tap T in [32 b, 32 b + 31] of a
# segment is met twice by a lane: in octets 4-7 of row step b (x row R - b, the NEWER one) and in octets 0-3 of step b + 1
# (x row R - b - 1, the OLDER one).  roll_block reads and forms it in both places.  Both reads fetch the same record
# (h0, d) while the two rows lie in one chunk; where the pair crosses a chunk boundary the newer row opens chunk c with
# weight 0 and h0_c = h0_{c-1} + d_{c-1}: the older row's record at weight K / K.  So the block walks MERGED half octets
# (b, i, h), b = 0 .. halo - 1, i = 0 .. 3: one read of four taps at the older row's slot (operand tap{b+1}: the tap row of
# step b + 1), two formed sets - N with the weight wn{b} (the newer row's own, or 1.0 in a lane whose pair crosses), O with
# wo{b} (the older row's own) - and the FMAs of (step b, octet 4 + i, h) on N and of (step b + 1, octet i, h) on O.
#   * The rolling x row holds both rows at once: merged half m = 2 i + h of a group uses quads 0 .. 7 - m of the newer row
#     and 7 - m .. 7 of the older.  Quad c = 7 - m is the only one both need: the newer row's FMAs on it go first (right
#     behind the forming of N), the older row's quad c is read into the same registers behind them, the other ~77 FMAs of
#     the half run under that read, and the older row's five FMAs on quad c close the half.  No second x buffer, 8 x-quad
#     reads per group as before.
#   * ONE half-octet tap buffer: it is free once both sets are formed, the next half's reads go out right there - in one
#     burst with the x quad - and land under ~77 FMAs.  One wait per half covers all five.
# Registers: accumulators v[0:115] as roll_block(psplit), x 32 + sums 16 + 8, taps 16, formed 2 x (12 + 2), weights 2:
# v[116:217].  Same FMAs per accumulator as ffa_unitp_asm; their order inside an accumulator interleaves the two steps.
def once_halves(lseg):
    """merged half octets (b, i, h) of a segment of lseg taps; both partners of a merged octet hold the same taps, so they
    are live or dead together, and together they are all the live octets of the unit"""
    steps = unit_steps(lseg)
    out = []
    for b in range(len(steps) - 1):
        for i in range(4):
            newer, older = steps[b][0] <= 4 + i < steps[b][1], steps[b + 1][0] <= i < steps[b + 1][1]
            assert newer == older
            if newer:
                out += [(b, i, 0), (b, i, 1)]
    assert len(out) == sum(hi - lo for lo, hi in steps)        # (two half octets per merged octet = one per live octet)
    assert steps[0][0] >= 4 and steps[-1][1] <= 4              # nothing in front of the first group or behind the last
    return out


def once_block(xr_stride, lseg, o):
    halo = len(unit_steps(lseg)) - 1
    halves = once_halves(lseg)
    m = ONCE_N
    blk = Block(m)

    def fma_list(i, h, regs):
        """[(line, x quad it reads)] of half octet (i, h) of a row step on the formed set of `regs`"""
        return [(text, c) for text, c, _ in fir_fmas(regs, i, h, 1, True)]

    def x_read(r, c):
        return (f"x{r}.{c}", "xread", f"ds_read_b128 {quad(m.x + 4 * c)}, %[xrow] offset:{(halo - r) * 16 + c * xr_stride * 16}")

    def tap_reads(n):
        b, i, h = halves[n]
        return [(f"t{n}", "tapread", f"ds_read_b128 {quad(m.tap + 4 * j)}, %[tap{b + 1}] offset:{(8 * i + 4 * h + j) * 16}") for j in range(4)]

    row_in = {}                                                 # x quad -> the row step whose row it holds (sums formed)

    def lines_on(lst, r):
        for ln, c in lst:
            assert row_in.get(c) == r, (ln, c, r, row_in)       # the quad holds this step's row, landed and summed
            blk.emit("fir", ln)

    blk.wait(0)                                                 # (scalar loads of the code around the block return out of order)
    first = sorted({c for b, i, h in halves if b == 0 for _, c in fma_list(4 + i, h, ONCE_N)})
    for c in first:
        blk.issue(*x_read(0, c))
    for rd in tap_reads(0):
        blk.issue(*rd)
    blk.wait_for([f"x0.{c}" for c in first] + ["t0"])
    for c in first:
        x_sums(blk, m, c, True)
        row_in[c] = 0
    for n, (b, i, h) in enumerate(halves):
        newer, older = fma_list(4 + i, h, ONCE_N), fma_list(i, h, ONCE_O)
        both = {c for _, c in newer} & {c for _, c in older}
        assert len(both) == 1, both                             # the one quad the two rows share in this half
        cx = both.pop()
        assert f"t{n}" in blk.landed
        if n == 0 or halves[n - 1][0] != b:                    # first half of a group: its two weights, (newer, older)
            blk.emit("weight", f"v_mov_b32_e64 v{m.w}, %[wn{b}]")
            blk.emit("weight", f"v_mov_b32_e64 v{m.w + 1}, %[wo{b}]")
        form_taps(blk, m.tap, ONCE_N.g, pr(m.w), W_LOW, ONCE_N.gss)
        lines_on([(ln, c) for ln, c in newer if c == cx], b)
        form_taps(blk, m.tap, ONCE_O.g, pr(m.w), W_HIGH, ONCE_O.gss)
        # ONE burst of reads per half (reads behind each other pipeline, a lone read between FMAs costs the next FMA its slot:
        # DESIGN.md 4.0): the next half's taps - the tap buffer is free, both sets are formed - and the older row's quad cx,
        # behind the newer row's last use of it
        if n + 1 < len(halves):
            for rd in tap_reads(n + 1):
                blk.issue(*rd)
        blk.issue(*x_read(b + 1, cx))
        del row_in[cx]
        lines_on([(ln, c) for ln, c in newer if c != cx], b)
        lines_on([(ln, c) for ln, c in older if c != cx], b + 1)
        blk.wait_for([f"t{n + 1}", f"x{b + 1}.{cx}"])
        assert f"x{b + 1}.{cx}" in blk.landed
        x_sums(blk, m, cx, True)
        row_in[cx] = b + 1
        lines_on([(ln, c) for ln, c in older if c == cx], b + 1)
    return blk.done()


# ---- the instruction lists of the unit blocks, as tests and tools import them (no options: the default schedule)
def gen_unit(xr_stride, lseg, o=None):
    return unit3_block(xr_stride, lseg, o or DEFAULT).lines(o or DEFAULT)


def gen_unit_roll(xr_stride, lseg, nsub=1, nbuf=2, psplit=False, o=None):
    blk = roll_block(xr_stride, lseg, nsub, nbuf, psplit, o or DEFAULT)
    return blk.lines(o or DEFAULT), blk.regs.last


def gen_unit_once(xr_stride, lseg, o=None):
    blk = once_block(xr_stride, lseg, o or DEFAULT)
    return blk.lines(o or DEFAULT), blk.regs.last


# ---------------------------------------------------------------------------------------------------------------------------
# The C++ around a block.  head: what the file holds in front of the wrapper's first function; decl_params: the parameters
# as the primary template declares them where their line breaks differ from `params` - behind the head, or (decl_each) in
# front of every specialisation, behind `pre`.
Wrapper = namedtuple("Wrapper", "name tparams head comment pre decl_each decl_params params acc ops clobbers")


def operands(label, array, n, first=0):
    return ", ".join(f'[{label}{first + k}] "v"({array}[{k}])' for k in range(n))


ACC_P = '"+{v[0:31]}"(accA), "+{v[32:63]}"(accB), "+{v[64:95]}"(accP), "+{v[96:97]}"(accB16)'
ACC_PSPLIT = ('"+{v[0:31]}"(accA), "+{v[32:63]}"(accB), "+{v[64:79]}"(accPA), "+{v[80:95]}"(accPB), "+{v[96:97]}"(accPB8),\n'
              '          "+{v[98:113]}"(accPP), "+{v[114:115]}"(accB16)')
OPS_UNIT = ['[xrow] "v"(xrow4), ' + operands("tap", "tap", 5), operands("al", "al", 5)]
F32X16 = "typedef float f32x16 __attribute__((ext_vector_type(16)));\n"

ROW_STEP = Wrapper(
    name="ffa_row_step_asm", tparams="int XR",
    head="""// GENERATED by tools/gen_fir_asm.py {xrs} - do not edit (see that file for the register map and the schedule).
// Row step of the fused FIR kernel as one gfx950 assembly block: {n_fma} v_pk_fma_f32 (784 FIR + 64 forming), 32 v_pk_add_f32,
// 16 v_add_f32, 72 ds_read_b128; reads of half octet u + 1 issued right behind the forming of half u, under its FMAs; every
// 64-bit instruction 8-byte aligned.  Same arithmetic and accumulation order as ffa_row_step_x (bas_fir.h).
// One instantiation per column stride XR of the x image (float4 units).
#pragma once
typedef float f32x32 __attribute__((ext_vector_type(32)));

""",
    comment="", pre="", decl_each=False,
    decl_params=None,
    params="""f32x32 &accA, f32x32 &accB, f32x2 &accB16, f32x32 &accP, unsigned xrow,
                                                  unsigned tap, float al, unsigned mask""",
    acc=ACC_P, ops=['[xrow] "v"(xrow), [tap] "v"(tap), [al] "v"(al), [mask] "s"(mask)'], clobbers='"memory", "scc"')

UNIT = Wrapper(
    name="ffa_unit_asm", tparams="int XR, int LSEG", head="\n",
    comment="""// One (tile, source) unit of a {lseg}-tap segment in one block (see tools/gen_fir_asm.py: gen_unit): {n_fma} v_pk_fma_f32,
// {n_ds} ds_read_b128, {n_wait} waits.  xrow4 = LDS address of the lane's x row of step 4 (the lowest: step r reads 16 (4 - r)
// bytes above); tap[r], al[r] = tap row address and crossfade weight of step r.
""",
    pre="", decl_each=False,
    decl_params=None,
    params="""f32x32 &accA, f32x32 &accB, f32x2 &accB16, f32x32 &accP, unsigned xrow4,
                                              const unsigned (&tap)[5], const float (&al)[5]""",
    acc=ACC_P, ops=OPS_UNIT, clobbers='"memory"')

UNITP = Wrapper(
    name="ffa_unitp_asm", tparams="int XR, int LSEG", head="",
    comment="""// The same unit with the half-rate product P split once more (gen_unit_roll: psplit): {n_fma} v_pk_fma_f32, {n_ds} ds_read_b128,
// {n_wait} waits.  116 accumulator registers: A, B as before, PA v[64:79], PB v[80:97] (entries r = -1 .. 7), PP v[98:113],
// B entry 16 v[114:115]; the flush combines P[2r] = PA[r] + PB[r-1], P[2r+1] = PP[r] - PA[r] - PB[r] first.
""",
    pre=F32X16, decl_each=True,
    decl_params="""f32x32 &accA, f32x32 &accB, f32x16 &accPA, f32x16 &accPB, f32x2 &accPB8, f32x16 &accPP,
                                               f32x2 &accB16, unsigned xrow4, const unsigned (&tap)[5], const float (&al)[5]""",
    params="""f32x32 &accA, f32x32 &accB, f32x16 &accPA, f32x16 &accPB, f32x2 &accPB8,
                                               f32x16 &accPP, f32x2 &accB16, unsigned xrow4, const unsigned (&tap)[5],
                                               const float (&al)[5]""",
    acc=ACC_PSPLIT, ops=OPS_UNIT, clobbers='"memory"')

UNIT2 = Wrapper(
    name="ffa_unit2_asm", tparams="int XR, int LSEG", head="",
    comment="""// The same unit for subchunks of 16 samples (apply_hrtf.py:401-402 accepts any divisor of the chunk; :442-443): inputs 0-15 of
// a row are crossfaded with al[r], inputs 16-31 with bl[r] - two formed tap sets, each formed only by the half octets whose
// inputs fall into it: {n_fma} v_pk_fma_f32, {n_ds} ds_read_b128, {n_wait} waits.
""",
    pre="", decl_each=True,
    decl_params=None,
    params="""f32x32 &accA, f32x32 &accB, f32x2 &accB16, f32x32 &accP, unsigned xrow4,
                                               const unsigned (&tap)[5], const float (&al)[5], const float (&bl)[5]""",
    acc=ACC_P, ops=[OPS_UNIT[0], OPS_UNIT[1], operands("bl", "bl", 5)], clobbers='"memory"')

UNIT4 = Wrapper(
    name="ffa_unit4_asm", tparams="int XR, int LSEG", head="",
    comment="""// The same unit for subchunks of 8 samples: four formed tap sets per row, each formed only by the half octets whose inputs
// fall into it; the weights of a row's subchunks are al[r] + u dl, dl = S / K (two tap buffers: the registers go to the
// formed sets): {n_fma} v_pk_fma_f32, {n_ds} ds_read_b128, {n_wait} waits.
""",
    pre="", decl_each=True,
    decl_params=None,
    params="""f32x32 &accA, f32x32 &accB, f32x2 &accB16, f32x32 &accP, unsigned xrow4,
                                               const unsigned (&tap)[5], const float (&al)[5], float dl""",
    acc=ACC_P, ops=[OPS_UNIT[0], OPS_UNIT[1] + ', [dl] "v"(dl)'], clobbers='"memory"')

UNITP1 = Wrapper(
    name="ffa_unitp1_asm", tparams="int XR, int LSEG",
    head="""// GENERATED by tools/gen_fir_asm.py - do not edit (see that file: gen_unit_once).
// The split-role kernel's unit block with every tap read once and formed for both x rows that meet it.
#pragma once
""" + F32X16,
    comment="""// One (tile, source) unit of a {lseg}-tap segment, P split as in ffa_unitp_asm, taps read once: {n_fma} v_pk_fma_f32, {n_ds} ds_read_b128
// ({n_tap} of them taps), {n_wait} waits.  Merged group b = octets 4-7 of row step b and octets 0-3 of step b + 1: tapo[b] = tap row
// address of step b + 1 (the older row's slot), wn[b] = weight of step b (1.0 where the two rows lie in different chunks),
// wo[b] = weight of step b + 1.  xrow4 as in ffa_unit_asm.
""",
    pre="", decl_each=False,
    decl_params="""f32x32 &accA, f32x32 &accB, f32x16 &accPA, f32x16 &accPB, f32x2 &accPB8, f32x16 &accPP,
                                                f32x2 &accB16, unsigned xrow4, const unsigned (&tapo)[4], const float (&wn)[4],
                                                const float (&wo)[4]""",
    params="""f32x32 &accA, f32x32 &accB, f32x16 &accPA, f32x16 &accPB, f32x2 &accPB8,
                                                f32x16 &accPP, f32x2 &accB16, unsigned xrow4, const unsigned (&tapo)[4],
                                                const float (&wn)[4], const float (&wo)[4]""",
    acc=ACC_PSPLIT, ops=['[xrow] "v"(xrow4), ' + operands("tap", "tapo", 4, 1), operands("wn", "wn", 4), operands("wo", "wo", 4)],
    clobbers='"memory"')


def render(w, targs, blk, o, first, xrs):
    """the specialisation of wrapper w for the template arguments targs around block blk, with what stands in front of it"""
    rows = blk.filtered(o)
    count = lambda *kinds: sum(1 for kind, _ in rows if kind in kinds)  # noqa: E731
    stats = dict(lseg=targs[-1], n_fma=count("fir", "form"), n_ds=count("tapread", "xread"), n_tap=count("tapread"), n_wait=count("wait"),
                 xrs=" ".join(str(x) for x in xrs))
    decl = f"template <{w.tparams}>\n__device__ __forceinline__ void {w.name}({w.decl_params or w.params});\n"
    body = "\n".join(f'        "{text}\\n\\t"' for _, text in rows)
    clob = ", ".join(f'"v{r}"' for r in range(blk.regs.x, blk.regs.last + 1))
    return ((w.head.format(**stats) + ("" if w.decl_each else decl) if first else "")
            + "\n" + w.comment.format(**stats) + (w.pre + decl if w.decl_each else "")
            + f"template <>\n__device__ __forceinline__ void {w.name}<{', '.join(str(t) for t in targs)}>({w.params}) {{\n"
            + "    asm volatile(\n" + body + "\n"
            + f"        : {w.acc}\n        : " + ",\n          ".join(w.ops) + f"\n        : {w.clobbers}, {clob});\n}}\n")


def block_table(o):
    """what is emitted, in file order: (wrapper, template arguments, block), one row per function"""
    rows = [(ROW_STEP, (xr,), row_step_block(xr, o)) for xr in o.xrs]
    if 261 in o.xrs and not o.generic:
        for w, build in ((UNIT, lambda ls: roll_block(261, ls, 1, o.roll, False, o) if o.roll else unit3_block(261, ls, o)),
                         (UNITP, lambda ls: roll_block(261, ls, 1, PSPLIT_NBUF, True, o)),     # fast-FIR level 1.5
                         (UNIT2, lambda ls: roll_block(261, ls, 2, o.roll or 3, False, o)),    # subchunks of 16: two tap sets per row
                         (UNIT4, lambda ls: roll_block(261, ls, 4, 2, False, o)),              # subchunks of 8: four tap sets per row
                         (UNITP1, lambda ls: once_block(261, ls, o))):                         # the second file
            rows += [(w, (261, lseg), build(lseg)) for lseg in U_LSEGS]
    return rows


def once_path(out):
    """the second generated file lies beside the first: bas_fir_asm.inc -> bas_fir_once_asm.inc, ab_NAME.inc -> ab_NAME_once.inc"""
    d, f = os.path.split(out)
    return os.path.join(d, "bas_fir_once_asm.inc" if f == "bas_fir_asm.inc" else f[:-4] + "_once.inc")


def main(argv=None):
    o = parse_args(sys.argv[1:] if argv is None else argv)
    if o.spread and o.roll:
        print("gen_fir_asm.py: --spread exists only in round 3's schedule of the unit block: give --roll=0 with it", file=sys.stderr)
        sys.exit(2)
    table = block_table(o)
    text = {False: "", True: ""}                                # the first file, and the second: the block that reads every tap once
    for n, (w, targs, blk) in enumerate(table):
        text[w is UNITP1] += render(w, targs, blk, o, n == 0 or table[n - 1][0] is not w, o.xrs)
    files = [(o.out, text[False])] + ([(once_path(o.out), text[True])] if text[True] else [])
    if o.check:                                                 # compare with the committed file instead of writing it
        ok = True
        for path, body in files:
            # (the second file is a build product - the Makefile writes it, git does not track it: checked where it exists)
            built = os.path.exists(path)
            same = built and open(path).read() == body
            ok = ok and (same or (not built and path != o.out))
            print(f"{path}: {'up to date' if same else 'DIFFERS from what the generator writes' if built or path == o.out else 'not built yet'}")
        sys.exit(0 if ok else 1)
    for path, body in files:
        if not (os.path.exists(path) and open(path).read() == body):    # (a file that is right stays untouched)
            with open(path, "w") as f:
                f.write(body)
    rows = table[len(o.xrs) - 1][2].filtered(o)
    print(f"{o.out}: {len(rows)} lines per variant, {sum(1 for kind, _ in rows if kind in ('fir', 'form'))} packed FMAs")


if __name__ == "__main__":
    main()
