"""The local error bound of DESIGN.md §3.23 on the CPU: the checker (oracle/whole.local_scale, compare_local), the staircase
scenes and their input conditions, the float32 reference arithmetic (where r_ref of the GPU tests comes from), the
2-parallel fast FIR against the direct form, and four defects that today's `rel_err <= 1e-5` cannot see and the local
bound must.  No GPU and no code under test: this module proves that the checker has teeth."""
import numpy as np
import pytest

from conftest import rel_err
from oracle import bas_oracle as orc
from oracle import whole
import local_error_support as les
from local_error_support import FIR_CASES, QUIET, SHARP, U32, W

REL = 1e-5                                    # today's parity bound


# ---- the helpers ----------------------------------------------------------------------------------------------------
def test_widen_and_frame_max():
    a = np.array([[0.0, 1.0, 0.0, 0.0, 0.0, 3.0, 0.0]])
    assert whole.widen_max(a, 1).tolist() == [[1.0, 1.0, 1.0, 0.0, 3.0, 3.0, 3.0]]
    assert np.array_equal(whole.widen_max(a, 0), a)
    f = whole.frame_max(np.array([0.0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0]), 2)       # frames of 2: the 5 lies in frame 2
    assert f.tolist() == [0.0, 0, 5, 5, 5, 5, 5, 5, 0, 0, 0]


def test_compare_local_takes_the_cast_off_and_finds_the_worst_sample():
    want = np.array([[1.0 + 2.0 ** -30, 2.0 ** -40, 0.0, 3.0], [1.0, 1.0, 0.0, 1.0]])
    scale = np.array([[4.0, 2.0 ** -38, 0.0, 4.0], [4.0, 4.0, 0.0, 4.0]])
    got = want.astype(np.float32).astype(np.float64)
    res = whole.compare_local(got, want, scale, K=2)
    assert res["ratio"] == 0.0 and res["zeros_ok"] and res["zeros"] == 2          # the cast alone costs nothing
    got[0, 1] += 2.0 ** -60                                                      # 4 units of 2^-24 scale
    res = whole.compare_local(got, want, scale, K=2)
    assert (res["ear"], res["n"], res["chunk"], res["n_mod_K"]) == (0, 1, 0, 1) and 3.7 < res["ratio"] <= 4.0
    got[1, 2] = -0.0
    assert whole.compare_local(got, want, scale)["zeros_ok"]
    got[1, 2] = 1e-30
    assert not whole.compare_local(got, want, scale)["zeros_ok"]
    got[1, 0] = np.nan
    res = whole.compare_local(got, want, scale)
    assert res["ratio"] == np.inf and not res["finite"]


def test_local_scale_bounds_every_term():
    """A >= sum |g[k]| |x[n - k]| (equal up to rounding here: one source), and A_W is its running maximum."""
    K, S, L, n = 64, 16, 20, 256
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1, n))
    irs = rng.standard_normal((n // K + 1, 2, L))
    A = whole.local_scale(x, K, S, lambda i: irs, W=0)
    want = orc.render_mix_f64(np.abs(x), K, S, [np.abs(irs)])
    assert A.shape == want.shape and np.allclose(A, want, rtol=1e-12, atol=0)
    y = whole.render_mix_whole(x, K, S, lambda i: irs)
    assert (np.abs(y) <= A * (1 + 1e-12)).all()
    assert np.array_equal(whole.local_scale(x, K, S, lambda i: irs, W=5), whole.widen_max(A, 5))


# ---- the staircase and the scenes -----------------------------------------------------------------------------------
def test_staircase_is_exact_and_scales_exactly():
    x = les.staircase(5, 3000, (0, -34, -20), 641)
    base = les.bas.synth.integer_noise(5, 3000).astype(np.float64)
    lev = np.array([0, -34, -20])[(np.arange(3000) // 641) % 3]
    assert x.dtype == np.float32 and np.array_equal(x.astype(np.float64), base * 2.0 ** lev)
    for k in (-40, 40):
        assert np.array_equal((x * np.float32(2.0 ** k)).astype(np.float64), x.astype(np.float64) * 2.0 ** k)


@pytest.mark.parametrize("name", sorted(FIR_CASES))
def test_scene_conditions_and_the_reference_arithmetic(name):
    """Every GPU case's exact scene: the input conditions of the issue, and the float32 direct form (r_ref) within the
    derived backstop."""
    case, how = FIR_CASES[name]
    sc, want, scale, ref = les.reference(case)
    n_src, n, K, S, L = case
    assert sc.run >= 4 * (L + W) and les.boundaries_ok(sc.run, n, K, S)
    n_runs = -(-n // sc.run)
    lev = np.array([les.levels_of_source(i, n_runs) for i in range(max(n_src - 1, 1))])
    assert (lev == QUIET).all(axis=0).sum() >= 2                                  # runs with every source quiet
    assert lev.max() - lev.min() >= 34 and (np.diff(lev[0]) > 0).any() and (np.diff(lev[0]) < 0).any()
    if n_src > 1:
        assert not sc.x[-1].any() and len({tuple(v) for v in lev}) == min(len(lev), len(les.CYCLE))   # a silent source; staggered runs
    quiet, zero = les.input_conditions(sc, scale)
    assert quiet >= 0.25, quiet
    # The zero padding behind the signal (n .. in_length) is the render's own: counted among the reachable outputs only
    assert zero <= 0.01, zero
    assert ref["zeros_ok"] and ref["finite"]
    print(f"{name}: r_ref {ref['ratio']:.3g}, c_wc {sc.c_wc}, quiet share {quiet:.2f}; {whole.describe_local(ref)}")
    assert 0 < ref["ratio"] <= sc.c_wc, whole.describe_local(ref)


# ---- the 2-parallel fast FIR of DESIGN.md §3.2 in float32 -----------------------------------------------------------
def _fma(acc, a, b):
    """float32 fused multiply-add (the product of two float32 is exact in float64)."""
    return np.float32(np.float64(a) * np.float64(b) + np.float64(acc))


def _direct_rows(x, g, n_rows):
    L = g.size
    y = np.zeros(32 * n_rows, dtype=np.float32)
    for n in range(y.size):
        for m in range(max(n - L + 1, 0), n + 1):                                # input rows ascend, as the row steps do
            y[n] = _fma(y[n], g[n - m], x[m])
    return y


def _fast_rows(x, g, n_rows):
    """A = g_e * x_e, B = g_o * x_o, P = (g_e + g_o) * (x_e + x_o) per 32 x 32 Toeplitz block, accumulated over the input
    rows of an output row; y[2p] = A[p] + B[p - 1], y[2p + 1] = P[p] - A[p] - B[p] at the flush."""
    L = g.size
    tap = lambda t: g[t] if 0 <= t < L else np.float32(0)                         # noqa: E731
    y = np.zeros(32 * n_rows, dtype=np.float32)
    for r in range(n_rows):
        A, B, P = np.zeros(16, np.float32), np.zeros(17, np.float32), np.zeros(16, np.float32)   # B[j] holds p = j - 1
        for r_in in range(max(r - (L + 30) // 32, 0), r + 1):
            D = 32 * (r - r_in)
            xr = x[32 * r_in:32 * r_in + 32]
            xe, xo = xr[0::2], xr[1::2]
            xs = xe + xo
            for p in range(-1, 16):
                for q in range(16):
                    ge, go = tap(D + 2 * (p - q)), tap(D + 2 * (p - q) + 1)
                    B[p + 1] = _fma(B[p + 1], go, xo[q])
                    if p >= 0:
                        A[p] = _fma(A[p], ge, xe[q])
                        P[p] = _fma(P[p], np.float32(ge + go), xs[q])
        y[32 * r:32 * r + 32:2] = A + B[:16]
        y[32 * r + 1:32 * r + 32:2] = (P - A) - B[1:]
    return y


@pytest.mark.parametrize("L", [8, 128])
def test_fast_fir_block_is_local(L):
    """A staircase block: the first half of input row 0 loud, its second half and the next rows at 2^-30.  The fast form
    stays within 8 x the direct form's ratio against the same local scale (W = 32), and within the backstop.  A numpy
    float32 transcription of the A / B / P formulas of DESIGN.md §3.2: tools/emulate_fir_asm.py executes the generated
    block in float64, where neither form rounds."""
    n_rows = 8
    rng = np.random.default_rng(L)
    x = les.bas.synth.integer_noise(11, 32 * n_rows).astype(np.float32)
    x[16:] *= np.float32(2.0 ** -30)
    g = (rng.standard_normal(L) * 2.0 ** (-np.arange(L) / 16.0)).astype(np.float32)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    want = np.convolve(x64, g64)[:x.size]
    scale = whole.widen_max(np.convolve(np.abs(x64), np.abs(g64))[:x.size], W)
    assert (scale <= 2.0 ** -25 * scale.max()).mean() >= (0.25 if L == 128 else 0.5)
    direct = whole.compare_local(_direct_rows(x, g, n_rows), want, scale)
    fast = whole.compare_local(_fast_rows(x, g, n_rows), want, scale)
    print(f"L {L}: direct {direct['ratio']:.3g}, fast {fast['ratio']:.3g} at n={fast['n']}")
    assert 0 < direct["ratio"] <= L + 4
    assert fast["ratio"] <= SHARP * direct["ratio"] and fast["ratio"] <= 4 * (-(-L // 8) * 8) + 64
    assert rel_err(_fast_rows(x, g, n_rows), want) <= REL


# ---- sensitivity: four defects the norm-relative bound passes -------------------------------------------------------
SENS = (3, 6000, 512, 32, 128)


def _sens():
    sc, want, scale, ref = les.reference(SENS, quiet=-70)
    clean = want.astype(np.float32).astype(np.float64)
    r = 3                                                                          # a run with every source at 2^-70
    lo, hi = r * sc.run + sc.L + W, (r + 1) * sc.run - W                           # its outputs of quiet widened support
    assert les.levels_of_source(0, 8, -70)[r] == -70 and hi - lo > 200
    assert (scale[:, lo:hi] <= 2.0 ** -60 * scale.max()).all()
    return sc, want, scale, clean, lo, hi


def _passes_today_fails_locally(got, want, scale, sc):
    assert rel_err(got, want) <= REL, rel_err(got, want)
    res = whole.compare_local(got, want, scale, sc.K)
    assert res["ratio"] > sc.c_wc, whole.describe_local(res)
    return res


def test_the_clean_cast_passes():
    sc, want, scale, clean, lo, hi = _sens()
    res = whole.compare_local(clean, want, scale, sc.K)
    assert res["ratio"] == 0.0 and res["zeros_ok"]


def test_defect_one_loud_ulp_in_a_quiet_run():
    sc, want, scale, got, lo, hi = _sens()
    got[1, lo + 50] += U32 * np.abs(want).max()
    res = _passes_today_fails_locally(got, want, scale, sc)
    assert (res["ear"], res["n"]) == (1, lo + 50)


def test_defect_a_loud_run_leaks_into_a_quiet_one():
    """1e-6 of the loud run before, added 100 samples past L + W into the quiet run."""
    sc, want, scale, got, lo, hi = _sens()
    n = np.arange(lo + 100, hi)
    got[:, n] += 1e-6 * want[:, n - (sc.L + W + 100) - 300]
    assert np.abs(want[:, n - (sc.L + W + 100) - 300]).max() > 2.0 ** -30 * np.abs(want).max()
    res = _passes_today_fails_locally(got, want, scale, sc)
    assert lo + 100 <= res["n"] < hi


def test_defect_small_values_flushed_to_zero():
    sc, want, scale, got, lo, hi = _sens()
    run = got[:, lo:hi]
    eaten = np.abs(run) < 2.0 ** -60
    assert eaten.mean() > 0.9 and (run != 0).mean() > 0.9
    run[eaten] = 0.0
    res = _passes_today_fails_locally(got, want, scale, sc)
    assert lo <= res["n"] < hi


def test_defect_a_quiet_run_rendered_with_the_neighbour_chunks_ir():
    """Source 0's samples of the quiet run alone go through the chunk IRs one chunk late; everything else is right."""
    sc, want, scale, clean, lo, hi = _sens()
    run = np.zeros((1, sc.in_length), dtype=np.float32)
    run[0, 3 * sc.run:4 * sc.run] = sc.x[0, 3 * sc.run:4 * sc.run]
    irs = np.asarray(sc.irs_of()(0))
    late = np.concatenate([irs[1:], irs[-1:]])
    acc = want - whole.render_mix_whole(run, sc.K, sc.S, lambda i: irs) + whole.render_mix_whole(run, sc.K, sc.S, lambda i: late)
    got = acc.astype(np.float32).astype(np.float64)
    assert not np.array_equal(got, clean)
    res = _passes_today_fails_locally(got, want, scale, sc)
    assert 3 * sc.run <= res["n"] < 4 * sc.run + sc.L


# ---- the late tail and the row stages: the reference arithmetic within the backstops --------------------------------
@pytest.mark.parametrize("Np,Lr,lag", les.LATE_CASES)
def test_late_tail_reference_arithmetic(Np, Lr, lag):
    """scipy.fft on complex64 computes in single precision (the function asserts its dtypes); its ratio on the frame-grid
    scale is r_ref of the GPU case, within the backstop; the staircase bus has its quiet passages after widening."""
    bus, h, n_out, want, A = les.long_fir_reference(Lr, lag)
    scale = whole.frame_max(A, Np)
    got = les.long_fir_f32_fft(bus, h, lag, n_out, Np)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert rel_err(got, want) <= REL
    ref = whole.compare_local(got, want, scale)
    assert (scale <= 2.0 ** -30 * scale.max()).mean() >= 0.25 and (scale == 0).mean() <= 0.01
    print(f"long_fir Np={Np} Lr={Lr} lag={lag}: r_ref {ref['ratio']:.3g} of {les.long_fir_backstop(Np)}")
    assert ref["zeros_ok"] and 0 < ref["ratio"] <= les.long_fir_backstop(Np), whole.describe_local(ref)


def test_row_stage_reference_arithmetic():
    """The float32 restatements of the row stages against their float64 definitions: within taps + 4 of the W = 0 scale,
    with weights that step by 2^-20 between chunk boundaries."""
    from binaural_audio_synthesis_amd import propagation, reverb
    T, K, run = 6000, 512, 211
    x = les.stage_rows(3, T, run, 6200)
    nq = (T - 1) // K + 2
    send = np.stack([les.step_levels(nq, 40 + s) * (0.3 + 0.2 * s) * (-1.0) ** s for s in range(3)])
    assert {-20.0, 20.0} <= set(np.log2(send[0, 1:] / send[0, :-1]))                         # steps both ways
    want = reverb.bus_mix(x, send, K)[:T]
    scale = reverb.bus_mix(np.abs(x), np.abs(send), K)[:T]
    assert (np.abs(want) <= scale * (1 + 1e-12)).all()
    res = whole.compare_local(les.bus_mix_f32(x, send, K), want, scale, K)
    assert 0 < res["ratio"] <= 3 + 4, whole.describe_local(res)
    rng = np.random.default_rng(1)
    color = ((rng.standard_normal((nq, 33)) * np.exp(-np.arange(33) / 6.0)) * les.step_levels(nq, 7)[:, None]).astype(np.float32)
    want = propagation.colored_inputs(x[:1], K, color[None])
    scale = propagation.colored_inputs(np.abs(x[:1]), K, np.abs(color[None]))
    res = whole.compare_local(les.color_f32(x[0], K, color)[None], want, scale, K)
    assert 0 < res["ratio"] <= 33 + 4, whole.describe_local(res)
    delay = 2.25 + 150.0 * (0.5 + 0.5 * np.sin(0.4 * np.arange(nq)))
    for interp, taps in (("cubic", 4), ("linear", 2)):
        idx, w = les.delay_taps(T, K, delay, interp)
        want = les.delay_apply(x[0].astype(np.float64), idx, w, np.float64)
        assert np.array_equal(want[None], propagation.delayed_inputs(x[:1], K, delay[None], interp))
        scale = les.delay_apply(np.abs(x[0]).astype(np.float64), idx, np.abs(w), np.float64)
        res = whole.compare_local(les.delay_apply(x[0], idx, w, np.float32), want, scale, K)
        assert 0 < res["ratio"] <= taps + 4, whole.describe_local(res)
