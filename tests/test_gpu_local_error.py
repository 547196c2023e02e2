"""GPU tests of the local error bound and of exact scaling.

Locality: the error of output sample n against float64 is held to float32 rounding of the magnitudes that can reach n -
A_W of oracle/whole.local_scale, the float64 oracle fed |x| and |chunk IRs| and widened by one FIR row - not to the render's
peak.  Inputs are staircases in level (local_error_support.staircase: 2^0 .. 2^-34, about 200 dB), so a leak of a loud
passage, source, item or session into a quiet one at 1e-6, stale data at -110 dB or a threshold that eats small values
fails, where `rel_err <= 1e-5` passes.  Two bounds per case: the derived backstop c_wc, and 8 x r_ref, r_ref being the
ratio of the float32 reference arithmetic (plain numpy, direct form; test_local_error_cpu.py) on the same scene.

Exact scaling: every linear stage is float32 multiply-add, so f(2^k x) == 2^k f(x) and f(-x) == -f(x) bit for bit while
nothing leaves the normal range (asserted from the data; subnormal behaviour is out of scope).

Every case prints its kernel, its ratio, r_ref and where the worst sample lies."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from oracle import whole
import binaural_audio_synthesis_amd as bas
from binaural_audio_synthesis_amd import propagation, reverb
import local_error_support as les
from local_error_support import FIR_CASES, SHARP

pytestmark = pytest.mark.gpu
KS = (-40, -13, 13, 40)


def device_table(h):
    return bas.irs_and_delaydiffs(h.upsampling, h.diffs_left, h.diffs_right, h.irs_left, h.irs_right)


@contextlib.contextmanager
def kernel_for(case, how):
    """The library and environment that give `case` the kernel `how` names (the mechanisms of test_gpu_parity.py,
    test_gpu_split.py and test_gpu_quad.py); checks that it lands there and yields the kernel's name."""
    n_src, n, K, S, L = case
    t_in = -(-n // K) * K
    env = {}
    if how.get("force"):
        env["BAS_FORCE_KERNEL"] = how["force"]
    if how.get("split"):
        env.update(BAS_FZ_NW="4", BAS_FZ_SPLIT="1")
    diag = bool(env) or "plan" in how
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        with (bas._hip.use_library(bas._hip.DIAG_LIB_PATH) if diag else contextlib.nullcontext()):
            lib = bas._hip.lib()
            if how["fused"]:
                assert lib.bas_render_fused_supported(n_src, t_in, K, S, L) == 1
                name = lib.bas_render_fused_kernel_name(n_src, t_in, K, S, L).decode()
            else:
                name = lib.bas_render_kernel_name(n_src, t_in, K, S, L).decode()
            if diag and how["fused"]:
                lib.bas_debug_fused_plan.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int]
                code = lib.bas_debug_fused_plan(n_src, t_in, K, S, L)
                if how.get("split"):
                    assert code & 32 and code & 15 == 4 and "bas_render_fs_kernel" in name, (code, name)
                else:
                    bit, nw = how["plan"]
                    assert code & bit and code & 15 == nw and name == "bas_render_fq_kernel", (code, name)
            if "name" in how:
                assert name == how["name"], name
            yield name
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def render_with_peak(x, K, S, elev, azim, d, fused):
    """render_sources' own steps with the peak handed out: (y [T_out, 2] device float32, the peak as a float)."""
    import torch
    ah = bas.apply_hrtf
    n_src, n = x.shape
    xp = ah.padded_rows(n_src, -(-n // K) * K, "cuda")
    xp[:, :n] = torch.from_numpy(x).cuda()
    idx, w = bas.sphere.interpolation_params_batch(elev, azim)
    idx_t, w_t = ah._params_to_device(d, idx, w)
    y, peak = ah.render_params_device(xp, K, S, d, idx_t, w_t, "none", fused=fused)
    return y.t().contiguous(), float(peak[0])


def check(tag, kernel, got, want, scale, K, r_ref, c_wc):
    """Both bounds and the exact zeros; prints the case's line.  Returns the comparison."""
    res = whole.compare_local(got, want, scale, K)
    print(f"{tag}: kernel {kernel}, ratio {res['ratio']:.3g}, r_ref {r_ref:.3g} (bound {SHARP * r_ref:.3g}, backstop {c_wc}); "
          f"{whole.describe_local(res)}")
    assert res["finite"] and res["zeros_ok"], whole.describe_local(res)
    assert res["ratio"] <= c_wc, (kernel, whole.describe_local(res))
    assert res["ratio"] <= SHARP * r_ref, (kernel, r_ref, whole.describe_local(res))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# locality on every FIR kernel
# ---------------------------------------------------------------------------------------------------------------------
def run_fir_case(name):
    """One locality case, also what tools/local_error_margins.py records: a dict with the kernel and the comparison."""
    case, how = FIR_CASES[name]
    sc, want, scale, ref = les.reference(case)
    with kernel_for(case, how) as kernel:
        d = device_table(sc.h)
        got = bas.render_sources(np.array(sc.x), sc.K, sc.S, sc.elev, sc.azim, d, normalize="none", fused=how["fused"]).cpu().numpy()
    assert got.shape == (sc.t_out, 2)
    return dict(case=name, shape=list(case), kernel=kernel, got=got.T, want=want, scale=scale, K=sc.K, r_ref=ref["ratio"],
                c_wc=sc.c_wc)


@pytest.mark.parametrize("name", sorted(FIR_CASES))
def test_fir_kernel_error_is_local(name):
    r = run_fir_case(name)
    check(name, r["kernel"], r["got"], r["want"], r["scale"], r["K"], r["r_ref"], r["c_wc"])


# ---------------------------------------------------------------------------------------------------------------------
# exact scaling on every FIR kernel
# ---------------------------------------------------------------------------------------------------------------------
def assert_normal_range(x, taps, n_src, ks=KS):
    """The issue's conditions, from the data: nothing underflows at the smallest k, nothing overflows at the largest.
    taps [rows, m]: the table's rows (a chunk IR is a convex blend of every U-th tap of such rows, so a row's sum of
    magnitudes bounds the chunk IR's)."""
    ax, at = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(taps, dtype=np.float64))
    assert 2.0 ** min(ks) * ax[ax > 0].min() * 2.0 ** -24 * at[at > 0].min() >= 2.0 ** -126
    assert 2.0 ** max(ks) * n_src * ax.max() * at.sum(axis=-1).max() < 2.0 ** 127


def admissible_ks(x, weights, n_terms):
    """KS, with the negative exponents raised as far as the first condition needs for these weights (a stage whose
    smallest weight lies far below the render table's 2^-18: said in the case's output), then both conditions asserted."""
    ax, aw = np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(weights, dtype=np.float64))
    k_min = int(np.ceil(-126 + 24 - np.log2(ax[ax > 0].min()) - np.log2(aw[aw > 0].min())))
    ks = tuple(sorted({max(k, k_min) if k < 0 else k for k in KS}))
    assert k_min <= -13, k_min
    if ks != KS:
        print(f"exponents {ks} instead of {KS}: the smallest weight is 2^{np.log2(aw[aw > 0].min()):.1f}")
    assert_normal_range(x, aw.reshape(-1, aw.shape[-1]), n_terms, ks)
    return ks


@pytest.mark.parametrize("name", sorted(FIR_CASES))
def test_fir_kernel_scales_exactly(name):
    """f(2^k x) == 2^k f(x) for k = -40, -13, 13, 40 and f(-x) == -f(x), outputs and peak, bit for bit, at the base level
    (white noise in multiples of 2^-17; the table's taps lie in 2^-18 .. 1, so every product and sum stays normal)."""
    import torch
    case, how = FIR_CASES[name]
    n_src, n, K, S, L = case
    h = les.table(L)
    x = np.stack([bas.synth.integer_noise(7000 + i, n, 0.25) for i in range(n_src)])
    elev, azim = les.angles(n_src, n, K)
    assert_normal_range(x, np.concatenate([h.irs_left, h.irs_right]), n_src)
    with kernel_for(case, how) as kernel:
        d = device_table(h)
        base, peak = render_with_peak(x, K, S, elev, azim, d, how["fused"])
        assert peak > 0 and peak == float(base.abs().max())
        for k in KS:
            s = np.float32(2.0 ** k)
            y, p = render_with_peak(x * s, K, S, elev, azim, d, how["fused"])
            assert torch.equal(y, base * float(s)), (kernel, k, int((y != base * float(s)).sum()))
            assert p == peak * 2.0 ** k, (kernel, k, p, peak)
        y, p = render_with_peak(-x, K, S, elev, azim, d, how["fused"])
        assert torch.equal(y, -base) and p == peak, kernel              # (-0 == +0 for torch.equal)
    print(f"{name}: kernel {kernel}, peak {peak:.6g}: exact for k in {KS} and under negation")


# ---------------------------------------------------------------------------------------------------------------------
# isolation between the items of a batch
# ---------------------------------------------------------------------------------------------------------------------
BATCH = dict(n_src=3, N=6000, K=512, S=32, L=128, overall=(0, -30, 0, -34))


def batch_scene():
    c = BATCH
    K, L = c["K"], c["L"]
    lengths = [6000, K + 1, 4700, 3300]                                  # ragged; one item of K + 1 samples
    run = les.pick_run(c["N"], K, c["S"], L)
    x = np.stack([les.staircase_rows(c["n_src"], c["N"], run, 5200 + 10 * b, overall=c["overall"][b]) for b in range(4)])
    for b, n in enumerate(lengths):
        x[b, :, n:] = 0
    elev, azim = les.angles(4 * c["n_src"], c["N"], K)
    nq = elev.shape[1]
    return x, lengths, elev.reshape(4, c["n_src"], nq), azim.reshape(4, c["n_src"], nq)


def batch_references(x, lengths, elev, azim):
    """Per item: (want, A_W, r_ref) of the item rendered alone, from the float64 oracle and the float32 restatement."""
    c = BATCH
    h = les.table(c["L"])
    out = []
    for b, n in enumerate(lengths):
        in_length = -(-n // c["K"]) * c["K"]
        nq = in_length // c["K"] + 1
        xp = np.zeros((c["n_src"], in_length), dtype=np.float32)
        xp[:, :n] = x[b, :, :n]
        irs_of = whole.irs_from_angles(h, elev[b][:, :nq], azim[b][:, :nq])
        want = whole.render_mix_whole(xp, c["K"], c["S"], irs_of)
        scale = whole.local_scale(xp, c["K"], c["S"], irs_of)
        ref = whole.compare_local(les.render_f32_direct(xp, c["K"], c["S"], irs_of), want, scale, c["K"])
        out.append((want, scale, ref["ratio"]))
    return out


def run_batch_case():
    c = BATCH
    x, lengths, elev, azim = batch_scene()
    refs = batch_references(x, lengths, elev, azim)
    d = device_table(les.table(c["L"]))
    out, out_len, peaks = bas.render_batch(x, c["K"], c["S"], elev, azim, d, lengths=lengths, normalize="none")
    out, out_len = out.cpu().numpy(), out_len.cpu().numpy()
    res = []
    for b, (want, scale, r_ref) in enumerate(refs):
        assert int(out_len[b]) == want.shape[1]
        res.append(dict(case=f"render_batch[{b}]", kernel="render_batch", got=out[b, :int(out_len[b])].T, want=want, scale=scale,
                        K=c["K"], r_ref=r_ref, c_wc=4 * c["n_src"] * c["L"] + 64, peak=float(peaks[b])))
    return res


def test_render_batch_items_are_isolated():
    """Four items at overall levels 2^0, 2^-30, 2^0, 2^-34 on top of the staircase, ragged lengths, one of K + 1
    samples: every item within the bounds of its OWN scale, so a loud neighbour leaks nothing into a quiet item."""
    res = run_batch_case()
    peaks = [r["peak"] for r in res]
    assert peaks[1] < 2.0 ** -25 * peaks[0] and peaks[3] < 2.0 ** -25 * peaks[2]
    for r in res:
        check(r["case"], r["kernel"], r["got"], r["want"], r["scale"], r["K"], r["r_ref"], r["c_wc"])
        assert r["peak"] == float(np.abs(r["got"]).max())


def test_render_batch_scales_exactly():
    import torch
    c = BATCH
    _, lengths, elev, azim = batch_scene()
    rng_x = np.stack([np.stack([bas.synth.integer_noise(7100 + 10 * b + i, c["N"], 0.25) for i in range(c["n_src"])])
                      for b in range(4)])
    h = les.table(c["L"])
    assert_normal_range(rng_x, np.concatenate([h.irs_left, h.irs_right]), c["n_src"])
    d = device_table(h)
    base, _, peaks = bas.render_batch(rng_x, c["K"], c["S"], elev, azim, d, lengths=lengths, normalize="none")
    for k in KS:
        s = np.float32(2.0 ** k)
        y, _, p = bas.render_batch(rng_x * s, c["K"], c["S"], elev, azim, d, lengths=lengths, normalize="none")
        assert torch.equal(y, base * float(s)) and torch.equal(p, peaks * float(s)), k
    y, _, p = bas.render_batch(-rng_x, c["K"], c["S"], elev, azim, d, lengths=lengths, normalize="none")
    assert torch.equal(y, -base) and torch.equal(p, peaks)


# ---------------------------------------------------------------------------------------------------------------------
# the late tail: the partitioned convolver against reverb.long_fir, on the frame grid
# ---------------------------------------------------------------------------------------------------------------------
def run_late_case(Np, Lr, lag):
    import torch
    bus, h, n_out, want, A = les.long_fir_reference(Lr, lag)
    scale = whole.frame_max(A, Np)
    ref = whole.compare_local(les.long_fir_f32_fft(bus, h, lag, n_out, Np), want, scale)
    out = torch.full((1, 2, n_out), float("nan"), dtype=torch.float32, device="cuda")
    reverb.long_fir_device(torch.from_numpy(np.array(bus)[None]).cuda(), reverb.LateTail(np.array(h), lag), Np, out)
    return dict(case=f"long_fir[Np={Np},Lr={Lr},lag={lag}]", kernel="bas_long_fir_f32", got=out[0].cpu().numpy(), want=want,
                scale=scale, K=Np, r_ref=ref["ratio"], c_wc=les.long_fir_backstop(Np))


@pytest.mark.parametrize("Np,Lr,lag", les.LATE_CASES)
def test_long_fir_error_is_local(Np, Lr, lag):
    """A staircase bus through a tail that decays by 60 dB; Np = 128 is what LateStream uses at K = 128."""
    r = run_late_case(Np, Lr, lag)
    check(r["case"], r["kernel"], r["got"], r["want"], r["scale"], r["K"], r["r_ref"], r["c_wc"])


@pytest.mark.parametrize("Np", [32, 128, 512])
def test_long_fir_scales_exactly(Np):
    import torch
    rng = np.random.default_rng(Np)
    Lr, lag, T = 4099, 700, 20000
    bus = bas.synth.integer_noise(7300 + Np, T, 0.25)[None]
    h = (rng.standard_normal((2, Lr)) * 10.0 ** (-3.0 * np.arange(Lr) / Lr)).astype(np.float32)
    ks = admissible_ks(bus, h, 1)
    tail = reverb.LateTail(h, lag)
    n_out = T + lag + Lr - 1

    def run(b):
        out = torch.full((1, 2, n_out), float("nan"), dtype=torch.float32, device="cuda")
        peak = torch.zeros(1, dtype=torch.float32, device="cuda")
        reverb.long_fir_device(torch.from_numpy(b).cuda(), tail, Np, out, peak=peak)
        return out, float(peak[0])

    base, peak = run(bus)
    assert peak == float(base.abs().max()) > 0
    for k in ks:
        y, p = run(bus * np.float32(2.0 ** k))
        assert torch.equal(y, base * 2.0 ** k) and p == peak * 2.0 ** k, k
    y, p = run(-bus)
    assert torch.equal(y, -base) and p == peak


# ---------------------------------------------------------------------------------------------------------------------
# the row stages alone, W = 0
# ---------------------------------------------------------------------------------------------------------------------
ROWS_T = 6000
ROWS_RUN = 211


def _rows(n_rows, seed):
    return les.stage_rows(n_rows, ROWS_T, ROWS_RUN, seed)


def _noise_rows(n_rows, seed):
    return np.stack([bas.synth.integer_noise(seed + s, ROWS_T, 0.25) for s in range(n_rows)])


def _scaling(f, x, what, weights, n_terms):
    """f(2^k x) == 2^k f(x) for k in KS and f(-x) == -f(x), bit for bit; f: numpy float32 -> device tensor.  weights: the
    stage's coefficients [.., taps] for the normal-range conditions, n_terms: rows summed into one output."""
    import torch
    ks = admissible_ks(x, weights, n_terms)
    base = f(x)
    for k in ks:
        assert torch.equal(f(x * np.float32(2.0 ** k)), base * 2.0 ** k), (what, k)
    assert torch.equal(f(-x), -base), what


def run_delay_case(interp):
    K, R = 512, 3
    x = _rows(R, 6100)
    nq = (ROWS_T - 1) // K + 2
    t = np.arange(nq, dtype=np.float64)
    delay = np.stack([2.25 + 150.0 * (0.5 + 0.5 * np.sin(0.4 * t + r)) for r in range(R)])
    want, scale, ref = (np.zeros((R, ROWS_T)) for _ in range(3))
    weights = []
    for r in range(R):
        idx, w = les.delay_taps(ROWS_T, K, delay[r], interp)
        want[r] = les.delay_apply(x[r].astype(np.float64), idx, w, np.float64)
        scale[r] = les.delay_apply(np.abs(x[r]).astype(np.float64), idx, np.abs(w), np.float64)
        ref[r] = les.delay_apply(x[r], idx, w, np.float32)
        weights.append(w.T)
    assert np.array_equal(want, propagation.delayed_inputs(x, K, delay, interp))              # the definition itself
    f = lambda v: propagation.delayed_inputs_device(v, K, delay, interp)                      # noqa: E731
    return dict(case=f"delay[{interp}]", kernel="bas_delay_rows_f32", got=f(x).cpu().numpy(), want=want, scale=scale, K=K,
                r_ref=whole.compare_local(ref, want, scale, K)["ratio"], c_wc=(4 if interp == "cubic" else 2) + 4,
                f=f, base=_noise_rows(1, 61).repeat(R, axis=0), weights=np.concatenate(weights), n_terms=1)


def _colour(R, nq, M, seed):
    """Decaying taps around a delta that drift over the boundaries and step by 2^-20 between them."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((R, nq, M)) * np.exp(-np.arange(M) / 6.0) * 0.4
    c[:, :, 0] += 1.0
    steps = np.stack([les.step_levels(nq, seed + 10 * r) for r in range(R)])
    return (c * steps[:, :, None]).astype(np.float32)


def run_colour_case(M):
    K, R = 512, 3
    x = _rows(R, 6200 + M)
    nq = (ROWS_T - 1) // K + 2
    color = _colour(R, nq, M, seed=M)
    want = propagation.colored_inputs(x, K, color)
    scale = propagation.colored_inputs(np.abs(x), K, np.abs(color))
    ref = np.stack([les.color_f32(x[r], K, color[r]) for r in range(R)])
    f = lambda v: propagation.colored_inputs_device(v, K, color)                              # noqa: E731
    return dict(case=f"colour[M={M}]", kernel="bas_color_rows_f32", got=f(x).cpu().numpy(), want=want, scale=scale, K=K,
                r_ref=whole.compare_local(ref, want, scale, K)["ratio"], c_wc=M + 4,
                f=f, base=_noise_rows(1, 62).repeat(R, axis=0), weights=color, n_terms=1)


def run_bus_mix_case(K):
    import torch
    n_src = 5
    x = _rows(n_src, 6300 + K)
    nq = (ROWS_T - 1) // K + 2
    send = np.stack([les.step_levels(nq, 40 + s) * (0.3 + 0.2 * s) * (-1.0) ** s for s in range(n_src)])
    in_length = -(-ROWS_T // K) * K
    assert send.shape[1] >= in_length // K + 1
    want = reverb.bus_mix(x, send[:, :in_length // K + 1], K)[:ROWS_T]
    scale = reverb.bus_mix(np.abs(x), np.abs(send[:, :in_length // K + 1]), K)[:ROWS_T]
    send_d = torch.from_numpy(send).cuda()

    def f(v):
        out = torch.full((ROWS_T,), float("nan"), dtype=torch.float32, device="cuda")
        reverb.bus_mix_device(torch.from_numpy(np.ascontiguousarray(v)).cuda(), send_d, K, out)
        return out

    return dict(case=f"bus_mix[K={K}]", kernel="bas_bus_mix_f32", got=f(x).cpu().numpy(), want=want, scale=scale, K=K,
                r_ref=whole.compare_local(les.bus_mix_f32(x, send, K), want, scale, K)["ratio"], c_wc=n_src + 4,
                f=f, base=_noise_rows(n_src, 63), weights=send.T, n_terms=1)


def _ambi_angles(n, nq, seed):
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, nq)[None, :]
    return (rng.uniform(-1.2, 1.2, (n, 1)) * np.cos(2.0 * t + rng.random((n, 1))),
            rng.uniform(-3.0, 3.0, (n, 1)) + 4.0 * t * rng.uniform(-1, 1, (n, 1)))


def run_encode_case():
    from binaural_audio_synthesis_amd import ambisonics as ambi
    K, n_src, order = 512, 6, 3
    x = _rows(n_src, 6400)
    nq = -(-ROWS_T // K) + 1
    elev, azim = _ambi_angles(n_src, nq, 3)
    gain = np.stack([les.step_levels(nq, 50 + s) * (0.5 + 0.1 * s) for s in range(n_src)])
    E = ambi.encoding_gains(elev, azim, order, "sn3d", gain)
    want = ambi.encode(x, K, E)
    scale = ambi.encode(np.abs(x), K, np.abs(E))
    f = lambda v: ambi.encode_bed(v, K, elev, azim, order, gain=gain)                         # noqa: E731
    return dict(case="encode_bed[order 3]", kernel="bas_ambi_encode_f32", got=f(x).cpu().numpy(), want=want, scale=scale, K=K,
                r_ref=whole.compare_local(les.lerp_mix_f32(x, E.astype(np.float32), K), want, scale, K)["ratio"],
                c_wc=n_src + 4, f=f, base=_noise_rows(n_src, 64), weights=np.abs(E).sum(axis=1), n_terms=1)


def run_decode_case():
    from binaural_audio_synthesis_amd import ambisonics as ambi
    from test_gpu_head import _head_track
    K, order = 512, 3
    dec = ambi.Decoder(order)
    bed = _rows(dec.C, 6500)
    nq = -(-ROWS_T // K) + 1
    head = _head_track(nq, seed=9)
    M = ambi.mixing_matrices(dec, head)
    want = ambi.decode(bed, K, M)
    scale = ambi.decode(np.abs(bed), K, np.abs(M))
    f = lambda v: ambi.bed_sources(v, K, dec, head)[0]                                        # noqa: E731
    return dict(case="bed_sources[order 3]", kernel="bas_matrix_mix_f32", got=f(bed).cpu().numpy(), want=want, scale=scale, K=K,
                r_ref=whole.compare_local(les.lerp_mix_f32(bed, M.astype(np.float32).transpose(0, 2, 1), K), want, scale, K)["ratio"],
                c_wc=dec.C + 4, f=f, base=_noise_rows(dec.C, 65), weights=M, n_terms=1)


ROW_CASES = {"delay-cubic": (run_delay_case, "cubic"), "delay-linear": (run_delay_case, "linear"),
             "colour-M1": (run_colour_case, 1), "colour-M33": (run_colour_case, 33), "colour-M64": (run_colour_case, 64),
             "bus_mix-K36": (run_bus_mix_case, 36), "bus_mix-K512": (run_bus_mix_case, 512),
             "encode_bed": (run_encode_case,), "bed_sources": (run_decode_case,)}


@pytest.mark.parametrize("name", sorted(ROW_CASES))
def test_row_stage_error_is_local_and_scales(name):
    """Delay (cubic, linear), colour (M = 1, 33, 64), bus mix (K = 36, 512), the ambisonic encoder and the decoder rows at
    order 3 against their float64 definitions: the scale is sum |weight| |input| over the taps of the sample (W = 0), the
    inputs are staircases, and colour taps, sends and gains step by 2^-20 between chunk boundaries.  Then exact scaling."""
    run, *args = ROW_CASES[name]
    r = run(*args)
    check(r["case"], r["kernel"], r["got"], r["want"], r["scale"], r["K"], r["r_ref"], r["c_wc"])
    _scaling(r["f"], r["base"], r["case"], r["weights"], r["n_terms"])


def test_limiter_scales_with_its_ceiling():
    """limit(2^k y, ceiling = 2^k c) == 2^k limit(y, ceiling = c) inside |y| <= 2^20 c, A, Hd = 64, 100."""
    import torch
    c, A, Hd = 0.5, 64, 100
    y = (np.random.default_rng(5).standard_normal((2, 6000, 2)) * 0.6).astype(np.float32)
    assert np.abs(y).max() > c and np.abs(y).max() <= 2.0 ** 20 * c
    yd = torch.from_numpy(y).cuda()
    base, red, peaks = bas.limit(yd, c, A, Hd, return_meters=True)
    assert float(base.abs().max()) <= c
    for k in (-13, 13):
        got, red_k, peaks_k = bas.limit(yd * 2.0 ** k, c * 2.0 ** k, A, Hd, return_meters=True)
        assert torch.equal(got, base * 2.0 ** k), k
        assert torch.equal(peaks_k, peaks * 2.0 ** k) and torch.equal(red_k, red), k
    assert torch.equal(bas.limit(-yd, c, A, Hd), -base)


# ---------------------------------------------------------------------------------------------------------------------
# isolation between the sessions of a batched stream, and between the blocks of a stream
# ---------------------------------------------------------------------------------------------------------------------
STREAM = dict(n_src=3, K=512, S=32, L=128, blocks=(512, 512, 2048, 512), overall=(0, -30, 0, -34))


def run_stream_batch_case():
    import torch
    c = STREAM
    K, S, L, n_src, G = c["K"], c["S"], c["L"], c["n_src"], 4
    n = sum(c["blocks"])
    run = les.pick_run(n, K, S, L)
    x = np.stack([les.staircase_rows(n_src, n, run, 5600 + 10 * g, overall=c["overall"][g]) for g in range(G)])
    elev, azim = les.angles(G * n_src, n, K)
    nq = elev.shape[1]
    elev, azim = elev.reshape(G, n_src, nq), azim.reshape(G, n_src, nq)
    h = les.table(L)
    sb = bas.StreamBatchRenderer(device_table(h), G, n_src, K, S, graph=True)
    outs, pos, last_B = [], 0, None
    for B in c["blocks"]:
        if B != last_B:
            sb.prepare(B)
        last_B = B
        q = slice(pos // K, (pos + B) // K + 1)
        outs.append(sb.process(x[:, :, pos:pos + B], elev[:, :, q], azim[:, :, q]).cpu().numpy())
        pos += B
    tails = sb.finish(range(G)).cpu().numpy()
    got = np.concatenate(outs + [tails], axis=1)                         # [G, n + L - 1, 2]
    res = []
    for g in range(G):
        irs_of = whole.irs_from_angles(h, elev[g], azim[g])
        want = whole.render_mix_whole(x[g], K, S, irs_of)
        scale = whole.local_scale(x[g], K, S, irs_of)
        r_ref = whole.compare_local(les.render_f32_direct(x[g], K, S, irs_of), want, scale, K)["ratio"]
        res.append(dict(case=f"stream_batch[{g}]", kernel="StreamBatchRenderer", got=got[g].T, want=want, scale=scale, K=K,
                        r_ref=r_ref, c_wc=4 * n_src * L + 64))
    return res


def test_stream_batch_sessions_are_isolated():
    """Four sessions at overall levels 2^0, 2^-30, 2^0, 2^-34, blocks of 512 and one of 2048 through prepare() and graph
    replay: every session within the bounds of its own scale, blocks and tail."""
    for r in run_stream_batch_case():
        check(r["case"], r["kernel"], r["got"], r["want"], r["scale"], r["K"], r["r_ref"], r["c_wc"])


def run_stream_case():
    from test_gpu_gain import _gains
    from test_gpu_delay import _smooth_delays
    from test_gpu_color import _filters
    c = STREAM
    K, S, L, n_src, M, max_delay = c["K"], c["S"], c["L"], c["n_src"], 64, 100.0
    n = sum(c["blocks"])
    block_of = np.repeat(np.arange(len(c["blocks"])), c["blocks"])
    x = np.zeros((n_src, n), dtype=np.float32)                          # a loud block, a quiet one, a loud one, a quiet one
    for i, lev in enumerate(((0, -34, 0, -34), (-10, -34, -20, -34))):
        x[i] = (bas.synth.integer_noise(5700 + i, n).astype(np.float64) * np.ldexp(1.0, np.array(lev)[block_of])).astype(np.float32)
    elev, azim = les.angles(n_src, n, K)
    nq = elev.shape[1]
    gain = _gains(n_src, nq, seed=83)
    delay = _smooth_delays(n_src, nq, K, seed=84, hi=max_delay)
    color = _filters(n_src, nq, M, seed=85)
    h = les.table(L)
    # float64: the stages' definitions, and the scale through their absolute forms
    x1 = propagation.delayed_inputs(x, K, delay, "cubic", max_delay=max_delay)
    assert np.array_equal(x1, propagation.delayed_inputs(x, K, delay, "cubic"))             # the clamp changes nothing here
    x2 = propagation.colored_inputs(x1, K, color)
    taps = [les.delay_taps(n, K, delay[r], "cubic") for r in range(n_src)]
    s1 = np.stack([les.delay_apply(np.abs(x[r]).astype(np.float64), idx, np.abs(w), np.float64) for r, (idx, w) in enumerate(taps)])
    s2 = propagation.colored_inputs(s1, K, np.abs(color))

    def irs_of(i):
        return whole.irs_from_angles(h, elev, azim)(i) * gain[i][:, None, None]

    want = whole.render_mix_whole(x2, K, S, irs_of)
    scale = whole.local_scale(s2, K, S, irs_of)
    r32 = np.stack([les.color_f32(les.delay_apply(x[r], idx, w, np.float32), K, color[r]) for r, (idx, w) in enumerate(taps)])
    r_ref = whole.compare_local(les.render_f32_direct(r32, K, S, irs_of), want, scale, K)["ratio"]
    st = bas.StreamRenderer(device_table(h), n_src, K, S, graph=True, max_delay=max_delay, color_taps=M)
    outs, pos, last_B = [], 0, None
    for B in c["blocks"]:
        if B != last_B:
            st.prepare(B)
        last_B = B
        q = slice(pos // K, (pos + B) // K + 1)
        outs.append(st.process(x[:, pos:pos + B], elev[:, q], azim[:, q], gain=gain[:, q], delay=delay[:, q],
                               color=color[:, q]).cpu().numpy())
        pos += B
    outs.append(st.finish().cpu().numpy())
    got = np.concatenate(outs)
    assert got.shape == (n + L - 1, 2)
    return dict(case="stream[gain,delay,colour]", kernel="StreamRenderer", got=got.T, want=want, scale=scale, K=K, r_ref=r_ref,
                c_wc=(4 * n_src * L + 64) + (M + 4) + (4 + 4), blocks=c["blocks"])


def test_stream_blocks_leak_nothing_into_quiet_ones():
    """graph=True, blocks (512, 512, 2048, 512), gain, delay (max_delay 100) and colour (M = 64) on: a loud block, then a
    quiet one.  The scale goes through the float64 definitions of the stages, so the quiet block's samples beyond the reach
    of the loud one (L - 1 + W, the delay and the colour's taps) are held to their own scale: halo, histories and the
    carried tail leak nothing."""
    r = run_stream_case()
    s = r["scale"]
    quiet = s[:, 512:1024] <= 2.0 ** -30 * s.max()
    assert 0.2 <= quiet.mean() < 1.0, quiet.mean()                       # the quiet block has samples out of the loud one's reach
    check(r["case"], r["kernel"], r["got"], r["want"], r["scale"], r["K"], r["r_ref"], r["c_wc"])
