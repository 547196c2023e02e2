"""Cost of the per-source colour, written to profiles/color_cost.json:
  - bas_color_rows_f32 alone on the bench scene's shape (256 x 441 000) for M = 16, 32, 64, static and per-boundary, beside
    a device copy of the same bytes (torch's copy kernel: the memory-bound floor) and §3.11's delay kernel on that shape;
  - a 256 x 512 StreamRenderer block with and without colour (graph replay, in-place inputs);
  - render_scene of 32 sources x 10 s at order 1 with a banded room and with a scalar room;
  - the band-centre errors of propagation.min_phase_fir for three materials (host only).
Every GPU step runs in a child process of its own under `timeout`, one after the other; the first that fails ends the run
(nothing is started on a device after a fault).  --host-only writes the design's errors alone and marks the GPU steps as
not measured.  Usage: python tools/bench_color.py [--reps N] [--out FILE] [--step NAME] [--host-only]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"kernel": 240, "stream": 240, "scene": 300}                # name -> time limit in seconds
BANDS = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)
CARPET = np.array([0.99, 0.97, 0.93, 0.80, 0.65, 0.55])
PANEL = np.array([0.80, 0.88, 0.93, 0.95, 0.96, 0.96])


def _events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def design_errors():
    from binaural_audio_synthesis_amd import propagation as prop
    fs, out = 48000.0, {}
    w = 2 * np.pi * np.array(BANDS) / fs
    for taps in (16, 32, 64):
        row = {}
        for name, mags in (("carpet", CARPET), ("panel", PANEL), ("carpet3", CARPET ** 3)):
            h = prop.min_phase_fir(BANDS, mags, fs, taps)
            H = np.abs(np.exp(-1j * np.outer(w, np.arange(taps))) @ h)
            row[name] = round(float(np.abs(20 * np.log10(H / mags)).max()), 3)
        out[str(taps)] = row
    return {"worst_band_centre_error_dB": out, "fs": fs, "bands_Hz": list(BANDS)}


def step_kernel(reps):
    import torch
    from binaural_audio_synthesis_amd import propagation as prop
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    n_src, N, K = 256, 441000, 512
    x = torch.from_numpy(rng.standard_normal((n_src, N)).astype(np.float32)).to(dev)
    nq = (N - 1) // K + 2
    out = torch.empty((n_src, (N + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :N]
    nbytes = 2 * 4 * n_src * N
    res = {"device": torch.cuda.get_device_name(0), "bytes_read_plus_written": nbytes}
    ms = _events_ms(lambda: out.copy_(x), reps)
    copy_us = ms * 1e3
    res["copy_same_bytes"] = {"us": round(copy_us, 1), "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 2)}
    t = np.arange(nq, dtype=np.float64)
    d = torch.from_numpy(2.0 + 400.0 * (0.5 + 0.5 * np.sin(t[None, :] * rng.uniform(0.02, 0.3, (n_src, 1))))).to(dev)
    ms = _events_ms(lambda: prop.delay_rows_device(x, d, K, "cubic", out), reps)
    res["delay_rows_cubic"] = {"us": round(ms * 1e3, 1), "ratio_to_copy": round(ms * 1e3 / copy_us, 2)}
    for M in (16, 32, 64):
        c = torch.from_numpy(rng.standard_normal((n_src, nq, M)).astype(np.float32)).to(dev)
        for name, cc, fmas in (("static", c[:, 0].contiguous(), M), ("per_boundary", c, 2 * M)):
            ms = _events_ms(lambda: prop.color_rows_device(x, cc, K, out), reps)
            res[f"color_rows_M{M}_{name}"] = {"us": round(ms * 1e3, 1), "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 2),
                                              "ratio_to_copy": round(ms * 1e3 / copy_us, 2),
                                              "TFMA_per_s": round(fmas * n_src * N / (ms * 1e-3) / 1e12, 2)}
    return res


def step_stream(reps):
    import torch
    import binaural_audio_synthesis_amd as bas
    rng = np.random.default_rng(1)
    dev = torch.device("cuda")
    n_src, K, B = 256, 512, 512
    tb = bas.synth.make_table("consistent", 0, upsampling=8).truncated(128)
    tbl = bas.irs_and_delaydiffs(tb.upsampling, tb.diffs_left, tb.diffs_right, tb.irs_left, tb.irs_right)
    blk = torch.from_numpy(rng.standard_normal((n_src, B)).astype(np.float32)).to(dev)
    res = {}
    for name, taps, static in (("no_color", None, False), ("color_M32_per_boundary", 32, False), ("color_M32_static", 32, True)):
        st = bas.StreamRenderer(tbl, n_src, K, 32, graph=True, copy_out=False, color_taps=taps)
        cv = None
        if taps:
            cv = st.color_view(B, static=static)
            cv.copy_(torch.from_numpy(rng.standard_normal(tuple(cv.shape)).astype(np.float32) * 0.2))
        st.prepare(B)
        iv = st.input_view(B)
        iv.copy_(blk)
        ev, ea = st.trajectory_views(B)

        def one():
            st.process(iv, ev, ea, color=cv)
        ms_gpu = _events_ms(one, reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            one()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / reps
        res[name] = {"wall_us_per_block": round(wall * 1e6, 1), "gpu_us_per_block": round(ms_gpu * 1e3, 1),
                     "launches_added_per_block_stated": "bas_color_rows_f32 + bas_delay_carry_f32" if taps else "none"}
    return res


def step_scene(reps):
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import scene
    rng = np.random.default_rng(2)
    dev = torch.device("cuda")
    n_src, N, K, fs = 32, 441000, 512, 44100.0
    tb = bas.synth.make_table("consistent", 0, upsampling=8).truncated(128)
    tbl = bas.irs_and_delaydiffs(tb.upsampling, tb.diffs_left, tb.diffs_right, tb.irs_left, tb.irs_right)
    sig = torch.from_numpy(rng.standard_normal((n_src, N)).astype(np.float32) * 0.1).to(dev)
    nq = -(-N // K) + 1
    size = np.array([6.0, 5.0, 4.0])
    tt = np.linspace(0, 1, nq)[None, :, None]
    pos = torch.from_numpy(size / 2 + (size / 2 - 0.4) * np.sin(2 * np.pi * rng.uniform(0.5, 2, (n_src, 1, 3)) * tt
                                                                   + rng.uniform(0, 6, (n_src, 1, 3)))).to(dev)
    lp = torch.from_numpy(np.tile(size / 2, (nq, 1))).to(dev)
    walls = np.stack([CARPET, PANEL, PANEL, CARPET, CARPET ** 0.5, PANEL])
    rooms = {"scalar_room": scene.Room(size, beta=walls[:, 3], order=1),
             "banded_room_32_taps": scene.Room(size, beta=walls, order=1, bands=BANDS, taps=32)}
    res = {}
    for name, room in rooms.items():
        ms = _events_ms(lambda: bas.render_scene(sig, K, 32, pos, tbl, fs, lp, room=room, normalize="none"), max(reps // 10, 3))
        res[name] = {"ms": round(ms, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_cost.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process and print its JSON")
    ap.add_argument("--host-only", action="store_true", help="write the filter design's errors only (no GPU step is run)")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: nothing is measured without one")
        print("RESULT " + json.dumps({"kernel": step_kernel, "stream": step_stream, "scene": step_scene}[args.step](args.reps)))
        return
    res = {"min_phase_fir": design_errors()}
    if args.host_only:
        res["gpu_steps"] = "not measured"
    for name, limit in ({} if args.host_only else STEPS).items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"step {name} failed with exit status {p.returncode}: nothing more is started")
        key = {"kernel": "rows_kernel_256x441000", "stream": "stream_renderer_256x512", "scene": "render_scene_32x10s_order1"}[name]
        res[key] = json.loads(lines[0][len("RESULT "):])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
