"""Cost of scene colour, written to profiles/scene_color_bench.json:
  - bas_color_design_f32 alone for 1792 rows x 87 boundaries of 6 bands (256 sources x 7 images, one second of chunks of
    512) at M = 16, 32 and 64, beside a device copy of the same output bytes (torch's copy kernel: the memory-bound floor)
    and the scene kernel with and without the bands on that shape;
  - a 256 x 512 SceneStreamRenderer block (order 1, banded room: 1792 rows) with and without color (graph replay);
  - render_scene of 32 sources x 10 s at order 1 (banded room) with and without color.
Every GPU step runs in a child process of its own under `timeout`, one after the other; the first that fails ends the run
(nothing is started on a device after a fault).  Usage: python tools/bench_scene_color.py [--reps N] [--out FILE] [--step NAME]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = {"kernel": 240, "stream": 300, "scene": 300}                # name -> time limit in seconds
KEYS = {"kernel": "design_kernel_1792x87", "stream": "scene_stream_256x512_order1", "scene": "render_scene_32x10s_order1"}
BANDS = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)
CARPET = np.array([0.99, 0.97, 0.93, 0.80, 0.65, 0.55])
PANEL = np.array([0.80, 0.88, 0.93, 0.95, 0.96, 0.96])
WALLS = np.stack([CARPET, PANEL, PANEL, CARPET, CARPET ** 0.5, PANEL])
SIZE = np.array([6.0, 5.0, 4.0])


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


def _paths(rng, n_src, nq):
    """Sources on closed paths inside the room, turning about the vertical: (pos [n_src, nq, 3], orient [n_src, nq, 4])."""
    tt = np.linspace(0, 1, nq)[None, :, None]
    pos = SIZE / 2 + (SIZE / 2 - 0.4) * np.sin(2 * np.pi * rng.uniform(0.5, 2, (n_src, 1, 3)) * tt + rng.uniform(0, 6, (n_src, 1, 3)))
    yaw = 2 * np.pi * rng.uniform(0.5, 3, (n_src, 1)) * tt[..., 0] + rng.uniform(0, 6, (n_src, 1))
    orient = np.stack([np.cos(yaw / 2), np.zeros_like(yaw), np.zeros_like(yaw), np.sin(yaw / 2)], axis=-1)
    return pos, orient


def _table():
    import binaural_audio_synthesis_amd as bas
    tb = bas.synth.make_table("consistent", 0, upsampling=8).truncated(128)
    return bas.irs_and_delaydiffs(tb.upsampling, tb.diffs_left, tb.diffs_right, tb.irs_left, tb.irs_right)


def step_kernel(reps):
    import torch
    from binaural_audio_synthesis_amd import propagation as prop, scene
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    n_src, nb, fs = 256, 87, 44100.0
    room = scene.Room(SIZE, beta=WALLS, order=1, bands=BANDS, taps=32)
    rows = n_src * room.n_img
    res = {"device": torch.cuda.get_device_name(0), "filters": rows * nb, "bands": len(BANDS)}
    L = torch.from_numpy(rng.uniform(np.log(prop.FIR_FLOOR), 0.0, (rows, nb, len(BANDS)))).to(dev)
    for M in (16, 32, 64):
        basis = torch.from_numpy(prop.cepstral_basis(BANDS, fs, M)).to(dev)
        out = torch.empty((rows, nb, M), dtype=torch.float32, device=dev)
        src = torch.from_numpy(rng.standard_normal((rows, nb, M)).astype(np.float32)).to(dev)
        copy_us = _events_ms(lambda: out.copy_(src), reps) * 1e3
        us = _events_ms(lambda: prop.design_colors_device(L, basis, out=out), reps) * 1e3
        fmas = rows * nb * (len(BANDS) * M + M * (M - 1) // 2)
        res[f"M{M}"] = {"design_us": round(us, 1), "copy_same_output_bytes_us": round(copy_us, 1), "output_bytes": 4 * rows * nb * M,
                        "ratio_to_copy": round(us / copy_us, 2), "f64_GFMA_per_s": round(fmas / (us * 1e-6) / 1e9, 1)}
    pos, orient = _paths(rng, n_src, nb)
    pos, orient = torch.from_numpy(pos).to(dev), torch.from_numpy(orient).to(dev)
    col = scene.SceneColor(BANDS, taps=32, air=True, directivity=np.full(6, 0.5))
    res["scene_kernel_us"] = round(_events_ms(lambda: scene.scene_params_device(pos, fs, room=room, chunksize=512), reps) * 1e3, 1)
    res["scene_kernel_with_bands_us"] = round(_events_ms(
        lambda: scene.scene_color_params_device(pos, fs, room=room, chunksize=512, color=col, orient=orient), reps) * 1e3, 1)
    res["scene_kernel_note"] = "wall time of the Python call's launches (output allocation included), device events"
    return res


def step_stream(reps):
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import scene
    rng = np.random.default_rng(1)
    dev = torch.device("cuda")
    n_src, K, B, fs = 256, 512, 512, 44100.0
    tbl = _table()
    room = scene.Room(SIZE, beta=WALLS, order=1, bands=BANDS, taps=32)
    blk = torch.from_numpy(rng.standard_normal((n_src, B)).astype(np.float32)).to(dev)
    pos, orient = _paths(rng, n_src, 2)
    pos, orient = torch.from_numpy(pos).to(dev), torch.from_numpy(orient).to(dev)
    res = {}
    for name, col in (("no_color_static_bank", None),
                      ("color_air_and_cardioid", scene.SceneColor(BANDS, taps=32, air=True, directivity=np.full(6, 0.5)))):
        st = bas.SceneStreamRenderer(tbl, n_src, K, 32, fs, max_distance=30.0, room=room, graph=True, copy_out=False, color=col)
        st.prepare(B)
        kw = {} if col is None else dict(orient=orient)

        def one():
            st.process(blk, pos, **kw)
        ms_gpu = _events_ms(one, reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            one()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / reps
        res[name] = {"wall_us_per_block": round(wall * 1e6, 1), "gpu_us_per_block": round(ms_gpu * 1e3, 1),
                     "rows": n_src * room.n_img}
    return res


def step_scene(reps):
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import scene
    rng = np.random.default_rng(2)
    dev = torch.device("cuda")
    n_src, N, K, fs = 32, 441000, 512, 44100.0
    tbl = _table()
    sig = torch.from_numpy(rng.standard_normal((n_src, N)).astype(np.float32) * 0.1).to(dev)
    nq = -(-N // K) + 1
    pos, orient = _paths(rng, n_src, nq)
    pos, orient = torch.from_numpy(pos).to(dev), torch.from_numpy(orient).to(dev)
    lp = torch.from_numpy(np.tile(SIZE / 2, (nq, 1))).to(dev)
    room = scene.Room(SIZE, beta=WALLS, order=1, bands=BANDS, taps=32)
    col = scene.SceneColor(BANDS, taps=32, air=True, directivity=np.full(6, 0.5))
    res = {"taps_buffer_bytes": n_src * room.n_img * nq * 32 * 4}
    for name, kw in (("no_color_static_bank", {}), ("color_air_and_cardioid", dict(color=col, orient=orient))):
        ms = _events_ms(lambda: bas.render_scene(sig, K, 32, pos, tbl, fs, lp, room=room, normalize="none", **kw), max(reps // 10, 3))
        res[name] = {"ms": round(ms, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_color_bench.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process and print its JSON")
    args = ap.parse_args()
    if args.step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: nothing is measured without one")
        print("RESULT " + json.dumps({"kernel": step_kernel, "stream": step_stream, "scene": step_scene}[args.step](args.reps)))
        return
    res = {}
    for name, limit in STEPS.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
               "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            sys.stderr.write(p.stdout + p.stderr)
            raise SystemExit(f"step {name} failed with exit status {p.returncode}: nothing more is started")
        res[KEYS[name]] = json.loads(lines[0][len("RESULT "):])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
