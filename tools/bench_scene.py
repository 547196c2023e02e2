"""Cost of Cartesian scenes, written to profiles/scene_cost.json:
  (a) bas_scene_params_f64 alone for the bench scene's 256 sources x 863 boundaries at orders 0, 1, 2 (1, 7, 25 images);
  (b) render_scene of 32 sources x 10 s at 44.1 kHz at orders 0, 1, 2 (wall time per call, device synchronised);
  (c) order 0 through the interface before render_scene: scene_params on the host, upload, render_sources(gain=, delay=);
  (d) a 64-source x 512-sample SceneStreamRenderer block with and without an order-1 room (graph replay, wall per block).
GPU times are between HIP events around `reps` back-to-back calls after a warm-up call; wall times are
time.perf_counter around the same loop with a device synchronisation at its end, host work included.
Usage: python tools/bench_scene.py [--reps N] [--out profiles/scene_cost.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROOM = (8.0, 6.0, 3.0)


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


def _wall_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def _paths(rng, n_src, nq):
    """Smooth closed paths inside ROOM and a listener walking a small circle."""
    size = np.array(ROOM)
    t = np.linspace(0.0, 1.0, nq)
    pos = size / 2 + (size / 2 - 0.4) * np.sin(2 * np.pi * rng.uniform(0.5, 2.0, (n_src, 1, 3)) * t[None, :, None]
                                               + rng.uniform(0, 2 * np.pi, (n_src, 1, 3)))
    lp = size / 2 + np.stack([0.5 * np.cos(2 * np.pi * t), 0.5 * np.sin(2 * np.pi * t), 0.0 * t], -1)
    return pos, lp


def main():
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import scene
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_cost.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps}
    fs, K, S = 44100.0, 512, 32
    rooms = {0: scene.Room(ROOM, order=0), 1: scene.Room(ROOM, order=1), 2: scene.Room(ROOM, order=2)}

    # ---- (a) the kernel alone
    n_src, nq = 256, 863
    pos, lp = _paths(rng, n_src, nq)
    pos_d, lp_d = torch.from_numpy(pos).to(dev), torch.from_numpy(lp).to(dev)
    kern = {}
    for order, room in rooms.items():
        out = tuple(torch.empty((n_src * room.n_img, nq), dtype=torch.float64, device=dev) for _ in range(4))
        ms = _events_ms(lambda: scene.scene_params_device(pos_d, fs, lp_d, room=room, out=out), 5 * args.reps)
        kern[f"order_{order}"] = {"n_img": room.n_img, "points": n_src * room.n_img * nq, "us": round(ms * 1e3, 1)}
    res["kernel_256x863"] = kern

    # ---- (b), (c) offline renders of 32 sources x 10 s
    host = bas.synth.make_table("consistent", 0).truncated(128)
    tbl = bas.irs_and_delaydiffs(host.upsampling, host.diffs_left, host.diffs_right, host.irs_left, host.irs_right)
    n_src, N = 32, 441000
    nq = -(-N // K) + 1
    x = torch.from_numpy((rng.standard_normal((n_src, N)) * 0.1).astype(np.float32)).to(dev)
    pos, lp = _paths(rng, n_src, nq)
    pos_d, lp_d = torch.from_numpy(pos).to(dev), torch.from_numpy(lp).to(dev)
    off = {}
    for order, room in rooms.items():
        ms = _wall_ms(lambda: bas.render_scene(x, K, S, pos_d, tbl, fs, lp_d, room=room), args.reps)
        off[f"order_{order}"] = {"rows": n_src * room.n_img, "wall_ms": round(ms, 3)}
    ms = _wall_ms(lambda: bas.render_scene(x, K, S, pos, tbl, fs, lp, room=rooms[0]), args.reps)
    off["order_0_host_positions"] = {"rows": n_src, "wall_ms": round(ms, 3)}

    def before():
        el, az, g, d = scene.scene_params(pos, fs, lp)
        return bas.render_sources(x, K, S, el, az, tbl, gain=g, delay=d)
    off["order_0_host_params_render_sources"] = {"rows": n_src, "wall_ms": round(_wall_ms(before, args.reps), 3)}
    res["render_32x10s"] = off

    # ---- (d) a stream block of 64 sources x 512 samples
    n_src, B = 64, 512
    nb = B // K + 1
    pos, lp = _paths(rng, n_src, nb)
    pos_d, lp_d = torch.from_numpy(pos).to(dev), torch.from_numpy(lp).to(dev)
    blk = torch.from_numpy((rng.standard_normal((n_src, B)) * 0.1).astype(np.float32)).to(dev)
    blocks = {}
    for name, room in (("free_field", None), ("order_1", rooms[1])):
        st = bas.SceneStreamRenderer(tbl, n_src, K, S, fs, max_distance=40.0, room=room, copy_out=False)
        st.prepare(B)
        ms = _wall_ms(lambda: st.process(blk, pos_d, lp_d), 10 * args.reps)
        blocks[name] = {"rows": n_src * st.n_img, "wall_us_per_block": round(ms * 1e3, 1)}
    res["stream_block_64x512"] = blocks

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
