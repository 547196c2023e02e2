"""Cost of screens, written to profiles/occlusion_bench.json:
  (a) the scene kernel on §3.18's shape - 256 sources x 7 or 25 images x 87 boundaries, 6 bands (one second of chunks of
      512), orders 1 and 2 - with 0, 1, 4 and 16 screens, beside the count of crossed copies that explains the time;
  (b) one SceneStreamRenderer block of 256 sources x 512 samples in a banded order-1 room, with and without 4 screens
      (graph replay);
  (c) with --parent DIR (another checkout of this project, built): the 0-screen figures of (a) and (b) from that checkout
      too, the two taken in turns on the same machine (--rounds of them), both recorded.
Every GPU step runs in a child process of its own under `timeout`, one after the other; the first that fails ends the run
(nothing is started on a device after a fault).
Usage: python tools/bench_occlusion.py [--reps N] [--rounds N] [--parent DIR] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STEPS = {"kernel": 300, "stream": 300, "kernel0": 240, "stream0": 240}   # name -> time limit in seconds
BANDS = (125.0, 250.0, 500.0, 1000.0, 2000.0, 4000.0)
CARPET = np.array([0.99, 0.97, 0.93, 0.80, 0.65, 0.55])
PANEL = np.array([0.80, 0.88, 0.93, 0.95, 0.96, 0.96])
WALLS = np.stack([CARPET, PANEL, PANEL, CARPET, CARPET ** 0.5, PANEL])
SIZE = np.array([6.0, 5.0, 4.0])
FS = 44100.0


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


def _screens(scene, n):
    """n upright screens about a metre wide and two high, spread over the room, half of them letting some sound through."""
    rng = np.random.default_rng(40 + n)
    c = np.stack([rng.uniform(1.2, 4.8, n), rng.uniform(1.2, 3.8, n), np.full(n, 1.1)], axis=1)
    yaw = rng.uniform(0, np.pi, n)
    e1 = 0.6 * np.stack([np.cos(yaw), np.sin(yaw), np.zeros(n)], axis=1)
    e2 = np.tile([0.0, 0.0, 1.0], (n, 1))
    T = np.where((np.arange(n) % 2 == 0)[:, None], 0.0, np.array([0.5, 0.4, 0.3, 0.2, 0.1, 0.05]))
    return scene.Screens(c, e1, e2, T)


def _table(bas):
    tb = bas.synth.make_table("consistent", 0, upsampling=8).truncated(128)
    return bas.irs_and_delaydiffs(tb.upsampling, tb.diffs_left, tb.diffs_right, tb.irs_left, tb.irs_right)


def _crossings(scene, pos, lp, room, screens, sample):
    """Crossed copies per (row, boundary) item, counted on the host over the first `sample` sources: (mean, share of the
    items with at least one)."""
    p = pos[:sample]
    m = room.images[:, None, :]
    q = m * room.size + np.where(m % 2 != 0, room.size - p[:, None], p[:, None])       # (sample, n_img, nb, 3): at rest
    cells = np.abs(m)
    count = np.zeros(q.shape[:-1], dtype=int)
    for k in range(screens.n):
        for ia in range(int(cells[..., 0].max()) + 1):
            for ja in range(int(cells[..., 1].max()) + 1):
                for ka in range(int(cells[..., 2].max()) + 1):
                    here = (ia <= cells[..., 0]) & (ja <= cells[..., 1]) & (ka <= cells[..., 2])
                    cell = np.where(m < 0, -1, 1) * np.array([ia, ja, ka])
                    odd = cell % 2 != 0
                    c = cell * room.size + np.where(odd, room.size - screens.centre[k], screens.centre[k])
                    e1, e2 = np.where(odd, -screens.half_u[k], screens.half_u[k]), np.where(odd, -screens.half_v[k], screens.half_v[k])
                    count += here & scene.screen_sides(q, lp, c, e1, e2)
    return float(count.mean()), float((count > 0).mean())


def step_kernel(reps, with_screens=True):
    """(a): the scene kernel alone, outputs allocated once."""
    import torch
    from binaural_audio_synthesis_amd import scene
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    n_src, nb = 256, 87
    pos_h, orient_h = _paths(rng, n_src, nb)
    lp_h = np.tile(SIZE / 2 + [0.3, -0.2, -0.4], (nb, 1))
    pos, orient, lp = (torch.from_numpy(a).to(dev) for a in (pos_h, orient_h, lp_h))
    res = {"device": torch.cuda.get_device_name(0), "sources": n_src, "boundaries": nb, "bands": len(BANDS)}
    for order in (1, 2):
        room = scene.Room(SIZE, beta=WALLS, order=order, bands=BANDS, taps=32)
        rows = n_src * room.n_img
        out = tuple(torch.empty((rows, nb), dtype=torch.float64, device=dev) for _ in range(4)) + \
            (torch.empty((rows, nb, len(BANDS)), dtype=torch.float64, device=dev),)
        r = {"items": rows * nb}
        r["no_bands_us"] = round(_events_ms(
            lambda: scene.scene_params_device(pos, FS, lp, room=room, chunksize=512, out=out[:4]), reps) * 1e3, 1)
        for n in (0, 1, 4, 16) if with_screens else (0,):
            kw = {} if n == 0 else dict(screens=_screens(scene, n))
            col = scene.SceneColor(BANDS, taps=32, air=True, directivity=np.full(6, 0.5), **kw)
            us = _events_ms(lambda: scene.scene_color_params_device(pos, FS, lp, room=room, chunksize=512, color=col,
                                                                    orient=orient, out=out), reps) * 1e3
            r[f"screens_{n}"] = {"us": round(us, 1)}
            if n:
                mean, share = _crossings(scene, pos_h, lp_h, room, col.screens, 16)
                copies = float(np.prod(np.abs(room.images) + 1, axis=1).mean()) * n
                r[f"screens_{n}"].update(copies_tested_per_item=round(copies, 2), copies_crossed_per_item=round(mean, 3),
                                         items_with_a_crossing=round(share, 3),
                                         ns_per_crossed_copy_and_band=round(
                                             (us - r["screens_0"]["us"]) * 1e3 / max(mean * rows * nb * len(BANDS), 1), 3))
        res[f"order_{order}"] = r
    res["note"] = ("device events around the Python call (validation and one launch), outputs allocated once; crossings "
                   "counted on the host over 16 of the sources, at rest")
    return res


def step_stream(reps, with_screens=True):
    """(b): one block of a SceneStreamRenderer, graph replay."""
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import scene
    rng = np.random.default_rng(1)
    dev = torch.device("cuda")
    n_src, K, B = 256, 512, 512
    tbl = _table(bas)
    room = scene.Room(SIZE, beta=WALLS, order=1, bands=BANDS, taps=32)
    blk = torch.from_numpy(rng.standard_normal((n_src, B)).astype(np.float32)).to(dev)
    pos, orient = _paths(rng, n_src, 2)
    pos, orient = torch.from_numpy(pos).to(dev), torch.from_numpy(orient).to(dev)
    res = {}
    for name, n in (("screens_0", 0), ("screens_4", 4)) if with_screens else (("screens_0", 0),):
        kw = {} if n == 0 else dict(screens=_screens(scene, n))
        col = scene.SceneColor(BANDS, taps=32, air=True, directivity=np.full(6, 0.5), **kw)
        st = bas.SceneStreamRenderer(tbl, n_src, K, 32, FS, max_distance=30.0, room=room, graph=True, copy_out=False, color=col)
        st.prepare(B)

        def one():
            st.process(blk, pos, orient=orient)
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


def _child(step, reps, root):
    """One step in a process of its own, importing the package from `root`; its result, or the end of the run."""
    cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
           "--reps", str(reps), "--root", root]
    p = subprocess.run(cmd, capture_output=True, text=True)
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"step {step} ({root}) failed with exit status {p.returncode}: nothing more is started")
    return json.loads(lines[0][len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3, help="(c): how often the two builds take turns")
    ap.add_argument("--parent", default=None, help="(c): a built checkout of the parent commit")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "occlusion_bench.json"))
    ap.add_argument("--step", choices=sorted(STEPS), help="run one GPU step in this process and print its JSON")
    ap.add_argument("--root", default=HERE, help="with --step: the checkout whose package is measured")
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, os.path.abspath(args.root))
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU: nothing is measured without one")
        fn = {"kernel": step_kernel, "stream": step_stream, "kernel0": lambda r: step_kernel(r, False),
              "stream0": lambda r: step_stream(r, False)}[args.step]
        print("RESULT " + json.dumps(fn(args.reps)))
        return
    res = {"scene_kernel_256x87": _child("kernel", args.reps, HERE),
           "scene_stream_256x512_order1": _child("stream", args.reps, HERE)}
    if args.parent:
        turns = {"this": [], "parent": []}
        for _ in range(args.rounds):
            for name, root in (("this", HERE), ("parent", os.path.abspath(args.parent))):
                k, s = _child("kernel0", args.reps, root), _child("stream0", args.reps, root)
                turns[name].append({"kernel_order_1_no_bands_us": k["order_1"]["no_bands_us"],
                                    "kernel_order_1_bands_us": k["order_1"]["screens_0"]["us"],
                                    "kernel_order_2_no_bands_us": k["order_2"]["no_bands_us"],
                                    "kernel_order_2_bands_us": k["order_2"]["screens_0"]["us"],
                                    "stream_block_gpu_us": s["screens_0"]["gpu_us_per_block"]})
        med = {n: {key: float(np.median([t[key] for t in ts])) for key in ts[0]} for n, ts in turns.items()}
        res["existing_paths_against_parent"] = {
            "turns": turns, "median": med,
            "this_over_parent": {key: round(med["this"][key] / med["parent"][key], 4) for key in med["this"]}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
