#!/usr/bin/env python3
"""One block of G independent streams: a StreamBatchRenderer against a loop of G StreamRenderers, in one process.

Every renderer is prepared (layout, warm-up, graph capture) before timing and fed device-resident blocks and angles, so
both sides pay the same staging copies.  Per case it reports, as medians over the timed steps:
  * gpu_us: HIP events recorded on the stream before the first and after the last launch of one block (for the loop that
    span includes the gaps the host leaves between the renderers' launches);
  * host_us: host time of the process() calls of one block (no synchronisation inside);
  * wall_us: host time of one block up to a stream synchronisation, and rtf = G B / fs / wall (real-time factor).
With --head both sides are head-tracked: world-frame angles and a device tensor of head orientations
per block (the batch rotates inside its pack launch, each lone renderer with one bas_head_relative_f64 launch).
With --gain both sides take per-source gains at every boundary: a device tensor per block, folded into
the batch's pack launch and into the read plans (no launch more on either side).
Prints one JSON line; --out also writes it to a file.
    python3 tools/bench_stream_batch.py [--steps 50] [--warmup 5] [--case 256x512] [--head] [--gain] [--out profiles/stream_batch_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import binaural_audio_synthesis_amd as bas  # noqa: E402

FS, K, S, L, N_SRC = 44100, 512, 32, 128, 4
CASES = [(1, 512), (16, 512), (64, 512), (256, 512), (16, 8192)]       # (sessions G, block B)


def _time(step, steps, warmup):
    gpu, host, wall = [], [], []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record()
        step()
        t1 = time.perf_counter()
        ev1.record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warmup:
            gpu.append(ev0.elapsed_time(ev1) * 1e3)
            host.append((t1 - t0) * 1e6)
            wall.append((t2 - t0) * 1e6)
    return {"gpu_us": round(statistics.median(gpu), 1), "host_us": round(statistics.median(host), 1),
            "wall_us": round(statistics.median(wall), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--case", action="append", default=None, metavar="GxB",
                    help="only these cases (e.g. 256x512; repeatable); default: all of CASES")
    ap.add_argument("--head", action="store_true", help="head-tracked: world angles + per-boundary head orientations")
    ap.add_argument("--gain", action="store_true", help="per-source gains at every chunk boundary (DESIGN.md §3.10)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_batch.py needs a GPU")
    host = bas.synth.make_table("consistent", 0).truncated(L)
    tbl = bas.irs_and_delaydiffs(host.upsampling, host.diffs_left, host.diffs_right, host.irs_left, host.irs_right)
    rng = np.random.default_rng(0)
    result = {"workload": f"G sessions x {N_SRC} sources, K={K} S={S} L={L}, fs={FS}; one block per step",
              "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "head": args.head, "gain": args.gain,
              "cases": []}
    cases = CASES if args.case is None else [tuple(int(v) for v in c.lower().split("x")) for c in args.case]
    for G, B in cases:
        nb = B // K + 1
        x = torch.from_numpy((rng.standard_normal((G, N_SRC, B)) * 0.1).astype(np.float32)).cuda()
        e = torch.from_numpy(rng.uniform(-0.7, 1.2, (G, N_SRC, nb))).cuda()
        a = torch.from_numpy(rng.uniform(-7, 7, (G, N_SRC, nb))).cuda()
        q = rng.standard_normal((G, nb, 4))
        hd = torch.from_numpy(q / np.linalg.norm(q, axis=-1, keepdims=True)).cuda() if args.head else None
        hg = (lambda g: None) if hd is None else (lambda g: hd[g])
        gn = torch.from_numpy(rng.uniform(0.0, 1.5, (G, N_SRC, nb))).cuda() if args.gain else None
        gg = (lambda g: None) if gn is None else (lambda g: gn[g])
        sb = bas.StreamBatchRenderer(tbl, G, N_SRC, K, S, graph=True, copy_out=False)
        sb.prepare(B)
        batch = _time(lambda: sb.process(x, e, a, head=hd, gain=gn), args.steps, args.warmup)
        loop_r = [bas.StreamRenderer(tbl, N_SRC, K, S, graph=True, copy_out=False) for _ in range(G)]
        for r in loop_r:
            r.prepare(B)

        def loop_step():
            for g, r in enumerate(loop_r):
                r.process(x[g], e[g], a[g], head=hg(g), gain=gg(g))
        loop = _time(loop_step, args.steps, args.warmup)
        # the same block through both: the batch's sessions against the lone renderers (carried state differs only by
        # the number of blocks each has seen, equal here)
        y = sb.process(x, e, a, head=hd, gain=gn).clone()
        diff = max(float((y[g] - r.process(x[g], e[g], a[g], head=hg(g), gain=gg(g))).abs().max()) for g, r in enumerate(loop_r))
        lay = sb.layout(B)
        audio_s = G * B / FS
        row = {"G": G, "n_src": N_SRC, "B": B, "T_in": lay.T_in,
               "kernel": bas._hip.lib().bas_render_fused_kernel_name(N_SRC, lay.T_in, K, S, L).decode(),
               "batch": dict(batch, rtf=round(audio_s / (batch["wall_us"] * 1e-6), 1)),
               "loop": dict(loop, rtf=round(audio_s / (loop["wall_us"] * 1e-6), 1)),
               "wall_speedup": round(loop["wall_us"] / batch["wall_us"], 2), "max_abs_diff_vs_loop": diff}
        result["cases"].append(row)
        del sb, loop_r
        torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
