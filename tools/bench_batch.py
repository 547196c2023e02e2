#!/usr/bin/env python3
"""Batched independent renders against a loop of single renders, in one process, timed with HIP events.

B mono 10-s clips at 44.1 kHz, K 512 / S 32 / L 128, each on its own trajectory; an equal-length batch and a ragged one
(lengths 5-10 s).  The batch reports pack, render and finish separately (events between the three stages of
batch.render_batch) and the whole call; the loop is make_signal_move_2d(vectorized=True) on device tensors, once per item.
Prints one JSON line.     python3 tools/bench_batch.py [--items 256] [--steps 10] [--warmup 3] [--loop-steps 2]"""
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
from binaural_audio_synthesis_amd import batch  # noqa: E402

FS, K, S, L = 44100, 512, 32, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loop-steps", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch.py needs a GPU")
    host = bas.synth.make_table("consistent", 0).truncated(L)
    tbl = bas.irs_and_delaydiffs(host.upsampling, host.diffs_left, host.diffs_right, host.irs_left, host.irs_right)
    B, N = args.items, int(args.seconds * FS)
    rng = np.random.default_rng(0)
    x = ((rng.random((B, N), dtype=np.float32) * 2 - 1) * 0.05).astype(np.float32)
    fns = [bas.synth.trajectory("spiral" if b % 2 == 0 else "circle_askew", period_s=2.0 + b / 64.0,
                                length_s=args.seconds, turns=5.0, phase=2 * np.pi * b / B) for b in range(B)]
    ragged = rng.integers(N // 2, N + 1, B)
    ragged[0] = N
    x_dev = torch.from_numpy(x).cuda()
    result = {"workload": f"{B} mono clips x {args.seconds:g} s @ {FS} Hz, K={K} S={S} L={L}",
              "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup}

    def angles(lengths):
        n_q = -(-int(max(lengths)) // K) + 1
        ea = np.empty((2, B, n_q))
        for b, (f, n) in enumerate(zip(fns, lengths)):
            _, e, a = batch.sample_trajectory(f, int(n), K, L)
            ea[0, b, :e.size], ea[1, b, :a.size] = e, a
            ea[:, b, e.size:] = ea[:, b, e.size - 1:e.size]
        return torch.from_numpy(ea).cuda()

    for name, lengths in (("equal", np.full(B, N)), ("ragged", ragged)):
        ea = angles(lengths)
        lens = None if name == "equal" else lengths
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        stages = {"pack": [], "render": [], "finish": [], "total": []}
        host_ms = []
        for step in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out, out_len, peaks = bas.render_batch(x_dev, K, S, ea[0], ea[1], tbl, lengths=lens, events=ev)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if step >= args.warmup:
                stages["pack"].append(ev[0].elapsed_time(ev[1]))
                stages["render"].append(ev[1].elapsed_time(ev[2]))
                stages["finish"].append(ev[2].elapsed_time(ev[3]))
                stages["total"].append(ev[0].elapsed_time(ev[3]))
                host_ms.append((t1 - t0) * 1e3)
        lay = batch.plan_layout(lengths, K, S, L)
        pack_bytes = 4 * (B * N + lay.T_in) + 8 * 2 * 2 * lay.n_q
        result[name] = {"ms_median": {k: round(statistics.median(v), 4) for k, v in stages.items()},
                        "host_wall_ms_median": round(statistics.median(host_ms), 3),
                        "T_in": lay.T_in, "renders": len(batch.split_items(lengths, K, L)),
                        "pack_GBps": round(pack_bytes / (statistics.median(stages["pack"]) * 1e-3) / 1e9, 1),
                        "zero_copy_view": not out.transpose(1, 2).is_contiguous()}
        # the loop of single renders, same items, same trajectories (each item's own call; device tensors in and out)
        loop_ms, loop_host = [], []
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        worst = 0.0
        for step in range(1 + args.loop_steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            singles = [bas.make_signal_move_2d(x_dev[b, :int(lengths[b])], K, S, fns[b], tbl, vectorized=True)
                       for b in range(B)]
            e1.record()
            torch.cuda.synchronize()
            if step:
                loop_ms.append(e0.elapsed_time(e1))
                loop_host.append((time.perf_counter() - t0) * 1e3)
        for b in (0, B // 2, B - 1):
            n = int(out_len[b])
            d = (out[b, :n] - singles[b]).abs().max().item() / max(singles[b].abs().max().item(), 1e-30)
            worst = max(worst, d)
        result[name]["loop_ms_median"] = round(statistics.median(loop_ms), 3)
        result[name]["loop_host_wall_ms_median"] = round(statistics.median(loop_host), 3)
        result[name]["speedup_vs_loop"] = round(statistics.median(loop_ms) / statistics.median(stages["total"]), 2)
        result[name]["max_rel_diff_vs_loop_items_0_mid_last"] = worst
    print(json.dumps(result))


if __name__ == "__main__":
    main()
