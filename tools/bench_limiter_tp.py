"""Cost of the true-peak limiter beside the look-ahead limiter of the same build, written to
profiles/limiter_tp_cost.json - a report, not a bar:
  (a) bas.limit on 10 s of stereo at 48 kHz, A = 240, Hd = 960, true_peak=False and true_peak=True alternating;
  (b) a StreamLimiter block of 512 samples, A = 240, Hd = 960, for 1 and for 256 sessions (one launch each), true_peak=False
      and True alternating, as plain calls and as replays of one captured graph.
GPU times are between HIP events around `reps` back-to-back calls after a warm-up call, host work included (a plain call is
bound by the host's launch rate where the kernel is shorter than a launch takes to issue: the graph figure is the GPU's).
Every figure is taken `rounds` times; the json holds the median and the spread (min, max) over the rounds.  The whole
measurement runs `--runs` times (2) in one process, and the file holds every run: compare them for the spread between runs.
Usage: python tools/bench_limiter_tp.py [--reps N] [--rounds R] [--runs K] [--out profiles/limiter_tp_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_limiter import _events_ms, _stats  # noqa: E402


def one_run(args, rng):
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import limiter
    dev = torch.device("cuda")
    c, A, Hd = 0.98, 240, 960
    res = {}

    def loud(shape):
        """Gaussian noise in 10 ms bursts at levels over two decades, about a third of them above the ceiling."""
        n = shape[-2]
        level = 10.0 ** rng.uniform(-1.5, 0.5, size=shape[:-2] + (-(-n // 480),))
        y = rng.standard_normal(shape) * np.repeat(level, 480, axis=-1)[..., :n, None]
        return torch.from_numpy(y.astype(np.float32)).to(dev)

    n = 480000
    y = loud((n, 2))
    outs = {tp: torch.empty_like(y) for tp in (False, True)}
    times = {False: [], True: []}
    for _ in range(args.rounds):
        for tp in (False, True):
            times[tp].append(_events_ms(lambda: bas.limit(y, c, A, Hd, out=outs[tp], true_peak=tp), args.reps))
    tiles = -(-n // limiter.TILE)
    frames = tiles * (limiter.history_tp(A, Hd) + limiter.TILE)            # frames of tile and context the detector forms d for
    med = {tp: sorted(times[tp])[len(times[tp]) // 2] * 1e3 for tp in times}
    res["whole_signal_10s_48k"] = {
        "samples": n, "workgroups": tiles, "limit_us": _stats(times[False]), "limit_true_peak_us": _stats(times[True]),
        "added_us": round(med[True] - med[False], 1), "ratio": round(med[True] / med[False], 3),
        "counted": {"detector_frames": frames, "binary64_fmas": frames * 90, "binary64_fmas_per_frame": 90},
        "true_peak_of_output_over_ceiling": {
            ("true_peak" if tp else "plain"): float(bas.measure(outs[tp], 48000).true_peak) / float(np.float32(c)) - 1.0
            for tp in (False, True)}}

    B, blocks = 512, {}
    for G in (1, 256):
        y = loud((G, B, 2))
        out = torch.empty_like(y)
        yb, ob = (y[0], out[0]) if G == 1 else (y, out)
        plain, graphs = {}, {}
        for tp in (False, True):
            plain[tp], captured = bas.StreamLimiter(G, c, A, Hd, true_peak=tp), bas.StreamLimiter(G, c, A, Hd, true_peak=tp)
            captured.process(yb, out=ob)
            torch.cuda.synchronize()
            graphs[tp] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[tp]):
                captured.process(yb, out=ob)
        t_plain, t_graph = {False: [], True: []}, {False: [], True: []}
        for _ in range(args.rounds):
            for tp in (False, True):
                t_plain[tp].append(_events_ms(lambda: plain[tp].process(yb, out=ob), 10 * args.reps))
                t_graph[tp].append(_events_ms(graphs[tp].replay, 10 * args.reps))
        med = {tp: sorted(t_graph[tp])[len(t_graph[tp]) // 2] * 1e3 for tp in t_graph}
        blocks[f"G_{G}"] = {"sessions": G, "block": B, "launches": 1, "workgroups": G,
                            "plain_us_per_block": _stats(t_plain[False]), "plain_true_peak_us_per_block": _stats(t_plain[True]),
                            "graph_us_per_block": _stats(t_graph[False]), "graph_true_peak_us_per_block": _stats(t_graph[True]),
                            "added_us_per_block_graph": round(med[True] - med[False], 1)}
    res["stream_block_512"] = blocks
    return res


def main():
    import torch
    from binaural_audio_synthesis_amd import limiter
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limiter_tp_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_limiter_tp.py needs a GPU")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "ceiling": 0.98, "lookahead": 240,
           "hold": 960, "tile": limiter.TILE, "runs": [one_run(args, np.random.default_rng(0)) for _ in range(args.runs)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
