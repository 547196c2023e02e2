"""Cost of the look-ahead limiter, written to profiles/limiter_cost.json:
  (a) bas.limit on 10 s of stereo at 48 kHz, A = 240, Hd = 960 (one launch), beside the same definition composed from torch
      pooling ops in the same process and alternating with it (max_pool1d on -r, avg_pool1d: what a user could do before
      this entry existed; float32 throughout, so its sum is not the mirror's), with the largest difference between the two;
  (b) a StreamLimiter block of 512 samples, A = 240, Hd = 960, for 1 and for 256 sessions (one launch: a block of at most
      one tile moves its state forward itself), as plain calls and as replays of one captured graph, beside the block
      renders it follows (the README's 28 us for one real-time block of StreamRenderer, 69.5 us for 256 sessions of
      StreamBatchRenderer: quoted, not run).
GPU times are between HIP events around `reps` back-to-back calls after a warm-up call, host work included (a plain call
is bound by the host's launch rate where the kernel is shorter than a launch takes to issue: the graph figure is the
GPU's).  Every figure is taken `rounds` times, alternating between the things compared; the json holds the median and the
spread (min, max) over the rounds.  Run the command twice and compare the files for the spread between runs.
Usage: python tools/bench_limiter.py [--reps N] [--rounds R] [--only whole|stream] [--out profiles/limiter_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RENDER_US = {1: 28.0, 256: 69.5}                           # README: the block renders a limiter block follows


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


def _stats(values, scale=1e3, digits=1):
    v = sorted(values)
    return {"median": round(v[len(v) // 2] * scale, digits), "min": round(v[0] * scale, digits),
            "max": round(v[-1] * scale, digits)}


def torch_limit(y, c, A, Hd):
    """The definition on y [n, 2] from torch ops, float32 throughout."""
    import torch
    import torch.nn.functional as F
    m = y.abs().amax(dim=1)
    r = torch.where(m > c, c / m, torch.ones_like(m))
    rp = F.pad(r[None, None], (A + Hd, A), value=1.0)
    e = -F.max_pool1d(-rp, Hd + A + 1, stride=1)
    s = F.avg_pool1d(e, A + 1, stride=1)[0, 0]
    return (y * torch.minimum(s, r)[:, None]).clamp(-c, c)


def main():
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import limiter
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("whole", "stream"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "limiter_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_limiter.py needs a GPU")
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    c, A, Hd = 0.98, 240, 960
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "ceiling": c, "lookahead": A,
           "hold": Hd, "tile": limiter.TILE}

    def loud(shape):
        """Gaussian noise in 10 ms bursts at levels over two decades, about a third of them above the ceiling."""
        n = shape[-2]
        level = 10.0 ** rng.uniform(-1.5, 0.5, size=shape[:-2] + (-(-n // 480),))
        y = rng.standard_normal(shape) * np.repeat(level, 480, axis=-1)[..., :n, None]
        return torch.from_numpy(y.astype(np.float32)).to(dev)

    # ---- (a) 10 s at 48 kHz, ours and the pooling composition, alternating
    if args.only in (None, "whole"):
        n = 480000
        y = loud((n, 2))
        out = torch.empty_like(y)
        c32 = float(np.float32(c))

        def ours():
            bas.limit(y, c, A, Hd, out=out)

        def pooled():
            return torch_limit(y, c32, A, Hd)
        ref = pooled()
        ours()
        t_ours, t_pool = [], []
        for _ in range(args.rounds):
            t_ours.append(_events_ms(ours, args.reps))
            t_pool.append(_events_ms(pooled, args.reps))
        tiles = -(-n // limiter.TILE)
        H = limiter.history(A, Hd)
        res["whole_signal_10s_48k"] = {
            "samples": n, "workgroups": tiles, "limit_us": _stats(t_ours), "torch_pooling_us": _stats(t_pool),
            "counted": {"bytes_read": tiles * (H + 2 * limiter.TILE) * 8, "bytes_written": n * 8,
                        "binary64_adds": n * (A + 1), "divisions": tiles * (H + 2 * limiter.TILE)},
            "max_difference_from_pooling": float((out - ref).abs().max()), "peak_in": float(y.abs().max()),
            "peak_out": float(out.abs().max())}

    # ---- (b) a stream block of 512 samples for 1 and 256 sessions: plain calls, and one captured graph replayed
    if args.only in (None, "stream"):
        B = 512
        blocks = {}
        for G in (1, 256):
            y = loud((G, B, 2))
            out = torch.empty_like(y)
            plain, captured = bas.StreamLimiter(G, c, A, Hd), bas.StreamLimiter(G, c, A, Hd)
            yb, ob = (y[0], out[0]) if G == 1 else (y, out)
            captured.process(yb, out=ob)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                captured.process(yb, out=ob)
            t_plain, t_graph = [], []
            for _ in range(args.rounds):
                t_plain.append(_events_ms(lambda: plain.process(yb, out=ob), 10 * args.reps))
                t_graph.append(_events_ms(graph.replay, 10 * args.reps))
            med = sorted(t_graph)[len(t_graph) // 2] * 1e3
            blocks[f"G_{G}"] = {"sessions": G, "block": B, "launches": 1, "workgroups": G * -(-B // limiter.TILE),
                                "plain_us_per_block": _stats(t_plain), "graph_us_per_block": _stats(t_graph),
                                "render_us_per_block_readme": RENDER_US[G],
                                "added_over_render": round(med / RENDER_US[G], 3)}
        res["stream_block_512"] = blocks

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
