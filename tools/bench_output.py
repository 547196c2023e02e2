"""Cost of the stereo output filter, written to profiles/output_bench.json:
  (a) the real-time block: 256 sessions x 512 frames, each session with its own taps, at M = 512 diagonal and at M = 1024
      full - as a stream block is launched (bas_output_filter_f32 on [history | block]: one launch, 256 workgroups), and the
      whole StreamOutputFilter.process() around it (the block's copy into the window, the filter, the carry);
  (b) 64 signals x 10 s at 48 kHz, M = 2048 full, whole signals.
Each is timed between HIP events around `reps` back-to-back replays of one captured graph after a warm-up; every figure is
taken `rounds` times and the json holds the median and the spread (min, max) over the rounds.
Beside each time: the binary64 multiply-adds of the call (sessions x outputs x 2 channels x taps read per channel) over the
time as a fraction of the vector peak, and the bytes it must move (window in, outputs out, the taps once) over the time as a
fraction of the HBM peak, with the peaks used.  Neither is a kernel-trace figure: the times are event times of the call.
Usage: python tools/bench_output.py [--reps N] [--rounds R] [--only block|long] [--out profiles/output_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12              # bytes / s (MI355X HBM3E, specified)
FMA64_PEAK = 39.3e12           # binary64 multiply-adds / s on the vector units (78.6 TFLOP/s specified)
RENDER_BLOCK_US = 28.0         # the render block this stage follows (256 sessions x 512 frames)


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


def _stats(values, scale=1e3, digits=2):
    v = sorted(values)
    return {"median": round(v[len(v) // 2] * scale, digits), "min": round(v[0] * scale, digits),
            "max": round(v[-1] * scale, digits)}


def _graph(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def main():
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import output
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("block", "long"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "output_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_output.py needs a GPU")
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "tile": output.TILE,
           "hbm_peak_bytes_per_s": HBM_PEAK, "binary64_fma_peak_per_s": FMA64_PEAK}

    def taps(G, M, full):
        t = rng.standard_normal((G, 2, 2, M) if full else (G, 2, M)) * np.exp(-np.arange(M) / (M / 6.0))
        return bas.OutputFilter(t, per_session=True)

    def counted(G, T_win, T_out, M, full):
        return {"sessions": G, "window_frames": T_win, "output_frames": T_out, "taps": M, "form": "full" if full else "diagonal",
                "workgroups": G * -(-T_out // output.TILE), "bytes": 4 * (G * 2 * (T_win + T_out) + G * (4 if full else 2) * M),
                "binary64_multiply_adds": G * T_out * 2 * (2 if full else 1) * M}

    def report(times_ms, c, extra=None):
        g = sorted(times_ms)[len(times_ms) // 2] * 1e-3                                    # seconds
        r = {"graph_us": _stats(times_ms), "counted": c, "fma64_fraction_of_peak": round(c["binary64_multiply_adds"] / g / FMA64_PEAK, 4),
             "hbm_fraction_of_peak": round(c["bytes"] / g / HBM_PEAK, 4)}
        r.update(extra or {})
        return r

    if args.only in (None, "block"):
        G, B = 256, 512
        blocks = {}
        for name, M, full in (("diagonal_512", 512, False), ("full_1024", 1024, True)):
            s = bas.StreamOutputFilter(taps(G, M, full), n_sessions=G)
            y = torch.from_numpy(rng.standard_normal((G, B, 2)).astype(np.float32)).to(dev)
            out = torch.empty((G, B, 2), dtype=torch.float32, device=dev)
            s.process(y, out=out)
            H = s.history

            def kernel(s=s, out=out, H=H):
                output._launch(s._window(H + B), H + B, H, s._taps, s._set, s.M, s.full, out)

            def process(s=s, y=y, out=out):
                s.process(y, out=out)
            blocks[name] = (_graph(kernel), _graph(process), counted(G, H + B, B, M, full))
        times = {k: ([], []) for k in blocks}
        for _ in range(args.rounds):
            for k, (kernel, process, _) in blocks.items():
                times[k][0].append(_events_ms(kernel, 10 * args.reps))
                times[k][1].append(_events_ms(process, 10 * args.reps))
        res["real_time_block_256x512"] = {"render_block_us": RENDER_BLOCK_US}
        for k, (_, _, c) in blocks.items():
            res["real_time_block_256x512"][k] = report(times[k][0], c, {"process_graph_us": _stats(times[k][1])})

    if args.only in (None, "long"):
        G, n, M = 64, 480000, 2048
        f = taps(G, M, True)
        y = torch.from_numpy(rng.standard_normal((G, n, 2)).astype(np.float32)).to(dev)
        out = torch.empty((G, n + M - 1, 2), dtype=torch.float32, device=dev)
        replay = _graph(lambda: bas.filter_output(y, f, out=out))
        times = [_events_ms(replay, max(1, args.reps // 10)) for _ in range(args.rounds)]
        res["whole_64_signals_10s"] = {"full_2048": report(times, counted(G, n, n + M - 1, M, True))}

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
