"""Cost of the sample-rate converter, written to profiles/rate_bench.json:
  (a) one real-time block: 256 rows, 512 outputs, 44100 -> 48000 and 48000 -> 44100, as a stream block is launched
      (bas_rate_convert_f32 on [history | block] in the middle of a stream: one launch, 256 workgroups);
  (b) 256 rows x 10 s, both directions, whole signals.
Each is one bas_rate_convert_f32 call with fixed arguments, timed between HIP events around `reps` back-to-back calls after a
warm-up call - as plain calls (host work included: a call shorter than a launch takes to issue is bound by the host) and as
replays of one captured graph of that call (the GPU's figure; a benchmark may capture the call because its counts are fixed,
a stream may not).  Every figure is taken `rounds` times, the two directions alternating; the json holds the median and the
spread (min, max) over the rounds.
Beside each time: the bytes the call must move (window in, outputs out, the tap table once) over the time as a fraction of the
HBM peak, and its binary64 multiply-adds (rows x outputs x N) over the time as a fraction of the vector peak, with the peaks
used.  Neither is a kernel-trace figure: the times are event times of the call.
Usage: python tools/bench_rate.py [--reps N] [--rounds R] [--only block|long] [--out profiles/rate_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12              # bytes / s (MI355X HBM3E, specified)
FMA64_PEAK = 78.6e12 / 2       # binary64 multiply-adds / s on the vector units (78.6 TFLOP/s specified)


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


def main():
    import torch
    from binaural_audio_synthesis_amd import rate
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("block", "long"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rate_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rate.py needs a GPU")
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    rows = 256
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "rows": rows, "tile": rate.TILE,
           "hbm_peak_bytes_per_s": HBM_PEAK, "binary64_fma_peak_per_s": FMA64_PEAK}

    def case(fs_in, fs_out, M, stream_block):
        """The call's closure, its graph and what it counts."""
        d = rate.design(fs_in, fs_out)
        if stream_block:                                   # block 100 of a stream that hands out M outputs per block
            m0 = 100 * M
            n_before, n_after = rate.needed(m0, d.p, d.q, d.K0), rate.needed(m0 + M, d.p, d.q, d.K0)
            H = rate.history(d.N)
            t0, T_win = n_before - H, H + n_after - n_before
        else:
            m0, t0 = 0, 0
            T_win = M * d.q // d.p
            M = d.out_length(T_win)
        x = torch.from_numpy(rng.standard_normal((1, rows, T_win)).astype(np.float32)).to(dev)
        out = torch.empty((1, rows, M), dtype=torch.float32, device=dev)

        def call():
            rate._launch(x, T_win, t0, d, out, m0)
        call()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        counted = {"inputs_per_row": T_win, "outputs_per_row": M, "taps_per_output": d.N, "workgroups": rows * -(-M // rate.TILE),
                   "bytes": 4 * (rows * (T_win + M) + d.p * d.N), "binary64_multiply_adds": rows * M * d.N}
        return call, graph.replay, counted

    def measure(name, M, stream_block, reps):
        cases = {f"{a}_to_{b}": case(a, b, M, stream_block) for a, b in ((44100, 48000), (48000, 44100))}
        times = {k: {"plain": [], "graph": []} for k in cases}
        for _ in range(args.rounds):
            for k, (call, replay, _) in cases.items():
                times[k]["plain"].append(_events_ms(call, reps))
                times[k]["graph"].append(_events_ms(replay, reps))
        res[name] = {}
        for k, (_, _, counted) in cases.items():
            g = sorted(times[k]["graph"])[len(times[k]["graph"]) // 2] * 1e-3          # seconds
            res[name][k] = {"plain_us": _stats(times[k]["plain"]), "graph_us": _stats(times[k]["graph"]), "counted": counted,
                            "hbm_fraction_of_peak": round(counted["bytes"] / g / HBM_PEAK, 4),
                            "fma64_fraction_of_peak": round(counted["binary64_multiply_adds"] / g / FMA64_PEAK, 4)}

    if args.only in (None, "block"):
        measure("real_time_block_256x512", 512, True, 10 * args.reps)
    if args.only in (None, "long"):
        measure("whole_256_rows_10s", 480000, False, args.reps)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
