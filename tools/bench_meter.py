"""Cost of the loudness and true-peak meter, written to profiles/meter_cost.json:
  (a) 10 s of stereo at 48 kHz: the entry alone (bas_meter_f32 with its buffers made once: three launches - every unit's
      end state from rest, the chain, the energies) and bas.measure as a user calls it (buffers, the entry, the readings in
      float64 torch ops), beside bas.limit on the same signal in the same process, alternating;
  (b) a StreamMeter block of 512 samples for 1 and for 256 sessions (one launch), as plain calls and as replays of one
      captured graph, beside a StreamLimiter block of the same shape, alternating.
GPU times are between HIP events around `reps` back-to-back calls after a warm-up call, host work included (a plain call is
bound by the host's launch rate where the kernel is shorter than a launch takes to issue: the graph figure is the GPU's).
Every figure is taken `rounds` times, alternating between the things compared; the json holds the median and the spread
(min, max) over the rounds.  Run the command twice and compare the files for the spread between runs.
Where the time goes inside the three launches is the kernel trace's to say (--trace-run: a short run of (a) and (b) for
`rocprofv3 --kernel-trace --stats -- python tools/bench_meter.py --trace-run`, which also shows every launch's grid): the
first launch is a staging pass, the runs from rest and the scan; the third is those again plus the true peak, the second
pass and the reduction; what the two-pass form costs over one pass is the first launch, the chain, and the first launch's
share of the third.
Usage: python tools/bench_meter.py [--reps N] [--rounds R] [--trace-run] [--out profiles/meter_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import loudness
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-run", action="store_true", help="a few calls of each shape and no timing: for a kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "meter_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_meter.py needs a GPU")
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    fs, hop = 48000, 4800
    c, A, Hd = 0.98, 240, 960
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "fs": fs}

    def loud(shape):
        """Gaussian noise in 10 ms bursts at levels over two decades."""
        n = shape[-2]
        level = 10.0 ** rng.uniform(-2.5, -0.5, size=shape[:-2] + (-(-n // 480),))
        y = rng.standard_normal(shape) * np.repeat(level, 480, axis=-1)[..., :n, None]
        return torch.from_numpy(y.astype(np.float32)).to(dev)

    # ---- (a) 10 s at 48 kHz
    n = 480000
    y = loud((n, 2))
    y3 = y.unsqueeze(0)
    energy = torch.zeros((1, 2, n // hop), dtype=torch.float64, device=dev)
    tp = torch.zeros((1, 2), dtype=torch.float32, device=dev)
    ws = loudness._workspace(1, n, fs, dev)
    out = torch.empty_like(y)

    def entry():
        loudness._launch(y3, 1, n, fs, energy, 0, None, tp, ws)

    def whole():
        return bas.measure(y, fs)

    def limit():
        bas.limit(y, c, A, Hd, out=out)

    # ---- (b) blocks of 512
    B = 512
    streams = {}
    for G in (1, 256):
        yb = loud((G, B, 2))
        ob = torch.empty_like(yb)
        yv, ov = (yb[0], ob[0]) if G == 1 else (yb, ob)
        # an hour per session: the timed blocks never fill the buffer (the replays move only the device's count)
        meter, cap = bas.StreamMeter(G, fs, max_seconds=3600.0), bas.StreamMeter(G, fs, max_seconds=3600.0)
        lim, lcap = bas.StreamLimiter(G, c, A, Hd), bas.StreamLimiter(G, c, A, Hd)
        cap.process(yv)
        lcap.process(yv, out=ov)
        torch.cuda.synchronize()
        g_meter, g_lim = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g_meter):
            cap.process(yv)
        with torch.cuda.graph(g_lim):
            lcap.process(yv, out=ov)

        def plain(meter=meter, yv=yv):
            meter.process(yv)
            if meter._count[0] > 3000 * fs:                                # (plain calls keep the host's count: start again)
                meter.reset()
        streams[G] = dict(plain=plain, graph=g_meter.replay, lim_plain=lambda lim=lim, yv=yv, ov=ov: lim.process(yv, out=ov),
                          lim_graph=g_lim.replay, cap=cap)

    if args.trace_run:
        for fn in (entry, whole, limit):
            for _ in range(3):
                fn()
        for G in streams:
            for k in ("plain", "graph", "lim_plain", "lim_graph"):
                for _ in range(3):
                    streams[G][k]()
        torch.cuda.synchronize()
        print("trace run done")
        return

    t = {k: [] for k in ("entry", "whole", "limit")}
    for _ in range(args.rounds):
        t["entry"].append(_events_ms(entry, args.reps))
        t["whole"].append(_events_ms(whole, args.reps))
        t["limit"].append(_events_ms(limit, args.reps))
    units = n // hop
    m = whole()
    res["whole_signal_10s_48k"] = {
        "samples": n, "units_per_ear": units, "launches": 3, "workgroups_per_unit_launch": 2 * units,
        "entry_us": _stats(t["entry"]), "measure_us": _stats(t["whole"]), "limit_us_same_signal": _stats(t["limit"]),
        "counted": {"bytes_read": 2 * n * 8, "cascade_steps_binary64": 2 * 2 * n, "true_peak_fma_binary64": 2 * n * 36},
        "integrated_lufs": float(m.integrated), "true_peak_dbtp": float(m.true_peak_db)}

    blocks = {}
    for G, s in streams.items():
        tt = {k: [] for k in ("plain", "graph", "lim_plain", "lim_graph")}
        for _ in range(args.rounds):
            for k in tt:
                if k == "graph":
                    s["cap"].reset()                                        # (10 reps x 512 samples x rounds stay far below the hour)
                tt[k].append(_events_ms(s[k], 10 * args.reps))
        blocks[f"G_{G}"] = {"sessions": G, "block": B, "launches": 1, "workgroups": 2 * G,
                            "meter_plain_us_per_block": _stats(tt["plain"]), "meter_graph_us_per_block": _stats(tt["graph"]),
                            "limiter_plain_us_per_block": _stats(tt["lim_plain"]),
                            "limiter_graph_us_per_block": _stats(tt["lim_graph"])}
    res["stream_block_512"] = blocks

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
