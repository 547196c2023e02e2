"""Cost of late reverberation, written to profiles/reverb_cost.json:
  (a) a whole-signal reverb.long_fir_device of 10 s at 48 kHz (one bus) through tails of 24 000 and 65 536 taps, Np = 512,
      per call (three launches), with the bytes and flop counted from the shapes;
  (b) beside it, in the same process and alternating with it, the full-length torch.fft.rfft / irfft convolution of the
      same tensors (what a user could do before this entry existed; the tail's spectrum precomputed, as ours is);
  (c) a 64-source x 512-sample SceneStreamRenderer block with an order-1 room, with and without late= at Lr = 24 000
      (graph replay; wall time per block and GPU time between events), and the difference per launch added.
GPU times are between HIP events around `reps` back-to-back calls after a warm-up call; wall times are time.perf_counter
around the same loop with a device synchronisation at its end, host work included.  Every figure is taken `rounds` times,
alternating between the things compared; the json holds the median and the spread (min, max) over the rounds.  Run the
command twice and compare the files for the spread between runs.
Usage: python tools/bench_reverb.py [--reps N] [--rounds R] [--out profiles/reverb_cost.json]"""
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


def _stats(values, scale=1e3, digits=1):
    v = sorted(values)
    return {"median": round(v[len(v) // 2] * scale, digits), "min": round(v[0] * scale, digits),
            "max": round(v[-1] * scale, digits)}


def counted(T_out, Lr, Np, n_bus=1):
    """Flop and bytes of one bas_long_fir_f32 call, from the shapes (the algorithm's, not the hardware's: every global
    load and store counted once, whether L2 serves it or HBM).  A radix-2 transform of N complex points is
    (N/2) log2 N butterflies of 10 flop; a bin's partition step is two complex multiply-adds of 8 flop."""
    N, nb = 2 * Np, Np + 1
    F, P = -(-T_out // Np), -(-Lr // Np)
    fft = (N // 2) * int(np.log2(N)) * 10
    flop = n_bus * ((F + P - 1) * fft + F * nb * P * 16 + F * fft + 2 * F * Np)
    FB = 1 if F < 4 else 8
    x_b, y_b = n_bus * (F + P - 1) * nb * 8, n_bus * F * 2 * nb * 8
    by = {"forward": n_bus * (F + P - 1) * N * 4 + x_b,
          "mac": n_bus * -(-F // FB) * nb * (P * 16 + (P + FB - 1) * 8) + y_b,
          "inverse": y_b + n_bus * F * Np * 2 * 4}
    return {"frames": F, "partitions": P, "flop": int(flop), "bytes": {k: int(v) for k, v in by.items()},
            "bytes_total": int(sum(by.values()))}


def main():
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import reverb, scene
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reverb_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reverb.py needs a GPU")
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds}
    fs, Np = 48000.0, 512

    # ---- (a), (b): 10 s through a long tail, ours and the full-length FFT, alternating
    T = int(10 * fs)
    bus = torch.from_numpy((rng.standard_normal((1, T)) * 0.1).astype(np.float32)).to(dev)
    whole = {}
    for Lr in (24000, 65536):
        h = (rng.standard_normal((2, Lr)) * np.exp(-6.9 * np.arange(Lr) / Lr)).astype(np.float32)
        tail = reverb.LateTail(h, 0)
        T_out = T + Lr - 1
        out = torch.empty((2, T_out), dtype=torch.float32, device=dev)
        ws = reverb.long_fir_workspace(1, T_out, Lr, Np, dev)
        n_fft = 1 << int(np.ceil(np.log2(T_out)))
        H = torch.fft.rfft(torch.from_numpy(h).to(dev), n_fft)

        def ours():
            reverb.long_fir_device(bus, tail, Np, out, ws=ws)

        def full_fft():
            return torch.fft.irfft(torch.fft.rfft(bus, n_fft) * H, n_fft)[:, :T_out]
        ref = full_fft()
        ours()
        err = float((out - ref).abs().max() / ref.abs().max())
        t_ours, t_fft = [], []
        for _ in range(args.rounds):
            t_ours.append(_events_ms(ours, args.reps))
            t_fft.append(_events_ms(full_fft, args.reps))
        c = counted(T_out, Lr, Np)
        us = sorted(t_ours)[len(t_ours) // 2] * 1e3
        whole[f"Lr_{Lr}"] = {"T_out": T_out, "counted": c, "long_fir_us": _stats(t_ours), "torch_fft_us": _stats(t_fft),
                             "torch_fft_points": n_fft, "gflop_per_s": round(c["flop"] / us * 1e-3, 1),
                             "gbyte_per_s": round(c["bytes_total"] / us * 1e-3, 1),
                             "max_difference_over_peak": err}
    res["whole_signal_10s_48k"] = whole

    # ---- (c) a stream block of 64 sources x 512 samples in an order-1 room, with and without the tail
    host = bas.synth.make_table("consistent", 0).truncated(128)
    tbl = bas.irs_and_delaydiffs(host.upsampling, host.diffs_left, host.diffs_right, host.irs_left, host.irs_right)
    n_src, K, S, B = 64, 512, 32, 512
    room = scene.Room(ROOM, order=1)
    tail = reverb.late_tail(room, fs, host, seconds=24000 / fs)
    size = np.array(ROOM)
    t = np.linspace(0.0, 1.0, B // K + 1)
    pos = size / 2 + (size / 2 - 0.4) * np.sin(2 * np.pi * rng.uniform(0.5, 2.0, (n_src, 1, 3)) * t[None, :, None]
                                               + rng.uniform(0, 2 * np.pi, (n_src, 1, 3)))
    lp = size / 2 + np.stack([0.5 * np.cos(2 * np.pi * t), 0.5 * np.sin(2 * np.pi * t), 0.0 * t], -1)
    pos_d, lp_d = torch.from_numpy(pos).to(dev), torch.from_numpy(lp).to(dev)
    blk = torch.from_numpy((rng.standard_normal((n_src, B)) * 0.1).astype(np.float32)).to(dev)
    sts = {}
    for name, late in (("dry", None), ("late", tail)):
        sts[name] = bas.SceneStreamRenderer(tbl, n_src, K, S, fs, max_distance=40.0, room=room, copy_out=False, late=late)
        sts[name].prepare(B)
    wall, gpu = {"dry": [], "late": []}, {"dry": [], "late": []}
    for _ in range(args.rounds):
        for name, st in sts.items():
            wall[name].append(_wall_ms(lambda: st.process(blk, pos_d, lp_d), 10 * args.reps))
            gpu[name].append(_events_ms(lambda: st.process(blk, pos_d, lp_d), 10 * args.reps))
    added = 5                                              # bus mix, three of the convolver, the bus's carry
    med = {k: {n: sorted(v[n])[len(v[n]) // 2] * 1e3 for n in v} for k, v in (("wall", wall), ("gpu", gpu))}
    res["stream_block_64x512_order_1"] = {
        "Lr": tail.Lr, "lag": tail.lag, "partitions": tail.partitions(Np), "launches_added": added,
        "counted": counted(B, tail.Lr, Np),
        "dry": {"wall_us_per_block": _stats(wall["dry"]), "gpu_us_per_block": _stats(gpu["dry"])},
        "late": {"wall_us_per_block": _stats(wall["late"]), "gpu_us_per_block": _stats(gpu["late"])},
        "difference_us": {"wall": round(med["wall"]["late"] - med["wall"]["dry"], 1),
                          "gpu": round(med["gpu"]["late"] - med["gpu"]["dry"], 1),
                          "wall_per_launch_added": round((med["wall"]["late"] - med["wall"]["dry"]) / added, 1),
                          "gpu_per_launch_added": round((med["gpu"]["late"] - med["gpu"]["dry"]) / added, 1)}}

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
