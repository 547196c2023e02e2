"""Cost of the ambisonic bed stage, written to profiles/ambisonic_cost.json:
  (a) offline: an order-3 bed decoded to the 25 default speakers, 479 744 samples (937 chunks of 512, 10 s at 48 kHz), one
      group, with the static decoder and with a turning head (bas_matrix_mix_f32, one launch; the turning head also pays
      bas_ambi_matrices_f32 for its 938 boundaries, timed on its own), beside the same decode from torch ops in the same
      process and alternating with it (static: one matmul; turning: the float32 matrices, two bmm over the chunks and the
      crossfade), with the largest difference between the two and the fraction of the byte floor 4 (C + V) T over the HBM
      peak (8.0 TB/s by the data sheet, 6.3 TB/s as a float4 copy reaches it);
  (b) streams: a block of 512 samples at K = 512, for one session and for 256 sessions that share one bed under 256 heads:
      the stage's two launches (matrices + mix) as plain calls and as replays of one captured graph, beside the block renders
      the README quotes (28 us for one real-time block of StreamRenderer, 69.5 us for 256 sessions of StreamBatchRenderer:
      quoted, not run), and the block render itself with and without the 25 speaker rows (2 against 27 sources per session,
      graph replays of the same renderer): what a bed costs the render.
GPU times are between HIP events around `reps` back-to-back calls after a warm-up call, host work included (a plain call is
bound by the host's launch rate where the kernel is shorter than a launch takes to issue: the graph figure is the GPU's).
Every figure is taken `rounds` times, alternating between the things compared; the json holds the median and the spread
(min, max) over the rounds.  Run the command twice and compare the files for the spread between runs.
Usage: python tools/bench_ambisonics.py [--reps N] [--rounds R] [--only offline|stream] [--out profiles/ambisonic_cost.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RENDER_US = {1: 28.0, 256: 69.5}                           # README: the block renders a bed block precedes
HBM_SPEC, HBM_COPY = 8.0e12, 6.3e12                         # bytes / s: the data sheet, and what a float4 copy reaches


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


def _median(values):
    return sorted(values)[len(values) // 2]


def _turning_head(nb, rng):
    t = np.linspace(0.0, 1.0, nb)
    yaw, pitch, roll = 2.5 * np.sin(2 * np.pi * t), 0.4 * np.sin(3 * np.pi * t + 1.0), 0.3 * np.cos(5 * np.pi * t)
    cy, sy, cp, sp, cr, sr = np.cos(yaw / 2), np.sin(yaw / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(roll / 2), np.sin(roll / 2)
    return np.stack([cy * cp * cr + sy * sp * sr, cy * sp * cr + sy * cp * sr, cy * cp * sr - sy * sp * cr,
                     sy * cp * cr - cy * sp * sr], axis=-1)


def main():
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import ambisonics as am
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("offline", "stream"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ambisonic_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ambisonics.py needs a GPU")
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    dec = am.Decoder(3)
    C, V, K = dec.C, dec.V, 512
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "order": 3, "channels": C,
           "speakers": V, "chunk": K, "tile": am.mix_tile(C, V, K)}

    # ---- (a) 10 s at 48 kHz: ours and the torch composition, alternating
    if args.only in (None, "offline"):
        n_chunks = 937
        T = n_chunks * K
        bed = torch.from_numpy((rng.standard_normal((C, T)) * 0.1).astype(np.float32)).to(dev)
        head = torch.from_numpy(_turning_head(n_chunks + 1, rng)).to(dev)
        out = torch.empty((V, T), dtype=torch.float32, device=dev)
        M = am.mixing_matrices_device(dec, head)
        D32 = dec.on(dev)[3]
        w = (torch.arange(K, dtype=torch.float32, device=dev) * (1.0 / K))[None, None, :]
        bed3 = bed.view(C, n_chunks, K).permute(1, 0, 2)                  # [chunks, C, K] (a view)

        def torch_turning():
            a, b = torch.bmm(M[:-1], bed3), torch.bmm(M[1:], bed3)
            return torch.addcmul(a, w, b - a).permute(1, 0, 2).reshape(V, T)

        floor_bytes = 4 * (C + V) * T
        offline = {"samples": T, "bytes_floor": floor_bytes, "flops": 4 * C * V * T}
        for name, ours, theirs in (("static", lambda: am.decode_device(bed, K, D32, out), lambda: torch.matmul(D32, bed)),
                                   ("turning_head", lambda: am.decode_device(bed, K, M, out), torch_turning)):
            ref = theirs()
            ours()
            t_ours, t_torch = [], []
            for _ in range(args.rounds):
                t_ours.append(_events_ms(ours, args.reps))
                t_torch.append(_events_ms(theirs, args.reps))
            sec = _median(t_ours) * 1e-3
            offline[name] = {"mix_us": _stats(t_ours), "torch_us": _stats(t_torch),
                             "fraction_of_byte_floor_at_8_0_TBps": round(floor_bytes / HBM_SPEC / sec, 4),
                             "fraction_of_byte_floor_at_6_3_TBps": round(floor_bytes / HBM_COPY / sec, 4),
                             "achieved_GBps": round(floor_bytes / sec / 1e9, 1),
                             "achieved_GFLOPs": round(2 * C * V * T * (1 if name == "static" else 2) / sec / 1e9, 1),
                             "max_difference_from_torch": float((out - ref).abs().max()), "peak_out": float(out.abs().max())}
        t_mat = [_events_ms(lambda: am.mixing_matrices_device(dec, head, out=M), args.reps) for _ in range(args.rounds)]
        offline["matrices_938_boundaries_us"] = _stats(t_mat)
        res["offline_10s_48k"] = offline

    # ---- (b) a stream block of 512 samples for 1 and 256 sessions
    if args.only in (None, "stream"):
        B = 512
        host = bas.synth.make_table("consistent", 0).truncated(128)
        tbl = bas.irs_and_delaydiffs(host.upsampling, host.diffs_left, host.diffs_right, host.irs_left, host.irs_right,
                                     device="cuda:0")
        blocks = {}
        for G in (1, 256):
            def renderer(n_src):
                if G == 1:
                    return bas.StreamRenderer(tbl, n_src, K, 32, graph=True, copy_out=False)
                return bas.StreamBatchRenderer(tbl, G, n_src, K, 32, graph=True, copy_out=False)
            lead = () if G == 1 else (G,)
            with_bed, without = renderer(2 + V), renderer(2)
            stage = bas.BedStream(with_bed, dec, row=2)
            timed = {}
            for name, r in (("with_bed_27_rows", with_bed), ("objects_only_2_rows", without)):
                r.prepare(B)
                if r is with_bed:
                    stage.prepare(B)
                xv, (ev, av) = r.input_view(B), r.trajectory_views(B)
                xv.copy_(torch.from_numpy((rng.standard_normal(tuple(xv.shape)) * 0.05).astype(np.float32)).to(dev))
                ev[..., :2, :].copy_(torch.from_numpy(rng.uniform(-0.7, 1.3, lead + (2, 2))).to(dev))
                av[..., :2, :].copy_(torch.from_numpy(rng.uniform(-3.0, 3.0, lead + (2, 2))).to(dev))
                timed[name] = (lambda r=r, xv=xv, ev=ev, av=av: r.process(xv, ev, av))
            bedv, hv = stage.bed_view(B), stage.head_view(B)
            bedv.copy_(torch.from_numpy((rng.standard_normal(tuple(bedv.shape)) * 0.1).astype(np.float32)).to(dev))
            q = rng.standard_normal(lead + (2, 4))
            q[..., 0] = np.abs(q[..., 0]) + 0.5
            hv.copy_(torch.from_numpy(q).to(dev))
            stage.write(bedv, hv)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                stage.write(bedv, hv)
            t = {k: [] for k in ("plain", "graph", "static_plain", *timed)}
            for _ in range(args.rounds):
                t["plain"].append(_events_ms(lambda: stage.write(bedv, hv), 10 * args.reps))
                t["graph"].append(_events_ms(graph.replay, 10 * args.reps))
                t["static_plain"].append(_events_ms(lambda: stage.write(bedv, None), 10 * args.reps))
                for name, fn in timed.items():
                    t[name].append(_events_ms(fn, 10 * args.reps))
            med = _median(t["graph"]) * 1e3
            rows_cost = (_median(t["with_bed_27_rows"]) - _median(t["objects_only_2_rows"])) * 1e3
            blocks[f"G_{G}"] = {"sessions": G, "block": B, "shared_bed": G > 1, "launches": 2,
                                "stage_plain_us_per_block": _stats(t["plain"]), "stage_graph_us_per_block": _stats(t["graph"]),
                                "head_fixed_stage_plain_us_per_block": _stats(t["static_plain"]),
                                "render_us_per_block_readme": RENDER_US[G], "stage_over_readme_render": round(med / RENDER_US[G], 3),
                                "render_with_bed_us_per_block": _stats(t["with_bed_27_rows"]),
                                "render_objects_only_us_per_block": _stats(t["objects_only_2_rows"]),
                                "cost_of_25_rows_in_the_render_us": round(rows_cost, 1)}
        res["stream_block_512"] = blocks

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
