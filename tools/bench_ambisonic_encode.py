"""Cost of the ambisonic encoder, written to profiles/ambisonic_encode_cost.json:
  (a) offline: 1024 sources x 479 744 samples (937 chunks of 512) into an order-3 bed, with one static bank and with banks
      per boundary (bas_ambi_encode_f32, one launch), beside the same sums from torch ops on the same tensors in the same
      process and alternating with them (static: one matmul; per boundary: two bmm over the chunks and an addcmul), with the
      largest difference between the two and the fraction of the byte floor 4 (n_src + C) T over the HBM peak (8.0 TB/s
      by the data sheet, 6.3 TB/s as a float4 copy reaches it); bas_ambi_encode_gains_f32 for the 938 boundaries on its own;
  (b) the point of the stage: 256 and 1024 rows rendered as objects (render_angles_device: angles and gains on the device)
      and as encode_bed + render_bed (the encoder, the decoder's mix and the FIR of its 25 rows), alternating;
  (c) a stream block of 512 samples at K = 512 with 256 and 1024 sources: the encoder's two launches as replays of one
      captured graph, alone and followed by a BedStream's write for one session and for 256 sessions sharing the bed.
GPU times are between HIP events around `reps` back-to-back calls after a warm-up call; every figure is taken `rounds` times,
alternating between the things compared; the json holds the median and the spread (min, max) over the rounds.  Run the
command twice and compare the files for the spread between runs.
Usage: python tools/bench_ambisonic_encode.py [--reps N] [--rounds R] [--only offline|objects|stream] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ambisonics import _events_ms, _stats, _median, _turning_head, HBM_SPEC, HBM_COPY  # noqa: E402


def main():
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import ambisonics as am
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=("offline", "objects", "stream"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ambisonic_encode_cost.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ambisonic_encode.py needs a GPU")
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    order, C, K, n_chunks = 3, 16, 512, 937
    T = n_chunks * K
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "order": order, "channels": C,
           "chunk": K, "samples": T, "encode_block": am.ENCODE_BLOCK}
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)

    def noise(shape, scale):
        return torch.randn(shape, generator=gen, device=dev, dtype=torch.float32) * scale

    def angles(n_src, nq):
        el = rng.uniform(-1.2, 1.2, (n_src, 1)) + 0.2 * np.sin(np.linspace(0, 3, nq))[None, :]
        az = rng.uniform(-3, 3, (n_src, 1)) + np.linspace(0, 2, nq)[None, :] * rng.uniform(-1, 1, (n_src, 1))
        return el, az, rng.uniform(0.2, 1.0, (n_src, nq))

    # ---- (a) offline: ours and the torch composition, alternating
    if args.only in (None, "offline"):
        n_src = 1024
        x = noise((n_src, T), 0.1)
        el, az, gn = (torch.from_numpy(a).to(dev) for a in angles(n_src, n_chunks + 1))
        E = am.encoding_gains_device(el, az, order, "sn3d", gn)                # [938, 1024, 16]
        E0 = E[0].contiguous()
        out = torch.empty((C, T), dtype=torch.float32, device=dev)
        w = (torch.arange(K, dtype=torch.float32, device=dev) * (1.0 / K))[None, None, :]
        x3 = x.view(n_src, n_chunks, K).permute(1, 0, 2)                       # [chunks, n_src, K] (a view)
        Et = E.transpose(1, 2)                                                 # [938, 16, 1024] (a view)

        def torch_boundary():
            a, b = torch.bmm(Et[:-1], x3), torch.bmm(Et[1:], x3)
            return torch.addcmul(a, w, b - a).permute(1, 0, 2).reshape(C, T)

        floor_bytes = 4 * (n_src + C) * T
        offline = {"sources": n_src, "bytes_floor": floor_bytes, "plan_static": am.encode_plan(C, K, T, True),
                   "plan_per_boundary": am.encode_plan(C, K, T, False)}
        for name, ours, theirs in (("static", lambda: am.encode_device(x, K, E0, out), lambda: torch.matmul(E0.t(), x)),
                                   ("per_boundary", lambda: am.encode_device(x, K, E, out), torch_boundary)):
            ref = theirs()
            ours()
            t_ours, t_torch = [], []
            for _ in range(args.rounds):
                t_ours.append(_events_ms(ours, args.reps))
                t_torch.append(_events_ms(theirs, args.reps))
            sec = _median(t_ours) * 1e-3
            offline[name] = {"encode_us": _stats(t_ours), "torch_us": _stats(t_torch),
                             "fraction_of_byte_floor_at_8_0_TBps": round(floor_bytes / HBM_SPEC / sec, 4),
                             "fraction_of_byte_floor_at_6_3_TBps": round(floor_bytes / HBM_COPY / sec, 4),
                             "achieved_GBps": round(floor_bytes / sec / 1e9, 1),
                             "achieved_GFLOPs": round(2 * C * n_src * T * (1 if name == "static" else 2) / sec / 1e9, 1),
                             "max_difference_from_torch": float((out - ref).abs().max()), "peak_out": float(out.abs().max())}
            del ref
        t_g = [_events_ms(lambda: am.encoding_gains_device(el, az, order, "sn3d", gn, out=E), args.reps)
               for _ in range(args.rounds)]
        offline["gains_938_boundaries_us"] = _stats(t_g)
        res["offline_1024_sources"] = offline
        del x, x3, E, Et, out
        torch.cuda.empty_cache()

    host = bas.synth.make_table("consistent", 0).truncated(128)
    tbl = bas.irs_and_delaydiffs(host.upsampling, host.diffs_left, host.diffs_right, host.irs_left, host.irs_right,
                                 device="cuda:0")
    dec = am.Decoder(order)

    # ---- (b) the same rows as objects and as one bed
    if args.only in (None, "objects"):
        objects = {}
        head = torch.from_numpy(_turning_head(n_chunks + 1, rng)).to(dev)
        for n_src in (256, 1024):
            x = noise((n_src, T), 0.1 / np.sqrt(n_src))
            el, az, gn = angles(n_src, n_chunks + 1)
            eld, azd, gnd = (torch.from_numpy(a).to(dev) for a in (el, az, gn))

            def as_objects():                                                  # angles and gains on the device, as the bed's
                return bas.apply_hrtf.render_angles_device(x, K, 32, tbl, eld, azd, normalize="none", gain=gnd)

            def as_bed():
                return bas.render_bed(bas.encode_bed(x, K, eld, azd, order, gain=gnd), K, 32, tbl, dec, head=head,
                                      normalize="none")

            def encode_only():
                return bas.encode_bed(x, K, eld, azd, order, gain=gnd)

            t = {"objects": [], "bed": [], "encode_bed": []}
            for _ in range(args.rounds):
                t["objects"].append(_events_ms(as_objects, max(1, args.reps // 4)))
                t["bed"].append(_events_ms(as_bed, max(1, args.reps // 4)))
                t["encode_bed"].append(_events_ms(encode_only, max(1, args.reps // 4)))
            objects[f"sources_{n_src}"] = {"objects_render_angles_device_ms": _stats(t["objects"], 1.0, 3),
                                           "encode_bed_plus_render_bed_ms": _stats(t["bed"], 1.0, 3),
                                           "encode_bed_alone_ms": _stats(t["encode_bed"], 1.0, 3),
                                           "objects_over_bed": round(_median(t["objects"]) / _median(t["bed"]), 2)}
            del x
            torch.cuda.empty_cache()
        res["objects_against_one_bed"] = objects

    # ---- (c) a stream block of 512 samples
    if args.only in (None, "stream"):
        B = 512
        blocks = {}
        for n_src in (256, 1024):
            enc = bas.BedEncoder(order, n_src, K)
            enc.prepare(B)
            enc.input_view(B).copy_(noise((n_src, B), 0.05))
            el, az, gn = angles(n_src, 2)
            ev, av = enc.trajectory_views(B)
            ev.copy_(torch.from_numpy(el).to(dev))
            av.copy_(torch.from_numpy(az).to(dev))
            enc.gain_view(B).copy_(torch.from_numpy(gn).to(dev))
            entry = {"sources": n_src, "block": B, "launches": 2, "plan": am.encode_plan(C, K, B, False)}
            graphs = {}
            for G in (1, 256):
                r = (bas.StreamRenderer(tbl, dec.V, K, 32, graph=False) if G == 1 else
                     bas.StreamBatchRenderer(tbl, G, dec.V, K, 32, graph=False))
                stage = bas.BedStream(r, dec, row=0)
                stage.prepare(B)
                bedv, hv = stage.bed_view(B), stage.head_view(B)
                q = rng.standard_normal(tuple(hv.shape))
                q[..., 0] = np.abs(q[..., 0]) + 0.5
                hv.copy_(torch.from_numpy(q).to(dev))
                enc.encode(bedv)
                stage.write(bedv, hv)
                torch.cuda.synchronize()
                if G == 1:
                    graphs["encoder"] = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graphs["encoder"]):
                        enc.encode(bedv)
                graphs[f"encoder_and_write_{G}_sessions"] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[f"encoder_and_write_{G}_sessions"]):
                    enc.encode(bedv)
                    stage.write(bedv, hv)
                graphs[f"write_{G}_sessions"] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[f"write_{G}_sessions"]):
                    stage.write(bedv, hv)
            t = {k: [] for k in graphs}
            for _ in range(args.rounds):
                for k, g in graphs.items():
                    t[k].append(_events_ms(g.replay, 10 * args.reps))
            for k in graphs:
                entry[k + "_graph_us_per_block"] = _stats(t[k])
            blocks[f"sources_{n_src}"] = entry
        res["stream_block_512"] = blocks

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
