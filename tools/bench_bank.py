#!/usr/bin/env python3
"""What a table bank costs one block of a StreamBatchRenderer, in one process on one GPU.

Per case (G sessions x n_src sources x blocks of B, K 512 / S 32 / L 128) and per row
  plain      one table (the renderer of DESIGN.md §3.8; the only row a tree without banks can run: --plain-only),
  bank-1     a bank of one table, every session on it,
  bank-51    a bank of 51 distinct tables with the sessions spread over all of them,
the renderer is prepared (layout, warm-up, graph capture) and fed device-resident blocks and angles; reported are medians
over the timed steps of gpu_us - HIP events around one block's launches (the pack and the replay of the captured graph) -
and wall_us (host time of one block up to a stream synchronisation).  table_bytes is what the bank's packed tables hold,
touched_table_bytes what the block's plans can reach: the tables some session is on.  The plan kernel's own time comes from
a kernel trace of a run of its own (--trace-steps N runs N blocks of the chosen --row / --case and nothing else).

--root PATH imports the package from another tree (the parent commit's, built), for the "plain at the parent" row.
Prints one JSON line; --out appends it to a file (the command is run twice and both lines are kept).
    python3 tools/bench_bank.py [--steps 200] [--warmup 20] [--plain-only] [--root PATH] [--label TEXT] [--out profiles/bank_cost.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

FS, K, S, L = 44100, 512, 32, 128
CASES = [(256, 4, 512), (32, 32, 2048)]                       # (sessions G, sources, block B)
N_BANK = 51


def _time(step, steps, warmup, torch):
    gpu, wall = [], []
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev0.record()
        step()
        ev1.record()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warmup:
            gpu.append(ev0.elapsed_time(ev1) * 1e3)
            wall.append((t2 - t0) * 1e6)
    q = statistics.quantiles(gpu, n=10)
    return {"gpu_us": round(statistics.median(gpu), 1), "gpu_us_p10": round(q[0], 1), "gpu_us_p90": round(q[-1], 1),
            "wall_us": round(statistics.median(wall), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--plain-only", action="store_true", help="the plain row alone (a tree without banks)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree the package is imported from (default: this one)")
    ap.add_argument("--label", default="this commit")
    ap.add_argument("--case", type=int, default=None, help="only this case (index into CASES)")
    ap.add_argument("--row", default=None, choices=["plain", "bank-1", "bank-51"], help="only this row")
    ap.add_argument("--trace-steps", type=int, default=0, help="run this many blocks untimed (for a kernel trace) and stop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import binaural_audio_synthesis_amd as bas
    if not torch.cuda.is_available():
        raise SystemExit("bench_bank.py needs a GPU")
    full = bas.synth.make_table("consistent", 0)
    host = full.truncated(L)
    rows = ["plain"] if args.plain_only else ["plain", "bank-1", "bank-51"]
    rows = [r for r in rows if args.row in (None, r)]
    tables = {}
    if "plain" in rows:
        tables["plain"] = bas.irs_and_delaydiffs(host.upsampling, host.diffs_left, host.diffs_right, host.irs_left,
                                                 host.irs_right)
    if "bank-1" in rows:
        tables["bank-1"] = bas.TableBank([host])
    if "bank-51" in rows:                                     # 51 distinct tables: the synthetic one and scaled, rolled copies
        many = [host] + [bas.synth.SyntheticTable(host.upsampling, np.roll(host.diffs_left, t, 0), np.roll(host.diffs_right, t, 1),
                                                  np.roll(host.irs_left, t, 0) * (1 - t / 128), np.roll(host.irs_right, t, 0))
                         for t in range(1, N_BANK)]
        tables["bank-51"] = bas.TableBank(many)
    rng = np.random.default_rng(0)
    result = {"label": args.label, "root": os.path.relpath(os.path.abspath(args.root)),
              "workload": f"G sessions x n_src sources x blocks of B, K={K} S={S} L={L}; one block per step, graph replay",
              "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "cases": []}
    for ci, (G, n_src, B) in enumerate(CASES):
        if args.case not in (None, ci):
            continue
        nb = B // K + 1
        x = torch.from_numpy((rng.standard_normal((G, n_src, B)) * 0.1).astype(np.float32)).cuda()
        e = torch.from_numpy(rng.uniform(-0.7, 1.2, (G, n_src, nb))).cuda()
        a = torch.from_numpy(rng.uniform(-7, 7, (G, n_src, nb))).cuda()
        case = {"G": G, "n_src": n_src, "B": B, "rows": {}}
        for row in rows:
            tbl = tables[row]
            kw = {}
            if row != "plain":
                kw["tables"] = [g % tbl.n_tables for g in range(G)]
            sb = bas.StreamBatchRenderer(tbl, G, n_src, K, S, graph=True, copy_out=False, **kw)
            sb.prepare(B)
            if args.trace_steps:
                for _ in range(args.trace_steps):
                    sb.process(x, e, a)
                torch.cuda.synchronize()
                continue
            t = _time(lambda: sb.process(x, e, a), args.steps, args.warmup, torch)
            lay = sb.layout(B)
            t["kernel"] = bas._hip.lib().bas_render_fused_kernel_name(n_src, lay.T_in, K, S, L).decode()
            t["rtf"] = round(G * B / FS / (t["wall_us"] * 1e-6), 1)
            per = tbl.packed.numel() * 4 // (1 if row == "plain" else tbl.n_tables)
            t["table_bytes"] = tbl.packed.numel() * 4
            t["touched_table_bytes"] = per * (1 if row == "plain" else len(set(kw["tables"])))
            case["rows"][row] = t
            del sb
            torch.cuda.synchronize()
        result["cases"].append(case)
    line = json.dumps(result)
    print(line)
    if args.out and not args.trace_steps:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
