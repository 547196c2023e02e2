"""Cost of the per-source propagation delay, written to profiles/delay_cost.json:
  - bas_delay_rows_f32 on the bench scene's shape (256 x 441 000), us and TB/s on its read + write bytes;
  - a 256 x 512 StreamRenderer block with and without delay (graph replay: wall time per block, GPU time between HIP
    events around the replay, kernel launches per block);
  - a StreamBatchRenderer block of 256 sessions x 4 sources x 512 with and without delay (dense inputs: the fused pack);
  - render_batch of 256 items x 10 s (one source each) with and without delay.
The rows kernel is set beside a device copy of the same bytes (torch's copy kernel): the memory-bound floor of its
traffic.  Launch counts per block are stated from the code (the block graph's kernels), not counted.
Usage: python tools/bench_delay.py [--reps N] [--out profiles/delay_cost.json]"""
import argparse
import json
import os
import sys
import time

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


def main():
    import torch
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import propagation as prop
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delay_cost.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0)}

    # ---- rows kernel on the bench scene's shape
    n_src, N, K = 256, 441000, 512
    x = torch.from_numpy(rng.standard_normal((n_src, N)).astype(np.float32)).to(dev)
    nq = (N - 1) // K + 2
    t = np.arange(nq, dtype=np.float64)
    dl = 2.0 + 400.0 * (0.5 + 0.5 * np.sin(t[None, :] * rng.uniform(0.02, 0.3, (n_src, 1))))
    d = torch.from_numpy(dl).to(dev)
    out = torch.empty((n_src, (N + 3) // 4 * 4), dtype=torch.float32, device=dev)[:, :N]
    rows = {}
    for interp in ("cubic", "linear"):
        ms = _events_ms(lambda: prop.delay_rows_device(x, d, K, interp, out), args.reps)
        nbytes = 2 * 4 * n_src * N
        rows[interp] = {"us": round(ms * 1e3, 1), "TB_per_s": round(nbytes / (ms * 1e-3) / 1e12, 2),
                        "bytes_read_plus_written": nbytes}
    ms = _events_ms(lambda: out.copy_(x), args.reps)
    rows["copy_same_bytes"] = {"us": round(ms * 1e3, 1), "TB_per_s": round(2 * 4 * n_src * N / (ms * 1e-3) / 1e12, 2)}
    res["rows_kernel_256x441000"] = rows

    # ---- a StreamRenderer block: graph replay, with and without delay
    tb = bas.synth.make_table("consistent", 0, upsampling=8).truncated(128)
    tbl = bas.irs_and_delaydiffs(tb.upsampling, tb.diffs_left, tb.diffs_right, tb.irs_left, tb.irs_right)
    B = 512
    blk = torch.from_numpy(rng.standard_normal((n_src, B)).astype(np.float32)).to(dev)
    stream = {}
    for name, kw in (("no_delay", {}), ("delay", {"max_delay": 2205.0})):
        st = bas.StreamRenderer(tbl, n_src, K, 32, graph=True, copy_out=False, **kw)
        st.prepare(B)
        dv = st.delay_view(B).fill_(100.0) if kw else None
        iv = st.input_view(B)
        iv.copy_(blk)
        ev, ea = st.trajectory_views(B)

        def one():
            st.process(iv, ev, ea, delay=dv)
        ms_gpu = _events_ms(one, args.reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            one()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.reps
        stream[name] = {"wall_us_per_block": round(wall * 1e6, 1), "gpu_us_per_block": round(ms_gpu * 1e3, 1),
                        "launches_added_per_block_stated": "bas_delay_rows_f32 + bas_delay_carry_f32" if kw else "none"}
    res["stream_renderer_256x512"] = stream

    # ---- a StreamBatchRenderer block: 256 sessions x 4 sources x 512, dense device inputs (the fused pack)
    G, ns = 256, 4
    blks = torch.from_numpy(rng.standard_normal((G, ns, B)).astype(np.float32)).to(dev)
    ang = torch.zeros((G, ns, B // K + 1), dtype=torch.float64, device=dev)
    dly = torch.full((G, ns, B // K + 1), 100.0, dtype=torch.float64, device=dev)
    sbr = {}
    for name, kw in (("no_delay", {}), ("delay", {"max_delay": 2205.0})):
        sb = bas.StreamBatchRenderer(tbl, G, ns, K, 32, graph=True, copy_out=False, **kw)
        sb.prepare(B)
        dd = dly if kw else None

        def one():
            sb.process(blks, ang, ang, delay=dd)
        ms_gpu = _events_ms(one, args.reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            one()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.reps
        sbr[name] = {"wall_us_per_block": round(wall * 1e6, 1), "gpu_us_per_block": round(ms_gpu * 1e3, 1),
                     "launches_added_per_block_stated": "bas_delay_carry_f32 (the pack delays)" if kw else "none"}
    res["stream_batch_256x4x512"] = sbr

    # ---- render_batch: 256 items x 10 s, one source each
    Bn = 256
    sig = torch.from_numpy(rng.standard_normal((Bn, N)).astype(np.float32) * 0.1).to(dev)
    nqb = -(-N // K) + 1
    el = torch.zeros((Bn, nqb), dtype=torch.float64, device=dev)
    dlb = torch.from_numpy(np.ascontiguousarray(dl[:, :nqb])).to(dev)
    batch = {}
    for name, dd in (("no_delay", None), ("delay", dlb)):
        ms = _events_ms(lambda: bas.render_batch(sig, K, 32, el, el, tbl, normalize="none", delay=dd), max(args.reps // 10, 3))
        batch[name] = {"ms": round(ms, 3)}
    res["render_batch_256x10s"] = batch
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
