#!/usr/bin/env python3
"""Benchmark of the moving-source render path on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

`python bench.py --gpus N` from a plain shell (no WORLD_SIZE) starts the N ranks itself through
torch.distributed.run - before anything touches the GPU - and relays rank 0's JSON line.

Workload = BASELINE config 4: ONE scene of 256 concurrent moving sources x 10 s of 44.1 kHz mono, chunk K=512,
subchunk S=32, IR L=128 taps (samples_to_keep=128, U=8), synthetic table + seeded noise + per-source
spiral / askew-circle trajectories, mixed to one stereo pair.  One "step" = one full pass of
the reference's make_signal_move_2d path over that scene with inputs resident in HBM when the timed region
starts - the audio AND the trajectories (elev, azim per chunk boundary, float64):

    bas_interp2d_plan_angles_f32   a3: angles -> (4 directions, 3 weights) per chunk boundary (sphere.py:78-121,
                               apply_hrtf.py:199-215, :261-266), and in the same launch the read plans: delays, shift splits,
                               folded blend weights (apply_hrtf.py:219-279)
    bas_render_mix_fused_f32   chunk IRs from the table + time-varying FIR + overlap-add + mix + max|y| + the peak rule
                               (apply_hrtf.py:462-464) in the tail of its last kernel
    [N>1: one RCCL gather of the un-normalised partial mixes to rank 0; there bas_mix_finish_f32: fixed-order sum +
     max|y| + peak rule in one launch]

Scaling: with N > 1 the ONE scene is sharded by source over the GPUs (config 4 read literally: strong scaling,
`value` = that scene's stereo samples per second).  The same invocation then also times the weak reading (every
GPU renders its own 256 sources) and reports it under "extra": {"weak": ...}.  `--scaling weak` makes weak the
headline instead.

Prints ONE JSON line on rank 0 (contract in the task statement) with `roofline` (dominant kernel = the FIR
kernel, timed live with HIP events on the launch stream) and `cpu_baseline` (the oracle's numpy port of the
reference loop, timed on this box's host cores).
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FS = 44100
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
FP32_VALU_PEAK_TF = 157.3      # MI355X_MICROARCH.md: peak FP32 vector


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sources", type=int, default=256, help="sources per GPU (weak) / in the whole scene (strong)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="strong",
                    help="strong (default): BASELINE config 4 read literally, ONE --sources-source scene sharded "
                         "over the GPUs; weak: every GPU renders --sources sources")
    ap.add_argument("--no-extra", action="store_true", help="N > 1: skip the second (weak) measurement")
    ap.add_argument("--root-weight", default="auto",
                    help="strong scaling, N > 1: fraction of an equal share of the sources that rank 0 renders - it also "
                         "receives the gather and sums the partial mixes while the others already render their next "
                         "step (distributed.shard_sources).  auto: an equal share minus the ~15 us the receive + sum "
                         "cost, at ~2.4 us of render per source = 6 sources' worth, spread over the other ranks; 1: equal shares")
    ap.add_argument("--settle-ms", type=float, default=400.0,
                    help="untimed steps for this many milliseconds BEFORE the --warmup steps: a cold MI355X needs ~40 ms "
                         "of load before its clock governor settles (profiles/r02_warmup_series.txt); 0 = off")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--subchunk", type=int, default=32)
    ap.add_argument("--taps", type=int, default=128)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--mode", choices=["scene", "stream"], default="scene",
                    help="scene = the contract's benchmark (default); stream = BASELINE config 5 shape: long stream "
                         "rendered block by block with carried state, inputs and trajectories generated on the device")
    ap.add_argument("--fs", type=int, default=FS)
    ap.add_argument("--block", type=int, default=0,
                    help="stream mode: input samples per block (default: stream.tile_filling_block(2^18, chunk, taps) = 261 120 - "
                         "the window [halo | block] + L - 1 outputs then fills 32 tiles of the FIR kernel; 2^18 itself spills 639 "
                         "samples into a 33rd)")
    ap.add_argument("--regen", action="store_true", help="stream mode: draw a fresh random block inside every timed step")
    ap.add_argument("--cpu-sources-per-core", type=int, default=16)
    ap.add_argument("--lib", default=None, help="another build of the ABI to route every call through (diagnostic / stamps "
                                                "builds of binaural-audio-synthesis_amd/csrc; profiling tools)")
    ap.add_argument("--unfused", action="store_true", help="ablation: chunk IRs through HBM (bas_interp2d_f32 + bas_render_mix_f32)")
    ap.add_argument("--graph", choices=["auto", "on", "off"], default="auto",
                    help="replay the render step (a3 -> plans -> FIR -> reduce [-> peak rule]) as ONE captured hipGraph. "
                         "auto: on whenever the step ends in a collective (N > 1 or --force-pg), where a rank's share is "
                         "short and launch gaps count, and for scenes small enough for the four-wave kernel (a single "
                         "source: three short launches); off for the headline scene at N = 1, where the FIR kernel is "
                         "timed with HIP events inside the timed steps (events cannot be read back from a graph replay: "
                         "under a graph it is timed in eager steps right behind the timed region)")
    ap.add_argument("--overlap-plans", choices=["on", "off"], default="off",
                    help="A/B: compute the read plans of step i+1 on a second stream beside the FIR of step i (they depend on "
                         "the trajectories alone; a rank's share leaves CUs free).  Measured SLOWER for every share (27..256 "
                         "sources: +5..+15 us per step, profiles/r04_ab_overlap_plans.txt): the two cross-stream event waits "
                         "cost more than the ~9 us launch they hide.  Off: the step is the plain sequence on one stream")
    ap.add_argument("--force-pg", action="store_true",
                    help="with --gpus 1: still create a real RCCL communicator (backend nccl, world_size 1) and run the "
                         "N > 1 code path - async gather to rank 0, fixed-order sum, overlapped steps, device-side "
                         "all_reduce of the settle loop.  Also switched on by BAS_BENCH_FORCE_PG=1")
    ap.add_argument("--no-self-check", action="store_true", help="skip the oracle comparison of the timed path's output")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step handed its caller as DIR/<name>.npy "
                         "(scene: y [2, T_out] and peak; stream: the last block and the running peak), at most 64 MB "
                         "in all; the inputs are seeded, so two builds can be compared output for output")
    ap.add_argument("--no-traffic", action="store_true",
                    help="do not measure roofline.traffic (two short child runs under rocprofv3 --pmc, ~10 s each, before "
                         "anything else; N = 1 scene mode only) - the figure of profiles/fir_hbm_traffic.json is then replayed")
    args = ap.parse_args()
    if os.environ.get("BAS_BENCH_FORCE_PG") == "1":
        args.force_pg = True
    return args


# ---------------------------------------------------------------------------
# CPU baseline (rank 0, N=1): the oracle's port of the reference loop, one process per core
# ---------------------------------------------------------------------------
def _cpu_worker(job):
    """Render `n_src` sources of `n` samples with the numpy port of apply_hrtf.py:431-464."""
    import numpy as np
    from oracle import bas_oracle as orc
    import importlib
    synth = importlib.import_module("binaural-audio-synthesis_amd.synth")
    first, n_src, n, k, s, l, total_src = job
    tbl = synth.make_table("consistent", 0).truncated(l)
    in_length, _ = orc.render_lengths(n, k, l)
    t0 = time.perf_counter()
    for i in range(first, first + n_src):
        x = synth.integer_noise(1000 + i, n, 1.0 / total_src)
        traj = source_trajectory(synth, i, total_src, n)
        irs = orc.chunk_irs(tbl, k, in_length, traj)
        orc.render_from_irs(x, k, s, irs, normalize=False)
    return time.perf_counter() - t0


def source_trajectory(synth, i, total_src, n):
    """spiral / circle per source, phase 2*pi*i/total, period 2 + i/64 s."""
    import numpy as np
    phase = 2 * np.pi * i / total_src
    period = 2.0 + (i % 256) / 64.0
    if i % 2 == 0:
        return synth.trajectory("spiral", fs=FS, length_s=n / FS, turns=5.0, phase=phase)
    return synth.trajectory("circle_askew", fs=FS, period_s=period, phase=phase)


def host_cores():
    """Host cores this process may really use: affinity, capped by the cgroup CPU quota."""
    cores = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            cores = min(cores, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return max(1, min(cores, int(os.environ.get("BAS_BENCH_MAX_CORES", "64"))))


def cpu_baseline(args, n, t_out):
    import multiprocessing as mp
    cores = host_cores()
    per = max(1, min(args.cpu_sources_per_core, -(-args.sources // cores)))   # at most the whole scene
    jobs = [(c * per, per, n, args.chunk, args.subchunk, args.taps, args.sources) for c in range(cores)]
    ctx = mp.get_context("spawn")
    t0 = time.perf_counter()
    with ctx.Pool(cores) as pool:
        busy = pool.map(_cpu_worker, jobs)                 # seconds each core spent rendering its sources
    wall = time.perf_counter() - t0
    n_rendered = cores * per
    # sources are independent and cost is linear in their number: extrapolate to the full scene.  The all-core
    # figure uses the slowest worker's render time (process start and table construction left out, which
    # favours the CPU); the single-core figure is one worker's rate (the reference itself is single-threaded).
    scene_seconds = max(busy) * args.sources / n_rendered
    one_core_scene_seconds = sorted(busy)[len(busy) // 2] * args.sources / per
    return {"value": t_out / scene_seconds, "unit": "stereo samples/s", "cores": cores, "kind": "port",
            "note": "the numpy port (per-subchunk np.convolve, vectorised shifts) runs ~5x faster per core than the "
                    "reference's own Python loop it stands in for (BASELINE.md 2: 8.8-11 x real time per core): "
                    "the baseline is conservative in the CPU's favour",
            "sample": f"{n_rendered} of {args.sources} sources x {n} samples ({per} per core, {cores} processes, "
                      f"slowest worker {max(busy):.1f} s of rendering, {wall:.1f} s wall incl. process start), "
                      f"extrapolated linearly to {args.sources} sources",
            "x_realtime": (n / FS) / scene_seconds,
            "single_core": {"value": t_out / one_core_scene_seconds, "unit": "stereo samples/s",
                            "x_realtime": (n / FS) / one_core_scene_seconds,
                            "x_realtime_one_source": (n / FS) / (one_core_scene_seconds / args.sources)}}


# ---------------------------------------------------------------------------
# HBM traffic of the FIR kernel, measured in THIS invocation: two short child runs of this script under rocprofv3, one per
# counter (MI355X_MICROARCH.md: FETCH_SIZE and WRITE_SIZE in separate --pmc passes, kernel trace only beside them).  They
# run before this process has made any GPU call, like the CPU leg.
# ---------------------------------------------------------------------------
def measure_traffic(args):
    import csv
    import glob
    import shutil
    import tempfile
    if shutil.which("rocprofv3") is None:
        return None, "rocprofv3 not found"
    # never from inside a profiled process: the profiler's preloaded library may have initialised the GPU already (a child
    # started from such a process is refused on this pool), and its environment would be inherited by the child
    if "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or any(k.startswith(("ROCPROF", "ROCP_TOOL", "ROCTRACER")) for k in os.environ):
        return None, "running under a profiler: not nesting rocprofv3"
    out = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        tmp = tempfile.mkdtemp(prefix="bas_pmc_", dir="/tmp")
        cmd = ["rocprofv3", "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", tmp, "-o", "pmc", "--",
               sys.executable, os.path.abspath(__file__), "--steps", "3", "--warmup", "1", "--settle-ms", "0", "--no-cpu-baseline",
               "--no-self-check", "--no-traffic", "--sources", str(args.sources), "--seconds", str(args.seconds), "--chunk",
               str(args.chunk), "--subchunk", str(args.subchunk), "--taps", str(args.taps)] + (["--unfused"] if args.unfused else [])
        try:
            env = dict(os.environ, TMPDIR="/tmp")
            r = subprocess.run(cmd, env=env, cwd="/tmp", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240)
            files = glob.glob(os.path.join(tmp, "**", "*counter_collection.csv"), recursive=True)
            if r.returncode != 0 or not files:
                return None, f"rocprofv3 --pmc {counter} failed (rc {r.returncode}): {r.stderr[-200:]}"
            per = {}
            for row in csv.DictReader(open(files[0])):
                if row["Counter_Name"] == counter and "bas_" in row["Kernel_Name"]:
                    per.setdefault(row["Kernel_Name"].split("(")[0].replace("void ", ""), []).append(float(row["Counter_Value"]))
            out[counter] = {k: sum(v) / len(v) for k, v in per.items()}           # KB per dispatch, by kernel
        except Exception as e:                                                    # noqa: BLE001
            return None, f"{counter}: {e}"
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    return out, None


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """Write {name: array} as out_dir/<name>.npy (float32 stays float32, anything else becomes float64).  An array that
    would take the total past 64 MB is replaced by a fixed, seeded sample of its elements (flattened, C order) and
    the sample's positions go beside it as <name>_sample_index.npy (float64).  Returns {file name: shape}."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    arrays = {k: v if v.dtype == np.float32 else v.astype(np.float64) for k, v in arrays.items()}
    budget = (DUMP_LIMIT_BYTES - 4096) // max(1, len(arrays))              # (room for the .npy headers)
    written = {}
    for name, a in arrays.items():
        if a.nbytes > budget:
            m = budget // (a.itemsize + 8)
            pos = np.sort(np.random.default_rng(0).choice(a.size, size=m, replace=False))
            np.save(os.path.join(out_dir, f"{name}_sample_index.npy"), pos.astype(np.float64))
            written[f"{name}_sample_index.npy"] = [m]
            a = a.reshape(-1)[pos]
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
        written[f"{name}.npy"] = list(a.shape)
    return written


class HipEvents:
    """Raw hipEvent_t pairs via libamdhip64 (the library records them on the launch stream)."""

    def __init__(self, n):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.pairs = []
        for _ in range(n):
            a, b = ctypes.c_void_p(), ctypes.c_void_p()
            assert self.hip.hipEventCreate(ctypes.byref(a)) == 0 and self.hip.hipEventCreate(ctypes.byref(b)) == 0
            self.pairs.append((a, b))

    def elapsed_ms(self, i):
        ms = ctypes.c_float()
        rc = self.hip.hipEventElapsedTime(ctypes.byref(ms), self.pairs[i][0], self.pairs[i][1])
        assert rc == 0, f"hipEventElapsedTime rc={rc}"
        return ms.value


def stream_mode(args):
    """BASELINE config 5 (1024 sources, 48 kHz, hours of audio): `steps` blocks of `block` samples through
    StreamRenderer; nothing but one block of inputs, chunk IRs and outputs is ever resident, and the
    trajectory -> parameter step runs on the device.  `--steps 662` is the whole hour at 48 kHz (blocks of 261 120 samples).  With --gpus N
    (torch.distributed.run) the sources are sharded over the ranks and every block ends in one gather of the
    partial stereo block (distributed.ShardedStreamRenderer); --force-pg runs that path on one rank with a real RCCL
    communicator.  One JSON line, not the contract's metric."""
    import math
    import torch
    import torch.distributed as dist
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import _hip
    if args.lib:
        _hip.set_library(os.path.abspath(args.lib))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if os.environ.get("BAS_BENCH_ONE_DEVICE") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run"
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)
    collective = world > 1 or args.force_pg
    if world > 1:
        backend = os.environ.get("BAS_BENCH_BACKEND", "nccl")
        dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))
    elif args.force_pg:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        dist.init_process_group("nccl", world_size=1, rank=0, device_id=dev)
    n_total, k, s, l, fs = args.sources, args.chunk, args.subchunk, args.taps, args.fs
    B = args.block if args.block > 0 else bas.stream.tile_filling_block(1 << 18, k, l)
    host = bas.synth.make_table("consistent", 0).truncated(l)
    tbl = bas.irs_and_delaydiffs(host.upsampling, host.diffs_left, host.diffs_right, host.irs_left, host.irs_right,
                                 device=dev)
    st = bas.distributed.ShardedStreamRenderer(tbl, n_total, k, s)
    n_src = len(st.sources)
    src = torch.arange(st.sources.start, st.sources.stop, dtype=torch.float64, device=dev)[:, None]
    phase = 2 * math.pi * src / n_total
    period = (2.0 + (src % 256) / 64.0) * fs
    gen = torch.Generator(device=dev).manual_seed(5 + rank)
    gloo = collective and dist.get_backend() == "gloo"

    # the input block lives in the renderer's own input buffer (what a decoder / H2D copy would fill in place):
    # resident in HBM when a timed step starts, as the bench contract asks; --regen draws a fresh block per step
    xin = st.local.input_view(B)
    xin.copy_((torch.rand((n_src, B), generator=gen, device=dev) * 2 - 1) * (1.0 / n_total))
    # synthetic trajectories, generated on the device inside every timed step, straight into the renderer's own angle
    # buffers: askew circles with a per-source period, angle = 2 pi t / period + phase at t = i B, i B + K, .., (i + 1) B
    ev_view, av_view = st.local.trajectory_views(B)
    w_src = 2 * math.pi / period                            # [n_src, 1] rad per sample
    base = w_src * (torch.arange(B // k + 1, dtype=torch.float64, device=dev)[None, :] * k) + phase

    def block(i):
        torch.add(base, w_src, alpha=float(i * B), out=av_view)                    # azimuth keeps winding (1e4 rad after an hour)
        torch.cos(av_view, out=ev_view)
        ev_view.mul_(math.pi / 4)
        if args.regen:
            xin.copy_((torch.rand((n_src, B), generator=gen, device=dev) * 2 - 1) * (1.0 / n_total))
        return xin, ev_view, av_view

    st.local.prepare(B)                                     # buffers + hipGraph before the stream starts

    def step(i):
        return st.process(*block(i))          # under gloo (rehearsal) gather_mix stages the gather through the host

    for i in range(args.warmup):
        step(i)
    if collective:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, args.warmup + args.steps):
        y = step(i)
    torch.cuda.synchronize()
    if collective:
        dist.barrier()
    el = time.perf_counter() - t0
    # (copied before the event blocks below render into the same buffers)
    dumped = {"y": y.cpu().numpy(), "peak": [st.peak]} if (args.dump_outputs and y is not None) else None
    if collective:
        t = torch.tensor([el], dtype=torch.float64, device="cpu" if gloo else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    # the FIR kernel alone: a few more blocks as plain launches with HIP events around the kernel (events cannot be
    # read back from a graph replay), outside the timed region
    loc = st.local
    n_ev = 5
    ev = HipEvents(n_ev)
    loc.graph_enabled, loc._graph = False, None
    for j in range(n_ev):
        loc._events = ev.pairs[j]
        step(args.warmup + args.steps + j)
    torch.cuda.synchronize()
    loc._events = None
    fir_ms = sum(ev.elapsed_ms(j) for j in range(n_ev)) / n_ev
    audio_s = args.steps * B / fs
    if rank == 0:
        m_cols = l * host.upsampling
        algo_bytes = 4 * n_src * B + 8 * B + 4 * (2 * 187 * m_cols + 2 * 187 * 187) + 28 * n_src * (B // k + 1)
        algo_flops = 4 * l * n_src * (B + loc.halo)
        emit(json.dumps({"metric": "streaming render, x real-time", "value": audio_s / el, "unit": "x real-time",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3,
                          "higher_is_better": True, "scaling": "strong", "dtype": "f32",
                          "data": "synthetic; input block resident in the renderer's input buffer" + (" (redrawn every step, included in time)" if args.regen else "") + ", trajectories computed per block on the device (included in time)",
                          "config": {"workload": f"BASELINE config 5 shape: {n_total} sources @ {fs} Hz streamed in blocks of {B} "
                                                 f"samples, chunk {k}, subchunk {s}, {l} taps; sources sharded over {world} GPU(s), "
                                                 f"one gather per block; {args.steps} blocks = {audio_s:.0f} s of audio", "block": B},
                          "source_samples_per_s": n_total * B * args.steps / el,
                          "ps_per_source_sample": el / (n_total * B * args.steps) * 1e12,
                          "hour_of_audio_seconds": 3600.0 / (audio_s / el), "peak": st.peak,
                          "collective_path": (f"{dist.get_backend()} world_size={world}" if collective else None),
                          "roofline": {"bound": "hbm", "bound_actual": "fp32 VALU (see the scene line)",
                                       "achieved": algo_bytes / (fir_ms / 1e3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                       "frac": algo_bytes / (fir_ms / 1e3) / 1e9 / HBM_PEAK_GBS, "traffic": None,
                                       "kernel": bas._hip.lib().bas_render_fused_kernel_name(n_src, B + loc.halo, k, s, l).decode(),
                                       "kernel_ms": fir_ms, "algorithmic_bytes": algo_bytes,
                                       "note": f"algorithmic bytes of one block on this GPU ({n_src} sources): inputs once, stereo "
                                               f"block once, table, 28 B per chunk boundary; the kernel also re-reads a "
                                               f"{loc.halo}-sample halo per source.  kernel_ms: HIP events around the FIR kernel in "
                                               f"{n_ev} plain-launch blocks behind the timed region (the timed blocks are graph replays)"},
                          "valu": {"achieved": algo_flops / (fir_ms / 1e3) / 1e12, "peak": FP32_VALU_PEAK_TF, "unit": "TFLOP/s",
                                   "frac": algo_flops / (fir_ms / 1e3) / 1e12 / FP32_VALU_PEAK_TF},
                          "out_block_shape": list(y.shape),
                          **({"dumped_outputs": dump_outputs(args.dump_outputs, dumped)} if dumped is not None else {})}))
    if collective:
        dist.destroy_process_group()


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks through torch.distributed.run and relay
    rank 0's line.  Nothing here touches the GPU (device_count() does not initialise it), the ranks are child
    processes.  On a box with fewer devices than ranks this becomes the one-device rehearsal (all ranks on
    cuda:0, gather staged through the host under gloo; the line says so) - at most 4 ranks."""
    import torch
    env = dict(os.environ)
    n_dev = torch.cuda.device_count()
    if n_dev < args.gpus:
        if args.gpus > 4:
            print(f"bench.py: {args.gpus} ranks asked, {n_dev} device(s) visible: refusing to stack more than 4 "
                  f"ranks on one device", file=sys.stderr)
            return 2
        env["BAS_BENCH_ONE_DEVICE"] = "1"
        env["BAS_BENCH_BACKEND"] = "gloo"
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
    for line in r.stdout.splitlines():                       # the launcher may add lines of its own: relay the JSON only
        if line.lstrip().startswith("{"):
            print(line, flush=True)
    return r.returncode


def root_weight(args, world):
    """--root-weight as a number (see its help text)."""
    if world == 1:
        return 1.0
    if args.root_weight == "auto":
        if args.sources < 16 * world:                        # (toy scenes: the fixed costs are not what the split is about)
            return 1.0
        return max(0.5, 1.0 - 6.0 * (world - 1) / args.sources)
    return float(args.root_weight)


class Scene:
    """One rank's share of a scene, resident in HBM, and the step that renders it."""

    def __init__(self, args, bas, dev, world, rank, scaling, tbl, host_u):
        import numpy as np
        import torch
        from binaural_audio_synthesis_amd import _hip
        self.args, self.bas, self.dev, self.world, self.rank, self.scaling = args, bas, dev, world, rank, scaling
        self.tbl = tbl
        n = int(round(args.seconds * FS))
        k, s, l = args.chunk, args.subchunk, args.taps
        if scaling == "strong":                                  # one scene, sources split over the ranks
            self.root_weight = root_weight(args, world)
            mine = bas.distributed.shard_sources(args.sources, world, rank, root_weight=self.root_weight)
            n_src, first_src, total_src = len(mine), mine.start, args.sources
        else:                                                    # every rank its own args.sources sources
            n_src, first_src, total_src = args.sources, rank * args.sources, args.sources * world
        self.n, self.n_src, self.total_src = n, n_src, total_src
        self.in_length = in_length = -(-n // k) * k
        self.t_out = t_out = in_length + l - 1
        self.n_q = n_q = in_length // k + 1
        gen = torch.Generator(device=dev).manual_seed(1000 + rank + (17 if scaling == "weak" else 0))
        self.x = torch.zeros((n_src, in_length), dtype=torch.float32, device=dev)
        self.x[:, :n] = (torch.rand((n_src, n), generator=gen, device=dev) * 2 - 1) * (1.0 / total_src)
        tq = np.arange(0, in_length + 1, k, dtype=np.float64)
        elev = np.empty((n_src, n_q))
        azim = np.empty((n_src, n_q))
        for i in range(n_src):
            elev[i], azim[i] = source_trajectory(bas.synth, first_src + i, total_src, n)(tq)
        # the trajectories are INPUTS of the timed step (device float64), not precomputed parameters
        self.elev = torch.from_numpy(elev).to(dev)
        self.azim = torch.from_numpy(azim).to(dev)
        self.idx = torch.empty((n_src * n_q, 4), dtype=torch.int32, device=dev)
        self.w = torch.empty((n_src * n_q, 3), dtype=torch.float64, device=dev)
        lib = _hip.lib()
        self.ws = _hip.new_workspace(max(lib.bas_render_workspace_bytes(n_src, in_length, k, s, l),
                                         lib.bas_render_fused_workspace_bytes(n_src, in_length, k, s, l)), dev)
        self.ws_mix = _hip.new_workspace(lib.bas_mix_workspace_bytes(), dev)
        self.ws_i = torch.empty((lib.bas_interp2d_workspace_bytes(n_src * n_q),), dtype=torch.uint8, device=dev)
        self.y = torch.empty((2, t_out), dtype=torch.float32, device=dev)
        self.parts = torch.empty((world, 2, t_out), dtype=torch.float32, device=dev) if (world > 1 and rank == 0) else None
        self.y_final = torch.empty((2, t_out), dtype=torch.float32, device=dev)
        self.peak = torch.empty((1,), dtype=torch.float32, device=dev)
        self.fused = False if args.unfused else None             # ablation: --unfused forces interp2d + render_mix
        self.fused_used = bool(lib.bas_render_fused_supported(n_src, in_length, k, s, l)) and self.fused is not False
        self.kernel = (lib.bas_render_fused_kernel_name(n_src, in_length, k, s, l).decode() if self.fused_used
                       else lib.bas_render_kernel_name(n_src, in_length, k, s, l).decode())
        self.host_u = host_u

    def render_into(self, y_buf, events, normalize="none", plans=None):
        """a3 -> plans -> (chunk IRs +) FIR + mix + peak [+ the peak rule in the last kernel's tail], all on the
        current stream.  Returns the peak tensor (max|y| before the rule).  plans = a buffer plan_into() has filled
        (on another stream, ordered before this call by the caller): only the FIR half is launched."""
        bas, a = self.bas, self.args
        return bas.apply_hrtf.render_angles_device(self.x, a.chunk, a.subchunk, self.tbl, self.elev, self.azim,
                                                   normalize=normalize, out=y_buf, events=events, ws=self.ws,
                                                   ws_plans=self.ws_i if plans is None else plans, fused=self.fused,
                                                   params=(self.idx, self.w), plans_ready=plans is not None)[1]

    def plan_into(self, plans):
        """The first launch of the step alone (angles -> a3 -> read plans), on the current stream."""
        self.bas.apply_hrtf.plan_angles_device(self.tbl, self.elev, self.azim, plans)


def self_check(sc, y_dev, peak_dev, n_windows=2):
    """Compare windows of the timed path's own output (device a3 -> plans -> fused FIR -> reduce -> peak rule) with
    the oracle's float64 definition (oracle.render_window over EVERY source of this GPU) - outside the timed
    region.  Returns the worst norm-relative error (max|got - want| / max|y|)."""
    import numpy as np
    from oracle import bas_oracle as orc
    a = sc.args
    k, s, l = a.chunk, a.subchunk, a.taps
    host_tbl = sc.bas.synth.make_table("consistent", 0).truncated(l)
    elev, azim = sc.elev.cpu().numpy(), sc.azim.cpu().numpy()
    scale = float(y_dev.abs().max())
    peak = float(peak_dev.reshape(-1)[0])                    # max|mix| before the peak rule (apply_hrtf.py:462-464)
    mid = (sc.t_out // 2 // k) * k                           # a chunk boundary in the middle, and the very beginning
    windows = [(mid - 16, mid + 16), (l - 8, l + 24)][:n_windows]
    worst = 0.0
    for n0, n1 in windows:
        m0, m1 = max(n0 - l + 1, 0), min(n1, sc.in_length)
        xw = sc.x[:, m0:m1].double().cpu().numpy()
        want = np.zeros((2, n1 - n0))
        for i in range(sc.n_src):
            cache = {}

            def ir_of(c, i=i, cache=cache):
                c = min(c, sc.n_q - 1)
                if c not in cache:
                    cache[c] = orc.interp2d(host_tbl, elev[i, c], azim[i, c])
                return cache[c]
            want += orc.render_window(xw[i], m0, k, s, ir_of, l, n0, n1)
        if peak > 1.0:
            want /= peak
        got = y_dev[:, n0:n1].double().cpu().numpy()
        worst = max(worst, float(np.abs(got - want).max()) / (scale if scale > 0 else 1.0))
    return worst


def run_scene(args, bas, dev, world, rank, backend, scaling, tbl, host_u, with_events, collective):
    """Warm up, time exactly args.steps steps (barrier + synchronize on both sides, max over ranks) and return
    (elapsed seconds, scene, FIR kernel milliseconds per launch or None, overlap flag, extra JSON fields)."""
    import torch
    import torch.distributed as dist
    from binaural_audio_synthesis_amd import _hip
    sc = Scene(args, bas, dev, world, rank, scaling, tbl, host_u)
    t_out = sc.t_out
    info = {}
    # auto: graphs where the step is a chain of short launches - the collective path, and scenes small enough for the
    # four-wave kernel (one source x 10 s: 33 us as plain launches, 28.5 us replayed: three kernels of 25 us together)
    use_graph = args.graph == "on" or (args.graph == "auto" and (collective or sc.kernel.startswith("bas_render_fq_kernel")))
    # events live inside the timed steps only while those are plain launches; under a graph the FIR kernel is timed
    # in eager steps of its own right after the timed region (same process, same clocks)
    ev = HipEvents(args.steps) if with_events else None

    # --overlap-plans on (A/B only - it lost, see the option's help): the plans of step i+1 (one launch, ~9 us, latency-bound) are computed on a second stream beside the
    # FIR of step i - a rank's share of a multi-GPU scene leaves CUs free (247 workgroups at 32 sources), and the plans
    # depend on the trajectories alone.  Plan buffers are double-buffered; two events per buffer order plan -> FIR -> the
    # next plan into the same buffer.  Every timed step still contains one plan launch and one FIR (the first step's
    # plans come from the warm-up, the last step computes the plans of a step that is not rendered).
    pipe = args.overlap_plans == "on" and sc.fused_used
    if pipe:
        side = torch.cuda.Stream(dev)
        plan_bufs = [sc.ws_i, torch.empty_like(sc.ws_i)]
        plan_done = [torch.cuda.Event(), torch.cuda.Event()]
        fir_done = [torch.cuda.Event(), torch.cuda.Event()]
        pcount = [0]
        with torch.cuda.stream(side):                         # prime: the plans of the first step
            sc.plan_into(plan_bufs[0])
            plan_done[0].record(side)
        info["overlap_plans"] = ("the read plans of step i+1 (bas_interp2d_plan_angles_f32) are computed on a second "
                                 "stream beside the FIR of step i; double-buffered, event-ordered")

    def mix_on_root(parts_buf):                             # fixed-order sum + max|y| + peak rule: ONE launch
        _hip.call("bas_mix_finish_f32", _hip.ptr(parts_buf), world, 2 * t_out, 2 * t_out, _hip.ptr(sc.y_final),
                  _hip.ptr(sc.peak), 1, _hip.ptr(sc.ws_mix), sc.ws_mix.numel(), _hip.current_stream(dev))

    def render_single(y_buf, events=None, plans=None):      # the whole N = 1 step: render with the peak rule in its tail
        sc.last_peak = sc.render_into(y_buf, events, normalize="mix", plans=plans)

    # N > 1: the gather of step i travels (RCCL stream, xGMI) while step i+1 renders; y and the root's receive
    # buffer are double-buffered, the root sums step i right after it has launched step i+1's gather.  Every
    # collective is issued by all ranks in step order; drain() inside the timed region completes the last one.
    # BAS_BENCH_SYNC_GATHER=1 restores gather-then-continue.
    overlap = collective and os.environ.get("BAS_BENCH_SYNC_GATHER", "0") != "1"
    ys = [sc.y, torch.empty_like(sc.y)] if overlap else [sc.y]
    if collective and sc.parts is None and rank == 0:
        sc.parts = torch.empty((world, 2, t_out), dtype=torch.float32, device=dev)
    parts2 = [sc.parts, torch.empty_like(sc.parts)] if (overlap and rank == 0) else [sc.parts]
    inflight = [None, None]
    counter = [0]

    # ---- the render part of a step as ONE hipGraph (per output buffer): a3 -> plans -> FIR -> reduce [-> peak rule]
    graphs = {}

    def fir_half(b, p, events=None):
        """The step behind its plans (pipelined form): FIR + reduce [+ rule] into ys[b] from plan_bufs[p]."""
        if use_graph and events is None and (b, p) in graphs:
            graphs[(b, p)].replay()
        elif collective:
            sc.render_into(ys[b], events, plans=plan_bufs[p])
        else:
            render_single(ys[b], events, plans=plan_bufs[p])

    def render(b, events=None):
        """Render this rank's sources into ys[b] (collective path: un-normalised partial mix; N = 1: with the peak
        rule), replaying the captured graph when there is one and no events are asked for."""
        if pipe:
            p = pcount[0] & 1
            pcount[0] += 1
            main = torch.cuda.current_stream(dev)
            main.wait_event(plan_done[p])                     # (computed beside the previous step's FIR)
            fir_half(b, p, events)
            fir_done[p].record(main)
            side.wait_event(fir_done[p ^ 1])                  # the FIR that read the other buffer (previous step) is over
            with torch.cuda.stream(side):
                sc.plan_into(plan_bufs[p ^ 1])
                plan_done[p ^ 1].record(side)
        elif use_graph and events is None and b in graphs:
            graphs[b].replay()
        elif collective:
            sc.render_into(ys[b], events)
        else:
            render_single(ys[b], events)

    def capture_graphs():
        for b in range(len(ys)):
            render(b)                                         # eager first: code objects, workspaces
        torch.cuda.synchronize(dev)
        for key in ([(b, p) for b in range(len(ys)) for p in (0, 1)] if pipe else range(len(ys))):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                if pipe:
                    fir_half(key[0], key[1])                  # (not in `graphs` yet: plain launches, recorded)
                elif collective:
                    sc.render_into(ys[key], None)
                else:
                    render_single(ys[key], None)
            graphs[key] = g

    def launch_gather(b, async_op):
        if backend == "nccl":
            work = dist.gather(ys[b], gather_list=list(parts2[b].unbind(0)) if rank == 0 else None, dst=0,
                               async_op=async_op)
            return (work, None)
        y_host = ys[b].cpu()                              # rehearsal only: gloo moves host memory
        host_parts = [torch.empty_like(y_host) for _ in range(world)] if rank == 0 else None
        return (dist.gather(y_host, gather_list=host_parts, dst=0, async_op=async_op), host_parts)

    def finish_gather(b):
        if inflight[b] is None:
            return
        work, host_parts = inflight[b]
        if work is not None:
            work.wait()                                   # nccl: the current stream waits, the host does not
        if rank == 0:
            if host_parts is not None:
                parts2[b].copy_(torch.stack(host_parts))
            mix_on_root(parts2[b])
        inflight[b] = None

    def step_single(i_event=None):
        render(0, None if (ev is None or i_event is None) else ev.pairs[i_event])

    def step_sync(i_event=None):
        render(0, None if (ev is None or i_event is None) else ev.pairs[i_event])
        inflight[0] = launch_gather(0, False)
        finish_gather(0)

    def step_overlapped(i_event=None):
        b = counter[0] & 1
        counter[0] += 1
        finish_gather(b)                                  # the collective that read ys[b] two steps ago is done
        render(b, None if (ev is None or i_event is None) else ev.pairs[i_event])
        inflight[b] = launch_gather(b, True)
        if rank == 0:
            finish_gather(b ^ 1)                          # previous step: its gather ran beside this render

    def drain():
        if overlap:
            b = counter[0] & 1
            finish_gather(b)                              # older one first
            finish_gather(b ^ 1)

    step = step_single if not collective else (step_overlapped if overlap else step_sync)

    def fence():
        drain()
        torch.cuda.synchronize(dev)
        if collective:
            dist.barrier()
        torch.cuda.synchronize(dev)

    # ---- cold figure (N = 1 only): what a single render sees on a GPU that has not been loaded yet
    if not collective and with_events and args.settle_ms > 0:
        step()                                               # code objects and workspaces only
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(20):
            step()
        torch.cuda.synchronize(dev)
        info["cold"] = {"ms_per_step": (time.perf_counter() - t0) / 20 * 1e3,
                        "meaning": "the first 20 steps after one untimed step, before the settle phase: the clock "
                                   "governor has not settled (profiles/r02_warmup_series.txt)"}
    if use_graph:
        capture_graphs()
    if args.settle_ms > 0:                                  # untimed: let the clock governor reach its steady state
        t_end = time.perf_counter() + args.settle_ms / 1e3
        while True:
            for _ in range(10):
                step()
            torch.cuda.synchronize(dev)
            go_on = torch.tensor([1.0 if time.perf_counter() < t_end else 0.0], dtype=torch.float64,
                                 device="cpu" if backend != "nccl" else dev)
            if collective:                                   # every rank must leave the loop at the same step count
                dist.all_reduce(go_on, op=dist.ReduceOp.MIN)
            if float(go_on.item()) == 0.0:
                break
    for _ in range(args.warmup):
        step()
    fence()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(None if use_graph else i)
    fence()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and with_events and rank == 0:      # the last timed step's (y, peak), before anything below renders again
        y_last, peak_last = (sc.y_final, sc.peak) if collective else (ys[0], sc.last_peak)
        sc.dumped = {"y": y_last.cpu().numpy(), "peak": peak_last.reshape(-1)[:1].cpu().numpy()}
    if collective:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if backend != "nccl" else dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    fir_ms = None
    if ev is not None:
        if use_graph:                                        # eager steps with events, right behind the timed region
            for i in range(args.steps):
                if collective:
                    sc.render_into(ys[0], ev.pairs[i])
                else:
                    render_single(ys[0], ev.pairs[i])
            torch.cuda.synchronize(dev)
        per = [ev.elapsed_ms(i) for i in range(args.steps)]
        fir_ms = sum(per) / len(per)
    info["graph"] = ("render step replayed as one hipGraph per step; the FIR kernel was timed with HIP events in "
                     f"{args.steps} eager steps right behind the timed region") if use_graph else "plain launches"
    if collective:
        info["collective_path"] = f"{backend} world_size={world}" + (" (--force-pg: one rank, real communicator)" if world == 1 else "")
    if collective and os.environ.get("BAS_BENCH_CHECK") == "1":   # rehearsal: the pipelined mix equals the synchronous one
        pipelined = sc.y_final.clone() if rank == 0 else None
        step_sync()
        torch.cuda.synchronize(dev)
        if rank == 0:
            assert torch.equal(pipelined, sc.y_final), "overlapped gather changed the mix"
            print("check: pipelined mix == synchronous mix", file=sys.stderr, flush=True)
            if world == 1:                                   # one rank: the collective path must reproduce the plain step
                plain = torch.empty_like(sc.y)
                render_single(plain)
                torch.cuda.synchronize(dev)
                assert torch.equal(plain, sc.y_final), "collective path at world_size 1 differs from the plain N = 1 step"
                print("check: collective path at world_size 1 == plain step, bit for bit", file=sys.stderr, flush=True)
    _hip.check_status(sc.ws, dev)                             # device-side error record of the workspace (outside the timed region)
    if with_events and rank == 0 and not args.no_self_check and scaling == args.scaling:
        y_chk = sc.y_final if collective else sc.y
        if not collective or world == 1:                     # (N > 1: the root's mix holds other ranks' sources too)
            if not collective:
                render_single(sc.y)                           # (a fresh eager step: under a graph the peak tensor is the pool's)
                torch.cuda.synchronize(dev)
            info["self_check_rel_err"] = self_check(sc, y_chk, sc.peak if collective else sc.last_peak)
            info["self_check"] = ("2 windows of the timed path's output (all sources of this GPU) against "
                                  "oracle.render_window, float64; bound 1e-5")
            assert info["self_check_rel_err"] <= 1e-5, f"self check failed: {info['self_check_rel_err']:.3e}"
    return elapsed, sc, fir_ms, overlap, info


_REAL_STDOUT = None


def claim_stdout():
    """stdout carries exactly ONE JSON line (the contract).  Libraries write there too - RCCL prints a version banner
    on the root rank when its first communicator comes up - so file descriptor 1 is pointed at stderr for the life
    of the process and the line goes out through a saved duplicate of the real stdout."""
    global _REAL_STDOUT
    if _REAL_STDOUT is None:
        sys.stdout.flush()
        _REAL_STDOUT = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)


def emit(line):
    out = _REAL_STDOUT if _REAL_STDOUT is not None else sys.stdout
    out.write(line + "\n")
    out.flush()


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    claim_stdout()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE={world}"
    # The CPU leg starts worker PROCESSES: it runs first, before this process has made any GPU call (anything
    # exec-shaped belongs in front of the first HIP call on this pool), and it does not depend on the GPU run.
    cpu_line = None
    traffic_pmc, traffic_err = None, None
    if args.mode == "scene" and world == 1 and not args.no_traffic and not args.force_pg and args.lib is None:
        traffic_pmc, traffic_err = measure_traffic(args)
    if args.mode == "scene" and world == 1 and not args.no_cpu_baseline:
        n_cpu = int(round(args.seconds * FS))
        cpu_line = cpu_baseline(args, n_cpu, -(-n_cpu // args.chunk) * args.chunk + args.taps - 1)
    if args.mode == "stream":
        return stream_mode(args)
    import torch
    import torch.distributed as dist
    import binaural_audio_synthesis_amd as bas
    from binaural_audio_synthesis_amd import _hip
    if args.lib:
        _hip.set_library(os.path.abspath(args.lib))

    # rehearsal knobs (a 1-GPU box; self_launch sets them when devices are missing): BAS_BENCH_ONE_DEVICE=1 puts
    # every rank on cuda:0, BAS_BENCH_BACKEND=gloo stages the gather through host memory.
    rehearsal = os.environ.get("BAS_BENCH_ONE_DEVICE") == "1"
    if rehearsal:
        local_rank = 0
    backend = os.environ.get("BAS_BENCH_BACKEND", "nccl")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    collective = world > 1 or args.force_pg                  # the step ends in the gather + fixed-order sum
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    elif args.force_pg:                                      # one rank, real RCCL communicator
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = "nccl"
        dist.init_process_group("nccl", world_size=1, rank=0, device_id=dev)

    k, s, l = args.chunk, args.subchunk, args.taps
    host = bas.synth.make_table("consistent", 0).truncated(l)
    tbl = bas.irs_and_delaydiffs(host.upsampling, host.diffs_left, host.diffs_right, host.irs_left,
                                 host.irs_right, device=dev)
    scaling = args.scaling                                   # (one GPU: the whole scene either way)
    elapsed, sc, fir_ms, overlap, info = run_scene(args, bas, dev, world, rank, backend, scaling, tbl, host.upsampling,
                                                   True, collective)
    extra = {}
    if world > 1 and not args.no_extra:
        other = "weak" if scaling == "strong" else "strong"
        del sc.x, sc.parts                                   # free the first scene's big buffers
        e2, sc2, _, _, _ = run_scene(args, bas, dev, world, rank, backend, other, tbl, host.upsampling, False, collective)
        scenes2 = world if other == "weak" else 1
        extra[other] = {"value": scenes2 * sc2.t_out * args.steps / e2, "unit": "stereo samples/s",
                        "ms_per_step": e2 / args.steps * 1e3, "sources_per_gpu": sc2.n_src,
                        "scene_sources": sc2.total_src,
                        "x_realtime": (sc2.n / FS) * scenes2 / (e2 / args.steps),
                        "meaning": "every GPU renders its own --sources sources; value counts 256-source scene "
                                   "equivalents" if other == "weak" else "ONE --sources-source scene sharded over the GPUs"}

    if rank == 0:
        n, n_src, in_length, t_out, n_q = sc.n, sc.n_src, sc.in_length, sc.t_out, sc.n_q
        ms_per_step = elapsed / args.steps * 1e3
        # weak: 256-source-scene equivalents per second; strong: the one scene's stereo samples per second
        scenes = world if scaling == "weak" else 1
        value = scenes * t_out * args.steps / elapsed
        # algorithmic bytes of one FIR launch: inputs once, stereo mix once,
        # table once, 28 B of parameters per chunk IR
        m_cols = l * host.upsampling
        algo_bytes = 4 * n_src * in_length + 8 * t_out + 4 * (2 * 187 * m_cols + 2 * 187 * 187) + 28 * n_src * n_q
        algo_flops = 4 * l * n_src * in_length            # 2 ears x L FMA per source-sample
        fir_s = fir_ms / 1e3
        # the 2-parallel fast FIR row step (3/4 of the multiplications) serves subchunks that are multiples of 32,
        # in the fused kernel and in the stored-IR hd kernel; the other kernels execute the direct form
        fast_fir = s % 32 == 0 and (sc.fused_used or sc.kernel == "bas_render_hd_kernel")
        # executed packed multiply-adds per 128-tap unit against the direct form's 4096 + 256 (FIR + crossfade forming): level 1 of
        # the fast FIR 3136 + 384; the unit blocks of the split-role kernel (level 1.5: the product P split once more) 2912 + 448
        exec_ratio = ((2912 + 448) if sc.kernel in ("bas_render_fs_kernel<128>", "bas_render_fs_kernel<104>") else (3136 + 384)) / (4096 + 256)
        traffic, traffic_source, traffic_parts = None, None, None
        # what the FIR kernel must move, by part (bytes per launch): x windows (each (tile, source) unit reads its tile + a
        # 128-sample halo), read plans (288 B per chunk IR, tile's chunks + 2 per unit), the packed table (once per XCD L2 at
        # least), the slab parts it writes; y and the plans' own write belong to the reduce / plan kernels
        if sc.fused_used:
            n_tiles = -(-t_out // 8192)
            traffic_parts = {"x": 4 * n_src * n_tiles * (8192 + 128), "plans": 288 * n_src * n_tiles * (8192 // k + 2),
                             "table_x8_xcd": 8 * 4 * (2 * 187 * 8 * (l + 4)), "slabs_written": None, "y": 0}
        if traffic_pmc is not None:
            fk = [kn for kn in traffic_pmc["FETCH_SIZE"] if "bas_render_f" in kn or "bas_render_hd" in kn]
            if fk:
                f_kb = traffic_pmc["FETCH_SIZE"][fk[0]]
                w_kb = traffic_pmc["WRITE_SIZE"].get(fk[0], 0.0)
                # gfx950: FETCH_SIZE counts half of the bytes of wide coalesced streaming reads (the x windows, the plans);
                # the table gathers are L2 hits.  x and plans are what is doubled; the rest of FETCH_SIZE is taken as it is.
                traffic = int(2 * f_kb * 1024 + w_kb * 1024)
                if traffic_parts is not None:
                    traffic_parts["slabs_written"] = int(w_kb * 1024)
                traffic_source = (f"measured in this invocation: rocprofv3 --pmc FETCH_SIZE ({f_kb / 1024:.1f} MB) and --pmc "
                                  f"WRITE_SIZE ({w_kb / 1024:.1f} MB) of {fk[0]} in two child runs of 3 steps; gfx950 correction "
                                  "(MI355X_MICROARCH.md: FETCH_SIZE x 2 for wide streaming reads) applied to all of FETCH_SIZE: an "
                                  "upper bound")
                info["traffic_by_kernel_KB"] = {c: {kn: round(v, 1) for kn, v in d.items()} for c, d in traffic_pmc.items()}
        elif traffic_err:
            info["traffic_error"] = traffic_err
        tpath = os.path.join(ROOT, "profiles", "fir_hbm_traffic.json")
        if traffic is None and os.path.exists(tpath):
            with open(tpath) as f:
                rec = json.load(f)
            if rec.get("workload") == f"{n_src}x{n}@K{k}S{s}L{l}" and rec.get("fused", False) == sc.fused_used:
                traffic = rec.get("bytes_per_launch")
                traffic_source = "profiles/fir_hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this " \
                                 "workload, gfx950 correction applied; replayed, not measured in this run)"
        out = {
            "metric": "stereo samples/sec, 256 concurrent moving sources @44.1kHz mixed to one stereo pair "
                      "(x real-time in x_realtime)",
            "value": value, "unit": "stereo samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": scaling, "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "settle": f"{args.settle_ms:g} ms of untimed steps before the {args.warmup} warm-up steps (clock governor)",
            "config": {"workload": f"BASELINE config 4: {sc.total_src} moving sources x {args.seconds:g} s @ {FS} Hz mono "
                                   f"-> 1 stereo mix; chunk {k}, subchunk {s}, {l}-tap HRIRs (U=8, 187 directions), "
                                   f"spiral/askew-circle trajectories given as (elev, azim) per chunk boundary on the "
                                   f"device; step = angles->parameters (a3) + read plans + "
                                   + ("fused chunk-IR evaluation/FIR/overlap-add/mix" if sc.fused_used else
                                      "chunk IRs (interp2d) + FIR/overlap-add/mix")
                                   + f" + peak rule (in the last kernel's tail); {n_src} sources on this GPU, {world} GPU(s)",
                       "sources_per_gpu": n_src, "scene_sources": sc.total_src, "samples_per_source": n, "chunk": k,
                       "subchunk": s, "taps": l, "out_samples": t_out, "fused": sc.fused_used,
                       "parallelism": f"sources sharded over {world} GPU(s), 1 gather per step" +
                                      (", travelling beside the next step's render" if overlap else "") +
                                      (f"; rank 0 (receives and sums) renders {sc.root_weight:.3f} of an equal share"
                                       if world > 1 and scaling == "strong" else "")},
            "x_realtime": (n / FS) * scenes / (elapsed / args.steps),
            "source_samples_per_s": sc.total_src * in_length * args.steps / elapsed,
            "multi_gpu_status": "no N > 1 figure of this repository is hardware-measured until the driver's SCALE run: the "
                                "builder's boxes have one GPU (the RCCL path runs there at world_size 1, --force-pg; two "
                                "ranks on one device under gloo)",
            "roofline": {"bound": "hbm", "bound_actual": "fp32 VALU at a power-limited clock (see valu; the HBM "
                         "fraction of a perfect 128-tap direct FIR tops out near 15 %)", "achieved": algo_bytes / fir_s / 1e9, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": algo_bytes / fir_s / 1e9 / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_source": traffic_source, "traffic_parts": traffic_parts,
                         "kernel": sc.kernel + (" (chunk IRs evaluated while staging)" if sc.fused_used else ""),
                         "kernel_ms": fir_ms, "algorithmic_bytes": algo_bytes},
            "valu": {"achieved": algo_flops / fir_s / 1e12, "peak": FP32_VALU_PEAK_TF, "unit": "TFLOP/s",
                     "frac": algo_flops / fir_s / 1e12 / FP32_VALU_PEAK_TF,
                     **({"executed": algo_flops * exec_ratio / fir_s / 1e12,
                         "frac_executed": algo_flops * exec_ratio / fir_s / 1e12 / FP32_VALU_PEAK_TF}
                        if fast_fir else {}),
                     "note": "the FIR is 128 flop/B: fp32-VALU bound, HBM fraction tops out near 15 %.  achieved = direct-form "
                             "arithmetic (4 L flop per source sample) per second; the row step is a 2-parallel fast FIR (its product "
                             "P split once more in the split-role kernel's unit blocks) and executes 3/4 (0.71) of those "
                             "multiplications plus forming (executed).  peak is nominal (2.4 GHz): a "
                             "bare v_pk_fma_f32 stream on random operands sustains ~122 TFLOP/s (power-limited clock; "
                             "profiles/r02_ubench_fir_pattern.txt, DESIGN.md 4.1)"},
        }
        if extra:
            out["extra"] = extra
        if rehearsal:
            out["rehearsal"] = f"{world} ranks on ONE device, gather staged through host memory ({backend}): " \
                               "a functional check of the multi-rank path, not a scaling measurement"
        out.update(info)
        if args.dump_outputs:
            out["dumped_outputs"] = dump_outputs(args.dump_outputs, sc.dumped)
        if cpu_line is not None:
            out["cpu_baseline"] = cpu_line
        emit(json.dumps(out))
    if collective:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
