"""Measure the margins of the local error bound: run every locality case of tests/test_gpu_local_error.py
(the same scenes, the same kernels, the same checker of oracle/whole.py) and write one record per case to
profiles/local_error_margins.json - the kernel, its worst ratio |got - want| / (2^-24 scale) and where it falls, r_ref (the
float32 reference arithmetic's ratio on the same scene, computed on the CPU), the backstop c_wc, the build and the date.
Needs the GPU.

    python tools/local_error_margins.py [--out profiles/local_error_margins.json] [--cases hd-S16,quad,..]
"""
import argparse
import datetime
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _cases_module():
    spec = importlib.util.spec_from_file_location("test_gpu_local_error", os.path.join(ROOT, "tests", "test_gpu_local_error.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _build():
    """The commit the tree was built from and a hash of the shipped library."""
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                                check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        commit = None
    import binaural_audio_synthesis_amd as bas
    with open(bas._hip.lib()._name, "rb") as f:
        lib_sha = hashlib.sha256(f.read()).hexdigest()[:16]
    return {"commit": commit, "libbas_hip_sha256": lib_sha}


def runners(mod):
    """name -> a function that returns the case's records (a list of the dicts the tests check)."""
    out = {name: (lambda name=name: [mod.run_fir_case(name)]) for name in mod.FIR_CASES}
    out["render_batch"] = mod.run_batch_case
    out["stream_batch"] = mod.run_stream_batch_case
    out["stream"] = lambda: [mod.run_stream_case()]
    for Np, Lr, lag in mod.les.LATE_CASES:
        out[f"long_fir-{Np}-{Lr}-{lag}"] = lambda a=(Np, Lr, lag): [mod.run_late_case(*a)]
    for name, (fn, *a) in mod.ROW_CASES.items():
        out[name] = lambda fn=fn, a=a: [fn(*a)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_error_margins.json"))
    ap.add_argument("--cases", default=None, help="comma-separated subset of the cases (default: all)")
    args = ap.parse_args()
    import torch
    from oracle import whole
    mod = _cases_module()
    run = runners(mod)
    names = args.cases.split(",") if args.cases else list(run)
    build = _build()
    records = []
    for name in names:
        t0 = time.time()
        for r in run[name]():
            res = whole.compare_local(r["got"], r["want"], r["scale"], r["K"])
            rec = {"case": r["case"], "kernel": r["kernel"], "r_ref": r["r_ref"], "sharp_bound": mod.SHARP * r["r_ref"],
                   "c_wc": r["c_wc"]}
            if "shape" in r:
                rec["shape"] = r["shape"]
            rec.update(res)
            rec.update(passes=bool(res["finite"] and res["zeros_ok"] and res["ratio"] <= min(r["c_wc"], mod.SHARP * r["r_ref"])),
                       seconds=round(time.time() - t0, 1), build=build,
                       date=datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
                       device=torch.cuda.get_device_properties(0).gcnArchName)
            records.append(rec)
            print(f"{rec['case']:28s} {rec['kernel']:30s} ratio {rec['ratio']:.3g} r_ref {rec['r_ref']:.3g} c_wc {rec['c_wc']} at row "
                  f"{rec['ear']} n={rec['n']} (mod K {rec['n_mod_K']}, mod tile {rec['n_mod_tile']})  {rec['seconds']} s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    return 0 if all(r["passes"] for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())
