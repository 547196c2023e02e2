"""Measure the margins of the whole-output checks: run every case of tests/test_gpu_whole_output.py (the same scenes, the
same kernels, the same float64 checker functions of oracle/whole.py) and write one record per case to
profiles/whole_output_margins.json - the kernel, the worst norm-relative error and where it falls, the 99.99th percentile
of |err| / peak, the samples checked, the build and the date.  Needs the GPU.

    python tools/whole_output_margins.py [--out profiles/whole_output_margins.json] [--cases bench_L128,sparse,..]
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
    spec = importlib.util.spec_from_file_location("test_gpu_whole_output",
                                                  os.path.join(ROOT, "tests", "test_gpu_whole_output.py"))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whole_output_margins.json"))
    ap.add_argument("--cases", default=None, help="comma-separated subset of the cases (default: all)")
    args = ap.parse_args()
    import torch
    mod = _cases_module()
    names = args.cases.split(",") if args.cases else list(mod.CASES)
    build = _build()
    records = []
    for name in names:
        t0 = time.time()
        rec = mod.run_case(name)
        rec = {k: v for k, v in rec.items() if k not in ("got", "want")}
        rec.update(case=name, bound=mod.REL, passes=bool(rec["rel"] <= mod.REL), seconds=round(time.time() - t0, 1),
                   build=build, date=datetime.datetime.now(datetime.timezone.utc).isoformat(timespec="seconds"),
                   device=torch.cuda.get_device_properties(0).gcnArchName)
        records.append(rec)
        print(f"{name:14s} {rec['kernel']:30s} rel {rec['rel']:.3e} p99.99 {rec['p9999']:.3e} at ear {rec['ear']} "
              f"n={rec['n']} (mod K {rec['n_mod_K']}, mod tile {rec['n_mod_tile']})  {rec['seconds']} s", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    return 0 if all(r["passes"] for r in records) else 1


if __name__ == "__main__":
    sys.exit(main())
