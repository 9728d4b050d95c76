"""calcphase with and without a binary orbit on one device-resident list of NPH (default 1e8) MJD times: kernel ms
(CRIMP_FLAG_TIME_KERNELS) of REPS (default 5) repeats per case, after SETTLE seconds (default 0.3, bench.py's) of the
same call untimed.

  (a) no binary: 1e2259.par on this build, and -- with PARENT_TREE=<a built checkout of the parent commit> -- on that
      tree's package and library in a fresh child process, same input (seeded);
  (b) BT at e = 0, 0.1, 0.7, 0.95;   (c) ELL1;   (d) crimp_binary_delay alone (BT e = 0.1).

Per binary case also the mean Newton iterations per photon, counted by the host twin of the device loop
(crimp_amd.binarymodels.binary_delay_host) on a 1e5 subsample of the same times. One JSON line per case; the last line
is the verdict of (a): this build's median against the parent's slowest repeat."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("CRIMP_TREE") or ROOT)  # the child of (a) imports the parent commit's package
from crimp_amd import _native as N, ops  # noqa: E402
from crimp_amd.readtimingmodel import ReadTimingModel  # noqa: E402

n = int(float(os.environ.get("NPH", 1e8)))
reps = int(os.environ.get("REPS", 5))
settle = float(os.environ.get("SETTLE", 0.3))
only_plain = os.environ.get("ONLY_PLAIN") == "1"
dev = torch.device("cuda", 0)
gen = torch.Generator(device=dev)
gen.manual_seed(7)
t = 58141.0 + torch.sort(torch.rand(n, dtype=torch.float64, device=dev, generator=gen) * 6.0).values
tot, fol = torch.empty_like(t), torch.empty_like(t)
L = N.load()
par = ReadTimingModel(os.path.join(ROOT, "tests", "golden", "1e2259.par")).readfulltimingmodel()[0]


def bt(e):
    return {**par, "BINARY": "BT", "PB": 1.7, "A1": 5.0, "ECC": e, "OM": 40.0, "T0": 58100.25}


def run(name, model, call):
    t_s = time.perf_counter()
    while time.perf_counter() - t_s < settle:
        call(model)
    ms = []
    for _ in range(reps):
        call(model)
        ms.append(L.crimp_last_kernel_ms())
    row = {"case": name, "n": n, "ms": [round(v, 4) for v in ms], "median_ms": round(float(np.median(ms)), 4),
           "photons_per_s": n / (float(np.median(ms)) * 1e-3)}
    if "BINARY" in model:
        from crimp_amd.binarymodels import binary_delay_host
        sub = t[:: max(n // 100000, 1)].cpu().numpy()
        _, its = binary_delay_host(sub, model, return_iterations=True)
        row["mean_iterations"] = round(float(its.mean()), 3)
        row["max_iterations"] = int(its.max())
    print(json.dumps(row), flush=True)
    return row


def phase(model):
    ops.calcphase(t, model, total=tot, folded=fol, flags=N.FLAG_TIME_KERNELS)


def delay(model):
    ops.binary_delay(t, model, delay=tot, t_emit=fol, flags=N.FLAG_TIME_KERNELS)


here = run("a_no_binary" + ("_parent" if only_plain else ""), par, phase)
if not only_plain:
    for e in (0.0, 0.1, 0.7, 0.95):
        run("b_bt_e%g" % e, bt(e), phase)
    run("c_ell1", {**par, "BINARY": "ELL1", "PB": 0.0839, "A1": 0.0628, "TASC": 58100.25, "EPS1": 1e-5, "EPS2": -2e-5},
        phase)
    run("d_binary_delay_bt_e0.1", bt(0.1), delay)
    parent_tree = os.environ.get("PARENT_TREE")
    if parent_tree:
        del tot, fol, t
        torch.cuda.empty_cache()
        env = dict(os.environ, CRIMP_TREE=os.path.abspath(parent_tree), ONLY_PLAIN="1")
        out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True,
                             timeout=300)
        sys.stdout.write(out.stdout)
        if out.returncode != 0:
            sys.stderr.write(out.stderr[-2000:])
            sys.exit(out.returncode)
        parent = json.loads(out.stdout.strip().splitlines()[-1])
        ok = here["median_ms"] <= max(parent["ms"])
        print(json.dumps({"case": "a_verdict", "this_median_ms": here["median_ms"], "parent_slowest_ms": max(parent["ms"]),
                          "parent_median_ms": parent["median_ms"], "not_above_parent_slowest": bool(ok)}))
        sys.exit(0 if ok else 1)
