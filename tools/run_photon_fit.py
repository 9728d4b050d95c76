"""Photon-domain timing fits on the device against the CPU cost of the same likelihood (csrc/photon_fit.h):
  nll     crimp_photon_nll at N in {1e5, 1e6, 1e7} x P in {16, 64, 256}, photons resident on the device, for the
          1e2259 template with (F0, F1) free and for the glitch + wave model with (F0, GLF0D_1, WAVE1_A) free: kernel
          ms (hipEvents) and photon x vector evaluations / s
  chain   crimp_photon_mcmc, 32 walkers x STEPS (default 10000) at N = 1e5 and 1e6: kernel and wall ms, ms per step,
          and the ratio of a step to two crimp_photon_nll calls of P = 16 (a step's two half-ensembles)
  cpu     seconds per evaluation of the NumPy restatement (tests/photon_reference.py) at the same N, and the CPU time
          a chain's 32 x STEPS evaluations would take at that rate: EXTRAPOLATED, not run
  peak    with FP64_PER_EVAL=<count> (the fp64 VALU instructions per photon x vector of the compiled loop, counted
          with tools/isa_loops.py on the kernel's listing): the fraction of the fp64 vector peak the nll rate implies,
          an FMA counted as one instruction, against PEAK_FP64_GINSTR (default 39300 = 256 CUs x 64 lanes x 2.4 GHz)
REPS timed repeats (default 3) after one warm-up; SIZES / PS override the grids. One JSON line, also written to
profiles/photon_fit.json."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from crimp_amd import _native as N, ops  # noqa: E402
from crimp_amd.fit_photons import PhotonFit  # noqa: E402
from crimp_amd.readPPtemplate import readPPtemplate  # noqa: E402
from crimp_amd.readtimingmodel import ReadTimingModel  # noqa: E402
import photon_reference as R  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
reps = int(os.environ.get("REPS", 3))
steps = int(os.environ.get("STEPS", 10000))
sizes = [int(float(v)) for v in os.environ.get("SIZES", "1e5,1e6,1e7").split(",")]
ps = [int(v) for v in os.environ.get("PS", "16,64,256").split(",")]
theta = readPPtemplate(os.path.join(GOLD, "1e2259_template.txt"))
dev = torch.device("cuda:0")

par_a = ReadTimingModel(os.path.join(GOLD, "1e2259.par")).readfulltimingmodel()[2]
par_a["F0"]["flag"] = par_a["F1"]["flag"] = 1
with open(os.path.join(GOLD, "timing_model_dict.json")) as fh:
    par_w = R.flagged(json.load(fh), ["F0", "GLF0D_1"])
MODELS = {"f0f1": (par_a, ["F0", "F1"], np.array([1e-9, 1e-16])),
          "glitch_wave": (par_w, ["F0", "GLF0D_1", "WAVE1_A"], np.array([1e-9, 1e-10, 1e-4]))}


def stat(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def problem(name, n):
    par, keys, scale = MODELS[name]
    rng = np.random.default_rng(n)
    pep = par["PEPOCH"]["value"]
    fit = PhotonFit(np.sort(pep + rng.uniform(-1.0, 8.0, n)), par, theta, keys=keys)
    return fit, torch.as_tensor(fit.t, device=dev), torch.as_tensor(fit.x, device=dev), scale


def time_nll(fit, t, x, pv):
    kern = []
    for r in range(reps + 1):
        ops.photon_nll(t, x, fit.par, fit.map, fit.tpl, fit.norm, pv, flags=N.FLAG_TIME_KERNELS)
        if r:
            kern.append(N.last_kernel_times()[0])
    return stat(kern)


out = {"tile": N.photon_tile(), "reps": reps, "steps": steps, "nll": {}, "chain": {}, "cpu": {}}
for name in MODELS:
    for n in sizes:
        fit, t, x, scale = problem(name, n)
        for P in ps:
            pv = torch.as_tensor(np.random.default_rng(P).uniform(-1, 1, (P, scale.size)) * scale, device=dev)
            k = time_nll(fit, t, x, pv)
            out["nll"]["%s_n%d_p%d" % (name, n, P)] = dict(k, evals_per_s=n * P / (k["median"] * 1e-3))
        if name == "f0f1":
            # the CPU cost of one likelihood of the restatement at this N (one vector)
            tc = []
            for _ in range(3):
                t0 = time.perf_counter()
                R.nll(fit.t, fit.x, fit.parfile, theta, scale, fit.model_keys)
                tc.append(time.perf_counter() - t0)
            out["cpu"]["n%d" % n] = {"s_per_eval": min(tc), "chain_s_extrapolated": min(tc) * 32 * steps}
        if name == "f0f1" and n <= 1000000:
            rng = np.random.default_rng(1)
            p0 = torch.as_tensor(rng.uniform(-3, 3, (32, 2)) * scale, device=dev)
            lo, hi = (torch.as_tensor(s * 1e3 * scale, device=dev) for s in (-1.0, 1.0))
            wall, kern = [], []
            for r in range(2):
                t0 = time.perf_counter()
                ops.photon_mcmc(t, x, fit.par, fit.map, fit.tpl, fit.norm, p0, lo, hi, steps, 5,
                                flags=N.FLAG_TIME_KERNELS)
                wall.append((time.perf_counter() - t0) * 1e3)
                kern.append(N.last_kernel_times()[0])
            half = time_nll(fit, t, x, p0[:16].contiguous())
            per_step = kern[-1] / steps
            out["chain"]["n%d" % n] = {"wall_ms": wall[-1], "kernel_ms": kern[-1], "ms_per_step": per_step,
                                       "two_nll_p16_ms": 2 * half["median"],
                                       "step_over_two_nll": per_step / (2 * half["median"])}
if os.environ.get("FP64_PER_EVAL"):
    per = float(os.environ["FP64_PER_EVAL"])
    peak = float(os.environ.get("PEAK_FP64_GINSTR", 39300.0)) * 1e9
    out["peak"] = {"fp64_per_eval": per,
                   "fraction": {k: v["evals_per_s"] * per / peak for k, v in out["nll"].items()}}
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "photon_fit.json"), "w") as fh:
    fh.write(line + "\n")
