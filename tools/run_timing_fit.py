"""Timing-model fits on the device against the CPU cost of the same likelihood (csrc/timing_fit.h):
  nll        crimp_timing_nll, P = 4096 vectors on the 84 bundled ToAs (F0, F1 free): evaluations / s
  fittoas    the default ``fittoas -mc`` shape, 32 walkers x 10000 steps on those ToAs: wall and kernel time
  local      the local-ephemerides chains (24 walkers x 1000 steps per window) of the bundled .tim, and of a
             synthetic set of 1000 windows of 20 ToAs, each set in one launch
  cpu        seconds per evaluation of the NumPy restatement of the reference's likelihood (tests/timing_reference.py)
             on the same 84 ToAs, and the CPU time the evaluations of each run above would take at that rate
REPS timed repeats (default 5) after one warm-up. One JSON line, also written to profiles/timing_fit.json."""
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from crimp_amd import _native as N, ops  # noqa: E402
from crimp_amd import get_local_ephem as GL  # noqa: E402
from crimp_amd.fit_toas import load_toas_for_fit  # noqa: E402
from crimp_amd.readtimingmodel import ReadTimingModel  # noqa: E402
from crimp_amd.timfile import readtimfile  # noqa: E402
from crimp_amd.utilities_fittoas import DeviceFit, list_fit_keys  # noqa: E402
import timing_reference as TR  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
reps = int(os.environ.get("REPS", 5))
par, tim = os.path.join(GOLD, "1e2259.par"), os.path.join(GOLD, "ToAs_2259.tim")
model = ReadTimingModel(par).readfulltimingmodel()[2]
model["F0"]["flag"] = model["F1"]["flag"] = 1
keys = list_fit_keys(model)
toas = load_toas_for_fit(readtimfile(tim, comment="C"), model)
fit = DeviceFit(toas["ToA"], model, keys, toas["phase"], toas["phase_err_cycle"])
rng = np.random.default_rng(0)
scale = np.array([1e-10, 1e-17])


def stat(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def timed(fn):
    """(wall ms, kernel ms) of every repeat after one warm-up."""
    wall, kern = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        fn()
        w = (time.perf_counter() - t0) * 1e3
        if r:
            wall.append(w)
            kern.append(N.last_kernel_times()[0])
    return {"wall_ms": stat(wall), "kernel_ms": stat(kern)}


def chains(fits, walkers, steps):
    nd = len(keys)
    off = np.concatenate([[0], np.cumsum([f.x.size for f in fits])]).astype(np.int64)
    x, y, e = (np.concatenate([getattr(f, a) for f in fits]) for a in ("x", "y", "yerr"))
    p0 = rng.normal(0, 1, (len(fits), walkers, nd)) * scale
    lo, hi = np.full((len(fits), nd), -np.inf), np.full((len(fits), nd), np.inf)
    return lambda: ops.timing_mcmc(x, y, e, [f.fit_base for f in fits], [f.wave_base for f in fits], fits[0].map, p0,
                                   lo, hi, steps, 1, offsets=off, flags=N.FLAG_TIME_KERNELS)


out = {"reps": reps, "ntoa": int(fit.x.size)}

# CPU: the restatement of the reference's per-call likelihood
ncpu = 300
t0 = time.perf_counter()
for i in range(ncpu):
    TR.nll(fit.x, fit.y, fit.yerr, model, rng.normal(0, 1, 2) * scale, keys)
cpu_s = (time.perf_counter() - t0) / ncpu
out["cpu_s_per_eval"] = cpu_s

P = 4096
pv = rng.normal(0, 1, (1, P, 2)) * scale
r = timed(lambda: ops.timing_nll(fit.x, fit.y, fit.yerr, fit.fit_base, fit.wave_base, fit.map, pv,
                                 flags=N.FLAG_TIME_KERNELS))
r["evals_per_s_kernel"] = P / (r["kernel_ms"]["median"] * 1e-3)
r["evals_per_s_wall"] = P / (r["wall_ms"]["median"] * 1e-3)
out["nll_P4096"] = r

r = timed(chains([fit], 32, 10000))
r["evaluations"] = 32 * 10000
r["kernel_us_per_step"] = r["kernel_ms"]["median"] * 1e3 / 10000
r["cpu_s_at_measured_rate"] = cpu_s * r["evaluations"]
out["fittoas_32x10000"] = r

wins = GL.local_ephem_windows(readtimfile(tim), par)
wfits = []
for w in wins:
    m = GL.window_model(w)
    t = load_toas_for_fit(w["toas"], m)
    wfits.append(DeviceFit(t["ToA"], m, keys, t["phase"], t["phase_err_cycle"]))
r = timed(chains(wfits, GL.MCMC_WALKERS, GL.MCMC_STEPS))
r["windows"] = len(wfits)
r["evaluations"] = len(wfits) * GL.MCMC_WALKERS * GL.MCMC_STEPS
r["cpu_s_at_measured_rate"] = cpu_s * r["evaluations"]
out["local_bundled"] = r
t0 = time.perf_counter()
GL.generate_local_ephemerides(tim, par, outputfile=None, seed=1)
out["local_bundled"]["generate_local_ephemerides_wall_ms"] = (time.perf_counter() - t0) * 1e3

# synthetic campaign: 1000 windows of 20 ToAs over 90 days each
sfits = []
base = copy.deepcopy(GL.window_model(wins[0]))
for i in range(1000):
    x = np.sort(base["PEPOCH"]["value"] + rng.uniform(-45, 45, 20))
    e = rng.uniform(0.004, 0.01, 20)
    sfits.append(DeviceFit(x, base, keys, rng.normal(0, e), e))
r = timed(chains(sfits, GL.MCMC_WALKERS, GL.MCMC_STEPS))
r["windows"] = len(sfits)
r["evaluations"] = len(sfits) * GL.MCMC_WALKERS * GL.MCMC_STEPS
r["kernel_us_per_step"] = r["kernel_ms"]["median"] * 1e3 / GL.MCMC_STEPS
r["cpu_s_at_measured_rate"] = cpu_s * r["evaluations"]
out["local_synthetic_1000"] = r

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "timing_fit.json"), "w") as fh:
    json.dump(out, fh, indent=1)
    fh.write("\n")
print(json.dumps(out), flush=True)
