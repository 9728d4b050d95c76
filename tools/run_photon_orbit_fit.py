"""Photon-domain orbit fits on the device (csrc/photon_orbit_fit.h) beside what they are built from:
  nll     crimp_photon_orbit_nll at N in {1e5, 1e6, 1e7} x P in {16, 64, 256}, photons resident on the device, under
          the 1e2259 model and template with a BT (e = 0.7) and an ELL1 orbit, (F0, F1) free alone (`spin`) and with
          five orbital keys added (`orbit`): kernel ms (hipEvents, the prologue kernel inside), photon x vector
          evaluations / s
  free    crimp_photon_nll on the same photons without BINARY, (F0, F1) free, same N x P: the binary-free likelihood
  delay   crimp_binary_delay on the same photons: the solve alone, photons / s
  ratio   per case: rate / binary-free rate, and rate / solve rate
  chain   crimp_photon_orbit_mcmc, 32 walkers x STEPS (default 10000) at N = 1e5, seven keys free: kernel and wall ms,
          ms per step, and the ratio of a step to two likelihood calls of P = 16
  cpu     seconds per evaluation of the NumPy twin (tests/photon_orbit_reference.py) at N <= 1e6
REPS timed repeats (default 3, the median is reported) after one warm-up; SIZES / PS override the grids. One JSON line,
also written to profiles/photon_orbit_fit.json."""
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
from crimp_amd.fit_photons_orbit import PhotonOrbitFit  # noqa: E402
from crimp_amd.readPPtemplate import readPPtemplate  # noqa: E402
from crimp_amd.readtimingmodel import ReadTimingModel  # noqa: E402
import binary_reference as B  # noqa: E402
import photon_orbit_reference as PO  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
reps = int(os.environ.get("REPS", 3))
steps = int(os.environ.get("STEPS", 10000))
sizes = [int(float(v)) for v in os.environ.get("SIZES", "1e5,1e6,1e7").split(",")]
ps = [int(v) for v in os.environ.get("PS", "16,64,256").split(",")]
theta = readPPtemplate(os.path.join(GOLD, "1e2259_template.txt"))
dev = torch.device("cuda:0")

spin = ReadTimingModel(os.path.join(GOLD, "1e2259.par")).readfulltimingmodel()[2]
spin["F0"]["flag"] = spin["F1"]["flag"] = 1
pep = spin["PEPOCH"]["value"]
ORBITS = {"bt_e07": ["PB", "A1", "T0", "ECC", "OM"], "ell1": ["PB", "A1", "TASC", "EPS1", "EPS2"]}
SCALE = {"F0": 1e-9, "F1": 1e-16, "PB": 1e-8, "A1": 1e-6, "T0": 1e-7, "TASC": 1e-7, "ECC": 1e-7, "OM": 1e-5,
         "EPS1": 1e-8, "EPS2": 1e-8}


def model(orbit):
    """The 1e2259 spin model with a fixture orbit under it, its epoch moved next to the data."""
    src = B.load_binary()["bt_e07" if orbit == "bt_e07" else "ell1_amxp"].tm
    par = dict(spin)
    for k, v in src.items():
        if k in PO.O.ORBITAL or k == "BINARY":
            par[k] = {"value": v, "flag": None if k == "BINARY" else 0}
    par["T0" if orbit == "bt_e07" else "TASC"]["value"] = pep - 0.37
    return par


def stat(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def timed(call):
    kern = []
    for r in range(reps + 1):
        call()
        if r:
            kern.append(N.last_kernel_times()[0])
    return stat(kern)


out = {"tile": N.photon_tile(), "reps": reps, "steps": steps, "nll": {}, "free": {}, "delay": {}, "ratio": {},
       "chain": {}, "cpu": {}}
for n in sizes:
    rng = np.random.default_rng(n)
    tm = np.sort(pep + rng.uniform(-1.0, 8.0, n))
    t = torch.as_tensor(tm, device=dev)
    free = PhotonFit(tm, spin, theta, keys=["F0", "F1"])
    xf = torch.as_tensor(free.x, device=dev)
    for P in ps:
        pv = torch.as_tensor(np.random.default_rng(P).uniform(-1, 1, (P, 2)) * [SCALE["F0"], SCALE["F1"]], device=dev)
        k = timed(lambda: ops.photon_nll(t, xf, free.par, free.map, free.tpl, free.norm, pv, flags=N.FLAG_TIME_KERNELS))
        out["free"]["n%d_p%d" % (n, P)] = dict(k, evals_per_s=n * P / (k["median"] * 1e-3))
    for orbit, okeys in ORBITS.items():
        par = model(orbit)
        k = timed(lambda: ops.binary_delay(t, par, flags=N.FLAG_TIME_KERNELS))
        out["delay"]["%s_n%d" % (orbit, n)] = dict(k, photons_per_s=n / (k["median"] * 1e-3))
        for label, keys in (("spin", ["F0", "F1"]), ("orbit", ["F0", "F1"] + okeys)):
            fit = PhotonOrbitFit(tm, par, theta, keys=keys)
            x = torch.as_tensor(fit.x, device=dev)
            scale = np.array([SCALE[k] for k in keys])
            for P in ps:
                pv = torch.as_tensor(np.random.default_rng(P).uniform(-1, 1, (P, len(keys))) * scale, device=dev)
                k = timed(lambda: ops.photon_orbit_nll(t, x, fit.par, fit.map, fit.tpl, fit.norm, pv,
                                                       flags=N.FLAG_TIME_KERNELS))
                name = "%s_%s_n%d_p%d" % (orbit, label, n, P)
                rate = n * P / (k["median"] * 1e-3)
                out["nll"][name] = dict(k, evals_per_s=rate)
                out["ratio"][name] = {"to_binary_free": rate / out["free"]["n%d_p%d" % (n, P)]["evals_per_s"],
                                      "to_solve": rate / out["delay"]["%s_n%d" % (orbit, n)]["photons_per_s"]}
            if label == "orbit" and n <= 1000000:
                plain = {k: v["value"] for k, v in par.items()}
                tc = []
                for _ in range(2):
                    t0 = time.perf_counter()
                    PO.nll_host(fit.t, fit.x, plain, theta, scale, keys)
                    tc.append(time.perf_counter() - t0)
                out["cpu"]["%s_n%d" % (orbit, n)] = {"s_per_eval": min(tc), "chain_s_extrapolated": min(tc) * 32 * steps}
            if label == "orbit" and n == 100000:
                rng = np.random.default_rng(1)
                p0 = torch.as_tensor(rng.uniform(-3, 3, (32, len(keys))) * scale, device=dev)
                lo, hi = (torch.as_tensor(s * 1e3 * scale, device=dev) for s in (-1.0, 1.0))
                wall, kern = [], []
                for r in range(2):
                    t0 = time.perf_counter()
                    ops.photon_orbit_mcmc(t, x, fit.par, fit.map, fit.tpl, fit.norm, p0, lo, hi, steps, 5,
                                          flags=N.FLAG_TIME_KERNELS)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    kern.append(N.last_kernel_times()[0])
                p16 = p0[:16].contiguous()
                half = timed(lambda: ops.photon_orbit_nll(t, x, fit.par, fit.map, fit.tpl, fit.norm, p16,
                                                          flags=N.FLAG_TIME_KERNELS))
                per_step = kern[-1] / steps
                out["chain"]["%s_n%d" % (orbit, n)] = {"wall_ms": wall[-1], "kernel_ms": kern[-1],
                                                       "ms_per_step": per_step, "two_nll_p16_ms": 2 * half["median"],
                                                       "step_over_two_nll": per_step / (2 * half["median"])}
line = json.dumps(out)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "photon_orbit_fit.json"), "w") as fh:
    fh.write(line + "\n")
