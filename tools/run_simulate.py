"""The device event simulator (csrc/sim_events.h) against the host generator it can replace (crimp_amd/synth.py):
  device   crimp_sim_events with the parameters of bench.py's config 3 (1e7 photons: T = 1e6 s, f0 = 7.123456789 Hz,
           pulsed fraction 0.1) and config 4 (1e8 photons: T = 1e7 s, pulsed fraction 0.05, fdot = -1e-12) as a K = 1
           Fourier shape of norm n / T: kernel time (count pass + offset scan + fill pass, hipEvents), wall time of
           ops.sim_events into device tensors (one call: the buffers are sized from the expected count), and into host
           arrays (adds the copy of the events)
  host     synth.pulsed_events with the same parameters on this machine's CPU (NumPy rejection sampling + sort)
REPS timed repeats (default 5; HOST_REPS for the host generator, default 2, the value of the
recorded profile) after one warm-up: median [min-max].
ns per accepted event, and the share of the VALU peak (3.93e13 lane-slots/s = 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz)
that OPS_PER_CANDIDATE vector instructions per candidate imply. One JSON line, also written to profiles/simulate.json."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crimp_amd import _native as N, ops  # noqa: E402
from crimp_amd.simulatemodulatedlc import build_shape, cell_count, cell_length  # noqa: E402
from crimp_amd.synth import pulsed_events  # noqa: E402

reps = int(os.environ.get("REPS", 5))
host_reps = int(os.environ.get("HOST_REPS", 2))
sizes = [float(v) for v in os.environ.get("SIZES", "1e7,1e8").split(",")]
VALU_PEAK = 3.93e13
# vector instructions per candidate of the K = 1 Fourier path: the source-level count of DESIGN.md 5.7
OPS_PER_CANDIDATE = float(os.environ.get("OPS_PER_CANDIDATE", 300))
CONFIGS = {1.0e7: dict(span=1.0e6, p=0.1, fdot=0.0, seed=0), 1.0e8: dict(span=1.0e7, p=0.05, fdot=-1.0e-12, seed=1)}
F0, MJD0 = 7.123456789, 58400.0


def stat(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def device_leg(n, cfg):
    import torch
    rate = n / cfg["span"]
    mid = MJD0 + 0.5 * cfg["span"] / 86400.0  # synth.pulsed_events measures the phase from the middle of the span
    tm = {"PEPOCH": mid, "F0": F0, "F1": cfg["fdot"]}
    shape, lam = build_shape({"model": "fourier", "norm": rate, "amp_1": cfg["p"] * rate, "ph_1": 0.0})
    cell = cell_length(lam)
    out = {"lam_max": lam, "cell_s": cell, "cells": cell_count(cfg["span"], cell),
           "candidates": lam * cfg["span"]}
    for name, dev in (("device_tensors", True), ("host_arrays", None)):
        wall, kern, cnt = [], [], 0
        for r in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t, b, cnt = ops.sim_events(tm, shape, MJD0, cfg["span"], cell, seed=cfg["seed"], device=dev,
                                       out_offset_s=5.0e9, flags=N.FLAG_TIME_KERNELS,
                                       cap=int(n + 6 * np.sqrt(n) + 64))
            torch.cuda.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            if r:
                wall.append(w)
                kern.append(N.last_kernel_times()[0])
            del t, b
        out[name] = {"wall_ms": stat(wall), "fill_call_kernel_ms": stat(kern), "events": cnt,
                     "wall_ns_per_event": float(np.median(wall)) * 1e6 / cnt}
    # the fill call's timed span covers its own count pass, the scan and the fill pass
    k = out["device_tensors"]["fill_call_kernel_ms"]["median"]
    out["kernel_ns_per_event"] = k * 1e6 / out["device_tensors"]["events"]
    # both passes draw every candidate
    out["valu_share"] = 2.0 * out["candidates"] * OPS_PER_CANDIDATE / (k * 1e-3) / VALU_PEAK
    return out


def host_leg(n, cfg):
    wall = []
    for r in range(host_reps + 1):
        t0 = time.perf_counter()
        pulsed_events(int(n), cfg["span"], F0, pulsed_frac=cfg["p"], fdot=cfg["fdot"], seed=cfg["seed"])
        if r:
            wall.append((time.perf_counter() - t0) * 1e3)
    return {"wall_ms": stat(wall), "ns_per_event": float(np.median(wall)) * 1e6 / n}


rec = {"reps": reps, "host_reps": host_reps, "ops_per_candidate": OPS_PER_CANDIDATE, "runs": {}}
for n in sizes:
    cfg = CONFIGS[n]
    d = device_leg(n, cfg)
    h = host_leg(n, cfg)
    d["host_synth"] = h
    d["device_over_host"] = h["wall_ms"]["median"] / d["device_tensors"]["wall_ms"]["median"]
    rec["runs"]["%g" % n] = d
line = json.dumps(rec)
print(line)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
out = os.environ.get("OUT", os.path.join(ROOT, "profiles", "simulate.json"))
with open(out, "w") as fh:
    fh.write(line + "\n")
