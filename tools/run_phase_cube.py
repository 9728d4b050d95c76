"""Fused 32 x 12 phase-time map (crimp_phase_cube with a timing model, 8 B/photon) against calcphase followed by
binphases (24 B + 8 B/photon) on one device-resident, time-sorted list of MJD times; both alternate in one process.
NPH photons (default 1e8), REPS timed repeats (default 10) after 2 warm-ups of every call. One JSON line."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crimp_amd import _native as N, ops  # noqa: E402
from crimp_amd.readtimingmodel import ReadTimingModel  # noqa: E402
from crimp_amd.synth import pulsed_events  # noqa: E402

n = int(float(os.environ.get("NPH", 1e8)))
reps = int(os.environ.get("REPS", 10))
dev = torch.device("cuda", 0)
tm = ReadTimingModel(os.path.join(ROOT, "tests", "golden", "1e2259.par")).readfulltimingmodel()[0]
sec = pulsed_events(n, 5.0e5, 0.1432825, pulsed_frac=0.3, seed=1, offset=0.0)
t = torch.as_tensor(58141.0 + sec / 86400.0, device=dev)
del sec
te = np.linspace(float(t[0]), float(t[-1]), 13)
pe = np.linspace(0.0, 1, 33)
tot, fol = torch.empty_like(t), torch.empty_like(t)
off = torch.tensor([0, n], dtype=torch.int64, device=dev)
ped = torch.as_tensor(pe, device=dev)
L = N.load()


def fused():
    c = ops.phase_cube(t, model=tm, y_edges=te, ph_edges=pe, options=N.CUBE_Y_IS_X, flags=N.FLAG_TIME_KERNELS)
    return L.crimp_last_kernel_ms(), c


def fold():
    ops.calcphase(t, tm, total=tot, folded=fol, flags=N.FLAG_TIME_KERNELS)
    return L.crimp_last_kernel_ms()


def bin1d():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    c = ops.binphases_counts(fol, off, ped)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), c


def unfused():
    c = ops.phase_cube(fol, y=t, y_edges=te, ph_edges=pe, flags=N.FLAG_TIME_KERNELS)
    return L.crimp_last_kernel_ms(), c


rows = {"fused": [], "calcphase": [], "binphases": [], "unfused_cube": []}
for r in range(reps + 2):
    a, cube = fused()
    b = fold()
    c, hist = bin1d()
    d, cube2 = unfused()
    if r >= 2:
        for k, v in zip(rows, (a, b, c, d)):
            rows[k].append(v)
assert int(cube.sum()) == n and torch.equal(cube.sum(0), hist[0]) and torch.equal(cube, cube2)


def stat(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


parent = [x + y for x, y in zip(rows["calcphase"], rows["binphases"])]
out = {"n": n, "reps": reps, "ms": {k: stat(v) for k, v in rows.items()}, "parent_two_kernels_ms": stat(parent)}
out["fused_GBps"] = 8.0 * n / out["ms"]["fused"]["median"] / 1e6
out["calcphase_GBps"] = 24.0 * n / out["ms"]["calcphase"]["median"] / 1e6
print(json.dumps(out), flush=True)
