"""Orbit fits on the device (csrc/orbit_fit.h) against the binary-free fits on the same ToAs:
  timing_nll   crimp_timing_nll, P = 4096 vectors on the 84 bundled ToAs (F0, F1 free): likelihoods / s
  orbit_nll    crimp_orbit_nll at the same shape for a BT (e = 0.7) and an ELL1 orbit put under those ToAs, with the
               spin keys alone (the fixed orbit) and with the orbital keys free as well
  chains       32 walkers x 10000 steps: crimp_timing_mcmc, and crimp_orbit_mcmc for both orbits with every key free
REPS timed repeats (default 5) after one warm-up, the binary-free and the orbit calls alternating.

--parent-lib PATH: another build of the library (the parent commit's). crimp_timing_nll then runs in fresh child
processes, the two builds alternating (ROUNDS rounds, default 3); the report holds each build's times, their spread, and
whether nll and mu are the same bits.
One JSON line, also written to profiles/orbit_fit.json."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from crimp_amd import _native as N, ops  # noqa: E402
from crimp_amd.fit_orbit import OrbitFit  # noqa: E402
from crimp_amd.fit_toas import load_toas_for_fit  # noqa: E402
from crimp_amd.readtimingmodel import ReadTimingModel  # noqa: E402
from crimp_amd.timfile import readtimfile  # noqa: E402
from crimp_amd.utilities_fittoas import DeviceFit, list_fit_keys  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
P = 4096
reps = int(os.environ.get("REPS", 5))
ORBITS = {
    "bt_e07": ({"BINARY": "BT", "PB": 8.3, "A1": 20.0, "ECC": 0.7, "OM": 200.0, "T0": 0.3},
               ["PB", "A1", "T0", "ECC", "OM"], [1e-7, 1e-5, 1e-6, 1e-6, 1e-4]),
    "ell1": ({"BINARY": "ELL1", "PB": 0.0839, "A1": 0.0628, "TASC": 0.04, "EPS1": 1e-5, "EPS2": -2e-5},
             ["PB", "A1", "TASC", "EPS1", "EPS2"], [1e-10, 1e-6, 1e-6, 1e-5, 1e-5]),
}
SPIN_SCALE = [1e-10, 1e-17]


def stat(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def bundled():
    model = ReadTimingModel(os.path.join(GOLD, "1e2259.par")).readfulltimingmodel()[2]
    model["F0"]["flag"] = model["F1"]["flag"] = 1
    toas = load_toas_for_fit(readtimfile(os.path.join(GOLD, "ToAs_2259.tim"), comment="C"), model)
    return model, toas


def timing_only(lib_path, data_path):
    """crimp_timing_nll of the build at ``lib_path`` on the ToAs saved at ``data_path``: kernel times and a digest of
    its outputs. The library is bound here, entry point by entry point: the parent's build has no orbit symbols for
    crimp_amd._native to bind."""
    import ctypes
    d = np.load(data_path)
    model = ReadTimingModel(os.path.join(GOLD, "1e2259.par")).readfulltimingmodel()[2]
    model["F0"]["flag"] = model["F1"]["flag"] = 1
    fit = DeviceFit(d["x"], model, list_fit_keys(model), d["y"], d["e"])
    pv = np.random.default_rng(0).normal(0, 1, (1, P, 2)) * np.array(SPIN_SCALE)
    L = ctypes.CDLL(lib_path)
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    MP, FP = ctypes.POINTER(N.TimingModel), ctypes.POINTER(N.FitMap)
    L.crimp_timing_nll.argtypes = [vp, vp, vp, vp, i64, MP, MP, FP, vp, i64, vp, vp, ctypes.c_uint32, vp]
    L.crimp_last_kernel_times.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int32]
    L.crimp_last_error.restype = ctypes.c_char_p
    n = fit.x.size
    off = np.array([0, n], dtype=np.int64)
    nll, mu = np.empty(P), np.empty(P * n)
    ms = (ctypes.c_double * 4)()
    kern = []
    for r in range(reps + 1):
        rc = L.crimp_timing_nll(fit.x.ctypes.data, fit.y.ctypes.data, fit.yerr.ctypes.data, off.ctypes.data, 1,
                                ctypes.byref(fit.fit_base), ctypes.byref(fit.wave_base), ctypes.byref(fit.map),
                                pv.ctypes.data, P, nll.ctypes.data, mu.ctypes.data, N.FLAG_TIME_KERNELS, None)
        if rc:
            raise RuntimeError(L.crimp_last_error().decode())
        L.crimp_last_kernel_times(ms, 4)
        if r:
            kern.append(ms[0])
    digest = hashlib.sha256(nll.tobytes() + mu.tobytes()).hexdigest()
    print(json.dumps({"kernel_ms": kern, "digest": digest}), flush=True)


def compare_with(parent_lib, x, y, e):
    import tempfile
    rounds = int(os.environ.get("ROUNDS", 3))
    runs = {"parent": [], "this": []}
    digests = {"parent": set(), "this": set()}
    libs = {"parent": os.path.abspath(parent_lib), "this": N.LIB_PATH}
    with tempfile.TemporaryDirectory() as tmp:
        data = os.path.join(tmp, "toas.npz")
        np.savez(data, x=x, y=y, e=e)
        for _ in range(rounds):
            for which in ("parent", "this"):
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--timing-only", libs[which], data],
                                     capture_output=True, text=True, timeout=300)
                if res.returncode:
                    raise RuntimeError("the %s build's run failed:\n%s" % (which, res.stderr[-2000:]))
                got = json.loads(res.stdout.strip().splitlines()[-1])
                runs[which] += got["kernel_ms"]
                digests[which].add(got["digest"])
    return {"rounds": rounds, "parent_kernel_ms": stat(runs["parent"]), "this_kernel_ms": stat(runs["this"]),
            "bit_identical": digests["parent"] == digests["this"] and len(digests["this"]) == 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--timing-only", nargs=2, metavar=("LIB", "TOAS_NPZ"), default=None)
    args = ap.parse_args()
    if args.timing_only:
        return timing_only(*args.timing_only)
    model, toas = bundled()
    spin_keys = list_fit_keys(model)
    x, y, e = toas["ToA"].to_numpy(), toas["phase"].to_numpy(), toas["phase_err_cycle"].to_numpy()
    rng = np.random.default_rng(0)
    free = DeviceFit(x, model, spin_keys, y, e)
    calls = {}
    pv = rng.normal(0, 1, (1, P, 2)) * np.array(SPIN_SCALE)
    calls["timing_nll"] = (P, lambda: ops.timing_nll(free.x, free.y, free.yerr, free.fit_base, free.wave_base, free.map,
                                                     pv, flags=N.FLAG_TIME_KERNELS))
    W, steps = 32, 10000
    p0 = rng.normal(0, 1, (1, W, 2)) * np.array(SPIN_SCALE)
    inf = np.full((1, 2), np.inf)
    chains = {"timing_mcmc": lambda: ops.timing_mcmc(free.x, free.y, free.yerr, free.fit_base, free.wave_base, free.map,
                                                     p0, -inf, inf, steps, 1, flags=N.FLAG_TIME_KERNELS)}
    for name, (orbit, okeys, oscale) in ORBITS.items():
        tm = dict(model)
        for k, v in orbit.items():
            if k in ("T0", "TASC"):
                v = float(np.floor(x.min())) + v
            tm[k] = {"value": v, "flag": None if k == "BINARY" else int(k in okeys)}
        for label, keys, scale in (("spin", spin_keys, SPIN_SCALE), ("all", spin_keys + okeys, SPIN_SCALE + oscale)):
            fit = OrbitFit(x, tm, keys, y, e)
            v = rng.normal(0, 1, (1, P, len(keys))) * np.array(scale)
            calls["orbit_nll_%s_%s" % (name, label)] = (P, lambda fit=fit, v=v: ops.orbit_nll(
                fit.x, fit.y, fit.yerr, fit.par, fit.fit_base, fit.wave_base, fit.map, v, flags=N.FLAG_TIME_KERNELS))
        nd = len(keys)
        q0 = rng.normal(0, 1, (1, W, nd)) * np.array(scale)
        box = np.full((1, nd), np.inf)
        chains["orbit_mcmc_%s_all" % name] = lambda fit=fit, q0=q0, box=box: ops.orbit_mcmc(
            fit.x, fit.y, fit.yerr, fit.par, fit.fit_base, fit.wave_base, fit.map, q0, -box, box, steps, 1,
            flags=N.FLAG_TIME_KERNELS)
    out = {"reps": reps, "ntoa": int(x.size), "P": P}
    for group, each in ((calls, None), (chains, W * steps)):
        wall = {k: [] for k in group}
        kern = {k: [] for k in group}
        for r in range(reps + 1):            # the calls alternate within every repeat
            for k, item in group.items():
                fn = item[1] if isinstance(item, tuple) else item
                t0 = time.perf_counter()
                fn()
                w = (time.perf_counter() - t0) * 1e3
                if r:
                    wall[k].append(w)
                    kern[k].append(N.last_kernel_times()[0])
        for k in group:
            n = group[k][0] if each is None else each
            out[k] = {"wall_ms": stat(wall[k]), "kernel_ms": stat(kern[k]),
                      "evals_per_s_kernel": n / (float(np.median(kern[k])) * 1e-3)}
    print(json.dumps(out), flush=True)
    if args.parent_lib:
        out["timing_nll_vs_parent"] = compare_with(args.parent_lib, x, y, e)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "orbit_fit.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
