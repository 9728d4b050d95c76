"""The fused orbit search (crimp_orbit_search, csrc/orbit_search.h) against the route without it, one shape per run.

  python tools/run_orbit_search.py --n 100000 --nf 1,16,64 --model ell1 [--norb 10000] [--out FILE]
      (a) the fused call at norb orbits (a TASC x A1 product grid around the model), m = 2, Z^2: REPS timed repeats
          (default 3) after one warm-up; kernel time (CRIMP_FLAG_TIME_KERNELS: search and finalize kernels) and the
          (photon x orbit) solves / s that time amounts to (an upper bound on the solve's own time: the trial sums are
          in it);
      (b) the route of a build without the fused call, per orbit: ops.binary_delay, dt = (t - tref) 86400 - tau on the
          device, ops.search(dt, 0, freq) -- with precision="f64" and with the default --, device arrays throughout,
          timed with device events around BASE_ORBITS = 64 orbits after a warm-up of 8 and extrapolated linearly to
          norb orbits (the per-orbit cost does not depend on the orbit; the figure says "extrapolated");
      the powers of the first 8 orbits of (a) and (b, f64) are compared (they differ by the fp64 rounding of dt).
  python tools/run_orbit_search.py --delay-rate [--model ell1]
      k_binary_delay's own rate in this session: 1e8 photons, kernel time, solves / s.

Each shape prints one JSON line and appends it to --out (default profiles/orbit_search.jsonl). Run the shapes as
separate steps, each under its own time limit, chained so that a failure ends the chain:
  timeout -k 10 120 python tools/run_orbit_search.py --delay-rate && \\
  timeout -k 10 300 python tools/run_orbit_search.py --n 100000 --nf 1,16,64 --model ell1 && ...
N in {1e5, 1e6}, nf in {1, 16, 64}, models ell1 and bt_e07 are the shapes DESIGN.md 5.10 tabulates."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {
    "ell1": ({"PEPOCH": 58000.0, "F0": 401.0, "BINARY": "ELL1", "PB": 0.084, "A1": 0.063, "TASC": 57999.93,
              "EPS1": 1e-5, "EPS2": -2e-5}, "TASC", 1e-5, 1e-5),
    "bt_e07": ({"PEPOCH": 58000.0, "F0": 29.7, "BINARY": "BT", "PB": 0.21, "A1": 1.2, "T0": 57999.95, "ECC": 0.7,
                "OM": 70.0, "OMDOT": 30.0, "GAMMA": 1e-4}, "T0", 1e-5, 1e-4),
}
SPAN = 0.31
reps = int(os.environ.get("REPS", 3))
base_orbits = int(os.environ.get("BASE_ORBITS", 64))


def stat(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--nf", type=str, default="16", help="trial frequencies; a comma list runs one shape after another")
    ap.add_argument("--norb", type=int, default=10000)
    ap.add_argument("--model", choices=sorted(MODELS), default="ell1")
    ap.add_argument("--delay-rate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbit_search.jsonl"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    from crimp_amd import _native as N, ops
    tm, t0key, dt0, da1 = MODELS[args.model]
    rng = np.random.default_rng(7)

    def emit(out):
        line = json.dumps(out)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")

    if args.delay_rate:
        n = 10 ** 8
        t = torch.as_tensor(58000.0 + np.sort(rng.uniform(0.0, SPAN, n)), device=dev)
        delay = torch.empty_like(t)
        ms = []
        for r in range(reps + 1):
            ops.binary_delay(t, tm, delay=delay, flags=N.FLAG_TIME_KERNELS)
            if r:
                ms.append(N.load().crimp_last_kernel_ms())
        out = {"what": "k_binary_delay", "model": args.model, "n": n, "kernel_ms": stat(ms),
               "solves_per_s": n / (float(np.median(ms)) * 1e-3)}
        return emit(out)
    for nf in [int(v) for v in args.nf.split(",")]:
        n, norb, m = args.n, args.norb, 2
        th = 58000.0 + np.sort(rng.uniform(0.0, SPAN, n))
        t = torch.as_tensor(th, device=dev)
        tref = 58000.0 + SPAN / 2
        f0 = float(tm["F0"])
        freq = f0 + (np.arange(nf) - nf // 2) / (SPAN * 86400.0)
        side = int(round(norb ** 0.5))
        assert side * side == norb, "norb must be a square: the grid is TASC x A1"
        ax0 = float(tm[t0key]) + (np.arange(side) - side // 2) * dt0
        ax1 = float(tm["A1"]) + (np.arange(side) - side // 2) * da1
        orbits = np.stack([g.ravel() for g in np.meshgrid(ax0, ax1, indexing="ij")], axis=1)
        keys = [t0key, "A1"]
        # (a) the fused call
        kern, wall = [], []
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(reps + 1):
            start.record()
            pw, _ = ops.orbit_search(t, tm, keys, orbits, freq, m, 0, tref=tref, flags=N.FLAG_TIME_KERNELS)
            stop.record()
            stop.synchronize()
            if r:
                kern.append(N.load().crimp_last_kernel_ms())
                wall.append(start.elapsed_time(stop))
        fused = pw[:8].cpu().numpy()
        plan = N.orbit_search_plan(n, nf, m, 0, norb)
        out = {"what": "orbit_search", "model": args.model, "n": n, "nf": nf, "norb": norb, "m": m, "reps": reps,
               "plan": plan, "fused_kernel_ms": stat(kern), "fused_call_ms": stat(wall),
               "fused_solves_per_s": n * norb / (float(np.median(kern)) * 1e-3)}
        # (b) per orbit: binary_delay + search, on the device
        fd = torch.as_tensor(freq, device=dev)
        tau = torch.empty_like(t)

        def route(o, precision):
            par = dict(tm)
            par[t0key], par["A1"] = float(orbits[o, 0]), float(orbits[o, 1])
            ops.binary_delay(t, par, delay=tau)
            d = (t - tref) * 86400.0 - tau
            return ops.search(d, 0.0, fd, m, 0, precision=precision)

        for label, precision in (("f64", "f64"), ("default", None)):
            for o in range(8):
                route(o, precision)
            per = []
            for r in range(reps):
                start.record()
                for o in range(base_orbits):
                    route(o, precision)
                stop.record()
                stop.synchronize()
                per.append(start.elapsed_time(stop) / base_orbits)
            med = float(np.median(per))
            out["route_%s_ms_per_orbit" % label] = stat(per)
            out["route_%s_ms_extrapolated" % label] = med * norb
            out["route_%s_over_fused" % label] = med * norb / float(np.median(wall))
        ref = np.stack([route(o, "f64").cpu().numpy() for o in range(8)])
        out["max_rel_diff_vs_route_f64"] = float(np.max(np.abs(fused - ref) / np.maximum(np.abs(ref), 1.0)))
        out["timed_orbits_of_route"] = base_orbits
        emit(out)


if __name__ == "__main__":
    main()
