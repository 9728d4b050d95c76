"""Writes tests/golden/photon_orbit.npz: delta of the photon-domain orbit fits at 60 digits for
photon arrays that span several tiles of the likelihood kernel. Needs mpmath; the fixture loads without it.

    python tests/golden/gen_photon_orbit_golden.py

The models are Taylor-only, so delta is the model residual of the orbit fits (orbit_fit_reference.residual_mp) for the
same keys and vector. Per model of photon_orbit_reference.GOLDEN_MODELS: its free keys, 3 T + 17 photon times (T = 1024,
the kernels' tile) drawn uniformly over the model's own time span with a fixed seed and left unsorted, the vectors
`orbital`, `typical` and `wide` of orbit_fit_reference.vectors for those times, delta as hi + lo (20 bits of lo) and the
error unit A (16 bits, cut towards zero). Smaller photon counts are prefixes of the arrays.
"""
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the package: photon_reference imports it
import binary_reference as B          # noqa: E402
import orbit_fit_reference as O       # noqa: E402
import phase_reference as R           # noqa: E402
import photon_orbit_reference as P    # noqa: E402


def _one(job):
    tm, keys, p, t = job
    val, mag = O.residual_mp(tm, keys, p, t)
    hi, lo = R.hi_lo(val)
    return hi, lo, R.mag_chopped(mag)


def main():
    src = B.load_binary()
    out = {"index": json.dumps(list(P.GOLDEN_MODELS)), "vectors": json.dumps(list(P.GOLDEN_VECTORS))}
    jobs, where = [], []
    for name in P.GOLDEN_MODELS:
        m = src[name]
        keys = O.free_keys(m.tm)
        rng = np.random.default_rng(P.GOLDEN_SEED)
        t = rng.uniform(float(np.min(m.t)), float(np.max(m.t)), P.GOLDEN_N)
        pvec = O.vectors(m.tm, t)[[O.VECTORS.index(v) for v in P.GOLDEN_VECTORS]]
        out[name + "_model"] = json.dumps(m.tm)
        out[name + "_keys"] = json.dumps(keys)
        out[name + "_pvec"] = pvec
        out[name + "_t"] = t
        for p in pvec:
            jobs.append((m.tm, keys, p, t))
            where.append(name)
    with ProcessPoolExecutor(max_workers=len(jobs)) as ex:
        res = list(ex.map(_one, jobs))
    for name in P.GOLDEN_MODELS:
        rows = [r for r, w in zip(res, where) if w == name]
        out[name + "_hi"] = np.array([r[0] for r in rows])
        out[name + "_lo"] = np.array([r[1] for r in rows])
        out[name + "_A"] = np.array([r[2] for r in rows])
        print(name, "max |delta| %.3g" % np.max(np.abs(out[name + "_hi"])), "max A %.3g" % np.max(out[name + "_A"]))
    path = os.path.join(HERE, "photon_orbit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
