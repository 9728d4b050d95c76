"""Writes tests/golden/orbit_fit.npz: the model residuals of the orbit fits at 60 digits (tests/orbit_fit_reference.py:
residual_mp) for the models, ToA counts and vectors the tests use. Needs mpmath; the fixture loads without it.

    python tests/golden/gen_orbit_fit_golden.py

Per model of orbit_fit_reference.MODELS (from calcphase_binary.npz): its free keys and five vectors (zero, orbital only,
spin only, typical posterior widths, 1e3 widths); per ToA count of SIZES the times, m as hi + lo (20 bits of lo) and the
error unit A (16 bits, cut towards zero).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import binary_reference as B          # noqa: E402
import orbit_fit_reference as O       # noqa: E402
import phase_reference as R           # noqa: E402


def main():
    src = B.load_binary()
    out = {"index": json.dumps(list(O.MODELS))}
    for name in O.MODELS:
        m = src[name]
        keys = O.free_keys(m.tm)
        pvec = O.vectors(m.tm, m.t)
        out[name + "_model"] = json.dumps(m.tm)
        out[name + "_keys"] = json.dumps(keys)
        out[name + "_pvec"] = pvec
        for n in O.SIZES:
            t = O.toa_set(m.t, n)
            hi, lo, a = [], [], []
            for p in pvec:
                val, mag = O.residual_mp(m.tm, keys, p, t)
                h, l = R.hi_lo(val)
                hi.append(h)
                lo.append(l)
                a.append(R.mag_chopped(mag))
            k = "%s_%d" % (name, n)
            out[k + "_t"] = t
            out[k + "_hi"], out[k + "_lo"], out[k + "_A"] = np.array(hi), np.array(lo), np.array(a)
            print(name, n, "max |m| %.3g" % np.max(np.abs(hi)), "max A %.3g" % np.max(a), flush=True)
    path = os.path.join(HERE, "orbit_fit.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
