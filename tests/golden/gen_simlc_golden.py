"""Regenerates tests/golden/simlc_reference.npz: one recorded run of the reference's simulatemodulatedlc
(simulatemodulatedlc.py:19-96), loaded by file path from a CRIMP v2.3.0 source tree, with NumPy's global RNG seeded.

    python tests/golden/gen_simlc_golden.py [path/to/src/crimp/simulatemodulatedlc.py]

Stored: the call's parameters, the seed, the two totals and the 16-bin folded histograms (phase = frac(freq * t)) of
the events with and without background. The fixture is data the reference wrote while it ran; none of its code."""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PARAMS = dict(freq=0.5, srcrate=20.0, exposure=2000.0, pulsedfraction=0.3, bgrrate=2.0, nbrPhaseBins=16)
SEED = 11


def main(path):
    spec = importlib.util.spec_from_file_location("reference_simulatemodulatedlc", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    np.random.seed(SEED)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        r = mod.simulatemodulatedlc(PARAMS["freq"], PARAMS["srcrate"], PARAMS["exposure"], PARAMS["pulsedfraction"],
                                    PARAMS["bgrrate"], nbrPhaseBins=PARAMS["nbrPhaseBins"])
    nb = PARAMS["nbrPhaseBins"]
    hist = {}
    for key in ("assigned_t_wBgr", "assigned_t_nobgr"):
        ph = (r[key] * PARAMS["freq"]) % 1.0
        hist[key] = np.histogram(ph, bins=nb, range=(0.0, 1.0))[0].astype(np.int64)
    np.savez(os.path.join(HERE, "simlc_reference.npz"), seed=np.int64(SEED),
             n_wbgr=np.int64(r["assigned_t_wBgr"].size), n_nobgr=np.int64(r["assigned_t_nobgr"].size),
             hist_wbgr=hist["assigned_t_wBgr"], hist_nobgr=hist["assigned_t_nobgr"],
             t_min=np.float64(r["assigned_t_wBgr"].min()), t_max=np.float64(r["assigned_t_wBgr"].max()),
             printed=np.array(out.getvalue()), **{k: np.float64(v) for k, v in PARAMS.items()})
    print("source events", r["assigned_t_nobgr"].size, "with background", r["assigned_t_wBgr"].size)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference/src/crimp/simulatemodulatedlc.py")
