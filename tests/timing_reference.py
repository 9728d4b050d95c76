"""NumPy restatement of the reference's fit likelihood (utilities_fittoas.py:204-293 over calcphase.py:73-149), for
the tests and for tools/run_timing_fit.py, which times it as the CPU cost of one likelihood evaluation. It goes
through the same steps per call as the reference -- the two injected dictionaries, then the Taylor, glitch and wave
phases as separate NumPy expressions -- so its cost is of the reference's kind."""
from math import factorial

import numpy as np

from crimp_amd.utilities_fittoas import gaussian_nll, inject_free_params


def _value(v):
    return v["value"] if isinstance(v, dict) and "value" in v and "flag" in v else v


def taylor(x, d):
    dt = (x - _value(d["PEPOCH"])) * 86400.0
    out = 0.0
    for n in range(1, 14):
        out = out + (1.0 / factorial(n)) * _value(d["F%d" % (n - 1)]) * dt ** n
    return out


def glitches(x, d):
    out = np.zeros(x.size)
    for j in range(1, sum(1 for k in d if k.startswith("GLEP_")) + 1):
        ep = float(_value(d["GLEP_%d" % j]))
        on = x >= ep
        if not on.any():
            continue
        ph, f0, f1, f2, f0d, td = (float(_value(d.get("%s_%d" % (b, j), 0.0)))
                                   for b in ("GLPH", "GLF0", "GLF1", "GLF2", "GLF0D", "GLTD"))
        t = x[on]
        s = (t - ep) * 86400.0
        ex = 0.0 if td == 0.0 else (td * 86400.0) * (1.0 - np.exp(-(t - ep) / td))
        out[on] += ph + f0 * s + 0.5 * f1 * s ** 2 + (1.0 / 6.0) * f2 * s ** 3 + f0d * ex
    return out


def waves(x, d):
    nkeys = sum(1 for k in d if k.startswith("WAVE"))
    out = 0
    if nkeys:
        ep, om = _value(d["WAVEEPOCH"]), _value(d["WAVE_OM"])
        for j in range(1, nkeys - 1):
            ab = _value(d["WAVE%d" % j])
            arg = j * om * (x - ep)
            out = out + ab["A"] * np.sin(arg) + ab["B"] * np.cos(arg)
    return out * _value(d["F0"])


def model_phase_residuals(x, model, pvec, keys):
    x = np.atleast_1d(np.asarray(x, dtype=float))
    fit, full = inject_free_params(model, pvec, keys)
    wave = ["wave" in k.lower() for k in keys]
    if all(wave):
        fit["F0"] = full["F0"]
        ph = waves(x, fit)
    elif not any(wave):
        ph = taylor(x, fit) + glitches(x, fit) + waves(x, full)
    else:
        te, gl = taylor(x, fit), glitches(x, fit)
        fit["F0"] = full["F0"]
        ph = te + gl + waves(x, fit)
    return ph - np.mean(ph)


def nll(x, y, yerr, model, pvec, keys):
    return gaussian_nll(y - np.mean(y), model_phase_residuals(x, model, pvec, keys), yerr)
