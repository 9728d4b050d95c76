"""NumPy restatement of the photon-domain likelihood (csrc/photon_fit.h), for the tests and for
tools/run_photon_fit.py, which times it as the CPU cost of one likelihood evaluation.

    delta_i(p) = Phi(t_i; par) - Phi(t_i; par - p)   from the linear expression: every term is of size |delta|
    u_i        = x_i - delta_i(p) - PHOFF
    NLL(p)     = -sum_i ln(m(u_i) / norm),  +inf when some m(u_i) <= 0

delta is built from inject_free_params' fit model (the free amplitudes, every other amplitude 0) with the shape
values it drops put back (GLTD), and the Taylor / glitch / wave pieces of tests/timing_reference.py."""
import numpy as np

import sim_reference as S
import timing_reference as T
from crimp_amd.utilities_fittoas import inject_free_params

TWO_PI = 2.0 * np.pi
_AMPLITUDES = ("GLPH", "GLF0", "GLF1", "GLF2", "GLF0D")


def _value(v):
    return v["value"] if isinstance(v, dict) and "value" in v else v


def flagged(plain, free=()):
    """A plain timing-model dict as a flagged one ({"value", "flag"} entries; WAVEj as {"value": {A, B}})."""
    out = {}
    for k, v in plain.items():
        if isinstance(v, dict) and "A" in v:
            out[k] = {"value": dict(v), "flag": None}
        else:
            out[k] = {"value": v, "flag": 1 if k in free else 0}
    return out


def delta(t, par, pvec, keys):
    """delta [n] of one vector (model keys only, no PHOFF), in cycles."""
    t = np.atleast_1d(np.asarray(t, dtype=float))
    plain = {k: _value(v) for k, v in par.items()}
    gltd = {k: plain[k] for k in plain if k.startswith("GLTD_")}
    fit, _ = inject_free_params(par, np.asarray(pvec, dtype=float), list(keys))
    fit = {k: _value(v) for k, v in fit.items()}
    fit.update(gltd)  # a shape value: kept, where the ToA fit model zeroes it
    for n in range(13):
        fit.setdefault("F%d" % n, 0.0)
    out = T.taylor(t, fit) + T.glitches(t, fit)
    names = [k for k in plain if k.startswith("WAVE") and k not in ("WAVEEPOCH", "WAVE_OM")]
    wave_free = any(k.startswith("WAVE") for k in keys)
    if names and (wave_free or "F0" in keys):
        df0 = float(pvec[list(keys).index("F0")]) if "F0" in keys else 0.0
        shape = {"WAVEEPOCH": plain["WAVEEPOCH"], "WAVE_OM": plain["WAVE_OM"]}
        corr, base = dict(shape), dict(shape)
        for name in names:
            corr[name] = {s: (float(pvec[list(keys).index(name + "_" + s)]) if name + "_" + s in keys else 0.0)
                          for s in "AB"}
            base[name] = dict(plain[name])
        corr["F0"], base["F0"] = plain["F0"] - df0, df0
        # F0 A - (F0 - dF0)(A - dA) = (F0 - dF0) dA + dF0 A
        out = out + T.waves(t, corr) + T.waves(t, base)
    return out


def template_value(theta, u, norm=None, ampShift=1.0):
    """(m, dm/du) of a template (plain values) at phases u in cycles; ``norm`` replaces the template's own."""
    th = {k: _value(v) for k, v in theta.items()}
    if norm is not None:
        th["norm"] = float(norm)
    u = np.asarray(u, dtype=float)
    m = S.template_rate(th, u, 0.0, ampShift)
    K = len([k for k in th if k.startswith("amp_")])
    d = np.zeros_like(u)
    for j in range(1, K + 1):
        a = float(th["amp_%d" % j]) * ampShift
        if th["model"] == "fourier":
            d -= a * j * TWO_PI * np.sin(j * TWO_PI * u + float(th["ph_%d" % j]))
            continue
        c, w = float(th["cen_%d" % j]), float(th["wid_%d" % j])
        x = TWO_PI * u - c
        if th["model"] == "cauchy":
            d -= (a / TWO_PI) * np.sinh(w) * np.sin(x) * TWO_PI / (np.cosh(w) - np.cos(x)) ** 2
        else:
            from scipy.special import i0
            k = 1.0 / w ** 2
            d -= (a / (TWO_PI * i0(k))) * np.exp(k * np.cos(x)) * k * np.sin(x) * TWO_PI
    return m, d


def terms(t, x, par, theta, pvec, keys, phoff=False, norm=None, ampShift=1.0):
    """Per-photon (delta, ln(m / norm) with NaN where m <= 0, |d ln m / du|) of one vector (PHOFF last if ``phoff``)."""
    p = np.asarray(pvec, dtype=float)
    nd = len(keys)
    d = delta(t, par, p[:nd], keys)
    u = np.asarray(x, dtype=float) - d - (p[nd] if phoff else 0.0)
    m, dm = template_value(theta, u, norm, ampShift)
    nrm = float(_value(theta["norm"]) if norm is None else norm)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.where(m > 0, np.log(np.where(m > 0, m, 1.0) / nrm), np.nan)
        slope = np.abs(dm / m)
    return d, ln, slope


def nll(t, x, par, theta, pvec, keys, phoff=False, norm=None, ampShift=1.0):
    _, ln, _ = terms(t, x, par, theta, pvec, keys, phoff, norm, ampShift)
    return np.inf if np.any(np.isnan(ln)) else -float(np.sum(ln))


def hessian(f, p, h):
    """Central-difference Hessian of f at p with steps h."""
    p, h = np.asarray(p, dtype=float), np.asarray(h, dtype=float)
    n = p.size
    H = np.empty((n, n))
    f0 = f(p)
    for i in range(n):
        ei = np.zeros(n)
        ei[i] = h[i]
        H[i, i] = (f(p + ei) - 2.0 * f0 + f(p - ei)) / h[i] ** 2
        for j in range(i + 1, n):
            ej = np.zeros(n)
            ej[j] = h[j]
            H[i, j] = H[j, i] = (f(p + ei + ej) - f(p + ei - ej) - f(p - ei + ej) + f(p - ei - ej)) / (4 * h[i] * h[j])
    return H


def mle(f, p0, scale):
    """Numerical maximum-likelihood point of the NLL f and the observed-information sigma: Nelder-Mead in units of
    ``scale`` (rough parameter uncertainties), then a central-difference Hessian with steps of 0.3 sigma, once from
    ``scale`` and once more from the sigma that gives. Returns (p, sigma, covariance)."""
    from scipy.optimize import minimize
    p0, scale = np.asarray(p0, dtype=float), np.asarray(scale, dtype=float)
    res = minimize(lambda q: f(p0 + q * scale), np.zeros(p0.size), method="Nelder-Mead",
                   options={"xatol": 1e-6, "fatol": 1e-10, "maxiter": 20000})
    p = p0 + res.x * scale
    sig = scale
    for _ in range(2):
        cov = np.linalg.inv(hessian(f, p, 0.3 * sig))
        sig = np.sqrt(np.diag(cov))
    return p, sig, cov


def host_events(par, theta, span_days, rate_scale, rng):
    """A host-drawn data set: sorted uniform candidate times over ``span_days`` around PEPOCH, thinned against
    template_rate(frac(total_phase)) / its bound. ``rate_scale`` candidates per day. Returns the kept MJDs."""
    plain = {k: _value(v) for k, v in par.items()}
    th = {k: _value(v) for k, v in theta.items()}
    n = rng.poisson(rate_scale * span_days)
    t = np.sort(rng.uniform(plain["PEPOCH"] - 0.5 * span_days, plain["PEPOCH"] + 0.5 * span_days, n))
    ph = S.total_phase(t, plain)
    rate = S.template_rate(th, ph - np.floor(ph))
    bound = th["norm"] + sum(abs(th[k]) for k in th if k.startswith("amp_"))
    assert th["model"] == "fourier" and rate.min() >= 0.0
    return t[rng.uniform(size=n) * bound < rate]
