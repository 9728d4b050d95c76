"""NumPy fp64 twin of the photon-domain orbit fits (csrc/photon_orbit_fit.h), the loader of their
60-digit fixture, and the host-drawn data set of the injection test. Built on orbit_fit_reference.py (full_model,
fit_model, the Taylor sums and the 60-digit residual), photon_reference.py (template_value) and timing_reference.py
(the glitch and wave pieces).

    te0 = t - tau_B0(t) / 86400,   teF = t - tau_B(p)(t) / 86400,   dtau = tau_B(p) - tau_B0
    delta_i(p) = phi_pf(p)(teF_i) + dtau_i (nu_i - nud_i dtau_i / 2)
    u_i = x_i - delta_i(p) - PHOFF,   NLL(p) = -sum_i ln(m(u_i) / norm),  +inf when some m(u_i) <= 0

phi_pf(p) is the photon fit model of DESIGN.md 5.8 (every linear amplitude of par 0, the free ones their p entries, the
wave cross term exact); nu, nud are the first two derivatives of par's spin phase at te0, glitches active there and
waves included. The Taylor part takes tau in seconds after the epoch difference, as the kernels do; the glitch and wave
pieces are timing_reference's at the emission MJD rounded to a double, which costs them up to 0.3 us times their own
rate: far below the 1e-9 cycles the glitch-and-wave test allows, and nothing on the Taylor-only fixture models.

For a Taylor-only model delta is the model residual m of the orbit fits (orbit_fit_reference.residual_mp) for the same
keys and vector, so tests/golden/orbit_fit.npz serves as a fixture of delta at ToA counts, and
tests/golden/photon_orbit.npz (gen_photon_orbit_golden.py) adds arrays of several tiles.
"""
import json
import os

import numpy as np

import orbit_fit_reference as O
import phase_reference as R
import photon_reference as PR
import timing_reference as T

U, FACTOR = O.U, O.FACTOR
TILE = 1024
GOLDEN_MODELS = ("bt_e07", "ell1_amxp")
GOLDEN_VECTORS = ("orbital", "typical", "wide")
GOLDEN_N = 3 * TILE + 17
GOLDEN_SIZES = (TILE - 1, TILE, TILE + 1, GOLDEN_N)
GOLDEN_SEED = 20241021
_GL_AMPS = ("GLPH", "GLF0", "GLF1", "GLF2", "GLF0D")


def _orbit_of(model):
    return {k: v for k, v in model.items() if k in O.ORBITAL or k == "BINARY"}


def full_orbit(tm, keys, p):
    """The corrected orbit of a vector: fl(par - p) on every orbital key, PBDOT and A1DOT dimensionless."""
    orb = [(k, d) for k, d in zip(keys, p) if k in O.ORBITAL]
    return _orbit_of(O.full_model(_orbit_of(R.plain(tm)), [k for k, _ in orb], [d for _, d in orb]))


def delays_host(tm, keys, p, t):
    """(tau_B0, tau_B(p)) in seconds from binary_delay_host; tau_B(p) is None for an orbit outside the limits."""
    from crimp_amd.binarymodels import binary_delay_host
    tm = R.plain(tm)
    tau0 = binary_delay_host(t, full_orbit(tm, [], []))
    try:
        tauf = binary_delay_host(t, full_orbit(tm, keys, p))
    except ValueError:
        tauf = None
    return tau0, tauf


def _wave_names(tm):
    return ["WAVE%d" % j for j in range(1, R.n_waves(tm) + 1)]


def _rates_host(tm, t, tau0):
    """(nu, nud) of par's spin phase at the emission time of B0: Taylor, the glitches active there, the waves."""
    pep = float(tm["PEPOCH"])
    fpar = [float(tm.get("F%d" % n, 0.0)) for n in range(13)]
    dt0 = (t - pep) * 86400.0 - tau0
    nu, nud = O._taylor64(fpar, dt0, 1), O._taylor64(fpar, dt0, 2)
    for j in range(1, R.n_glitches(tm) + 1):
        ep = float(tm["GLEP_%d" % j])
        f0, f1, f2, f0d, td = (float(tm.get("%s_%d" % (b, j), 0.0)) for b in ("GLF0", "GLF1", "GLF2", "GLF0D", "GLTD"))
        ds = (t - ep) * 86400.0 - tau0
        on = ds >= 0.0
        ex = np.zeros_like(t) if td == 0.0 else np.exp(-np.where(on, ds, 0.0) / (td * 86400.0))
        nu = nu + np.where(on, f0 + f1 * ds + 0.5 * f2 * ds * ds + f0d * ex, 0.0)
        nud = nud + np.where(on, f1 + f2 * ds - (0.0 if td == 0.0 else f0d * ex / (td * 86400.0)), 0.0)
    names = _wave_names(tm)
    if names:
        dw = (t - float(tm["WAVEEPOCH"])) - tau0 / 86400.0
        a1 = a2 = 0.0
        for j, name in enumerate(names, start=1):
            om = j * float(tm["WAVE_OM"])
            a, b = float(tm[name]["A"]), float(tm[name]["B"])
            s, c = np.sin(om * dw), np.cos(om * dw)
            a1 = a1 + (om / 86400.0) * (a * c - b * s)
            a2 = a2 - (om / 86400.0) ** 2 * (a * s + b * c)
        nu, nud = nu + float(tm["F0"]) * a1, nud + float(tm["F0"]) * a2
    return nu, nud


def delta_host(tm, keys, p, t):
    """delta_i(p) [n] in NumPy fp64 (model keys only, no PHOFF). +inf where the corrected orbit is outside the limits,
    NaN for a photon whose delay iteration did not converge."""
    tm = R.plain(tm)
    t = np.atleast_1d(np.asarray(t, dtype=np.float64)).ravel()
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    tau0, tauf = delays_host(tm, keys, p, t)
    if tauf is None:
        return np.full(t.shape, np.inf)
    ffit = O.fit_model(tm, keys, p)
    dtf = (t - float(tm["PEPOCH"])) * 86400.0 - tauf
    out = O._taylor64([float(ffit["F%d" % n]) for n in range(13)], dtf)
    tef = t - tauf / 86400.0
    entry = dict(zip(keys, p))
    if R.n_glitches(tm):
        gl = {k: v for k, v in tm.items() if k.startswith("GLEP_") or k.startswith("GLTD_")}
        for j in range(1, R.n_glitches(tm) + 1):
            for b in _GL_AMPS:
                gl["%s_%d" % (b, j)] = float(entry.get("%s_%d" % (b, j), 0.0))
        out = out + T.glitches(tef, gl)
    names = _wave_names(tm)
    if names and ("F0" in entry or any(k.startswith("WAVE") for k in keys)):
        df0 = float(entry.get("F0", 0.0))
        shape = {"WAVEEPOCH": tm["WAVEEPOCH"], "WAVE_OM": tm["WAVE_OM"]}
        corr, base = dict(shape), dict(shape)
        for name in names:
            corr[name] = {s: float(entry.get(name + "_" + s, 0.0)) for s in "AB"}
            base[name] = dict(tm[name])
        corr["F0"], base["F0"] = float(tm["F0"]) - df0, df0     # F0 A - (F0 - dF0)(A - dA) = (F0 - dF0) dA + dF0 A
        out = out + T.waves(tef, corr) + T.waves(tef, base)
    nu, nud = _rates_host(tm, t, tau0)
    dtau = tauf - tau0
    return out + dtau * (nu - (0.5 * nud) * dtau)


def terms_from_delta(x, d, theta, phoff=0.0, norm=None, ampShift=1.0):
    """Per-photon (ln(m / norm) with NaN where m <= 0, |d ln m / du|) for a given delta."""
    u = np.asarray(x, dtype=float) - d - phoff
    m, dm = PR.template_value(theta, u, norm, ampShift)
    nrm = float(PR._value(theta["norm"]) if norm is None else norm)
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.where(m > 0, np.log(np.where(m > 0, m, 1.0) / nrm), np.nan)
        slope = np.abs(dm / m)
    return ln, slope


def nll_host(t, x, tm, theta, pvec, keys, phoff=False, norm=None, ampShift=1.0):
    """NLL of one vector (PHOFF last if ``phoff``) through photon_reference.template_value; +inf for an inadmissible
    orbit, a photon whose solve did not converge or a template value <= 0."""
    p = np.asarray(pvec, dtype=float).reshape(-1)
    nd = len(keys)
    d = delta_host(tm, keys, p[:nd], t)
    if not np.all(np.isfinite(d)):
        return np.inf
    ln, _ = terms_from_delta(x, d, theta, p[nd] if phoff else 0.0, norm, ampShift)
    return np.inf if np.any(np.isnan(ln)) else -float(np.sum(ln))


def a_tau_host(tm, t):
    """A_tau of binary_reference._Orbit.at (the unit of a delay's rounding errors) restated in fp64, at the emission
    time binary_delay_host gives: 2 pi |orbits| s + (|E| + e |sin E| + |M|) s + mag, s = |D' / g'|."""
    import binary_reference as B
    from crimp_amd.binarymodels import binary_delay_host
    tm = R.plain(tm)
    t = np.atleast_1d(np.asarray(t, dtype=np.float64)).ravel()
    o = B.orbit_values(tm)
    tau = binary_delay_host(t, _orbit_of(O.full_model(tm, [], [])))
    tt0 = (t - o["t0"]) * 86400.0 - tau
    pbs = o["pb"] * 86400.0
    uu = tt0 / pbs
    orbits = uu - o["pbdot"] * uu * uu / 2
    m_r = 2 * np.pi * (orbits - np.rint(orbits))
    x = o["a1"] + o["a1dot"] * tt0
    dmdt = (2 * np.pi / pbs) * (1 - o["pbdot"] * uu)
    if o["bt"]:
        e = o["ecc"]
        E = m_r + e * np.sin(m_r) / np.sqrt(1 - 2 * e * np.cos(m_r) + e * e)
        for _ in range(60):
            E = E - np.clip((E - e * np.sin(E) - m_r) / (1 - e * np.cos(E)), -0.5, 0.5)
        s, c = np.sin(E), np.cos(E)
        w = np.deg2rad(o["om"]) + np.deg2rad(o["omdot"]) / (365.25 * 86400.0) * tt0
        sw, cw, s1 = np.sin(w), np.cos(w), np.sqrt(1 - e * e)
        al, be = x * sw, x * s1 * cw + o["gamma"]
        d1 = be * c - al * s
        mag = np.abs(al) * (np.abs(c) + e) + (x * s1 * np.abs(cw) + abs(o["gamma"])) * np.abs(s) + \
            np.abs(w) * np.abs(x) * (np.abs(cw) * (np.abs(c) + e) + s1 * np.abs(sw) * np.abs(s))
        kep = 1 - e * c
    else:
        E, e = m_r, 0.0
        s, c, s2, c2 = np.sin(E), np.cos(E), np.sin(2 * E), np.cos(2 * E)
        d1 = x * (c + o["eps2"] * c2 + o["eps1"] * s2)
        mag = np.abs(x) * (np.abs(s) + np.abs(o["eps2"] / 2 * s2) + np.abs(o["eps1"] / 2 * c2))
        kep = 1.0
    sens = np.abs(d1 / (kep + dmdt * d1))
    return 2 * np.pi * np.abs(orbits) * sens + (np.abs(E) + e * np.abs(s) + np.abs(m_r)) * sens + mag


# ------------------------------------------------------------------------------------------- the fixtures
class Case:
    """delta of one model over n photons: tm, keys, t [n], pvec [V, ndim], vectors (names), hi + lo [V, n], A [V, n]."""

    def __init__(self, name, n, tm, keys, t, pvec, vectors, hi, lo, a):
        self.name, self.n, self.tm, self.keys, self.t, self.pvec, self.vectors = name, n, tm, keys, t, pvec, vectors
        self.hi, self.lo, self.A = hi, lo.astype(np.float64), a.astype(np.float64)

    def err(self, d):
        """|d - delta_60| per element for the first rows of the case (the difference formed in long double)."""
        d = np.asarray(d, dtype=np.float64).reshape(-1, self.n)
        k = d.shape[0]
        ref = self.hi[:k].astype(np.longdouble) + self.lo[:k].astype(np.longdouble)
        return np.abs(d.astype(np.longdouble) - ref).astype(np.float64)

    def ratio(self, d):
        """max |d - delta_60| / (FACTOR u A): at most 1 inside the bound; inf for a NaN, or where A == 0 and d != 0."""
        e = self.err(d)
        a = self.A[:e.shape[0]]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(a > 0, e / (FACTOR * U * a), np.where(e == 0, 0.0, np.inf))
        r = np.where(np.isnan(e), np.inf, r)
        return float(np.max(r)) if r.size else 0.0

    def delta64(self):
        """The 60-digit delta rounded to fp64 [V, n]."""
        return (self.hi.astype(np.longdouble) + self.lo.astype(np.longdouble)).astype(np.float64)


def load_toa_cases():
    """{(name, n): Case} of tests/golden/orbit_fit.npz read as delta: all five models, the six ToA counts, the five
    vectors."""
    return {k: Case(c.name, c.n, c.tm, c.keys, c.t, c.pvec, O.VECTORS, c.hi, c.lo, c.A)
            for k, c in O.load_fixture().items()}


def load_golden(path=None):
    """{(name, n): Case} of tests/golden/photon_orbit.npz for n in GOLDEN_SIZES: prefixes of the stored arrays."""
    if path is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "photon_orbit.npz")
    g = np.load(path, allow_pickle=False)
    vec = tuple(json.loads(str(g["vectors"])))
    out = {}
    for name in json.loads(str(g["index"])):
        tm = json.loads(str(g[name + "_model"]))
        keys = json.loads(str(g[name + "_keys"]))
        for n in GOLDEN_SIZES:
            out[(name, n)] = Case(name, n, tm, keys, g[name + "_t"][:n], g[name + "_pvec"], vec,
                                  g[name + "_hi"][:, :n], g[name + "_lo"][:, :n], g[name + "_A"][:, :n])
    return out


def flagged_model(tm, keys):
    """A fixture's plain model as the flagged dict the package takes (BINARY carries no flag)."""
    return {k: ({"value": v, "flag": None} if k == "BINARY" or (isinstance(v, dict) and "A" in v)
                else {"value": v, "flag": int(k in keys)}) for k, v in tm.items()}


# ------------------------------------------------------------------------------------------- injection and recovery
INJECTION_SEED = 20241022
INJECTION_N = 20000
INJECTION_KEYS = ("F0", "A1", "TASC")
INJECTION_OFFSET = 3.0


def injection_model():
    """The truth: F0-only spin, ELL1 with PB = 2 h and A1 = 0.05 lt-s, ten orbits of data from PEPOCH on."""
    return {"PEPOCH": 58000.0, "F0": 9.87654321, "BINARY": "ELL1", "PB": 2.0 / 24.0, "A1": 0.05,
            "TASC": 58000.4 - 0.013, "EPS1": 0.0, "EPS2": 0.0}


def injection_photons(theta, seed=INJECTION_SEED, n=INJECTION_N):
    """Arrival MJDs of n photons: emission times uniform over ten orbits, thinned against the template at the truth's
    phase of the emission time (rejection, a seeded default_rng), arrival = emission + D(emission) / 86400."""
    tm = injection_model()
    th = {k: PR._value(v) for k, v in theta.items()}
    assert th["model"] == "fourier"
    rng = np.random.default_rng(seed)
    bound = th["norm"] + sum(abs(th[k]) for k in th if k.startswith("amp_"))
    span = 10.0 * tm["PB"]
    kept = []
    have = 0
    while have < n:
        te = rng.uniform(58000.4, 58000.4 + span, 2 * n)
        ph = tm["F0"] * ((te - tm["PEPOCH"]) * 86400.0)
        rate = PR.S.template_rate(th, ph - np.floor(ph))
        assert rate.min() >= 0.0
        te = te[rng.uniform(size=te.size) * bound < rate]
        kept.append(te)
        have += te.size
    te = np.concatenate(kept)[:n]
    orb = 2.0 * np.pi * (te - tm["TASC"]) / tm["PB"]
    return np.sort(te + tm["A1"] * np.sin(orb) / 86400.0)


def fold_host(tm, t):
    """The folded phase of a Taylor-only model with an orbit at the emission time, on the host (cycles in [0, 1))."""
    from crimp_amd.binarymodels import binary_delay_host
    tm = R.plain(tm)
    tau = binary_delay_host(t, _orbit_of(O.full_model(tm, [], [])))
    dt = (t - float(tm["PEPOCH"])) * 86400.0 - tau
    ph = O._taylor64([float(tm.get("F%d" % n, 0.0)) for n in range(13)], dt)
    return ph - np.floor(ph)


def injection_problem(theta):
    """{t, truth, par (flagged: the start model), keys, p_true, sigma, nll (the twin's, under par)} of the injection
    test: sigma is the observed-information sigma of the twin's NLL at the truth, the start model lies
    INJECTION_OFFSET sigma from the truth on every key (signs alternating), so p_true = par - truth."""
    truth = injection_model()
    keys = list(INJECTION_KEYS)
    t = injection_photons(theta)
    x0 = fold_host(truth, t)

    def f0(p):
        return nll_host(t, x0, truth, theta, p, keys)

    dphi = 3e-3
    scale = np.array([dphi / (10 * truth["PB"] * 86400.0), dphi / truth["F0"],
                      dphi / (truth["F0"] * truth["A1"] * 2 * np.pi / truth["PB"])])
    sig = scale
    for _ in range(2):
        sig = np.sqrt(np.diag(np.linalg.inv(PR.hessian(f0, np.zeros(3), 0.3 * sig))))
    start = dict(truth)
    for i, k in enumerate(keys):
        start[k] = truth[k] + INJECTION_OFFSET * sig[i] * (-1.0) ** i
    p_true = np.array([start[k] - truth[k] for k in keys])
    x = fold_host(start, t)
    return {"t": t, "truth": truth, "par": flagged_model(start, keys), "start": start, "keys": keys, "p_true": p_true,
            "sigma": sig, "x": x, "nll": lambda p: nll_host(t, x, start, theta, p, keys)}
