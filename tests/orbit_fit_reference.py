"""The model residual of the orbit fits (csrc/orbit_fit.h) at 60 digits, the unit its fp64 rounding
errors scale with, and a NumPy fp64 twin of the definition. Built on binary_reference.py (delay_mp, the Taylor part at
the emission time) and phase_reference.py (FACTOR, U, the fixture's hi / lo / A encodings).

Definition. par is a model with an orbit B0, keys its free keys, p the correction vector; full(p)[k] = fl(par[k] - p[k])
-- the fp64 difference, the number the patched .par holds; PBDOT and A1DOT in dimensionless form. B(p) is the orbit of
full(p), tau_B(t) the delay of binary_reference.py.

    te0 = t - tau_B0(t) / 86400,   teF = t - tau_B(p)(t) / 86400
    m_i(p) = phi_fit(p)(teF_i) + R_i(p),   R_i(p) = phi_par(te0_i) - phi_par(teF_i),   mu = m - mean(m)

phi_fit(p) is the fit model (every non-epoch scalar 0, the free spin keys their p entries), phi_par the spin model of
par. The models here are the Taylor-only ones of the calcphase_binary set (no glitches, no waves): ``residual_mp`` and
the twin assert it. ``residual_mp`` evaluates R exactly (both phases at 60 digits), not by its series.

The error unit A_i, by counting roundings as binary_reference.py does (u = 2**-53, FACTOR = 32, FACTOR_TAU = 16):

* phi_fit at the emission time: binary_reference's unit of the Taylor part for the fit model at teF,
  sum_n |p_{n-1} dt^n / n!| + (FACTOR_TAU / FACTOR) |d phi_fit / dt'| A_tau(B(p));
* R = dtau (nu - nud dtau / 2), dtau = tau_B(p) - tau_B0: each delay is within FACTOR_TAU u A_tau of its value, and
  the difference multiplies nu: |nu_i| (FACTOR_TAU / FACTOR) (A_tau(B0) + A_tau(B(p))). The product itself, nu (a
  Taylor sum: 16 roundings at most), the subtraction and the nud term cost fewer than FACTOR roundings of |R|: + |R_i|;
* the series drops |phi_par'''| |dtau|^3 / 6 (bounded with the largest |phi_par'''| between the two emission times):
  an absolute error, entered as itself / (FACTOR u) so that FACTOR u A_i contains it once.

``mu_bound``: FACTOR u (A_i + mean(A)) -- the mean's share of the errors -- plus the roundings of the mean itself:
wave_sum adds ceil(n / 64) values per lane and six butterfly steps, the division and the subtraction add two:
(ceil(n / 64) + 8) u (mean|m| + |m_i|). ``nll_bound`` is what that implies for the NLL: sum_i (|r_i| d_i + d_i^2 / 2)
with d_i = mu_bound_i / yerr_i, plus (ceil(n / 64) + 16) u sum_i (r_i^2 + |log(2 pi yerr_i^2)|) for the NLL's own sums
(r, its square, the log within 2 ulp, the same summation tree).

``load_fixture`` reads tests/golden/orbit_fit.npz (tests/golden/gen_orbit_fit_golden.py) and needs no mpmath.
"""
import json
import math
import os

import numpy as np

import binary_reference as B
import phase_reference as R

U, FACTOR, FACTOR_TAU = R.U, R.FACTOR, B.FACTOR_TAU
MODELS = ("bt_e07", "bt_e095", "bt_full", "ell1_amxp", "hmxb_wide")
SIZES = (1, 2, 63, 64, 65, 257)
VECTORS = ("zero", "orbital", "spin", "typical", "wide")      # row order of every case's arrays
ORBITAL = ("PB", "A1", "T0", "TASC", "ECC", "E", "OM", "OMDOT", "GAMMA", "EPS1", "EPS2", "PBDOT", "A1DOT", "XDOT")
DIMENSIONLESS = ("PBDOT", "A1DOT", "XDOT")


def free_keys(tm):
    """The free keys of a fixture model: F0, F1 and every orbital number its kind has and its .par sets."""
    bt = str(tm["BINARY"]).upper() == "BT"
    keys = ["F0", "F1", "PB", "A1"] + (["T0", "ECC", "OM"] if bt else ["TASC", "EPS1", "EPS2"])
    keys += [k for k in ("OMDOT", "GAMMA", "PBDOT", "A1DOT") if k in tm]
    return keys


def widths(tm, t):
    """A correction per free key that moves the phase by about 1e-3 cycles over the span of ``t`` (what a posterior of
    ToAs with errors of 1e-3 cycles is wide), capped so that 1e3 widths stay inside the orbit's limits -- and, for PBDOT
    and A1DOT, below the 1e-7 above which a .par value is read in units of 1e-12 (binary_reference.orbit_values applies
    that convention to whatever it is given)."""
    f0, a1, pb = float(tm["F0"]), float(tm["A1"]), float(tm["PB"]) * 86400.0
    span = max(float(np.max(t) - np.min(t)), float(tm["PB"])) * 86400.0
    k = 2 * math.pi * a1 / pb          # d tau / d (orbital phase in s)
    dph = 1e-3
    w = {"F0": dph / span, "F1": 2 * dph / span ** 2, "A1": min(dph / f0, 1e-4 * a1),
         "PB": min(dph / f0 / (k * span / pb) / 86400.0, 1e-5 * pb / 86400.0),
         "T0": min(dph / f0 / k / 86400.0, 1e-5 * pb / 86400.0), "ECC": min(dph / (f0 * a1), 2e-5),
         "OM": min(dph / (f0 * a1) * 180 / math.pi, 0.01), "EPS1": min(dph / (f0 * a1), 1e-6),
         "EPS2": min(dph / (f0 * a1), 1e-6), "OMDOT": min(dph / (f0 * a1) * 180 / math.pi, 0.01) / (span / 31557600.0),
         "GAMMA": min(dph / f0, 1e-5), "PBDOT": min(dph / f0 / (2 * math.pi * a1) * 2 / (span / pb) ** 2, 4e-11),
         "A1DOT": min(min(dph / f0, 1e-4 * a1) / span, 4e-11)}
    w["TASC"] = w["T0"]
    return w


def vectors(tm, t):
    """[5, ndim]: the VECTORS of a model, signs alternating with the key's position."""
    keys = free_keys(tm)
    w = widths(tm, t)
    base = np.array([w[k] * (0.7 + 0.1 * i) * (-1.0) ** i for i, k in enumerate(keys)])
    orb = np.array([k in ORBITAL for k in keys])
    return np.vstack([0 * base, np.where(orb, base, 0.0), np.where(orb, 0.0, base), base, 1e3 * base])


def toa_set(times, n):
    """n of a model's fixture times, evenly strided over the sorted array (n = 1: the middle one)."""
    ts = np.sort(np.asarray(times, dtype=np.float64))
    if n == 1:
        return ts[ts.size // 2: ts.size // 2 + 1].copy()
    return ts[np.round(np.linspace(0, ts.size - 1, n)).astype(int)].copy()


def _tiny(v):
    v = float(v)
    return v * 1e-12 if abs(v) > 1e-7 else v


def _check_taylor_only(tm):
    assert R.n_glitches(tm) == 0 and R.n_waves(tm) == 0, "the orbit-fit reference covers Taylor-only spin models"


def full_model(tm, keys, p):
    """par with the vector applied: fl(par - p) on every free key, PBDOT and A1DOT as dimensionless numbers."""
    tm = R.plain(tm)
    out = dict(tm)
    for k in DIMENSIONLESS:
        if k in out:
            out[k] = _tiny(out[k])
    for k, d in zip(keys, p):
        out[k] = np.float64(out[k]) - np.float64(d)
    for k in DIMENSIONLESS:
        assert k not in out or abs(out[k]) <= 1e-7, "a dimensionless %s above 1e-7 would be read in units of 1e-12" % k
    return out


def fit_model(tm, keys, p):
    """The fit model: PEPOCH kept, every F 0 but the free ones, which are their p entries."""
    tm = R.plain(tm)
    out = {"PEPOCH": tm["PEPOCH"]}
    for n in range(13):
        out["F%d" % n] = 0.0
    for k, d in zip(keys, p):
        if k not in ORBITAL:
            out[k] = float(d)
    return out


def residual_mp(tm, keys, p, t):
    """([m_i], [A_i]) at 60 digits for one vector."""
    mp = B._mp()
    f = mp.mpf
    tm = R.plain(tm)
    _check_taylor_only(tm)
    t = np.atleast_1d(np.asarray(t, dtype=np.float64)).ravel()
    full = full_model(tm, keys, p)
    tau0, a0 = B.delay_mp(tm, t)
    tauf, af = B.delay_mp(full, t, starts=[float(x) for x in tau0])
    pep = f(float(tm["PEPOCH"]))
    dt0 = [(f(float(x)) - pep) * 86400 - d for x, d in zip(t, tau0)]
    dtf = [(f(float(x)) - pep) * 86400 - d for x, d in zip(t, tauf)]
    fit = B._taylor(fit_model(tm, keys, p), dtf)
    par0 = B._taylor(tm, dt0)
    parf = B._taylor(tm, dtf)
    coef = [f(float(tm["F%d" % (n - 1)])) / mp.factorial(n) for n in range(1, 14)]
    w = f(FACTOR_TAU) / f(FACTOR)
    val, mag = [], []
    for i in range(t.size):
        r = par0[0][i] - parf[0][i]
        dtau = tauf[i] - tau0[i]
        d3 = max(abs(mp.fsum(n * (n - 1) * (n - 2) * coef[n - 1] * x ** (n - 3) for n in range(3, 14)))
                 for x in (dt0[i], dtf[i]))
        cubic = d3 * abs(dtau) ** 3 / 6
        a = fit[1][i] + w * abs(fit[2][i]) * af[i]
        a += abs(par0[2][i]) * w * (a0[i] + af[i]) + abs(r)
        a += cubic / (f(FACTOR) * f(U))
        val.append(fit[0][i] + r)
        mag.append(a)
    return val, mag


# ------------------------------------------------------------------------------------------- bounds
def mu_bound(A, m):
    """Per ToA: the most an fp64 mu may differ from the 60-digit m - mean(m)."""
    A, m = np.asarray(A, dtype=np.float64), np.asarray(m, dtype=np.float64)
    n = A.shape[-1]
    adds = math.ceil(n / 64) + 8
    return (FACTOR * U * (A + np.mean(A, axis=-1, keepdims=True))
            + adds * U * (np.mean(np.abs(m), axis=-1, keepdims=True) + np.abs(m)))


def nll_exact(y, mu, yerr):
    """gaussian_nll(y - mean(y), mu, yerr) with every sum exact (math.fsum)."""
    y = np.asarray(y, dtype=np.float64)
    yc = y - math.fsum(y) / y.size
    r = (yc - mu) / yerr
    return 0.5 * math.fsum(r * r + np.log(2.0 * np.pi * yerr ** 2))


def nll_bound(y, mu, yerr, dmu):
    """The most an fp64 NLL may differ from nll_exact when its mu is within dmu."""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    yc = y - math.fsum(y) / n
    r = np.abs((yc - mu) / yerr)
    d = (dmu + (math.ceil(n / 64) + 8) * U * (np.mean(np.abs(y)) + np.abs(y))) / yerr
    own = (math.ceil(n / 64) + 16) * U * math.fsum(r * r + np.abs(np.log(2.0 * np.pi * yerr ** 2)))
    return math.fsum(r * d + 0.5 * d * d) + own


# ------------------------------------------------------------------------------------------- the NumPy fp64 twin
def _taylor64(coef_f, dt, deriv=0):
    """sum_n F_{n-1} / n! dt^n (deriv = 0), its first or its second derivative in dt, summed in increasing n."""
    out = np.zeros_like(dt)
    fact = 1.0
    for k in range(13):
        fact *= k + 1
        c = (1.0 / fact) * coef_f[k]
        if coef_f[k] == 0.0:
            continue
        if deriv == 0:
            out = out + c * dt ** (k + 1)
        elif deriv == 1:
            out = out + ((k + 1) * c) * dt ** k
        elif k >= 1:
            out = out + ((k + 1) * k * c) * dt ** (k - 1)
    return out


def residual_host(tm, keys, p, t):
    """m_i(p) in NumPy fp64, as the kernels form it: the delays from binary_delay_host (the device loop step for
    step), phi_fit at the emission time of the corrected orbit, R = dtau (nu - nud dtau / 2). NaN where the corrected
    orbit is outside the limits (binary_params raises)."""
    from crimp_amd.binarymodels import binary_delay_host
    tm = R.plain(tm)
    _check_taylor_only(tm)
    t = np.atleast_1d(np.asarray(t, dtype=np.float64)).ravel()
    full = full_model(tm, keys, p)
    base = full_model(tm, [], [])
    orbit = {k: v for k, v in full.items() if k in ORBITAL or k == "BINARY"}
    orbit0 = {k: v for k, v in base.items() if k in ORBITAL or k == "BINARY"}
    try:
        tauf = binary_delay_host(t, orbit)
    except ValueError:
        return np.full(t.shape, np.nan)
    tau0 = binary_delay_host(t, orbit0)
    pep = float(tm["PEPOCH"])
    fpar = [float(tm.get("F%d" % n, 0.0)) for n in range(13)]
    ffit = fit_model(tm, keys, p)
    ffit = [float(ffit["F%d" % n]) for n in range(13)]
    dt0 = (t - pep) * 86400.0 - tau0
    dtf = (t - pep) * 86400.0 - tauf
    nu, nud = _taylor64(fpar, dt0, 1), _taylor64(fpar, dt0, 2)
    dtau = tauf - tau0
    return _taylor64(ffit, dtf) + dtau * (nu - (0.5 * nud) * dtau)


def mu_host(tm, keys, p, t):
    m = residual_host(tm, keys, p, t)
    return m - np.mean(m)


# ------------------------------------------------------------------------------------------- the fixture
class Case:
    """One (model, n) of orbit_fit.npz: tm, keys, t [n], pvec [5, ndim], m as hi + lo [5, n], A [5, n]."""

    def __init__(self, name, n, tm, keys, t, pvec, hi, lo, a):
        self.name, self.n, self.tm, self.keys, self.t, self.pvec = name, n, tm, keys, t, pvec
        self.hi, self.lo, self.A = hi, lo.astype(np.float64), a.astype(np.float64)

    @property
    def m(self):
        return self.hi + self.lo

    def _ref_ld(self, j):
        m = self.hi[j].astype(np.longdouble) + self.lo[j].astype(np.longdouble)
        return m - np.sum(m) / self.n

    def mu_err(self, mu):
        """|mu - (m - mean(m))| per element against the 60-digit value, mu [P, n] for the first P vectors (the
        difference is formed in long double: its own rounding is 2**-11 of fp64's)."""
        mu = np.asarray(mu, dtype=np.float64).reshape(-1, self.n)
        return np.array([np.abs(mu[j].astype(np.longdouble) - self._ref_ld(j)).astype(np.float64)
                         for j in range(mu.shape[0])])

    def mu_ref(self):
        """m - mean(m) rounded to fp64 [5, n]."""
        return np.array([self._ref_ld(j).astype(np.float64) for j in range(self.hi.shape[0])])

    def bound(self):
        return mu_bound(self.A, self.m)


def load_fixture(path=None):
    """{(name, n): Case} of tests/golden/orbit_fit.npz."""
    if path is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orbit_fit.npz")
    g = np.load(path, allow_pickle=False)
    out = {}
    for name in json.loads(str(g["index"])):
        tm = json.loads(str(g[name + "_model"]))
        keys = json.loads(str(g[name + "_keys"]))
        for n in SIZES:
            k = "%s_%d" % (name, n)
            out[(name, n)] = Case(name, n, tm, keys, g[k + "_t"], g[name + "_pvec"], g[k + "_hi"], g[k + "_lo"],
                                  g[k + "_A"])
    return out


# ------------------------------------------------------------------------------------------- injection and recovery
INJECTION = {
    # name: (fixture model it starts from, ToA span (MJD), ToA error (cycles), seed)
    "ell1": ("ell1_amxp", (58000.0, 58010.0), 2e-3, 20240611),
    "bt": ("bt_e07", (57900.0, 58100.0), 2e-3, 20240612),
}
INJECTION_NTOA = 64
INJECTION_OFFSET = 3.0       # |p_true| in units of the linearised sigma of its key


def jacobian_host(tm, keys, p, t, steps):
    """d mu / d p [n, ndim] of the twin by central differences with the given steps."""
    cols = []
    for k, h in enumerate(steps):
        d = np.zeros(len(keys))
        d[k] = h
        cols.append((mu_host(tm, keys, p + d, t) - mu_host(tm, keys, p - d, t)) / (2 * h))
    return np.array(cols).T


def linear_sigma(tm, keys, p, t, yerr, steps):
    """(sigma [ndim], covariance) of the linearised least squares at p: (J^T W J)^-1, solved in units of the steps."""
    j = jacobian_host(tm, keys, p, t, steps) * steps / yerr[:, None]
    cov = np.linalg.inv(j.T @ j) * np.outer(steps, steps)
    return np.sqrt(np.diag(cov)), cov


def injection_problem(name):
    """{tm (flagged), keys, t, y, yerr, p_true, sigma, cov, steps}: 64 ToAs drawn from full(p_true) of the model, with
    Gaussian errors of a fixed seed. p_true lies INJECTION_OFFSET linearised sigma from 0 on every key, signs
    alternating; y is the twin's m(p_true) plus the noise, mean-subtracted."""
    src, (t0, t1), err, seed = INJECTION[name]
    tm = dict(B.load_binary()[src].tm)
    if "TASC" in tm:
        tm["TASC"] = 0.5 * (t0 + t1) - 0.04   # an epoch inside the data: 1e5 orbits away, PB and TASC are one parameter
    free = [k for k in free_keys(tm) if k in ("F0", "F1", "PB", "A1", "T0", "TASC", "ECC", "OM", "EPS1", "EPS2")]
    keys = [k for k in tm if k in free]          # the model's order: what list_orbit_fit_keys gives for the flags
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(t0, t1, INJECTION_NTOA))
    yerr = err * rng.uniform(0.5, 1.5, INJECTION_NTOA)
    w = widths(tm, t)
    steps = np.array([w[k] for k in keys])
    zero = np.zeros(len(keys))
    sigma, _ = linear_sigma(tm, keys, zero, t, yerr, steps)
    p_true = INJECTION_OFFSET * sigma * (-1.0) ** np.arange(len(keys))
    sigma, cov = linear_sigma(tm, keys, p_true, t, yerr, sigma)
    y = residual_host(tm, keys, p_true, t) + yerr * rng.standard_normal(INJECTION_NTOA)
    flagged = {k: ({"value": v, "flag": None} if k == "BINARY" else {"value": v, "flag": int(k in keys)})
               for k, v in tm.items()}
    return {"tm": flagged, "keys": keys, "t": t, "y": y - np.mean(y), "yerr": yerr, "p_true": p_true, "sigma": sigma,
            "cov": cov, "steps": sigma}


def least_squares_host(prob, iters=8):
    """The twin's own Gauss-Newton solution from p = 0 (what the device minimiser has to find)."""
    tm, keys, t = R.plain(prob["tm"]), prob["keys"], prob["t"]
    p = np.zeros(len(keys))
    h = prob["steps"]
    for _ in range(iters):
        j = jacobian_host(tm, keys, p, t, h) * h / prob["yerr"][:, None]
        r = (prob["y"] - mu_host(tm, keys, p, t)) / prob["yerr"]
        p = p + np.linalg.lstsq(j, r, rcond=None)[0] * h
    return p
