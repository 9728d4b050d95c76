"""The orbit search (crimp_orbit_search) in long double, with the unit its fp64 errors scale
with, and the cases tests/test_gpu_orbit_search.py runs. No GPU, no mpmath.

Truth.  An orbit is the dict of ``binary_reference.orbit_values`` (fp64 numbers, taken exactly). ``delay_ld`` evaluates
the definition of csrc/binary_delay.h in ``np.longdouble``: tau is the root of F(tau) = tau - D(tta - tau), tta = (t -
T0|TASC) 86400, found by Newton on F with the full derivative
    dD/dtt = D_E Mdot / (1 - e cos E) + A1DOT dD/dx + OMDOT dD/dw,   Mdot = (2 pi / pb)(1 - PBDOT tt / pb),
every D evaluated from its own Kepler root (long-double Newton from the starter M + e sin M / sqrt(1 - 2 e cos M + e^2),
steps cut to 1 rad), with long-double sin / cos. Both iterations stop when a step is below 1e-18 (of max(1, |value|):
long double resolves 1.1e-19 of the value), or one step after a step below 1e-10 (Newton is quadratic there: that step
lands below 1e-20, under the resolution, and may not report itself below 1e-18 at |tau| of hundreds of seconds).
Nothing of the fp64 iteration (its bracket, its joint equation in E, its fixed point for x and w) is used. The
arguments are exact: t - T0 is a difference of doubles, the product by 86400 rounds at 2^-64.

``dt_truth`` = (t - tref) 86400 - tau in long double, rounded once to fp64. The sums over those dt are
``search_reference.Truth``'s (the argument carried exactly).

Unit of a trial.  ``unit`` = search_reference.fp64_unit(Truth(dt_truth, f, c2, m)) -- the kernel's phase B is
k_search_f64's arithmetic -- plus ``stat_bound(cumulative_bound(d))`` of the harmonic bound
    d_k = 2 pi k sum_i (|f| + 2 |c2 dt_i|) eps_i,
|d ph / d dt| eps summed over the photons (|e^{ia} - e^{ib}| <= |a - b|), where eps_i bounds |dt_kernel - dt_truth|
(u = 2^-53):
  * a = fl(fl(t - tref) 86400): the product rounds, u |a|; the difference is exact when tref / 2 <= t <= 2 tref
    (Sterbenz) and rounds otherwise, another u |a|;
  * fl(a - tau): u |dt|; and dt_truth is itself rounded to fp64: u |dt|;
  * tau: FACTOR_TAU u A_tau (binary_reference's FACTOR_TAU = 16).
A_tau is binary_reference's unit restated in NumPy for an arbitrary orbit (``a_tau``), by the same count of roundings:
  * orbital phase: orbits = tt / pb - PBDOT (tt / pb)^2 / 2 carries at most 6 roundings relative to |orbits| (PB 86400,
    (t - T0) 86400 and its difference, the subtraction of tau, the division, the small PBDOT term); an error dM of the
    mean anomaly moves the delay by D' dM / g', g' = 1 - e cos E + Mdot D': unit 2 pi |orbits| |D' / g'|;
  * solve: g = (E - e sin E) - M at the reduced angles, at most 8 roundings on any term: (|E| + e |sin E| + |M_r|)
    |D' / g'|;
  * delay: D's own products and trigonometry, at most 16 roundings on a term: x |sin w| (|cos E| + e) + (x sqrt(1 - e^2)
    |cos w| + |GAMMA|) |sin E|, plus the angle w = OM pi / 180 + OMDOT tt at its absolute size, |w| x (|cos w| (|cos E| +
    e) + sqrt(1 - e^2) |sin w| |sin E|); ELL1: x (|sin P| + |EPS2 / 2 sin 2P| + |EPS1 / 2 cos 2P|).
A_tau is their sum. The device derives the orbit with make_binmodel's expressions (of_derive), so the count is the one
tests/test_gpu_binary.py holds crimp_binary_delay to. The unit is a function of the truth and the inputs only.
"""
import math

import numpy as np

import search_reference as SR

LD = np.longdouble
U = SR.U
FACTOR_TAU = 16.0
PI = SR.PI_LD
TWO_PI = 2 * PI
assert np.finfo(LD).nmant >= 63, "the truth needs an extended long double"


def orbit_of(tm):
    """The orbit dict of a plain timing-model dict (binary_reference.orbit_values, restated: no phase_reference)."""
    name = str(tm["BINARY"]).upper()
    assert name in ("BT", "ELL1")
    bt = name == "BT"

    def tiny(v):
        v = float(v)
        return v * 1e-12 if abs(v) > 1e-7 else v

    def get(*keys):
        for k in keys:
            if k in tm:
                return float(tm[k])
        return 0.0
    return {"bt": bt, "pb": get("PB"), "pbdot": tiny(get("PBDOT")), "a1": get("A1"),
            "a1dot": tiny(get("A1DOT", "XDOT")), "t0": get("T0") if bt else get("TASC"),
            "ecc": get("ECC", "E") if bt else 0.0, "om": get("OM") if bt else 0.0, "omdot": get("OMDOT") if bt else 0.0,
            "gamma": get("GAMMA") if bt else 0.0, "eps1": 0.0 if bt else get("EPS1"), "eps2": 0.0 if bt else get("EPS2")}


_ALIASES = {"TASC": "t0", "T0": "t0", "E": "ecc", "XDOT": "a1dot"}


def with_keys(orbit, keys, values):
    """``orbit`` with the keyed fields (the .par's names) replaced by ``values``."""
    o = dict(orbit)
    for k, v in zip(keys, values):
        o[_ALIASES.get(k.upper(), k.lower())] = float(v)
    return o


class _Eval:
    """D, its derivatives and the pieces of A_tau at the emission times tt (s since T0|TASC, long double)."""

    def __init__(self, o, tt):
        ld = lambda k: LD(o[k])
        pbs = ld("pb") * 86400
        u = tt / pbs
        self.orbits = u - ld("pbdot") * u * u / 2
        m_r = TWO_PI * (self.orbits - np.rint(self.orbits))
        self.mdot = (TWO_PI / pbs) * (1 - ld("pbdot") * u)
        x = ld("a1") + ld("a1dot") * tt
        if o["bt"]:
            e = ld("ecc")
            E = m_r + e * np.sin(m_r) / np.sqrt(1 - 2 * e * np.cos(m_r) + e * e)
            idx = np.arange(E.size)          # the times still iterating
            polish = np.zeros(E.size, bool)
            for _ in range(200):
                Ei, Mi = E[idx], m_r[idx]
                dE = (Ei - e * np.sin(Ei) - Mi) / (1 - e * np.cos(Ei))
                dE = np.where(np.abs(dE) > 1, np.sign(dE), dE)
                E[idx] = Ei - dE
                done = (np.abs(dE) < LD(1e-18) * np.maximum(1, np.abs(E[idx]))) | polish
                polish = (np.abs(dE) < LD(1e-10))[~done]
                idx = idx[~done]
                if idx.size == 0:
                    break
            live = idx
            assert live.size == 0, "Kepler's equation did not converge"
            s, c = np.sin(E), np.cos(E)
            deg = PI / 180
            wdot = ld("omdot") * deg / (LD(36525) / 100 * 86400)
            w = ld("om") * deg + wdot * tt
            sw, cw = np.sin(w), np.cos(w)
            s1 = np.sqrt(1 - e * e)
            al, be = x * sw, x * s1 * cw + ld("gamma")
            self.D = al * (c - e) + be * s
            self.D1 = be * c - al * s
            kep = 1 - e * c
            # d D / d tt at fixed E: through x and through w
            self.Dt = ld("a1dot") * (sw * (c - e) + s1 * cw * s) + wdot * x * (cw * (c - e) - s1 * sw * s)
            self.mag = np.abs(al) * (np.abs(c) + e) + (x * s1 * np.abs(cw) + abs(ld("gamma"))) * np.abs(s) + \
                np.abs(w) * np.abs(x) * (np.abs(cw) * (np.abs(c) + e) + s1 * np.abs(sw) * np.abs(s))
        else:
            E, e = m_r, LD(0)
            s, c = np.sin(E), np.cos(E)
            s2, c2 = np.sin(2 * E), np.cos(2 * E)
            shape = s + ld("eps2") / 2 * s2 - ld("eps1") / 2 * c2
            self.D = x * shape
            self.D1 = x * (c + ld("eps2") * c2 + ld("eps1") * s2)
            kep = LD(1) + 0 * E
            self.Dt = ld("a1dot") * shape
            self.mag = np.abs(x) * (np.abs(s) + np.abs(ld("eps2") / 2 * s2) + np.abs(ld("eps1") / 2 * c2))
        self.kep = kep
        gp = kep + self.mdot * self.D1
        sens = np.abs(self.D1 / gp)
        self.a_tau = TWO_PI * np.abs(self.orbits) * sens + (np.abs(E) + e * np.abs(s) + np.abs(m_r)) * sens + self.mag


def _solve(o, t):
    """(tau, A_tau) in long double; A_tau is evaluated one step (< 1e-10 s) before the root, which a unit does not
    see."""
    t = np.atleast_1d(np.asarray(t, np.float64)).ravel()
    tta = (t.astype(LD) - LD(o["t0"])) * 86400
    tau = np.zeros(t.shape, LD)
    a = np.zeros(t.shape, LD)
    idx = np.arange(t.size)          # the times still iterating
    polish = np.zeros(t.size, bool)
    for _ in range(100):
        ev = _Eval(o, tta[idx] - tau[idx])
        step = (tau[idx] - ev.D) / (1 + ev.D1 * ev.mdot / ev.kep + ev.Dt)
        tau[idx] -= step
        a[idx] = ev.a_tau
        done = (np.abs(step) < LD(1e-18) * np.maximum(1, np.abs(tau[idx]))) | polish
        polish = (np.abs(step) < LD(1e-10))[~done]
        idx = idx[~done]
        if idx.size == 0:
            break
    assert idx.size == 0, "the light-travel equation did not converge"
    return tau, a


def delay_ld(orbit, t):
    """tau (s, long double) of every arrival time t (MJD, fp64 taken exactly)."""
    return _solve(orbit, t)[0]


def a_tau(orbit, t):
    """The unit A_tau (fp64) of every arrival time: |tau_fp64 - tau| <= FACTOR_TAU u A_tau."""
    return _solve(orbit, t)[1].astype(np.float64)


def dt_truth(orbit, t, tref):
    """(dt fp64, eps fp64): the emission times in seconds since tref, rounded once; the bound on |dt_kernel - dt|."""
    t = np.atleast_1d(np.asarray(t, np.float64)).ravel()
    tau, atau = _solve(orbit, t)
    a = (t.astype(LD) - LD(float(tref))) * 86400
    dt = (a - tau).astype(np.float64)
    tref = float(tref)
    sterbenz = (t >= tref / 2) & (t <= 2 * tref) if tref > 0 else np.zeros(t.shape, bool)
    absa = np.abs(a).astype(np.float64)
    eps = U * absa * np.where(sterbenz, 1.0, 2.0) + 2.0 * U * np.abs(dt) + FACTOR_TAU * U * atau.astype(np.float64)
    return dt, eps * SR.GROW


def trial_unit(T, eps, stat):
    """The unit of every trial of the Truth T (its dt from ``dt_truth``, with eps)."""
    k = np.arange(1, T.m + 1, dtype=np.float64)
    w = np.abs(T.f) * float(eps.sum())
    if T.c2 is not None:
        w = w + 2.0 * np.abs(T.c2) * float((np.abs(T.dt) * eps).sum())
    d = 2.0 * math.pi * k[:, None] * w[None, :]
    return SR.fp64_unit(T, stat) + SR.stat_bound(T.g, SR.cumulative_bound(T.A, d, T.n), stat)


def truth_and_unit(orbit, t, tref, f, fdot, m, stat):
    """(power fp64 [J], unit [J]) of the trials f under ``orbit``."""
    dt, eps = dt_truth(orbit, t, tref)
    f = np.atleast_1d(np.asarray(f, np.float64))
    c2 = None if fdot == 0.0 else np.full(f.shape, 0.5 * fdot)
    T = SR.Truth(dt, f, c2, m)
    return T.power(stat), trial_unit(T, eps, stat)


# ------------------------------------------------------------------------------------------------- the cases
KAPPA = 4.0     # concentration of the pulse exp(KAPPA (cos 2 pi phi - 1)): harmonics up to ~6 above the noise
SPAN = 0.31     # days of data
MODELS = {
    "ell1": {"PEPOCH": 58000.0, "F0": 401.0, "BINARY": "ELL1", "PB": 0.084, "A1": 0.063, "TASC": 57999.93,
             "EPS1": 1e-5, "EPS2": -2e-5},
    "bt_e0": {"PEPOCH": 58000.0, "F0": 29.7, "BINARY": "BT", "PB": 0.21, "A1": 1.2, "T0": 57999.95, "ECC": 0.0,
              "OM": 70.0},
    "bt_e07": {"PEPOCH": 58000.0, "F0": 29.7, "BINARY": "BT", "PB": 0.21, "A1": 1.2, "T0": 57999.95, "ECC": 0.7,
               "OM": 70.0, "OMDOT": 30.0, "GAMMA": 1e-4},
    "bt_e095": {"PEPOCH": 58000.0, "F0": 29.7, "BINARY": "BT", "PB": 0.21, "A1": 1.2, "T0": 57999.95, "ECC": 0.95,
                "OM": 70.0},
}


def draw_photons(tm, n, f0, fdot, seed, sort=True):
    """n arrival times (MJD) in [58000, 58000 + SPAN) drawn by thinning from the pulse exp(KAPPA (cos 2 pi phi - 1)),
    phi = f0 dt + fdot dt^2 / 2 at the emission time under tm's orbit (dt in seconds since the mid-span)."""
    from crimp_amd.binarymodels import binary_delay_host
    rng = np.random.default_rng(seed)
    out = np.zeros(0)
    tref = 58000.0 + SPAN / 2
    while out.size < n:
        t = 58000.0 + rng.uniform(0.0, SPAN, 4 * n + 64)
        dt = (t - tref) * 86400.0 - binary_delay_host(t, tm)
        ph = f0 * dt + 0.5 * fdot * dt * dt
        keep = rng.uniform(0.0, 1.0, t.size) < np.exp(KAPPA * (np.cos(2 * np.pi * ph) - 1.0))
        out = np.concatenate([out, t[keep]])
    out = out[:n]
    return np.sort(out) if sort else out


class Case:
    """One search: photons of a known orbit, a grid of orbits that holds it, a frequency list that holds the spin."""

    def __init__(self, name, model, n, nf, m, stat, fdot, axes, seed, sort=True, jtrue=None):
        self.name, self.tm, self.n, self.nf, self.m, self.stat, self.fdot = name, MODELS[model], n, nf, m, stat, fdot
        self.f0 = float(self.tm["F0"])
        self.t = draw_photons(self.tm, n, self.f0, fdot, seed, sort)
        self.tref = 58000.0 + SPAN / 2
        self.jtrue = nf // 2 if jtrue is None else jtrue
        self.freq = self.f0 + (np.arange(nf) - self.jtrue) / (SPAN * 86400.0)
        self.keys = list(axes)
        # every axis: points around the true value, the true value the middle one
        self.axes = {k: float(self.tm[k]) + np.arange(-(cnt // 2), cnt - cnt // 2) * step
                     for k, (cnt, step) in axes.items()}
        mesh = np.meshgrid(*[self.axes[k] for k in self.keys], indexing="ij")
        self.orbits = np.stack([g.ravel() for g in mesh], axis=1)
        self.otrue = int(np.ravel_multi_index([cnt // 2 for cnt, _ in axes.values()],
                                              [cnt for cnt, _ in axes.values()]))
        self.base = orbit_of(self.tm)

    def orbit(self, o):
        return with_keys(self.base, self.keys, self.orbits[o])

    def truth(self, o, trials):
        return truth_and_unit(self.orbit(o), self.t, self.tref, self.freq[trials], self.fdot, self.m, self.stat)


def grid2(kind, t0key):
    """The 5 x 5 grid over (TASC | T0, A1): steps that move the pulse by more than a cycle."""
    return {"ell1": {t0key: (5, 1e-3), "A1": (5, 0.004)}, "bt": {t0key: (5, 1.5e-3), "A1": (5, 0.05)}}[kind]


def cases(slice_len, jof):
    """The cases of the truth test; ``jof(m)``: the trial chunk J in force for m harmonics (the plan accessor)."""
    big = 2 * slice_len + 257
    g_ell1, g_bt = grid2("ell1", "TASC"), grid2("bt", "T0")
    g3 = {"T0": (3, 1.5e-3), "A1": (3, 0.05), "PB": (3, 2e-3)}
    return [
        Case("ell1_big_z2m2", "ell1", big, 5 * jof(2) + 3, 2, 0, 0.0, g_ell1, 11),
        Case("bt_e0_big_z2m1_fdot", "bt_e0", big, jof(1) + 1, 1, 0, -3e-11, g_bt, 12),
        Case("bt_e07_big_hm5_pb", "bt_e07", big, 1, 5, 1, 0.0, g3, 13),
        Case("bt_e095_big_hm9_fdot_unsorted", "bt_e095", big, jof(9) + 1, 9, 1, -3e-11, g_bt, 14, sort=False),
        Case("ell1_slice1_hm20", "ell1", slice_len + 1, jof(20) + 1, 20, 1, 0.0, g_ell1, 15),
        Case("ell1_n1_z2m2", "ell1", 1, jof(2) + 1, 2, 0, 0.0, g_ell1, 16),
        Case("ell1_n255_hm5_fdot", "ell1", 255, 5 * jof(5) + 3, 5, 1, -3e-11, g_ell1, 17),
        Case("ell1_n257_z2m1", "ell1", 257, 1, 1, 0, 0.0, g_ell1, 18),
    ]
