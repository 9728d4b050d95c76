"""The orbital delay of a binary model (BT, ELL1) and the timing-model phase at the emission time, at 60 digits, with
the unit their fp64 rounding errors scale with. The reference project has no binary models: the definition below
 is the contract.

Definition. t is a barycentric arrival time (MJD). tau (s) is the root of tau = D(t - tau / 86400), D(t') the orbital
delay of the emission time t':

    tt0 = (t' - T0|TASC) 86400,  pb = PB 86400,  orbits = tt0 / pb - PBDOT (tt0 / pb)^2 / 2,  x = A1 + A1DOT tt0
    BT:    M = 2 pi frac(orbits),  E - e sin E = M,  w = OM + OMDOT tt0  (deg, deg / yr of 365.25 d),
           D = x sin w (cos E - e) + (x sqrt(1 - e^2) cos w + GAMMA) sin E
    ELL1:  P = 2 pi frac(orbits) from TASC,  D = x (sin P + EPS2 / 2 sin 2P - EPS1 / 2 cos 2P)

PBDOT and A1DOT (XDOT) with a magnitude above 1e-7 are in units of 1e-12. Every part of the phase is evaluated at the
emission time, the delay entering in seconds after the epoch difference:

    Taylor:  dt = (t - PEPOCH) 86400 - tau
    glitch j: ds = (t - GLEP_j) 86400 - tau, counted when ds >= 0; recovery GLF0D GLTD 86400 (1 - exp(-ds / (GLTD 86400)))
    waves:   arg_j = j WAVE_OM ((t - WAVEEPOCH) - tau / 86400)

``delay_mp`` takes the fp64 model values and times exactly and works at ``mp.dps = 60``: Kepler's equation by Newton
to 1e-55, the light-travel equation by the secant method until |tau - D(t - tau / 86400)| < 1e-50 (asserted).

The error unit A(t), derived as tests/phase_reference.py derives its own by counting roundings (u = 2**-53):

* orbital phase. orbits is formed from PB 86400 (1 rounding), (t - T0) 86400 (1, and 1 more when the difference is not
  exact), the subtraction of tau (1) and the division (1); the PBDOT term adds three roundings of a term 1e-9 of the
  first. Each is relative to |orbits|; the reduction orbits - rint(orbits) is exact. An error dM of the mean anomaly
  moves the root by dM / g' and the delay by D'(E) dM / g', g' = 1 - e cos E + (2 pi / pb) D'(E), so the unit is
  2 pi |orbits| |D' / g'|, with at most 6 roundings;
* solve. g = (E - e sin E) - M at the reduced angles: E carries 1 rounding, e sin E 5 (a device sincos within 2 ulp
  is 4 u, the product 1), M 2 (the product by 2 pi and 2 pi itself), the two subtractions 2 more on magnitudes already
  counted; the accepted Newton step leaves < 0.2 u. Unit (|E_r| + e |sin E| + |M_r|) |D' / g'|, at most 8 roundings on
  any term;
* delay. D = x sin w (cos E - e) + (x sqrt(1 - e^2) cos w + GAMMA) sin E: sin w and cos w (4 u each, 3 more for the
  rotation by OMDOT tau), x (2), sqrt(1 - e^2) (2), cos E or sin E (4), the products and sums (4): at most 16 on a
  term. Unit x |sin w| (|cos E| + e) + (x sqrt(1 - e^2) |cos w| + |GAMMA|) |sin E|; ELL1 the same with its three
  terms. The angle w = OM pi / 180 + OMDOT tt0 itself carries 3 roundings at its absolute size (as the wave arguments
  of phase_reference.py do), which move D by |w| |dD / dw| = |w| x (|cos w| (|cos E| + e) + sqrt(1 - e^2) |sin w| |sin E|):
  that is added to the unit;
* the delay's own error re-enters M through t - tau with weight (2 pi / pb) |D' / g'| < 1: it is counted once more in
  the delay's 16.

A_tau is the sum of the three units and every fp64 evaluation of tau has to stay within ``FACTOR_TAU * U * A_tau``
with FACTOR_TAU = 16, the largest count above.

* parts. A part of the phase at the emission time carries its own roundings -- the unit of phase_reference.py at the
  emission time; dt now has one more rounding (the subtraction of tau), so Taylor term n carries 2 n + 3 <= 29 <= 32 --
  plus the delay's error times the part's rate |d part / d t'| (Hz). With one FACTOR = 32 for the parts,
  A_part = A_part(phase_reference, at emission) + (FACTOR_TAU / FACTOR) |rate_part| A_tau.

``load_binary`` reads tests/golden/calcphase_binary.npz (tests/golden/gen_calcphase_binary_golden.py) and needs no
mpmath.
"""
import json
import os

import numpy as np

import phase_reference as R

U = R.U
FACTOR = R.FACTOR          # the parts: 32
FACTOR_TAU = 16.0
ROWS = ("total", "te", "gl", "wv", "tau")     # row order of the fixture's hi / lo arrays
A_ROWS = ("te", "gl", "wv", "tau")            # row order of its A array; A(total) = A(te) + A(gl) + A(wv)
PART_MASK = dict(R.PART_MASK)
MODELS = ("bt_circular", "bt_e01", "bt_e07", "bt_e095", "bt_full", "ell1_amxp", "hmxb_wide", "binary_all",
          "binary_short")
DPS = 60


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def _tiny_units(v):
    v = float(v)
    return v * 1e-12 if abs(v) > 1e-7 else v      # the fp64 product: the value the C-ABI is handed


def orbit_values(tm):
    """The orbit's fp64 numbers as the definition uses them (the 1e-12 convention applied in fp64, as the packing of
    crimp_timing_model does), or None without BINARY."""
    tm = R.plain(tm)
    name = tm.get("BINARY")
    if name in (None, ""):
        return None
    name = str(name).upper()
    assert name in ("BT", "ELL1")
    bt = name == "BT"

    def get(*keys):
        for k in keys:
            if k in tm:
                return float(tm[k])
        return 0.0
    return {"bt": bt, "pb": get("PB"), "pbdot": _tiny_units(get("PBDOT")), "a1": get("A1"),
            "a1dot": _tiny_units(get("A1DOT", "XDOT")), "t0": get("T0") if bt else get("TASC"),
            "ecc": get("ECC", "E") if bt else 0.0, "om": get("OM") if bt else 0.0, "omdot": get("OMDOT") if bt else 0.0,
            "gamma": get("GAMMA") if bt else 0.0, "eps1": 0.0 if bt else get("EPS1"), "eps2": 0.0 if bt else get("EPS2")}


def orbit_keys():
    """Every model key the orbit is read from."""
    return ("BINARY", "PB", "PBDOT", "A1", "A1DOT", "XDOT", "T0", "ECC", "E", "OM", "OMDOT", "GAMMA", "TASC", "EPS1",
            "EPS2")


def contraction(tm):
    """2 pi A1 / (pb (1 - e)): the definition has one root while this is below 1/2."""
    o = orbit_values(tm)
    e = o["ecc"] if o["bt"] else float(np.hypot(o["eps1"], o["eps2"]))
    return 2 * np.pi * o["a1"] / (o["pb"] * 86400.0 * (1 - e))


class _Orbit:
    """D(tt0) and what A needs, in mpmath."""

    def __init__(self, tm):
        mp = _mp()
        f = mp.mpf
        o = orbit_values(tm)
        self.mp, self.bt = mp, o["bt"]
        for k, v in o.items():
            if k != "bt":
                setattr(self, k, f(v))
        self.pbs = self.pb * 86400
        self.deg = mp.pi / 180
        self.omdot_s = self.omdot * self.deg / (f(36525) / 100 * 86400)

    def at(self, tt0, e_start=None):
        """D and the pieces of A at the emission time tt0 (s since T0|TASC)."""
        mp = self.mp
        u = tt0 / self.pbs
        orbits = u - self.pbdot * u * u / 2
        n = mp.nint(orbits)
        m_r = 2 * mp.pi * (orbits - n)
        x = self.a1 + self.a1dot * tt0
        dmdt = (2 * mp.pi / self.pbs) * (1 - self.pbdot * u)
        if self.bt:
            e = self.ecc
            E = mp.mpf(e_start) if e_start is not None else m_r + e * mp.sin(m_r) / mp.sqrt(1 - 2 * e * mp.cos(m_r) + e * e)
            for _ in range(200):
                dE = (E - e * mp.sin(E) - m_r) / (1 - e * mp.cos(E))
                if abs(dE) > 1:          # a Newton step that runs away next to periastron: halve towards M
                    dE = dE / abs(dE) / 2
                E -= dE
                if abs(dE) < mp.mpf(10) ** -55:
                    break
            else:
                raise AssertionError("Kepler's equation did not converge")
            assert abs(E - e * mp.sin(E) - m_r) < mp.mpf(10) ** -55
            s, c = mp.sin(E), mp.cos(E)
            w = self.om * self.deg + self.omdot_s * tt0
            sw, cw = mp.sin(w), mp.cos(w)
            s1 = mp.sqrt(1 - e * e)
            al, be = x * sw, x * s1 * cw + self.gamma
            D = al * (c - e) + be * s
            D1 = be * c - al * s
            mag = abs(al) * (abs(c) + e) + (x * s1 * abs(cw) + abs(self.gamma)) * abs(s) + \
                abs(w) * abs(x) * (abs(cw) * (abs(c) + e) + s1 * abs(sw) * abs(s))
            kep = 1 - e * c
        else:
            E, e = m_r, mp.mpf(0)
            s, c = mp.sin(E), mp.cos(E)
            s2, c2 = mp.sin(2 * E), mp.cos(2 * E)
            D = x * (s + self.eps2 / 2 * s2 - self.eps1 / 2 * c2)
            D1 = x * (c + self.eps2 * c2 + self.eps1 * s2)
            mag = abs(x) * (abs(s) + abs(self.eps2 / 2 * s2) + abs(self.eps1 / 2 * c2))
            kep = mp.mpf(1)
        gp = kep + dmdt * D1
        sens = abs(D1 / gp)
        a_tau = 2 * mp.pi * abs(orbits) * sens + (abs(E) + e * abs(s) + abs(m_r)) * sens + mag
        return D, a_tau, float(E)


def delay_mp(tm, t, starts=None):
    """([tau], [A_tau]) per arrival time; ``starts``: fp64 estimates of tau (the secant method's first point)."""
    mp = _mp()
    f = mp.mpf
    orb = _Orbit(tm)
    tol = f(10) ** -50
    val, mag = [], []
    for i, x in enumerate(np.atleast_1d(np.asarray(t, dtype=np.float64)).ravel()):
        tta = (f(float(x)) - orb.t0) * 86400

        def resid(tau, hint=None):
            D, a, E = orb.at(tta - tau, hint)
            return tau - D, a, E

        t0 = f(float(starts[i])) if starts is not None else f(0)
        r0, a, E = resid(t0)
        t1 = t0 - r0                      # one fixed-point step: tau <- D(t - tau)
        r1, a, E = resid(t1, E)
        for _ in range(100):
            if abs(r1) < tol:
                break
            t2 = t1 - r1 * (t1 - t0) / (r1 - r0) if r1 != r0 else t1 - r1
            t0, r0 = t1, r1
            t1 = t2
            r1, a, E = resid(t1, E)
        assert abs(r1) < tol, ("no root", float(x), float(r1))
        val.append(t1)
        mag.append(a)
    return val, mag


def _taylor(tm, dts):
    mp = _mp()
    f = mp.mpf
    coef = [f(float(tm["F%d" % (n - 1)])) / mp.factorial(n) for n in range(1, 14)]
    val, mag, rate = [], [], []
    for dt in dts:
        terms = [coef[n - 1] * dt ** n for n in range(1, 14)]
        val.append(mp.fsum(terms))
        mag.append(mp.fsum(abs(c) for c in terms))
        rate.append(mp.fsum(n * coef[n - 1] * dt ** (n - 1) for n in range(1, 14)))
    return val, mag, rate


def _glitches(tm, t, taus):
    mp = _mp()
    f = mp.mpf
    rows = [[f(float(tm["GLEP_%d" % j]))] + [f(float(tm.get("%s_%d" % (b, j), 0.0))) for b in R.GLITCH_KEYS]
            for j in range(1, R.n_glitches(tm) + 1)]
    val, mag, rate, edge = [], [], [], []
    for x, tau in zip(t, taus):
        x = f(float(x))
        v, a, r, near = f(0), f(0), f(0), mp.inf
        for glep, glph, glf0, glf1, glf2, glf0d, gltd in rows:
            ds = (x - glep) * 86400 - tau
            near = min(near, abs(ds))
            if not ds >= 0:
                continue
            td = gltd * 86400
            rec = f(0) if gltd == 0 else td * (1 - mp.exp(-ds / td))
            v += glph + glf0 * ds + glf1 * ds ** 2 / 2 + glf2 * ds ** 3 / 6 + glf0d * rec
            a += abs(glph) + abs(glf0 * ds) + abs(glf1 * ds ** 2 / 2) + abs(glf2 * ds ** 3 / 6) + abs(glf0d * td)
            r += glf0 + glf1 * ds + glf2 * ds ** 2 / 2 + (f(0) if gltd == 0 else glf0d * mp.exp(-ds / td))
        val.append(v)
        mag.append(a)
        rate.append(r)
        edge.append(near)
    return val, mag, rate, edge


def _waves(tm, t, taus):
    mp = _mp()
    f = mp.mpf
    nh = R.n_waves(tm)
    if nh == 0:
        z = [f(0)] * len(t)
        return z, z, z
    ep, om, f0 = f(float(tm["WAVEEPOCH"])), f(float(tm["WAVE_OM"])), f(float(tm["F0"]))
    ab = [(f(float(tm["WAVE%d" % j]["A"])), f(float(tm["WAVE%d" % j]["B"]))) for j in range(1, nh + 1)]
    val, mag, rate = [], [], []
    for x, tau in zip(t, taus):
        d = (f(float(x)) - ep) - tau / 86400
        v, a, r = f(0), f(0), f(0)
        for j, (ca, cb) in enumerate(ab, start=1):
            arg = j * om * d
            v += ca * mp.sin(arg) + cb * mp.cos(arg)
            a += (abs(ca) + abs(cb)) * (1 + abs(arg))
            r += (j * om / 86400) * (ca * mp.cos(arg) - cb * mp.sin(arg))
        val.append(v * f0)
        mag.append(a * abs(f0))
        rate.append(r * f0)
    return val, mag, rate


def phase_mp(tm, t, starts=None):
    """{row: ([value], [A])} for ROWS, and the smallest |emission time - GLEP| (s) per time."""
    mp = _mp()
    f = mp.mpf
    tm = R.plain(tm)
    t = np.atleast_1d(np.asarray(t, dtype=np.float64)).ravel()
    tau, a_tau = delay_mp(tm, t, starts)
    pep = f(float(tm["PEPOCH"]))
    te = _taylor(tm, [(f(float(x)) - pep) * 86400 - d for x, d in zip(t, tau)])
    gl = _glitches(tm, t, tau)
    wv = _waves(tm, t, tau)
    w = f(FACTOR_TAU) / f(FACTOR)
    out = {"tau": (tau, a_tau)}
    for name, part in (("te", te), ("gl", gl), ("wv", wv)):
        out[name] = (part[0], [a + w * abs(r) * at for a, r, at in zip(part[1], part[2], a_tau)])
    out["total"] = ([a + b + c for a, b, c in zip(te[0], gl[0], wv[0])],
                    [a + b + c for a, b, c in zip(out["te"][1], out["gl"][1], out["wv"][1])])
    return out, [float(e) for e in gl[3]]


# ------------------------------------------------------------------------------------------- the fixture
class BinaryModel:
    """One model of calcphase_binary.npz: tm, t, and per row of ROWS the 60-digit value as hi + lo and its unit A."""

    def __init__(self, name, tm, t, hi, lo, a4):
        self.name, self.tm, self.t = name, tm, t
        a = a4.astype(np.float64)
        self.hi = dict(zip(ROWS, hi))
        self.lo = dict(zip(ROWS, lo.astype(np.float64)))
        self.A = dict(zip(A_ROWS, a))
        self.A["total"] = a[0] + a[1] + a[2]

    def err(self, x, row="total", sl=slice(None)):
        x = np.asarray(x, dtype=np.float64)
        return np.abs((x - self.hi[row][sl]) - self.lo[row][sl])

    def ratio(self, x, row="total", sl=slice(None)):
        """max over the elements of |x - mp| / (u A); inf where A == 0 and x is not exactly the (zero) value, and for a
        NaN."""
        e, a = self.err(x, row, sl), self.A[row][sl]
        if e.size == 0:
            return 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(a > 0, e / (U * a), np.where(e == 0, 0.0, np.inf))
        r = np.where(np.isnan(e), np.inf, r)
        return float(np.max(r))

    def factor(self, row):
        return FACTOR_TAU if row == "tau" else FACTOR


def load_binary(path=None):
    """{name: BinaryModel} of tests/golden/calcphase_binary.npz, in the file's order."""
    if path is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calcphase_binary.npz")
    g = np.load(path, allow_pickle=False)
    index = json.loads(str(g["index"]))
    return {name: BinaryModel(name, json.loads(str(g[name + "_model"])), g[name + "_t"], g[name + "_hi"],
                              g[name + "_lo"], g[name + "_A"]) for name in index}
