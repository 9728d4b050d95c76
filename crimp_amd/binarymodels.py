"""Binary orbits (BT, ELL1) of a timing model: the orbital delay and emission times. Not in the reference, whose
documentation lists binary motion as missing; the definition is DESIGN.md section 2.

Event times are barycentric arrival times t (MJD). The delay tau (s) is the root of tau = D(t - tau / 86400), D the
orbital delay of the emission time t':

    tt0 = (t' - T0|TASC) 86400,  pb = PB 86400,  orbits = tt0 / pb - PBDOT (tt0 / pb)^2 / 2,  x = A1 + A1DOT tt0
    BT:    M = 2 pi frac(orbits),  E - e sin E = M,  w = OM + OMDOT tt0  (deg, deg / yr of 365.25 d),
           D = x sin w (cos E - e) + (x sqrt(1 - e^2) cos w + GAMMA) sin E
    ELL1:  P = 2 pi frac(orbits) from TASC,  D = x (sin P + EPS2 / 2 sin 2P - EPS1 / 2 cos 2P)

``binary_delay`` and ``emission_times`` run on the GPU (crimp_binary_delay); ``binary_delay_host`` is the same
iteration in NumPy fp64 -- the scalar host paths (ephemIntegerRotation, the .tim writer) use it, and it checks the
definition where there is no GPU.
"""
import numpy as np

from . import _native as N
from .readtimingmodel import BINARY_MODELS, ReadTimingModel, get_parameter_value

KINDS = {"BT": N.BINARY_BT, "ELL1": N.BINARY_ELL1}
MAX_ITER = 32                      # kBinMaxIter of csrc/binary_delay.h
TOL = 2.0 ** -31                   # kBinTol
_TWO_PI = 6.283185307179586476925
_DEG = 3.141592653589793 / 180.0
_YEAR_S = 365.25 * 86400.0


def _plain(timMod):
    if isinstance(timMod, dict):
        return {k: get_parameter_value(v) for k, v in timMod.items()}
    return ReadTimingModel(str(timMod)).readfulltimingmodel()[0]


def has_binary(timMod):
    """The model (a dict, plain or {value, flag}) has a BINARY entry."""
    return isinstance(timMod, dict) and get_parameter_value(timMod.get("BINARY")) not in (None, "")


def _tiny_units(v):
    """PBDOT and A1DOT as Tempo2 and PINT read them: a magnitude above 1e-7 is in units of 1e-12."""
    v = float(v)
    return v * 1e-12 if abs(v) > 1e-7 else v


def binary_params(timMod):
    """The orbit of a model as the numbers crimp_timing_model's binary block holds (None without BINARY): kind, pb
    (days), pbdot and a1dot (dimensionless), a1, t0 (T0 or TASC), ecc, om, omdot, gamma, eps1, eps2. ValueError for a
    model outside the limits: another BINARY name, PB <= 0, A1 < 0, ECC outside [0, 1) (ELL1: EPS1^2 + EPS2^2 >= 1),
    2 pi A1 / (pb (1 - e)) >= 1/2 -- beyond it the light-travel equation need not have a single root."""
    d = _plain(timMod)
    name = d.get("BINARY")
    if name in (None, ""):
        return None
    name = str(name).upper()
    if name not in BINARY_MODELS:
        raise ValueError("BINARY %s is not supported: the supported binary models are BT and ELL1" % name)
    bt = name == "BT"

    def get(key, *aliases):
        for k in (key,) + aliases:
            if k in d:
                return float(d[k])
        return 0.0

    p = {"kind": KINDS[name], "pb": get("PB"), "pbdot": _tiny_units(get("PBDOT")), "a1": get("A1"),
         "a1dot": _tiny_units(get("A1DOT", "XDOT")), "t0": get("T0") if bt else get("TASC"),
         "ecc": get("ECC", "E") if bt else 0.0, "om": get("OM") if bt else 0.0, "omdot": get("OMDOT") if bt else 0.0,
         "gamma": get("GAMMA") if bt else 0.0, "eps1": 0.0 if bt else get("EPS1"), "eps2": 0.0 if bt else get("EPS2")}
    if not all(np.isfinite(v) for v in p.values()):
        raise ValueError("a binary parameter is not finite")
    if not p["pb"] > 0:
        raise ValueError("PB must be positive")
    if not p["a1"] >= 0:
        raise ValueError("A1 must be >= 0")
    e = p["ecc"]
    if bt and not 0 <= e < 1:
        raise ValueError("ECC must be in [0, 1)")
    if not bt:
        e = float(np.hypot(p["eps1"], p["eps2"]))
        if not e < 1:
            raise ValueError("EPS1^2 + EPS2^2 must be below 1")
    if not 2.0 * 3.141592653589793 * p["a1"] / (p["pb"] * 86400.0 * (1.0 - e)) < 0.5:
        raise ValueError("2 pi A1 / (PB (1 - e)) must be below 1/2")
    return p


def fill_native(m, timMod):
    """Write the binary block of the crimp_timing_model ``m``; a model without BINARY leaves the zero tail."""
    p = binary_params(timMod)
    if p is None:
        return m
    m.binary = p["kind"]
    for k in ("pb", "pbdot", "a1dot", "a1", "t0", "ecc", "om", "omdot", "gamma", "eps1", "eps2"):
        setattr(m, "bin_" + k, p[k])
    return m


def require_no_binary(timMod):
    """The timing fits do not model the orbit."""
    if has_binary(timMod):
        raise ValueError("binary models are not fitted yet")


# ------------------------------------------------------------------------------------------- host evaluation
def _orbit(p, bt, tt, tau, sw, cw, s, c):
    """D, D', D'' of csrc/binary_delay.h: bin_orbit."""
    x = p["a1"] + p["a1dot"] * tt
    if bt:
        d = p["omdot_rad_s"] * tau
        d2 = d * d
        sd, cd = d * (1.0 - d2 * (1.0 / 6.0)), 1.0 - 0.5 * d2 * (1.0 - d2 * (1.0 / 12.0))
        so, co = sw * cd - cw * sd, cw * cd + sw * sd
        al, be = x * so, (x * p["s1me2"]) * co + p["gamma"]
        return al * (c - p["ecc"]) + be * s, be * c - al * s, -(al * c + be * s)
    s2, c2 = 2.0 * s * c, (c - s) * (c + s)
    h1, h2 = 0.5 * p["eps1"], 0.5 * p["eps2"]
    return (x * ((s + h2 * s2) - h1 * c2), x * ((c + p["eps2"] * c2) + p["eps1"] * s2),
            -x * ((s + (4.0 * h2) * s2) - (4.0 * h1) * c2))


def binary_delay_host(timeMJD, timMod, return_iterations=False):
    """tau (s) per arrival time (MJD) in NumPy fp64: the iteration of the device function bin_delay, step for step --
    the same starter, bracket, Newton-or-midpoint step, stopping rule and cap (NaN at the cap and for a NaN time).
    A model without BINARY gives zeros. ``return_iterations``: also the iterations each time took."""
    t = np.atleast_1d(np.asarray(timeMJD, dtype=np.float64))
    shape = t.shape
    t = t.reshape(-1)
    p = binary_params(timMod)
    if p is None:
        z = np.zeros(shape)
        return (z, np.zeros(shape, dtype=np.int64)) if return_iterations else z
    p = dict(p)
    bt = p["kind"] == N.BINARY_BT
    e = p["ecc"]
    pb = p["pb"] * 86400.0
    p["s1me2"] = float(np.sqrt((1.0 - e) * (1.0 + e)))
    p["omdot_rad_s"] = p["omdot"] * _DEG / _YEAR_S
    amp = 1.0 + e if bt else 1.0 + 0.5 * (abs(p["eps1"]) + abs(p["eps2"]))
    with np.errstate(invalid="ignore", over="ignore"):
        tta = (t - p["t0"]) * 86400.0
        ua = tta / pb
        oa = ua - (0.5 * p["pbdot"]) * (ua * ua)
        n = np.rint(oa)
        Ma = _TWO_PI * (oa - n)
        w = p["om"] * _DEG + p["omdot_rad_s"] * tta
        sw, cw = (np.sin(w), np.cos(w)) if bt else (np.zeros_like(t), np.ones_like(t))
        s, c = np.sin(Ma), np.cos(Ma)
        E = Ma + e * s / np.sqrt((1.0 - 2.0 * e * c) + e * e)
        span = e + 1.0001 * (_TWO_PI / pb) * (np.abs(p["a1"] + p["a1dot"] * tta) * amp + abs(p["gamma"])) + 1e-12
        lo, hi = Ma - span, Ma + span
        tau = np.zeros_like(t)
        res = np.full_like(t, np.nan)
        its = np.full(t.shape, MAX_ITER, dtype=np.int64)
        live = np.ones(t.shape, dtype=bool)
        for it in range(MAX_ITER):
            if not live.any():
                break
            s, c = np.sin(E), np.cos(E)
            D, D1, D2 = _orbit(p, bt, tta - tau, tau, sw, cw, s, c)
            u = (tta - D) / pb
            M = _TWO_PI * ((u - (0.5 * p["pbdot"]) * (u * u)) - n)
            g = (E - e * s) - M
            gp = (1.0 - e * c) + (_TWO_PI / pb) * (1.0 - p["pbdot"] * u) * D1
            pos = g > 0.0
            hi = np.where(live & pos, E, hi)
            lo = np.where(live & ~pos, E, lo)
            dE = -g / gp
            newton = (E + dE >= lo) & (E + dE <= hi)
            dE = np.where(newton, dE, 0.5 * (lo + hi) - E)
            En = E + dE
            done = live & ~(np.abs(dE) > TOL) & (newton | ~(hi - lo > 1e-15 * (1.0 + np.abs(En))))
            tau1 = D + dE * (D1 + 0.5 * dE * D2)
            Df, D1f, D2f = _orbit(p, bt, tta - tau1, tau1, sw, cw, s, c)
            res = np.where(done, Df + dE * (D1f + 0.5 * dE * D2f), res)
            its = np.where(done, it + 1, its)
            tau = np.where(live, D, tau)
            E = np.where(live, En, E)
            live &= ~done
    res = res.reshape(shape)
    return (res, its.reshape(shape)) if return_iterations else res


# ------------------------------------------------------------------------------------------- device
def _device_delay(time, timMod, want_emit):
    from . import ops
    flat = time.reshape(-1) if N._is_torch(time) else np.atleast_1d(np.asarray(time, dtype=np.float64)).reshape(-1)
    return ops.binary_delay(flat, _plain(timMod), want_emit=want_emit)


def binary_delay(timeMJD, timMod):
    """The orbital delay tau (s) of every arrival time (MJD; a NumPy array or a torch CUDA tensor, whose result stays
    on the device), in the input's shape. ValueError for a model without BINARY or outside the limits."""
    if binary_params(timMod) is None:
        raise ValueError("the timing model has no BINARY")
    shape = tuple(timeMJD.shape) if N._is_torch(timeMJD) else np.shape(timeMJD)
    tau, _ = _device_delay(timeMJD, timMod, False)
    return float(tau[0]) if shape == () else tau.reshape(shape)


def emission_times(time, timMod, unit="mjd"):
    """Emission times of the arrival times ``time`` (MJD): with ``unit="mjd"`` the MJD t - tau / 86400 (rounded to a
    double once: good to 0.3 us), with ``unit="s"`` the seconds (t - PEPOCH) 86400 - tau since PEPOCH, which keep the
    delay's precision -- the array to hand to PeriodSearch to search a pulsar in a known orbit. A model without
    BINARY gives the arrival times themselves in that unit."""
    if unit not in ("mjd", "s"):
        raise ValueError("unit must be 'mjd' or 's'")
    d = _plain(timMod)
    shape = tuple(time.shape) if N._is_torch(time) else np.shape(time)
    if binary_params(d) is None:
        tt = time if N._is_torch(time) else np.asarray(time, dtype=np.float64)
        return tt if unit == "mjd" else (tt - float(d["PEPOCH"])) * 86400.0
    tau, emit = _device_delay(time, d, unit == "mjd")
    if unit == "mjd":
        out = emit
    else:
        flat = time.reshape(-1) if N._is_torch(time) else np.atleast_1d(np.asarray(time, dtype=np.float64)).reshape(-1)
        out = (flat - float(d["PEPOCH"])) * 86400.0 - tau
    return float(out[0]) if shape == () else out.reshape(shape)
