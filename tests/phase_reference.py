"""The timing-model phase (calcphase.py:73-176) at 60 digits, and the unit its fp64 rounding errors scale with.

``taylor_mp`` / ``glitches_mp`` / ``waves_mp`` restate the three parts in mpmath: the fp64 model values and times are
taken exactly, every operation after that runs at ``mp.dps = 60``. Beside each value they return the magnitude A(t)
that the rounding errors of an fp64 evaluation are proportional to (u = 2**-53):

* Taylor:  sum_n |F_{n-1}/n! dt^n|;
* glitch j (t >= GLEP_j):  |GLPH| + |GLF0 ds| + |GLF1 ds^2/2| + |GLF2 ds^3/6| + |GLF0D GLTD 86400| -- the recovery term
  at its size before the 1 - exp cancellation, whose lost digits every fp64 form of the formula loses;
* waves:  |F0| sum_j (|A_j| + |B_j|) (1 + |arg_j|) -- the three roundings of the argument enter the sine at their
  absolute size.

Every fp64 evaluation (the reference's NumPy, the oracle, the kernel) has to stay within ``FACTOR * U * A(t)`` of the
60-digit value. The factor is derived, not fitted: Taylor term n carries at most n + 3 roundings (16 for n <= 13), the
13-term sum adds at most 13 u of its partial sums, glitch and wave terms carry fewer, the device sin / cos / exp are
within 2 ulp, the final additions cost 2 more.

``load_wide`` reads tests/golden/calcphase_wide.npz (tests/golden/gen_calcphase_wide_golden.py) and ``ratio`` measures
an fp64 result against it; neither needs mpmath, which is imported only by the *_mp functions.
"""
import json
import os

import numpy as np

U = 2.0 ** -53
FACTOR = 32.0
PARTS = ("total", "te", "gl", "wv")          # row order of the fixture's stacked arrays
PART_MASK = {"total": 7, "te": 1, "gl": 2, "wv": 4}
GLITCH_KEYS = ("GLPH", "GLF0", "GLF1", "GLF2", "GLF0D", "GLTD")
DPS = 60


def plain(tm):
    """The model with {value, flag} entries replaced by their value (readtimingmodel.py:309-321)."""
    return {k: (v["value"] if isinstance(v, dict) and "value" in v and "flag" in v else v) for k, v in tm.items()}


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def n_glitches(tm):
    return sum(1 for k in tm if k.startswith("GLEP_"))          # calcphase.py:94


def n_waves(tm):
    nw = sum(1 for k in tm if k.startswith("WAVE"))             # calcphase.py:135, :142
    return max(nw - 2, 0) if nw else 0


def taylor_mp(tm, t):
    """([value], [A]) of calcphase.py:80-85 per time."""
    mp = _mp()
    f = mp.mpf
    pep = f(float(tm["PEPOCH"]))
    coef = [f(float(tm["F%d" % (n - 1)])) / mp.factorial(n) for n in range(1, 14)]
    val, mag = [], []
    for x in t:
        dt = (f(float(x)) - pep) * 86400
        terms = [coef[n - 1] * dt ** n for n in range(1, 14)]
        val.append(mp.fsum(terms))
        mag.append(mp.fsum(abs(c) for c in terms))
    return val, mag


def glitches_mp(tm, t, only=None):
    """([value], [A]) of calcphase.py:94-126 per time; ``only`` restricts the sum to those glitch numbers."""
    mp = _mp()
    f = mp.mpf
    rows = []
    for j in range(1, n_glitches(tm) + 1):
        if only is not None and j not in only:
            continue
        rows.append([f(float(tm["GLEP_%d" % j]))] + [f(float(tm.get("%s_%d" % (b, j), 0.0))) for b in GLITCH_KEYS])
    val, mag = [], []
    for x in t:
        x = f(float(x))
        v, a = f(0), f(0)
        for glep, glph, glf0, glf1, glf2, glf0d, gltd in rows:
            if not x >= glep:
                continue
            ds = (x - glep) * 86400
            rec = f(0) if gltd == 0 else (gltd * 86400) * (1 - mp.exp(-(x - glep) / gltd))
            v += glph + glf0 * ds + glf1 * ds ** 2 / 2 + glf2 * ds ** 3 / 6 + glf0d * rec
            a += abs(glph) + abs(glf0 * ds) + abs(glf1 * ds ** 2 / 2) + abs(glf2 * ds ** 3 / 6) + \
                abs(glf0d * gltd * 86400)
        val.append(v)
        mag.append(a)
    return val, mag


def waves_mp(tm, t, only=None):
    """([value], [A]) of calcphase.py:135-149 per time (zeros with no harmonic); ``only`` restricts the sum to those
    harmonic numbers."""
    mp = _mp()
    f = mp.mpf
    nh = n_waves(tm)
    if nh == 0:
        return [f(0)] * len(t), [f(0)] * len(t)
    ep, om, f0 = f(float(tm["WAVEEPOCH"])), f(float(tm["WAVE_OM"])), f(float(tm["F0"]))
    ab = [(f(float(tm["WAVE%d" % j]["A"])), f(float(tm["WAVE%d" % j]["B"]))) for j in range(1, nh + 1)]
    val, mag = [], []
    for x in t:
        d = f(float(x)) - ep
        v, a = f(0), f(0)
        for j, (ca, cb) in enumerate(ab, start=1):
            if only is not None and j not in only:
                continue
            arg = j * om * d
            v += ca * mp.sin(arg) + cb * mp.cos(arg)
            a += (abs(ca) + abs(cb)) * (1 + abs(arg))
        val.append(v * f0)
        mag.append(a * abs(f0))
    return val, mag


def phase_mp(tm, t):
    """{part: ([value], [A])} for PARTS; the total is the sum of the three parts, its A the sum of theirs."""
    tm = plain(tm)
    t = np.atleast_1d(np.asarray(t, dtype=np.float64)).ravel()
    te, gl, wv = taylor_mp(tm, t), glitches_mp(tm, t), waves_mp(tm, t)
    tot = ([a + b + c for a, b, c in zip(te[0], gl[0], wv[0])], [a + b + c for a, b, c in zip(te[1], gl[1], wv[1])])
    return {"total": tot, "te": te, "gl": gl, "wv": wv}


LO_BITS, A_BITS = 20, 16     # significant bits the fixture keeps of lo and of A (fp64 exponent range for both)


def chop(x, bits):
    """fp64 values cut towards zero to ``bits`` significant bits (the cleared low bits are what lets the fixture
    compress); the exponent range stays fp64's, so a phase of 1e-170 cycles next to an epoch keeps its lo and its A."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    return (x.view(np.uint64) & np.uint64(~((1 << (53 - bits)) - 1) & (2 ** 64 - 1))).view(np.float64)


def hi_lo(vals):
    """fp64 hi = the nearest double, lo = mp - hi to 20 bits: hi + lo carries the 60-digit value to 2**-72 of itself,
    orders below the smallest error the bound has to resolve."""
    mp = _mp()
    hi = np.array([float(v) for v in vals], dtype=np.float64)
    lo = np.array([float(v - mp.mpf(float(h))) for v, h in zip(vals, hi)], dtype=np.float64)
    return hi, chop(lo, LO_BITS)


def mag_chopped(mags):
    """A(t) cut towards zero to 16 bits: the stored bound is never wider than the exact one (and at most 2**-15 of
    itself narrower)."""
    a = np.array([float(v) for v in mags], dtype=np.float64)
    r = chop(a, A_BITS)
    assert np.all(r <= a) and np.all(r >= a * (1 - 2.0 ** -15))
    return r


# ------------------------------------------------------------------------------------------- the fixture
class WideModel:
    """One model of calcphase_wide.npz: tm (dict), t, and per part the 60-digit value as hi + lo, its error unit A and
    the reference's own fp64 result."""

    def __init__(self, name, tm, t, hi, lo, a3, refd):
        self.name, self.tm, self.t = name, tm, t
        a = a3.astype(np.float64)
        amag = np.vstack([a[0] + a[1] + a[2], a])    # A(total) = A(te) + A(gl) + A(wv)
        self.hi = dict(zip(PARTS, hi))
        self.lo = dict(zip(PARTS, lo.astype(np.float64)))
        self.A = dict(zip(PARTS, amag))
        self.ref = dict(zip(PARTS, hi + refd))       # stored as the (exact) difference from hi

    def err(self, x, part="total", sl=slice(None)):
        """|x - mp| per element."""
        x = np.asarray(x, dtype=np.float64)
        return np.abs((x - self.hi[part][sl]) - self.lo[part][sl])

    def ratio(self, x, part="total", sl=slice(None)):
        """max over the elements of |x - mp| / (u A); inf where A == 0 and x is not exactly the (zero) value."""
        e, a = self.err(x, part, sl), self.A[part][sl]
        if e.size == 0:
            return 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(a > 0, e / (U * a), np.where(e == 0, 0.0, np.inf))
        r = np.where(np.isnan(e), np.inf, r)
        return float(np.max(r))


def load_wide(path=None):
    """{name: WideModel} of tests/golden/calcphase_wide.npz, in the file's order."""
    if path is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "calcphase_wide.npz")
    g = np.load(path, allow_pickle=False)
    index = json.loads(str(g["index"]))
    # index: name -> [key of its times, name whose arrays it shares] (the {value, flag} copy of a model has the
    # arrays of the plain one: the generator asserts the reference returns the same bits for both)
    return {name: WideModel(name, json.loads(str(g[name + "_model"])), g[tkey], g[data + "_hi"], g[data + "_lo"],
                            g[data + "_A"], g[data + "_refd"]) for name, (tkey, data) in index.items()}
