"""The unbinned extended likelihood of the three template models (templatemodels.py:64-82, :98-121, :166-185, :201-226,
:271-290, :306-329) at 60 digits, and the unit its fp64 rounding errors scale with.

``points_mp`` restates the eight sums of ``crimp_toa_points`` and ``shape_mp`` the ``CRIMP_SHAPE_SUMS`` sums of
``crimp_toa_shape_points`` in mpmath: the fp64 photons, template values and points are taken exactly, every operation
after that runs at ``mp.dps = 60`` (kappa = 1/wid^2, I0 and I1/I0 from ``mp.besseli`` included). ``ll_mp`` assembles
the reference's extended LL with its -inf rule. Beside every value stands a magnitude A; an fp64 evaluation (the
reference's NumPy, the oracle, a kernel) has to stay within ``FACTOR * U * A`` of the 60-digit value, U = 2**-53.

The unit, by first-order propagation per photon (theta the cosine's argument, v = x - cen - phShift):

* Fourier harmonic j:  e_j = |a_j| (1 + 2 pi j |x| + |ph_j| + j |phShift|  +  j^2).  The first bracket is the size of
  the argument a direct ``cos`` is handed (its roundings enter at their absolute size); j^2 is the Chebyshev
  recurrence c_{j+1} = 2 c_1 c_j - c_{j-1}: dT_j/dc_1 = j U_{j-1} <= j^2 multiplies the error of the first harmonic
  and the recurrence's own roundings add about j^2/2 more. The same unit serves sin; h' carries j e_j, h'' j^2 e_j.
* Cauchy component c = (a/2 pi) sinh w / D, D = cosh w - cos v:  e = |c| (cosh w + 1) / D  -- D is a difference of
  two numbers of size cosh w and 1, each a few roundings wrong.  h' = c sin v / D and h'' = -c (cos v - 2 sin^2 v / D)
  / D carry D's relative unit once per power of D, plus the absolute unit 1 of sin v / cos v.
* von Mises component c = a exp(k cos v) / (2 pi I0(k)):  e = |c| (1 + k (|cos v| + 1))  -- the roundings of k and
  of cos v (absolute size 1) are multiplied by k in the exponent.  h' = k sin v c, h'' = (k^2 sin^2 v - k cos v) c.
* model value m = norm + sum_j c_j:  A_m = |norm| + sum_j e_j.
* every sum S = sum_i t_i:  A_S = sum_i (|t_i| times the relative units of its factors, e.g. |q| (A_m/|m| + 1) for
  q = 1/m, A_m/|m| + |ln m| for ln m)  +  (ceil(N/stride) + 9 + 3) sum_i |t_i|  for the strided per-thread sums
  (stride 512 for crimp_toa_points, 256 for the shape kernel), the wave tree (6 levels) and the cross-wave sum.
* min m:  A_m of the photons that can hold the minimum (m_i within 1e-9 A_m,i of the smallest).

FACTOR = 32, counted, not fitted.  In units of u relative to the component's e:
  - first harmonic / photon sin, cos: the table's rotation ~2 ulp, + 1 for the coefficient's own cos (tpl_coef), so
    3 j^2 through the recurrence, + j^2/2 of its own roundings: 3.5 on the j^2 part; the reference's direct cos: 3
    roundings of the argument (1.5), the cos (1), two products (1): 3.5 on the argument part;
  - Cauchy: cos v is wrong by (|x| + |cen + phShift|) u/2 <~ 6 from the argument roundings, + 2 (table) + 2
    (coefficient sincos) + 1.5 (the rotation's three operations) ~ 11.5 absolute, against e's cosh w + 1 >= 2: 6;
    cosh w at 1 ulp and the subtraction: 1.5; (a/2 pi) sinh w, 1/D, the product: 4.  About 12.
  - von Mises: the same 11.5 on cos v, times k, against e's k: 11.5; k = 1/(w w): 1.5 on k |cos v|; exp at 2 ulp, the
    products 1.5, a/(2 pi I0) 1.5 and scipy's I0 (cephes: peak 5.8e-16 = 5.2 u): about 13, never added to the
    11.5 k at full size.  About 16.
  - sum over K <= 16 components: <= K/2 = 8 on the partial sums (each >= 1 in e).  So m is within 24 A_m at the worst.
  - q = 1/m through lk_rcp (v_rcp_f64 and two Newton steps: the result of a correctly rounded division to 1 ulp):
    1; the products h'q, q q, h'q q, h''q - h'^2 q^2: <= 4; log at 2 ulp; a product of 16 model values before one
    log: <= 15 roundings = 7.5 u on that log, under 0.5 per photon, each photon's A_m/|m| >= 1.
  24 + 4 + 2 + 0.5 < 32.  The summation part of A_S is counted at 1 per addition where u/2 would do.

``load_wide`` reads tests/golden/toa_ll_wide.npz (tests/golden/gen_toa_ll_wide_golden.py), ``ratio`` measures fp64
results against it and ``hi_lo`` splits mp values; none of the three needs mpmath, which is imported only by the *_mp
functions.
"""
import json
import math
import os

import numpy as np

U = 2.0 ** -53
FACTOR = 32.0
DPS = 60
MAX_COMP = 16
SUMS = ("lnm", "q", "h1q", "mq2", "mh1q2", "hess", "min", "N")     # crimp_toa_points' out[p*8 + ...]
SHAPE_SUMS = 4 + 3 * MAX_COMP                                        # lnm, min, q, hphi q, then amp/loc/wid per j
PTS_BLOCK, SHAPE_BLOCK = 512, 256
MODELS = ("fourier", "cauchy", "vonmises")
PH_BOUND = {"fourier": math.pi, "cauchy": 1.5 * math.pi, "vonmises": 1.5 * math.pi}
TINY = 1e-290                # errors below this are fp64 underflow (a von Mises tail at kappa = 625), not rounding
TIE = 1e-9                   # photons within TIE * A_m of the smallest m can hold the fp64 minimum


def _mp():
    import mpmath
    mpmath.mp.dps = DPS
    return mpmath


def _ex(v):
    """An fp64 input taken exactly (an mpf passes through: the generator's Newton iterates)."""
    mp = _mp()
    return v if isinstance(v, mp.mpf) else mp.mpf(float(v))


def tree_terms(n, stride):
    """Additions one photon's term passes through: its thread's strided sum, the 64-lane and the cross-wave trees."""
    return -(-int(n) // stride) + 9 + 3


class _Tpl:
    """A template's exact values: model, K, a_j = amp_j ampShift, loc, wid and the derived constants."""

    def __init__(self, tpl):
        mp = _mp()
        f = mp.mpf
        self.model, self.K = tpl["model"], len(tpl["amp"])
        self.A = f(float(tpl.get("amp_shift", 1.0)))
        self.amp = [f(float(v)) for v in tpl["amp"]]
        self.a = [v * self.A for v in self.amp]
        self.loc = [f(float(v)) for v in tpl["loc"]]
        self.wid = [f(float(v)) for v in tpl.get("wid", [])]
        tp = 2 * mp.pi
        if self.model == "cauchy":
            self.sh = [mp.sinh(w) for w in self.wid]
            self.ch = [mp.cosh(w) for w in self.wid]
            self.pre = [a / tp for a in self.a]
            self.preA = [self.A / tp] * self.K
        elif self.model == "vonmises":
            self.k = [1 / (w * w) for w in self.wid]
            i0 = [mp.besseli(0, k) for k in self.k]
            self.r = [mp.besseli(1, k) / z for k, z in zip(self.k, i0)]
            self.pre = [a / (tp * z) for a, z in zip(self.a, i0)]
            self.preA = [self.A / (tp * z) for z in i0]


def _rot(T, phi):
    """e_j with z^j e_j = exp(i theta_j) (fourier) or exp(i (x - cen_j - phShift))."""
    mp = _mp()
    if T.model == "fourier":
        return [mp.expj(T.loc[j] - (j + 1) * phi) for j in range(T.K)]
    return [mp.expj(-(T.loc[j] + phi)) for j in range(T.K)]


def _photon(T, xf):
    """z^1..z^K (fourier: z = exp(2 pi i x)) or [z] * K (z = exp(i x)), and |x|."""
    mp = _mp()
    x = mp.mpf(float(xf))
    if T.model == "fourier":
        z = mp.expj(2 * mp.pi * x)
        zs, w = [], mp.mpc(1)
        for _ in range(T.K):
            w = w * z
            zs.append(w)
        return zs, abs(x)
    return [mp.expj(x)] * T.K, abs(x)


def _comp(T, j, w, ax, aphi, shape, aux):
    """Component j at one photon and point, w = exp(i theta): (c, e, c', e', c'', e'') and, with ``shape``, the
    template-shape derivatives [(dh/damp, unit), (dh/dloc, unit), (dh/dwid, unit)]."""
    mp = _mp()
    cu, su = w.real, w.imag
    acu, asu = abs(cu), abs(su)
    g = None
    if T.model == "fourier":
        jj = j + 1
        a = T.a[j]
        rel = 1 + 2 * mp.pi * jj * ax + abs(T.loc[j]) + jj * aphi + jj * jj
        e = abs(a) * rel
        out = (a * cu, e, jj * a * su, jj * e, -(jj * jj) * a * cu, jj * jj * e)
        if shape:
            g = [(T.A * cu, abs(T.A) * rel), (-a * su, e), (mp.mpf(0), mp.mpf(0))]
    elif T.model == "cauchy":
        ch, sh, P = T.ch[j], T.sh[j], T.pre[j]
        D = ch - cu
        rD = (ch + 1) / D
        c = P * sh / D
        ac = abs(c)
        pd2 = abs(P * sh) / (D * D)
        out = (c, ac * rD,
               P * sh * su / (D * D), pd2 * (1 + 2 * asu * rD),
               -(P * sh / (D * D)) * (cu - 2 * su * su / D),
               pd2 * (acu * 2 * rD + 1 + (2 * su * su / D) * 3 * rD + 4 * asu / D))
        if shape:
            num = 1 - ch * cu
            g = [(T.preA[j] * sh / D, abs(T.preA[j] * sh / D) * rD),
                 (out[2], out[3]),
                 (P * num / (D * D), abs(P) / (D * D) * ((1 + ch) + abs(num) * 2 * rD))]
    else:
        k, B = T.k[j], T.pre[j]
        ex = mp.exp(k * cu)
        c = B * ex
        ac = abs(c)
        rel = 1 + k * (acu + 1)
        out = (c, ac * rel,
               k * su * c, k * ac * (asu * rel + 1),
               (k * k * su * su - k * cu) * c, ac * ((k * acu + k * k * su * su) * rel + k + 2 * k * k * asu))
        if shape:
            r = T.r[j] if aux else mp.mpf(0)
            w3 = 2 / (T.wid[j] ** 3)
            g = [(T.preA[j] * ex, abs(T.preA[j] * ex) * rel),
                 (out[2], out[3]),
                 (-c * (cu - r) * w3, ac * w3 * (abs(cu - r) * rel + 1 + abs(r)))]
    return out, g


def _model_at(T, zs, ax, rot, norm, aphi, shape=False, aux=True):
    """(m, A_m, h', A', h'', A'', [per component shape terms]) at one photon and point."""
    mp = _mp()
    h = [mp.mpf(0)] * 6
    gs = []
    for j in range(T.K):
        o, g = _comp(T, j, zs[j] * rot[j], ax, aphi, shape, aux)
        h = [a + b for a, b in zip(h, o)]
        gs.append(g)
    return norm + h[0], abs(norm) + h[1], h[2], h[3], h[4], h[5], gs


class _Acc:
    """sum of the terms, of their units and of their sizes."""

    def __init__(self, mp):
        self.v, self.u, self.s = mp.mpf(0), mp.mpf(0), mp.mpf(0)

    def add(self, term, unit, size=None):
        self.v += term
        self.u += unit
        self.s += abs(term) if size is None else size

    def done(self, n, stride):
        return self.v, self.u + tree_terms(n, stride) * self.s


def _min_unit(ms, ams):
    mp = _mp()
    if not ms:
        return mp.inf, mp.mpf(0)
    mn = min(ms)
    return mn, max(a for m, a in zip(ms, ams) if m - mn <= TIE * a)


def points_mp(tpl, x, pts):
    """crimp_toa_points at 60 digits: for every (norm, phShift) of ``pts`` the lists (values[8], A[8]) in SUMS' order.
    sum ln m is nan (A 0) where a model value is not positive."""
    mp = _mp()
    f = mp.mpf
    T = _Tpl(tpl)
    x = np.asarray(x, dtype=np.float64).ravel()
    ph = [_photon(T, v) for v in x]
    res = []
    for norm, phi in pts:
        norm, phi = _ex(norm), _ex(phi)
        rot, aphi = _rot(T, phi), abs(phi)
        acc = [_Acc(mp) for _ in range(6)]
        ms, ams, neg = [], [], False
        for zs, ax in ph:
            m, am, h1, a1, h2, a2, _ = _model_at(T, zs, ax, rot, norm, aphi)
            ms.append(m)
            ams.append(am)
            q = 1 / m
            aq, rm = abs(q), am / abs(m)
            if m > 0:
                lm = mp.log(m)
                acc[0].add(lm, rm + abs(lm))
            else:
                neg = True
            acc[1].add(q, aq * (rm + 1))
            acc[2].add(h1 * q, aq * a1 + abs(h1 * q) * (rm + 1))
            acc[3].add(-q * q, q * q * (2 * rm + 1))
            acc[4].add(-h1 * q * q, q * q * a1 + abs(h1) * q * q * (2 * rm + 1))
            acc[5].add(h2 * q - h1 * h1 * q * q,
                       aq * a2 + abs(h2 * q) * (rm + 1) + 2 * abs(h1) * q * q * a1 + h1 * h1 * q * q * (2 * rm + 1),
                       abs(h2 * q) + h1 * h1 * q * q)
        out = [a.done(x.size, PTS_BLOCK) for a in acc]
        if neg:
            out[0] = (mp.nan, f(0))
        out.append(_min_unit(ms, ams))
        out.append((f(x.size), f(0)))
        res.append(([o[0] for o in out], [o[1] for o in out]))
    return res


def shape_mp(tpl, x, norm, phi, aux=True):
    """crimp_toa_shape_points at 60 digits for one point: (values[SHAPE_SUMS], A[SHAPE_SUMS]); ``aux`` False is the
    call without I1/I0 (the von Mises width term then has 0 in its place)."""
    mp = _mp()
    f = mp.mpf
    T = _Tpl(tpl)
    x = np.asarray(x, dtype=np.float64).ravel()
    norm, phi = _ex(norm), _ex(phi)
    rot, aphi = _rot(T, phi), abs(phi)
    acc = [_Acc(mp) for _ in range(SHAPE_SUMS)]
    ms, ams = [], []
    for v in x:
        zs, ax = _photon(T, v)
        m, am, h1, a1, _, _, gs = _model_at(T, zs, ax, rot, norm, aphi, shape=True, aux=aux)
        ms.append(m)
        ams.append(am)
        q = 1 / m
        aq, rm = abs(q), am / abs(m)
        lm = mp.log(m)
        acc[0].add(lm, rm + abs(lm))
        acc[2].add(q, aq * (rm + 1))
        acc[3].add(h1 * q, aq * a1 + abs(h1 * q) * (rm + 1))
        for j, g in enumerate(gs):
            for c, (val, unit) in enumerate(g):
                acc[4 + 3 * j + c].add(val * q, aq * unit + abs(val * q) * (rm + 1))
    out = [a.done(x.size, SHAPE_BLOCK) for a in acc]
    out[1] = _min_unit(ms, ams)
    return [o[0] for o in out], [o[1] for o in out]


def norm_factor(tpl, norm):
    """fp64 F of the -inf rule min(m / F) <= 0: norm (fourier) or 2 pi norm + sum amp_j ampShift."""
    if tpl["model"] == "fourier":
        return float(norm)
    return 2 * math.pi * float(norm) + sum(float(a) * float(tpl.get("amp_shift", 1.0)) for a in tpl["amp"])


def ll_mp(tpl, n_photons, norm, exposure, lnm, a_lnm, mn):
    """(LL, A) of templatemodels.py:112-121, :215-226, :320-329 from sum ln m, its A and min m; -inf (A 0) where
    min(m / F) <= 0."""
    mp = _mp()
    f = mp.mpf
    T = _Tpl(tpl)
    norm, E, N = _ex(norm), f(float(exposure)), f(int(n_photons))
    if T.model == "fourier":
        F, fmag, rate = norm, abs(norm), norm * E
    else:
        F = 2 * mp.pi * norm + mp.fsum(T.a)
        fmag = 2 * mp.pi * abs(norm) + mp.fsum(abs(a) for a in T.a)
        rate = F * E / (2 * mp.pi)
    if not mn / F > 0:
        return -mp.inf, f(0)
    ll = -rate + N * mp.log(rate) + lnm - N * mp.log(F)
    # the roundings of F ((K/2 + 2) u of fmag, counted as fmag here) move the rate and both logarithms
    a = a_lnm + abs(rate) + N * (abs(mp.log(rate)) + 1) + N * (abs(mp.log(F)) + 1) + \
        fmag * (abs(rate / F) + 2 * N / abs(F))
    return ll, a


# ------------------------------------------------------------------------------------------- packing
LO_BITS, A_BITS = 20, 16     # significant bits the fixture keeps of lo and of A


def chop(x, bits):
    x = np.ascontiguousarray(x, dtype=np.float64)
    return (x.view(np.uint64) & np.uint64(~((1 << (53 - bits)) - 1) & (2 ** 64 - 1))).view(np.float64)


def hi_lo(vals):
    """fp64 hi = the nearest double, lo = mp - hi to 20 bits (nan / inf: lo 0)."""
    mp = _mp()
    vals = list(vals)
    hi = np.array([float(v) for v in vals], dtype=np.float64)
    lo = np.array([float(v - mp.mpf(float(h))) if np.isfinite(h) else 0.0 for v, h in zip(vals, hi)], dtype=np.float64)
    return hi, chop(lo, LO_BITS)


def mag_chopped(mags):
    """A cut towards zero to 16 bits: the stored bound is never wider than the exact one."""
    a = np.array([float(v) for v in mags], dtype=np.float64)
    r = chop(a, A_BITS)
    assert np.all(r <= a) and np.all((r >= a * (1 - 2.0 ** -15)) | (a < TINY))
    return r


def pack(vals, mags, shape=None):
    hi, lo = hi_lo(vals)
    a = mag_chopped(mags)
    if shape is not None:
        hi, lo, a = hi.reshape(shape), lo.reshape(shape), a.reshape(shape)
    return hi, lo, a


def err_ratio(x, hi, lo, a):
    """|x - mp| / (u A) per element; inf where A == 0 and x is not exactly the value; nan values of the fixture
    (sum ln m of a non-positive model) are not compared."""
    x = np.asarray(x, dtype=np.float64)
    skip = np.isnan(hi)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(x == hi, np.abs(lo), np.abs((x - hi) - lo))
        e = np.where(e < TINY, 0.0, e)
        r = np.where(e == 0, 0.0, np.where(a > 0, e / (U * a), np.inf))      # (u A itself may underflow to 0)
    r = np.where(np.isnan(e), np.inf, r)
    return np.where(skip, 0.0, r)


# ------------------------------------------------------------------------------------------- the fixture
class Case:
    """One sums case of toa_ll_wide.npz: template, photons x, exposure E, points pts[P, 2] = (norm, phShift) with
    kind[P] (0 comfortable, 1 min m just positive, 2 model negative at designed photons), the eight sums as
    hi/lo/A[P, 8], the LL as ll_hi/ll_lo/ll_A[P] (-inf where the reference says so; nan with no photon: the
    reference's np.min fails there), the reference's own NumPy LL ll_ref[P], and the shape sums at points
    shape_pts as sh_hi/sh_lo/sh_A[S, SHAPE_SUMS] (von Mises: sh0_* the width rows of the call without aux)."""

    def __init__(self, name, g):
        self.name = name
        self.tpl = json.loads(str(g[name + "_tpl"]))
        self.model = self.tpl["model"]
        for k in ("x", "pts", "kind", "hi", "lo", "A", "ll_hi", "ll_lo", "ll_A", "ll_ref", "shape_pts", "sh_hi",
                  "sh_lo", "sh_A", "sh0_hi", "sh0_lo", "sh0_A"):
            if name + "_" + k in g.files:
                setattr(self, k, g[name + "_" + k].astype(np.float64) if k not in ("kind", "shape_pts")
                        else g[name + "_" + k])
        self.E = float(g[name + "_E"])

    def ratio(self, values, s, pts=slice(None)):
        """max |x - mp| / (u A) of sum ``s`` (a name of SUMS or its index) over the points."""
        c = SUMS.index(s) if isinstance(s, str) else int(s)
        r = err_ratio(values, self.hi[pts, c], self.lo[pts, c], self.A[pts, c])
        return float(np.max(r)) if r.size else 0.0

    def ll_ratio(self, values, pts=slice(None)):
        fin = np.isfinite(self.ll_hi[pts])
        v = np.asarray(values, dtype=np.float64)
        r = err_ratio(v[fin], self.ll_hi[pts][fin], self.ll_lo[pts][fin], self.ll_A[pts][fin])
        return float(np.max(r)) if r.size else 0.0

    def theta(self, p):
        """The reference's theta dict of point p."""
        th = {"norm": float(self.pts[p, 0]), "phShift": float(self.pts[p, 1]),
              "ampShift": float(self.tpl.get("amp_shift", 1.0))}
        loc = "ph" if self.model == "fourier" else "cen"
        for j, a in enumerate(self.tpl["amp"], start=1):
            th["amp_%d" % j] = a
            th["%s_%d" % (loc, j)] = self.tpl["loc"][j - 1]
            if self.model != "fourier":
                th["wid_%d" % j] = self.tpl["wid"][j - 1]
        return th


def ratio(values, case, s):
    return case.ratio(values, s)


class FitCase:
    """One fit case: template dict ``tmpl`` (readPPtemplate's form), photons x, exposure E, the 60-digit optimum
    norm / phi (fp64 roundings of it), LL* as ll_hi + ll_lo, the 2x2 Hessian H at the optimum, A of LL, g_norm, g_phi
    there, and the oracle's 1-sigma bounds and reduced chi2."""

    def __init__(self, name, g):
        self.name = name
        self.tmpl = json.loads(str(g[name + "_tmpl"]))
        self.model = self.tmpl["model"]
        self.K = sum(1 for k in self.tmpl if k.startswith("amp_"))
        self.x = g[name + "_x"]
        v = g[name + "_fit"]
        (self.E, self.norm, self.phi, self.ll_hi, self.ll_lo, self.hnn, self.hnp, self.hpp, self.A_ll, self.A_gn,
         self.A_gp, self.phShi_LL, self.phShi_UL, self.redchi2) = [float(t) for t in v]
        self.H = np.array([[self.hnn, self.hnp], [self.hnp, self.hpp]])


def load_wide(path=None):
    """({name: Case}, {name: FitCase}) of tests/golden/toa_ll_wide.npz, in the file's order."""
    if path is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "toa_ll_wide.npz")
    g = np.load(path, allow_pickle=False)
    index = json.loads(str(g["index"]))
    return ({n: Case(n, g) for n in index["sums"]}, {n: FitCase(n, g) for n in index["fits"]})
