"""The Z^2_m / H periodicity search with its argument carried exactly, and the error unit of every search path.

Truth.  The fp64 inputs -- photon times t, the reference time t0, a trial frequency f, the row's fdot coefficient c2
and the harmonic k -- are taken exactly:

    C_k = sum_i cos 2 pi k (f dt_i + c2 dt_i^2),   S_k likewise with sin,   dt_i = fl(t_i - t0).

dt is the fp64 difference: that is the reference's definition (periodsearch.py:67 subtracts in fp64 before anything
else), exact anyway whenever t and t0 lie within a factor two of each other. For CRIMP_FLAG_TIME_DAYS the times are
fl(t * 86400), the reference's ``TIME_toa*86400`` (measureToAs.py:211), and t0 the fp64 mean of the first and last of
them. c2 is the library's value for a 2-D row, 0.5 * (-1 * pow(10, log10_negfdot)) with the C library's pow
(``c2_of``; search_impl forms it on the host with std::pow, periodsearch.py:95).

The phase in cycles is reduced exactly before any trigonometry (``phase_fraction``): f dt = p + e by Dekker's error-free
product (Veltkamp splitting; NumPy has no fma), r = p - rint(p) exactly, k r = q + qe by a second error-free product,
q - rint(q) exactly; c2 dt^2 the same way through dt^2 = s + se and c2 s = a + ae (c2 se is rounded: 2^-53 of a term
that is itself 2^-53 of c2 dt^2). What is left -- two centred fractions and low words below 1e-9 cycles -- is added
in ``np.longdouble`` (64-bit significand: 2^-65 cycles), cos/sin are the long-double ones and the sums over photons run
in long double. tests/test_search_reference.py holds all of it to 60-digit mpmath sums and to the oracle's double-double
``orc_search_true`` at 1/50 of the smallest unit below. Z^2 and H follow the reference's formula order
(periodsearch.py:67-69, :120-123: the harmonics' (C^2 + S^2) summed then scaled by 2/n for Z^2, scaled then cumulated
and reduced by 4(k-1) for H), in long double, rounded to fp64 at the end. Any subset of trials can be evaluated: the
cost is photons x trials x harmonics.

Units.  Functions of the truth sums A_k = |C_k + i S_k| and of the inputs, never of a path's output; u = 2^-53. Each
path gets a bound d_k on |delta(C_k + i S_k)|, turned into a bound on the cumulative statistic
g_k = sum_{i<=k} Z^2_i by  e_k = (2/n) sum_{i<=k} (2 A_i d_i + d_i^2)  (``cumulative_bound``), and into the
statistic's (``stat_bound``): Z^2_m takes e_m; H = max_k (g_k - 4(k-1)) moves by at most max(e_k*, e_w) over the
harmonics w the errors could lift to the maximum, g_w - 4(w-1) + e_w >= H - e_k* (|max a - max b| <= max|a - b|
restricted to the candidates; k_search_finalize_exact argues the same way).

* fp64 (k_search_f64, k_search_f64_few, k_search_sets; ``fp64_unit``).  Harmonics run in groups starting at k0
  (``group_starts``: 8, 4, 2, 1 harmonics as harm_group cuts them; k_search_sets: groups of 8). ph = fl(f d) is wrong
  by <= u |f d|; ph - rint(ph) is exact; the group's first harmonic uses fl(ph k0) (exact for k0 = 1), wrong by
  another <= u k0 |f d|; harmonic k = k0 + j is the first rotated j times by 2 pi ph. So the phase of harmonic k is
  wrong by <= u (k + [k0 > 1] k0) |f d| cycles, and the term by 2 pi times that (|e^{ia} - e^{ib}| <= |a - b|). 2-D:
  ph = fma(f, d, fl(c2 fl(d d))) errs by u |f d + c2 d^2| + 2 u |c2 d^2| <= u (|f d| + 3 |c2 d^2|), which replaces
  |f d|. sincospi is taken at OpenCL's 4 ulp per component, so a (cos, sin) pair is wrong by < 6 u as a vector; one
  angle addition (c, s) <- (fma(c, c1, -s s1), fma(s, c1, c s1)) multiplies the incoming error by a rotation, adds the
  step pair's own 6 u and two roundings per component (< 3 u as a vector): TRIG0 + TRIG1 j = (6 + 9 j) u after j
  additions. The sums: n terms of size <= 1 added in any order err by <= u n^2 per component (the classical
  (n-1) u sum|x|), sqrt(2) u n^2 as a vector. So
      d_k = 2 pi u (k + [k0 > 1] k0) sum_i (|f d_i| + 3 |c2 d_i^2|) + n (6 + 9 (k - k0)) u + sqrt(2) u n^2.
  The statistic's own arithmetic -- c c + s s (2 u), the m additions, the product by fl(2/n) (2 u) -- adds
  (m + 4) u (sum_k Z^2_k + 4 m). Everything times 1 + 2^-40 for the second-order terms.
* exact kernel, raw (``exact_raw_unit``).  k_search_finalize_exact's bound restated: each term of U.V errs with
  rms <= 1e-9, so C_k and S_k carry sc = sqrt(N) 1e-9, g_k one sigma (4/N) sc sqrt(sum_{i<=k} A_i^2), and the bound is
  kappa = 10 of them plus the bias: lin sqrt(sum A^2) + k quad, lin = kappa 2 (2/N) sc, quad = (2/N) 2 (kappa sc)^2,
  with H's reach rule. The certificate knows nothing of the argument: the kernel forms U's phase from fl(f_a k 4096)
  times d and V's from fl(fl(b delta) k 4096) times d (the products themselves exact, search_exact.h), two roundings
  of the fp64 unit's size, so d_k = 2 pi u 2 k sum_i (|f d_i| + 3 |c2 d_i^2|) is added through ``cumulative_bound``,
  and it evaluates f[j - j % 64] + (j % 64) delta, not f[j]: the grid term 2 pi k |Df_j| sum_i |d_i| (``grid_term``;
  exactly 0 on a dyadic grid). ``sigma`` is the 1 sigma value of Z^2 for the normalised-residual test.
* NUFFT, raw (``nufft_raw_unit``).  DESIGN.md section 5.3: d_k = E(jc) = N (2.4 (x/2)^P / P! + 1e-13), x = pi |jc| / n,
  jc the trial's offset from the row centre j0 + nf // 2, n and P the plan's; plus the grid term for the frequency
  f0 + j delta it evaluates, delta = fl((f[nf-1] - f[0]) / (nf - 1)) as k_ap_final forms it. Its phase is carried as
  TwoProd pairs to ~1e-16 cycles, inside the 1e-13 allowance: no argument term.
* default path, any precision (``default_unit``): rel |P_true| + the fp64 unit, rel = CRIMP_FIXUP_REL's value
  (1e-6): a trial is either certified within rel of its power or recomputed by k_search_f64_few.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LD = np.longdouble
GROW = 1.0 + 2.0 ** -40
TRIG0, TRIG1 = 6.0, 9.0
KAPPA, EXACT_RMS = 10.0, 1e-9
NUFFT_ROUND = 1e-13
FIXUP_REL = 1e-6
assert np.finfo(LD).nmant >= 63, "the truth needs an extended long double"
PI_LD = LD("3.14159265358979323846264338327950288")
_SPLIT = 134217729.0  # 2^27 + 1


def two_prod(a, b):
    """a b = p + e exactly (Dekker), p = fl(a b)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p = a * b
    c = _SPLIT * a
    ah = c - (c - a)
    al = a - ah
    c = _SPLIT * b
    bh = c - (c - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def c2_of(log10_negfdot):
    """The library's fdot coefficient of every 2-D row: 0.5 * (-1 * pow(10, fd)) with the C library's pow."""
    return np.array([0.5 * (-1.0 * math.pow(10.0, float(v))) for v in np.atleast_1d(log10_negfdot)])


def _times_k(x, k):
    """(r, e): k x = r + e (mod 1) exactly, r a centred fp64 fraction, for fp64 x and an integer k."""
    r = x - np.rint(x)
    q, qe = two_prod(r, float(k))
    return q - np.rint(q), qe


class _Pairs:
    """The error-free products of photons [n] x trials [J], shared by the harmonics."""

    def __init__(self, dt, f, c2):
        self.p, self.e = two_prod(f[None, :], dt[:, None])
        self.twod = c2 is not None
        if self.twod:
            s, se = two_prod(dt, dt)
            self.a, self.ae = two_prod(c2[None, :], s[:, None])
            self.b = c2[None, :] * se[:, None]

    def fraction(self, k):
        r, re = _times_k(self.p, k)
        x = LD(k) * self.e.astype(LD) + re.astype(LD)
        if self.twod:
            r2, re2 = _times_k(self.a, k)
            x += LD(k) * (self.ae.astype(LD) + self.b.astype(LD)) + re2.astype(LD)
            x += r2.astype(LD)
        x += r.astype(LD)
        return x - np.rint(x)


def phase_fraction(dt, f, c2, k):
    """Centred fraction of a cycle of k (f dt + c2 dt^2), long double [n, J]; c2 None: the 1-D search."""
    dt, f = np.atleast_1d(np.asarray(dt, np.float64)), np.atleast_1d(np.asarray(f, np.float64))
    return _Pairs(dt, f, None if c2 is None else np.atleast_1d(np.asarray(c2, np.float64))).fraction(k)


def truth_sums(dt, f, c2, m, block=1 << 18):
    """(C, S), long double [m, J]: the harmonic sums of trials (f[j], c2[j]) over photons dt."""
    dt = np.ascontiguousarray(dt, np.float64).reshape(-1)
    f = np.ascontiguousarray(f, np.float64).reshape(-1)
    c2 = None if c2 is None else np.broadcast_to(np.asarray(c2, np.float64), f.shape)
    J = f.size
    C, S = np.zeros((m, J), LD), np.zeros((m, J), LD)
    step = max(1, block // max(dt.size, 1))
    for j0 in range(0, J, step):
        j1 = min(J, j0 + step)
        pr = _Pairs(dt, f[j0:j1], None if c2 is None else c2[j0:j1])
        for k in range(1, m + 1):
            ang = (2 * PI_LD) * pr.fraction(k)
            C[k - 1, j0:j1] = np.cos(ang).sum(axis=0)
            S[k - 1, j0:j1] = np.sin(ang).sum(axis=0)
    return C, S


def cumulative(C, S, n):
    """g[k-1] = sum_{i<=k} Z^2_i, long double [m, J], in H's order (each harmonic scaled by 2/n, then cumulated)."""
    return np.cumsum((C * C + S * S) * (LD(2) / LD(n)), axis=0)


def statistic(C, S, n, stat):
    """Z^2_m (stat 0) or H (stat 1) per trial in the reference's formula order, fp64 [J]."""
    if stat == 0:
        return ((C * C + S * S).sum(axis=0) * (LD(2) / LD(n))).astype(np.float64)
    g = cumulative(C, S, n) - 4 * np.arange(C.shape[0], dtype=LD)[:, None]
    return g.max(axis=0).astype(np.float64)


class Truth:
    """The truth of chosen trials: sums, amplitudes and both statistics' ingredients."""

    def __init__(self, dt, f, c2, m):
        self.dt = np.ascontiguousarray(dt, np.float64).reshape(-1)
        self.f = np.ascontiguousarray(f, np.float64).reshape(-1)
        self.c2 = None if c2 is None else np.ascontiguousarray(np.broadcast_to(c2, self.f.shape), dtype=np.float64)
        self.m, self.n = int(m), self.dt.size
        self.C, self.S = truth_sums(self.dt, self.f, self.c2, self.m)
        self.A = np.sqrt((self.C * self.C + self.S * self.S).astype(np.float64))
        self.g = cumulative(self.C, self.S, self.n).astype(np.float64)
        absd = np.abs(self.dt)
        self.sum_abs_dt = float(absd.sum())
        # sum_i (|f d_i| + 3 |c2 d_i^2|) per trial
        self.argmag = np.abs(self.f) * self.sum_abs_dt
        if self.c2 is not None:
            self.argmag = self.argmag + 3.0 * np.abs(self.c2) * float((absd * absd).sum())

    def power(self, stat):
        return statistic(self.C, self.S, self.n, stat)

    def head(self, m):
        """The same trials with the first m harmonics only."""
        import copy
        T = copy.copy(self)
        T.m, T.C, T.S, T.A, T.g = int(m), self.C[:m], self.S[:m], self.A[:m], self.g[:m]
        return T


def truth_of_sets(t, offsets, freq, m, days=False):
    """One Truth per set of crimp_search_sets: set i = t[offsets[i]:offsets[i+1]] at freq[i], its own t0."""
    out = []
    for i in range(len(offsets) - 1):
        x = np.asarray(t[offsets[i]:offsets[i + 1]], np.float64)
        if days:
            x = x * 86400.0
        t0 = (x[0] + x[-1]) / 2
        out.append(Truth(x - t0, [freq[i]], None, m))
    return out


# ------------------------------------------------------------------------------------------------- units
def group_starts(m, sets=False):
    """k0 of the group every harmonic 1..m runs in: harm_group's 8, 4, 2, 1 (k_search_sets: groups of 8)."""
    out, k0 = [], 1
    while k0 <= m:
        rem = m - k0 + 1
        G = min(rem, 8) if sets else (8 if rem >= 8 else 4 if rem >= 4 else 2 if rem >= 2 else 1)
        out += [k0] * G
        k0 += G
    return np.array(out)


def cumulative_bound(A, d, n):
    """e[k-1] = (2/n) sum_{i<=k} (2 A_i d_i + d_i^2): what errors |dA_i| <= d_i move g_k by."""
    return np.cumsum((2.0 / n) * (2.0 * A * d + d * d), axis=0)


def stat_bound(g, e, stat):
    """The statistic's bound from the cumulative ones (module docstring): e_m for Z^2, the reach rule for H."""
    if stat == 0:
        return e[-1].copy()
    v = g - 4.0 * np.arange(g.shape[0])[:, None]
    ks = np.argmax(v, axis=0)
    cols = np.arange(g.shape[1])
    best, ebest = v[ks, cols], e[ks, cols]
    reach = v + e >= best - ebest
    return np.maximum(ebest, np.where(reach, e, 0.0).max(axis=0))


def fp64_harmonic_bound(T, sets=False):
    """d_k [m, J] of the fp64 kernels."""
    k = np.arange(1, T.m + 1)
    k0 = group_starts(T.m, sets)
    coef = (k + np.where(k0 > 1, k0, 0)).astype(np.float64)
    n = float(T.n)
    const = n * (TRIG0 + TRIG1 * (k - k0)) * U + math.sqrt(2.0) * U * n * n
    return 2.0 * math.pi * U * coef[:, None] * T.argmag[None, :] + const[:, None]


def fp64_unit(T, stat, sets=False):
    e = cumulative_bound(T.A, fp64_harmonic_bound(T, sets), T.n)
    final = (T.m + 4) * U * (T.g[-1] + 4.0 * T.m)
    return (stat_bound(T.g, e, stat) + final) * GROW


def grid_term(T, dfreq):
    """d_k [m, J] of evaluating f[j] - dfreq[j] in place of f[j]: 2 pi k |Df_j| sum_i |dt_i|."""
    k = np.arange(1, T.m + 1, dtype=np.float64)
    return 2.0 * math.pi * k[:, None] * np.abs(np.asarray(dfreq, np.float64))[None, :] * T.sum_abs_dt


def progression_step(f):
    """delta of the grid as k_ap_final forms it: fl(fl(f[nf-1] - f[0]) / (nf - 1))."""
    f = np.asarray(f, np.float64)
    return float((f[-1] - f[0]) / float(f.size - 1))


def nufft_grid_deviation(f, idx):
    """f[j] - (f[0] + j delta) exactly (Fraction), rounded once, for the row's trials idx."""
    d, f0 = Fraction(progression_step(f)), Fraction(float(f[0]))
    return np.array([float(Fraction(float(f[j])) - (f0 + int(j) * d)) for j in idx])


def exact_grid_deviation(f, idx):
    """f[j] - (f[j - j % 64] + (j % 64) delta) exactly: the frequency the exact kernel's U_a V_b evaluates."""
    d = Fraction(progression_step(f))
    return np.array([float(Fraction(float(f[j])) - (Fraction(float(f[j - j % 64])) + int(j % 64) * d)) for j in idx])


def exact_raw_unit(T, stat, dfreq=None):
    """(unit, sigma): the exact kernel's raw bound on the truth sums and the 1 sigma value of Z^2_m."""
    n = float(T.n)
    sc = math.sqrt(n) * EXACT_RMS
    w = 2.0 / n
    lin, quad = KAPPA * 2.0 * w * sc, w * 2.0 * (KAPPA * sc) ** 2
    raw = np.cumsum(T.A * T.A, axis=0)
    k = np.arange(1, T.m + 1, dtype=np.float64)
    d = 2.0 * math.pi * U * 2.0 * k[:, None] * T.argmag[None, :]
    if dfreq is not None:
        d = d + grid_term(T, dfreq)
    e = lin * np.sqrt(raw) + k[:, None] * quad + cumulative_bound(T.A, d, T.n)
    sigma = 2.0 * w * sc * np.sqrt(raw[-1])
    return stat_bound(T.g, e, stat) * GROW, sigma


def nufft_E(n_photons, jc, nfft, P):
    x = math.pi * np.abs(np.asarray(jc, np.float64)) / float(nfft)
    return n_photons * (2.4 * (x / 2.0) ** P / math.factorial(P) + NUFFT_ROUND)


def nufft_plan_rule(nseg, stat, m, gather=True):
    """(FFT length, moments) of nu_plan for a row of nseg trials, restated from DESIGN.md section 5.3: among the powers
    of two n >= max(nseg, 64) (up to 2^24) whose edge bound 2.4 (x/2)^P / P! is <= 5e-14 (5e-13 for Z^2_m, m >= 2)
    within the spread's moments (24 for the cell gather, 16 for the MFMA slots), the least n P; the smaller n on a tie,
    no n beyond the first that needs <= 4 moments."""
    eps, pmax = (5e-13 if stat == 0 and m >= 2 else 5e-14), (24 if gather else 16)
    edge = max(nseg // 2, nseg - 1 - nseg // 2)
    best = None
    for l in range(max(int(nseg - 1).bit_length(), 6), 25):
        x = math.pi * edge / 2.0 ** l
        p = next((q for q in range(1, pmax + 1) if 2.4 * (x / 2.0) ** q / math.factorial(q) <= eps), None)
        if p is None:
            continue
        if best is None or (p << l) < (best[1] << best[0]):
            best = (l, p)
        if p <= 4:
            break
    return 1 << best[0], best[1]


def nufft_raw_unit(T, stat, jc, nfft, P, dfreq=None):
    d = np.broadcast_to(nufft_E(float(T.n), jc, nfft, P)[None, :], T.A.shape)
    if dfreq is not None:
        d = d + grid_term(T, dfreq)
    return stat_bound(T.g, cumulative_bound(T.A, d, T.n), stat) * GROW


def default_unit(T, stat, rel=FIXUP_REL, sets=False):
    return rel * np.abs(T.power(stat)) + fp64_unit(T, stat, sets)


# ------------------------------------------------------------------------------------------------- helpers
def checked_trials(nf, edges=(), nrandom=64, seed=0, rows=1):
    """The stated subset of a row of nf trials (every row of ``rows``): both edges, the centre nf // 2 and +-1, each
    named tile or block edge and its two neighbours, and nrandom random trials; flat fd-outer indices, sorted."""
    rng = np.random.default_rng(seed)
    pick = {0, nf - 1, nf // 2 - 1, nf // 2, nf // 2 + 1}
    for e in edges:
        pick |= {e - 1, e, e + 1}
    pick |= set(int(v) for v in rng.integers(0, nf, nrandom))
    row = np.array(sorted(j for j in pick if 0 <= j < nf), dtype=np.int64)
    return np.concatenate([r * nf + row for r in range(rows)])


def fp64_model(dt, f, c2, m, sets=False):
    """(C, S) fp64 [m, J] of a NumPy restatement of the fp64 kernels' arithmetic: ph = fl(f d) (2-D: the fma of f d
    and fl(c2 fl(d d)), formed from the error-free product and rounded once), the group's first harmonic from
    fl(ph k0), sincospi as the correctly rounded long-double value, angle additions with emulated fmas, fp64 sums."""
    dt = np.asarray(dt, np.float64).reshape(-1)
    f = np.asarray(f, np.float64).reshape(-1)
    d = dt[:, None]
    if c2 is None:
        ph = f[None, :] * d
    else:
        p, e = two_prod(f[None, :], d)
        w = np.asarray(c2, np.float64).reshape(-1)[None, :] * (d * d)
        ph = ((p.astype(LD) + w.astype(LD)) + e.astype(LD)).astype(np.float64)

    def sincospi2(x):
        a = (2 * PI_LD) * (x - np.rint(x)).astype(LD)
        return np.sin(a).astype(np.float64), np.cos(a).astype(np.float64)

    def fma(a, b, c):
        p, e = two_prod(a, b)
        return ((p.astype(LD) + c.astype(LD)) + e.astype(LD)).astype(np.float64)

    s1, c1 = sincospi2(ph)
    C, S = np.zeros((m, f.size)), np.zeros((m, f.size))
    k0s = group_starts(m, sets)
    for k in range(1, m + 1):
        if k0s[k - 1] == k:
            s, c = (s1, c1) if k == 1 else sincospi2(ph * float(k))
        else:
            c, s = fma(c, c1, -(s * s1)), fma(s, c1, c * s1)
        C[k - 1], S[k - 1] = c.sum(axis=0), s.sum(axis=0)
    return C, S


def power_fp64(C, S, n, stat):
    """k_search_finalize's arithmetic in fp64."""
    z = C * C + S * S
    w = 2.0 / n
    if stat == 0:
        return z.sum(axis=0) * w
    return (np.cumsum(z * w, axis=0) - 4.0 * np.arange(C.shape[0])[:, None]).max(axis=0)
