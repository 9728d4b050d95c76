"""CPU checks of tests/search_reference.py, before any kernel is judged by it: the truth against 60-digit mpmath sums and
against the oracle's double-double ``orc_search_true`` (an independent implementation, pinned here for the first time),
both at 1/50 of the smallest unit the truth adjudicates; NumPy restatements of the fp64 kernels' arithmetic inside the
fp64 unit at every shape tests/test_gpu_search_truth.py uses; the reference's own NumPy formula told apart from the
truth; and the input conditions of the GPU cases (a clear best trial where an argmax is asserted, |P| > 0 everywhere,
the H_20 cancellation), so that the GPU tests cannot hide a failure behind their inputs."""
import math

import numpy as np
import pytest

import search_reference as R
import test_gpu_search_truth as G
from oracle import oracle as O

F0 = G.F0


def photons(n, span, seed, frac=0.3):
    from crimp_amd.synth import pulsed_events
    t = pulsed_events(n, span, F0, pulsed_frac=frac, seed=seed)
    return t, (t[0] + t[-1]) / 2


def smallest_unit(T, stat):
    """The smallest unit any path can be held to at these trials: the fp64 unit, the exact kernel's raw bound, the
    NUFFT's at the row centre (E = N 1e-13, no truncation term)."""
    nu = R.nufft_raw_unit(T, stat, np.zeros(T.f.size), 64, 13)
    return np.minimum(np.minimum(R.fp64_unit(T, stat), R.exact_raw_unit(T, stat)[0]), nu)


def mp_sums(dt, f, c2, m):
    """C, S [m, J] at 60 digits: every fp64 input exact, the phase reduced exactly (mp.frac of an exact product)."""
    import mpmath as mp
    mp.mp.dps = 60
    C = [[mp.mpf(0)] * len(f) for _ in range(m)]
    S = [[mp.mpf(0)] * len(f) for _ in range(m)]
    for j, fj in enumerate(f):
        for d in dt:
            d = mp.mpf(float(d))
            ph = mp.mpf(float(fj)) * d
            if c2 is not None:
                ph += mp.mpf(float(c2[j])) * d * d
            for k in range(1, m + 1):
                x = 2 * mp.frac(k * ph)
                C[k - 1][j] += mp.cospi(x)
                S[k - 1][j] += mp.sinpi(x)
    return C, S


def mp_power(C, S, n, m, stat):
    import mpmath as mp
    out = []
    for j in range(len(C[0])):
        z = [C[k][j] ** 2 + S[k][j] ** 2 for k in range(m)]
        if stat == 0:
            out.append(mp.fsum(z) * (mp.mpf(2) / n))
        else:
            cum, vals = mp.mpf(0), []
            for k in range(m):
                cum += z[k] * (mp.mpf(2) / n)
                vals.append(cum - 4 * k)
            out.append(max(vals))
    return out


@pytest.mark.parametrize("twod", [False, True], ids=["1d", "2d"])
def test_truth_vs_mpmath(twod):
    """Every photon of a small shape (|f dt| up to ~1e6 cycles), k = 1 .. 20, Z^2 and H at m = 1 and 20: the truth's
    distance to the 60-digit value is at most 1/50 of the smallest unit at that shape."""
    import mpmath as mp
    n, J = (150, 4) if twod else (300, 8)
    t, t0 = photons(n, 2.8e5, 71 + twod)
    dt = t - t0
    f = F0 + (np.arange(J) - J // 2) * 2.0 ** -19
    c2 = R.c2_of(np.linspace(-11.5, -10.9, J)) if twod else None
    assert np.abs(f[:, None] * dt).max() > 9e5
    C, S = mp_sums(dt, f, c2, 20)
    T20 = R.Truth(dt, f, c2, 20)
    def ld(x):  # a long double as an mpf, exactly
        hi = np.float64(x)
        return mp.mpf(float(hi)) + mp.mpf(float(x - hi))
    dsum = max(max(abs(ld(T20.C[k, j]) - C[k][j]), abs(ld(T20.S[k, j]) - S[k][j])) for k in range(20) for j in range(J))
    print("truth vs mpmath (%s): max |dC_k|, |dS_k| = %.2e" % ("2-D" if twod else "1-D", float(dsum)))
    for m in (1, 20):
        T = T20.head(m)
        for stat in (0, 1):
            want = mp_power(C, S, n, m, stat)
            got = T.power(stat)
            err = np.array([float(abs(mp.mpf(float(g)) - w)) for g, w in zip(got, want)])
            half_ulp = np.spacing(np.abs(got)) / 2  # the fp64 rounding of the truth's own result
            unit = smallest_unit(T, stat)
            margin = float((unit / np.maximum(err, 1e-300)).min())
            print("truth vs mpmath (%s) m=%d %s: max err %.2e, smallest unit %.2e, unit/err >= %.1f"
                  % ("2-D" if twod else "1-D", m, G.NAMES[stat], err.max(), unit.min(), margin))
            assert (err <= half_ulp * 1.01).all()       # correctly rounded: the last fp64 digit of the 60-digit value
            assert (err <= unit / 50).all()


@pytest.fixture(scope="module")
def oracle_case():
    t, t0 = photons(1537, 2.0e5, 1)
    f = F0 + (np.arange(64) - 32) * 2.0 ** -21
    return t, t0, f, R.Truth(t - t0, f, None, 20)


def test_truth_vs_oracle_exact_argument(oracle_case):
    """orc_search_true (double-double phase, fp64 sums) against the truth on 1537 photons x 64 trials, m = 20, and on a
    3 x 16 2-D grid, m = 5: within 1/50 of the smallest unit."""
    t, t0, f, T = oracle_case
    fd = np.array([-11.5, -11.0, -10.7])
    f2 = f[24:40]
    T2 = R.Truth(t - t0, np.tile(f2, 3), np.repeat(R.c2_of(fd), f2.size), 5)
    for name, TT, kw in (("1-D m=20", T, dict(freq=f, nharm=20)), ("2-D m=5", T2, dict(freq=f2, nharm=5, freq_dot=fd))):
        for stat in (0, 1):
            got = O.search(t, stat=G.NAMES[stat], exact_argument=True, **kw)
            err = np.abs(got - TT.power(stat))
            unit = smallest_unit(TT, stat)
            print("orc_search_true vs truth %s %s: max |d| %.2e, smallest unit %.2e, unit/err >= %.1f"
                  % (name, G.NAMES[stat], err.max(), unit.min(), float((unit / np.maximum(err, 1e-300)).min())))
            assert (err <= unit / 50).all()


def test_numpy_reference_is_told_apart(oracle_case):
    """The reference's own formula np.cos(2 * k * np.pi * f * dt) rounds its argument three times (2 k pi, f, dt) where
    the fp64 kernels round f dt once: its distance to the truth is at most 3.5 argument terms of the fp64 unit -- and
    at least 100 times the distance between the two exact-argument evaluations, so the truth tests can tell a kernel
    that follows the reference's rounding from one that carries the argument."""
    t, t0, f, T = oracle_case
    k = np.arange(1, 21)[:, None, None]
    arg = 2 * k * np.pi * f[None, None, :] * (t - t0)[None, :, None]
    C, S = np.cos(arg).sum(axis=1), np.sin(arg).sum(axis=1)
    kk = np.arange(1, 21, dtype=np.float64)[:, None]
    d_arg = 2.0 * math.pi * R.U * kk * T.argmag[None, :]
    for stat in (0, 1):
        dist = np.abs(R.power_fp64(C, S, T.n, stat) - T.power(stat))
        arg_unit = R.stat_bound(T.g, R.cumulative_bound(T.A, d_arg, T.n), stat)
        exact2 = np.abs(O.search(t, f, 20, stat=G.NAMES[stat], exact_argument=True) - T.power(stat))
        print("numpy reference vs truth %s: max |d| %.2e = %.3f argument terms; orc_search_true vs truth %.2e"
              % (G.NAMES[stat], dist.max(), (dist / arg_unit).max(), exact2.max()))
        assert (dist <= 3.5 * arg_unit + R.fp64_unit(T, stat) - arg_unit).all()
        assert dist.max() >= 100 * exact2.max()


def model_subset(case, mmax, rng):
    """At most 24 of the case's checked trials (both ends and random ones): the model costs what the truth costs."""
    idx = case.idx(mmax)
    if idx.size > 24:
        idx = np.unique(np.concatenate([idx[:1], idx[-1:], rng.choice(idx, 22, replace=False)]))
    return idx


def test_fp64_models_stay_inside_the_fp64_unit():
    """NumPy models of the fp64 kernels (fl(f d), fl(ph k0), angle additions, groups of 8/4/2/1 and of 8 for the sets)
    at every shape the GPU tests use: inside the unit, the largest fractions printed."""
    rng = np.random.default_rng(5)
    worst = {}
    for case, mmax in G.CASES:
        idx = model_subset(case, mmax, rng)
        dt = case.t - case.t0
        f = case.f[idx % case.nf]
        c2 = None if case.c2 is None else case.c2[idx // case.nf]
        T = R.Truth(dt, f, c2, mmax)
        for sets in (False, True):
            for m in sorted({1, min(3, mmax), mmax}):
                C, S = R.fp64_model(dt, f, c2, m, sets)
                Tm = T.head(m)
                for stat in (0, 1):
                    frac = np.abs(R.power_fp64(C, S, T.n, stat) - Tm.power(stat)) / R.fp64_unit(Tm, stat, sets)
                    assert (frac <= 1.0).all(), (case.name, m, stat, sets, float(frac.max()))
                    key = ("sets" if sets else "direct", G.NAMES[stat])
                    worst[key] = max(worst.get(key, (0.0, "")), (float(frac.max()), "%s m=%d" % (case.name, m)))
    for key, (v, where) in sorted(worst.items()):
        print("fp64 model / unit, %s %s: max %.4f at %s" % (key + (v, where)))


def test_set_models_stay_inside_the_fp64_unit():
    for days in (False, True):
        t, off, f = G.set_photons(days)
        worst = 0.0
        for i, T in enumerate(G.set_truth(days)):
            C, S = R.fp64_model(T.dt, T.f, None, T.m, sets=True)
            for m in G.SET_HARMONICS:
                for stat in (0, 1):
                    Tm = T.head(m)
                    assert Tm.power(stat)[0] > 0
                    frac = abs(R.power_fp64(C[:m], S[:m], T.n, stat)[0] - Tm.power(stat)[0]) / R.fp64_unit(Tm, stat, True)[0]
                    assert frac <= 1.0, (days, i, m, stat)
                    worst = max(worst, float(frac))
        print("fp64 model / unit, sets (%s): max %.4f" % ("MJD days" if days else "seconds", worst))


def test_gpu_case_input_conditions():
    """What the GPU tests rely on, checked on the truth alone: |P| > 0 at every checked trial of every case and both
    statistics; where an argmax is asserted, the truth's two best trials lie further apart than the sum of their
    (default) units; the H_20 noise case has a checked trial with sum_k Z^2_k / |H| >= 50; the FFT families are the
    planned ones; the wrap cases are within the 32-wrap limit and the last one next to it."""
    for case, mmax in G.CASES:
        idx, T = case.truth(mmax)
        for m in sorted({1, mmax}):
            for stat in (0, 1):
                assert (np.abs(T.head(m).power(stat)) > 0).all(), (case.name, m, stat)
    for case, m in G.ARGMAX_CASES:
        idx, T = case.truth(m)
        assert idx.size == case.nf * case.rows
        for stat in (0, 1):
            p, u = T.power(stat), R.default_unit(T, stat)
            a, b = np.argsort(p)[-1], np.argsort(p)[-2]
            print("clear best %-22s %s: gap %.3e, units %.3e" % (case.name, G.NAMES[stat], p[a] - p[b], u[a] + u[b]))
            assert p[a] - p[b] > u[a] + u[b], (case.name, stat)
    idx, T = G.E_NOISE.truth(20)
    ratio = T.g[-1] / np.abs(T.power(1))
    print("H_20 on noise: max sum_k Z^2_k / |H| = %.1f at trial %d" % (ratio.max(), int(idx[np.argmax(ratio)])))
    assert ratio.max() >= 50.0
    for key, (case, nfft) in G.E_CASES.items():
        assert {R.nufft_plan_rule(case.nf, stat, 2)[0] for stat in (0, 1)} == {nfft}, key
    for key, case in G.E_WRAPS.items():
        wraps = 3 * case.step * (case.t[-1] - case.t[0]) + 1
        assert wraps < 32 and (key != "31" or wraps > 30), (key, wraps)
    assert not R.nufft_grid_deviation(G.E_GATHER.f, np.arange(G.E_GATHER.nf)).any()
    assert R.nufft_grid_deviation(G.E_LINSPACE.f, np.arange(G.E_LINSPACE.nf)).any()
