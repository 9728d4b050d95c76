"""Timing-model fits on the device (csrc/timing_fit.h): crimp_timing_nll against the reference's recorded residuals
and likelihoods (tests/golden/fittoas_nll_<case>.npz), crimp_timing_mcmc's bookkeeping, determinism and posterior,
the maximum-likelihood path and the local ephemerides. The reference's numbers come from
tests/golden/gen_fittoas_golden.py; nothing here needs emcee."""
import copy
import json
import os

import numpy as np
import pytest

from conftest import gold, gpath

SIZES = (1, 2, 63, 64, 65, 84, 257)
CASES = ("a", "b", "c", "d")
TOL_MU = 1e-9  # cycles: the project's calcphase bound


@pytest.fixture(scope="module")
def side():
    with open(gpath("fittoas.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def nllgold():
    return {c: dict(gold("fittoas_nll_%s.npz" % c)) for c in CASES}


def device_fit(side, g, case, n):
    from crimp_amd.utilities_fittoas import DeviceFit
    c = side["cases"][case]
    return DeviceFit(g["x_%d" % n], copy.deepcopy(c["model"]), c["keys"], g["y_%d" % n], g["e_%d" % n])


def evaluate(fit, pvec):
    """(nll [P], mu [P, n]) of one problem."""
    from crimp_amd import ops
    p = np.ascontiguousarray(pvec, dtype=float)
    nll, mu = ops.timing_nll(fit.x, fit.y, fit.yerr, fit.fit_base, fit.wave_base, fit.map, p[None], want_mu=True)
    return nll[0], mu.reshape(p.shape[0], fit.x.size)


# ------------------------------------------------------------------ 1. NLL and residual parity
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_nll_and_residuals_match_reference(gpu, side, nllgold, case):
    g = nllgold[case]
    assert float(g["max_abs_phase"]) <= 1e3
    for n in SIZES:
        fit = device_fit(side, g, case, n)
        nll, mu = evaluate(fit, g["pvec"])
        ref_mu, ref_nll = g["mu_%d" % n], g["nll_%d" % n]
        err = np.max(np.abs(mu - ref_mu))
        print(case, n, "max |mu - ref| %.3g" % err, "max |nll - ref| %.3g" % np.max(np.abs(nll - ref_nll)))
        assert err <= TOL_MU, (case, n, err)
        if n == 1:
            assert not mu.any()
        # the NLL bound a 1e-9-cycle error of every residual implies, from the fixture's residuals
        y, e = g["y_%d" % n], g["e_%d" % n]
        r = np.abs((y - np.mean(y))[None, :] - ref_mu)
        bound = np.sum(r * TOL_MU / e ** 2, axis=1) + 0.5 * np.sum((TOL_MU / e) ** 2) + 1e-13 * np.abs(ref_nll)
        assert np.all(np.abs(nll - ref_nll) <= bound), (case, n, np.max(np.abs(nll - ref_nll) / bound))
        # independent of P: one vector, five vectors and all 64 give the same bits
        nll1, mu1 = evaluate(fit, g["pvec"][:1])
        nll5, mu5 = evaluate(fit, g["pvec"][:5])
        np.testing.assert_array_equal(nll1, nll[:1])
        np.testing.assert_array_equal(mu1, mu[:1])
        np.testing.assert_array_equal(nll5, nll[:5])
        np.testing.assert_array_equal(mu5, mu[:5])


@pytest.mark.gpu
def test_nll_three_problems_in_one_call_are_bit_identical(gpu, side, nllgold):
    from crimp_amd import ops
    g = nllgold["b"]
    fits = [device_fit(side, g, "b", n) for n in (2, 65, 257)]
    pv = np.stack([g["pvec"][:5], g["pvec"][5:10], g["pvec"][10:15]])
    off = np.concatenate([[0], np.cumsum([f.x.size for f in fits])]).astype(np.int64)
    nll, mu = ops.timing_nll(np.concatenate([f.x for f in fits]), np.concatenate([f.y for f in fits]),
                             np.concatenate([f.yerr for f in fits]), [f.fit_base for f in fits],
                             [f.wave_base for f in fits], fits[0].map, pv, offsets=off, want_mu=True)
    for i, f in enumerate(fits):
        one_nll, one_mu = evaluate(f, pv[i])
        np.testing.assert_array_equal(nll[i], one_nll)
        np.testing.assert_array_equal(mu[5 * off[i]:5 * off[i + 1]].reshape(5, -1), one_mu)


@pytest.mark.gpu
def test_model_phase_residuals_and_make_nll_dropins(gpu, side, nllgold):
    from crimp_amd import utilities_fittoas as UF
    g, c = nllgold["d"], side["cases"]["d"]
    model = copy.deepcopy(c["model"])
    mu = UF.model_phase_residuals(g["x_84"], model, g["pvec"][3], c["keys"])
    assert mu.shape == (84,) and np.max(np.abs(mu - g["mu_84"][3])) <= TOL_MU
    nll, p0, keys, same = UF.make_nll(g["x_84"], g["y_84"], g["e_84"], model)
    assert keys == c["keys"] and same is model and not p0.any()
    assert isinstance(nll(g["pvec"][3]), float)
    assert nll(g["pvec"][3]) == evaluate(device_fit(side, g, "d", 84), g["pvec"][3:4])[0][0]


@pytest.mark.gpu
def test_timing_fit_argument_errors(gpu, side, nllgold):
    from crimp_amd import _native as N
    from crimp_amd import ops
    g = nllgold["a"]
    fit = device_fit(side, g, "a", 84)
    args = (fit.x, fit.y, fit.yerr, fit.fit_base, fit.wave_base)
    with pytest.raises(N.CrimpNativeError, match="no ToAs"):
        ops.timing_nll(fit.x, fit.y, fit.yerr, [fit.fit_base] * 2, [fit.wave_base] * 2, fit.map, np.zeros((2, 1, 2)),
                       offsets=np.array([0, 0, 84]))
    bad = ops.fit_map(["F0", "GLPH_1"])  # the model of case (a) has no glitch
    with pytest.raises(N.CrimpNativeError, match="glitch outside the model"):
        ops.timing_nll(*args, bad, np.zeros((1, 1, 2)))
    wide = ops.fit_map(["F0", "F1"])
    wide.ndim = N.FIT_MAX_DIM + 1  # above the cap
    with pytest.raises(N.CrimpNativeError, match="ndim"):
        ops.timing_nll(*args, wide, np.zeros((1, 1, N.FIT_MAX_DIM + 1)))
    with pytest.raises(ValueError):
        ops.timing_nll(*args, N.FitMap(), np.zeros((1, 1, 1)))  # ndim 0
    lo, hi = np.full((1, 2), -np.inf), np.full((1, 2), np.inf)
    for W in (3, 2, 258):  # odd, fewer than 2 ndim, more than 256
        with pytest.raises(N.CrimpNativeError, match="walkers"):
            ops.timing_mcmc(*args, fit.map, np.zeros((1, W, 2)), lo, hi, 5, 1)


@pytest.mark.gpu
def test_device_tensors_give_the_host_arrays_results(gpu, side, nllgold):
    """Device pointers (torch tensors, results stay on the GPU) and staged host arrays run the same kernels."""
    import torch
    from crimp_amd import ops
    g = nllgold["b"]
    fit = device_fit(side, g, "b", 65)
    nll, mu = evaluate(fit, g["pvec"][:7])
    dev = [torch.as_tensor(a, device=gpu) for a in (fit.x, fit.y, fit.yerr)]
    pv = torch.as_tensor(g["pvec"][None, :7], device=gpu)
    dnll, dmu = ops.timing_nll(*dev, fit.fit_base, fit.wave_base, fit.map, pv, want_mu=True)
    assert dnll.is_cuda and dmu.is_cuda
    np.testing.assert_array_equal(dnll.cpu().numpy()[0], nll)
    np.testing.assert_array_equal(dmu.cpu().numpy().reshape(7, 65), mu)
    p0 = g["pvec"][None, :18]
    lo, hi = np.full((1, 9), -np.inf), np.full((1, 9), np.inf)
    host = ops.timing_mcmc(fit.x, fit.y, fit.yerr, fit.fit_base, fit.wave_base, fit.map, p0, lo, hi, 10, 3)
    devo = ops.timing_mcmc(*dev, fit.fit_base, fit.wave_base, fit.map, *(torch.as_tensor(a, device=gpu)
                                                                       for a in (p0, lo, hi)), 10, 3)
    for h, d in zip(host, devo):
        np.testing.assert_array_equal(h, d.cpu().numpy())


# ------------------------------------------------------------------ 2. load_toas_for_fit
@pytest.mark.gpu
def test_load_toas_for_fit_matches_reference(gpu, side):
    from crimp_amd.fit_toas import load_toas_for_fit
    from crimp_amd.timfile import readtimfile
    g = gold("fittoas.npz")
    tim = readtimfile(gpath("ToAs_2259.tim"), comment="C")
    model = side["cases"]["a"]["model"]
    for name, kw in (("load", {}), ("load_wrapped", {"t_mjd_phasewrap": list(g["load_wraps"]), "mode": "add"})):
        df = load_toas_for_fit(tim.copy(), copy.deepcopy(model), **kw)
        assert list(df.columns) == ["ToA", "phase", "phase_err_cycle"]
        np.testing.assert_array_equal(df["ToA"], g[name + "_ToA"])
        np.testing.assert_array_equal(df["phase_err_cycle"], g[name + "_phase_err_cycle"])
        assert np.max(np.abs(df["phase"].to_numpy() - g[name + "_phase"])) <= TOL_MU


# ------------------------------------------------------------------ the linear (F0, F1) problem of case (a)
def linear_solution(x, y, e, pepoch):
    """Weighted least squares of y - mean(y) on the mean-subtracted design columns of (dF0, dF1): the posterior of
    case (a) is exactly Gaussian with this mean and covariance."""
    dt = (x - pepoch) * 86400.0
    A = np.stack([dt, 0.5 * dt * dt], axis=1)
    A = A - A.mean(axis=0)
    w = 1.0 / e ** 2
    cov = np.linalg.inv(A.T @ (A * w[:, None]))
    return cov @ (A.T @ (w * (y - y.mean()))), cov


@pytest.fixture(scope="module")
def case_a(side, nllgold):
    g = nllgold["a"]
    sol, cov = linear_solution(g["x_84"], g["y_84"], g["e_84"], side["cases"]["a"]["model"]["PEPOCH"]["value"])
    return g, sol, np.sqrt(np.diag(cov))


def run_chain(fit, p0, lo, hi, steps, seed, first_problem=0):
    from crimp_amd import ops
    return ops.timing_mcmc(fit.x, fit.y, fit.yerr, fit.fit_base, fit.wave_base, fit.map, p0[None], lo[None], hi[None],
                           steps, seed, first_problem=first_problem)


# ------------------------------------------------------------------ 3. sampler bookkeeping
@pytest.mark.gpu
@pytest.mark.parametrize("W, steps", [(4, 50), (32, 200)])
def test_sampler_bookkeeping(gpu, side, case_a, W, steps):
    g, sol, sig = case_a
    fit = device_fit(side, g, "a", 84)
    rng = np.random.default_rng(W)
    p0 = sol + rng.uniform(-3, 3, (W, 2)) * sig
    lo, hi = sol - 4 * sig, sol + 4 * sig  # tight enough that proposals leave the box
    chain, logprob, accepted = run_chain(fit, p0, lo, hi, steps, 11)
    chain, logprob, accepted = chain[0], logprob[0], accepted[0]
    # every stored log-probability is minus the likelihood kernel's value at the stored position, bit for bit
    nll, _ = evaluate(fit, chain.reshape(-1, 2))
    np.testing.assert_array_equal(logprob.reshape(-1), -nll)
    assert np.all((chain > lo) & (chain < hi))
    prev = np.concatenate([p0[None], chain[:-1]])
    moved = np.any(chain != prev, axis=2)
    np.testing.assert_array_equal(accepted, moved.sum(axis=0))
    assert 0 < moved.sum() < moved.size
    for s, w in zip(*np.nonzero(moved)):
        # the other half as it stood: the odd walkers of the previous step for an even walker, the even walkers of
        # this step for an odd one
        other = prev[s, 1::2] if w % 2 == 0 else chain[s, 0::2]
        z = (other - chain[s, w]) / (other - prev[s, w])  # per candidate and dimension
        ok = (np.abs(z[:, 0] - z[:, 1]) <= 1e-6 * np.abs(z[:, 0])) & (z[:, 0] >= 0.5 - 1e-9) & (z[:, 0] <= 2 + 1e-9)
        assert ok.any(), (s, w, z)


# ------------------------------------------------------------------ 4. determinism
@pytest.mark.gpu
def test_sampler_determinism_and_sharding(gpu, side, case_a):
    from crimp_amd import ops
    g, sol, sig = case_a
    fits = [device_fit(side, g, "a", n) for n in (63, 64, 65, 84, 257)]
    rng = np.random.default_rng(3)
    W, steps = 8, 30
    p0 = sol + rng.uniform(-3, 3, (5, W, 2)) * sig
    lo, hi = np.tile(sol - 50 * sig, (5, 1)), np.tile(sol + 50 * sig, (5, 1))

    def run(idx, seed, first):
        sub = [fits[i] for i in idx]
        off = np.concatenate([[0], np.cumsum([f.x.size for f in sub])]).astype(np.int64)
        return ops.timing_mcmc(np.concatenate([f.x for f in sub]), np.concatenate([f.y for f in sub]),
                               np.concatenate([f.yerr for f in sub]), [f.fit_base for f in sub],
                               [f.wave_base for f in sub], sub[0].map, p0[idx], lo[idx], hi[idx], steps, seed,
                               offsets=off, first_problem=first)

    all5 = run([0, 1, 2, 3, 4], 7, 0)
    again = run([0, 1, 2, 3, 4], 7, 0)
    for a, b in zip(all5, again):
        np.testing.assert_array_equal(a, b)
    other = run([0, 1, 2, 3, 4], 8, 0)
    assert np.any(other[0] != all5[0])
    head, tail = run([0, 1], 7, 0), run([2, 3, 4], 7, 2)
    for full, h, t in zip(all5, head, tail):
        np.testing.assert_array_equal(full[:2], h)
        np.testing.assert_array_equal(full[2:], t)


@pytest.mark.gpu
def test_chain_is_the_same_bits_staged_in_lds_or_read_from_global_memory(gpu, side, case_a):
    """Staging is decided by the call's largest problem: 6000 ToAs (3 doubles each) exceed the 128 KiB of LDS, so in
    the pair [small, large] both problems read their ToAs from global memory; alone, the small one is staged."""
    from crimp_amd import ops
    from crimp_amd.utilities_fittoas import DeviceFit
    g, sol, sig = case_a
    c = side["cases"]["a"]
    small = device_fit(side, g, "a", 65)
    rng = np.random.default_rng(6000)
    n = 6000
    assert 3 * 8 * n > 128 * 1024
    large = DeviceFit(np.sort(rng.uniform(small.x.min(), small.x.max(), n)), copy.deepcopy(c["model"]), c["keys"],
                      rng.normal(0, 0.01, n), np.full(n, 0.01))
    W, steps = 8, 10
    p0 = sol + rng.uniform(-3, 3, (2, W, 2)) * sig
    lo, hi = sol - 50 * sig, sol + 50 * sig
    alone = run_chain(small, p0[0], lo, hi, steps, 7)
    fits = [small, large]
    off = np.array([0, 65, 65 + n], dtype=np.int64)
    pair = ops.timing_mcmc(np.concatenate([f.x for f in fits]), np.concatenate([f.y for f in fits]),
                           np.concatenate([f.yerr for f in fits]), [f.fit_base for f in fits],
                           [f.wave_base for f in fits], small.map, p0, np.tile(lo, (2, 1)), np.tile(hi, (2, 1)), steps,
                           7, offsets=off, first_problem=0)
    for a, b in zip(alone, pair):
        np.testing.assert_array_equal(a[0], b[0])
    nll, _ = evaluate(large, pair[0][1].reshape(-1, 2))
    np.testing.assert_array_equal(pair[1][1].reshape(-1), -nll)


# ------------------------------------------------------------------ 5. posterior
MEDIAN_TOL, WIDTH_TOL, ACCEPT_RANGE = 0.15, 0.08, (0.55, 0.85)


def check_posterior(chain, accepted, burn, sol, sig):
    flat = chain[burn:].reshape(-1, chain.shape[-1])
    q16, q50, q84 = np.percentile(flat, [16, 50, 84], axis=0)
    acc = float(np.mean(accepted / chain.shape[0]))
    print("median offset / sigma", (q50 - sol) / sig, "half-widths / sigma", (q50 - q16) / sig, (q84 - q50) / sig,
          "acceptance", acc)
    assert np.all(np.abs(q50 - sol) <= MEDIAN_TOL * sig)
    assert np.all(np.abs((q50 - q16) / sig - 1) <= WIDTH_TOL) and np.all(np.abs((q84 - q50) / sig - 1) <= WIDTH_TOL)
    assert ACCEPT_RANGE[0] <= acc <= ACCEPT_RANGE[1]


def numpy_stretch(logp, p0, steps, rng, a=2.0):
    """The same move in NumPy: fixed even / odd halves, each updated against the other as it stands."""
    W, nd = p0.shape
    pos, lp = p0.copy(), logp(p0)
    chain, acc = np.empty((steps, W, nd)), np.zeros(W)
    for s in range(steps):
        for h in (0, 1):
            mine, other = np.arange(h, W, 2), np.arange(1 - h, W, 2)
            z = ((a - 1) * rng.uniform(size=mine.size) + 1) ** 2 / a
            c = pos[rng.choice(other, mine.size)]
            q = c - (c - pos[mine]) * z[:, None]
            lq = logp(q)
            ok = np.log(rng.uniform(size=mine.size)) < (nd - 1) * np.log(z) + lq - lp[mine]
            pos[mine[ok]], lp[mine[ok]] = q[ok], lq[ok]
            acc[mine[ok]] += 1
        chain[s] = pos
    return chain, acc


def test_numpy_restatement_meets_the_posterior_bounds():
    """The bounds of the device test, on the CPU: the NumPy restatement of the move on a 40-ToA synthetic (F0, F1)
    problem, 3000 steps, four seeds."""
    for seed in range(4):
        rng = np.random.default_rng(100 + seed)
        x = np.sort(rng.uniform(58000, 58400, 40))
        e = rng.uniform(0.005, 0.02, 40)
        y = rng.normal(0, e)
        sol, cov = linear_solution(x, y, e, 58200.0)
        sig = np.sqrt(np.diag(cov))
        dt = (x - 58200.0) * 86400.0
        A = np.stack([dt, 0.5 * dt * dt], axis=1)
        A = A - A.mean(axis=0)

        def logp(p):
            r = ((y - y.mean())[None, :] - p @ A.T) / e
            return -0.5 * np.sum(r ** 2 + np.log(2 * np.pi * e ** 2), axis=1)

        p0 = sol + rng.uniform(-50, 50, (32, 2)) * sig
        chain, acc = numpy_stretch(logp, p0, 3000, rng)
        check_posterior(chain, acc, 500, sol, sig)


@pytest.mark.gpu
def test_posterior_of_the_linear_problem(gpu, side, case_a):
    g, sol, sig = case_a
    fit = device_fit(side, g, "a", 84)
    rng = np.random.default_rng(1)
    p0 = sol + rng.uniform(-50, 50, (32, 2)) * sig
    chain, _, accepted = run_chain(fit, p0, sol - 1e4 * sig, sol + 1e4 * sig, 4000, 2024)
    check_posterior(chain[0], accepted[0], 500, sol, sig)


@pytest.mark.gpu
def test_run_mcmc_dropin(gpu, side, case_a):
    from crimp_amd import fit_toas as FT
    from crimp_amd.utilities_fittoas import Prior
    g, sol, sig = case_a
    c = side["cases"]["a"]
    prior = Prior(bounds={k: (sol[i] - 20 * sig[i], sol[i] + 20 * sig[i]) for i, k in enumerate(c["keys"])},
                  initial_guess={})
    out = [FT.run_mcmc(g["x_84"], g["y_84"], g["e_84"], copy.deepcopy(c["model"]), c["keys"], prior, steps=600,
                       burn=200, walkers=16, progress=False, seed=5) for _ in range(2)]
    sampler, flat, summ = out[0]
    assert sampler.get_chain().shape == (600, 16, 2) and flat.shape == (400 * 16, 2)
    assert sampler.get_log_prob(discard=200, flat=True).shape == (400 * 16,)
    assert sampler.acceptance_fraction.shape == (16,)
    np.testing.assert_array_equal(flat, out[1][1])  # seeded: reproducible
    assert summ == FT.summarize_chain(flat, sampler.get_log_prob(discard=200, flat=True), c["keys"])
    for i, k in enumerate(c["keys"]):
        assert abs(summ[k]["median"] - sol[i]) <= 0.5 * sig[i]


# ------------------------------------------------------------------ 6. maximum-likelihood path
@pytest.mark.gpu
def test_device_objective_reaches_reference_minimum(gpu, side, case_a):
    from crimp_amd import fit_toas as FT
    g, _, _ = case_a
    ref = gold("fittoas.npz")
    c = side["cases"]["a"]
    nll, p0, keys, _ = FT.make_nll(g["x_84"], g["y_84"], g["e_84"], copy.deepcopy(c["model"]))
    res = FT.minimize_nll(nll, p0, keys)
    print("device Nelder-Mead", res.x, res.fun, "reference", ref["nm_x"], float(ref["nm_fun"]))
    assert res.fun <= float(ref["nm_fun"]) + 1e-3  # 10 x scipy's fatol


# ------------------------------------------------------------------ 7. local ephemerides
@pytest.mark.gpu
def test_local_ephemerides_one_launch_for_all_windows(gpu, monkeypatch):
    from crimp_amd import get_local_ephem as GL
    from crimp_amd.fit_toas import load_toas_for_fit
    from crimp_amd.readtimingmodel import ReadTimingModel
    from crimp_amd.timfile import readtimfile
    ref = gold("fittoas.npz")
    calls = []
    real = GL.ops.timing_mcmc
    monkeypatch.setattr(GL.ops, "timing_mcmc", lambda *a, **k: calls.append(1) or real(*a, **k))
    par, tim = gpath("1e2259.par"), gpath("ToAs_2259.tim")
    df = GL.generate_local_ephemerides(tim, par, outputfile=None, seed=9)
    assert len(calls) == 1
    assert list(df.columns) == ["TOA_MJD_ref", "TOA_MJD_ref_err", "F0", "F0_err", "F1", "F1_err", "CHI2R", "DOF"]
    for c in ("TOA_MJD_ref", "TOA_MJD_ref_err", "DOF"):
        np.testing.assert_array_equal(df[c], ref["win_" + c])
    assert np.all(np.isfinite(df["CHI2R"]))
    params = ReadTimingModel(par).readfulltimingmodel()[0]
    for i, win in enumerate(GL.local_ephem_windows(readtimfile(tim), par)):
        model = GL.window_model(win)
        toas = load_toas_for_fit(win["toas"], model)
        sol, cov = linear_solution(toas["ToA"].to_numpy(), toas["phase"].to_numpy(),
                                   toas["phase_err_cycle"].to_numpy(), win["mid"])
        sig = np.sqrt(np.diag(cov))
        trend = params["F0"] + params["F1"] * ((win["mid"] - params["PEPOCH"]) * 86400)
        f0 = (win["F0_mid"] - sol[0]) - trend
        f1 = win["F1_mid"] - sol[1]
        print(i, "F0 offset / sigma", (df["F0"][i] - f0) / sig[0], "F1 offset / sigma", (df["F1"][i] - f1) / sig[1])
        assert abs(df["F0"][i] - f0) <= 0.3 * sig[0]
        assert abs(df["F1"][i] - f1) <= 0.3 * sig[1]
