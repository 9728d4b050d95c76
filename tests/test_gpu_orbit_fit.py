"""Orbit fits on the device (csrc/orbit_fit.h): crimp_orbit_nll against the 60-digit residuals of
tests/golden/orbit_fit.npz within the derived bound (tests/orbit_fit_reference.py), the exactness of zero orbital
entries, independence of the launch shape, inadmissible orbits, crimp_orbit_mcmc's bookkeeping, injection and recovery
through crimp_amd.fit_orbit, and the C-ABI's errors."""
import ctypes

import numpy as np
import pytest

import orbit_fit_reference as O

P_EDGE = (1, 4, 5)      # 4 -> 5 is the waves-per-block edge of kTfNllWaves = 4


@pytest.fixture(scope="module")
def fixture():
    return O.load_fixture()


def flagged(tm, keys):
    return {k: ({"value": v, "flag": None} if k == "BINARY" else {"value": v, "flag": int(k in keys)})
            for k, v in tm.items()}


def data(c, seed=0):
    """(y, yerr) of a fixture case: the 'typical' vector's residuals plus noise of 1e-3 cycles, a fixed seed."""
    rng = np.random.default_rng(1000 * c.n + seed)
    e = 1e-3 * rng.uniform(0.5, 1.5, c.n)
    return c.mu_ref()[3] + e * rng.standard_normal(c.n), e


def problem(c, keys=None, seed=0):
    from crimp_amd.fit_orbit import OrbitFit
    keys = c.keys if keys is None else keys
    y, e = data(c, seed)
    return OrbitFit(c.t, flagged(c.tm, keys), keys, y, e)


def evaluate(fit, pvec):
    """(nll [P], mu [P, n]) of one problem."""
    from crimp_amd import ops
    p = np.ascontiguousarray(pvec, dtype=float)
    nll, mu = ops.orbit_nll(fit.x, fit.y, fit.yerr, fit.par, fit.fit_base, fit.wave_base, fit.map, p[None],
                            want_mu=True)
    return nll[0], mu.reshape(p.shape[0], fit.x.size)


def sample(fit, p0, lo, hi, steps, seed, first_problem=0):
    from crimp_amd import ops
    ch, lp, acc = ops.orbit_mcmc(fit.x, fit.y, fit.yerr, fit.par, fit.fit_base, fit.wave_base, fit.map, p0[None],
                                 lo[None], hi[None], steps, seed, first_problem=first_problem)
    return ch[0], lp[0], acc[0]


def many(fits, pvecs=None, mcmc=None):
    """Several problems that share their keys in one launch: ([nll_i], [mu_i]) or, with ``mcmc`` = (p0 list, lo, hi,
    steps, seed, first_problem), (chain, logprob, accepted) of all."""
    from crimp_amd import ops
    t = np.concatenate([f.x for f in fits])
    y = np.concatenate([f.y for f in fits])
    e = np.concatenate([f.yerr for f in fits])
    off = np.concatenate([[0], np.cumsum([f.x.size for f in fits])]).astype(np.int64)
    pars, fb, wb = [f.par for f in fits], [f.fit_base for f in fits], [f.wave_base for f in fits]
    if mcmc is None:
        P = pvecs[0].shape[0]
        nll, mu = ops.orbit_nll(t, y, e, pars, fb, wb, fits[0].map, np.stack(pvecs), offsets=off, want_mu=True)
        return [nll[i] for i in range(len(fits))], [mu[P * off[i]: P * off[i + 1]].reshape(P, -1)
                                                    for i in range(len(fits))]
    p0, lo, hi, steps, seed, first = mcmc
    return ops.orbit_mcmc(t, y, e, pars, fb, wb, fits[0].map, np.stack(p0), np.stack(lo), np.stack(hi), steps, seed,
                          offsets=off, first_problem=first)


# ------------------------------------------------------------------ 1. residuals and NLL against the fixture
@pytest.mark.gpu
@pytest.mark.parametrize("name", O.MODELS)
def test_residuals_and_nll_within_the_derived_bound(gpu, fixture, name):
    """mu within FACTOR u A plus the mean's share of the 60-digit value for every vector (zero, orbital only, spin only,
    typical widths, 1e3 widths), every n and P in {1, 4, 5}; the NLL within the bound that implies. Largest
    |mu - mp| / bound measured on the MI355X: 0.070 (bt_e07, the 1e3-width vector; the host twin: 0.071)."""
    worst = 0.0
    for n in O.SIZES:
        c = fixture[(name, n)]
        fit = problem(c)
        bound, ref = c.bound(), c.mu_ref()
        full_nll = None
        for P in P_EDGE[::-1]:
            nll, mu = evaluate(fit, c.pvec[:P])
            assert np.isfinite(nll).all() and np.isfinite(mu).all()
            ratio = float(np.max(c.mu_err(mu) / bound[:P]))
            worst = max(worst, ratio)
            print(name, n, P, "max |mu - mp| / bound %.3g" % ratio)
            assert ratio <= 1.0, (name, n, P, ratio)
            for j in range(P):
                want = O.nll_exact(fit.y, ref[j], fit.yerr)
                lim = O.nll_bound(fit.y, ref[j], fit.yerr, bound[j])
                assert abs(nll[j] - want) <= lim, (name, n, P, j, abs(nll[j] - want) / lim)
            if full_nll is None:
                full_nll, full_mu = nll, mu
            else:                               # a value does not depend on P
                np.testing.assert_array_equal(nll, full_nll[:P])
                np.testing.assert_array_equal(mu, full_mu[:P])
        if n == 1:
            assert not full_mu.any()
    print(name, "largest ratio %.3g" % worst)


# ------------------------------------------------------------------ 2. zero orbital entries change nothing
@pytest.mark.gpu
@pytest.mark.parametrize("name", ("bt_full", "ell1_amxp"))
def test_zero_orbital_entries_equal_the_spin_fit_under_the_fixed_orbit(gpu, fixture, name):
    for n in (2, 65, 257):
        c = fixture[(name, n)]
        orb = np.array([k in O.ORBITAL for k in c.keys])
        spin_keys = [k for k, o in zip(c.keys, orb) if not o]
        rows = c.pvec[[0, 2, 2, 2, 2]] * np.array([1.0, 1.0, -1.0, 1e3, 0.5])[:, None]
        assert not rows[:, orb].any() and rows[1:, ~orb].all()
        nll_a, mu_a = evaluate(problem(c), rows)
        nll_s, mu_s = evaluate(problem(c, spin_keys), rows[:, ~orb])
        np.testing.assert_array_equal(mu_a, mu_s)
        np.testing.assert_array_equal(nll_a, nll_s)


# ------------------------------------------------------------------ 3. independence of the launch shape
def walkers(c, W, seed):
    rng = np.random.default_rng(seed)
    w = np.abs(c.pvec[3])
    return rng.uniform(-3, 3, (W, len(c.keys))) * w, -20 * w, 20 * w


@pytest.mark.gpu
def test_values_do_not_depend_on_the_launch_shape(gpu, fixture):
    cs = [fixture[("bt_e07", 63)], fixture[("bt_e095", 65)], fixture[("hmxb_wide", 257)]]
    assert cs[0].keys == cs[1].keys == cs[2].keys
    fits = [problem(c) for c in cs]
    alone = [evaluate(f, c.pvec) for f, c in zip(fits, cs)]
    nll3, mu3 = many(fits, [c.pvec for c in cs])
    for i in range(3):
        np.testing.assert_array_equal(nll3[i], alone[i][0])
        np.testing.assert_array_equal(mu3[i], alone[i][1])
    again = evaluate(fits[1], cs[1].pvec)
    np.testing.assert_array_equal(again[0], alone[1][0])
    np.testing.assert_array_equal(again[1], alone[1][1])
    # the sampler: alone with first_problem = 1 is the middle of three from first_problem = 0, and a repeat is identical
    W, steps, seed = 16, 40, 77
    starts = [walkers(c, W, 5 + i) for i, c in enumerate(cs)]
    ch3, lp3, acc3 = many(fits, mcmc=([s[0] for s in starts], [s[1] for s in starts], [s[2] for s in starts], steps,
                                      seed, 0))
    ch, lp, acc = sample(fits[1], *starts[1], steps, seed, first_problem=1)
    np.testing.assert_array_equal(ch, ch3[1])
    np.testing.assert_array_equal(lp, lp3[1])
    np.testing.assert_array_equal(acc, acc3[1])
    ch2, lp2, acc2 = sample(fits[1], *starts[1], steps, seed, first_problem=1)
    np.testing.assert_array_equal(ch, ch2)
    np.testing.assert_array_equal(lp, lp2)
    ch0, _, _ = sample(fits[1], *starts[1], steps, seed, first_problem=0)
    assert not np.array_equal(ch0, ch)        # another global index: another random stream
    assert 0 < acc.sum() < W * steps


# ------------------------------------------------------------------ 4. inadmissible vectors
def bad_vectors(c):
    """{what: vector} pushing the corrected orbit outside each limit of the case's kind."""
    tm, keys = c.tm, c.keys
    z = np.zeros(len(keys))

    def one(key, value):
        v = z.copy()
        v[keys.index(key)] = value
        return v
    pb, a1 = float(tm["PB"]), float(tm["A1"])
    out = {"PB = 0": one("PB", pb), "PB < 0": one("PB", 2 * pb), "A1 < 0": one("A1", a1 + 1.0),
           "NaN": one("A1", np.nan), "inf": one("PB", np.inf), "-inf": one("PB", -np.inf)}
    if str(tm["BINARY"]) == "BT":
        e = float(tm["ECC"])
        out.update({"ECC = 1": one("ECC", e - 1.0), "ECC > 1": one("ECC", e - 1.5), "ECC < 0": one("ECC", e + 0.25),
                    "contraction": one("A1", a1 - 0.26 * pb * 86400.0 * (1 - e) / np.pi)})
    else:
        out.update({"EPS1 = 1": one("EPS1", float(tm["EPS1"]) - 1.0), "EPS2 = -2": one("EPS2", float(tm["EPS2"]) + 2.0),
                    "contraction": one("A1", a1 - 0.26 * pb * 86400.0 / np.pi)})
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("bt_e07", "ell1_amxp"))
def test_inadmissible_vectors_give_inf_and_leave_their_neighbours_alone(gpu, fixture, name):
    c = fixture[(name, 65)]
    fit = problem(c)
    bad = bad_vectors(c)
    good_nll, good_mu = evaluate(fit, c.pvec)
    rows, kinds = [], []
    for i, (what, v) in enumerate(bad.items()):     # good and bad vectors interleaved: 5 + len(bad) rows
        if i < 5:
            rows.append(c.pvec[i])
            kinds.append(i)
        rows.append(v)
        kinds.append(what)
    nll, mu = evaluate(fit, np.array(rows))
    assert not np.isnan(nll).any()
    for k, what in enumerate(kinds):
        if isinstance(what, str):
            assert nll[k] == np.inf, what
            assert np.all(mu[k] == np.inf), what
        else:
            assert nll[k] == good_nll[what] and np.array_equal(mu[k], good_mu[what])
    # alone, too (P = 1)
    for what, v in bad.items():
        assert evaluate(fit, v[None])[0][0] == np.inf, what


@pytest.mark.gpu
def test_inadmissible_orbits_never_enter_a_chain(gpu, fixture):
    """ToA errors of 1e6 cycles make the likelihood flat: the walkers wander through a box that reaches past ECC = 1
    and A1 = 0, and only the orbit's limits stop them."""
    from crimp_amd.fit_orbit import OrbitFit
    c = fixture[("bt_e07", 64)]
    keys = ["ECC", "A1"]
    ecc, a1 = float(c.tm["ECC"]), float(c.tm["A1"])
    fit = OrbitFit(c.t, flagged(c.tm, keys), keys, np.zeros(c.n), np.full(c.n, 1e6))
    W, steps = 32, 600
    rng = np.random.default_rng(3)
    p0 = np.column_stack([rng.uniform(-0.2, 0.2, W), rng.uniform(-5, 5, W)])
    lo, hi = np.array([ecc - 1.5, a1 - 60.0]), np.array([ecc + 0.5, a1 + 20.0])     # ECC in (-0.5, 1.5), A1 in (-20, 60)
    ch, lp, acc = sample(fit, p0, lo, hi, steps, 11)
    e_full, a_full = ecc - ch[..., 0], a1 - ch[..., 1]
    assert np.isfinite(lp).all()
    assert e_full.min() >= 0.0 and e_full.max() < 1.0 and a_full.min() >= 0.0
    assert e_full.min() < 0.2 and e_full.max() > 0.9 and a_full.min() < 5.0      # they did reach the limits
    assert (acc < steps).all() and acc.sum() > 0
    nll, _ = evaluate(fit, ch.reshape(-1, 2)[::7])
    assert np.isfinite(nll).all()


# ------------------------------------------------------------------ 5. the sampler's bookkeeping
@pytest.mark.gpu
@pytest.mark.parametrize("name,n", (("ell1_amxp", 65), ("bt_full", 257)))
def test_mcmc_logprob_and_accepted(gpu, fixture, name, n):
    c = fixture[(name, n)]
    fit = problem(c)
    W, steps = 2 * len(c.keys) + 2, 30
    p0, lo, hi = walkers(c, W, 9)
    ch, lp, acc = sample(fit, p0, lo, hi, steps, 123)
    nll, _ = evaluate(fit, ch.reshape(-1, len(c.keys)))
    np.testing.assert_array_equal(lp.reshape(-1), -nll)
    prev = np.concatenate([p0[None], ch[:-1]])
    moved = np.any(ch != prev, axis=2)
    np.testing.assert_array_equal(moved.sum(axis=0), acc)
    assert 0 < acc.sum() < W * steps
    assert np.all((ch > lo) & (ch < hi))


@pytest.mark.gpu
def test_chain_is_the_same_bits_staged_in_lds_or_read_from_global_memory(gpu, fixture):
    """Staging is decided by the call's largest problem: 3000 ToAs (6 doubles each) exceed the 128 KiB of LDS, so in
    the pair [small, large] both problems read their ToAs and constants from global memory; alone, the small one is
    staged. W = 2 ndim + 2 = 16: the case has seven free keys, and a call with fewer than 2 ndim walkers is refused."""
    from crimp_amd.fit_orbit import OrbitFit
    c = fixture[("ell1_amxp", 65)]
    small = problem(c)
    rng = np.random.default_rng(3000)
    n = 3000
    assert 6 * 8 * n > 128 * 1024
    large = OrbitFit(np.sort(rng.uniform(c.t.min(), c.t.max(), n)), flagged(c.tm, c.keys), c.keys,
                     rng.normal(0, 0.01, n), np.full(n, 0.01))
    W, steps = 2 * len(c.keys) + 2, 10
    starts = [walkers(c, W, 21), walkers(c, W, 22)]
    alone = sample(small, *starts[0], steps, 31)
    pair = many([small, large], mcmc=([s[0] for s in starts], [s[1] for s in starts], [s[2] for s in starts], steps,
                                      31, 0))
    for a, b in zip(alone, pair):
        np.testing.assert_array_equal(a, b[0])
    nll, _ = evaluate(large, pair[0][1].reshape(-1, len(c.keys)))
    np.testing.assert_array_equal(pair[1][1].reshape(-1), -nll)


# ------------------------------------------------------------------ 6. injection and recovery
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(O.INJECTION))
def test_injection_recovery(gpu, name):
    """64 ToAs drawn from full(p_true): the minimiser and a 32 x 2000 chain recover every parameter within 5 posterior
    sigma, and every posterior sigma is within a factor 2 of the linearised least-squares sigma of the host twin."""
    from crimp_amd import fit_orbit as F
    from crimp_amd.utilities_fittoas import Prior
    prob = O.injection_problem(name)
    keys, sig, truth = prob["keys"], prob["sigma"], prob["p_true"]
    nll, p0, fkeys, _ = F.make_nll(prob["t"], prob["y"], prob["yerr"], prob["tm"])
    assert fkeys == keys and not p0.any()
    res = F.minimize_orbit(nll.problem, p0)
    print(name, "minimiser pull", np.round((res.x - truth) / sig, 2), "sigma ratio", np.round(res.sigma / sig, 3))
    assert np.all(np.abs(res.x - O.least_squares_host(prob)) < 0.01 * sig)     # the twin's own solution
    prior = Prior(bounds={k: (-10 * s, 10 * s) for k, s in zip(keys, sig)}, initial_guess={})
    sampler, flat, summ = F.run_mcmc(prob["t"], prob["y"], prob["yerr"], prob["tm"], keys, prior, steps=2000,
                                     burn=500, walkers=32, seed=4)
    assert sampler.get_chain().shape == (2000, 32, len(keys))
    post = flat.std(axis=0)
    med = np.array([summ[k]["median"] for k in keys])
    print(name, "chain pull", np.round((med - truth) / post, 2), "sigma ratio", np.round(post / sig, 3),
          "acceptance %.2f" % sampler.acceptance_fraction.mean())
    assert np.all(np.abs(res.x - truth) < 5 * post)
    assert np.all(np.abs(med - truth) < 5 * post)
    assert np.all((post > 0.5 * sig) & (post < 2 * sig))
    assert np.all((res.sigma > 0.5 * sig) & (res.sigma < 2 * sig))


# ------------------------------------------------------------------ 7. the C-ABI's errors
SENTINEL = -7.0


class Raw:
    """crimp_orbit_nll / _mcmc / crimp_timing_nll called through ctypes with sentinel-filled outputs."""

    def __init__(self, c):
        from crimp_amd import _native as N
        self.N, self.L = N, N.load()
        self.fit = problem(c)
        n = self.fit.x.size
        self.n = n
        self.off = np.array([0, n], dtype=np.int64)
        self.nd = len(c.keys)

    def slots(self, slots, ndim=None, branch=0, f0=-1):
        m = self.N.FitMap()
        m.ndim = len(slots) if ndim is None else ndim
        m.branch, m.f0_param = branch, f0
        for i, s in enumerate(slots):
            m.slot[i].kind, m.slot[i].index, m.slot[i].sub = s
        return m

    def _ptr(self, a):
        return ctypes.c_void_p(a.ctypes.data)

    def nll(self, par=None, fmap=None, P=1, timing=False, fit_base=None):
        f = self.fit
        par = f.par if par is None else par
        fmap = f.map if fmap is None else fmap
        nd = max(int(fmap.ndim), 1)
        pvec = np.zeros(max(P, 1) * nd)
        nll, mu = np.full(max(P, 1), SENTINEL), np.full(max(P, 1) * self.n, SENTINEL)
        head = [self._ptr(f.x), self._ptr(f.y), self._ptr(f.yerr), self._ptr(self.off), 1]
        tail = [ctypes.byref(fmap), self._ptr(pvec), P, self._ptr(nll), self._ptr(mu), 0, None]
        fb = f.fit_base if fit_base is None else fit_base
        if timing:
            rc = self.L.crimp_timing_nll(*head, ctypes.byref(fb), ctypes.byref(f.wave_base), *tail)
        else:
            rc = self.L.crimp_orbit_nll(*head, ctypes.byref(par), ctypes.byref(fb), ctypes.byref(f.wave_base), *tail)
        msg = self.L.crimp_last_error().decode() if rc else ""
        return rc, msg, bool(np.all(nll == SENTINEL) and np.all(mu == SENTINEL))

    def mcmc(self, par=None, fmap=None, W=None, steps=3):
        f = self.fit
        par = f.par if par is None else par
        fmap = f.map if fmap is None else fmap
        nd = max(int(fmap.ndim), 1)
        W = 2 * nd if W is None else W
        Wn = max(W, 2)
        p0, lo, hi = np.zeros(Wn * nd), np.full(nd, -1.0), np.full(nd, 1.0)
        chain, lp = np.full(steps * Wn * nd, SENTINEL), np.full(steps * Wn, SENTINEL)
        acc = np.full(Wn, int(SENTINEL), dtype=np.int64)
        rc = self.L.crimp_orbit_mcmc(self._ptr(f.x), self._ptr(f.y), self._ptr(f.yerr), self._ptr(self.off), 1,
                                     ctypes.byref(par), ctypes.byref(f.fit_base), ctypes.byref(f.wave_base),
                                     ctypes.byref(fmap), self._ptr(p0), self._ptr(lo), self._ptr(hi), W, steps, 1, 0,
                                     self._ptr(chain), self._ptr(lp), self._ptr(acc), 0, None)
        msg = self.L.crimp_last_error().decode() if rc else ""
        return rc, msg, bool(np.all(chain == SENTINEL) and np.all(lp == SENTINEL) and np.all(acc == int(SENTINEL)))


def changed(par, **fields):
    out = type(par).from_buffer_copy(par)       # a ctypes structure: a bytewise copy
    for k, v in fields.items():
        setattr(out, k, v)
    return out


@pytest.mark.gpu
def test_capi_errors_write_nothing(gpu, fixture):
    bt, ell1 = Raw(fixture[("bt_e07", 63)]), Raw(fixture[("ell1_amxp", 63)])
    N = bt.N
    B = N.FIT_SLOT_BINARY
    field = N.ORBIT_FIELDS.index
    for call in ("nll", "mcmc"):
        def err(raw, **kw):
            rc, msg, untouched = getattr(raw, call)(**kw)
            assert rc != 0 and untouched, (call, kw, rc, msg)
            return msg
        # the calls work as set up
        rc, msg, untouched = getattr(bt, call)()
        assert rc == 0 and not untouched, msg
        assert err(bt, par=changed(bt.fit.par, binary=0)) == "the model has no binary"
        assert err(bt, par=changed(bt.fit.par, binary=7)).startswith("binary must be CRIMP_BINARY_NONE")
        # a base orbit outside the limits: the texts of crimp_binary_delay
        assert err(bt, par=changed(bt.fit.par, bin_pb=0.0)) == "PB must be positive"
        assert err(bt, par=changed(bt.fit.par, bin_a1=-1.0)) == "A1 must be >= 0"
        assert err(bt, par=changed(bt.fit.par, bin_ecc=1.0)) == "ECC must be in [0, 1)"
        assert err(bt, par=changed(bt.fit.par, bin_a1=2e4)) == "2 pi A1 / (PB (1 - e)) must be below 1/2"
        assert err(bt, par=changed(bt.fit.par, bin_om=float("nan"))) == "a binary parameter is not finite"
        assert err(ell1, par=changed(ell1.fit.par, bin_eps1=0.8, bin_eps2=0.7)) == "EPS1^2 + EPS2^2 must be below 1"
        # a field the model's kind does not have
        text = "slot names an orbit field the model's kind does not have"
        for name in ("ECC", "OM", "OMDOT", "GAMMA"):
            assert err(ell1, fmap=ell1.slots([(0, 0, 0), (B, field(name), 0)], f0=0)) == text
            rc, _, _ = getattr(bt, call)(fmap=bt.slots([(0, 0, 0), (B, field(name), 0)], f0=0))
            assert rc == 0
        for name in ("EPS1", "EPS2"):
            assert err(bt, fmap=bt.slots([(B, field(name), 0)])) == text
            rc, _, _ = getattr(ell1, call)(fmap=ell1.slots([(B, field(name), 0)]))
            assert rc == 0
        assert err(bt, fmap=bt.slots([(B, 11, 0)])) == "slot names an orbit field outside CRIMP_ORBIT_PB..CRIMP_ORBIT_A1DOT"
        assert err(bt, fmap=bt.slots([(B, -1, 0)])) == "slot names an orbit field outside CRIMP_ORBIT_PB..CRIMP_ORBIT_A1DOT"
        assert err(bt, fmap=bt.slots([(B, 0, 0), (B, 0, 0)])) == "two slots name one orbit field"
        # the existing argument errors
        assert err(bt, fmap=bt.slots([], ndim=0)) == "ndim must be 1..CRIMP_FIT_MAX_DIM"
        assert err(bt, fmap=bt.slots([(4, 0, 0)])) == "unknown slot kind"
        assert err(bt, fmap=bt.slots([(0, 13, 0)])) == "slot names an F term outside F0..F12"
        assert err(bt, fmap=bt.slots([(1, 0, 1)])) == "slot names a glitch outside the model"
        assert err(bt, fmap=bt.slots([(2, 0, 0)])) == "a wave slot with CRIMP_FIT_WAVES_FIXED"
        assert err(bt, fmap=bt.slots([(B, 0, 0), (0, 1, 0)], f0=1)) == "f0_param is not an F0 slot"
    assert bt.nll(P=0)[1] == "P out of range" and bt.nll(P=0)[2]
    assert bt.mcmc(W=3)[1] == "walkers: even, >= 2 ndim and <= 256" and bt.mcmc(W=3)[2]
    assert bt.mcmc(W=2)[1] == "walkers: even, >= 2 ndim and <= 256"
    assert bt.mcmc(steps=0)[1] == "steps out of range"
    # the binary-free calls still refuse the orbit, and a BINARY slot
    rc, msg, untouched = bt.nll(timing=True, fmap=bt.slots([(0, 0, 0), (B, 0, 0)], f0=0))
    assert rc != 0 and untouched and msg == "a BINARY slot: crimp_orbit_nll and crimp_orbit_mcmc fit the orbit"
    rc, msg, untouched = bt.nll(timing=True, fmap=bt.slots([(0, 0, 0)], f0=0), fit_base=bt.fit.par)
    assert rc != 0 and untouched and msg == "binary models are not fitted yet"
    rc, msg, untouched = bt.nll(timing=True, fmap=bt.slots([(0, 0, 0)], f0=0))
    assert rc == 0 and not untouched, msg


@pytest.mark.gpu
def test_python_entry_points(gpu, fixture):
    """OrbitFit, make_nll and the ops wrappers on one case: shapes, the scalar / batched forms, and the refusals that
    stay (ops.timing_nll with a model that has an orbit)."""
    from crimp_amd import ops
    c = fixture[("ell1_amxp", 64)]
    fit = problem(c)
    one = fit.nll(c.pvec[3])
    allv = fit.nll(c.pvec)
    assert isinstance(one, float) and allv.shape == (5,) and allv[3] == one
    assert fit.residuals(c.pvec[3]).shape == (64,) and fit.residuals(c.pvec).shape == (5, 64)
    with pytest.raises(ValueError, match="binary models are not fitted yet"):
        ops.timing_nll(fit.x, fit.y, fit.yerr, fit.par, fit.par, ops.fit_map(["F0"]), np.zeros((1, 1, 1)))
    with pytest.raises(ValueError, match="BINARY ELL1 has no ECC"):
        problem(c, ["F0", "ECC"])


# ------------------------------------------------------------------ 8. the driver: .tim + .par -> fitted .par
def write_par_and_tim(tmp_path, prob, seed=8):
    """A flagged .par of the injection model and a .tim whose ToAs follow full(p_true): every arrival time moved onto
    an integer phase of that model (two Newton steps on the host twin's absolute phase), plus the ToA's noise."""
    from crimp_amd.binarymodels import binary_delay_host
    tm, keys = O.R.plain(prob["tm"]), prob["keys"]
    truth = O.full_model(tm, keys, prob["p_true"])
    orbit = {k: v for k, v in truth.items() if k in O.ORBITAL or k == "BINARY"}
    f0, f1, f2, pep = (float(truth[k]) for k in ("F0", "F1", "F2", "PEPOCH"))

    def phase(t):
        dt = (t - pep) * 86400.0 - binary_delay_host(t, orbit)
        return dt * (f0 + dt * (f1 / 2 + dt * f2 / 6))
    rng = np.random.default_rng(seed)
    t = prob["t"].copy()
    for _ in range(2):
        ph = phase(t)
        t = t - (ph - np.round(ph)) / f0 / 86400.0
    err_s = prob["yerr"] / f0
    t = t + err_s * rng.standard_normal(t.size) / 86400.0
    par = tmp_path / "psr.par"
    lines = ["PSR J0000+0000"]
    for k, v in tm.items():
        if k.startswith("F") and k[1:].isdigit() and int(k[1:]) > 2:
            continue
        lines.append("%s %s%s" % (k, v if k == "BINARY" else repr(float(v)), " 1" if k in keys else ""))
    par.write_text("\n".join(lines) + "\n")
    tim = tmp_path / "psr.tim"
    tim.write_text("FORMAT 1\n" + "".join("tpl.txt 700 %.17g %.6f @ -i Xray\n" % (x, e * 1e6) for x, e in zip(t, err_s)))
    return str(par), str(tim)


@pytest.mark.gpu
def test_driver_fits_a_tim_file_and_writes_the_par(gpu, tmp_path, monkeypatch):
    from crimp_amd import fit_orbit as F
    from crimp_amd.binarymodels import binary_params
    from crimp_amd.readtimingmodel import ReadTimingModel
    prob = O.injection_problem("bt")
    par, tim = write_par_and_tim(tmp_path, prob)
    new = str(tmp_path / "new.par")
    out = F.fit_orbit_toas(tim, par, new, plot=False)
    assert sorted(out["keys"]) == sorted(prob["keys"]) and out["residuals"].shape == (O.INJECTION_NTOA,)
    order = [prob["keys"].index(k) for k in out["keys"]]          # the .par's order of the keys, not the dict's
    truth, sig = prob["p_true"][order], prob["sigma"][order]
    unc = np.array([out["uncertainties"][k] for k in out["keys"]])
    pull = (out["p"] - truth) / unc
    print("driver pull", np.round(pull, 2), "sigma ratio", np.round(unc / sig, 3))
    assert np.all(np.abs(pull) < 5.0)
    assert np.all((unc > 0.5 * sig) & (unc < 2 * sig))
    # the written .par is the full model: BINARY untouched, every free key par - p, the rest as it was
    text = open(new).read()
    assert "BINARY BT\n" in text
    again = ReadTimingModel(new).readfulltimingmodel()[0]
    before = ReadTimingModel(par).readfulltimingmodel()[0]
    for k, d in zip(out["keys"], out["p"]):
        assert float(again[k]) == float(before[k]) - d, k
    assert binary_params(again)["om"] == binary_params(before)["om"] - out["p"][out["keys"].index("OM")]
    # the command line does the same and appends the statistics
    monkeypatch.setattr(F, "plot_residuals", lambda *a, **k: None)
    cli = str(tmp_path / "cli.par")
    F.main([tim, par, cli])
    body = open(cli).read()
    assert "CHI2R" in body and "NTOA" in body
    values = ReadTimingModel(cli).readfulltimingmodel()[0]
    assert all(float(values[k]) == float(again[k]) for k in out["keys"])
