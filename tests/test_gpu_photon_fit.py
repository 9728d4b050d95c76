"""Photon-domain timing fits on the device (csrc/photon_fit.h): crimp_photon_nll against the NumPy reference
(tests/photon_reference.py) at every size around the tile, its independence of the launch shape, invalid models,
what a vector means, crimp_photon_mcmc's bookkeeping, determinism and posterior, the argument errors and the
fitphotons script end to end.

The reference is computed once per model at the largest size: delta of a photon does not depend on how many photons
there are, so every smaller size is a prefix of it and every prefix sum a cumulative sum."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

import photon_reference as R
from conftest import gpath
from test_photon_fit_host import (POSTERIOR_KEYS, POSTERIOR_THETA, check_posterior, posterior_problem)

TOL_MU = 1e-9  # cycles: the project's calcphase bound
P = 64
MODELS = ("a", "b", "c", "d", "wave")
WAVE_KEYS = ["F0", "GLF0D_1", "WAVE1_A"]


def tile():
    from crimp_amd import _native as N
    return N.photon_tile()


def sizes():
    T = tile()
    return (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)


@pytest.fixture(scope="module")
def templates():
    from crimp_amd.readPPtemplate import readPPtemplate
    with open(gpath("cauchy_vm_theta.json")) as fh:
        cv = json.load(fh)
    cv = {k: v for k, v in cv.items() if k not in ("ampShift", "phShift")}
    k16 = {"model": "fourier", "norm": 3.0}
    for j in range(1, 17):
        k16["amp_%d" % j], k16["ph_%d" % j] = 1.0 / (j + 1) ** 1.5, 0.37 * j * j
    return {"1e2259": readPPtemplate(gpath("1e2259_template.txt")),
            "k1": {"model": "fourier", "norm": 2.0, "amp_1": 1.2, "ph_1": 0.7},
            "k16": k16,
            "cauchy": dict(cv, model="cauchy"),
            "vonmises": dict(cv, model="vonmises")}


def model_case(name):
    """(flagged model, admitted free keys) of a parity model."""
    if name == "wave":
        with open(gpath("timing_model_dict.json")) as fh:
            return R.flagged(json.load(fh), WAVE_KEYS), list(WAVE_KEYS)
    with open(gpath("fittoas.json")) as fh:
        c = json.load(fh)["cases"][name]
    return c["model"], [k for k in c["keys"] if not k.startswith(("GLEP_", "GLTD_"))]


@pytest.fixture(scope="module")
def parity(gpu):
    """Per model: photon times, the device-folded x, 64 vectors with PHOFF last and the reference's delta [P, nmax]."""
    from crimp_amd import ops
    out = {}
    nmax = sizes()[-1]
    for name in MODELS:
        par, keys = model_case(name)
        rng = np.random.default_rng(sum(map(ord, name)))
        pep = par["PEPOCH"]["value"]
        t = np.sort(pep + rng.uniform(-1.0, 8.0, nmax))
        x = np.ascontiguousarray(ops.calcphase(t, par)[1])
        nd = len(keys)
        # every key's largest |delta| for a unit entry; entries then draw up to 300 / ndim cycles each, at
        # magnitudes spread over six decades
        unit = np.array([np.max(np.abs(R.delta(t, copy.deepcopy(par), np.eye(nd)[k], keys))) for k in range(nd)])
        vec = rng.uniform(-1, 1, (P, nd)) * (300.0 / nd) / unit * 10.0 ** rng.uniform(-6, 0, (P, 1))
        vec = np.concatenate([vec, rng.uniform(-0.5, 0.5, (P, 1))], axis=1)
        ref = np.stack([R.delta(t, copy.deepcopy(par), v[:nd], keys) for v in vec])
        assert 1.0 < np.max(np.abs(ref)) <= 1e3
        out[name] = (par, keys, t, x, vec, ref)
    return out


def reference_sums(theta, x, ref_delta, vec, phoff):
    """(ln(m / norm) [P, n], |d ln m / du| [P, n]) of the reference at u = x - delta - PHOFF."""
    u = x[None, :] - ref_delta - (vec[:, -1:] if phoff else 0.0)
    m, dm = R.template_value(theta, u)
    assert np.all(m > 0)
    return np.log(m / float(R._value(theta["norm"]))), np.abs(dm / m)


# ------------------------------------------------------------------ 1, 2. parity and shape independence
@pytest.mark.gpu
@pytest.mark.parametrize("name", MODELS)
def test_nll_and_delta_match_reference_at_every_size_and_shape(gpu, parity, templates, name):
    from crimp_amd.fit_photons import PhotonFit
    par, keys, t, x, vec, ref = parity[name]
    worst_d = worst_n = 0.0
    for tname, theta in templates.items():
        for phoff in (False, True):
            v = np.ascontiguousarray(vec if phoff else vec[:, :-1])
            ln, slope = reference_sums(theta, x, ref, vec, phoff)
            want = -np.cumsum(ln, axis=1)
            bound = np.cumsum(slope, axis=1) * TOL_MU + 1e-12 * np.cumsum(1.0 + np.abs(ln), axis=1)
            for n in sizes():
                fit = PhotonFit(t[:n], copy.deepcopy(par), theta, keys=keys, phoff=phoff)
                fit.x = np.ascontiguousarray(x[:n])  # the array the reference was given
                nll = fit.nll(v)
                if tname == "1e2259":
                    d = fit.delta(v)
                    err = np.max(np.abs(d - ref[:, :n]))
                    worst_d = max(worst_d, err)
                    assert err <= TOL_MU, (name, n, phoff, err)
                ratio = np.max(np.abs(nll - want[:, n - 1]) / bound[:, n - 1])
                worst_n = max(worst_n, ratio)
                assert ratio <= 1.0, (name, tname, phoff, n, ratio)
                # independent of P and of how the vectors fall into blocks
                np.testing.assert_array_equal(fit.nll(v[:1]), nll[:1])
                np.testing.assert_array_equal(fit.nll(v[:5]), nll[:5])
                np.testing.assert_array_equal(fit.nll(v[3:12]), nll[3:12])
    print(name, "max |delta - ref| %.3g cycles" % worst_d, "max |nll - ref| / bound %.3g" % worst_n)


# ------------------------------------------------------------------ 3. invalid model
@pytest.mark.gpu
def test_a_vector_that_puts_a_photon_where_the_model_is_not_positive_is_inf(gpu, parity):
    from crimp_amd.fit_photons import PhotonFit
    par, keys, t, x, vec, ref = parity["a"]
    theta = {"model": "fourier", "norm": 1.0, "amp_1": 1.5, "ph_1": 0.2}  # m <= 0 over ~27 % of the cycle
    n = 5
    fit = PhotonFit(t[:n], copy.deepcopy(par), theta, keys=keys, phoff=True)
    fit.x = np.ascontiguousarray(x[:n])
    nll = fit.nll(vec)
    u = x[None, :n] - ref[:, :n] - vec[:, -1:]
    m, dm = R.template_value(theta, u)
    clear = np.min(np.abs(m), axis=1) > 1e-6  # not within the delta bound of the zero crossing
    bad = np.any(m <= 0, axis=1)
    assert (bad & clear).sum() >= 5 and (~bad & clear).sum() >= 5
    assert np.all(np.isposinf(nll[bad & clear]))
    ok = ~bad & clear
    ln = np.log(m[ok])
    bound = np.sum(np.abs(dm[ok] / m[ok]), axis=1) * TOL_MU + 1e-12 * np.sum(1.0 + np.abs(ln), axis=1)
    assert np.all(np.isfinite(nll[ok])) and np.all(np.abs(nll[ok] + ln.sum(axis=1)) <= bound)


# ------------------------------------------------------------------ 4. what a vector means
@pytest.mark.gpu
def test_nll_of_p_is_the_likelihood_of_the_photons_refolded_under_full_p(gpu, templates):
    from crimp_amd.fit_photons import PhotonFit
    with open(gpath("timing_model_dict.json")) as fh:
        plain = json.load(fh)
    keys = ["F0", "F1", "GLF0_1", "WAVE1_B"]
    par = R.flagged(plain, keys)
    rng = np.random.default_rng(8)
    t = np.sort(plain["PEPOCH"] + rng.uniform(-1.0, 8.0, 3 * tile() + 17))
    theta = templates["1e2259"]
    fit = PhotonFit(t, copy.deepcopy(par), theta, keys=keys)
    for p in (np.array([2e-6, 3e-15, 3e-8, 0.004]), np.array([-1e-7, 1e-16, -2e-9, -0.0003])):
        full = {k: R._value(v) for k, v in fit.full(p).items()}
        refit = PhotonFit(t, R.flagged(full, keys), theta, keys=keys)
        a, b = fit.nll(p), refit.nll(np.zeros(4))
        _, _, slope = R.terms(t, fit.x, copy.deepcopy(par), theta, p, keys)
        tol = np.sum(slope) * 3e-9  # two calcphase folds plus delta
        print("nll(p) %.9f refolded %.9f tol %.3g max |delta| %.3g" % (a, b, tol, np.max(np.abs(fit.delta(p)))))
        assert np.max(np.abs(fit.delta(p))) > 0.01
        assert abs(a - b) <= tol


# ------------------------------------------------------------------ 5. the sampler
@pytest.fixture(scope="module")
def drawn(gpu):
    """The host-drawn data set of the CPU test (seed 200): the whole of it with its MLE and sigma, and its first
    3 T + 17 photons with theirs."""
    from crimp_amd.fit_photons import PhotonFit
    t, x, par, _, _, sol, sig = posterior_problem(200)
    n = 3 * tile() + 17
    assert t.size >= n
    head = PhotonFit(t[:n], copy.deepcopy(par), POSTERIOR_THETA, keys=POSTERIOR_KEYS)
    hsol, hsig, _ = R.mle(lambda p: R.nll(t[:n], head.x, copy.deepcopy(par), POSTERIOR_THETA, p, POSTERIOR_KEYS),
                          sol, sig)
    return PhotonFit(t, copy.deepcopy(par), POSTERIOR_THETA, keys=POSTERIOR_KEYS), sol, sig, head, hsol, hsig


def run_chain(fit, p0, lo, hi, steps, seed):
    from crimp_amd import ops
    return ops.photon_mcmc(fit.t, fit.x, fit.par, fit.map, fit.tpl, fit.norm, p0, lo, hi, steps, seed,
                           phoff=fit.phoff)


@pytest.mark.gpu
@pytest.mark.parametrize("W, steps", [(4, 50), (32, 200)])
def test_sampler_bookkeeping(gpu, drawn, W, steps):
    _, _, _, fit, sol, sig = drawn
    rng = np.random.default_rng(W)
    p0 = sol + rng.uniform(-3, 3, (W, 2)) * sig
    lo, hi = sol - 4 * sig, sol + 4 * sig  # tight enough that proposals leave the box
    chain, logprob, accepted = run_chain(fit, p0, lo, hi, steps, 11)
    # every stored log-probability is minus the likelihood call's value at the stored position, bit for bit
    np.testing.assert_array_equal(logprob.reshape(-1), -fit.nll(chain.reshape(-1, 2)))
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


@pytest.mark.gpu
def test_sampler_determinism(gpu, drawn):
    _, _, _, fit, sol, sig = drawn
    rng = np.random.default_rng(3)
    p0 = sol + rng.uniform(-3, 3, (8, 2)) * sig
    lo, hi = sol - 50 * sig, sol + 50 * sig
    first, again, other = (run_chain(fit, p0, lo, hi, 30, seed) for seed in (7, 7, 8))
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    assert np.any(other[0] != first[0])


@pytest.mark.gpu
def test_posterior_of_the_drawn_photons(gpu, drawn):
    fit, sol, sig, _, _, _ = drawn
    rng = np.random.default_rng(1)
    p0 = sol + rng.uniform(-5, 5, (32, 2)) * sig
    chain, _, accepted = run_chain(fit, p0, sol - 1e3 * sig, sol + 1e3 * sig, 3000, 2024)
    check_posterior(chain, accepted, 500, sol, sig)


# ------------------------------------------------------------------ 6. argument errors
SENTINEL = -7.25


@pytest.mark.gpu
def test_argument_errors_leave_the_outputs_untouched(gpu, parity, templates):
    from crimp_amd import _native as N
    from crimp_amd import ops
    from crimp_amd.simulatemodulatedlc import template_parts
    L = N.load()
    par, keys, t, x, vec, _ = parity["b"]
    t, x = np.ascontiguousarray(t[:9]), np.ascontiguousarray(x[:9])
    model, norm, amps, locs, wids = template_parts(templates["1e2259"])
    tpl = ops.make_template(model, amps, locs, wids)
    good = ops._modeltm(par)
    W, steps = 8, 3
    nll, delta = np.full(2, SENTINEL), np.full((2, 9), SENTINEL)
    chain, lp, acc = np.full((steps, W, 4), SENTINEL), np.full((steps, W), SENTINEL), np.full(W, -7, dtype=np.int64)
    pv = np.zeros((W, 4))
    lo, hi = np.full(4, -1.0), np.full(4, 1.0)

    def ptr(a):
        return ctypes.c_void_p(a.ctypes.data)

    def both(want, n=9, m=good, fmap=None, template=tpl, phoff=0, nrm=norm):
        fmap = ops.fit_map(["F0", "F1"]) if fmap is None else fmap
        rc = L.crimp_photon_nll(ptr(t), ptr(x), n, ctypes.byref(m), ctypes.byref(fmap), ctypes.byref(template), nrm,
                                phoff, ptr(pv), 2, ptr(nll), ptr(delta), 0, None)
        assert rc == -1 and L.crimp_last_error().decode() == want, (want, rc, L.crimp_last_error())
        rc = L.crimp_photon_mcmc(ptr(t), ptr(x), n, ctypes.byref(m), ctypes.byref(fmap), ctypes.byref(template), nrm,
                                 phoff, ptr(pv), ptr(lo), ptr(hi), W, steps, 5, ptr(chain), ptr(lp), ptr(acc), 0,
                                 None)
        assert rc == -1 and L.crimp_last_error().decode() == want, (want, rc, L.crimp_last_error())
        assert np.all(nll == SENTINEL) and np.all(delta == SENTINEL) and np.all(chain == SENTINEL)
        assert np.all(lp == SENTINEL) and np.all(acc == -7)

    both("n < 1", n=0)
    both("slot names a glitch outside the model", fmap=ops.fit_map(["F0", "GLF0_3"]))
    both("slot names a wave harmonic outside the model", fmap=ops.fit_map(["WAVE9_A"]))
    bad_f = ops.fit_map(["F0"])
    bad_f.slot[0].index = 13
    both("slot names an F term outside F0..F12", fmap=bad_f)
    both("GLEP is not fitted to photons", fmap=ops.fit_map(["F0", "GLEP_1"]))
    both("GLTD is not fitted to photons", fmap=ops.fit_map(["GLTD_1", "F0"]))
    zero = ops.fit_map(["F0"])
    zero.ndim = 0
    both("ndim must be 1..CRIMP_FIT_MAX_DIM - phoff", fmap=zero)
    both("ndim must be 1..CRIMP_FIT_MAX_DIM - phoff", fmap=ops.fit_map(["F%d" % (i % 13) for i in range(32)]), phoff=1)
    orbit = N.TimingModel.from_buffer_copy(good)
    orbit.binary = N.BINARY_BT
    both("binary models are not fitted yet", m=orbit)
    empty = N.Template.from_buffer_copy(tpl)
    empty.ncomp = 0
    both("ncomp out of range", template=empty)
    unknown = N.Template.from_buffer_copy(tpl)
    unknown.model = 3
    both("unknown template model", template=unknown)
    both("norm must be positive", nrm=0.0)
    with pytest.raises(ValueError, match="binary models are not fitted yet"):
        ops.photon_nll(t, x, orbit, ops.fit_map(["F0"]), tpl, norm, np.zeros((1, 1)))
    # and the same arguments, valid, compute
    rc = L.crimp_photon_nll(ptr(t), ptr(x), 9, ctypes.byref(good), ctypes.byref(ops.fit_map(["F0", "F1"])),
                            ctypes.byref(tpl), norm, 0, ptr(pv), 2, ptr(nll), ptr(delta), 0, None)
    assert rc == 0 and np.all(np.isfinite(nll)) and not delta.any()


# ------------------------------------------------------------------ 7. end to end
@pytest.mark.gpu
def test_fitphotons_recovers_the_simulated_f0(gpu, tmp_path, templates):
    from crimp_amd import fit_photons as FP
    from crimp_amd.readtimingmodel import ReadTimingModel
    from crimp_amd.simulatemodulatedlc import simulate_events, write_eventfile
    theta = templates["1e2259"]
    with open(gpath("1e2259.par")) as fh:
        lines = fh.read().splitlines()
    par_path = tmp_path / "start.par"
    start = 58400.0
    # F0 flagged, and PEPOCH in the middle of the data so that F0 and PHOFF are nearly uncorrelated
    lines = ["PEPOCH %r" % (start + 1.0) if ln.split()[:1] == ["PEPOCH"] else ln for ln in lines]
    par_path.write_text("\n".join(ln + " 1" if ln.split()[:1] == ["F0"] else ln for ln in lines) + "\n")
    values, _, both = ReadTimingModel(str(par_path)).readfulltimingmodel()
    assert both["F0"]["flag"] == 1 and values["PEPOCH"] == start + 1.0
    # over 2 days, observed in three 1500 s windows: ~77000 photons
    gti = np.array([[start + d, start + d + 1500.0 / 86400.0] for d in (0.0, 0.9, 2.0 - 1500.0 / 86400.0)])
    ev = simulate_events(str(par_path), theta, start, start + 2.0, gti=gti, seed=17)
    evt = write_eventfile(str(tmp_path / "sim.fits"), ev["time"], gti=gti)
    t = np.asarray(ev["time"], dtype=float)
    fit = FP.PhotonFit(t, both, theta, phoff=True)
    assert fit.keys == ["F0", "PHOFF"]

    def f(p):
        return R.nll(t, fit.x, copy.deepcopy(both), theta, p, ["F0"], phoff=True)

    span = 2.0 * 86400.0
    cov = np.linalg.inv(R.hessian(f, np.zeros(2), 0.3 * np.array([0.05 / span, 0.005])))
    sig = np.sqrt(np.diag(cov))
    cov = np.linalg.inv(R.hessian(f, np.zeros(2), 0.3 * sig))
    sig = np.sqrt(np.diag(cov))
    yaml_path = tmp_path / "prior.yaml"
    yaml_path.write_text("F0: [%r, %r]\nPHOFF: [%r, %r]\n" % tuple(float(v) for v in (-20 * sig[0], 20 * sig[0], -20 * sig[1], 20 * sig[1])))
    new_par = tmp_path / "new.par"
    FP.main([evt, str(par_path), gpath("1e2259_template.txt"), str(new_par), "-mc", "-po", "-iy", str(yaml_path),
             "-st", "400", "-bu", "150", "-wa", "16", "-bf", "median"])
    out = new_par.read_text()
    row = [ln.split() for ln in out.splitlines() if ln.split()[:1] == ["F0"]][0]
    f0, unc = float(row[1]), float(row[3])
    print("photons", t.size, "sigma(F0) %.3g" % sig[0], "offset / sigma %.3g" % ((f0 - values["F0"]) / sig[0]),
          "written uncertainty / sigma %.3g" % (unc / sig[0]))
    assert abs(f0 - values["F0"]) <= 5 * sig[0]
    assert 0.5 <= unc / sig[0] <= 2.0
    keys = {ln.split()[0] for ln in out.splitlines() if ln.split()}
    assert {"START", "FINISH", "NTOA"} <= keys
    ntoa = [ln.split() for ln in out.splitlines() if ln.split()[:1] == ["NTOA"]][0]
    assert int(ntoa[1]) == t.size
