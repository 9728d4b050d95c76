"""Photon-domain timing fits on the CPU: the host plan (csrc/photon_fit_plan.h) through its stand-alone check program,
the NumPy reference (tests/photon_reference.py) against high-precision folds, PhotonFit's refusals, the PHOFF key of
the YAML prior, the packaging lines, and the posterior bounds of the sampler's move on the reference likelihood.

`make -C crimp_amd/csrc photon-plan-check` builds photon_fit_plan_check.cpp with the host compiler under
-fsanitize=address,undefined; every plan case below is one run of that program (no GPU, no preloaded library)."""
import copy
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import photon_reference as R
from conftest import gpath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crimp_amd", "csrc")
SLOT_F, SLOT_GLITCH, SLOT_WAVE = 0, 1, 2
GLITCH_FIELDS = ("GLEP", "GLPH", "GLF0", "GLF1", "GLF2", "GLF0D", "GLTD")


@pytest.fixture(scope="module")
def plan_check():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-s", "-B", "-C", CSRC, "photon-plan-check"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(CSRC, "build", "photon_plan_check")


@pytest.fixture(scope="module")
def wave_model():
    with open(gpath("timing_model_dict.json")) as fh:
        return json.load(fh)


def slots(keys):
    out = []
    for k in keys:
        if k[0] == "F":
            out.append((SLOT_F, int(k[1:]), 0))
        elif k.startswith("GL"):
            name, j = k.split("_")
            out.append((SLOT_GLITCH, int(j) - 1, GLITCH_FIELDS.index(name)))
        else:
            name, s = k.split("_")
            out.append((SLOT_WAVE, int(name[4:]) - 1, "AB".index(s)))
    return out


def run_plan(exe, n, P, phoff, model, slot_list, vec, binary=0, ndim=None):
    ngl = sum(1 for k in model if k.startswith("GLEP_"))
    nwv = max(sum(1 for k in model if k.startswith("WAVE")) - 2, 0)
    words = [n, P, phoff, repr(model["PEPOCH"]), repr(model["F0"]), binary, ngl, nwv,
             repr(model.get("WAVEEPOCH", 0.0)), repr(model.get("WAVE_OM", 0.0))]
    for j in range(1, ngl + 1):
        words += [repr(float(model.get("%s_%d" % (f, j), 0.0))) for f in GLITCH_FIELDS]
    for j in range(1, nwv + 1):
        words += [repr(model["WAVE%d" % j]["A"]), repr(model["WAVE%d" % j]["B"])]
    words.append(len(slot_list) if ndim is None else ndim)
    for s in slot_list:
        words += list(s)
    words += [repr(float(v)) for v in vec]
    r = subprocess.run([exe], input=" ".join(str(w) for w in words) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    out = {}
    for line in r.stdout.splitlines():
        key, *vals = line.split()
        out.setdefault(key, []).append(vals)
    return out


def one(plan, key):
    return plan[key][0][0]


# ------------------------------------------------------------------ 1. the host plan
def test_plan_tile_and_group_counts(plan_check, wave_model):
    T = int(one(run_plan(plan_check, 1, 1, 0, wave_model, slots(["F0"]), [0.0]), "tile"))
    assert T >= 64 and T % 64 == 0
    for n in (1, T - 1, T, T + 1, 3 * T + 17):
        for P in (1, 4, 5, 8, 9, 64):
            plan = run_plan(plan_check, n, P, 0, wave_model, slots(["F0"]), [0.0])
            waves = int(one(plan, "waves"))
            assert int(one(plan, "tiles")) == -(-n // T)
            assert int(one(plan, "groups")) == -(-P // waves)
            assert int(one(plan, "partials")) == P * -(-n // T)
    assert run_plan(plan_check, 0, 1, 0, wave_model, slots(["F0"]), [0.0])["error"] == [["n", "<", "1"]]
    assert " ".join(run_plan(plan_check, 5, 0, 0, wave_model, slots(["F0"]), [0.0])["error"][0]) == "P out of range"
    # the 32-bit limits it declines: more than 2^31 partial sums, more than 65535 groups of vectors
    big = run_plan(plan_check, 1 << 40, -(-(1 << 31) // ((1 << 40) // T)) + 1, 0, wave_model, slots(["F0"]), [0.0])
    assert " ".join(big["error"][0]) == "too many partial sums for one launch"
    assert " ".join(run_plan(plan_check, 5, 65535 * 8 + 1, 0, wave_model, slots(["F0"]), [0.0])["error"][0]) == \
        "P out of range"


def test_plan_refused_slots(plan_check, wave_model):
    def err(slot_list, phoff=0, binary=0, ndim=None):
        vec = [0.0] * (len(slot_list) + phoff)
        return " ".join(run_plan(plan_check, 10, 1, phoff, wave_model, slot_list, vec, binary, ndim)["error"][0])

    assert err(slots(["F0", "GLEP_1"])) == "GLEP is not fitted to photons"
    assert err(slots(["GLTD_1"])) == "GLTD is not fitted to photons"
    assert err(slots(["GLF0_3"])) == "slot names a glitch outside the model"
    assert err(slots(["WAVE4_A"])) == "slot names a wave harmonic outside the model"
    assert err([(SLOT_F, 13, 0)]) == "slot names an F term outside F0..F12"
    assert err([(SLOT_GLITCH, 0, 7)]) == "slot names a glitch field outside the model"
    assert err([(SLOT_WAVE, 0, 2)]) == "slot names a wave field outside the model"
    assert err([(3, 0, 0)]) == "unknown slot kind"
    assert err(slots(["F0"]), binary=1) == "binary models are not fitted yet"
    assert err([], ndim=0) == "ndim must be 1..CRIMP_FIT_MAX_DIM - phoff"
    assert err(slots(["F%d" % (i % 13) for i in range(32)]), phoff=1) == "ndim must be 1..CRIMP_FIT_MAX_DIM - phoff"
    assert "error" not in run_plan(plan_check, 10, 1, 0, wave_model, slots(["F%d" % (i % 13) for i in range(32)]),
                                   [0.0] * 32)
    assert "error" not in run_plan(plan_check, 10, 1, 1, wave_model, slots(["F%d" % (i % 13) for i in range(31)]),
                                   [0.0] * 32)


def test_plan_model_keeps_shapes_and_combines_the_wave_coefficients(plan_check, wave_model):
    keys = ["F0", "GLF0D_1", "WAVE1_A", "WAVE3_B"]
    vec = [3e-8, 1.5e-9, 0.004, -0.0007, 0.25]
    plan = run_plan(plan_check, 100, 3, 1, wave_model, slots(keys), vec)
    assert one(plan, "amplitudes_zero") == "1" and one(plan, "D") == "5" and one(plan, "f0_param") == "0"
    assert int(one(plan, "parts")) == 7 and int(one(plan, "nterms")) == 1 and one(plan, "use_waves") == "1"
    assert float.fromhex(one(plan, "fit_pepoch")) == wave_model["PEPOCH"]
    # glitches up to the last free one, GLEP and GLTD kept
    assert int(one(plan, "fit_n_glitch")) == 1
    assert [float.fromhex(v) for v in plan["glitch"][0][1:]] == [wave_model["GLEP_1"], wave_model["GLTD_1"]]
    assert [float.fromhex(v) for v in plan["wave_shape"][0]] == [wave_model["WAVEEPOCH"], wave_model["WAVE_OM"]]
    f0, df0 = wave_model["F0"], vec[0]
    da = {("WAVE1", "A"): vec[2], ("WAVE3", "B"): vec[3]}
    assert len(plan["wave_coef"]) == 3
    for row in plan["wave_coef"]:
        j = int(row[0]) + 1
        for s, got in zip("AB", row[1:]):
            want = (f0 - df0) * da.get(("WAVE%d" % j, s), 0.0) + df0 * wave_model["WAVE%d" % j][s]
            assert abs(float.fromhex(got) - want) <= 4e-16 * abs(want), (j, s)
    # a glitch amplitude of the second glitch: both glitches are evaluated, the first with zero amplitudes
    plan = run_plan(plan_check, 100, 3, 0, wave_model, slots(["F2", "GLPH_2"]), [0.0, 0.0])
    assert int(one(plan, "fit_n_glitch")) == 2 and int(one(plan, "nterms")) == 3 and int(one(plan, "parts")) == 3


def test_plan_skips_the_waves_without_f0_or_a_wave_key(plan_check, wave_model):
    plan = run_plan(plan_check, 100, 3, 0, wave_model, slots(["F1", "GLF0_1"]), [1e-16, 1e-9])
    assert one(plan, "use_waves") == "0" and int(one(plan, "fit_n_wave")) == 0 and int(one(plan, "parts")) == 3
    assert "wave_coef" not in plan and one(plan, "f0_param") == "-1"
    plan = run_plan(plan_check, 100, 3, 0, wave_model, slots(["WAVE2_B"]), [1e-3])
    assert one(plan, "use_waves") == "1" and int(one(plan, "parts")) == 4
    plan = run_plan(plan_check, 100, 3, 0, wave_model, slots(["F0"]), [1e-9])
    assert one(plan, "use_waves") == "1" and int(one(plan, "parts")) == 5


# ------------------------------------------------------------------ 2. the reference's delta against 60-digit folds
def test_reference_delta_equals_the_difference_of_two_high_precision_folds(wave_model):
    pytest.importorskip("mpmath")
    import phase_reference as PR
    from crimp_amd.utilities_fittoas import inject_free_params
    rng = np.random.default_rng(5)
    t = np.sort(rng.uniform(58139.0, 58147.0, 8))  # |Phi| <= 1e6 cycles; both glitches and the recovery inside
    assert np.max(np.abs(R.S.total_phase(t, wave_model))) <= 1e6
    # every entry below half its base value (or the base is 0), so that snapping makes par - p exact in fp64: the
    # contract's full(p) is then the same model in both folds, not one that differs by ulp(F0) * dt ~ 1e-11 cycles
    cases = [(["F0", "F1", "GLF0_1", "WAVE1_B"], [2e-5, 3e-15, 3e-8, 0.004]),
             (["F0", "GLF0D_1", "WAVE1_A"], [-4e-5, 5e-9, -0.003]),
             (["GLPH_2", "GLF1_1", "GLF2_1", "WAVE2_A", "WAVE3_B"], [0.01, 1e-15, 3e-24, 0.001, 0.0002]),
             (["F2", "F3", "GLF1_2"], [4e-24, 5e-32, 1e-15])]

    def base_value(k):
        return wave_model[k.rsplit("_", 1)[0]][k[-1]] if k.startswith("WAVE") else wave_model[k]

    def snap(k, p):
        from fractions import Fraction
        base = base_value(k)
        q = base - (base - p)
        assert Fraction(base) - Fraction(q) == Fraction(base - q), k
        return q

    for keys, pvec in cases:
        pvec = [snap(k, p) for k, p in zip(keys, pvec)]
        par = R.flagged(wave_model, keys)
        got = R.delta(t, copy.deepcopy(par), np.array(pvec), keys)
        _, full = inject_free_params(copy.deepcopy(par), np.array(pvec), keys)
        full = {k: (v["value"] if isinstance(v, dict) and "value" in v else v) for k, v in full.items()}
        a, b = PR.phase_mp(wave_model, t)["total"][0], PR.phase_mp(full, t)["total"][0]
        want = np.array([float(x - y) for x, y in zip(a, b)])
        print(keys, "max |delta| %.3g" % np.max(np.abs(want)), "max err %.3g" % np.max(np.abs(got - want)))
        assert np.max(np.abs(want)) > 1e-8
        assert np.max(np.abs(got - want)) <= 1e-12


# ------------------------------------------------------------------ 3. PhotonFit's refusals, YAML, packaging
def test_photonfit_refusals(wave_model):
    from crimp_amd.fit_photons import PhotonFit, check_photon_keys
    theta = {"model": "fourier", "norm": 1.0, "amp_1": 0.5, "ph_1": 0.3}
    t = np.array([58141.0, 58143.0])
    for key in ("GLEP_1", "GLTD_1"):
        with pytest.raises(ValueError, match=key):
            PhotonFit(t, R.flagged(wave_model, ["F0", key]), theta)
        with pytest.raises(ValueError, match=key):
            PhotonFit(t, R.flagged(wave_model, ["F0"]), theta, keys=["F0", key])
    for key in ("PEPOCH", "WAVEEPOCH", "WAVE_OM", "PB", "F13"):
        with pytest.raises(ValueError, match=key):
            check_photon_keys([key])
    check_photon_keys(["F0", "F12", "GLPH_1", "GLF0_2", "GLF1_1", "GLF2_1", "GLF0D_1", "WAVE1_A", "WAVE12_B"])
    binary = R.flagged(wave_model, ["F0"])
    binary.update({"BINARY": {"value": "BT", "flag": 0}, "PB": {"value": 1.5, "flag": 0},
                   "A1": {"value": 2.0, "flag": 0}, "T0": {"value": 58140.0, "flag": 0},
                   "ECC": {"value": 0.1, "flag": 0}, "OM": {"value": 10.0, "flag": 0}})
    with pytest.raises(ValueError) as e:
        PhotonFit(t, binary, theta)
    assert str(e.value) == "binary models are not fitted yet"


def test_phoff_is_a_legal_yaml_key(tmp_path):
    from crimp_amd.fit_toas import prior_box
    from crimp_amd.utilities_fittoas import initguess_prior_from_yaml, initialize_params
    path = tmp_path / "prior.yaml"
    path.write_text("F0: {low: -1.0e-8, high: 1.0e-8, guess: 0.0}\nPHOFF: {low: -0.5, high: 0.5, guess: 0.1}\n")
    prior = initguess_prior_from_yaml(str(path))
    lo, hi = prior_box(prior, ["F0", "PHOFF"])
    np.testing.assert_array_equal(lo, [-1e-8, -0.5])
    np.testing.assert_array_equal(hi, [1e-8, 0.5])
    np.testing.assert_array_equal(initialize_params(["F0", "PHOFF"], str(path)), [0.0, 0.1])


def test_fitphotons_script_is_declared():
    with open(os.path.join(ROOT, "pyproject.toml")) as fh:
        assert 'fitphotons = "crimp_amd.fit_photons:main"' in fh.read()
    with open(os.path.join(ROOT, "setup.cfg")) as fh:
        assert "fitphotons = crimp_amd.fit_photons:main" in fh.read()
    from crimp_amd.fit_photons import build_parser
    opts = {s for a in build_parser()._actions for s in a.option_strings}
    assert {"-el", "-eh", "-ts", "-te", "-iy", "-po", "-mc", "-st", "-bu", "-wa", "-ch", "-fl", "-bf"} <= opts


# ------------------------------------------------------------------ 4. the posterior bounds on the CPU
# the bounds tests/test_gpu_timing_fit.py uses for a two-parameter posterior
MEDIAN_TOL, WIDTH_TOL, ACCEPT_RANGE = 0.15, 0.08, (0.55, 0.85)
POSTERIOR_PAR = {"PEPOCH": 58000.0, "F0": 0.14328254547263483, "F1": -9.7e-15}
POSTERIOR_THETA = {"model": "fourier", "norm": 1.0, "amp_1": 0.6, "ph_1": 0.4, "amp_2": 0.25, "ph_2": -1.1}
POSTERIOR_SPAN, POSTERIOR_RATE, POSTERIOR_KEYS = 30.0, 250.0, ["F0", "F1"]


def posterior_problem(seed):
    """(t, x, par, (F0, F1) logp over [P, 2] vectors, MLE, sigma) of the host-drawn data set of one seed: ~4000
    photons over 30 days around PEPOCH under a K = 2 template."""
    rng = np.random.default_rng(seed)
    t = R.host_events(POSTERIOR_PAR, POSTERIOR_THETA, POSTERIOR_SPAN, POSTERIOR_RATE, rng)
    ph = R.S.total_phase(t, POSTERIOR_PAR)
    x = ph - np.floor(ph)
    par = R.flagged(POSTERIOR_PAR, POSTERIOR_KEYS)
    dt = (t - POSTERIOR_PAR["PEPOCH"]) * 86400.0
    basis = np.stack([dt, 0.5 * dt * dt])  # delta = p @ basis for (F0, F1)

    th = POSTERIOR_THETA

    def logp(p):  # the K = 2 Fourier likelihood written out (the chain's 24000 calls; held to R.nll below)
        a = (2.0 * np.pi) * (x[None, :] - np.atleast_2d(p) @ basis)
        m = th["norm"] + th["amp_1"] * np.cos(a + th["ph_1"]) + th["amp_2"] * np.cos(2.0 * a + th["ph_2"])
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(np.all(m > 0, axis=1), np.sum(np.log(m / th["norm"]), axis=1), -np.inf)

    def f(p):
        return R.nll(t, x, copy.deepcopy(par), POSTERIOR_THETA, p, POSTERIOR_KEYS)

    # rough scales: a quarter cycle of drift over the half span in each term
    half = 0.5 * POSTERIOR_SPAN * 86400.0
    sol, sig, _ = R.mle(f, np.zeros(2), np.array([0.05 / half, 0.1 / half ** 2]))
    return t, x, par, logp, f, sol, sig


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
    """tests/test_gpu_timing_fit.py's restatement of the move: fixed even / odd halves, each updated against the
    other as it stands."""
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
    for seed in range(4):
        t, x, par, logp, f, sol, sig = posterior_problem(200 + seed)
        rng = np.random.default_rng(300 + seed)
        probe = sol + rng.uniform(-2, 2, (3, 2)) * sig
        np.testing.assert_allclose(-logp(probe), [f(p) for p in probe], rtol=0, atol=1e-9)
        print("seed", seed, "photons", t.size, "mle / sigma", sol / sig, "sigma", sig)
        p0 = sol + rng.uniform(-5, 5, (32, 2)) * sig
        chain, acc = numpy_stretch(logp, p0, 1500, rng)
        check_posterior(chain, acc, 300, sol, sig)
