"""Host side of the photon-domain orbit fits (crimp_amd/fit_photons_orbit.py, csrc/photon_orbit_fit_plan.h) and the
definition itself: key lists and refusals, the full model's round trip through a .par, the host plan through its
stand-alone check program, the NumPy fp64 twin of DESIGN.md 5.11 (tests/photon_orbit_reference.py) against the 60-digit
fixtures, and injection and recovery on the twin. No GPU.

`make -C crimp_amd/csrc photon-orbit-plan-check` builds photon_orbit_fit_plan_check.cpp with the host compiler under
-fsanitize=address,undefined; every plan case below is one run of that program (no GPU, no preloaded library)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import orbit_fit_reference as O
import photon_orbit_reference as PO
import photon_reference as PR
from conftest import gpath
from test_orbit_fit_host import PAR_BT, PAR_ELL1, read

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crimp_amd", "csrc")
SLOT_F, SLOT_GLITCH, SLOT_WAVE, SLOT_BINARY = 0, 1, 2, 3
FIELDS = ("PB", "A1", "T0", "ECC", "OM", "OMDOT", "GAMMA", "EPS1", "EPS2", "PBDOT", "A1DOT")
BT, ELL1 = 1, 2
ORBIT_BT = {"PB": 3.2, "A1": 12.0, "T0": 57000.125, "ECC": 0.3, "OM": 350.0, "OMDOT": 12.0, "GAMMA": 0.004,
            "PBDOT": 2.5e-12, "A1DOT": 3e-13}
ORBIT_ELL1 = {"PB": 0.0839, "A1": 0.0628, "T0": 58004.96, "EPS1": 1e-5, "EPS2": -2e-5, "A1DOT": -4e-14}


# ------------------------------------------------------------------ 1. keys, refusals, the full model, packaging
def test_keys_and_refusals(tmp_path):
    from crimp_amd import fit_photons_orbit as F
    _, bt = read(tmp_path, PAR_BT)
    _, ell1 = read(tmp_path, PAR_ELL1, "e.par")
    assert F.photon_orbit_keys(bt) == ["F0", "F1", "PB", "PBDOT", "A1", "A1DOT", "T0", "ECC"]
    assert F.photon_orbit_keys(ell1) == ["F0", "PB", "A1", "A1DOT", "TASC", "EPS1", "EPS2"]
    assert F.photon_orbit_keys(bt, ["A1", "F0"]) == ["A1", "F0"]
    theta = {"model": "fourier", "norm": 1.0, "amp_1": 0.5, "ph_1": 0.3}
    t = np.array([58001.0, 58002.0])
    with pytest.raises(ValueError, match="no BINARY"):
        F.PhotonOrbitFit(t, {k: v for k, v in bt.items() if k != "BINARY"}, theta)
    bad = dict(bt)
    bad["EPS1"] = {"value": 0.0, "flag": 1}
    with pytest.raises(ValueError, match="BINARY BT has no EPS1"):
        F.PhotonOrbitFit(t, bad, theta)
    out = dict(bt)
    out["ECC"] = {"value": 1.2, "flag": 1}
    with pytest.raises(ValueError, match=r"ECC must be in \[0, 1\)"):
        F.PhotonOrbitFit(t, out, theta)
    # GLEP and GLTD stay refused with fit_photons' texts, flagged or asked for
    gl = dict(bt)
    gl.update({"GLEP_1": {"value": 58001.5, "flag": 1}, "GLF0_1": {"value": 1e-8, "flag": 0},
               "GLTD_1": {"value": 10.0, "flag": 0}})
    with pytest.raises(ValueError, match=r"GLEP_1 cannot be fitted to photons \(the phase is not linear in it\)"):
        F.PhotonOrbitFit(t, gl, theta)
    with pytest.raises(ValueError, match=r"GLTD_1 cannot be fitted to photons \(the phase is not linear in it\)"):
        F.PhotonOrbitFit(t, bt, theta, keys=["F0", "A1", "GLTD_1"])
    with pytest.raises(ValueError, match="WAVE_OM cannot be fitted to photons"):
        F.photon_orbit_keys(bt, ["PB", "WAVE_OM"])
    # the binary-free photon fit still refuses the model
    from crimp_amd.fit_photons import PhotonFit
    with pytest.raises(ValueError) as e:
        PhotonFit(t, bt, theta)
    assert str(e.value) == "binary models are not fitted yet"


def test_full_model_round_trip_through_the_par_text(tmp_path):
    from crimp_amd import fit_orbit as FO
    from crimp_amd import fit_photons_orbit as F
    from crimp_amd.binarymodels import binary_params
    path, bt = read(tmp_path, PAR_BT)
    keys = F.photon_orbit_keys(bt)
    p = np.array([1e-9, 2e-16, 1e-6, 1e-13, 1e-4, -2e-15, 1e-5, 1e-3])
    full = F.full_model(bt, np.append(p, 0.25), keys)            # a PHOFF entry past the model keys is not read
    assert full == F.full_model(bt, p, keys)
    assert full["F0"] == 17.1 - 1e-9 and full["BINARY"] == "BT" and full["PB"] == 3.2 - 1e-6
    assert full["PBDOT"] == pytest.approx((2.5e-12 - 1e-13) / 1e-12, rel=1e-15)   # back in units of 1e-12
    assert full["A1DOT"] == 3e-13 + 2e-15
    new = str(tmp_path / "new.par")
    FO.patch_orbit_par(path, new, full)
    text = open(new).read()
    assert "BINARY BT\n" in text
    lines = {ln.split()[0]: ln.split() for ln in text.splitlines() if ln.strip()}
    assert float(lines["PBDOT"][1]) == pytest.approx(2.4, rel=1e-15)
    assert float(lines["T0"][1]) == 57000.125 - 1e-5 and float(lines["F0"][1]) == 17.1 - 1e-9
    _, again = read(tmp_path, text, "again.par")
    b0, b1 = binary_params(bt), binary_params(again)
    assert b1["pbdot"] == pytest.approx(b0["pbdot"] - 1e-13, rel=1e-15) and b1["a1dot"] == b0["a1dot"] + 2e-15
    assert b1["pb"] == b0["pb"] - 1e-6 and b1["t0"] == b0["t0"] - 1e-5 and b1["ecc"] == b0["ecc"] - 1e-3
    # the corrected model read back is the model a zero vector of the new .par stands for
    assert F.full_model(again, np.zeros(len(keys)), keys)["PB"] == full["PB"]


def test_fitphotonsorbit_script_is_declared():
    with open(os.path.join(ROOT, "pyproject.toml")) as fh:
        assert 'fitphotonsorbit = "crimp_amd.fit_photons_orbit:main"' in fh.read()
    with open(os.path.join(ROOT, "setup.cfg")) as fh:
        assert "fitphotonsorbit = crimp_amd.fit_photons_orbit:main" in fh.read()
    from crimp_amd.fit_photons import build_parser as photon_parser
    from crimp_amd.fit_photons_orbit import build_parser
    opts = {s for a in build_parser()._actions for s in a.option_strings}
    assert opts == {s for a in photon_parser()._actions for s in a.option_strings}
    import crimp.fit_photons_orbit as alias
    import crimp_amd.fit_photons_orbit as mod
    assert alias is mod


# ------------------------------------------------------------------ 2. the host plan
@pytest.fixture(scope="module")
def plan_check():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-s", "-B", "-C", CSRC, "photon-orbit-plan-check"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(CSRC, "build", "photon_orbit_plan_check")


def run_plan(exe, slot_list, vec, binary=BT, orbit=None, n=10, P=1, phoff=0, ndim=None, n_glitch=0):
    orbit = dict(ORBIT_BT if binary != ELL1 else ORBIT_ELL1) if orbit is None else orbit
    words = [n, P, phoff, 58000.0, 17.1, binary, n_glitch, 0, 0.0, 0.0]
    words += [repr(float(orbit.get(f, 0.0))) for f in FIELDS]
    for _ in range(n_glitch):
        words += [58001.0, 0.0, 1e-8, 0.0, 0.0, 1e-9, 10.0]
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


def orb(name):
    return (SLOT_BINARY, FIELDS.index(name), 0)


def test_plan_of_an_admitted_map(plan_check):
    slot_list = [orb("A1"), (SLOT_F, 0, 0), orb("T0"), (SLOT_F, 1, 0), orb("PBDOT")]
    vec = [1e-4, 1e-9, 1e-5, 2e-16, 1e-13, 0.25]
    T = 1024
    plan = run_plan(plan_check, slot_list, vec, n=3 * T + 17, P=9, phoff=1)
    assert plan["tile"] == [[str(T)]] and plan["tiles"] == [["4"]] and plan["groups"] == [["2"]]
    assert plan["partials"] == [["36"]] and plan["D"] == [["6"]]
    assert plan["parts"] == [["1"]] and plan["nterms"] == [["2"]] and plan["f0_param"] == [["1"]]
    assert plan["fit_binary"] == [["0"]] and plan["orbit_kind"] == [[str(BT)]]
    # every entry keeps its place in a vector; BINARY slots carry their field
    assert [[int(x) for x in row] for row in plan["slot"]] == [[k] + list(s) for k, s in enumerate(slot_list)]
    base = {int(r[0]): float.fromhex(r[1]) for r in plan["orbit"]}
    corr = {int(r[0]): float.fromhex(r[2]) for r in plan["orbit"]}
    assert [base[k] for k in range(11)] == [ORBIT_BT.get(f, 0.0) for f in FIELDS]
    want = dict(ORBIT_BT)
    want["A1"], want["T0"], want["PBDOT"] = 12.0 - 1e-4, 57000.125 - 1e-5, 2.5e-12 - 1e-13
    assert [corr[k] for k in range(11)] == [want.get(f, 0.0) for f in FIELDS]
    # orbital keys alone: nothing of the spin model is evaluated
    plan = run_plan(plan_check, [orb("PB"), orb("ECC")], [0.0, 0.0])
    assert plan["parts"] == [["0"]] and plan["nterms"] == [["1"]] and plan["f0_param"] == [["-1"]]
    plan = run_plan(plan_check, [orb("PB"), orb("EPS1"), orb("EPS2"), (SLOT_F, 0, 0)], [0.0] * 4, binary=ELL1)
    assert plan["orbit_kind"] == [[str(ELL1)]] and "error" not in plan


def test_plan_refusals(plan_check):
    def err(slot_list, **kw):
        vec = [0.0] * (len(slot_list) + kw.get("phoff", 0))
        return " ".join(run_plan(plan_check, slot_list, vec, **kw)["error"][0])

    f0 = [(SLOT_F, 0, 0)]
    assert err(f0, binary=0) == "the model has no binary"
    assert err(f0, binary=3) == "binary must be CRIMP_BINARY_NONE, CRIMP_BINARY_BT or CRIMP_BINARY_ELL1"
    # crimp_orbit_nll's three texts for bad, duplicate and wrong-kind fields
    assert err([(SLOT_BINARY, 11, 0)]) == "slot names an orbit field outside CRIMP_ORBIT_PB..CRIMP_ORBIT_A1DOT"
    assert err([(SLOT_BINARY, -1, 0)]) == "slot names an orbit field outside CRIMP_ORBIT_PB..CRIMP_ORBIT_A1DOT"
    assert err([orb("A1"), (SLOT_F, 0, 0), orb("A1")]) == "two slots name one orbit field"
    for name in ("EPS1", "EPS2"):
        assert err([orb(name)]) == "slot names an orbit field the model's kind does not have"
    for name in ("ECC", "OM", "OMDOT", "GAMMA"):
        assert err([orb(name)], binary=ELL1) == "slot names an orbit field the model's kind does not have"
    # the base orbit by crimp_binary_delay's limits and texts
    assert err(f0, orbit=dict(ORBIT_BT, PB=0.0)) == "PB must be positive"
    assert err(f0, orbit=dict(ORBIT_BT, A1=-1.0)) == "A1 must be >= 0"
    assert err(f0, orbit=dict(ORBIT_BT, ECC=1.0)) == "ECC must be in [0, 1)"
    assert err(f0, orbit=dict(ORBIT_BT, OM="nan")) == "a binary parameter is not finite"
    assert err(f0, binary=ELL1, orbit=dict(ORBIT_ELL1, EPS1=0.8, EPS2=0.6)) == "EPS1^2 + EPS2^2 must be below 1"
    assert err(f0, orbit=dict(ORBIT_BT, A1=1e6)) == "2 pi A1 / (PB (1 - e)) must be below 1/2"
    # the photon plan's own texts stay
    assert err([(SLOT_GLITCH, 0, 0)], n_glitch=1) == "GLEP is not fitted to photons"
    assert err([(SLOT_GLITCH, 0, 6)], n_glitch=1) == "GLTD is not fitted to photons"
    assert err([(SLOT_GLITCH, 0, 2)]) == "slot names a glitch outside the model"
    assert err([(4, 0, 0)]) == "unknown slot kind"
    assert err([], ndim=0) == "ndim must be 1..CRIMP_FIT_MAX_DIM - phoff"
    assert err(f0, n=0) == "n < 1"
    assert err(f0, P=0) == "P out of range"


# ------------------------------------------------------------------ 3. the twin against the 60-digit fixtures
@pytest.fixture(scope="module")
def fixtures():
    out = {("toa",) + k: c for k, c in PO.load_toa_cases().items()}
    out.update({("golden",) + k: c for k, c in PO.load_golden().items()})
    return out


def test_fixtures_cover_the_cases(fixtures):
    assert {k[1:] for k in fixtures if k[0] == "toa"} == {(m, n) for m in O.MODELS for n in O.SIZES}
    assert {k[1:] for k in fixtures if k[0] == "golden"} == {(m, n) for m in PO.GOLDEN_MODELS for n in PO.GOLDEN_SIZES}
    for name in PO.GOLDEN_MODELS:
        c = fixtures[("golden", name, PO.GOLDEN_N)]
        assert c.vectors == PO.GOLDEN_VECTORS and c.t.size == 3 * PO.TILE + 17 and c.hi.shape == (3, PO.GOLDEN_N)
        assert np.any(np.diff(c.t) < 0) and np.all(c.A > 0)
        small = fixtures[("golden", name, PO.TILE - 1)]
        np.testing.assert_array_equal(small.t, c.t[:PO.TILE - 1])
        np.testing.assert_array_equal(small.hi, c.hi[:, :PO.TILE - 1])
        # the vectors are orbit_fit_reference's for these photons
        want = O.vectors(c.tm, c.t)[[O.VECTORS.index(v) for v in c.vectors]]
        np.testing.assert_array_equal(c.pvec, want)


@pytest.mark.parametrize("kind", ["toa", "golden"])
def test_twin_is_within_the_bound_of_the_60_digit_delta(fixtures, kind):
    """|delta_host - delta_60| <= 32 u A_i without the mean subtracted, on every case of orbit_fit.npz (150 vector
    cases, worst 0.141 of the bound: bt_full, wide) and of photon_orbit.npz; every zero vector is exact."""
    worst = (0.0, None)
    for k, c in fixtures.items():
        if k[0] != kind or (kind == "golden" and k[2] != PO.GOLDEN_N):
            continue
        d = np.array([PO.delta_host(c.tm, c.keys, p, c.t) for p in c.pvec])
        r = c.ratio(d)
        worst = max(worst, (r, k))
        assert r <= 1.0, (k, r)
        if "zero" in c.vectors:
            assert not d[c.vectors.index("zero")].any()
    print(kind, "worst ratio %.3f at %s" % worst)
    assert worst[0] > 0.01


def test_twin_marks_inadmissible_orbits_and_bad_templates(fixtures):
    c = fixtures[("toa", "bt_e07", 65)]
    p = np.zeros(len(c.keys))
    p[c.keys.index("ECC")] = float(c.tm["ECC"]) - 1.0
    assert np.all(np.isposinf(PO.delta_host(c.tm, c.keys, p, c.t)))
    theta = {"model": "fourier", "norm": 1.0, "amp_1": 0.5, "ph_1": 0.3}
    x = PO.fold_host(c.tm, c.t)
    assert np.isposinf(PO.nll_host(c.t, x, c.tm, theta, p, c.keys))
    assert np.isfinite(PO.nll_host(c.t, x, c.tm, theta, c.pvec[3], c.keys))
    assert np.isposinf(PO.nll_host(c.t, x, c.tm, dict(theta, amp_1=1.5), c.pvec[3], c.keys))
    # PHOFF shifts every phase: the same NLL as the data shifted the other way
    a = PO.nll_host(c.t, x, c.tm, theta, np.append(c.pvec[3], 0.2), c.keys, phoff=True)
    b = PO.nll_host(c.t, x - 0.2, c.tm, theta, c.pvec[3], c.keys)
    assert a == pytest.approx(b, abs=1e-12)


# ------------------------------------------------------------------ 4. injection and recovery on the twin
def test_injection_is_recoverable_on_the_twin():
    """The inputs of tests/test_gpu_photon_orbit_fit.py's recovery test: the twin's own minimum for the fixed seed has
    to lie within 3 sigma of the truth on every key (measured: -0.55, -0.54, -0.08), which leaves the device minimiser
    one sigma of its four."""
    from crimp_amd.readPPtemplate import readPPtemplate
    pr = PO.injection_problem(readPPtemplate(gpath("1e2259_template.txt")))
    assert pr["t"].size == PO.INJECTION_N and np.all(np.diff(pr["t"]) >= 0)
    span = pr["t"].max() - pr["t"].min()
    assert 9.9 * pr["truth"]["PB"] <= span <= 10.0 * pr["truth"]["PB"] + 1e-5
    np.testing.assert_allclose(np.abs(pr["p_true"]) / pr["sigma"], PO.INJECTION_OFFSET, rtol=1e-6)
    sol, sig, _ = PR.mle(pr["nll"], np.zeros(3), pr["sigma"])
    dist = (sol - pr["p_true"]) / pr["sigma"]
    print("twin minimum - truth in sigma", dist, "sigma there / sigma at the truth", sig / pr["sigma"])
    assert np.all(np.abs(dist) <= 3.0)
    assert np.all(np.abs(sig / pr["sigma"] - 1) <= 0.05)
    assert pr["nll"](sol) < pr["nll"](pr["p_true"]) < pr["nll"](np.zeros(3))
