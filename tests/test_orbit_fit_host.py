"""Host side of the orbit fits (crimp_amd/fit_orbit.py, ops.orbit_fit_map) and the definition itself: the NumPy fp64
twin of DESIGN.md 5.9 against the 60-digit fixture (tests/orbit_fit_reference.py, tests/golden/orbit_fit.npz), within
the derived bound. No GPU."""
import numpy as np
import pytest

import orbit_fit_reference as O

PAR_BT = """PSR J0000+0000
PEPOCH 58000
F0 17.1 1 1e-9
F1 -4e-13 1
BINARY BT
PB 3.2 1
A1 12.0 1
T0 57000.125 1
E 0.3 1
OM 350.0
OMDOT 12.0
GAMMA 0.004
PBDOT 2.5 1
XDOT 3e-13 1
"""

PAR_ELL1 = """PSR J0001+0000
PEPOCH 58000
F0 401.0 1
F1 -1e-15
BINARY ELL1
PB 0.0839 1
A1 0.0628 1
TASC 58004.96 1
EPS1 1e-05 1
EPS2 -2e-05 1
A1DOT -4.0e-14 1
"""


@pytest.fixture(scope="module")
def fixture():
    return O.load_fixture()


def read(tmp_path, text, name="m.par"):
    from crimp_amd.readtimingmodel import ReadTimingModel
    path = tmp_path / name
    path.write_text(text)
    return str(path), ReadTimingModel(str(path)).readfulltimingmodel()[2]


# ------------------------------------------------------------------------------------------- keys, injection, .par
def test_keys_validation_and_kind_mismatch(tmp_path):
    from crimp_amd import fit_orbit as F
    from crimp_amd.utilities_fittoas import validate_parfile
    _, bt = read(tmp_path, PAR_BT)
    _, ell1 = read(tmp_path, PAR_ELL1, "e.par")
    assert F.list_orbit_fit_keys(bt) == ["F0", "F1", "PB", "PBDOT", "A1", "A1DOT", "T0", "ECC"]
    assert F.list_orbit_fit_keys(ell1) == ["F0", "PB", "A1", "A1DOT", "TASC", "EPS1", "EPS2"]
    # the BINARY entry holds a name: the binary-free validation refuses it, the orbit validation takes it
    with pytest.raises(ValueError, match="BINARY"):
        validate_parfile(bt)
    assert F.validate_orbit_parfile(bt) == "BT" and F.validate_orbit_parfile(ell1) == "ELL1"
    with pytest.raises(ValueError, match="no BINARY"):
        F.validate_orbit_parfile({k: v for k, v in bt.items() if k != "BINARY"})
    # a key of the other kind, flagged
    bad = dict(bt)
    bad["EPS1"] = {"value": 0.0, "flag": 1}
    with pytest.raises(ValueError, match="BINARY BT has no EPS1"):
        F.list_orbit_fit_keys(bad)
    bad = dict(ell1)
    bad["OM"] = {"value": 10.0, "flag": 1}
    with pytest.raises(ValueError, match="BINARY ELL1 has no OM"):
        F.validate_orbit_parfile(bad)
    # nothing flagged, and a base orbit outside the limits
    none = {k: ({**v, "flag": 0} if v.get("flag") == 1 else v) for k, v in bt.items()}
    with pytest.raises(ValueError, match="no free parameters"):
        F.validate_orbit_parfile(none)
    out = dict(bt)
    out["ECC"] = {"value": 1.2, "flag": 1}
    with pytest.raises(ValueError, match=r"ECC must be in \[0, 1\)"):
        F.validate_orbit_parfile(out)


def test_injection_semantics_and_aliases(tmp_path):
    from crimp_amd import fit_orbit as F
    _, bt = read(tmp_path, PAR_BT)
    keys = F.list_orbit_fit_keys(bt)
    p = np.array([1e-9, 2e-16, 1e-6, 1e-13, 1e-4, -2e-15, 1e-5, 1e-3])
    fit, full = F.inject_orbit_params(bt, p, keys)
    # the fit model is the spin fit model: no orbit in it, the free spin keys their entries
    assert not any(k in fit for k in F.ORBIT_KEYS + ("BINARY",))
    assert fit["F0"] == 1e-9 and fit["F1"] == 2e-16 and fit["PEPOCH"] == 58000
    assert full["F0"] == 17.1 - 1e-9 and full["BINARY"] == "BT"
    assert full["PB"] == 3.2 - 1e-6 and full["A1"] == 12.0 - 1e-4 and full["T0"] == 57000.125 - 1e-5
    assert full["ECC"] == 0.3 - 1e-3 and full["OM"] == 350.0 and full["GAMMA"] == 0.004
    # PBDOT 2.5 is in units of 1e-12; its entry of p is dimensionless, and the value goes back in units of 1e-12
    assert full["PBDOT"] == pytest.approx((2.5e-12 - 1e-13) / 1e-12, rel=1e-15)
    # A1DOT 3e-13 is dimensionless as written and stays so
    assert full["A1DOT"] == 3e-13 + 2e-15
    # a hand-built model under the alias names
    alias = {("XDOT" if k == "A1DOT" else "E" if k == "ECC" else k): v for k, v in bt.items()}
    akeys = F.list_orbit_fit_keys(alias)
    assert "XDOT" in akeys and "E" in akeys and "ECC" not in akeys
    _, afull = F.inject_orbit_params(alias, p, akeys)
    assert afull["E"] == full["ECC"] and afull["XDOT"] == full["A1DOT"]
    with pytest.raises(KeyError):
        F.inject_orbit_params(bt, [1.0], ["F0X"])


def test_patched_par_round_trip_keeps_units_and_binary_line(tmp_path):
    from crimp_amd import fit_orbit as F
    from crimp_amd.binarymodels import binary_params
    path, bt = read(tmp_path, PAR_BT)
    keys = F.list_orbit_fit_keys(bt)
    p = np.array([1e-9, 2e-16, 1e-6, 1e-13, 1e-4, -2e-15, 1e-5, 1e-3])
    _, full = F.inject_orbit_params(bt, p, keys)
    new = str(tmp_path / "new.par")
    F.patch_orbit_par(path, new, full, {k: 1.0 for k in keys})
    text = open(new).read()
    assert "BINARY BT\n" in text
    lines = {ln.split()[0]: ln.split() for ln in text.splitlines() if ln.strip()}
    assert float(lines["PBDOT"][1]) == pytest.approx(2.4, rel=1e-15)      # still in units of 1e-12
    assert float(lines["XDOT"][1]) == 3e-13 + 2e-15 and "A1DOT" not in lines   # the line keeps its name
    assert float(lines["E"][1]) == 0.3 - 1e-3
    assert float(lines["T0"][1]) == 57000.125 - 1e-5                      # 17 digits: the MJD survives
    assert float(lines["OM"][1]) == 350.0 and len(lines["OM"]) == 2      # an unflagged line: its value, no uncertainty
    _, again = read(tmp_path, text, "again.par")
    b0, b1 = binary_params(bt), binary_params(again)
    assert b1["pbdot"] == pytest.approx(b0["pbdot"] - 1e-13, rel=1e-15)
    assert b1["a1dot"] == b0["a1dot"] + 2e-15
    assert b1["pb"] == b0["pb"] - 1e-6 and b1["t0"] == b0["t0"] - 1e-5 and b1["ecc"] == b0["ecc"] - 1e-3
    # a value in units of 1e-12 whose corrected magnitude would read back as dimensionless is written dimensionless
    assert F._par_units("PBDOT", 2.5, 1e-20) == 1e-20
    assert F._par_units("PBDOT", 2.5, 2.4e-12) == pytest.approx(2.4)
    assert F._par_units("PBDOT", 3e-13, 2.9e-13) == 2.9e-13
    assert F._par_units("PBDOT", 3e-13, 2e-7) == pytest.approx(2e5)       # above 1e-7 only units of 1e-12 read back


def test_existing_fits_still_refuse_and_loader_is_shared(tmp_path):
    from crimp_amd import fit_orbit as F
    from crimp_amd import fit_toas
    _, bt = read(tmp_path, PAR_BT)
    import pandas as pd
    with pytest.raises(ValueError, match="binary models are not fitted yet"):
        fit_toas.load_toas_for_fit(pd.DataFrame(), bt)
    with pytest.raises(ValueError, match="no BINARY"):
        F.load_toas_for_fit(pd.DataFrame(), {"F0": {"value": 1.0, "flag": 1}})
    assert callable(F.main) and callable(F.fit_orbit_toas) and callable(F.run_mcmc) and callable(F.make_nll)


# ------------------------------------------------------------------------------------------- the map
def test_orbit_fit_map_packing():
    from crimp_amd import _native as N
    from crimp_amd import ops
    assert N.ORBIT_FIELDS == ("PB", "A1", "T0", "ECC", "OM", "OMDOT", "GAMMA", "EPS1", "EPS2", "PBDOT", "A1DOT")
    assert N.FIT_SLOT_BINARY == 3
    keys = ["PB", "F1", "TASC", "F0", "E", "XDOT", "GLF0_2", "A1DOT", "PBDOT"]
    m = ops.orbit_fit_map(keys)
    got = [(m.slot[i].kind, m.slot[i].index, m.slot[i].sub) for i in range(m.ndim)]
    assert m.ndim == 9 and m.f0_param == 3 and m.branch == N.FIT_WAVES_FIXED
    assert got == [(3, 0, 0), (0, 1, 0), (3, 2, 0), (0, 0, 0), (3, 3, 0), (3, 10, 0), (1, 1, 2), (3, 10, 0), (3, 9, 0)]
    # orbital keys alone: no spin slot, the fixed-wave branch; a wave key beside them: the mixed branch
    m = ops.orbit_fit_map(["A1", "T0"])
    assert (m.ndim, m.f0_param, m.branch) == (2, -1, N.FIT_WAVES_FIXED)
    assert ops.orbit_fit_map(["A1", "WAVE1_A", "F0"]).branch == N.FIT_WAVES_MIXED
    assert ops.orbit_fit_map(["WAVE1_A", "WAVE1_B", "PB"]).branch == N.FIT_WAVES_ONLY
    with pytest.raises(ValueError, match="cannot be fitted"):
        ops.orbit_fit_map(["A1", "SINI"])
    with pytest.raises(ValueError, match="1..32"):
        ops.orbit_fit_map([])
    # the binary-free map still refuses an orbital key
    with pytest.raises(ValueError, match="cannot be fitted"):
        ops.fit_map(["F0", "PB"])


# ------------------------------------------------------------------------------------------- the definition
def test_fixture_covers_the_cases(fixture):
    assert set(fixture) == {(m, n) for m in O.MODELS for n in O.SIZES}
    for (name, n), c in fixture.items():
        assert c.t.shape == (n,) and c.hi.shape == (5, n) and c.pvec.shape == (5, len(c.keys))
        orb = np.array([k in O.ORBITAL for k in c.keys])
        assert not c.pvec[0].any()
        assert c.pvec[1][orb].all() and not c.pvec[1][~orb].any()
        assert c.pvec[2][~orb].all() and not c.pvec[2][orb].any()
        np.testing.assert_array_equal(c.pvec[4], 1e3 * c.pvec[3])
        assert np.max(np.abs(c.m[0])) < 1e-40         # the zero vector: no residual (two 60-digit solves of one root)
    assert {str(c.tm["BINARY"]) for c in fixture.values()} == {"BT", "ELL1"}


@pytest.mark.parametrize("name", O.MODELS)
def test_numpy_twin_is_within_the_derived_bound(fixture, name):
    """The fp64 twin of the definition -- the delays of binary_delay_host, R by its series -- against the 60-digit
    values with the exact R: every ToA of every vector within FACTOR u A plus the mean's share. Largest ratio measured:
    0.071 (bt_e07, the 1e3-width vector)."""
    worst = 0.0
    for n in O.SIZES:
        c = fixture[(name, n)]
        mu = np.array([O.mu_host(c.tm, c.keys, p, c.t) for p in c.pvec])
        ratio = float(np.max(c.mu_err(mu) / c.bound()))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, n, ratio)
        assert not mu[0].any()
        # the bound is far below the residuals it checks, and it is not the 1e-9 of the binary-free fits
        assert np.max(c.bound()) < 1e-6
        # with the orbital entries 0 the twin is the spin fit at the fixed orbit's emission times, bit for bit
        orb = [k in O.ORBITAL for k in c.keys]
        spin_keys = [k for k, o in zip(c.keys, orb) if not o]
        spin_p = c.pvec[2][~np.array(orb)]
        np.testing.assert_array_equal(O.residual_host(c.tm, c.keys, c.pvec[2], c.t),
                                      O.residual_host(c.tm, spin_keys, spin_p, c.t))
    print(name, "largest |mu - mp| / bound %.3g" % worst)


def test_twin_marks_inadmissible_orbits(fixture):
    c = fixture[("bt_e07", 63)]
    p = np.zeros(len(c.keys))
    p[c.keys.index("ECC")] = -0.4            # ECC = 1.1
    assert np.isnan(O.residual_host(c.tm, c.keys, p, c.t)).all()


@pytest.mark.parametrize("name", sorted(O.INJECTION))
def test_injection_problem_is_recoverable_on_the_host(name):
    """What tests/test_gpu_orbit_fit.py asks of the device fit holds for the twin's own least-squares solution:
    every parameter within 5 linearised sigma of p_true (and sigma is the linearised one by construction)."""
    prob = O.injection_problem(name)
    p = O.least_squares_host(prob)
    pull = (p - prob["p_true"]) / prob["sigma"]
    print(name, prob["keys"], np.round(pull, 2))
    assert np.all(np.abs(pull) < 5.0)
    assert np.allclose(np.abs(prob["p_true"]) / prob["sigma"], O.INJECTION_OFFSET, rtol=0.2)
    assert len(prob["t"]) == 64 and abs(np.mean(prob["y"])) < 1e-15
