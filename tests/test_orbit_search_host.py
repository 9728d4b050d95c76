"""The orbit search's host side on the CPU: the long-double truth of tests/orbit_search_reference.py against the
60-digit fixture, the restated unit A_tau against the fixture's, the host plan (csrc/orbit_search_plan.h) through its
stand-alone check program (`make -C crimp_amd/csrc orbit-search-plan-check`: the host compiler under
-fsanitize=address,undefined; no GPU, no preloaded library), the product grid and the orbit ValueErrors of
crimp_amd/orbitsearch.py, and the cap that keeps the GPU test's unit from being vacuous."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import binary_reference as BR
import orbit_search_reference as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crimp_amd", "csrc")
LD = np.longdouble
U_LD = 2.0 ** -64
SLICE, BLOCK, ACC = 3072, 256, 16


@pytest.fixture(scope="module")
def fixture_models():
    return BR.load_binary()


# ---------------------------------------------------------------------------------------- the truth and its unit
def test_delay_ld_matches_the_stored_60_digit_delay(fixture_models):
    """|delay_ld - tau_60| <= FACTOR_TAU 2^-64 A_tau: the rounding count of the unit with long double's unit roundoff
    (the fixture's hi + lo carries tau to 2^-72 of itself)."""
    for name, M in fixture_models.items():
        tau = OR.delay_ld(OR.orbit_of(M.tm), M.t)
        err = np.abs((tau - M.hi["tau"].astype(LD)) - M.lo["tau"].astype(LD)).astype(np.float64)
        bound = OR.FACTOR_TAU * U_LD * M.A["tau"] + 2.0 ** -70 * np.abs(M.hi["tau"])
        worst = float(np.max(err / bound))
        print(name, "max |delay_ld - tau_60| / bound = %.3f" % worst)
        assert worst <= 1.0, name


def test_delay_ld_matches_delay_mp(fixture_models):
    pytest.importorskip("mpmath")
    rng = np.random.default_rng(5)
    for name, M in fixture_models.items():
        t = rng.uniform(M.t.min(), M.t.max(), 20)
        tau = OR.delay_ld(OR.orbit_of(M.tm), t)
        val, mag = BR.delay_mp(M.tm, t, starts=tau.astype(np.float64))
        for i in range(t.size):
            err = abs(float(LD(float(val[i])) - tau[i]) + float(val[i] - float(val[i])))
            assert err <= OR.FACTOR_TAU * U_LD * float(mag[i]) + 2.0 ** -70 * abs(float(val[i])), (name, i, err)


def test_restated_a_tau_equals_the_fixture_unit(fixture_models):
    """The fixture stores A cut towards zero to 16 bits: within [a (1 - 2^-15), a] of the restated value."""
    for name, M in fixture_models.items():
        a = OR.a_tau(OR.orbit_of(M.tm), M.t)
        A = M.A["tau"]
        assert np.all(A <= a * (1 + 1e-9)) and np.all(A >= a * (1 - 2.0 ** -15) * (1 - 1e-9)), name


def test_orbit_of_equals_binary_reference(fixture_models):
    for M in fixture_models.values():
        assert OR.orbit_of(M.tm) == BR.orbit_values(M.tm)


# ---------------------------------------------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def plan_check():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-s", "-B", "-C", CSRC, "orbit-search-plan-check"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(CSRC, "build", "orbit_search_plan_check")


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, text + r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def run_plan(exe, n, nf, m, stat, norb, cap):
    p = {"groups": []}
    for ln in _run(exe, "plan %d %d %d %d %d %d\n" % (n, nf, m, stat, norb, cap)).splitlines():
        key, *v = ln.split()
        if key == "group":
            p["groups"].append((int(v[0]), int(v[1])))
        else:
            p[key] = int(v[0])
    return p


def groups_of(m):
    out, k = [], 1
    while k <= m:
        rem = m - k + 1
        g = 8 if rem >= 8 else 4 if rem >= 4 else 2 if rem >= 2 else 1
        out.append((k, g))
        k += g
    return out


def j_of(m):
    return ACC // groups_of(m)[0][1]


def rule(n, nf, m, norb, cap):
    nslices = -(-n // SLICE)
    per = nslices * 2 * m * nf
    batch = min(max(1, (cap // 8) // per), 65535, norb)
    return {"slice": SLICE, "nslices": nslices, "J": j_of(m), "batch": batch, "nbatches": -(-norb // batch),
            "part_elems": per * batch, "grid_x": nslices, "grid_y": batch, "groups": groups_of(m)}


GIB = 1 << 30


def _check_plan(exe, n, nf, m, norb, cap):
    p = run_plan(exe, n, nf, m, m % 2, norb, cap)
    assert p == rule(n, nf, m, norb, cap), (n, nf, m, norb, cap, p)
    assert all(g * p["J"] <= ACC for _, g in p["groups"])
    assert sum(g for _, g in p["groups"]) == m
    assert p["nslices"] * SLICE >= n > (p["nslices"] - 1) * SLICE
    assert p["batch"] * p["nbatches"] >= norb and 1 <= p["batch"] <= 65535


def test_plan_equals_the_restated_rule_on_the_edge_shapes(plan_check):
    for m in (1, 2, 3, 5, 7, 9, 15, 20, 256):  # every trial-chunk edge of every J
        J = j_of(m)
        for nf in sorted({1, max(1, J - 1), J, J + 1, 5 * J + 3}):
            _check_plan(plan_check, SLICE + 1, nf, m, 25, GIB)
    for n in (1, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 257, 10 ** 6):  # every slice edge under every batching
        for norb, cap in ((1, GIB), (25, GIB), (10 ** 4, GIB), (70000, 1 << 40), (25, 8), (10 ** 4, 1 << 20)):
            _check_plan(plan_check, n, j_of(2) + 1, 2, norb, cap)


def test_plan_batches(plan_check):
    # more orbits than a launch holds; a cap that forces batches of one orbit
    assert run_plan(plan_check, 10 ** 5, 16, 2, 0, 70000, 1 << 40)["batch"] == 65535
    p = run_plan(plan_check, 2 * SLICE + 257, 43, 2, 0, 25, 8)
    assert (p["batch"], p["nbatches"]) == (1, 25)
    per = 3 * 4 * 43 * 8
    p = run_plan(plan_check, 2 * SLICE + 257, 43, 2, 0, 25, 7 * per + 5)
    assert (p["batch"], p["nbatches"]) == (7, 4)


def test_slice_structure_depends_on_n_only(plan_check):
    for n in (1, SLICE, SLICE + 1, 123457):
        seen = {(p["slice"], p["nslices"], p["grid_x"])
                for p in (run_plan(plan_check, n, nf, m, 0, norb, cap)
                          for nf in (1, 17) for m in (1, 20) for norb in (1, 999) for cap in (8, 1 << 16, GIB))}
        assert len(seen) == 1, (n, seen)
    for m in (1, 2, 5, 9, 20):  # J and the groups: from m only
        seen = {(p["J"], tuple(p["groups"]))
                for p in (run_plan(plan_check, n, nf, m, 0, norb, cap)
                          for n in (1, 10 ** 5) for nf in (1, 64) for norb in (1, 999) for cap in (8, GIB))}
        assert len(seen) == 1, (m, seen)


def test_plan_accessor_equals_the_check_program(plan_check):
    from crimp_amd import _native as N
    for n, nf, m, norb in ((1, 1, 1, 1), (2 * SLICE + 257, 43, 2, 25), (10 ** 6, 64, 20, 10 ** 4)):
        a = N.orbit_search_plan(n, nf, m, 0, norb)
        p = run_plan(plan_check, n, nf, m, 0, norb, GIB)
        assert (a["slice"], a["nslices"], a["J"], a["batch"], a["nbatches"], a["part_bytes"]) == \
            (p["slice"], p["nslices"], p["J"], p["batch"], p["nbatches"], 8 * p["part_elems"])


RAW = {"PB": 0.21, "A1": 1.2, "T0": 57999.95, "ECC": 0.7, "OM": 70.0, "OMDOT": 30.0, "GAMMA": 1e-4, "EPS1": 0.0,
       "EPS2": 0.0, "PBDOT": 0.0, "A1DOT": 0.0}
FIELDS = ("PB", "A1", "T0", "ECC", "OM", "OMDOT", "GAMMA", "EPS1", "EPS2", "PBDOT", "A1DOT")


def _orbit_fault(exe, kind, **over):
    raw = dict(RAW, **over)
    return _run(exe, "orbit %d %s\n" % (kind, " ".join(repr(float(raw[k])) for k in FIELDS))).strip()


def test_orbit_limits_of_the_host_check(plan_check):
    assert _orbit_fault(plan_check, 1) == "ok"
    assert _orbit_fault(plan_check, 1, ECC=1.0) == "fault ECC must be in [0, 1)"
    assert _orbit_fault(plan_check, 1, ECC=-0.1) == "fault ECC must be in [0, 1)"
    assert _orbit_fault(plan_check, 1, PB=0.0) == "fault PB must be positive"
    assert _orbit_fault(plan_check, 1, A1=-1.0) == "fault A1 must be >= 0"
    assert _orbit_fault(plan_check, 1, A1=500.0) == "fault 2 pi A1 / (PB (1 - e)) must be below 1/2"
    assert _orbit_fault(plan_check, 1, OM=float("nan")) == "fault a binary parameter is not finite"
    assert _orbit_fault(plan_check, 2, ECC=0.0, EPS1=0.8, EPS2=0.7) == "fault EPS1^2 + EPS2^2 must be below 1"
    # the limit itself: 2 pi A1 / (pb (1 - e)) = 1/2 is refused, the double below it admitted
    a1 = 0.5 * 0.21 * 86400.0 * (1.0 - 0.7) / (2.0 * 3.141592653589793)
    lim = [a for a in (np.nextafter(a1, 0), a1, np.nextafter(a1, 9))
           if not 2.0 * 3.141592653589793 * a / (0.21 * 86400.0 * (1.0 - 0.7)) < 0.5]
    assert _orbit_fault(plan_check, 1, A1=lim[0]).startswith("fault 2 pi")
    assert _orbit_fault(plan_check, 1, A1=np.nextafter(lim[0], 0)) == "ok"


# ------------------------------------------------------------------------------------------ the Python layer
def test_product_grid_first_axis_outermost():
    from crimp_amd.orbitsearch import product_grid
    keys, orb = product_grid({"TASC": [1.0, 2.0], "A1": [10.0, 20.0, 30.0], "PB": [7.0, 8.0]})
    assert keys == ["TASC", "A1", "PB"] and orb.shape == (12, 3)
    assert orb[:, 0].tolist() == [1.0] * 6 + [2.0] * 6
    assert orb[:6, 1].tolist() == [10.0, 10.0, 20.0, 20.0, 30.0, 30.0]
    assert orb[:, 2].tolist() == [7.0, 8.0] * 6
    for o, row in enumerate(orb):  # the row of flat index o is the cell np.unravel_index names
        i, j, k = np.unravel_index(o, (2, 3, 2))
        assert row.tolist() == [[1.0, 2.0][i], [10.0, 20.0, 30.0][j], [7.0, 8.0][k]]


def test_inadmissible_orbits_raise_and_name_the_orbit():
    from crimp_amd.orbitsearch import check_orbits
    bt, ell1 = OR.MODELS["bt_e07"], OR.MODELS["ell1"]
    ok = np.array([[0.7, 1.2], [0.2, 1.0], [0.5, 1.1]])
    idx, orb = check_orbits(bt, ["ECC", "A1"], ok)
    assert idx == [3, 1] and np.array_equal(orb, ok)
    bad = ok.copy()
    bad[1, 0] = 1.0
    with pytest.raises(ValueError, match=r"orbit 1 .*ECC must be in \[0, 1\)"):
        check_orbits(bt, ["ECC", "A1"], bad)
    bad = ok.copy()
    bad[2, 1] = 0.5 * 0.21 * 86400.0 * (1.0 - 0.5) / (2.0 * np.pi) * 1.001   # 2 pi A1 / (PB (1 - e)) just above 1/2
    with pytest.raises(ValueError, match=r"orbit 2 .*must be below 1/2"):
        check_orbits(bt, ["ECC", "A1"], bad)
    with pytest.raises(ValueError, match="not an orbit key"):
        check_orbits(bt, ["F0"], [[1.0]])
    with pytest.raises(ValueError, match="not a key of a BT orbit"):
        check_orbits(bt, ["EPS1"], [[1e-5]])
    with pytest.raises(ValueError, match="not a key of a BT orbit"):
        check_orbits(bt, ["TASC"], [[58000.0]])
    with pytest.raises(ValueError, match="not a key of a ELL1 orbit"):
        check_orbits(ell1, ["ECC"], [[0.1]])
    with pytest.raises(ValueError, match="named twice"):
        check_orbits(ell1, ["TASC", "TASC"], [[58000.0, 58000.0]])
    with pytest.raises(ValueError, match="no BINARY"):
        check_orbits({"PEPOCH": 58000.0, "F0": 1.0}, ["A1"], [[1.0]])


def test_orbit_search_without_binary_raises():
    from crimp_amd.orbitsearch import OrbitSearch
    with pytest.raises(ValueError, match="no BINARY"):
        OrbitSearch(np.array([58000.0, 58000.1]), {"PEPOCH": 58000.0, "F0": 1.0}, [1.0])
    s = OrbitSearch(np.array([58000.0, 58000.2]), OR.MODELS["ell1"], [401.0])
    assert s.tref == 58000.1


def test_cli_axes_from_yaml_and_flags(tmp_path):
    from crimp_amd import orbitsearch as S
    args = S.build_parser().parse_args(["ev.npy", "m.par", "out.txt", "-fl", "400.9", "-fh", "401.1", "-a",
                                        "a1=0.05:0.07:5", "-a", "PB=0.08:0.09:3"])
    assert [k for k, _ in args.axis] == ["A1", "PB"] and np.array_equal(args.axis[0][1], np.linspace(0.05, 0.07, 5))
    y = tmp_path / "axes.yaml"
    y.write_text("TASC: {min: 57999.9, max: 58000.0, n: 4}\nA1: [0.06, 0.063]\n")
    axes = S.load_axes(str(y), args.axis)
    assert list(axes) == ["TASC", "A1", "PB"]          # the YAML's order first; a flag replaces a YAML axis in place
    assert np.array_equal(axes["TASC"], np.linspace(57999.9, 58000.0, 4)) and axes["A1"].size == 5
    with pytest.raises(SystemExit):
        S.build_parser().parse_args(["ev.npy", "m.par", "out.txt", "-fl", "1", "-fh", "2", "-a", "A1=1:2"])
    t = np.linspace(58000.0, 58000.3, 7)
    np.save(tmp_path / "t.npy", t.reshape(7, 1))
    assert np.array_equal(S.load_times(str(tmp_path / "t.npy")), t)


# --------------------------------------------------------------------------------- the unit is not vacuous
def test_signal_trial_unit_is_below_1e_6_of_the_power():
    """The cap of tests/test_gpu_orbit_search.py, checked here for its inputs: at the true orbit and frequency the unit
    is at most 1e-6 of the power."""
    for c in OR.cases(SLICE, j_of):
        power, unit = c.truth(c.otrue, np.array([c.jtrue]))
        print(c.name, "power %.6g unit %.3g ratio %.3g" % (power[0], unit[0], unit[0] / power[0]))
        assert unit[0] <= 1e-6 * power[0], c.name
