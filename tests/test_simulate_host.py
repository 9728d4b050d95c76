"""CPU-side checks of the event simulator: the drop-in's boundary (import name, messages, exposure truncation), the
host-side rate bounds and validation, the event-file writer, the fixture recorded from the reference, and the NumPy
restatement of the process (tests/sim_reference.py) against every statistical bound the device tests use, with the
device tests' parameters."""
import json

import numpy as np
import pytest

import sim_reference as R
from conftest import GOLDEN, gold, gpath


def test_crimp_simulatemodulatedlc_is_the_dropin():
    import crimp.simulatemodulatedlc
    import crimp_amd.simulatemodulatedlc
    assert crimp.simulatemodulatedlc is crimp_amd.simulatemodulatedlc
    from crimp.simulatemodulatedlc import main, simulatemodulatedlc  # noqa: F401
    import inspect
    sig = inspect.signature(simulatemodulatedlc)
    assert list(sig.parameters) == ["freq", "srcrate", "exposure", "pulsedfraction", "bgrrate", "resolution",
                                    "nbrPhaseBins", "seed"]
    assert [p.default for p in sig.parameters.values()][1:] == [1, 10000, 0.2, 0.05, 0.073, None, None]
    assert sig.parameters["seed"].kind is inspect.Parameter.KEYWORD_ONLY


def test_value_errors_and_printed_lines_precede_any_device_call(capsys, monkeypatch):
    from crimp_amd import ops
    from crimp_amd.simulatemodulatedlc import simulatemodulatedlc

    def no_device(*a, **k):
        raise AssertionError("device call before the host checks")
    monkeypatch.setattr(ops, "sim_events", no_device)
    with pytest.raises(ValueError, match=r"RMS pulse fraction cannot be larger than 1/sqrt\(2\)"):
        simulatemodulatedlc(0.5, pulsedfraction=0.8)
    with pytest.raises(ValueError, match="nbrPhaseBins is very small. Increase time resolution or set nbrPhaseBins "
                                         "manually"):
        simulatemodulatedlc(5.0)  # floor(1 / (0.073 * 5)) = 2 bins
    with pytest.raises(ValueError, match="nbrPhaseBins is very small"):
        simulatemodulatedlc(0.5, nbrPhaseBins=3)
    capsys.readouterr()
    with pytest.raises(ValueError):
        simulatemodulatedlc(0.3, exposure=1001.0, nbrPhaseBins=2)
    out = capsys.readouterr().out.splitlines()
    # int(1001 * 0.3) = 300 cycles -> 1000 s
    assert out == ["Requested exposure (s): 1001.000000",
                   "Simulation exposure (s): 1000.000000 (300 complete cycles at f = 0.300000 Hz)"]


def test_printed_lines_match_the_reference_fixture(capsys, monkeypatch):
    from crimp_amd import ops
    from crimp_amd.simulatemodulatedlc import simulatemodulatedlc
    g = gold("simlc_reference.npz")
    seen = {}

    def fake(model, shape, mjd_start, span_s, cell_s, **kw):
        seen.update(model=model, span=span_s, steps=np.array(shape._steps), bkg=shape.bkg, lam=shape.lam_max,
                    cell=cell_s, seed=kw["seed"])
        return np.zeros(0), np.zeros(0, np.uint8), 0
    monkeypatch.setattr(ops, "sim_events", fake)
    np.random.seed(5)
    r = simulatemodulatedlc(float(g["freq"]), float(g["srcrate"]), float(g["exposure"]), float(g["pulsedfraction"]),
                            float(g["bgrrate"]), nbrPhaseBins=int(g["nbrPhaseBins"]))
    assert capsys.readouterr().out == str(g["printed"])
    assert set(r) == {"assigned_t_wBgr", "assigned_t_nobgr"}
    amp = np.sqrt(2) * 0.3 * 20
    np.testing.assert_allclose(seen["steps"], 20 + amp * np.cos(2 * np.pi * np.arange(16) / 16 + np.pi), rtol=1e-15)
    assert seen["span"] == 2000.0 and seen["bkg"] == 2.0 and seen["model"] == {"PEPOCH": 0.0, "F0": 0.5}
    assert seen["lam"] == seen["steps"].max() + 2.0 and seen["cell"] == 192.0 / seen["lam"]
    first = seen["seed"]
    np.random.seed(5)  # seed=None draws from NumPy's global RNG: np.random.seed makes the run repeatable
    simulatemodulatedlc(0.5, 20, 2000, 0.3, 2, nbrPhaseBins=16)
    assert seen["seed"] == first
    simulatemodulatedlc(0.5, 20, 2000, 0.3, 2, nbrPhaseBins=16)
    assert seen["seed"] != first
    simulatemodulatedlc(0.5, 20, 2000, 0.3, 2, nbrPhaseBins=16, seed=77)
    assert seen["seed"] == 77


def test_reference_fixture_follows_the_analytic_profile():
    """The recorded run of the reference: 39640 source events; its 16 bin counts are independent Poisson variables
    of mean (srcrate + amp cos(2 pi k / n + pi)) T / n (simulatemodulatedlc.py:66, :75): chi^2 = 11.9, bound 58.3."""
    g = gold("simlc_reference.npz")
    assert int(g["n_nobgr"]) == 39640 and int(g["hist_nobgr"].sum()) == 39640
    assert int(g["hist_wbgr"].sum()) == int(g["n_wbgr"])
    nb = 16
    amp = np.sqrt(2) * float(g["pulsedfraction"]) * float(g["srcrate"])
    exp_src = (float(g["srcrate"]) + amp * np.cos(2 * np.pi * np.arange(nb) / nb + np.pi)) * (2000.0 / nb)
    c = float(np.sum((g["hist_nobgr"] - exp_src) ** 2 / exp_src))
    assert abs(c - 11.93) < 0.01 and abs(R.chi2_bound(nb) - 58.32) < 0.01 and c <= R.chi2_bound(nb)
    exp_all = exp_src + float(g["bgrrate"]) * 2000.0 / nb
    assert float(np.sum((g["hist_wbgr"] - exp_all) ** 2 / exp_all)) <= R.chi2_bound(nb)
    R.check_counts(int(g["n_nobgr"]), 40000.0)
    R.check_counts(int(g["n_wbgr"]), 44000.0)
    assert 0.0 <= float(g["t_min"]) and float(g["t_max"]) < 2000.0


def _theta(name):
    th = json.load(open(gpath("cauchy_vm_theta.json")))
    return dict(th, model=name)


def test_rate_bound_dominates_each_model_on_a_dense_sample():
    from crimp_amd.readPPtemplate import readPPtemplate
    from crimp_amd.simulatemodulatedlc import rate_bound, template_rate
    ph = np.arange(200001) / 200001.0
    k6 = readPPtemplate(gpath("1e2259_template.txt"))
    for tmpl in (k6, _theta("cauchy"), _theta("vonmises")):
        for sh in (0.0, 0.3, -2.0):
            for a in (1.0, 0.5, 2.5):
                bound = rate_bound(tmpl, a, 0.25)
                top = float(np.max(template_rate(tmpl, ph, sh, a))) + 0.25
                assert bound >= top, (tmpl["model"], sh, a, bound, top)
                assert bound <= 3.0 * top  # a bound, not a wild over-estimate (efficiency of the thinning)
    # the host's template values are the independent restatement's
    for tmpl in (_theta("cauchy"), _theta("vonmises"), R.FOURIER1):
        np.testing.assert_allclose(template_rate(tmpl, ph[::97], 0.3, 1.2), R.template_rate(tmpl, ph[::97], 0.3, 1.2),
                                   rtol=1e-13)


def test_a_narrow_von_mises_component_stays_finite():
    """kappa = 1 / wid^2 = 2500: exp(kappa) and I0(kappa) overflow separately, their ratio does not."""
    from crimp_amd.simulatemodulatedlc import rate_bound, template_rate
    tmpl = {"model": "vonmises", "norm": 1.0, "amp_1": 2.0, "cen_1": 1.0, "wid_1": 0.02}
    ph = np.arange(4096) / 4096.0
    y = template_rate(tmpl, ph)
    bound = rate_bound(tmpl)
    assert np.all(np.isfinite(y)) and np.isfinite(bound) and y.min() >= 1.0
    # the peak of a narrow von Mises is the normal density's: amp / (wid sqrt(2 pi)), to O(wid^2)
    assert abs(bound - 1.0 - 2.0 / (0.02 * np.sqrt(2.0 * np.pi))) < 1e-3 * bound
    assert y.max() <= bound and abs(y.mean() - (1.0 + 2.0 / (2.0 * np.pi))) < 1e-9


def test_negative_rate_and_bad_inputs_are_refused_on_the_host():
    from crimp_amd.simulatemodulatedlc import build_shape, check_gti, simulate_events
    with pytest.raises(ValueError, match="negative"):
        build_shape({"model": "fourier", "norm": 1.0, "amp_1": 1.5, "ph_1": 0.0})
    with pytest.raises(ValueError, match="negative"):
        build_shape(dict(_theta("cauchy"), norm=-1.0))
    with pytest.raises(ValueError, match="negative"):
        build_shape(np.array([1.0, -0.1, 2.0]))
    with pytest.raises(ValueError):
        build_shape(np.zeros(0))
    with pytest.raises(ValueError):
        build_shape(R.FOURIER1, bgrrate=-1.0)
    shape, lam = build_shape(R.FOURIER1, phShift=0.3, bgrrate=0.5)
    assert lam == 6.0 + 4.0 + 0.5 and shape.lam_max == lam and shape.ph_shift == 0.3 and shape.norm == 6.0
    shape, lam = build_shape(np.array([1.0, 3.0, 2.0]), bgrrate=0.5)
    assert lam == 3.5 and shape.n_steps == 3
    for bad in ([[2.0, 1.0]], [[1.0, 2.0], [1.5, 3.0]], [[3.0, 4.0], [1.0, 2.0]], [1.0, 2.0], [[1.0, np.nan]]):
        with pytest.raises(ValueError):
            check_gti(bad)
    assert check_gti(None) is None
    assert check_gti([[1.0, 2.0], [2.0, 3.0]]).shape == (2, 2)  # touching half-open intervals are disjoint
    with pytest.raises(ValueError):
        simulate_events(R.FLAT_MODEL, R.FOURIER1, 58400.0, 58400.0)
    with pytest.raises(ValueError):
        simulate_events(R.FLAT_MODEL, R.FOURIER1, 58400.0, 58401.0, gti=[[2.0, 1.0]])
    with pytest.raises(ValueError):
        simulate_events(R.FLAT_MODEL, R.FOURIER1, 58400.0, 58401.0, unit="days")
    with pytest.raises(TypeError):
        simulate_events(3.0, R.FOURIER1, 58400.0, 58401.0)


def test_cell_length_is_a_pure_function_of_the_bound():
    from crimp_amd.simulatemodulatedlc import cell_count, cell_length
    assert cell_length(48.0) == 4.0 and cell_length(48.0) == cell_length(48.0)
    assert cell_length(10.5) == 192.0 / 10.5
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            cell_length(bad)
    assert cell_count(2.0, 4.0) == 1 and cell_count(8.0, 4.0) == 2 and cell_count(8.000001, 4.0) == 3
    span = float(2083) * 4.8
    assert cell_count(span, 4.8) == 2083
    for span, cell in ((1000.0, 0.3), (123.456, 7.0), (1.0e7, 1.7)):
        nc = cell_count(span, cell)
        assert float(nc - 1) * cell < span <= float(nc) * cell


def test_without_a_gpu_the_simulator_raises():
    import torch
    from crimp_amd import _native
    from crimp_amd.simulatemodulatedlc import simulate_events, simulatemodulatedlc
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_native.CrimpNativeError):
        simulate_events(R.FLAT_MODEL, R.FOURIER1, 58400.0, 58400.01)
    with pytest.raises(_native.CrimpNativeError):
        simulatemodulatedlc(0.5, exposure=100.0, seed=1)


def test_write_eventfile_round_trip(tmp_path):
    from crimp_amd.eventfile import EvtFileOps
    from crimp_amd.simulatemodulatedlc import write_eventfile
    rng = np.random.default_rng(3)
    t = np.sort(58400.0 + rng.uniform(0.0, 0.7, 5000))
    gti = np.array([[58400.0, 58400.3], [58400.35, 58400.7]])
    p = write_eventfile(str(tmp_path / "sim.fits"), t, gti=gti)
    ef = EvtFileOps(p)
    kw, g = ef.readGTI()
    assert kw["TELESCOPE"] == "NICER"
    df = ef.build_time_energy_df().time_energy_df
    ulp = np.spacing(58400.0)
    assert np.max(np.abs(df["TIME"].to_numpy() - t)) <= 2 * ulp
    assert np.max(np.abs(g - gti)) <= 2 * ulp
    np.testing.assert_allclose(df["PI"].to_numpy(), 2.0)  # channel 200 of NICER's 0.01 keV channels
    p2 = write_eventfile(str(tmp_path / "sim2.fits"), t, pi=np.arange(t.size) % 1000)
    _, g2 = EvtFileOps(p2).readGTI()
    assert np.max(np.abs(g2 - [[t[0], t[-1]]])) <= 2 * ulp


# ---------------------------------------------------------------- the NumPy restatement meets the device tests' bounds
@pytest.fixture(scope="module")
def cases():
    return R.shape_cases(GOLDEN)


def test_numpy_restatement_meets_the_shape_bounds(cases):
    """Host thinning with the parameters of the device shape tests: count, 32-bin chi^2 (before and after the glitch
    for the glitch model) and background fraction."""
    for i, (name, c) in enumerate(cases.items()):
        rate, steps = R.case_rate(c)
        lam = (float(np.max(steps)) if steps is not None
               else float(np.max(rate(np.arange(1 << 14) / (1 << 14)))) * 1.02) + c["bkg"]
        s, isb = R.host_thinning(rate, lam, c["bkg"], c["tm"], R.MJD0, c["span_s"], np.random.default_rng(50 + i))
        ph = R.total_phase(R.MJD0 + s / 86400.0, c["tm"])
        R.check_case(c, s, isb, ph - np.floor(ph), name)


def test_numpy_restatement_meets_the_poisson_bounds():
    """Flat rate, ~4e5 events: count, index of dispersion in 4096 bins and in the cells' own bins, repeated times."""
    lam, cell = 40.0, 4.8
    span = float(2083) * cell
    flat = np.array([lam])
    s, _ = R.host_thinning(lambda ph: R.step_rate(flat, ph), lam, 0.0, R.FLAT_MODEL, R.MJD0, span,
                           np.random.default_rng(9))
    R.check_counts(len(s), lam * span)
    R.check_dispersion(s, span, 4096)
    R.check_dispersion(s, span, 2083)
    mjd = R.MJD0 + s / 86400.0
    assert np.sum(np.diff(mjd) == 0.0) < 20


def test_numpy_restatement_meets_the_gti_bounds():
    gti, span, lam = R.gti_case()
    flat = np.array([lam])
    s, _ = R.host_thinning(lambda ph: R.step_rate(flat, ph), lam, 0.0, R.FLAT_MODEL, R.MJD0, span,
                           np.random.default_rng(10), gti=gti)
    R.check_gti_draw(R.MJD0 + s / 86400.0, gti, span, lam)


def test_numpy_restatement_and_oracle_meet_the_recovery_bound():
    """Two of the injection-recovery intervals drawn by host thinning and fitted by the oracle (brute start)."""
    from oracle import oracle as O
    from crimp_amd.readPPtemplate import readPPtemplate
    from crimp_amd.readtimingmodel import ReadTimingModel
    tm = ReadTimingModel(gpath("1e2259.par")).readfulltimingmodel()[0]
    tmpl = readPPtemplate(gpath("1e2259_template.txt"))
    plain = {k: (v["value"] if isinstance(v, dict) else v) for k, v in tmpl.items()}
    starts, span, shifts = R.recovery_case()
    got = []
    for i in (1, 6):
        lam = plain["norm"] + sum(abs(plain["amp_%d" % j]) for j in range(1, 7))
        s, _ = R.host_thinning(lambda ph: R.template_rate(plain, ph, shifts[i]), lam, 0.0, tm, starts[i], span,
                               np.random.default_rng(20 + i))
        ph = R.total_phase(starts[i] + s / 86400.0, tm)
        r = O.fit_toa(ph - np.floor(ph), span, tmpl, brutemin=True)
        got.append((r["phShi"], r["phShi_LL"], r["phShi_UL"], shifts[i]))
    got = np.array(got)
    R.check_recovery(got[:, 0], got[:, 1], got[:, 2], got[:, 3])
