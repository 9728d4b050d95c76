"""Host side of the timing-model fits against the reference's recorded behaviour (tests/golden/fittoas.json,
fittoas.npz; tests/golden/gen_fittoas_golden.py): parameter bookkeeping, validation and YAML errors, .par patching,
the small statistics, the local-ephemerides window walk, and the packaging of the three scripts. No GPU."""
import copy
import importlib
import json
import os

import numpy as np
import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

from crimp_amd import fit_toas as FT  # noqa: E402
from crimp_amd import get_local_ephem as GL  # noqa: E402
from crimp_amd import readtimingmodel as RT  # noqa: E402
from crimp_amd import utilities_fittoas as UF  # noqa: E402
from crimp_amd.timfile import readtimfile  # noqa: E402


@pytest.fixture(scope="module")
def side():
    with open(os.path.join(GOLD, "fittoas.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(GOLD, "fittoas.npz")))


def plain(d):
    """Nested dicts with floats, as the fixture stores them."""
    return {k: plain(v) if isinstance(v, dict) else (None if v is None else float(v)) for k, v in d.items()}


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_keys_and_injected_dicts_equal_reference(side, case):
    c = side["cases"][case]
    model = copy.deepcopy(c["model"])
    keys = UF.list_fit_keys(model)
    assert keys == c["keys"]
    p0, k2 = UF.extract_free_params(model)
    assert k2 == keys and p0.shape == (len(keys),) and not p0.any()
    fit, full = UF.inject_free_params(model, np.array(c["pvec"]), keys)
    assert list(fit) == list(c["fit"]) and list(full) == list(c["full"])
    assert plain(fit) == c["fit"]
    assert plain(full) == c["full"]


def test_case_a_model_is_what_the_reader_returns(side):
    """Case (a) of the fixture is 1e2259.par as this build's reader lays it out, with F0 and F1 flagged."""
    m = RT.ReadTimingModel(os.path.join(GOLD, "1e2259.par")).readfulltimingmodel()[2]
    m["F0"]["flag"] = m["F1"]["flag"] = 1
    assert plain(m) == side["cases"]["a"]["model"]
    assert list(m) == list(side["cases"]["a"]["model"])


def test_gltd_without_glf0d_is_zeroed_in_place():
    model = {"PEPOCH": {"value": 5.0, "flag": 0}, "F0": {"value": 1.0, "flag": 1},
             "GLEP_1": {"value": 6.0, "flag": 0}, "GLF0D_1": {"value": 0, "flag": 0},
             "GLTD_1": {"value": 30.0, "flag": 1}}
    fit, full = UF.inject_free_params(model, np.array([1e-3, 2.0]), ["F0", "GLTD_1"])
    assert model["GLTD_1"]["value"] == 0
    assert fit == {"PEPOCH": 5.0, "F0": 1e-3, "GLEP_1": 6.0, "GLF0D_1": 0.0, "GLTD_1": 2.0}
    assert full == {"PEPOCH": 5.0, "F0": 1.0 - 1e-3, "GLEP_1": 6.0, "GLF0D_1": 0, "GLTD_1": 2.0}
    with pytest.raises(KeyError, match="Parameter 'F5' not found in parfile."):
        UF.inject_free_params(model, np.array([1.0]), ["F5"])
    with pytest.raises(KeyError, match="Parameter 'WAVE3' not found in parfile."):
        UF.inject_free_params(model, np.array([1.0]), ["WAVE3_A"])


def test_validate_parfile_messages():
    ok = {"PEPOCH": {"value": 1.0, "flag": 0}, "F0": {"value": 1.0, "flag": 1},
          "WAVEEPOCH": {"value": 1.0, "flag": None}, "WAVE1": {"value": {"A": 1.0, "B": 2.0}, "flag": None}}
    UF.validate_parfile(ok)
    with pytest.raises(ValueError, match="Initial timing model must be a dict"):
        UF.validate_parfile([1])
    with pytest.raises(ValueError, match="Parameter 'F1' must be a dict with 'value' and 'flag'"):
        UF.validate_parfile({**ok, "F1": 3.0})
    with pytest.raises(ValueError, match="Parameter 'F1': value must be numeric, got <class 'str'>"):
        UF.validate_parfile({**ok, "F1": {"value": "x", "flag": 0}})
    with pytest.raises(ValueError, match="Parameter 'F1': fit flag must be 0 or 1, got 2"):
        UF.validate_parfile({**ok, "F1": {"value": 1.0, "flag": 2}})
    with pytest.raises(ValueError, match=r"Template has no free parameters \(flag==1\). Nothing to optimize."):
        UF.validate_parfile({**ok, "F0": {"value": 1.0, "flag": 0}})


def test_yaml_priors_and_consistency_errors(tmp_path):
    def load(text):
        p = tmp_path / "p.yaml"
        p.write_text(text)
        return UF.initguess_prior_from_yaml(str(p))

    pr = load("F0: {low: -1e-8, high: 1e-8, guess: 1e-9}\nF1: {low: -2, high: 3, guess: 0}\n")
    assert pr.bounds == {"F0": (-1e-8, 1e-8), "F1": (-2.0, 3.0)} and pr.initial_guess == {"F0": 1e-9, "F1": 0.0}
    assert pr.log_prior(np.array([0.0, 1.0]), ["F0", "F1"]) == 0.0
    assert pr.log_prior(np.array([1e-8, 1.0]), ["F0", "F1"]) == -np.inf  # strict
    assert pr.log_prior(np.array([0.0, 7.0]), ["F0", "F9"]) == 0.0       # no bounds for a key: no penalty
    np.testing.assert_array_equal(UF.initialize_params(["F1", "F0"], str(tmp_path / "p.yaml")), [0.0, 1e-9])
    assert load("F0: [-1, 1]\n").bounds == {"F0": (-1.0, 1.0)}
    assert load("F0: 3\n").initial_guess == {"F0": 3.0}
    for text, msg in (("- 1\n", "YAML must map parameter -> prior/guess"),
                      ("F0: [1, 2, 3]\n", "F0: expected \\[low, high\\]"),
                      ("F0: [2, 1]\n", "F0: low < high required"),
                      ("F0: {low: 1}\n", "F0: need both 'low' and 'high' if providing bounds"),
                      ("F0: {low: 2, high: 1}\n", "F0: low < high required"),
                      ("F0: abc\n", "F0: unsupported value 'abc'"),
                      ("F0: [-1, 1]\nF1: 2\n",
                       "Bounds provided for some parameters but missing for others: F1"),
                      ("F0: {low: -1, high: 1, guess: 0}\nF1: [-1, 1]\n",
                       "Initial guesses provided for some parameters but missing for others: F1")):
        with pytest.raises(ValueError, match=msg):
            load(text)
    (tmp_path / "b.yaml").write_text("F0: [-1, 1]\n")
    with pytest.raises(ValueError, match="No initial guesses found in YAML file."):
        UF.initialize_params(["F0"], str(tmp_path / "b.yaml"))
    (tmp_path / "g.yaml").write_text("F0: 1\n")
    with pytest.raises(KeyError, match="Missing initial guesses for: F1"):
        UF.initialize_params(["F0", "F1"], str(tmp_path / "g.yaml"))


def test_gaussian_nll_is_the_reference_expression():
    rng = np.random.default_rng(2)
    y, mu, s = rng.normal(size=9), rng.normal(size=9), rng.uniform(0.1, 1, 9)
    assert UF.gaussian_nll(y, mu, s) == 0.5 * np.sum(((y - mu) / s) ** 2 + np.log(2.0 * np.pi * s ** 2))


def test_patched_par_files_are_text_identical(side, tmp_path):
    p = side["par"]
    src, dst = str(tmp_path / "in.par"), str(tmp_path / "out.par")
    with open(src, "w") as fh:
        fh.write(p["input"])
    RT.patch_par_values(in_path=src, out_path=dst, new_values=p["new_values"])
    assert open(dst).read() == p["mle_values"]
    RT.patch_statistics(in_path=dst, out_path=dst, new_stats=p["stats"])
    RT.patch_miscellaneous(in_path=dst, out_path=dst, new_misc=p["misc"])
    assert open(dst).read() == p["mle_final"]
    RT.patch_par_values(in_path=src, out_path=dst, new_values=p["new_values"], uncertainties=p["uncertainties"])
    assert open(dst).read() == p["mcmc_values"]
    RT.patch_statistics(in_path=dst, out_path=dst, new_stats=p["stats"])
    RT.patch_statistics(in_path=dst, out_path=dst, new_stats=p["stats"])
    RT.patch_miscellaneous(in_path=dst, out_path=dst, new_misc=p["misc"])
    assert open(dst).read() == p["mcmc_final"]


def test_patch_par_values_waves_and_untouched_lines(tmp_path):
    src, dst = str(tmp_path / "w.par"), str(tmp_path / "w2.par")
    text = "# comment\nF0   1.5 1 0.25 tail\nF3 2.0 0.5\nF4 2.0 3.5\nWAVE_OM 0.1 0\nWAVE1 0.5 -0.5 extra\nWAVE2 1 2\n"
    open(src, "w").write(text)
    RT.patch_par_values(in_path=src, out_path=dst, new_values={
        "F0": {"value": 2.25, "flag": 1}, "F3": 4.0, "F4": 5.0,
        "WAVE1": {"value": {"A": 0.125, "B": 8.0}, "flag": None}})
    # (an unflagged line loses its uncertainty, unless that starts with 0 or 1 and so reads as a flag: as the
    # reference does)
    assert open(dst).read() == ("# comment\nF0   2.25 1 0.25 tail\nF3 4 0.5\nF4 5\nWAVE_OM 0.1 0\nWAVE1 0.125 8\n"
                                "WAVE2 1 2\n")


def test_add_pntrack_parfile(tmp_path):
    par = tmp_path / "t.par"
    par.write_text("F0 1.0\nTRACK -2\n")
    d1, d2 = {"F0": 1.0}, {"F0": {"value": 1.0, "flag": 0}}
    RT.add_pntrack_parfile(d1, str(par))
    RT.add_pntrack_parfile(d2, str(par))
    assert d1["TRACK"] == -2 and d2["TRACK"] == {"value": -2.0, "flag": 0}
    d3 = {"F0": 1.0}
    RT.add_pntrack_parfile(d3, os.path.join(GOLD, "1e2259.par"))
    assert "TRACK" not in d3


def test_add_phasewrap_chi2_and_rms_are_exact():
    df = pd.DataFrame({"ToA": [1.0, 2.0, 3.0, 4.0], "phase": [0.1, 0.2, 0.3, 0.4], "phase_err_cycle": [0.1] * 4})
    out = FT.add_phasewrap(df.copy(), [2.0, 3.5])
    np.testing.assert_array_equal(out["phase"], np.array([0.1, 0.2, 0.3, 0.4]) + np.array([0.0, 1.0, 1.0, 2.0]))
    out = FT.add_phasewrap(df.copy(), 3.0, mode="subtract")
    np.testing.assert_array_equal(out["phase"], np.array([0.1, 0.2, 0.3, 0.4]) - np.array([0.0, 0.0, 1.0, 1.0]))
    assert FT.add_phasewrap(df, []) is df
    with pytest.raises(ValueError, match="mode must be 'add' or 'subtract'."):
        FT.add_phasewrap(df.copy(), 2.0, mode="wrap")
    y, m, e = np.array([1.0, 2.0, 4.0, 8.0]), np.array([0.5, 2.5, 3.0, 8.0]), np.array([0.5, 0.5, 1.0, 2.0])
    st = FT.chi2_fit(y, m, e, 2)
    assert st == {"chi2": np.sum((y - m) ** 2 / e ** 2), "redchi2": np.sum((y - m) ** 2 / e ** 2) / 2, "dof": 2}
    assert FT.rms_residual(y, m) == np.sqrt((1 / 4) * np.sum((y - m) ** 2))


def test_sampler_object_and_summaries():
    rng = np.random.default_rng(5)
    chain, lp = rng.normal(size=(20, 4, 2)), rng.normal(size=(20, 4))
    s = FT.DeviceSampler(chain, lp, np.array([5, 10, 0, 20]))
    assert s.get_chain().shape == (20, 4, 2) and s.get_chain(discard=5, flat=True).shape == (60, 2)
    np.testing.assert_array_equal(s.get_chain(discard=5, flat=True), chain[5:].reshape(-1, 2))
    np.testing.assert_array_equal(s.get_log_prob(discard=5, flat=True), lp[5:].reshape(-1))
    np.testing.assert_array_equal(s.acceptance_fraction, [0.25, 0.5, 0.0, 1.0])
    flat, flp = s.get_chain(discard=5, flat=True), s.get_log_prob(discard=5, flat=True)
    sm = FT.summarize_chain(flat, flp, ["F0", "F1"])
    q = np.percentile(flat[:, 1], [16, 50, 84])
    assert sm["F1"] == {"median": q[1], "minus": q[1] - q[0], "plus": q[2] - q[1], "map": flat[np.argmax(flp), 1]}


def test_run_mcmc_corner_needs_the_package():
    try:
        import corner  # noqa: F401
        pytest.skip("corner is installed")
    except ImportError:
        pass
    with pytest.raises(ImportError, match="corner"):
        FT.run_mcmc(np.arange(4.0), np.zeros(4), np.ones(4), {}, ["F0"], UF.Prior({"F0": (-1, 1)}, {}),
                    corner_pdf="c")


@pytest.mark.parametrize("name, glitch", [("win", False), ("win_glitch", True)])
def test_window_walk_reproduces_reference(gold, side, tmp_path, name, glitch):
    par = os.path.join(GOLD, "1e2259.par")
    if glitch:
        text = open(par).read().rstrip("\n") + "\n" + side["glitch_par_lines"]
        par = str(tmp_path / "glitch.par")
        open(par, "w").write(text)
    wins = GL.local_ephem_windows(readtimfile(os.path.join(GOLD, "ToAs_2259.tim")), par)
    np.testing.assert_array_equal([w["mid"] for w in wins], gold[name + "_TOA_MJD_ref"])
    np.testing.assert_array_equal([w["span_days"] / 2.0 for w in wins], gold[name + "_TOA_MJD_ref_err"])
    np.testing.assert_array_equal([len(w["toas"]) - 2 for w in wins], gold[name + "_DOF"])
    m = GL.window_model(wins[0])
    assert UF.list_fit_keys(m) == ["F0", "F1"] and m["TRACK"] == -2 and m["PEPOCH"]["value"] == wins[0]["mid"]


def test_scripts_are_declared_and_mains_callable():
    import crimp.fit_toas
    import crimp.utilities_fittoas
    import crimp.get_local_ephem
    import crimp.plot_local_ephem
    assert crimp.fit_toas is FT and crimp.utilities_fittoas is UF and crimp.get_local_ephem is GL
    py = open(os.path.join(ROOT, "pyproject.toml")).read()
    cfg = open(os.path.join(ROOT, "setup.cfg")).read()
    for script, mod in {"fittoas": "fit_toas", "localephemerides": "get_local_ephem",
                        "localephemerides_plot": "plot_local_ephem"}.items():
        assert '%s = "crimp_amd.%s:main"' % (script, mod) in py
        assert "    %s = crimp_amd.%s:main" % (script, mod) in cfg
        assert callable(importlib.import_module("crimp_amd." + mod).main)
    # every flag of the reference's fittoas parser (fit_toas.py:285-324)
    opts = {o for a in FT.build_parser()._actions for o in a.option_strings}
    for flag in ("-ts", "--t_start", "-te", "--t_end", "-tm", "--t_mjd", "-md", "--mode", "-iy", "--init_yaml", "-mc",
                 "--mcmc", "--no-mcmc", "-st", "--mcmc-steps", "-bu", "--mcmc-burn", "-wa", "--mcmc-walkers", "-cp",
                 "--corner_plot", "-ch", "--chain-npy", "-fl", "--flat-npy", "-bf", "--best_fit", "-rp",
                 "--residual_plot"):
        assert flag in opts, flag


def test_fit_map_slots_and_branches():
    from crimp_amd import _native as N
    from crimp_amd import ops
    m = ops.fit_map(["F1", "F0", "GLTD_2", "GLEP_1"])
    assert (m.ndim, m.branch, m.f0_param) == (4, N.FIT_WAVES_FIXED, 1)
    assert [(s.kind, s.index, s.sub) for s in list(m.slot)[:4]] == [(0, 1, 0), (0, 0, 0), (1, 1, 6), (1, 0, 0)]
    assert ops.fit_map(["WAVE2_B", "WAVE1_A"]).branch == N.FIT_WAVES_ONLY
    m = ops.fit_map(["F0", "WAVE3_B"])
    assert m.branch == N.FIT_WAVES_MIXED and (m.slot[1].kind, m.slot[1].index, m.slot[1].sub) == (2, 2, 1)
    with pytest.raises(ValueError):
        ops.fit_map(["PEPOCH"])
    with pytest.raises(ValueError):
        ops.fit_map([])
    with pytest.raises(ValueError):
        ops.fit_map(["F%d" % (i % 13) for i in range(33)])


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_numpy_restatement_reproduces_reference_likelihood(side, case):
    """tests/timing_reference.py (the CPU yardstick of tools/run_timing_fit.py) computes what the reference recorded."""
    import timing_reference as TR
    g = np.load(os.path.join(GOLD, "fittoas_nll_%s.npz" % case))
    c = side["cases"][case]
    for n in (1, 65, 257):
        x, y, e = g["x_%d" % n], g["y_%d" % n], g["e_%d" % n]
        for j in (0, 1, 17):
            mu = TR.model_phase_residuals(x, copy.deepcopy(c["model"]), g["pvec"][j], c["keys"])
            assert np.max(np.abs(mu - g["mu_%d" % n][j])) <= 1e-12
            ref = g["nll_%d" % n][j]
            assert abs(TR.nll(x, y, e, copy.deepcopy(c["model"]), g["pvec"][j], c["keys"]) - ref) <= 1e-9 * abs(ref)
