"""Host side of the pulse-profile plots (crimp_amd/plot_pps.py), no GPU: update_gti, the golden fixture's bookkeeping,
and the NumPy restatement of the device bin rule (tests/cube_reference.py) -- the yardstick of
tests/test_gpu_phase_cube.py -- against np.histogram2d on the golden observation, folded by the CPU oracle (within
1e-9 cycles of the reference, whose phases keep >= 6.3e-8 cycles from every recorded bin edge)."""
import numpy as np
import pytest

import cube_reference as R
from conftest import gold, gpath

BAND_SIZES = {"b03_10": 87394, "b1_5": 68877}
GRID_BINS = (20, 24, 24, 24, 20, 16)


def _gti():
    return np.array([[10.0, 20.0], [30.0, 40.0], [50.0, 60.0]])


def test_update_gti_four_cases():
    from crimp_amd.plot_pps import update_gti
    g = _gti()
    assert update_gti(g, None, None) is g
    np.testing.assert_array_equal(update_gti(_gti(), 35.0, None), [[35.0, 40.0], [50.0, 60.0]])
    np.testing.assert_array_equal(update_gti(_gti(), 25.0, None), [[30.0, 40.0], [50.0, 60.0]])  # in a gap: no move
    np.testing.assert_array_equal(update_gti(_gti(), None, 35.0), [[10.0, 20.0], [30.0, 35.0]])
    np.testing.assert_array_equal(update_gti(_gti(), None, 45.0), [[10.0, 20.0], [30.0, 40.0]])
    np.testing.assert_array_equal(update_gti(_gti(), 15.0, 55.0), [[15.0, 20.0], [30.0, 40.0], [50.0, 55.0]])
    np.testing.assert_array_equal(update_gti(_gti(), 20.0, 50.0), [[30.0, 40.0]])  # rows touching a bound go
    np.testing.assert_array_equal(update_gti(_gti(), 32.0, 38.0), [[32.0, 38.0]])
    np.testing.assert_array_equal(g, _gti())  # the caller's table is not written to


def test_golden_sums_equal_band_sizes():
    g = gold("plotpps_1e2259.npz")
    for name, (t, e) in R.bands().items():
        n = BAND_SIZES[name]
        assert t.size == n and int(g[name + "_n"]) == n
        assert g[name + "_pp"].shape == (100,) and g[name + "_pp"].sum() == n
        assert g[name + "_phase_energy"].shape == (64, 24) and g[name + "_phase_energy"].sum() == n
        assert g[name + "_phase_time"].shape == (32, 12) and g[name + "_phase_time"].sum() == n
        assert g[name + "_grid"].shape == (6, sum(GRID_BINS))
        assert g[name + "_grid"].sum() == n - int(g[name + "_grid_dropped"])
        # the half-open last tiles drop the latest photon, and the photons at the top energy edge
        assert int(g[name + "_grid_dropped"]) == 1 + int(g[name + "_grid_top_energy"])
        assert g[name + "_before_after"].shape == (2, 48)
        ba = float(g[name + "_ba_epoch"])
        w = float(g[name + "_ba_window"])
        assert g[name + "_before_after"][0].sum() == ((t >= ba - w) & (t <= ba)).sum()
        assert g[name + "_before_after"][1].sum() == ((t >= ba) & (t <= ba + w)).sum()
        assert (t == ba).any()  # the shared epoch is a photon's own time: it counts in both windows
    assert int(g["b03_10_grid_top_energy"]) >= 1  # the 10 keV photons really fall out of the 0.3-10 keV grid


@pytest.fixture(scope="module")
def folded_bands():
    from oracle import oracle as O
    return {name: (t, e, O.calcphase(t, gpath("1e2259.par"))[1]) for name, (t, e) in R.bands().items()}


def test_bin_rule_restatement_equals_histogram2d(folded_bands):
    """cube_reference.cube is np.histogram2d / np.histogram on the fixture's own columns and edges, and reproduces the
    golden arrays from the oracle's phases."""
    g = gold("plotpps_1e2259.npz")
    for name, (t, e, ph) in folded_bands.items():
        pe = np.linspace(0.0, 1, 65)
        ee = np.logspace(np.log10(e.min()), np.log10(e.max()), 25)
        np.testing.assert_array_equal(ee, g[name + "_energy_edges24"])
        H = np.histogram2d(ph, e, bins=[pe, ee])[0]
        mine = R.cube(ph, [pe], y=e, y_edges=ee).T
        np.testing.assert_array_equal(mine, H)
        np.testing.assert_array_equal(mine, g[name + "_phase_energy"])
        pt = np.linspace(0.0, 1, 33)
        te = np.linspace(t.min(), t.max(), 13)
        mine = R.cube(ph, [pt], y=t, y_edges=te).T
        np.testing.assert_array_equal(mine, np.histogram2d(ph, t, bins=[pt, te])[0])
        np.testing.assert_array_equal(mine, g[name + "_phase_time"])
        np.testing.assert_array_equal(R.cube(ph, [np.linspace(0, 1, 101)])[0], g[name + "_pp"])
        te6 = np.linspace(t.min(), t.max(), 7)
        ee6 = np.logspace(np.log10(e.min()), np.log10(e.max()), 7)
        cols = [np.linspace(0, 1, k + 1) for k in GRID_BINS]
        np.testing.assert_array_equal(R.cube(ph, cols, y=t, y_edges=te6, z=e, z_edges=ee6, open_y=True, open_z=True),
                                      g[name + "_grid"])


def test_bin_rule_restatement_edge_cases():
    edges = np.array([0.0, 0.25, 0.5, 1.0])
    v = np.array([0.0, 0.25, 1.0, -1e-300, np.nextafter(1.0, 2.0), np.nan, 0.4999999999999999])
    idx, keep = R.axis_bin(v, edges)
    np.testing.assert_array_equal(keep, [True, True, True, False, False, False, True])
    np.testing.assert_array_equal(idx[keep], [0, 1, 2, 1])
    idx, keep = R.axis_bin(v, edges, open_last=True)
    np.testing.assert_array_equal(keep, [True, True, False, False, False, False, True])
    np.testing.assert_array_equal(np.histogram(v[:3], bins=edges)[0], np.bincount(R.axis_bin(v[:3], edges)[0]))


def test_map_scaling_matches_the_description():
    """Row-wise min-max scaling: NaN rows for time slices without data, which the smoothing steps over."""
    from crimp_amd.plot_pps import phase_energy_rate, phase_time_rate
    H = np.array([[4, 0, 2], [8, 0, 2], [6, 0, 5], [4, 0, 3]])  # [phase, time]: the middle time row is empty
    raw = phase_time_rate(H, None)
    np.testing.assert_array_equal(raw[0], [0.0, 1.0, 0.5, 0.0])
    assert np.isnan(raw[1]).all()
    np.testing.assert_array_equal(raw[2], [0.0, 0.0, 1.0, 1.0 / 3.0])
    smooth = phase_time_rate(H, 0.5)
    assert np.isfinite(smooth).all()  # weights from the neighbouring rows reach the empty one
    assert np.isnan(phase_time_rate(np.zeros((4, 3)), [0.5, 0.5])).all()
    pe = phase_energy_rate(H[:, [0, 2]], None)
    np.testing.assert_array_equal(pe[0], [0.0, 1.0, 0.5, 0.0])
    from scipy.ndimage import gaussian_filter
    np.testing.assert_array_equal(phase_energy_rate(H[:, [0, 2]], [0.5, 1.0]),
                                  gaussian_filter(pe, sigma=(0.5, 1.0), mode="nearest"))


def test_console_script_and_public_names():
    """pulseprofile_plots is declared for both setuptools paths, and the module carries the reference's public names
    without importing matplotlib."""
    import importlib
    import os
    import subprocess
    import sys
    from conftest import ROOT
    assert 'pulseprofile_plots = "crimp_amd.plot_pps:main"' in open(os.path.join(ROOT, "pyproject.toml")).read()
    assert "pulseprofile_plots = crimp_amd.plot_pps:main" in open(os.path.join(ROOT, "setup.cfg")).read()
    P = importlib.import_module("crimp_amd.plot_pps")
    for name in ("prep_for_plotting", "update_gti", "plotting_pp", "plotting_phase_energy", "plotting_phase_time",
                 "plotting_pp_grid", "plotting_pp_before_after", "run_plots_from_yaml", "main", "pp_counts",
                 "phase_energy_counts", "phase_time_counts", "pp_grid_counts", "before_after_counts", "profile_cube"):
        assert callable(getattr(P, name)), name
    code = "import sys; sys.path.insert(0, %r); import crimp_amd.plot_pps; print('matplotlib' in sys.modules)" % ROOT
    assert subprocess.check_output([sys.executable, "-c", code], text=True).strip() == "False"
