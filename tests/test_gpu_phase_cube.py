"""crimp_phase_cube (csrc/phase_cube.h) and the counts functions of crimp_amd/plot_pps.py on the device.

Counts are integers and the rule is exact comparisons, so every check is array_equal: against the reference's golden
arrays (tests/golden/gen_plotpps_golden.py: its phases keep >= 6.3e-8 cycles from every recorded bin edge, the build
folds within 1e-9 cycles of it), against np.histogram2d, and against the NumPy restatement of the bin rule
(tests/cube_reference.py, itself checked against np.histogram2d in tests/test_plot_pps_host.py)."""
import json
import math

import numpy as np
import pandas as pd
import pytest

import cube_reference as R
from conftest import gold, gpath

pytestmark = pytest.mark.gpu
GRID_BINS = (20, 24, 24, 24, 20, 16)


@pytest.fixture(scope="module")
def frames(gpu):
    """The golden observation's two bands as the DataFrames prep_for_plotting builds (TIME, PI, foldedphases)."""
    from crimp_amd.calcphase import calcphase
    out = {}
    for name, (t, e) in R.bands().items():
        out[name] = pd.DataFrame({"TIME": t, "PI": e, "foldedphases": calcphase(t, gpath("1e2259.par"))[1]})
    return out


# ------------------------------------------------------------------ fixture parity
@pytest.mark.parametrize("band", ["b03_10", "b1_5"])
def test_counts_functions_equal_reference_fixture(frames, band):
    from crimp_amd import plot_pps as P
    g, df = gold("plotpps_1e2259.npz"), frames[band]
    cts, edges = P.pp_counts(df, 100)
    np.testing.assert_array_equal(cts, g[band + "_pp"])
    np.testing.assert_array_equal(edges, np.linspace(0, 1, 101))
    H, pe, ee = P.phase_energy_counts(df, 64, 24)
    np.testing.assert_array_equal(H, g[band + "_phase_energy"])
    np.testing.assert_array_equal(ee, g[band + "_energy_edges24"])
    np.testing.assert_array_equal(
        H, np.histogram2d(df["foldedphases"].to_numpy(), df["PI"].to_numpy(), bins=[pe, ee])[0])
    H, pe, te = P.phase_time_counts(df, 32, 12)
    np.testing.assert_array_equal(H, g[band + "_phase_time"])
    np.testing.assert_array_equal(te, g[band + "_time_edges12"])
    cube, te6, ee6, off = P.pp_grid_counts(df)
    np.testing.assert_array_equal(cube, g[band + "_grid"])
    np.testing.assert_array_equal(off, np.concatenate(([0], np.cumsum(GRID_BINS))))
    assert cube.sum() == len(df) - int(g[band + "_grid_dropped"])  # OPEN_LAST drops the latest / top-energy photons
    cts, edges, windows = P.before_after_counts(df, float(g[band + "_ba_epoch"]), float(g[band + "_ba_window"]), 48)
    np.testing.assert_array_equal(cts, g[band + "_before_after"])
    # a pair of windows
    cts2, _, _ = P.before_after_counts(df, float(g[band + "_ba_epoch"]), [float(g[band + "_ba_window"])] * 2, 48)
    np.testing.assert_array_equal(cts2, cts)


# ------------------------------------------------------------------ fused = calcphase, then unfused
def _models():
    from crimp_amd.readtimingmodel import ReadTimingModel
    return {"par": ReadTimingModel(gpath("1e2259.par")).readfulltimingmodel()[0],
            "dict": json.load(open(gpath("timing_model_dict.json")))}


@pytest.mark.parametrize("which", ["par", "dict"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_fused_equals_calcphase_then_unfused(gpu, which, where):
    """With the .par model and with the glitch + wave model, 64 x 24 phase-energy and 32 x 12 phase-time (Y_IS_X and
    y = t passed explicitly): the fused call counts exactly what calcphase followed by the unfused call counts."""
    import torch
    from crimp_amd import _native as N
    from crimp_amd import ops
    from crimp_amd.calcphase import calcphase
    tm = _models()[which]
    t, e = R.bands()["b03_10"]
    if which == "dict":  # the dict's epochs: glitches at 58142 and 58144.5 inside the span
        t = 58140.0 + (t - t[0]) * (6.0 / (t[-1] - t[0]))
    t = t[:50001]  # odd: the pair tail
    e = e[:50001]
    te = np.linspace(t.min(), t.max(), 13)
    ee = np.logspace(np.log10(e.min()), np.log10(e.max()), 25)
    if where == "device":
        t, e = torch.as_tensor(t, device=gpu), torch.as_tensor(e, device=gpu)
    folded = calcphase(t, tm)[1]

    def host(c):
        return c.cpu().numpy() if where == "device" else c
    a = host(ops.phase_cube(t, model=tm, y=e, y_edges=ee, nph=64))
    b = host(ops.phase_cube(folded, y=e, y_edges=ee, nph=64))
    assert a.sum() == 50001 and a.dtype == np.int64
    np.testing.assert_array_equal(a, b)
    a = host(ops.phase_cube(t, model=tm, y_edges=te, nph=32, options=N.CUBE_Y_IS_X))
    b = host(ops.phase_cube(folded, y=t, y_edges=te, nph=32))
    c = host(ops.phase_cube(t, model=tm, y=t, y_edges=te, nph=32))
    assert a.sum() == 50001
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c)
    fh = host(folded)
    np.testing.assert_array_equal(a, R.cube(fh, [np.linspace(0, 1, 33)], y=host(t), y_edges=te))


def test_profile_cube_fused_public_function(gpu, frames):
    """profile_cube on host arrays and on device tensors: the golden phase-time map without an energy axis, the golden
    grid with one (open_last, per-column phase bins), edges from the data as the DataFrame functions form them."""
    import torch
    from crimp_amd.plot_pps import profile_cube
    g, df = gold("plotpps_1e2259.npz"), frames["b03_10"]
    t, e = df["TIME"].to_numpy(), df["PI"].to_numpy()
    for tt, ee in ((t, e), (torch.as_tensor(t, device=gpu), torch.as_tensor(e, device=gpu))):
        cube, te, en, pe = profile_cube(tt, gpath("1e2259.par"), nphase=32, ntimebins=12)
        cube = cube.cpu().numpy() if hasattr(cube, "cpu") else cube
        assert cube.shape == (12, 1, 32) and en is None
        np.testing.assert_array_equal(cube[:, 0, :].T, g["b03_10_phase_time"])
        np.testing.assert_array_equal(te, g["b03_10_time_edges12"])
        cube, te, en, pe = profile_cube(tt, gpath("1e2259.par"), energy=ee, nphase=GRID_BINS, ntimebins=6,
                                        nenergybins=6, open_last=True)
        cube = cube.cpu().numpy() if hasattr(cube, "cpu") else cube
        np.testing.assert_array_equal(cube, g["b03_10_grid"])
        assert len(pe) == 6 and en.size == 7


# ------------------------------------------------------------------ edge semantics
def _edge_values(edges):
    """A few hundred values around one axis: on the first, an inner and the last edge, one ulp either side of them,
    below and above the range, NaN, infinities, and points inside every bin."""
    e = np.asarray(edges, dtype=np.float64)
    special = [e[0], e[len(e) // 2], e[-1], np.nextafter(e[0], -np.inf), np.nextafter(e[0], np.inf),
               np.nextafter(e[len(e) // 2], -np.inf), np.nextafter(e[len(e) // 2], np.inf),
               np.nextafter(e[-1], -np.inf), np.nextafter(e[-1], np.inf), e[0] - 1.0, e[-1] + 1.0, np.nan, np.inf,
               -np.inf]
    inside = np.concatenate([np.linspace(e[i], e[i + 1], 7) for i in range(len(e) - 1)])
    return np.concatenate([special, inside, e])


@pytest.mark.parametrize("upper", [1.0, 2 * math.pi])
def test_edge_semantics_every_axis_open_and_closed(gpu, upper):
    from crimp_amd import _native as N
    from crimp_amd import ops
    rng = np.random.default_rng(12)
    ye = np.logspace(np.log10(0.3), np.log10(10.0), 8)
    ze = np.array([-2.0, -0.5, 0.0, 0.125, 3.0])
    cols = [np.linspace(0, upper, k + 1) for k in (5, 16, 7, 3)]
    pool_p = np.concatenate([_edge_values(c) for c in cols])
    pool_y, pool_z = _edge_values(ye), _edge_values(ze)
    n = 701
    # the first values walk the special cases of one axis with the other two safely inside; the rest mix all three
    ph = rng.choice(pool_p, n)
    y = rng.choice(pool_y, n)
    z = rng.choice(pool_z, n)
    k, ky, kz = len(pool_p), len(pool_y), len(pool_z)
    ph[:k], y[:k], z[:k] = pool_p, 1.0, rng.choice(ze[:-1] + 0.01, k)
    ph[k:k + ky], y[k:k + ky], z[k:k + ky] = 0.3, pool_y, 0.01
    ph[k + ky:k + ky + kz], y[k + ky:k + ky + kz], z[k + ky:k + ky + kz] = 0.3, 1.0, pool_z
    assert k + ky + kz < n and (ph == upper).any() and np.isnan(ph).any()
    kept = {}
    for opts in range(16):
        if opts & N.CUBE_Y_IS_X:
            continue
        oy, oz, op = bool(opts & N.CUBE_Y_OPEN_LAST), bool(opts & N.CUBE_Z_OPEN_LAST), bool(opts & N.CUBE_PH_OPEN_LAST)
        got = ops.phase_cube(ph, y=y, y_edges=ye, z=z, z_edges=ze, ph_edges=cols, options=opts)
        want = R.cube(ph, cols, y=y, y_edges=ye, z=z, z_edges=ze, open_y=oy, open_z=oz, open_p=op)
        np.testing.assert_array_equal(got, want)
        kept[opts] = int(got.sum())
    # every option really drops the photons on its axis's last edge
    assert all(kept[o] < kept[0] for o in (N.CUBE_Y_OPEN_LAST, N.CUBE_Z_OPEN_LAST, N.CUBE_PH_OPEN_LAST))
    # one axis at a time, the others absent: phase alone (a phase of exactly `upper` lands in the last bin), y alone
    got = ops.phase_cube(pool_p, ph_edges=cols[1])
    np.testing.assert_array_equal(got, R.cube(pool_p, [cols[1]]))
    assert got[0, -1] >= (pool_p == upper).sum() > 0
    np.testing.assert_array_equal(ops.phase_cube(pool_p, ph_edges=cols[1], options=N.CUBE_PH_OPEN_LAST),
                                  R.cube(pool_p, [cols[1]], open_p=True))
    np.testing.assert_array_equal(ops.phase_cube(np.full(pool_y.size, 0.5 * upper), y=pool_y, y_edges=ye,
                                                 ph_edges=cols[0], options=N.CUBE_Y_OPEN_LAST),
                                  R.cube(np.full(pool_y.size, 0.5 * upper), [cols[0]], y=pool_y, y_edges=ye,
                                         open_y=True))


# ------------------------------------------------------------------ shapes and counting paths
@pytest.fixture(scope="module")
def uniform_photons():
    rng = np.random.default_rng(77)
    n = 300001
    return rng.random(n), rng.uniform(-1.0, 1.0, n), np.exp(rng.uniform(np.log(0.2), np.log(12.0), n))


def test_small_shapes(gpu, uniform_photons):
    import torch
    from crimp_amd import ops
    ph, y, z = uniform_photons
    ye = np.linspace(-0.9, 0.9, 4)
    for n in (0, 1, 2, 3, 511, 513):  # empty, one photon, the odd pair tail, either side of one block's pairs
        got = ops.phase_cube(ph[:n], y=y[:n], y_edges=ye, nph=16)
        np.testing.assert_array_equal(got, R.cube(ph[:n], [np.linspace(0, 1, 17)], y=y[:n], y_edges=ye))
    got = ops.phase_cube(torch.empty(0, dtype=torch.float64, device=gpu), nph=8)
    assert got.shape == (1, 8) and int(got.sum()) == 0
    # device tensors that start 8 bytes off a 16-byte boundary: the scalar-load kernel
    d = torch.as_tensor(ph[:1000], device=gpu)
    dy = torch.as_tensor(y[:1000], device=gpu)
    got = ops.phase_cube(d[1:], y=dy[1:], y_edges=ye, nph=16).cpu().numpy()
    np.testing.assert_array_equal(got, R.cube(ph[1:1000], [np.linspace(0, 1, 17)], y=y[1:1000], y_edges=ye))
    # the same with a z axis of log-spaced edges (the general form of the kernel, scalar loads)
    dz = torch.as_tensor(z[:1000], device=gpu)
    ze = np.logspace(np.log10(0.3), np.log10(10.0), 6)
    got = ops.phase_cube(d[1:], y=dy[1:], y_edges=ye, z=dz[1:], z_edges=ze, nph=16).cpu().numpy()
    np.testing.assert_array_equal(got, R.cube(ph[1:1000], [np.linspace(0, 1, 17)] * 5, y=y[1:1000], y_edges=ye,
                                              z=z[1:1000], z_edges=ze))


def test_many_blocks_and_columns_of_different_bins(gpu, uniform_photons):
    from crimp_amd import _native as N
    from crimp_amd import ops
    ph, y, z = uniform_photons  # 300,001 photons: 587 blocks merge into one cube; odd
    ye = np.linspace(-0.9, 0.9, 6)
    ze = np.logspace(np.log10(0.3), np.log10(10.0), 7)
    cols = [np.linspace(0, 1, k + 1) for k in GRID_BINS]
    got = ops.phase_cube(ph, y=y, y_edges=ye, z=z, z_edges=ze, ph_edges=cols)
    want = R.cube(ph, cols, y=y, y_edges=ye, z=z, z_edges=ze)
    assert 0 < want.sum() < ph.size  # some photons lie outside the y and z ranges
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(ops.phase_cube(ph, y=y, y_edges=ye, z=z, z_edges=ze, nph=GRID_BINS), want)
    # sorted y (a wave of neighbours shares its time row, as event lists do)
    o = np.argsort(y)
    np.testing.assert_array_equal(ops.phase_cube(ph[o], y=y[o], y_edges=ye, z=z[o], z_edges=ze, ph_edges=cols), want)


@pytest.mark.parametrize("spacing", ["linear", "log", "ragged"])
def test_both_lookups_on_every_axis(gpu, uniform_photons, spacing):
    """Every axis with near-uniform edges (estimate and one step), log-spaced edges and ragged edges (binary search,
    3 and 63 bins: one step short of and at a power of two of edges); the phase columns mix the three."""
    from crimp_amd import ops
    ph, y, z = (a[:60001] for a in uniform_photons)
    rng = np.random.default_rng(5)

    def edges(lo, hi, nb):
        if spacing == "linear":
            return np.linspace(lo, hi, nb + 1)
        if spacing == "log":
            return lo + (hi - lo) * (np.logspace(0, 3, nb + 1) - 1.0) / 999.0
        e = np.sort(rng.uniform(lo, hi, nb - 1))
        return np.concatenate(([lo], e, [hi]))
    ye, ze = edges(-0.8, 0.7, 63), edges(0.25, 11.0, 3)
    cols = [edges(0.0, 1.0, 31), np.linspace(0, 1, 9), edges(0.0, 1.0, 64)]
    got = ops.phase_cube(ph, y=y, y_edges=ye, z=z, z_edges=ze, ph_edges=cols)
    np.testing.assert_array_equal(got, R.cube(ph, cols, y=y, y_edges=ye, z=z, z_edges=ze))
    # the phase axis alone in each form, and on the values of its own edges
    v = np.concatenate([ph, cols[2], np.nextafter(cols[2], 2.0), np.nextafter(cols[2], -1.0)])
    np.testing.assert_array_equal(ops.phase_cube(v, ph_edges=cols[2]), R.cube(v, [cols[2]]))
    np.testing.assert_array_equal(ops.phase_cube(y, ph_edges=ye), R.cube(y, [ye]))


def test_few_bin_contention_path(gpu, uniform_photons):
    """1 x 1 x 16: every lane of a wave adds to one of 16 cells (256 LDS copies of the cube, one per thread)."""
    from crimp_amd import ops
    ph = uniform_photons[0]
    got = ops.phase_cube(ph, nph=16)
    assert got.shape == (1, 16)
    np.testing.assert_array_equal(got[0], np.histogram(ph, bins=np.linspace(0, 1, 17))[0])
    one = ops.phase_cube(ph, nph=1)
    assert one.shape == (1, 1) and int(one[0, 0]) == ph.size


@pytest.mark.parametrize("cells", ["lds_limit", "above_lds_limit", "far_above"])
def test_lds_limit_and_global_atomic_path(gpu, uniform_photons, cells):
    """Cubes of exactly CUBE_LDS_BINS cells (the largest counted in LDS, one copy), just above it and far above it
    (global 64-bit atomics), uniformly random photons."""
    from crimp_amd import _native as N
    from crimp_amd import ops
    ph, y, z = uniform_photons
    assert N.CUBE_LDS_BINS == 4096
    ny, nz, nb = {"lds_limit": (16, 8, 32), "above_lds_limit": (17, 8, 32), "far_above": (64, 16, 100)}[cells]
    assert (ny * nz * nb > N.CUBE_LDS_BINS) == (cells != "lds_limit")
    ye = np.linspace(-1.0, 1.0, ny + 1)
    ze = np.logspace(np.log10(0.2), np.log10(12.0), nz + 1)
    cols = [np.linspace(0, 1, nb + 1)] * nz
    got = ops.phase_cube(ph, y=y, y_edges=ye, z=z, z_edges=ze, ph_edges=cols)
    np.testing.assert_array_equal(got, R.cube(ph, cols, y=y, y_edges=ye, z=z, z_edges=ze))
    assert got.sum() == ph.size


def test_timed_kernel_hook(gpu, uniform_photons):
    import torch
    from crimp_amd import _native as N
    from crimp_amd import ops
    d = torch.as_tensor(uniform_photons[0], device=gpu)
    ops.phase_cube(d, nph=32, flags=N.FLAG_TIME_KERNELS)
    assert N.load().crimp_last_kernel_ms() > 0.0


# ------------------------------------------------------------------ errors
def test_argument_errors(gpu):
    from crimp_amd import _native as N
    from crimp_amd import ops
    ph = np.linspace(0.0, 0.99, 50)
    y = np.linspace(0.0, 1.0, 50)
    for bad in ([0.0, 0.5, 0.5, 1.0], [0.0, 0.6, 0.5, 1.0], [0.0, np.nan, 1.0], [0.0, 0.5, np.inf]):
        with pytest.raises(N.CrimpNativeError, match="status -1"):
            ops.phase_cube(ph, y=y, y_edges=bad, nph=8)
        with pytest.raises(N.CrimpNativeError, match="status -1"):
            ops.phase_cube(ph, z=y, z_edges=bad, nph=8)
        with pytest.raises(N.CrimpNativeError, match="status -1"):
            ops.phase_cube(ph, ph_edges=np.array(bad))
    with pytest.raises(N.CrimpNativeError, match="status -1"):  # more than CUBE_MAX_BINS bins on an axis
        ops.phase_cube(ph, y=y, y_edges=np.linspace(0, 1, N.CUBE_MAX_BINS + 2), nph=1)
    with pytest.raises(N.CrimpNativeError, match="status -1"):
        ops.phase_cube(ph, nph=N.CUBE_MAX_BINS + 1)
    with pytest.raises(N.CrimpNativeError, match="status -1"):  # y == NULL with ny != 1
        ops.phase_cube(ph, y_edges=[0.0, 0.5, 1.0], nph=8)
    with pytest.raises(N.CrimpNativeError, match="status -1"):  # z == NULL with nz != 1
        ops.phase_cube(ph, z_edges=[0.0, 0.5, 1.0], nph=[8, 8])
    with pytest.raises(N.CrimpNativeError, match="status -1"):  # Y_IS_X with a y of its own
        ops.phase_cube(ph, y=y, y_edges=[0.0, 0.5, 1.0], nph=8, options=N.CUBE_Y_IS_X)
    with pytest.raises(N.CrimpNativeError, match="status -1"):
        ops.phase_cube(ph, nph=8, options=64)
    with pytest.raises(N.CrimpNativeError, match="status -1"):  # more phase edges than CUBE_MAX_PH_EDGES
        ops.phase_cube(ph, z=y, z_edges=np.linspace(0, 1, 5), nph=[600] * 4)
    ok = ops.phase_cube(ph, y=y, y_edges=np.linspace(0, 1, N.CUBE_MAX_BINS + 1), nph=2)  # the limits themselves pass
    assert ok.shape == (N.CUBE_MAX_BINS, 2) and ok.sum() == 50
    assert ops.phase_cube(ph, nph=N.CUBE_MAX_BINS).sum() == 50


# ------------------------------------------------------------------ drawing
def _small_frame(frames):
    return frames["b1_5"].iloc[::7].reset_index(drop=True)


def test_plot_functions_write_pdfs(frames, tmp_path):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    from crimp_amd import plot_pps as P
    df = _small_frame(frames)
    t_mid = float(np.median(df["TIME"]))
    calls = {"pp": lambda p: P.plotting_pp(df, nbrbins=20, plotname=p),
             "pe": lambda p: P.plotting_phase_energy(df, 16, 6, smooth_sigma=[0.5, 1.0], plotname=p),
             "pt": lambda p: P.plotting_phase_time(df, 16, 6, plotname=p),
             "pt_raw": lambda p: P.plotting_phase_time(df, 16, 6, smooth_sigma=None, plotname=p),
             "grid": lambda p: P.plotting_pp_grid(df, 2, 3, nbrbins=(8, 10, 8), plotname=p),
             "ba": lambda p: P.plotting_pp_before_after(df, t_mid, days_window=(0.1, 0.2), nbrbins=12, plotname=p)}
    for name, call in calls.items():
        base = tmp_path / name
        call(str(base))
        out = tmp_path / (name + ".pdf")
        assert out.exists() and out.stat().st_size > 1000, name
    with pytest.raises(ValueError):
        P.plotting_pp_grid(df, 2, 3, nbrbins=(8, 10), plotname=str(tmp_path / "bad"))
    with pytest.raises(ValueError):
        P.plotting_pp_before_after(df, t_mid, days_window=(1, 2, 3), plotname=str(tmp_path / "bad"))


def test_run_plots_from_yaml(frames, tmp_path, capsys):
    pytest.importorskip("matplotlib")
    import matplotlib
    matplotlib.use("Agg")
    from crimp_amd.plot_pps import run_plots_from_yaml
    cfg = tmp_path / "plots.yaml"
    cfg.write_text("plots:\n"
                   "  - type: pp\n"
                   "    params: {nbrbins: 16, plotname: '%s'}\n"
                   "  - type: waterfall\n"
                   "  - type: phase_time\n"
                   "    params: {nphasebins: 8, ntimebins: 4, plotname: '%s'}\n"
                   % (tmp_path / "y_pp", tmp_path / "y_pt"))
    run_plots_from_yaml(str(cfg), _small_frame(frames))
    assert (tmp_path / "y_pp.pdf").stat().st_size > 1000 and (tmp_path / "y_pt.pdf").stat().st_size > 1000
    assert "Unknown plot type 'waterfall'" in capsys.readouterr().out
    bad = tmp_path / "bad.yaml"
    bad.write_text("plots: 3\n")
    with pytest.raises(ValueError):
        run_plots_from_yaml(str(bad), _small_frame(frames))
