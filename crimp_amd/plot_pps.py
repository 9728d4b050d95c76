"""Pulse-profile plots of CRIMP v2.3.0 ``plot_pps.py`` (console script ``pulseprofile_plots``): the pulse profile, the
phase-energy and phase-time maps, a time x energy grid of profiles and the profiles before / after an epoch.

Everything under the drawing is photon counting, and it runs on the MI355X: each ``plotting_*`` function calls a
``*_counts`` function that needs no matplotlib and bins on the device (``ops.phase_cube``, csrc/phase_cube.h) with
edges formed on the host by the reference's expressions. The DataFrame functions bin the columns they are given
(``foldedphases``, ``TIME``, ``PI``), as the reference does. ``profile_cube`` is this build's addition: it folds and
bins MJD times in one pass, for event lists that live on the device and never need their phases written out.

matplotlib is the optional ``plots`` extra and is imported inside the drawing functions only.
"""
from __future__ import annotations

import argparse

import numpy as np

from . import _native as N
from . import ops

DEFAULT_GRID_BINS = (20, 24, 24, 24, 20, 16)  # plot_pps.py:277
PHASE_LABEL = r'$\,\mathrm{Phase\,(cycles)}$'
RATE_LABEL = r'$\,\mathrm{Normalized\,rate}$'


# ------------------------------------------------------------------ event preparation (plot_pps.py:19-74)
def prep_for_plotting(eventfile: str, parfile: str, enelow=0, enehigh=100, t_start=None, t_end=None):
    """(DataFrame TIME [MJD] / PI [keV] / foldedphases [cycles], GTI [MJD]) of an event file: the events inside the
    energy band and the time span, folded with the .par model on the device (plot_pps.py:19-41)."""
    from .calcphase import calcphase
    from .eventfile import EvtFileOps
    evt = EvtFileOps(eventfile)
    df = evt.build_time_energy_df().filtenergy(eneLow=enelow, eneHigh=enehigh).filttime(t_start, t_end).time_energy_df
    gti = update_gti(evt.readGTI()[1], t_start, t_end)
    df["foldedphases"] = calcphase(df["TIME"].to_numpy(), parfile)[1]
    return df, gti


def update_gti(GTI, tstart, tend):
    """The GTI table [[start, stop], ...] cut to [tstart, tend] (plot_pps.py:44-74): rows that end at or before tstart
    or begin at or after tend go, the first start moves up to tstart and the last stop down to tend. With neither
    bound the table comes back as it is; otherwise a cut copy."""
    if tstart is not None:
        GTI = GTI[GTI[:, 1] > tstart]
        if GTI[0, 0] < tstart:
            GTI[0, 0] = tstart
    if tend is not None:
        GTI = GTI[GTI[:, 0] < tend]
        if GTI[-1, -1] > tend:
            GTI[-1, -1] = tend
    return GTI


# ------------------------------------------------------------------ counting (device)
def _column(df, name):
    col = df[name]
    return col.to_numpy() if hasattr(col, "to_numpy") else np.asarray(col)


def _cycle(phases):
    """binphases' upper edge (binphases.py:21-26): 1 for phases in [0, 1], else 2 pi for phases in [0, 2 pi]."""
    ph = np.asarray(phases)
    if ((ph >= 0) & (ph <= 1)).all():
        return 1
    if ((ph >= 0) & (ph <= 2 * np.pi)).all():
        return 2 * np.pi
    raise Exception('Array in not cycle folded between [0,1) or [0, 2*pi)')


def _minmax(values):
    return np.nanmin(values), np.nanmax(values)


def pp_counts(time_energy_phase_df, nbrbins=100):
    """(counts [nbrbins], phase edges): binphases' histogram of the ``foldedphases`` column (plot_pps.py:82)."""
    phases = _column(time_energy_phase_df, "foldedphases")
    edges = np.linspace(0, _cycle(phases), nbrbins + 1, endpoint=True)
    return ops.phase_cube(phases, ph_edges=edges)[0], edges


def phase_energy_counts(time_energy_phase_df, nphasebins=64, nenergybins=24):
    """(H [nphasebins, nenergybins], phase edges, energy edges) = np.histogram2d(phases, energies, bins=[...]) with
    linear phase edges over [0, 1] and log-spaced energy edges from the lowest to the highest PI
    (plot_pps.py:139-149)."""
    phases = _column(time_energy_phase_df, "foldedphases")
    energies = _column(time_energy_phase_df, "PI")
    phase_edges = np.linspace(0.0, 1, nphasebins + 1)
    lo, hi = _minmax(energies)
    energy_edges = np.logspace(np.log10(lo), np.log10(hi), nenergybins + 1)
    cube = ops.phase_cube(phases, y=energies, y_edges=energy_edges, ph_edges=phase_edges)
    return np.ascontiguousarray(cube.T), phase_edges, energy_edges


def phase_time_counts(time_energy_phase_df, nphasebins=32, ntimebins=12):
    """(H [nphasebins, ntimebins], phase edges, time edges) = np.histogram2d(phases, times, bins=[...]), both axes
    linear, the time edges from the first to the last TIME (plot_pps.py:204-214)."""
    phases = _column(time_energy_phase_df, "foldedphases")
    times = _column(time_energy_phase_df, "TIME")
    phase_edges = np.linspace(0.0, 1, nphasebins + 1)
    lo, hi = _minmax(times)
    time_edges = np.linspace(lo, hi, ntimebins + 1)
    cube = ops.phase_cube(phases, y=times, y_edges=time_edges, ph_edges=phase_edges)
    return np.ascontiguousarray(cube.T), phase_edges, time_edges


def _grid_bins(nbrbins, n_energybins):
    if np.isscalar(nbrbins):
        return [int(nbrbins)] * n_energybins
    bins = [int(v) for v in nbrbins]
    if len(bins) != n_energybins:
        raise ValueError("nbrbins: one number, or one per energy column (%d given for %d)" % (len(bins), n_energybins))
    return bins


def pp_grid_counts(time_energy_phase_df, n_timebins=6, n_energybins=6, nbrbins=DEFAULT_GRID_BINS):
    """(counts [n_timebins, S], time edges, energy edges, offsets [n_energybins + 1]): the profile of tile (i, j) is
    counts[i, offsets[j] : offsets[j + 1]], binned with the j-th entry of ``nbrbins`` (plot_pps.py:288-333).

    As in the reference every tile selects [t0, t1) and [e0, e1), the last one too, so the latest and the most
    energetic photons fall out of the grid. The reference settles the phase cycle (1 or 2 pi) tile by tile from the
    tile's own phases; here the whole column settles it once."""
    phases = _column(time_energy_phase_df, "foldedphases")
    times = _column(time_energy_phase_df, "TIME")
    energies = _column(time_energy_phase_df, "PI")
    time_edges = np.linspace(*_minmax(times), n_timebins + 1)
    lo, hi = _minmax(energies)
    lo = max(lo, np.nextafter(0, 1))  # log10 of a zero energy
    energy_edges = np.logspace(np.log10(lo), np.log10(hi), n_energybins + 1)
    bins = _grid_bins(nbrbins, n_energybins)
    upper = _cycle(phases)
    cube = ops.phase_cube(phases, y=times, y_edges=time_edges, z=energies, z_edges=energy_edges,
                          ph_edges=[np.linspace(0, upper, k + 1, endpoint=True) for k in bins],
                          options=N.CUBE_Y_OPEN_LAST | N.CUBE_Z_OPEN_LAST)
    return cube, time_edges, energy_edges, np.concatenate(([0], np.cumsum(bins)))


def _windows(t_mjd, days_window):
    if isinstance(days_window, (list, tuple)):
        if len(days_window) != 2:
            raise ValueError("days_window: a number of days, or a pair (before, after)")
        before, after = float(days_window[0]), float(days_window[1])
    else:
        before = after = float(days_window)
    return [(t_mjd - before, t_mjd), (t_mjd, t_mjd + after)]


def before_after_counts(time_energy_phase_df, t_mjd, days_window=7, nbrbins=48):
    """(counts [2, nbrbins], phase edges [2][nbrbins + 1], windows [(t0, t1), (t0, t1)]): the profiles of the photons
    with t0 <= TIME <= t1 in [t_mjd - w, t_mjd] and [t_mjd, t_mjd + w] (plot_pps.py:447-477). Both windows are closed
    and share t_mjd, so a photon at exactly t_mjd counts in both: one device call per window. A window without
    photons gives a row of zeros."""
    phases = _column(time_energy_phase_df, "foldedphases")
    times = _column(time_energy_phase_df, "TIME")
    windows = _windows(t_mjd, days_window)
    counts = np.zeros((2, nbrbins), dtype=np.int64)
    edges = []
    for row, (t0, t1) in enumerate(windows):
        inside = (times >= t0) & (times <= t1)
        upper = _cycle(phases[inside]) if inside.any() else 1
        edges.append(np.linspace(0, upper, nbrbins + 1, endpoint=True))
        if inside.any():
            counts[row] = ops.phase_cube(phases, y=times, y_edges=np.array([t0, t1]), ph_edges=edges[row])[0]
    return counts, edges, windows


def profile_cube(timeMJD, timMod, energy=None, time_edges=None, energy_edges=None, nphase=32, ntimebins=12,
                 nenergybins=24, open_last=False):
    """Fold and bin in one device pass (crimp_phase_cube with a timing model): the (time, energy, phase) cube of an
    event list, without the phases ever being written out. Not in the reference.

    ``timeMJD``: MJD times, a NumPy array or a torch device tensor; ``timMod``: a timing-model dict or a .par path, as
    calcphase takes it. ``energy`` (optional, same placement as the times): the second axis. ``time_edges`` /
    ``energy_edges``: the bin edges; without them ``ntimebins`` linear bins -- from the lowest to the highest time of a
    host array, from the first to the last element of a device tensor (time-sorted, as event lists are) -- and
    ``nenergybins`` log-spaced bins from the lowest to the highest energy. ``nphase``: phase bins over [0, 1], one
    count or one per energy column. ``open_last``: the grid's rule, the last time and energy bins half-open.

    Returns (counts, time_edges, energy_edges, phase_edges): counts int64 [ntime, nenergy, nphase] -- [ntime, S] with
    the columns side by side when they differ in phase bins -- where the photons are; energy_edges None without
    energies; phase_edges one array, or one per column."""
    from .calcphase import Phases
    ph = Phases(timeMJD, timMod)
    t = ph.timeMJD
    on_device = N._is_torch(t)
    if t.shape[0] == 0 and time_edges is None:
        raise ValueError("no photons and no time_edges")
    if time_edges is None:
        lo, hi = (float(t[0]), float(t[-1])) if on_device else _minmax(t)
        time_edges = np.linspace(lo, hi, ntimebins + 1)
    time_edges = np.asarray(time_edges, dtype=np.float64)
    if energy is not None:
        energy = energy.reshape(-1) if on_device else np.asarray(energy, dtype=np.float64).reshape(-1)
        if energy_edges is None:
            lo, hi = (float(energy.min()), float(energy.max())) if on_device else _minmax(energy)
            lo = max(lo, np.nextafter(0, 1))
            energy_edges = np.logspace(np.log10(lo), np.log10(hi), nenergybins + 1)
        energy_edges = np.asarray(energy_edges, dtype=np.float64)
    else:
        energy_edges = None
    ncol = 1 if energy is None else energy_edges.size - 1
    bins = _grid_bins(nphase, ncol)
    phase_edges = [np.linspace(0.0, 1, k + 1) for k in bins]
    options = N.CUBE_Y_IS_X | ((N.CUBE_Y_OPEN_LAST | N.CUBE_Z_OPEN_LAST) if open_last else 0)
    cube = ops.phase_cube(t, model=ph.timModParam, y_edges=time_edges, z=energy, z_edges=energy_edges,
                          ph_edges=phase_edges, options=options)
    if len(set(bins)) == 1:
        cube = cube.reshape(time_edges.size - 1, ncol, bins[0])
        phase_edges = phase_edges[0]
    return cube, time_edges, energy_edges, phase_edges


# ------------------------------------------------------------------ scaling of the maps (host, a few KB)
def _smooth_sigma(smooth_sigma):
    return tuple(smooth_sigma) if isinstance(smooth_sigma, list) else smooth_sigma


def phase_energy_rate(H, smooth_sigma=0.5):
    """The phase-energy map's colour values [nenergy, nphase] (plot_pps.py:154-165): every energy row scaled to its own
    minimum and maximum, then one Gaussian filter over both axes (sigma a float or [sigma_energy, sigma_phase], edge
    mode 'nearest'); None: no filter."""
    rows = np.asarray(H, dtype=float).T
    low = rows.min(axis=1, keepdims=True)
    high = rows.max(axis=1, keepdims=True)
    rate = (rows - low) / (high - low)
    if smooth_sigma is not None:
        from scipy.ndimage import gaussian_filter
        rate = gaussian_filter(rate, sigma=_smooth_sigma(smooth_sigma), mode='nearest')
    return rate


def phase_time_rate(H, smooth_sigma=0.5):
    """The phase-time map's colour values [ntime, nphase] (plot_pps.py:217-243): row-wise min-max scaling with NaN for
    a flat row (a time slice without data), and a Gaussian filter that steps over the gaps: the scaled map (NaN as 0)
    and the mask of its finite cells are filtered alike and divided; NaN stays where the filtered mask is 0."""
    rows = np.asarray(H, dtype=float).T
    low = rows.min(axis=1, keepdims=True)
    span = rows.max(axis=1, keepdims=True) - low
    rate = np.full_like(rows, np.nan, dtype=float)
    np.divide(rows - low, span, out=rate, where=span != 0)
    if smooth_sigma is not None:
        from scipy.ndimage import gaussian_filter
        sigma = _smooth_sigma(smooth_sigma)
        finite = np.isfinite(rate)
        filled = gaussian_filter(np.where(finite, rate, 0.0).astype(float), sigma=sigma, mode='nearest')
        weight = gaussian_filter(finite.astype(float), sigma=sigma, mode='nearest')
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = filled / weight
        rate = np.where(weight > 0, ratio, np.nan)
    return rate


# ------------------------------------------------------------------ drawing (matplotlib)
def _pyplot():
    try:
        import matplotlib.pyplot as plt
    except ImportError as e:  # pragma: no cover - depends on the installation
        raise ImportError("the pulse-profile plots draw with matplotlib (pip install crimp-amd[plots])") from e
    return plt


def _finish(plt, fig, plotname):
    if plotname is None:
        plt.show()
    else:
        fig.savefig("%s.pdf" % plotname, format="pdf", dpi=300, bbox_inches="tight")
    plt.close(fig)


def _two_cycles(edges, counts):
    """(x, normalised rate, its error) over two cycles: bin centres, counts / mean and sqrt(counts) / mean."""
    edges = np.asarray(edges)
    cycle = edges[-1]
    centres = (np.linspace(0, cycle, counts.size, endpoint=False)) + (cycle / counts.size) / 2
    cts = counts.astype(float)
    mean = cts.mean()
    second = 2 * np.pi if np.max(centres) > 1 else 1.0
    return (np.append(centres, centres + second), np.append(cts / mean, cts / mean),
            np.append(np.sqrt(cts) / mean, np.sqrt(cts) / mean), second)


def _axes(plt, rows, cols, size):
    """A white figure of rows x cols panels; (fig, 2-D array of axes)."""
    return plt.subplots(rows, cols, figsize=size, dpi=80, facecolor='w', edgecolor='k', squeeze=False)


def _labels(ax, xlabel, ylabel, size):
    ax.tick_params(axis='both', labelsize=size)
    if xlabel is None:
        ax.set_xticklabels([])
    else:
        ax.set_xlabel(xlabel, fontsize=size)
    if ylabel is None:
        ax.set_yticklabels([])
    else:
        ax.set_ylabel(ylabel, fontsize=size)
    ax.xaxis.offsetText.set_fontsize(size)
    ax.yaxis.offsetText.set_fontsize(size)


def _frame(ax, width):
    for side in ('top', 'bottom', 'left', 'right'):
        ax.spines[side].set_linewidth(width)
    ax.tick_params(width=width)


def _profile(ax, x, rate, err):
    ax.errorbar(x, rate, yerr=err, fmt='ok', zorder=10)
    ax.step(x, rate, 'k+-', where='mid', zorder=10)


def _common_ylim(lows, highs):
    if not lows:
        return 0.85, 1.15
    low, high = min(lows), max(highs)
    pad = 0.05 * (high - low if high > low else 0.3)
    return max(0.0, low - pad), high + pad


def plotting_pp(time_energy_phase_df, nbrbins=100, plotname: str | None = None):
    """The pulse profile of the ``foldedphases`` column over two cycles, rate normalised to its mean, with sqrt(N)
    errors. Shown on screen, or saved as <plotname>.pdf."""
    counts, edges = pp_counts(time_energy_phase_df, nbrbins)
    plt = _pyplot()
    x, rate, err, second = _two_cycles(edges, counts)
    fig, axes = _axes(plt, 1, 1, (12, 6))
    ax = axes[0, 0]
    _labels(ax, PHASE_LABEL, RATE_LABEL, 12)
    ax.ticklabel_format(style='plain', axis='y', scilimits=(0, 0))
    _profile(ax, x, rate, err)
    ax.set_xlim(0.0, 2 * second)
    _frame(ax, 1.5)
    fig.tight_layout()
    _finish(plt, fig, plotname)


def _draw_map(xedges, yedges, rate, ylabel, barlabel, plotname):
    plt = _pyplot()
    fig, axes = _axes(plt, 1, 1, (12, 6))
    ax = axes[0, 0]
    mesh = ax.pcolormesh(xedges, yedges, rate, shading='auto')
    _labels(ax, PHASE_LABEL, ylabel, 12)
    ax.set_yscale('log')
    _frame(ax, 1.5)
    bar = fig.colorbar(mesh, ax=ax)
    bar.ax.tick_params(labelsize=12)
    bar.set_label(barlabel, fontsize=12)
    fig.tight_layout()
    _finish(plt, fig, plotname)


def plotting_phase_energy(time_energy_phase_df, nphasebins=64, nenergybins=24,
                          smooth_sigma: float | list | None = 0.5, plotname: str | None = None):
    """Phase-energy map: phase (cycles) across, energy (log) up, colour = the count rate of every energy row scaled to
    its own minimum and maximum, lightly Gaussian-smoothed unless ``smooth_sigma`` is None."""
    H, phase_edges, energy_edges = phase_energy_counts(time_energy_phase_df, nphasebins, nenergybins)
    _draw_map(phase_edges, energy_edges, phase_energy_rate(H, smooth_sigma), r'$\,\mathrm{Energy}$',
              r'$\,\mathrm{Min-Max\,scaling}$', plotname)


def plotting_phase_time(time_energy_phase_df, nphasebins=32, ntimebins=12,
                        smooth_sigma: float | list | None = 0.5, plotname: str | None = None):
    """Phase-time map: phase (cycles) across, time (MJD) up, colour = min-max scaled count rate of every time row; time
    rows without data stay blank, and the smoothing does not bleed into them."""
    H, phase_edges, time_edges = phase_time_counts(time_energy_phase_df, nphasebins, ntimebins)
    _draw_map(phase_edges, time_edges, phase_time_rate(H, smooth_sigma), r'$\,\mathrm{Time\,(MJD)}$',
              r'$\,\mathrm{Min-Max\,\,Scaling}$', plotname)


def _side_label(ax, text):
    right = ax.twinx()
    right.set_ylabel(text, fontsize=14, rotation=270, labelpad=14)
    right.set_yticks([])
    right.tick_params(right=True, labelright=True, length=0)


def plotting_pp_grid(time_energy_phase_df, n_timebins=6, n_energybins=6, nbrbins=DEFAULT_GRID_BINS,
                     plotname: str | None = None):
    """A grid of pulse profiles, time bins down and (log-spaced) energy bins across, two cycles each with errors and
    one common rate scale; the top row is headed by the energy ranges (keV), the last column carries the time ranges
    (whole MJD) on its right. ``nbrbins``: phase bins, one number or one per energy column. Empty tiles are hidden."""
    cube, time_edges, energy_edges, offsets = pp_grid_counts(time_energy_phase_df, n_timebins, n_energybins, nbrbins)
    upper = _cycle(_column(time_energy_phase_df, "foldedphases"))
    plt = _pyplot()
    fig, axes = _axes(plt, n_timebins, n_energybins, (3.8 * n_energybins, 2.9 * n_timebins))
    tiles, lows, highs = {}, [], []
    for i in range(n_timebins):
        for j in range(n_energybins):
            cts = cube[i, offsets[j]:offsets[j + 1]]
            if cts.sum() <= 0:
                axes[i, j].set_visible(False)
                continue
            tiles[i, j] = _two_cycles(np.linspace(0, upper, cts.size + 1), cts)[:3]
            lows.append(np.nanmin(tiles[i, j][1]))
            highs.append(np.nanmax(tiles[i, j][1]))
    ylim = _common_ylim(lows, highs)
    for i in range(n_timebins):
        for j in range(n_energybins):
            ax = axes[i, j]
            if (i, j) in tiles:
                x, rate, err = tiles[i, j]
                _profile(ax, x, rate, err)
                ax.set_xlim(0.0, np.max(x))
                ax.set_ylim(*ylim)
                _labels(ax, 'Phase (cycles)' if i == n_timebins - 1 else None, 'Norm. rate' if j == 0 else None, 14)
                ax.tick_params(axis='both', length=3)
                _frame(ax, 1.2)
            if i == 0:
                ax.set_title("%.2g - %.2g keV" % (energy_edges[j], energy_edges[j + 1]), fontsize=14, pad=4)
            if j == n_energybins - 1:
                _side_label(ax, "%d - %d MJD" % (int(time_edges[i]), int(time_edges[i + 1])))
    fig.subplots_adjust(hspace=0.02, wspace=0.02)
    _finish(plt, fig, plotname)


def plotting_pp_before_after(time_energy_phase_df, t_mjd: float, days_window: float | list | tuple = 7,
                             nbrbins: int = 48, plotname: str | None = None):
    """Two stacked pulse profiles around ``t_mjd``: the photons of [t_mjd - w, t_mjd] above those of
    [t_mjd, t_mjd + w]; ``days_window`` is w in days, or a pair (before, after). The same bins, two cycles, errors and
    rate scale in both panels; the energy band is whatever the DataFrame was filtered to."""
    counts, edges, windows = before_after_counts(time_energy_phase_df, t_mjd, days_window, nbrbins)
    plt = _pyplot()
    fig, axes = _axes(plt, 2, 1, (8, 6))
    panels, lows, highs = {}, [], []
    for row in range(2):
        if counts[row].sum() <= 0:
            axes[row, 0].set_visible(False)
            continue
        panels[row] = _two_cycles(edges[row], counts[row])[:3]
        lows.append(np.nanmin(panels[row][1]))
        highs.append(np.nanmax(panels[row][1]))
    ylim = _common_ylim(lows, highs)
    for row, (x, rate, err) in panels.items():
        ax = axes[row, 0]
        _profile(ax, x, rate, err)
        ax.set_xlim(0.0, np.max(x))
        ax.set_ylim(*ylim)
        _labels(ax, PHASE_LABEL if row == 1 else None, RATE_LABEL, 12)
        ax.set_title("%d - %d MJD" % (int(windows[row][0]), int(windows[row][1])), fontsize=12, pad=4)
        _frame(ax, 1.5)
    fig.tight_layout()
    _finish(plt, fig, plotname)


# ------------------------------------------------------------------ YAML driver and CLI (plot_pps.py:546-603)
_PLOT_REGISTRY = dict(pp=plotting_pp, phase_energy=plotting_phase_energy, phase_time=plotting_phase_time,
                      pp_grid=plotting_pp_grid, before_after=plotting_pp_before_after)


def run_plots_from_yaml(config_path: str, time_energy_phase_df):
    """Draw, in order, the plots listed in a YAML file: a top-level ``plots`` list of {type: pp | phase_energy |
    phase_time | pp_grid | before_after, params: {keyword arguments of that plotting function}}. An entry that is no
    mapping, an unknown type, or parameters the function does not take are skipped with a printed warning."""
    import yaml
    with open(config_path, "r") as fh:
        plots = (yaml.safe_load(fh) or {}).get("plots", [])
    if not isinstance(plots, list):
        raise ValueError("the YAML file needs a top-level list named 'plots'")
    for number, entry in enumerate(plots, 1):
        if not isinstance(entry, dict):
            print("[WARN] plots[%d] is not a mapping; skipping" % number)
            continue
        kind, params = entry.get("type"), entry.get("params") or {}
        draw = _PLOT_REGISTRY.get(kind)
        if draw is None:
            print("[WARN] Unknown plot type '%s'; skipping" % kind)
            continue
        try:
            draw(time_energy_phase_df, **params)
        except TypeError as e:
            print("[WARN] Failed to run plot '%s' with params %s: %s" % (kind, params, e))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Pulse-profile plots of an event file folded with a timing model "
                                             "(profile, phase-energy and phase-time maps, time x energy grid, "
                                             "before / after an epoch), listed in a YAML file")
    ap.add_argument("eventfile", type=str, help="Event file")
    ap.add_argument("parfile", type=str, help="A tempo2 .par file")
    ap.add_argument("yamlconfig", type=str, default=None,
                    help="YAML file listing the plots to generate and their parameters")
    ap.add_argument("-el", "--enelow", type=float, default=0.3, help="Low energy cut (keV), default=0.3")
    ap.add_argument("-eh", "--enehigh", type=float, default=10, help="High energy cut (keV), default=10")
    ap.add_argument("-ts", "--tstart", type=float, default=40000, help="Use events from tstart (MJD) on")
    ap.add_argument("-te", "--tend", type=float, default=70000, help="Use events up to tend (MJD)")
    ap.add_argument("-op", "--outputplot", type=str, default=None, help="Name of output plot file")
    a = ap.parse_args(argv)
    df, _ = prep_for_plotting(a.eventfile, a.parfile, a.enelow, a.enehigh, a.tstart, a.tend)
    run_plots_from_yaml(a.yamlconfig, df)


if __name__ == '__main__':
    main()
