"""Generate tests/golden/plotpps_1e2259.npz: the counts behind the reference's pulse-profile plots (plot_pps.py) on the
bundled 1E 2259+586 observation.

Run in the build container, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_plotpps_golden.py

The reference's plot_pps module pulls in astropy through its event-file reader and cannot be imported here, so this
script folds with the reference's calcphase and then applies numpy and the reference's binphases exactly as
plot_pps.py states: np.histogram2d with linspace / logspace edges (:139-149, :204-214), binphases on the
[t0, t1) & [e0, e1) selection of every grid tile (:288-333) and on the two closed windows around an epoch (:447-477).
Inputs: tests/golden/events_1e2259.npz (TIME / 86400 + MJDREFI + MJDREFF, PI * 0.01) and 1e2259.par, in the 0.3-10 keV
band (the CLI default) and the 1-5 keV band. Only result arrays are written.

The device folds within 1e-9 cycles of the reference, so the script asserts that no photon lies within MARGIN cycles
of an edge of any phase binning it records: the fixtures then hold for the device exactly, no photon excused. It
also asserts that no energy lies on an inner edge of the log bins and that every 2-D histogram keeps every photon.
"""
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REF, "src"))
sys.dont_write_bytecode = True

from crimp.calcphase import calcphase  # noqa: E402
from crimp.binphases import binphases  # noqa: E402
import crimp.calcphase as _cp  # noqa: E402
import crimp.binphases as _bp  # noqa: E402

# the repository's own ``crimp`` alias package would shadow the reference: make sure it did not
for _m in (_cp, _bp):
    assert os.path.abspath(_m.__file__).startswith(REF + os.sep), _m.__file__

BANDS = {"b03_10": (0.3, 10.0, 87394), "b1_5": (1.0, 5.0, 68877)}
GRID_BINS = (20, 24, 24, 24, 20, 16)  # plotting_pp_grid's default
MARGIN = 5e-8  # cycles; 50 x the build's agreement with the reference's fold


def edge_margin(phases, nb):
    """Smallest distance (cycles) of a phase to an edge of numpy.linspace(0, 1, nb + 1)."""
    edges = np.linspace(0, 1, nb + 1)
    i = np.clip(np.searchsorted(edges, phases), 1, nb)
    return float(np.minimum(np.abs(phases - edges[i - 1]), np.abs(edges[i] - phases)).min())


def band_fixture(name, times, energies, phases, out):
    n = times.size
    for nb in sorted({100, 64, 32, 48} | set(GRID_BINS)):
        m = edge_margin(phases, nb)
        print(name, "phase bins", nb, "edge margin %.3g" % m)
        assert m >= MARGIN, (name, nb, m)
    out[name + "_n"] = np.int64(n)

    # plotting_pp: binphases(foldedphases, 100)
    out[name + "_pp"] = binphases(phases, 100)["ctsBins"].astype(np.int64)

    # plotting_phase_energy: 64 x 24
    pe = np.linspace(0.0, 1, 64 + 1)
    ee = np.logspace(np.log10(np.nanmin(energies)), np.log10(np.nanmax(energies)), 24 + 1)
    assert not np.isin(energies, ee[1:-1]).any(), "an energy on an inner edge"
    H = np.histogram2d(phases, energies, bins=[pe, ee])[0]
    assert H.sum() == n
    out[name + "_phase_energy"] = H.astype(np.int64)
    out[name + "_energy_edges24"] = ee

    # plotting_phase_time: 32 x 12
    pt = np.linspace(0.0, 1, 32 + 1)
    te = np.linspace(np.nanmin(times), np.nanmax(times), 12 + 1)
    H = np.histogram2d(phases, times, bins=[pt, te])[0]
    assert H.sum() == n
    out[name + "_phase_time"] = H.astype(np.int64)
    out[name + "_time_edges12"] = te

    # plotting_pp_grid: 6 x 6 tiles, [t0, t1) & [e0, e1) each, the default bins per energy column
    te6 = np.linspace(np.nanmin(times), np.nanmax(times), 6 + 1)
    e_min = max(np.nanmin(energies), np.nextafter(0, 1))
    ee6 = np.logspace(np.log10(e_min), np.log10(np.nanmax(energies)), 6 + 1)
    rows = []
    for i in range(6):
        row = []
        for j in range(6):
            sel = (times >= te6[i]) & (times < te6[i + 1]) & (energies >= ee6[j]) & (energies < ee6[j + 1])
            if sel.any():
                row.append(binphases(phases[sel], GRID_BINS[j])["ctsBins"].astype(np.int64))
            else:
                row.append(np.zeros(GRID_BINS[j], dtype=np.int64))
        rows.append(np.concatenate(row))
    grid = np.stack(rows)
    dropped = n - int(grid.sum())
    out[name + "_grid"] = grid
    out[name + "_grid_dropped"] = np.int64(dropped)
    out[name + "_grid_top_energy"] = np.int64((energies == ee6[-1]).sum())
    print(name, "grid keeps", int(grid.sum()), "of", n, "- photons at the top energy edge:",
          int((energies == ee6[-1]).sum()))

    # plotting_pp_before_after: two closed windows that share the epoch -- a photon's own time, so that it counts twice
    t_mjd = float(np.sort(times)[n // 2])
    half = float((np.nanmax(times) - np.nanmin(times)) / 4)
    both = []
    for t0, t1 in ((t_mjd - half, t_mjd), (t_mjd, t_mjd + half)):
        sel = (times >= t0) & (times <= t1)
        assert sel.any()
        both.append(binphases(phases[sel], 48)["ctsBins"].astype(np.int64))
    out[name + "_before_after"] = np.stack(both)
    out[name + "_ba_epoch"] = np.float64(t_mjd)
    out[name + "_ba_window"] = np.float64(half)
    print(name, "before/after", int(both[0].sum()), int(both[1].sum()), "at", t_mjd, "+-", half)


def main():
    ev = np.load(os.path.join(HERE, "events_1e2259.npz"))
    tmjd = ev["TIME"] / 86400 + (float(ev["MJDREFI"]) + float(ev["MJDREFF"]))
    ene = ev["PI"].astype(np.float64) * 0.01
    par = os.path.join(HERE, "1e2259.par")
    out = {}
    for name, (lo, hi, want) in BANDS.items():
        keep = (ene >= lo) & (ene <= hi)
        assert int(keep.sum()) == want, (name, int(keep.sum()))
        t, e = tmjd[keep], ene[keep]
        _, folded = calcphase(t, par)
        band_fixture(name, t, e, np.asarray(folded), out)
    np.savez_compressed(os.path.join(HERE, "plotpps_1e2259.npz"), **out)
    print("wrote plotpps_1e2259.npz", os.path.getsize(os.path.join(HERE, "plotpps_1e2259.npz")), "bytes")


if __name__ == "__main__":
    main()
