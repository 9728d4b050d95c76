"""NumPy restatement of crimp_phase_cube's bin rule (include/crimp_hip.h), the yardstick of tests/test_gpu_phase_cube.py;
tests/test_plot_pps_host.py checks it against np.histogram2d on the golden observation.

Rule of every axis: bin = np.searchsorted(edges, v, 'right') - 1; v == edges[-1] counts in the last bin unless the axis
is open_last; a value outside the edges or a NaN drops the photon."""
import os

import numpy as np

from conftest import GOLDEN


def axis_bin(v, edges, open_last=False):
    """(bin index, kept mask) of the values v on one axis."""
    v = np.asarray(v, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    nb = edges.size - 1
    idx = np.searchsorted(edges, v, side="right") - 1
    at_last = v == edges[-1]
    keep = (v >= edges[0]) & (v <= edges[-1])
    if open_last:
        keep &= ~at_last
    else:
        idx = np.where(at_last, nb - 1, idx)
    return idx, keep


def cube(ph, ph_cols, y=None, y_edges=None, z=None, z_edges=None, open_y=False, open_z=False, open_p=False):
    """int64 [ny, S] counts; ph_cols: the phase edges of every z column."""
    ph = np.asarray(ph, dtype=np.float64)
    n = ph.size
    keep = np.ones(n, bool)
    iy = np.zeros(n, np.int64)
    iz = np.zeros(n, np.int64)
    ny = nz = 1
    if y is not None:
        iy, k = axis_bin(y, y_edges, open_y)
        keep &= k
        ny = len(y_edges) - 1
    if z is not None:
        iz, k = axis_bin(z, z_edges, open_z)
        keep &= k
        nz = len(z_edges) - 1
    assert len(ph_cols) == nz
    zoff = np.concatenate(([0], np.cumsum([len(c) - 1 for c in ph_cols])))
    out = np.zeros((ny, int(zoff[-1])), dtype=np.int64)
    for j, edges in enumerate(ph_cols):
        b, k = axis_bin(ph, edges, open_p)
        sel = keep & k & (iz == j)
        np.add.at(out, (iy[sel], zoff[j] + b[sel]), 1)
    return out


def bands():
    """The golden observation in the fixture's two bands: {name: (TIME [MJD], PI [keV])}."""
    ev = np.load(os.path.join(GOLDEN, "events_1e2259.npz"))
    tmjd = ev["TIME"] / 86400 + (float(ev["MJDREFI"]) + float(ev["MJDREFF"]))
    ene = ev["PI"].astype(np.float64) * 0.01
    out = {}
    for name, (lo, hi) in {"b03_10": (0.3, 10.0), "b1_5": (1.0, 5.0)}.items():
        keep = (ene >= lo) & (ene <= hi)
        out[name] = (tmjd[keep], ene[keep])
    return out
