"""Drop-in ``simulatemodulatedlc`` and a general event simulator running on the MI355X.

``simulatemodulatedlc`` mirrors CRIMP v2.3.0 ``simulatemodulatedlc.py`` (:19-96): same signature and defaults (plus a
keyword-only ``seed``), the same two printed exposure lines, the same two ``ValueError`` texts, the same truncation
of the exposure to whole cycles and the same return value, a dict of two sorted time arrays in seconds from 0. The
events themselves are drawn on the device by ``crimp_sim_events`` (csrc/sim_events.h) from the process the reference
samples -- a rate that is constant on each of ``nbrPhaseBins`` phase bins, ``srcrate + amp cos(2 pi k / n + pi)`` on
bin k, plus a flat background -- with a seeded counter-based generator instead of NumPy's global RNG: the two agree
in distribution, not draw for draw. There is no NumPy fallback.

``simulate_events`` is the general form (not in the reference): an inhomogeneous Poisson process of rate
``S(frac(phi(t))) + b`` where ``phi`` is ``calcphase``'s phase under any ``.par`` model (F1..., glitches, waves) and
``S`` a pulse-profile template (Fourier, wrapped Cauchy, von Mises) with the fit's ``norm`` / ``phShift`` /
``ampShift``, or a table of step rates. A simulated ``phShift`` is what ``measureToA_*`` returns on the events.
``write_eventfile`` stores simulated events as a FITS event file that ``timeintervalsfortoas`` and ``measuretoas``
read.
"""
import argparse
import math
import os

import numpy as np

from . import _native as N
from . import ops
from .readPPtemplate import readPPtemplate
from .readtimingmodel import ReadTimingModel, get_parameter_value

TWO_PI = 2.0 * math.pi
CANDIDATES_PER_CELL = 192.0  # lam_max * cell length: about three rounds of one wave's 64 candidates
SHAPE_SAMPLES = 1 << 16      # phases on which a shape is checked for a negative rate


def cell_length(lam_max):
    """The cell length (s) the simulator uses for a rate bound ``lam_max``: a pure function of the bound, so that
    shards and repeated calls agree on the cells (and with them on every event)."""
    lam_max = float(lam_max)
    if not (math.isfinite(lam_max) and lam_max > 0.0):
        raise ValueError("the rate bound must be positive and finite")
    return CANDIDATES_PER_CELL / lam_max


def cell_count(span_s, cell_s):
    """Cells of ``cell_s`` seconds that cover [0, span_s), as crimp_sim_events counts them."""
    nc = max(int(math.ceil(span_s / cell_s)), 1)
    while nc > 1 and float(nc - 1) * cell_s >= span_s:
        nc -= 1
    while float(nc) * cell_s < span_s:
        nc += 1
    return nc


def _val(v):
    return float(v["value"] if isinstance(v, dict) and "value" in v else v)


def template_parts(tempModPP):
    """(model, norm, amps, locs, wids) of a template dict (readPPtemplate's, or plain values)."""
    model = str(tempModPP["model"]).lower()
    if model not in N.MODEL_IDS:
        raise ValueError("Unknown template model. Only fourier, cauchy, or vonmises are supported")
    K = len([k for k in tempModPP if str(k).startswith("amp_")])
    amps = [_val(tempModPP["amp_%d" % j]) for j in range(1, K + 1)]
    if model == "fourier":
        locs, wids = [_val(tempModPP["ph_%d" % j]) for j in range(1, K + 1)], None
    else:
        locs = [_val(tempModPP["cen_%d" % j]) for j in range(1, K + 1)]
        wids = [_val(tempModPP["wid_%d" % j]) for j in range(1, K + 1)]
    return model, _val(tempModPP["norm"]), amps, locs, wids


def template_rate(tempModPP, phase, phShift=0.0, ampShift=1.0):
    """Source rate S (counts/s) of a template at folded phases in cycles: the model values of templatemodels.py
    (:64-82, :166-185, :271-290), evaluated on the host."""
    model, norm, amps, locs, wids = template_parts(tempModPP)
    ph = np.asarray(phase, dtype=np.float64)
    y = np.full(ph.shape, norm, dtype=np.float64)
    if model == "fourier":
        for j, (a, p) in enumerate(zip(amps, locs), start=1):
            y += (a * ampShift) * np.cos(j * TWO_PI * ph + p - j * phShift)
        return y
    x = ph * TWO_PI
    if model == "cauchy":
        for a, c, w in zip(amps, locs, wids):
            y += ((a * ampShift) / TWO_PI) * (np.sinh(w) / (np.cosh(w) - np.cos(x - c - phShift)))
        return y
    from scipy.special import i0e
    for a, c, w in zip(amps, locs, wids):
        k = 1.0 / w ** 2  # exp(k cos) / I0(k) with exp(-k) taken out of both: finite for a narrow component too
        y += ((a * ampShift) / (TWO_PI * i0e(k))) * np.exp(k * (np.cos(x - c - phShift) - 1.0))
    return y


def rate_bound(tempModPP, ampShift=1.0, bgrrate=0.0):
    """lam_max of a template: norm + ampShift sum |amp_j| (Fourier), norm + the sum of the components' peaks (wrapped
    Cauchy, von Mises), plus the background. A bound at every phase and every phShift."""
    model, norm, amps, locs, wids = template_parts(tempModPP)
    if model == "fourier":
        return norm + abs(ampShift) * sum(abs(a) for a in amps) + bgrrate
    peaks = 0.0
    for a, w in zip(amps, wids):
        if model == "cauchy":
            pk = ((a * ampShift) / TWO_PI) * (math.sinh(w) / (math.cosh(w) - 1.0))
        else:
            from scipy.special import i0e
            pk = (a * ampShift) / (TWO_PI * float(i0e(1.0 / w ** 2)))  # exp(k) / I0(k) = 1 / i0e(k)
        peaks += max(pk, 0.0)  # a component of negative amplitude is <= 0 everywhere
    return norm + peaks + bgrrate


def check_gti(gti):
    """[ngti, 2] MJD array of sorted, disjoint, half-open intervals (ValueError otherwise), or None."""
    if gti is None:
        return None
    g = np.asarray(gti, dtype=np.float64)
    if g.ndim != 2 or g.shape[1] != 2:
        raise ValueError("gti must be an [n, 2] array of MJD (start, stop) rows")
    if not np.all(np.isfinite(g)):
        raise ValueError("gti holds a non-finite value")
    if np.any(g[:, 1] < g[:, 0]):
        raise ValueError("a GTI ends before it starts")
    if np.any(g[1:, 0] < g[:-1, 1]):
        raise ValueError("the GTIs must be sorted and disjoint")
    return np.ascontiguousarray(g)


def _timing_model(timMod):
    if isinstance(timMod, dict):
        return {k: get_parameter_value(v) for k, v in timMod.items()}
    if isinstance(timMod, (str, os.PathLike)):
        return ReadTimingModel(str(timMod)).readfulltimingmodel()[0]
    raise TypeError("timMod must be a dict or path to a .par file")


def build_shape(tempModPP, phShift=0.0, ampShift=1.0, bgrrate=0.0):
    """The device shape (ops.make_sim_shape) of a template (path or dict) or of a 1-D table of step rates, checked on
    the host: a shape whose rate is negative anywhere on a 2^16-point sample of the phase is refused."""
    bgrrate = float(bgrrate)
    if not (math.isfinite(bgrrate) and bgrrate >= 0.0):
        raise ValueError("the background rate must be finite and >= 0")
    if isinstance(tempModPP, (str, os.PathLike)):
        tempModPP = readPPtemplate(str(tempModPP))
    if isinstance(tempModPP, dict):
        model, norm, amps, locs, wids = template_parts(tempModPP)
        sample = template_rate(tempModPP, np.arange(SHAPE_SAMPLES) / SHAPE_SAMPLES, phShift, ampShift)
        if not np.all(np.isfinite(sample)):
            raise ValueError("the template's rate is not finite")
        if sample.min() < 0.0:
            raise ValueError("the template's rate is negative at phase %.6f (%.6g counts/s)"
                             % (np.argmin(sample) / SHAPE_SAMPLES, sample.min()))
        lam = rate_bound(tempModPP, ampShift, bgrrate)
        tpl = ops.make_template(model, amps, locs, wids, amp_shift=float(ampShift))
        shape = ops.make_sim_shape(template=tpl, norm=norm, ph_shift=float(phShift), bkg=bgrrate, lam_max=lam)
        shape._mean_rate = float(sample.mean()) + bgrrate
        return shape, lam
    steps = np.ascontiguousarray(tempModPP, dtype=np.float64)
    if steps.ndim != 1 or steps.size < 1:
        raise ValueError("a step shape needs a 1-D table of at least one rate")
    if not np.all(np.isfinite(steps)):
        raise ValueError("the step rates are not finite")
    if steps.min() < 0.0:
        raise ValueError("the step rate of bin %d is negative (%.6g counts/s)" % (int(np.argmin(steps)), steps.min()))
    lam = float(steps.max()) + bgrrate
    shape = ops.make_sim_shape(steps=steps, bkg=bgrrate, lam_max=lam)
    shape._mean_rate = float(steps.mean()) + bgrrate
    return shape, lam


def expected_cap(shape, seconds):
    """A buffer size that holds the events of ``seconds`` of good time but for a 6-sigma fluctuation: the mean rate's
    expectation plus 6 sqrt of it (ops.sim_events counts first when it does not suffice)."""
    lam = shape._mean_rate * seconds
    return int(lam + 6.0 * math.sqrt(lam) + 64)


def simulate_events(timMod, tempModPP, tstart, tstop, *, phShift=0.0, ampShift=1.0, bgrrate=0.0, gti=None, seed=0,
                    unit="mjd", offset_s=0.0, device=False, first_cell=0, n_cells=None):
    """Events of rate ``S(frac(phi(t))) + bgrrate`` on [tstart, tstop) MJD, inside ``gti`` ([n, 2] MJD, half-open)
    when given. ``timMod``: a ``.par`` path or dict, as ``calcphase`` takes it; ``tempModPP``: a template path or
    dict, as ``measureToA_*`` takes it (``norm`` in counts/s), or a 1-D array of step rates, one per phase bin.
    Returns {'time', 'is_bgr', 'cell_s', 'n_cells'}: the sorted times -- MJD, or with ``unit='s'`` ``offset_s`` +
    seconds since ``tstart`` --, the background flag of every event, and the cells of the run. ``first_cell`` /
    ``n_cells`` simulate a range of the cells only: shards of one (seed, inputs) concatenate to the whole list
    exactly. ``device``: tensors on the current GPU instead of NumPy arrays."""
    if unit not in ("mjd", "s"):
        raise ValueError("unit must be 'mjd' or 's'")
    tm = _timing_model(timMod)
    tstart, tstop = float(tstart), float(tstop)
    span_s = (tstop - tstart) * 86400.0
    if not (math.isfinite(span_s) and span_s > 0.0):
        raise ValueError("tstop must be later than tstart")
    g = check_gti(gti)
    shape, lam = build_shape(tempModPP, phShift, ampShift, bgrrate)
    if lam <= 0.0:  # nothing to draw: any positive bound gives the empty list
        lam = shape.lam_max = 1.0 / span_s
    cell_s = cell_length(lam)
    total_cells = cell_count(span_s, cell_s)
    t, b, _ = ops.sim_events(tm, shape, tstart, span_s, cell_s, gti=g, seed=seed, first_cell=first_cell,
                             n_cells=-1 if n_cells is None else int(n_cells), out_offset_s=offset_s,
                             days=(unit == "mjd"), device=device or None,
                             cap=expected_cap(shape, span_s) if n_cells is None and first_cell == 0 else None)
    return {"time": t, "is_bgr": b, "cell_s": cell_s, "n_cells": total_cells}


def _sinusoid_setup(freq, srcrate, exposure, pulsedfraction, resolution, nbrPhaseBins):
    """Host-side checks of the drop-in, before any device call: (whole cycles, their exposure in s, step rates)."""
    cycles = int(exposure * freq)  # the exposure is cut down to whole rotations
    t_sim = cycles / freq
    print(f"Requested exposure (s): {exposure:.6f}")
    print(f"Simulation exposure (s): {t_sim:.6f} ({cycles} complete cycles at f = {freq:.6f} Hz)")
    swing = math.sqrt(2.0) * pulsedfraction * srcrate  # amplitude of a sinusoid of that RMS pulsed fraction
    if swing > srcrate:
        raise ValueError("RMS pulse fraction cannot be larger than 1/sqrt(2)")
    n = math.floor(1.0 / (resolution * freq)) if nbrPhaseBins is None else nbrPhaseBins
    if n < 4:
        raise ValueError("nbrPhaseBins is very small. Increase time resolution or set nbrPhaseBins manually")
    n = int(n)
    # bin k holds the rate at its left edge; the minimum is at phase 0 and the peak in the middle of a cycle
    rates = srcrate - swing * np.cos(TWO_PI * np.arange(n) / n)
    return cycles, t_sim, np.maximum(rates, 0.0)


def simulatemodulatedlc(freq, srcrate: float = 1, exposure: float = 10000, pulsedfraction: float = 0.2,
                        bgrrate: float = 0.05, resolution: float = 0.073, nbrPhaseBins=None, *, seed=None):
    """Simulated sinusoidal light curve (simulatemodulatedlc.py:19-96): {'assigned_t_wBgr', 'assigned_t_nobgr'},
    sorted seconds from 0 with and without the background events. ``seed=None`` draws the seed from NumPy's global
    RNG (``np.random.seed`` makes runs repeatable, as it does for the reference)."""
    _, t_sim, rates = _sinusoid_setup(freq, srcrate, exposure, pulsedfraction, resolution, nbrPhaseBins)
    if seed is None:
        seed = int(np.random.randint(0, np.iinfo(np.int64).max, dtype=np.int64))
    if not t_sim > 0:
        return {'assigned_t_wBgr': np.zeros(0), 'assigned_t_nobgr': np.zeros(0)}
    # phase = freq * t from t = 0: PEPOCH at the start of the run, which is MJD 0 so that the seconds are exact
    shape, lam = build_shape(rates, bgrrate=bgrrate)
    if lam <= 0.0:
        lam = shape.lam_max = 1.0 / t_sim
    t, b, _ = ops.sim_events({"PEPOCH": 0.0, "F0": float(freq)}, shape, 0.0, t_sim, cell_length(lam), seed=seed,
                             cap=expected_cap(shape, t_sim))
    return {'assigned_t_wBgr': t, 'assigned_t_nobgr': t[b == 0]}


def write_eventfile(path, time_mjd, gti=None, pi=200, mjdref=(56658, 0.000777592592592593), telescope="NICER"):
    """Simulated events as a FITS event file (eventfile.write_fits): an EVENTS table with TIME (seconds since
    ``mjdref`` = (MJDREFI, MJDREFF)) and PI (a scalar or one per event; NICER's 0.01 keV channels by default), and a
    GTI table (``gti`` [n, 2] MJD; default: one interval from the first to the last event)."""
    from .eventfile import write_fits
    t = np.asarray(time_mjd.cpu().numpy() if N._is_torch(time_mjd) else time_mjd, dtype=np.float64).reshape(-1)
    ref = float(mjdref[0]) + float(mjdref[1])
    sec = (t - ref) * 86400.0
    pis = np.broadcast_to(np.asarray(pi, dtype=np.int32), t.shape)
    if gti is None:
        g = np.array([[t[0], t[-1]]]) if t.size else np.zeros((0, 2))
    else:
        g = check_gti(gti)
    gs = (g - ref) * 86400.0
    kws = {"TELESCOP": telescope, "MJDREFI": int(mjdref[0]), "MJDREFF": float(mjdref[1]), "TIMESYS": "TDB",
           "TSTART": float(gs[0, 0]) if len(gs) else 0.0, "TSTOP": float(gs[-1, 1]) if len(gs) else 0.0}
    write_fits(path, [("EVENTS", [("TIME", "D", sec), ("PI", "J", pis)], kws),
                      ("GTI", [("START", "D", gs[:, 0]), ("STOP", "D", gs[:, 1])], dict(kws))])
    return path


def main(argv=None):
    p = argparse.ArgumentParser(description="Draw a sinusoidally modulated light curve on the device")
    p.add_argument("freq", type=float)
    p.add_argument("-sr", "--srcrate", type=float, default=1.0)
    p.add_argument("-ex", "--exposure", type=float, default=10000.0)
    p.add_argument("-pf", "--pulsedfraction", type=float, default=0.2)
    p.add_argument("-bg", "--bgrrate", type=float, default=0.05)
    p.add_argument("-rs", "--resolution", type=float, default=0.073)
    p.add_argument("-nb", "--nbrPhaseBins", type=int, default=None)
    p.add_argument("--seed", type=int, default=None, help="default: drawn from NumPy's global RNG")
    a = p.parse_args(argv)
    simulatemodulatedlc(a.freq, a.srcrate, a.exposure, a.pulsedfraction, a.bgrrate, a.resolution, a.nbrPhaseBins,
                        seed=a.seed)


if __name__ == '__main__':
    main()
