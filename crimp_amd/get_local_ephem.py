"""Local [F0, F1] ephemerides from sliding windows of ToAs (drop-in for CRIMP's ``get_local_ephem.py``, v2.3.0; the
``localephemerides`` script).

The reference walks the windows and samples each one's (F0, F1) posterior with emcee before it moves on. The windows
are independent, so here the walk comes first (``local_ephem_windows``, host only) and every window's chain then
runs in ONE ``crimp_timing_mcmc`` launch, one workgroup per window (csrc/timing_fit.h).
"""
import argparse

import numpy as np
import pandas as pd

from . import ops
from .ephemIntegerRotation import ephemIntegerRotation
from .fit_toas import load_toas_for_fit, plot_residuals, prior_box, summarize_chain
from .logging_utils import configure_logging, get_logger
from .binarymodels import require_no_binary
from .readtimingmodel import ReadTimingModel
from .timfile import readtimfile
from .utilities_fittoas import DeviceFit, Prior

logger = get_logger(__name__)

MCMC_STEPS, MCMC_BURN, MCMC_WALKERS = 1000, 100, 24  # the per-window sampler settings of get_local_ephem.py:197


def local_ephem_windows(toa_df, parfile, interval_days=90, jump_days=15, t_start=None, t_end=None, min_interval=45):
    """The window walk of generate_local_ephemerides (get_local_ephem.py:104-239), without the fits: every window
    that will be fitted, in order. A window starts at the first ToA at or after the running start, spans at most
    ``interval_days``, ends at its last ToA, and is cut at the first glitch epoch inside it (the walk then resumes
    just after the glitch, otherwise ``jump_days`` later). It is kept when it holds at least 4 ToAs over more than
    ``min_interval`` days. Each entry: the window's ToA table ``toas``, ``span_days``, and ``mid`` / ``F0_mid`` /
    ``F1_mid`` -- the integer-rotation epoch nearest before mid-window and the spin parameters of ``parfile`` there."""
    params = ReadTimingModel(parfile).readfulltimingmodel()[0] if isinstance(parfile, str) else parfile
    require_no_binary(params)  # ValueError: the local fits do not model an orbit
    glitch_epochs = sorted(v for k, v in params.items() if "GLEP_" in k)
    times = toa_df["pulse_ToA"]
    if t_start is None:
        t_start = np.min(times)
    if t_end is None:
        t_end = np.max(times)
    windows = []
    start = t_start
    while start < t_end:
        later = times[times >= start]
        if later.empty:  # nothing left before t_end
            break
        start = later.min()
        end = min(start + interval_days, t_end)
        sel = toa_df.loc[(times >= start) & (times <= end)]
        if sel.empty:
            start += jump_days
            continue
        end = sel["pulse_ToA"].max()
        glitch = next((g for g in glitch_epochs if start < g < end), None)
        if glitch:
            sel = sel.loc[sel["pulse_ToA"] <= glitch]
            end = sel["pulse_ToA"].max()
        span = (end - start) if len(sel) > 0 else 0.0
        if len(sel) >= 4 and span > min_interval:
            eph = ephemIntegerRotation(start + (end - start) / 2.0, parfile)
            windows.append({"toas": sel, "span_days": span, "mid": float(eph["Tmjd_intRotation"]),
                            "F0_mid": float(eph["freq_intRotation"]), "F1_mid": float(eph["freqdot_intRotation"])})
        start = glitch + 1e-5 if glitch else start + jump_days
    return windows


def window_model(win):
    """The flagged model a window is fitted with (get_local_ephem.py:162-176): PEPOCH at the window's reference
    epoch, F0 and F1 there and free, F2..F12 zero and fixed, TRACK -2 (a ``pn`` column is used when present)."""
    names = ["PEPOCH"] + ["F%d" % i for i in range(13)]
    values = [win["mid"], win["F0_mid"], win["F1_mid"]] + [0.0] * 11
    flags = [0, 1, 1] + [0] * 11
    model = {k: {"value": np.float64(v), "flag": f} for k, v, f in zip(names, values, flags)}
    model["TRACK"] = -2
    return model


def window_prior(win):
    """Box prior of a window's corrections: 100 cycles over the span for F0, over the span squared for F1."""
    sec = win["span_days"] * 86400
    return Prior(bounds={"F0": (-100 / sec, 100 / sec), "F1": (-100 / sec ** 2, 100 / sec ** 2)}, initial_guess={})


def generate_local_ephemerides(tim_file, parfile, interval_days=90, jump_days=15, t_start=None, t_end=None,
                               min_interval=45, debug_with_plots=False, outputfile="local_ephemerides",
                               ephem_plot=None, clobber=False, *, seed=None):
    """Local F0, F1 every ``jump_days`` over windows of ``interval_days``, stopping at glitch epochs and resuming after
    them. Returns (and writes to ``outputfile``.txt) a DataFrame TOA_MJD_ref, TOA_MJD_ref_err, F0 (minus the .par
    file's linear trend), F0_err, F1, F1_err, CHI2R, DOF. ``seed`` makes the chains reproducible."""
    logger.info("generate_local_ephemerides: tim_file %s parfile %s interval_days %s jump_days %s t_start %s "
                "t_end %s min_interval %s outputfile %s", tim_file, parfile, interval_days, jump_days, t_start, t_end,
                min_interval, outputfile)
    params = ReadTimingModel(parfile).readfulltimingmodel()[0]
    require_no_binary(params)
    glitch_epochs = sorted(v for k, v in params.items() if "GLEP_" in k)
    windows = local_ephem_windows(readtimfile(tim_file), parfile, interval_days, jump_days, t_start, t_end,
                                  min_interval)
    if not windows:
        logger.warning("No interval made the criteria - try decreasing min_interval and/or increasing interval_days; "
                       "returning empty dataframe")
        return pd.DataFrame([])

    keys = ["F0", "F1"]
    rng = np.random.default_rng(seed)
    kernel_seed = int(rng.integers(0, 2 ** 63)) if seed is None else int(seed)
    problems, models, p0, lo, hi = [], [], [], [], []
    for win in windows:
        model = window_model(win)
        toas = load_toas_for_fit(win["toas"], model)
        prior = window_prior(win)
        blo, bhi = prior_box(prior, keys)
        problems.append(DeviceFit(toas["ToA"], model, keys, toas["phase"], toas["phase_err_cycle"]))
        models.append((model, toas))
        p0.append(rng.uniform(blo, bhi, size=(MCMC_WALKERS, 2)))
        lo.append(blo)
        hi.append(bhi)
    offsets = np.concatenate([[0], np.cumsum([p.x.size for p in problems])]).astype(np.int64)
    chain, logprob, _ = ops.timing_mcmc(np.concatenate([p.x for p in problems]),
                                        np.concatenate([p.y for p in problems]),
                                        np.concatenate([p.yerr for p in problems]),
                                        [p.fit_base for p in problems], [p.wave_base for p in problems],
                                        problems[0].map, np.stack(p0), np.stack(lo), np.stack(hi), MCMC_STEPS,
                                        kernel_seed, offsets=offsets)
    # the residuals of every window's median vector: one likelihood launch for all of them
    summaries = [summarize_chain(chain[i, MCMC_BURN:].reshape(-1, 2), logprob[i, MCMC_BURN:].reshape(-1), keys)
                 for i in range(len(windows))]
    med = np.array([[s[k]["median"] for k in keys] for s in summaries])
    _, mu = ops.timing_nll(np.concatenate([p.x for p in problems]), np.concatenate([p.y for p in problems]),
                           np.concatenate([p.yerr for p in problems]), [p.fit_base for p in problems],
                           [p.wave_base for p in problems], problems[0].map, med[:, None, :], offsets=offsets,
                           want_mu=True)
    rows = []
    for i, (win, (model, toas), s) in enumerate(zip(windows, models, summaries)):
        resid = mu[offsets[i]:offsets[i + 1]]
        if debug_with_plots:
            plot_residuals(toas, resid, plotname=f"residuals_interval_{i}")
        phase, err = toas["phase"].to_numpy(), toas["phase_err_cycle"].to_numpy()
        chi2 = np.sum((phase - resid) ** 2 / err ** 2)
        dof = phase.size - 2
        rows.append({"TOA_MJD_ref": win["mid"], "TOA_MJD_ref_err": win["span_days"] / 2.0,
                     "F0": model["F0"]["value"] - s["F0"]["median"], "F0_err": max(s["F0"]["plus"], s["F0"]["minus"]),
                     "F1": model["F1"]["value"] - s["F1"]["median"], "F1_err": max(s["F1"]["plus"], s["F1"]["minus"]),
                     "CHI2R": chi2 / dof, "DOF": dof})
    df = pd.DataFrame(rows)
    df["F0"] -= params["F0"] + params["F1"] * ((df["TOA_MJD_ref"] - params["PEPOCH"]) * 86400)
    if outputfile is not None:
        df.to_csv(f"{outputfile}.txt", sep="\t", index=True, header=True, mode="w" if clobber else "x")
    else:
        print("No output text file created for local ephemerides.")
    if ephem_plot is not None:
        from .plot_local_ephem import plot_local_ephemerides
        plot_local_ephemerides(df, glitch_epochs, ephem_plot)
    else:
        print("No local ephemerides plot created.")
    return df


def main(argv=None):
    p = argparse.ArgumentParser(description="Module to generate local [F0, F1] ephemerides in a moving average fashion")
    p.add_argument("timfile", help=".tim TOA file", type=str)
    p.add_argument("parfile", help="A tempo2 .par file", type=str)
    p.add_argument("-id", "--interval_days", help="Length of separate time interval (days)", type=float, default=90.)
    p.add_argument("-jd", "--jump_days", help="Shift time interval by (days)", type=float, default=15.)
    p.add_argument("-ts", "--t_start", help="Start from (MJD)", type=float, default=None)
    p.add_argument("-te", "--t_end", help="Stop at (MJD)", type=float, default=None)
    p.add_argument("-mi", "--min_interval", help="Minimum time between first and last ToA in each interval (MJD)",
                   type=float, default=45)
    p.add_argument("-dp", "--debug_with_plots", help="For debugging purposes - plot the ToAs of each interval",
                   default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("-of", "--outputfile", type=str, default="local_ephemerides",
                   help="Name of output .txt file of local ephemerides (default='local_ephemerides'.txt)")
    p.add_argument("-ep", "--ephem_plot", help="Plot of local ephemerides (default=None)", type=str, default=None)
    p.add_argument("-cl", "--clobber", help="Override output .txt file of local ephemerides (default=False)",
                   default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("-v", "--verbose", action="count", default=0, help="WARNING if absent, -v: INFO, -vv: DEBUG")
    a = p.parse_args(argv)
    level = ("WARNING", "INFO", "DEBUG")[min(a.verbose, 2)]
    log_file = f"{a.outputfile}.log" if a.outputfile is not None else "local_ephemerides.log"
    configure_logging(console_level=level, file_path=log_file, file_level="INFO", force=True)
    generate_local_ephemerides(a.timfile, a.parfile, a.interval_days, a.jump_days, a.t_start, a.t_end, a.min_interval,
                               a.debug_with_plots, a.outputfile, a.ephem_plot, a.clobber)


if __name__ == "__main__":
    main()
