"""Fit pulse ToAs to a timing model (drop-in for CRIMP's ``fit_toas.py``, v2.3.0; the ``fittoas`` script).

Free parameters are the ones flagged 1 in the .par file (Taylor terms F0..F12, glitch terms, or the WAVE whitening
model); what is fitted is the correction to each, on the phase residuals. The likelihood and the ensemble sampler run
on the device: ``crimp_timing_nll`` is the objective of the scipy minimisers, ``crimp_timing_mcmc`` runs the whole
chain of ``run_mcmc`` in one launch (csrc/timing_fit.h) in place of the reference's emcee loop.
"""
import argparse

import numpy as np
import pandas as pd

from . import ops
from .calcphase import calcphase
from .logging_utils import get_logger
from .binarymodels import require_no_binary
from .readtimingmodel import (ReadTimingModel, get_parameter_value, patch_miscellaneous, patch_par_values,
                              patch_statistics)
from .timfile import PulseToAs, readtimfile
from .utilities_fittoas import *  # noqa: F401,F403  (the reference re-exports these names the same way)
from .utilities_fittoas import (DeviceFit, Prior, initguess_prior_from_yaml, inject_free_params, list_fit_keys,
                                make_nll, model_phase_residuals, validate_parfile)

logger = get_logger(__name__)


def load_toas_for_fit(tim_file_df: pd.DataFrame, parfile: dict, t_start: float | None = None,
                      t_stop: float | None = None, t_mjd_phasewrap: float | None = None,
                      mode: str = "add") -> pd.DataFrame:
    """ToAs of a .tim table as fit input: a DataFrame ['ToA', 'phase', 'phase_err_cycle'], time-sorted, optionally
    cut to [t_start, t_stop]. The phase is calcphase's (on the device) under ``parfile``: minus the pulse number when
    the model has TRACK -2 and the table a ``pn`` column, else folded into [-0.5, 0.5); then mean-subtracted.
    ``t_mjd_phasewrap`` adds (``mode`` 'add') or removes ('subtract') one cycle from each given MJD on.
    ValueError for a model with a binary orbit: these fits do not model it (crimp_amd.fit_orbit does)."""
    require_no_binary(parfile)
    return _load_toas(tim_file_df, parfile, t_start, t_stop, t_mjd_phasewrap, mode)


def _load_toas(tim_file_df, parfile, t_start, t_stop, t_mjd_phasewrap, mode):
    # calcphase evaluates a model with an orbit at the emission time: fit_orbit.load_toas_for_fit comes here directly
    f0 = get_parameter_value(parfile["F0"])
    pt = PulseToAs(tim_file_df)
    pt.time_filter(t_start, t_stop)
    pt.df = pt.df.sort_values("pulse_ToA").reset_index(drop=True)
    toas = pd.to_numeric(pt.df["pulse_ToA"], errors="coerce").to_numpy(dtype=float)
    err_us = pd.to_numeric(pt.df["pulse_ToA_err"], errors="coerce").to_numpy(dtype=float)
    phases, _ = calcphase(toas, parfile)
    if "TRACK" in parfile and get_parameter_value(parfile["TRACK"]) == -2 and "pn" in pt.df.columns:
        phases = phases - pt.df["pn"].to_numpy(dtype=float)
        logger.info("TRACK -2 in the timing model and -pn (pulse number) flags in the .tim file: using those")
    else:
        phases = ((phases + 0.5) % 1.0) - 0.5
        logger.info("Phase folding between [-0.5, 0.5)")
    phases = phases - np.mean(phases)
    out = pd.DataFrame({"ToA": toas, "phase": phases, "phase_err_cycle": (err_us / 1e6) * f0})
    if t_mjd_phasewrap is not None:
        out = add_phasewrap(out, t_mjd_phasewrap, mode=mode)
        out["phase"] -= np.mean(out["phase"])
    return out


def add_phasewrap(toas_to_fit, t_mjd, mode: str = "add") -> pd.DataFrame:
    """Shift the phase of every ToA at or after each MJD in ``t_mjd`` by one cycle (cumulative over the cuts)."""
    cuts = np.atleast_1d(np.array(t_mjd, dtype=float))
    if cuts.size == 0:
        return toas_to_fit
    sign = {"add": 1.0, "subtract": -1.0}.get(mode.lower())
    if sign is None:
        raise ValueError("mode must be 'add' or 'subtract'.")
    crossed = np.searchsorted(cuts, toas_to_fit["ToA"].to_numpy(dtype=float), side="right")
    toas_to_fit["phase"] += sign * crossed
    return toas_to_fit


class DeviceSampler:
    """What ``run_mcmc`` returns in place of an ``emcee.EnsembleSampler``: the chain [steps, walkers, ndim], its
    log-probabilities [steps, walkers] and the accepted moves per walker, with emcee's accessors."""

    def __init__(self, chain, logprob, accepted):
        self.chain, self.logprob, self.accepted = chain, logprob, accepted

    def get_chain(self, discard=0, flat=False):
        c = self.chain[discard:]
        return c.reshape(-1, c.shape[-1]) if flat else c

    def get_log_prob(self, discard=0, flat=False):
        lp = self.logprob[discard:]
        return lp.reshape(-1) if flat else lp

    @property
    def acceptance_fraction(self):
        return self.accepted / float(self.chain.shape[0])


def prior_box(prior: Prior, keys):
    """(lo, hi) arrays of the box prior in the order of ``keys``; a key without bounds is unbounded."""
    lo = np.array([prior.bounds[k][0] if k in prior.bounds else -np.inf for k in keys], dtype=float)
    hi = np.array([prior.bounds[k][1] if k in prior.bounds else np.inf for k in keys], dtype=float)
    return lo, hi


def summarize_chain(flat, flat_logprob, keys):
    """Median, 16/84 half-widths and the maximum a posteriori sample of each parameter (fit_toas.py:192-201)."""
    best = np.argmax(flat_logprob)
    out = {}
    for i, name in enumerate(keys):
        q16, q50, q84 = np.percentile(flat[:, i], [16, 50, 84])
        out[name] = {"median": float(q50), "minus": float(q50 - q16), "plus": float(q84 - q50),
                     "map": float(flat[best, i])}
    return out


def sample_posterior(mcmc, keys: list[str], prior: Prior, steps, burn, walkers, chain_npy, flat_npy, seed):
    """What every ``run_mcmc`` does around its sampler: walkers start uniform inside the prior box, ``mcmc(p0, lo, hi,
    steps, kernel_seed)`` runs one problem's chain on the device (``ops.timing_mcmc`` or ``ops.orbit_mcmc`` on the
    caller's problem), the first ``burn`` steps are discarded and the chains saved where asked. ``seed`` None draws the
    kernel's seed; else it is the kernel's seed too. Returns (sampler, flat post-burn samples, summaries)."""
    ndim = len(keys)
    rng = np.random.default_rng(seed)
    p0 = np.empty((walkers, ndim), dtype=float)
    for i, name in enumerate(keys):
        lo, hi = prior.bounds[name]
        p0[:, i] = rng.uniform(lo, hi, size=walkers)
    kernel_seed = int(rng.integers(0, 2 ** 63)) if seed is None else int(seed)
    lo, hi = prior_box(prior, keys)
    chain, logprob, accepted = mcmc(p0[None], lo[None], hi[None], steps, kernel_seed)
    sampler = DeviceSampler(chain[0], logprob[0], accepted[0])
    if chain_npy:
        np.save(chain_npy, sampler.get_chain())
    discard = max(0, burn)
    flat = sampler.get_chain(discard=discard, flat=True)
    flat_logprob = sampler.get_log_prob(discard=discard, flat=True)
    if flat_npy:
        np.save(flat_npy, flat)
    return sampler, flat, summarize_chain(flat, flat_logprob, keys)


def run_mcmc(x, y, yerr, init_parfile: dict, keys: list[str], prior: Prior, steps: int = 10000, burn: int = 500,
             walkers: int = 32, corner_pdf: str | None = None, chain_npy: str | None = None,
             flat_npy: str | None = None, progress: bool = True, *, seed=None):
    """Sample the posterior of the free parameters: walkers start uniform inside the prior box and take ``steps``
    stretch moves on the device (one ``crimp_timing_mcmc`` launch; ``progress`` has nothing to show). Returns
    (sampler, flat post-burn samples, summaries). ``seed`` makes the run reproducible; None draws one."""
    if corner_pdf is not None:
        try:
            import corner
        except ImportError as e:
            raise ImportError("corner_pdf needs the 'corner' package, which is not installed") from e

    def mcmc(*box_steps_seed):
        prob = DeviceFit(x, init_parfile, keys, y, yerr)
        return ops.timing_mcmc(prob.x, prob.y, prob.yerr, prob.fit_base, prob.wave_base, prob.map, *box_steps_seed)
    sampler, flat, summaries = sample_posterior(mcmc, keys, prior, steps, burn, walkers, chain_npy, flat_npy, seed)
    if corner_pdf is not None:
        import matplotlib.pyplot as plt
        fig = corner.corner(flat, bins=32, smooth=1.5, plot_datapoints=False, fill_contours=True, plot_density=True,
                            show_titles=True, title_fmt=".3g", labels=list(keys), quantiles=[0.16, 0.50, 0.84],
                            fontsize=14)
        fig.tight_layout()
        fig.subplots_adjust(hspace=0.13)
        fig.savefig(corner_pdf + ".pdf", format="pdf", dpi=300)
        plt.close(fig)
    return sampler, flat, summaries


def rms_residual(phaseresid, model_phaseresid):
    return np.sqrt((1 / np.size(phaseresid)) * np.sum((phaseresid - model_phaseresid) ** 2))


def chi2_fit(phaseresid, model_phaseresid, phase_err, freeparameters):
    chi2 = np.sum(np.divide((phaseresid - model_phaseresid) ** 2, phase_err ** 2))
    dof = np.size(phaseresid) - freeparameters
    return {"chi2": chi2, "redchi2": np.divide(chi2, dof), "dof": dof}


def plot_residuals(toas_pre_fit, phase_residuals_post_fit, plotname=None):
    """Two panels over time: the pre-fit residuals with the best-fit model, and data minus model. Shown, or saved
    as ``plotname``.pdf."""
    import matplotlib.pyplot as plt
    fig, axs = plt.subplots(2, 1, figsize=(10, 8), dpi=80, facecolor="w", edgecolor="k", sharex=True,
                            gridspec_kw={"height_ratios": [1, 0.7]})
    t, ph, err = toas_pre_fit["ToA"], toas_pre_fit["phase"], toas_pre_fit["phase_err_cycle"]
    axs[0].errorbar(t, ph, yerr=err, color="k", fmt="o", zorder=0, markersize=8, ls="", alpha=0.5,
                    label="Pre-fit residuals")
    axs[0].plot(t, phase_residuals_post_fit, color="k", linestyle="-", alpha=0.5, zorder=10, label="Best-fit model")
    axs[1].errorbar(t, ph - phase_residuals_post_fit, yerr=err, color="k", fmt="o", zorder=10, markersize=8, ls="",
                    alpha=0.5, label="Post-fit (data-model) residuals")
    axs[1].axhline(0, color="k", linestyle="-", linewidth=2.0, zorder=10, alpha=0.5)
    axs[1].set_xlabel(r"$\,\mathrm{Time\,(MJD)}$", fontsize=14)
    for ax in axs:
        ax.set_ylabel(r"$\,\mathrm{Residuals\,(cycle)}$", fontsize=14)
        ax.tick_params(axis="both", labelsize=14, width=1.5)
        ax.ticklabel_format(style="plain", axis="y", scilimits=(0, 0))
        ax.xaxis.offsetText.set_fontsize(14)
        ax.yaxis.offsetText.set_fontsize(14)
        ax.legend(fontsize=14)
        for side in ("top", "bottom", "left", "right"):
            ax.spines[side].set_linewidth(1.5)
    fig.tight_layout()
    if plotname is None:
        plt.show()
    else:
        fig.savefig(str(plotname) + ".pdf", format="pdf", dpi=300, bbox_inches="tight")
        plt.close(fig)


def minimize_nll(nll, p0, keys):
    """The reference's maximum-likelihood step (fit_toas.py:417-424) on the device objective: BFGS with 3-point
    differences when a wave key is free, Nelder-Mead otherwise."""
    from scipy.optimize import minimize
    if any("wave" in s.lower() for s in keys):
        if any("glep_" in s.lower() for s in keys):
            logger.warning("Fitting a glitch epoch and waves together is discouraged: fix the GLEP, or start close to "
                           "its true value. MCMC is an option but may converge slowly.")
        return minimize(nll, p0, method="BFGS", options={"maxiter": int(1e5)}, tol=1.0e-16, jac="3-point")
    return minimize(nll, p0, method="Nelder-Mead", options={"maxiter": int(1e5)})


def _report_and_patch(args, toas, model_resid, nfree, f0, misc):
    phase = toas["phase"].to_numpy()
    rms = rms_residual(phase, model_resid)
    stats = chi2_fit(phase, model_resid, toas["phase_err_cycle"].to_numpy(), nfree)
    print("Statistics of new best-fit:")
    print(f"RMS residual in cycle = {rms}")
    print(f"RMS residual in seconds = {rms * (1 / f0)} (assuming F0 = {f0} from input .par file)")
    print(f"Chi2 = {stats['chi2']} for {stats['dof']} dof")
    print(f"reduced Chi2 = {stats['redchi2']}\n")
    par_stats = {"CHI2R": stats["redchi2"], "NTOA": len(toas["ToA"]), "TRES": rms * (1 / f0) * 1.0e6,
                 "CHI2R_DOF": stats["dof"]}
    patch_statistics(in_path=args.newparfile, out_path=args.newparfile, new_stats=par_stats)
    patch_miscellaneous(in_path=args.newparfile, out_path=args.newparfile, new_misc=misc)
    print(f"Appended best-fit statistical properties to {args.newparfile} par file\n")


def build_parser():
    p = argparse.ArgumentParser(description="Script to fit ToAs to a timing model")
    p.add_argument("timfile_path", help="path to .tim file", type=str)
    p.add_argument("parfile", help="Initial timing .par file, with fitting flags (1 following at least one parameter)",
                   type=str)
    p.add_argument("newparfile", help="New post-fit .par file", type=str)
    p.add_argument("-ts", "--t_start", type=float, default=None, help="Start time for fit (MJD)")
    p.add_argument("-te", "--t_end", type=float, default=None, help="End time for fit (MJD)")
    p.add_argument("-tm", "--t_mjd", type=float, nargs="+", default=None,
                   help="Shift 1 cycle all ToAs >= t_mjd (MJD) - list of t_mjds is allowed, shift is cumulative")
    p.add_argument("-md", "--mode", choices=["add", "subtract"], default="add",
                   help="Add or subtract 1 cycle as desired at times > each t_mjd")
    p.add_argument("-iy", "--init_yaml", type=str,
                   help="YAML file mapping parameter names to initial starting points and/or bounds")
    p.add_argument("-mc", "--mcmc", help="Sample posteriors with the ensemble sampler", default=False,
                   action=argparse.BooleanOptionalAction)
    p.add_argument("-st", "--mcmc-steps", type=int, default=10000, help="Number of MCMC steps (default = 10000)")
    p.add_argument("-bu", "--mcmc-burn", type=int, default=500,
                   help="Burn-in steps to discard when saving flat chain (default=500)")
    p.add_argument("-wa", "--mcmc-walkers", type=int, default=32, help="Number of walkers (default=32)")
    p.add_argument("-cp", "--corner_plot", type=str, default=None, help="Path to save Corner plot PDF (default=None)")
    p.add_argument("-ch", "--chain-npy", type=str, default=None, help="Path to save full chain as .npy (default=None)")
    p.add_argument("-fl", "--flat-npy", type=str, default=None,
                   help="Path to save flattened post burn-in samples as .npy (default=None)")
    p.add_argument("-bf", "--best_fit", help="Which values to use for residual plot", choices=["median", "map"],
                   type=str, default="map")
    p.add_argument("-rp", "--residual_plot", help="Plot of pre- and post-fit residuals", type=str, default=None)
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    init = ReadTimingModel(args.parfile).readfulltimingmodel()[2]
    f0 = get_parameter_value(init["F0"])
    toas = load_toas_for_fit(readtimfile(args.timfile_path, comment="C"), init, args.t_start, args.t_end, args.t_mjd,
                             args.mode)
    validate_parfile(init)
    misc = {"START": toas["ToA"].min(), "FINISH": toas["ToA"].max()}
    if args.mcmc:
        keys = list_fit_keys(init)
        if args.init_yaml is None:
            parser.error("-iy (or --init_yaml) is required when -mc (or --mcmc) is used")
        prior = initguess_prior_from_yaml(args.init_yaml)
        print("Running MCMC on the device...")
        _, _, summaries = run_mcmc(x=toas["ToA"], y=toas["phase"], yerr=toas["phase_err_cycle"], init_parfile=init,
                                   keys=keys, prior=prior, steps=args.mcmc_steps, burn=args.mcmc_burn,
                                   walkers=args.mcmc_walkers, corner_pdf=args.corner_plot, chain_npy=args.chain_npy,
                                   flat_npy=args.flat_npy, progress=True)
        print("Posterior summaries(median - / + 1σ approx using 16th / 84th percentiles):")
        uncertainties = {}
        for name, s in summaries.items():
            print(f"  {name}: {s['median']:.8e} -{s['minus']:.2e} +{s['plus']:.2e}")
            uncertainties[name] = max(s["minus"], s["plus"])
        which = args.best_fit
        best = np.array([summaries[name][which] for name in keys], dtype=float)
        _, full = inject_free_params(init, best, keys)
        resid = model_phase_residuals(toas["ToA"], init, best, keys)
        plot_residuals(toas, resid, None if args.residual_plot is None else args.residual_plot + "_" + which)
        patch_par_values(in_path=args.parfile, out_path=args.newparfile, new_values=full,
                         uncertainties=uncertainties)
        label = f"MCMC (posterior {which})"
    else:
        nll, p0, keys, init = make_nll(toas["ToA"], toas["phase"], toas["phase_err_cycle"], init, args.init_yaml)
        res = minimize_nll(nll, p0, keys)
        _, full = inject_free_params(init, res.x, keys)
        resid = model_phase_residuals(toas["ToA"], init, res.x, keys)
        plot_residuals(toas, resid, args.residual_plot)
        patch_par_values(in_path=args.parfile, out_path=args.newparfile, new_values=full)
        label = "Maximum Likelihood Estimation"
    print("---------------------------")
    print(f"Wrote new timing model to {args.newparfile} using {label} values\n")
    _report_and_patch(args, toas, resid, len(keys), f0, misc)


if __name__ == "__main__":
    main()
