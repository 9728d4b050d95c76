"""Fit a timing model to the photons themselves (the ``fitphotons`` script; not in the reference).

Free parameters are the ones flagged 1 in the .par file, as for ``fittoas``, and optionally a phase offset ``PHOFF``
(cycles). What is fitted is the correction ``p`` to each (``inject_free_params``' convention: the full model is
``par - p``), on the unbinned template likelihood of every photon folded with the corrected model. Only keys in which
the phase is linear are admitted: F0..F12, GLPH / GLF0 / GLF1 / GLF2 / GLF0D and the WAVE A/B values; GLEP, GLTD and
binary models are refused. The likelihood and the ensemble sampler run on the device: ``crimp_photon_nll`` is the
objective of the minimiser, ``crimp_photon_mcmc`` runs the whole chain (csrc/photon_fit.h).
"""
import argparse
import copy
import re

import numpy as np

from . import ops
from .binarymodels import require_no_binary
from .fit_toas import DeviceSampler, prior_box, summarize_chain
from .logging_utils import get_logger
from .readPPtemplate import readPPtemplate
from .readtimingmodel import ReadTimingModel, patch_miscellaneous, patch_par_values, patch_statistics
from .simulatemodulatedlc import template_parts
from .utilities_fittoas import (initguess_prior_from_yaml, initialize_params, inject_free_params, list_fit_keys,
                                validate_parfile)

logger = get_logger(__name__)

PHOFF = "PHOFF"
_REFUSED = re.compile(r"^(GLEP|GLTD)_\d+$")
_ADMITTED = re.compile(r"^(F([0-9]|1[0-2])|(GLPH|GLF0|GLF1|GLF2|GLF0D)_\d+|WAVE\d+_[AB])$")


def check_photon_keys(keys):
    """ValueError naming the first key the photon likelihood does not fit."""
    for k in keys:
        if _REFUSED.match(k):
            raise ValueError("%s cannot be fitted to photons (the phase is not linear in it): fix it" % k)
        if not _ADMITTED.match(k):
            raise ValueError("%s cannot be fitted to photons (F0..F12, GLPH/GLF0/GLF1/GLF2/GLF0D_j and WAVEj_A/B "
                             "can)" % k)


class PhotonFit:
    """One photon-domain fit problem as the device sees it: the photon times, their folded phases under ``parfile``
    (folded once, on the device), the template with its fixed ``norm`` / ``ampShift`` and the map of the free keys.
    ``keys`` defaults to the flagged ones; ``phoff`` adds the free phase offset PHOFF as the last key."""

    def __init__(self, t_mjd, parfile, tempModPP, keys=None, phoff=False, norm=None, ampShift=1.0):
        require_no_binary(parfile)  # before the validation, which would stop at the BINARY entry's name
        validate_parfile(parfile)
        model_keys = list_fit_keys(parfile) if keys is None else list(keys)
        check_photon_keys(model_keys)
        self.parfile = parfile
        self.model_keys = model_keys
        self.phoff = bool(phoff)
        self.keys = model_keys + ([PHOFF] if self.phoff else [])
        if isinstance(tempModPP, str):
            tempModPP = readPPtemplate(tempModPP)
        model, tnorm, amps, locs, wids = template_parts(tempModPP)
        self.norm = float(tnorm if norm is None else norm)
        self.tpl = ops.make_template(model, amps, locs, wids, amp_shift=float(ampShift))
        self.map = ops.fit_map(model_keys)
        self.par = ops._modeltm(parfile)
        self.t = np.ascontiguousarray(np.asarray(t_mjd, dtype=float).reshape(-1))
        if self.t.size < 1:
            raise ValueError("no photons to fit")
        self.x = np.ascontiguousarray(ops.calcphase(self.t, parfile)[1])

    def _vectors(self, pvec):
        p = np.asarray(pvec, dtype=float)
        return p, np.ascontiguousarray(p.reshape(-1, len(self.keys)))

    def nll(self, pvec):
        """NLL of one vector [D] (a float) or of many [P, D] (an array [P])."""
        p, v = self._vectors(pvec)
        out = ops.photon_nll(self.t, self.x, self.par, self.map, self.tpl, self.norm, v, phoff=self.phoff)
        return float(out[0]) if p.ndim == 1 else out

    def delta(self, pvec):
        """delta = Phi(t; par) - Phi(t; par - p) in cycles, of one vector [n] or of many [P, n]."""
        p, v = self._vectors(pvec)
        _, d = ops.photon_nll(self.t, self.x, self.par, self.map, self.tpl, self.norm, v, phoff=self.phoff,
                              want_delta=True)
        return d[0] if p.ndim == 1 else d

    def mcmc(self, p0, lo, hi, steps, seed):
        """(chain [steps, W, D], logprob [steps, W], accepted [W]) of the device sampler on this problem."""
        return ops.photon_mcmc(self.t, self.x, self.par, self.map, self.tpl, self.norm, p0, lo, hi, steps, seed,
                               phoff=self.phoff)

    def full(self, pvec):
        """The full model of one vector: ``parfile``'s values with the correction applied (PHOFF is not a model key)."""
        p = np.asarray(pvec, dtype=float).reshape(-1)
        full = inject_free_params(copy.deepcopy(self.parfile), p[:len(self.model_keys)], self.model_keys)[1]
        for k, v in self.parfile.items():  # a shape value here: kept even where the ToA fits would zero it
            if k.startswith("GLTD_"):
                full[k] = v["value"]
        return full


def minimize_photon_nll(problem: PhotonFit, p0=None):
    """Maximum-likelihood correction by Nelder-Mead on the device objective (as ``fit_toas.minimize_nll``)."""
    from scipy.optimize import minimize
    p0 = np.zeros(len(problem.keys)) if p0 is None else np.asarray(p0, dtype=float)
    return minimize(lambda p: problem.nll(np.asarray(p, dtype=float).reshape(-1)), p0, method="Nelder-Mead",
                    options={"maxiter": int(1e5)})


def run_photon_mcmc(problem: PhotonFit, prior, steps: int = 10000, burn: int = 500, walkers: int = 32,
                    chain_npy: str | None = None, flat_npy: str | None = None, *, seed=None):
    """Sample the posterior of the free corrections: walkers start uniform inside the prior box (every key of
    ``problem.keys``, PHOFF included, needs bounds) and take ``steps`` stretch moves on the device
    (``crimp_photon_mcmc``). Returns (DeviceSampler, flat post-burn samples, summaries). ``seed`` makes the run
    reproducible; None draws one."""
    keys = problem.keys
    missing = [k for k in keys if k not in prior.bounds]
    if missing:
        raise KeyError("Missing prior bounds for: " + ", ".join(missing))
    rng = np.random.default_rng(seed)
    p0 = np.empty((walkers, len(keys)), dtype=float)
    for i, name in enumerate(keys):
        lo, hi = prior.bounds[name]
        p0[:, i] = rng.uniform(lo, hi, size=walkers)
    kernel_seed = int(rng.integers(0, 2 ** 63)) if seed is None else int(seed)
    lo, hi = prior_box(prior, keys)
    chain, logprob, accepted = problem.mcmc(p0, lo, hi, steps, kernel_seed)
    sampler = DeviceSampler(chain, logprob, accepted)
    if chain_npy:
        np.save(chain_npy, sampler.get_chain())
    discard = max(0, burn)
    flat = sampler.get_chain(discard=discard, flat=True)
    flat_logprob = sampler.get_log_prob(discard=discard, flat=True)
    if flat_npy:
        np.save(flat_npy, flat)
    return sampler, flat, summarize_chain(flat, flat_logprob, keys)


def build_parser():
    p = argparse.ArgumentParser(description="Script to fit a timing model to the photons of an event file")
    p.add_argument("evtfile", help="path to the (barycentred) event file", type=str)
    p.add_argument("parfile", help="Initial timing .par file, with fitting flags (1 following at least one parameter)",
                   type=str)
    p.add_argument("template", help="Parameters of template pulse profile", type=str)
    p.add_argument("newparfile", help="New post-fit .par file", type=str)
    p.add_argument("-el", "--eneLow", type=float, default=0.5, help="Low energy cut (keV, default = 0.5)")
    p.add_argument("-eh", "--eneHigh", type=float, default=10.0, help="High energy cut (keV, default = 10)")
    p.add_argument("-ts", "--t_start", type=float, default=None, help="Start time for fit (MJD)")
    p.add_argument("-te", "--t_end", type=float, default=None, help="End time for fit (MJD)")
    p.add_argument("-iy", "--init_yaml", type=str,
                   help="YAML file mapping parameter names (PHOFF included) to initial starting points and/or bounds")
    p.add_argument("-po", "--phoff", help="Fit a phase offset PHOFF (cycles) beside the flagged parameters",
                   default=False, action=argparse.BooleanOptionalAction)
    p.add_argument("-mc", "--mcmc", help="Sample posteriors with the ensemble sampler", default=False,
                   action=argparse.BooleanOptionalAction)
    p.add_argument("-st", "--mcmc-steps", type=int, default=10000, help="Number of MCMC steps (default = 10000)")
    p.add_argument("-bu", "--mcmc-burn", type=int, default=500,
                   help="Burn-in steps to discard when saving flat chain (default=500)")
    p.add_argument("-wa", "--mcmc-walkers", type=int, default=32, help="Number of walkers (default=32)")
    p.add_argument("-ch", "--chain-npy", type=str, default=None, help="Path to save full chain as .npy (default=None)")
    p.add_argument("-fl", "--flat-npy", type=str, default=None,
                   help="Path to save flattened post burn-in samples as .npy (default=None)")
    p.add_argument("-bf", "--best_fit", help="Which values to write", choices=["median", "map"], type=str,
                   default="map")
    return p


def main(argv=None):
    from .eventfile import EvtFileOps
    parser = build_parser()
    args = parser.parse_args(argv)
    init = ReadTimingModel(args.parfile).readfulltimingmodel()[2]
    ef = EvtFileOps(args.evtfile).build_time_energy_df().filtenergy(eneLow=args.eneLow, eneHigh=args.eneHigh)
    t = ef.time_energy_df["TIME"].to_numpy(dtype=float)
    if args.t_start is not None:
        t = t[t >= args.t_start]
    if args.t_end is not None:
        t = t[t <= args.t_end]
    if t.size == 0:
        parser.error("no photons inside the energy and time cuts")
    problem = PhotonFit(t, init, args.template, phoff=args.phoff)
    keys, nmodel = problem.keys, len(problem.model_keys)
    misc = {"START": t.min(), "FINISH": t.max()}
    if args.mcmc:
        if args.init_yaml is None:
            parser.error("-iy (or --init_yaml) is required when -mc (or --mcmc) is used")
        prior = initguess_prior_from_yaml(args.init_yaml)
        print("Running MCMC on the device...")
        _, _, summaries = run_photon_mcmc(problem, prior, steps=args.mcmc_steps, burn=args.mcmc_burn,
                                          walkers=args.mcmc_walkers, chain_npy=args.chain_npy, flat_npy=args.flat_npy)
        print("Posterior summaries(median - / + 1σ approx using 16th / 84th percentiles):")
        uncertainties = {}
        for name, s in summaries.items():
            print(f"  {name}: {s['median']:.8e} -{s['minus']:.2e} +{s['plus']:.2e}")
            if name != PHOFF:
                uncertainties[name] = max(s["minus"], s["plus"])
        best = np.array([summaries[name][args.best_fit] for name in keys], dtype=float)
        patch_par_values(in_path=args.parfile, out_path=args.newparfile, new_values=problem.full(best),
                         uncertainties=uncertainties)
        label = f"MCMC (posterior {args.best_fit})"
    else:
        p0 = None if args.init_yaml is None else initialize_params(keys, args.init_yaml)
        res = minimize_photon_nll(problem, p0)
        best = np.asarray(res.x, dtype=float)
        patch_par_values(in_path=args.parfile, out_path=args.newparfile, new_values=problem.full(best))
        label = "Maximum Likelihood Estimation"
    print("---------------------------")
    print(f"Wrote new timing model to {args.newparfile} using {label} values")
    if problem.phoff:
        print(f"PHOFF = {best[nmodel]:.8e} cycles")
    print(f"NLL = {problem.nll(best)} over {t.size} photons\n")
    patch_statistics(in_path=args.newparfile, out_path=args.newparfile, new_stats={"NTOA": int(t.size)})
    patch_miscellaneous(in_path=args.newparfile, out_path=args.newparfile, new_misc=misc)


if __name__ == "__main__":
    main()
