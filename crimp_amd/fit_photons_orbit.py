"""Fit a timing model with a binary orbit (BT, ELL1) to the photons themselves (the ``fitphotonsorbit`` script; not in
the reference): the counterpart of ``fit_photons`` for a .par with a ``BINARY`` line, and the
last step of the route photons -> ``searchorbit`` -> refined orbit for a source too faint for ToAs.

Free parameters are the ones flagged 1 in the .par: the spin keys ``fit_photons`` admits (F0..F12, GLPH / GLF0 / GLF1 /
GLF2 / GLF0D, WAVE A/B) and the orbital keys ``fit_orbit`` knows (PB, A1, T0 | TASC, ECC | E, OM, OMDOT, GAMMA, EPS1,
EPS2, PBDOT, A1DOT | XDOT), and optionally a phase offset ``PHOFF`` (cycles). What is fitted is the correction to each,
``full(p)[k] = par[k] - p[k]`` in the .par's unit of the key (PBDOT and A1DOT entries dimensionless always), on the
unbinned template likelihood of every photon folded with the corrected model at its emission time. The likelihood and
the ensemble sampler run on the device (``crimp_photon_orbit_nll``, ``crimp_photon_orbit_mcmc``,
csrc/photon_orbit_fit.h). A vector whose corrected orbit leaves the limits of the delay has NLL = +inf and never
enters a chain.
"""
import copy

import numpy as np

from . import ops
from .fit_orbit import (inject_orbit_params, is_orbit_key, list_orbit_fit_keys, parameter_steps, patch_orbit_par,
                        validate_orbit_parfile)
from .fit_photons import PHOFF, build_parser as _photon_parser, check_photon_keys, run_photon_mcmc
from .logging_utils import get_logger
from .readPPtemplate import readPPtemplate
from .readtimingmodel import ReadTimingModel, patch_miscellaneous, patch_statistics
from .simulatemodulatedlc import template_parts
from .utilities_fittoas import initguess_prior_from_yaml, initialize_params

logger = get_logger(__name__)

_STEP_PHOTONS = 1 << 16   # parameter_steps probes at most this many photons (a stride over the array)


def photon_orbit_keys(parfile, keys=None):
    """The model keys of a fit (default: the flagged ones, in the model's order), checked: orbital keys of the model's
    kind (``fit_orbit.list_orbit_fit_keys``' ValueError) and spin keys the photon likelihood admits
    (``fit_photons.check_photon_keys``' ValueError: GLEP, GLTD and every non-linear key are refused)."""
    validate_orbit_parfile(parfile)
    keys = list_orbit_fit_keys(parfile) if keys is None else list(keys)
    check_photon_keys([k for k in keys if not is_orbit_key(k)])
    return keys


def full_model(parfile, pvec, model_keys):
    """The full model of one vector: ``parfile``'s values with the correction applied, the orbit's as
    ``fit_orbit.inject_orbit_params`` gives them; entries past the model keys (PHOFF) are not read."""
    p = np.asarray(pvec, dtype=float).reshape(-1)
    full = inject_orbit_params(copy.deepcopy(parfile), p[:len(model_keys)], list(model_keys))[1]
    for k, v in parfile.items():  # a shape value here: kept even where the ToA fits would zero it
        if k.startswith("GLTD_"):
            full[k] = v["value"]
    return full


class PhotonOrbitFit:
    """One photon-domain fit problem under an orbit as the device sees it: the photon times, their folded phases under
    ``parfile`` at the emission time (folded once, on the device), the template with its fixed ``norm`` / ``ampShift``
    and the map of the free keys. ``keys`` defaults to the flagged ones; ``phoff`` adds PHOFF as the last key."""

    def __init__(self, t_mjd, parfile, tempModPP, keys=None, phoff=False, norm=None, ampShift=1.0):
        model_keys = photon_orbit_keys(parfile, keys)
        self.parfile = parfile
        self.model_keys = model_keys
        self.phoff = bool(phoff)
        self.keys = model_keys + ([PHOFF] if self.phoff else [])
        if isinstance(tempModPP, str):
            tempModPP = readPPtemplate(tempModPP)
        model, tnorm, amps, locs, wids = template_parts(tempModPP)
        self.norm = float(tnorm if norm is None else norm)
        self.tpl = ops.make_template(model, amps, locs, wids, amp_shift=float(ampShift))
        self.map = ops.orbit_fit_map(model_keys)
        self.par = ops._modeltm(parfile)
        self.t = np.ascontiguousarray(np.asarray(t_mjd, dtype=float).reshape(-1))
        if self.t.size < 1:
            raise ValueError("no photons to fit")
        self.x = np.ascontiguousarray(ops.calcphase(self.t, parfile)[1])

    def _vectors(self, pvec):
        p = np.asarray(pvec, dtype=float)
        return p, np.ascontiguousarray(p.reshape(-1, len(self.keys)))

    def _call(self, v, want_delta=False):
        return ops.photon_orbit_nll(self.t, self.x, self.par, self.map, self.tpl, self.norm, v, phoff=self.phoff,
                                    want_delta=want_delta)

    def nll(self, pvec):
        """NLL of one vector [D] (a float) or of many [P, D] (an array [P]); +inf outside the orbit's limits."""
        p, v = self._vectors(pvec)
        out = self._call(v)
        return float(out[0]) if p.ndim == 1 else out

    def delta(self, pvec):
        """delta = Phi(t; par) - Phi(t; full(p)) in cycles, of one vector [n] or of many [P, n]; +inf rows outside the
        orbit's limits."""
        p, v = self._vectors(pvec)
        _, d = self._call(v, want_delta=True)
        return d[0] if p.ndim == 1 else d

    residuals = delta   # the name fit_orbit.parameter_steps probes a problem by

    def mcmc(self, p0, lo, hi, steps, seed):
        """(chain [steps, W, D], logprob [steps, W], accepted [W]) of the device sampler on this problem."""
        return ops.photon_orbit_mcmc(self.t, self.x, self.par, self.map, self.tpl, self.norm, p0, lo, hi, steps, seed,
                                     phoff=self.phoff)

    def full(self, pvec):
        """The full model of one vector: ``parfile``'s values with the correction applied, the orbit's as
        ``fit_orbit.inject_orbit_params`` gives them (PHOFF is not a model key)."""
        return full_model(self.parfile, pvec, self.model_keys)

    def steps(self, p0=None, target=None):
        """A step per key that moves delta by about ``target`` cycles rms (default 1 / sqrt(n): about the width of the
        likelihood), from ``fit_orbit.parameter_steps`` on a stride of at most 65536 photons; PHOFF's is ``target``."""
        p0 = np.zeros(len(self.keys)) if p0 is None else np.asarray(p0, dtype=float)
        target = 1.0 / np.sqrt(self.t.size) if target is None else float(target)
        probe = copy.copy(self)
        stride = -(-self.t.size // _STEP_PHOTONS)
        probe.t, probe.x = np.ascontiguousarray(self.t[::stride]), np.ascontiguousarray(self.x[::stride])
        probe.keys, probe.phoff = self.model_keys, False
        h = parameter_steps(probe, p0[:len(self.model_keys)], target)
        return np.concatenate([h, [target]]) if self.phoff else h


def minimize_photon_orbit_nll(problem: PhotonOrbitFit, p0=None):
    """Maximum-likelihood correction by Nelder-Mead on the device objective, every parameter in units of its step
    (``PhotonOrbitFit.steps``: the keys span twenty orders of magnitude). ``res.x`` is in the keys' own units,
    ``res.steps`` the units the simplex moved in."""
    from scipy.optimize import minimize
    p0 = np.zeros(len(problem.keys)) if p0 is None else np.asarray(p0, dtype=float)
    h = problem.steps(p0)
    nd = p0.size
    q0 = p0 / h
    simplex = np.vstack([q0, q0 + np.eye(nd)])
    res = minimize(lambda q: problem.nll(np.asarray(q, dtype=float).reshape(-1) * h), q0, method="Nelder-Mead",
                   options={"maxiter": int(1e5), "initial_simplex": simplex, "xatol": 1e-3, "fatol": 1e-7})
    res.x = res.x * h
    res.steps = h
    return res


def run_photon_orbit_mcmc(problem: PhotonOrbitFit, prior, steps: int = 10000, burn: int = 500, walkers: int = 32,
                          chain_npy: str | None = None, flat_npy: str | None = None, *, seed=None):
    """``fit_photons.run_photon_mcmc`` on ``crimp_photon_orbit_mcmc``: walkers start uniform inside the prior box (a
    start outside the orbit's limits has log-probability -inf and is left by the first accepted move). Returns
    (DeviceSampler, flat post-burn samples, summaries)."""
    return run_photon_mcmc(problem, prior, steps=steps, burn=burn, walkers=walkers, chain_npy=chain_npy,
                           flat_npy=flat_npy, seed=seed)


def build_parser():
    p = _photon_parser()
    p.description = "Script to fit a timing model with a binary orbit (BT, ELL1) to the photons of an event file"
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
    problem = PhotonOrbitFit(t, init, args.template, phoff=args.phoff)
    keys, nmodel = problem.keys, len(problem.model_keys)
    misc = {"START": t.min(), "FINISH": t.max()}
    uncertainties = None
    if args.mcmc:
        if args.init_yaml is None:
            parser.error("-iy (or --init_yaml) is required when -mc (or --mcmc) is used")
        prior = initguess_prior_from_yaml(args.init_yaml)
        print("Running MCMC on the device...")
        _, _, summaries = run_photon_orbit_mcmc(problem, prior, steps=args.mcmc_steps, burn=args.mcmc_burn,
                                                walkers=args.mcmc_walkers, chain_npy=args.chain_npy,
                                                flat_npy=args.flat_npy)
        print("Posterior summaries(median - / + 1σ approx using 16th / 84th percentiles):")
        uncertainties = {}
        for name, s in summaries.items():
            print(f"  {name}: {s['median']:.8e} -{s['minus']:.2e} +{s['plus']:.2e}")
            if name != PHOFF:
                uncertainties[name] = max(s["minus"], s["plus"])
        best = np.array([summaries[name][args.best_fit] for name in keys], dtype=float)
        label = f"MCMC (posterior {args.best_fit})"
    else:
        p0 = None if args.init_yaml is None else initialize_params(keys, args.init_yaml)
        best = np.asarray(minimize_photon_orbit_nll(problem, p0).x, dtype=float)
        label = "Maximum Likelihood Estimation"
    patch_orbit_par(args.parfile, args.newparfile, problem.full(best), uncertainties)
    print("---------------------------")
    print(f"Wrote new timing model to {args.newparfile} using {label} values")
    if problem.phoff:
        print(f"PHOFF = {best[nmodel]:.8e} cycles")
    print(f"NLL = {problem.nll(best)} over {t.size} photons\n")
    patch_statistics(in_path=args.newparfile, out_path=args.newparfile, new_stats={"NTOA": int(t.size)})
    patch_miscellaneous(in_path=args.newparfile, out_path=args.newparfile, new_misc=misc)


if __name__ == "__main__":
    main()
