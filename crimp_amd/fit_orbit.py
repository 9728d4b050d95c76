"""Fit pulse ToAs to a timing model with a binary orbit (BT, ELL1): the counterpart of ``fit_toas`` for a .par with a
``BINARY`` line. Not in the reference; the definition is DESIGN.md section 5.9.

Free parameters are the ones flagged 1 in the .par: the spin keys ``fit_toas`` knows and the orbital keys PB, A1, T0
(BT) or TASC (ELL1), ECC | E, OM, OMDOT, GAMMA (BT), EPS1, EPS2 (ELL1), PBDOT, A1DOT | XDOT. What is fitted is the
correction to each, ``full(p)[k] = par[k] - p[k]``, in the .par's unit of the key; the PBDOT and A1DOT entries of ``p``
are dimensionless always, and the patched .par is written back in the unit convention its own value had. With no
orbital key flagged this is the spin fit under the fixed orbit.

The likelihood and the sampler run on the device (``crimp_orbit_nll``, ``crimp_orbit_mcmc``, csrc/orbit_fit.h). A
vector whose corrected orbit leaves the limits of the delay (PB <= 0, A1 < 0, ECC outside [0, 1), ...) has NLL = +inf
and never enters a chain.
"""

import numpy as np
import pandas as pd

from . import ops
from .binarymodels import _tiny_units, binary_params, has_binary
from .fit_toas import _load_toas, _report_and_patch, build_parser, plot_residuals, sample_posterior
from .logging_utils import get_logger
from .readtimingmodel import BINARY_MODELS, ReadTimingModel, get_parameter_value, patch_par_values
from .timfile import readtimfile
from .utilities_fittoas import (Prior, initguess_prior_from_yaml, initialize_params, inject_free_params, list_fit_keys,
                                validate_parfile)

logger = get_logger(__name__)

ORBIT_KEYS = ("PB", "A1", "T0", "TASC", "ECC", "E", "OM", "OMDOT", "GAMMA", "EPS1", "EPS2", "PBDOT", "A1DOT", "XDOT")
_BT_ONLY = ("T0", "ECC", "E", "OM", "OMDOT", "GAMMA")
_ELL1_ONLY = ("TASC", "EPS1", "EPS2")
_DIMENSIONLESS = ("PBDOT", "A1DOT", "XDOT")
_PAR_ALIASES = {"A1DOT": "XDOT", "ECC": "E"}     # the other name a .par line of the key may carry


def binary_kind(parfile):
    """'BT' or 'ELL1'; ValueError for a model without BINARY or with another one."""
    if not has_binary(parfile):
        raise ValueError("the timing model has no BINARY: fit_toas fits it")
    name = str(get_parameter_value(parfile["BINARY"])).upper()
    if name not in BINARY_MODELS:
        raise ValueError("BINARY %s is not supported: the supported binary models are BT and ELL1" % name)
    return name


def is_orbit_key(key):
    return key in ORBIT_KEYS


def list_orbit_fit_keys(parfile: dict):
    """``list_fit_keys`` of a model with an orbit: the flagged spin keys and the flagged orbital keys, in the model's
    order. ValueError for a flagged key the model's kind does not have (T0, ECC, OM, OMDOT, GAMMA under ELL1; TASC,
    EPS1, EPS2 under BT)."""
    kind = binary_kind(parfile)
    keys = list_fit_keys(parfile)
    wrong = [k for k in keys if k in (_ELL1_ONLY if kind == "BT" else _BT_ONLY)]
    if wrong:
        raise ValueError("BINARY %s has no %s: it cannot be fitted" % (kind, ", ".join(wrong)))
    return keys


def validate_orbit_parfile(parfile):
    """``validate_parfile`` for a model with an orbit: the BINARY entry holds the model's name, not a number; every
    other entry is checked as there, and the base orbit has to lie inside the limits of the delay."""
    kind = binary_kind(parfile)
    validate_parfile({k: v for k, v in parfile.items() if k != "BINARY"})
    list_orbit_fit_keys(parfile)
    binary_params(parfile)
    return kind


def _spin_part(parfile):
    return {k: v for k, v in parfile.items() if k != "BINARY" and k not in ORBIT_KEYS}


def _par_units(key, par_value, dimensionless):
    """A dimensionless PBDOT / A1DOT in the convention of the .par's own value: units of 1e-12 when that value was read
    so (magnitude above 1e-7) and the new one reads back the same way, else the number itself -- unless the number
    itself is above 1e-7, which only units of 1e-12 can hold."""
    in_units = dimensionless / 1e-12
    if abs(dimensionless) > 1e-7 or (abs(float(par_value)) > 1e-7 and abs(in_units) > 1e-7):
        return in_units
    return dimensionless


def inject_orbit_params(parfile, pvec, keys):
    """(fit model, full model) of ``inject_free_params`` for a model with an orbit. The fit model is the spin fit model
    (no orbit). The full model carries the corrected orbit: every orbital key ``par - p`` in the .par's unit, PBDOT
    and A1DOT corrected in dimensionless form and given back in the .par value's own convention; BINARY untouched."""
    pvec = np.asarray(pvec, dtype=float).reshape(-1)
    spin = [(k, d) for k, d in zip(keys, pvec) if not is_orbit_key(k)]
    fit, full = inject_free_params(_spin_part(parfile), np.array([d for _, d in spin]), [k for k, _ in spin])
    for k, v in parfile.items():
        if k == "BINARY" or k in ORBIT_KEYS:
            full[k] = get_parameter_value(v)
    for k, delta in zip(keys, pvec):
        if not is_orbit_key(k):
            continue
        if k not in parfile:
            raise KeyError(f"Parameter '{k}' not found in parfile.")
        base = float(get_parameter_value(parfile[k]))
        if k in _DIMENSIONLESS:
            full[k] = _par_units(k, base, _tiny_units(base) - float(delta))
        else:
            full[k] = base - float(delta)
    return fit, full


class OrbitFit:
    """One fit problem as ``crimp_orbit_nll`` / ``crimp_orbit_mcmc`` see it: the ToAs, the full model with its orbit,
    the two spin bases and the parameter map (the ``DeviceFit`` of a model with an orbit)."""

    def __init__(self, x, parfile, keys, y=None, yerr=None):
        self.keys = list(keys)
        self.x = np.ascontiguousarray(np.asarray(x, dtype=float).reshape(-1))
        self.y = np.zeros_like(self.x) if y is None else np.ascontiguousarray(np.asarray(y, dtype=float).reshape(-1))
        self.yerr = (np.ones_like(self.x) if yerr is None
                     else np.ascontiguousarray(np.asarray(yerr, dtype=float).reshape(-1)))
        if not (self.x.size == self.y.size == self.yerr.size):
            raise ValueError("x, y and yerr differ in length")
        kind = binary_kind(parfile)
        wrong = [k for k in self.keys if k in (_ELL1_ONLY if kind == "BT" else _BT_ONLY)]
        if wrong:
            raise ValueError("BINARY %s has no %s: it cannot be fitted" % (kind, ", ".join(wrong)))
        self.map = ops.orbit_fit_map(self.keys)
        spin_keys = [k for k in self.keys if not is_orbit_key(k)]
        fit, full = inject_free_params(_spin_part(parfile), np.zeros(len(spin_keys)), spin_keys)
        self.fit_base = ops._modeltm(fit)
        self.wave_base = ops._modeltm({k: v for k, v in full.items() if not k.startswith("GL")})
        self.par = ops._modeltm(parfile)

    def _call(self, pvec, want_mu):
        p = np.asarray(pvec, dtype=float)
        return p, ops.orbit_nll(self.x, self.y, self.yerr, self.par, self.fit_base, self.wave_base, self.map,
                                p.reshape(1, -1, len(self.keys)), want_mu=want_mu)

    def nll(self, pvec):
        """NLL of one vector [ndim] (a float) or of many [P, ndim] (an array [P]); +inf outside the orbit's limits."""
        p, out = self._call(pvec, False)
        return float(out[0][0]) if p.ndim == 1 else out[0]

    def residuals(self, pvec):
        """Mean-subtracted model phase residuals of one vector [n] or of many [P, n]."""
        p, (_, mu) = self._call(pvec, True)
        mu = mu.reshape(-1, self.x.size)
        return mu[0] if p.ndim == 1 else mu


def load_toas_for_fit(tim_file_df: pd.DataFrame, parfile: dict, t_start: float | None = None,
                      t_stop: float | None = None, t_mjd_phasewrap: float | None = None,
                      mode: str = "add") -> pd.DataFrame:
    """``fit_toas.load_toas_for_fit`` for a model with an orbit: the phases are calcphase's at the emission time."""
    binary_kind(parfile)
    return _load_toas(tim_file_df, parfile, t_start, t_stop, t_mjd_phasewrap, mode)


def make_nll(x, y, y_err, parfile, yaml_init=None):
    """(nll, p0, keys, parfile) as ``utilities_fittoas.make_nll``: one ``crimp_orbit_nll`` call with P = 1 per value."""
    validate_orbit_parfile(parfile)
    keys = list_orbit_fit_keys(parfile)
    p0 = np.zeros(len(keys)) if yaml_init is None else initialize_params(keys, yaml_init)
    problem = OrbitFit(x, parfile, keys, y, y_err)

    def nll(pvec):
        return problem.nll(np.asarray(pvec, dtype=float).reshape(-1))

    nll.problem = problem
    return nll, p0, keys, parfile


def parameter_steps(problem: OrbitFit, p0, target=None):
    """A step per parameter that moves the model residuals by about ``target`` cycles rms (default: the median ToA
    error): the scale of the minimiser's differences. The keys span twenty orders of magnitude, and the model is close
    to linear in each, so two batched probes settle a step: h -> h * target / rms(mu(p0 + h e_k) - mu(p0))."""
    p0 = np.asarray(p0, dtype=float)
    nd = p0.size
    target = float(np.median(problem.yerr)) if target is None else float(target)
    h = np.full(nd, 1e-12)
    for _ in range(4):
        mu = problem.residuals(np.vstack([p0, p0 + np.diag(h)]))
        rms = np.sqrt(np.mean((mu[1:] - mu[0]) ** 2, axis=1))
        good = np.isfinite(rms) & (rms > 0)
        grow = np.where(good, target / np.where(good, rms, 1.0), 1e3)  # no effect yet (or below rounding): a larger step
        grow = np.where(np.isfinite(rms), grow, 1e-3)                  # outside the orbit's limits: a smaller one
        h = h * np.clip(grow, 1e-6, 1e6)
    return h


def minimize_orbit(problem: OrbitFit, p0):
    """Maximum likelihood of the Gaussian NLL: scipy's least_squares on (y - mu(p)) / yerr, the Jacobian from central
    differences of one batched ``crimp_orbit_nll`` launch (2 ndim vectors), every parameter scaled by its step."""
    from scipy.optimize import least_squares
    p0 = np.asarray(p0, dtype=float)
    nd = p0.size
    h = parameter_steps(problem, p0)

    def fun(q):
        return (problem.y - np.mean(problem.y) - problem.residuals(q * h)) / problem.yerr

    def jac(q):
        p = q * h
        mu = problem.residuals(np.vstack([p + np.diag(h), p - np.diag(h)]))
        return -((mu[:nd] - mu[nd:]) / 2.0 / problem.yerr).T

    res = least_squares(fun, p0 / h, jac=jac, method="lm", xtol=1e-12, ftol=1e-12, gtol=1e-12)
    j = jac(res.x)
    cov = np.linalg.pinv(j.T @ j) * np.outer(h, h)
    res.x = res.x * h
    res.cov = cov
    res.sigma = np.sqrt(np.diag(cov))
    res.nll = problem.nll(res.x)
    return res


def run_mcmc(x, y, yerr, init_parfile: dict, keys: list[str], prior: Prior, steps: int = 10000, burn: int = 500,
             walkers: int = 32, chain_npy: str | None = None, flat_npy: str | None = None, *, seed=None):
    """``fit_toas.run_mcmc`` on ``crimp_orbit_mcmc``: walkers start uniform inside the prior box (a start outside the
    orbit's limits has log-probability -inf and is left by the first accepted move). Returns (sampler, flat post-burn
    samples, summaries)."""
    def mcmc(*box_steps_seed):
        prob = OrbitFit(x, init_parfile, keys, y, yerr)
        return ops.orbit_mcmc(prob.x, prob.y, prob.yerr, prob.par, prob.fit_base, prob.wave_base, prob.map,
                              *box_steps_seed)
    return sample_posterior(mcmc, keys, prior, steps, burn, walkers, chain_npy, flat_npy, seed)


def patch_orbit_par(in_path, out_path, full, uncertainties=None):
    """Write the full model ``full`` (``inject_orbit_params``) over the .par: 17 significant digits (an MJD epoch needs
    them), a key's line found under either of its names (A1DOT | XDOT, ECC | E), the BINARY line untouched."""
    values = dict(full)
    unc = None if uncertainties is None else dict(uncertainties)
    for k, alias in _PAR_ALIASES.items():
        for a, b in ((k, alias), (alias, k)):
            if a in full and b not in full:
                values[b] = full[a]
                if unc is not None and a in unc:
                    unc[b] = unc[a]
    patch_par_values(in_path=in_path, out_path=out_path, new_values=values, float_fmt=".17g", uncertainties=unc)


def fit_orbit_toas(timfile_path, parfile, newparfile, t_start=None, t_end=None, t_mjd=None, mode="add", init_yaml=None,
                   mcmc=False, mcmc_steps=10000, mcmc_burn=500, mcmc_walkers=32, chain_npy=None, flat_npy=None,
                   best_fit="map", residual_plot=None, seed=None, plot=True):
    """Fit the ToAs of ``timfile_path`` to the flagged model ``parfile`` and write ``newparfile``: the maximum
    likelihood (``minimize_orbit``), or with ``mcmc`` the posterior's ``best_fit`` ('map' | 'median') with its 16 / 84
    half-widths as uncertainties. Returns {keys, p, uncertainties, full, residuals, toas}."""
    init = ReadTimingModel(parfile).readfulltimingmodel()[2]
    validate_orbit_parfile(init)
    toas = load_toas_for_fit(readtimfile(timfile_path, comment="C"), init, t_start, t_end, t_mjd, mode)
    x, y, yerr = toas["ToA"].to_numpy(), toas["phase"].to_numpy(), toas["phase_err_cycle"].to_numpy()
    if mcmc:
        if init_yaml is None:
            raise ValueError("an MCMC run needs init_yaml: the box prior of every free parameter")
        keys = list_orbit_fit_keys(init)
        _, _, summaries = run_mcmc(x, y, yerr, init, keys, initguess_prior_from_yaml(init_yaml), steps=mcmc_steps,
                                   burn=mcmc_burn, walkers=mcmc_walkers, chain_npy=chain_npy, flat_npy=flat_npy,
                                   seed=seed)
        best = np.array([summaries[k][best_fit] for k in keys], dtype=float)
        unc = {k: max(s["minus"], s["plus"]) for k, s in summaries.items()}
        problem = OrbitFit(x, init, keys, y, yerr)
        label = f"MCMC (posterior {best_fit})"
    else:
        nll, p0, keys, init = make_nll(x, y, yerr, init, init_yaml)
        problem = nll.problem
        res = minimize_orbit(problem, p0)
        best, unc = res.x, dict(zip(keys, res.sigma))
        label = "Maximum Likelihood Estimation"
    _, full = inject_orbit_params(init, best, keys)
    resid = problem.residuals(best)
    if plot:
        plot_residuals(toas, resid, residual_plot)
    patch_orbit_par(parfile, newparfile, full, unc)
    return {"keys": keys, "p": best, "uncertainties": unc, "full": full, "residuals": resid, "toas": toas,
            "label": label}


def main(argv=None):
    parser = build_parser()
    parser.description = "Script to fit ToAs to a timing model with a binary orbit (BT, ELL1)"
    args = parser.parse_args(argv)
    if args.mcmc and args.init_yaml is None:
        parser.error("-iy (or --init_yaml) is required when -mc (or --mcmc) is used")
    if args.corner_plot is not None:
        parser.error("-cp (or --corner_plot) is not provided here: save the flat samples with -fl and plot those")
    out = fit_orbit_toas(args.timfile_path, args.parfile, args.newparfile, args.t_start, args.t_end, args.t_mjd,
                         args.mode, args.init_yaml, args.mcmc, args.mcmc_steps, args.mcmc_burn, args.mcmc_walkers,
                         args.chain_npy, args.flat_npy, args.best_fit, args.residual_plot)
    for k, v in zip(out["keys"], out["p"]):
        print(f"  {k}: correction {v:.8e} +- {out['uncertainties'][k]:.2e}")
    print("---------------------------")
    print(f"Wrote new timing model to {args.newparfile} using {out['label']} values\n")
    toas = out["toas"]
    f0 = get_parameter_value(ReadTimingModel(args.parfile).readfulltimingmodel()[2]["F0"])
    _report_and_patch(args, toas, out["residuals"], len(out["keys"]), f0,
                      {"START": toas["ToA"].min(), "FINISH": toas["ToA"].max()})


if __name__ == "__main__":
    main()
