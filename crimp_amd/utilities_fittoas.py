"""Host side of the timing-model fits (drop-in for CRIMP's ``utilities_fittoas.py``, v2.3.0).

The likelihood itself runs on the device: ``make_nll``'s closure and ``model_phase_residuals`` call
``crimp_timing_nll`` (csrc/timing_fit.h) through ``ops.timing_nll``. What stays here is the bookkeeping around it:
which parameters are free (:14-58), how a parameter vector maps onto the fit model and the full model (:61-159),
the validation of a flagged model (:162-200) and the YAML of initial guesses and box priors (:244-266, :296-390).
"""
import copy
import re
from dataclasses import dataclass

import numpy as np

from . import ops

_WAVE_KEY = re.compile(r"^WAVE(\d+)?$")
_WAVE_HARMONIC = re.compile(r"^WAVE(\d+)$")
_WAVE_AB = re.compile(r"^WAVE\d+_[AB]$")
_GLEP = re.compile(r"^GLEP_\d+$")
_GLTD = re.compile(r"^GLTD_\d+$")
_KEPT_EPOCHS = ("PEPOCH", "WAVEEPOCH", "WAVE_OM")


def list_fit_keys(parfile: dict):
    """Names of the parameters with flag 1, in the model's order. A flagged WAVE_OM stands for the whole whitening
    model: it is replaced by WAVEj_A, WAVEj_B of every harmonic, appended at the end."""
    keys = [k for k, v in parfile.items() if isinstance(v, dict) and "value" in v and "flag" in v and v["flag"] == 1]
    om = parfile.get("WAVE_OM")
    if om is not None and om.get("flag") == 1:
        keys = [k for k in keys if k != "WAVE_OM"]
        for k in parfile:
            if _WAVE_KEY.match(k):
                keys += [k + "_A", k + "_B"]
    return keys


def extract_free_params(parfile, yaml_initialguesses: str | None = None):
    """(p0, keys): the free parameters' names and their starting vector -- zeros, or the YAML's guesses."""
    keys = list_fit_keys(parfile)
    if yaml_initialguesses is None:
        return np.zeros(len(keys), dtype=float), keys
    return initialize_params(keys, yaml_initialguesses), keys


def _is_scalar_entry(v):
    return isinstance(v, dict) and "value" in v and not isinstance(v["value"], dict)


def _zero_gltd_without_glf0d(parfile):
    # a recovery timescale whose frequency jump GLF0D is 0 plays no part: the reference sets it to 0 in the model
    # it was given (in place), before anything else
    for key, entry in parfile.items():
        if key.startswith("GLTD_"):
            jump = parfile.get("GLF0D_" + key.split("_", 1)[1])
            if jump and jump.get("value") == 0:
                entry["value"] = 0


def inject_free_params(parfile, pvec: np.ndarray, keys: list):
    """(fit model, full model) for a parameter vector.

    Fit model: plain values; every scalar 0 except PEPOCH, GLEP_*, WAVEEPOCH and WAVE_OM, every free parameter its
    ``pvec`` entry. Full model: the .par values with the vector applied as a correction in phase space -- a glitch
    epoch is the fitted value itself, GLTD_* is base + delta, everything else (WAVE A/B included) base - delta."""
    _zero_gltd_without_glf0d(parfile)
    fit, full = {}, {}
    for k, v in parfile.items():
        if _is_scalar_entry(v):
            keep = k in _KEPT_EPOCHS or _GLEP.match(k)
            fit[k] = v["value"] if keep else 0.0
            full[k] = v["value"]
        else:
            fit[k] = copy.deepcopy(v)
            full[k] = copy.deepcopy(v)
    for k, delta in zip(keys, pvec):
        if k in _KEPT_EPOCHS:
            continue
        if _WAVE_AB.match(k):
            name, coeff = k.rsplit("_", 1)
            if name not in parfile:
                raise KeyError(f"Parameter '{name}' not found in parfile.")
            base = parfile[name]["value"][coeff]
            fit[name]["value"][coeff] = delta
            full[name]["value"][coeff] = base - delta
            continue
        if k not in parfile:
            raise KeyError(f"Parameter '{k}' not found in parfile.")
        base = parfile[k]["value"]
        fit[k] = delta
        if _GLEP.match(k):
            full[k] = delta
        elif _GLTD.match(k):
            full[k] = base + delta
        else:
            full[k] = base - delta
    return fit, full


def validate_parfile(parfile):
    """Raise ValueError unless ``parfile`` is a flagged model: every entry but WAVEEPOCH and the WAVEj harmonics a
    {"value": number, "flag": 0 | 1} dict, and at least one flag set."""
    if not isinstance(parfile, dict):
        raise ValueError("Initial timing model must be a dict")
    nfree = 0
    for k, v in parfile.items():
        if k == "WAVEEPOCH" or _WAVE_HARMONIC.match(k):
            continue
        if not (isinstance(v, dict) and "value" in v and "flag" in v):
            raise ValueError(f"Parameter '{k}' must be a dict with 'value' and 'flag'")
        if not isinstance(v["value"], (int, float, np.floating)):
            raise ValueError(f"Parameter '{k}': value must be numeric, got {type(v['value'])}")
        if v["flag"] not in (0, 1):
            raise ValueError(f"Parameter '{k}': fit flag must be 0 or 1, got {v['flag']}")
        nfree += v["flag"] == 1
    if nfree == 0:
        raise ValueError("Template has no free parameters (flag==1). Nothing to optimize.")


def gaussian_nll(y, mu, sigma):
    """Gaussian negative log-likelihood, with its log(2 pi sigma^2) term."""
    r = (y - mu) / sigma
    return 0.5 * np.sum(r ** 2 + np.log(2.0 * np.pi * sigma ** 2))


class DeviceFit:
    """One fit problem as the device sees it: the ToAs, the two base models and the parameter map of
    ``crimp_timing_nll`` / ``crimp_timing_mcmc`` for a flagged model and its free keys."""

    def __init__(self, x, parfile, keys, y=None, yerr=None):
        self.keys = list(keys)
        self.x = np.ascontiguousarray(np.asarray(x, dtype=float).reshape(-1))
        self.y = np.zeros_like(self.x) if y is None else np.ascontiguousarray(np.asarray(y, dtype=float).reshape(-1))
        self.yerr = (np.ones_like(self.x) if yerr is None
                     else np.ascontiguousarray(np.asarray(yerr, dtype=float).reshape(-1)))
        if not (self.x.size == self.y.size == self.yerr.size):
            raise ValueError("x, y and yerr differ in length")
        self.map = ops.fit_map(self.keys)
        fit, full = inject_free_params(parfile, np.zeros(len(self.keys)), self.keys)
        # a free glitch epoch is 0 in `full`; only F0 and the WAVE A/B values of the full model are used
        self.fit_base = ops._modeltm(fit)
        self.wave_base = ops._modeltm({k: v for k, v in full.items() if not k.startswith("GL")})

    def nll(self, pvec):
        """NLL of one vector [ndim] (a float) or of many [P, ndim] (an array [P])."""
        p = np.asarray(pvec, dtype=float)
        out = ops.timing_nll(self.x, self.y, self.yerr, self.fit_base, self.wave_base, self.map,
                             p.reshape(1, -1, len(self.keys)))[0]
        return float(out[0]) if p.ndim == 1 else out

    def residuals(self, pvec):
        """Mean-subtracted model phase residuals of one vector [n] or of many [P, n]."""
        p = np.asarray(pvec, dtype=float)
        _, mu = ops.timing_nll(self.x, self.y, self.yerr, self.fit_base, self.wave_base, self.map,
                               p.reshape(1, -1, len(self.keys)), want_mu=True)
        mu = mu.reshape(-1, self.x.size)
        return mu[0] if p.ndim == 1 else mu


def make_nll(x, y, y_err, parfile, yaml_init=None):
    """(nll, p0, keys, parfile): ``nll(pvec)`` is the Gaussian NLL of the mean-subtracted residuals ``y`` against the
    model residuals of ``pvec``, one ``crimp_timing_nll`` call with P = 1."""
    validate_parfile(parfile)
    p0, keys = extract_free_params(parfile, yaml_init)
    problem = DeviceFit(x, parfile, keys, y, y_err)

    def nll(pvec):
        return problem.nll(np.asarray(pvec, dtype=float).reshape(-1))

    return nll, p0, keys, parfile


def initialize_params(keys: list[str], yaml_init: str) -> np.ndarray:
    """The YAML's initial guesses as a vector in the order of ``keys``."""
    prior = initguess_prior_from_yaml(yaml_init)
    if not prior.initial_guess:
        raise ValueError("No initial guesses found in YAML file.")
    missing = [k for k in keys if k not in prior.initial_guess]
    if missing:
        raise KeyError(f"Missing initial guesses for: {', '.join(missing)}")
    return np.array([prior.initial_guess[k] for k in keys], dtype=float)


def model_phase_residuals(x_mjd, timmodel, pvec, keys: list[str]) -> np.ndarray:
    """Mean-subtracted phase residuals of the fit model for ``pvec`` (the ``mu`` output of ``crimp_timing_nll``)."""
    return DeviceFit(x_mjd, timmodel, keys).residuals(np.asarray(pvec, dtype=float).reshape(-1))


@dataclass
class Prior:
    bounds: dict[str, tuple[float, float]]  # may be empty
    initial_guess: dict[str, float]         # may be empty

    def log_prior(self, theta: np.ndarray, keys: list[str]) -> float:
        """Box prior with strict inequalities; a key without bounds is unconstrained."""
        for val, name in zip(theta, keys):
            if name in self.bounds:
                lo, hi = self.bounds[name]
                if not (lo < val < hi):
                    return -np.inf
        return 0.0


def initguess_prior_from_yaml(path: str) -> Prior:
    """Read ``parameter: [low, high]`` (bounds), ``parameter: number`` (guess) or ``parameter: {low:, high:,
    guess:}`` entries. If any parameter has bounds all must, and likewise for guesses."""
    import yaml
    with open(path, "r") as fh:
        data = yaml.safe_load(fh)
    if not isinstance(data, dict):
        raise ValueError("YAML must map parameter -> prior/guess")
    bounds, guesses = {}, {}

    def box(k, low, high):
        low, high = float(low), float(high)
        if not (low < high):
            raise ValueError(f"{k}: low < high required")
        bounds[k] = (low, high)

    for k, v in data.items():
        if isinstance(v, (list, tuple)):
            if len(v) != 2:
                raise ValueError(f"{k}: expected [low, high]")
            box(k, *v)
        elif isinstance(v, dict):
            if ("low" in v) != ("high" in v):
                raise ValueError(f"{k}: need both 'low' and 'high' if providing bounds")
            if "low" in v:
                box(k, v["low"], v["high"])
            if "guess" in v:
                guesses[k] = float(v["guess"])
        elif isinstance(v, (int, float)):
            guesses[k] = float(v)
        else:
            raise ValueError(f"{k}: unsupported value {v!r}")
    if bounds:
        missing = [p for p in data if p not in bounds]
        if missing:
            raise ValueError("Bounds provided for some parameters but missing for others: " + ", ".join(missing))
    if guesses:
        missing = [p for p in data if p not in guesses]
        if missing:
            raise ValueError("Initial guesses provided for some parameters but missing for others: "
                             + ", ".join(missing))
    return Prior(bounds=bounds, initial_guess=guesses)
