"""Generate the fixtures of the timing-model fits from the reference (fit_toas.py, utilities_fittoas.py,
readtimingmodel.py, get_local_ephem.py of CRIMP v2.3.0):

    tests/golden/fittoas.npz            load_toas_for_fit outputs, the Nelder-Mead minimum, the window lists
    tests/golden/fittoas_nll_<case>.npz the likelihood goldens of case a, b, c, d (one file per case: together they
                                        would pass the 1 MiB limit of a committed file)
    tests/golden/fittoas.json           key lists, injected dicts, .par texts (no pickles anywhere)

Run in the build container, never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_fittoas_golden.py

emcee and corner are not installed: empty stand-in modules let ``crimp.fit_toas`` import (nothing here samples), and
``crimp.get_local_ephem.run_mcmc`` is replaced by a weighted-least-squares stand-in so that the reference's own
window walk runs and records its windows.

Cases: (a) 1e2259.par with F0 and F1 flagged; (b) timing_model_dict.json (2 glitches, waves) with F0, F1, F2 and
GLEP / GLPH / GLF0 / GLF1 / GLF0D / GLTD of glitch 1 free; (c) the same model with WAVE_OM flagged (all WAVEj_A/B
free); (d) F0 and F1 plus waves.
"""
import copy
import json
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REF, "src"))
sys.dont_write_bytecode = True
for _name in ("emcee", "corner"):
    sys.modules.setdefault(_name, types.ModuleType(_name))

from scipy.optimize import minimize  # noqa: E402
import crimp  # noqa: E402
import crimp.fit_toas as FT  # noqa: E402
import crimp.utilities_fittoas as UF  # noqa: E402
import crimp.readtimingmodel as RT  # noqa: E402
import crimp.get_local_ephem as GL  # noqa: E402
from crimp.timfile import readtimfile  # noqa: E402

# the repository's own ``crimp`` alias package must not win the import
for _m in (crimp, FT, UF, RT, GL):
    assert os.path.abspath(_m.__file__).startswith(REF + os.sep), _m.__file__

PAR = os.path.join(HERE, "1e2259.par")
TIM = os.path.join(HERE, "ToAs_2259.tim")
SIZES = (1, 2, 63, 64, 65, 84, 257)
NVEC = 64
GLITCH1_FREE = ("GLEP_1", "GLPH_1", "GLF0_1", "GLF1_1", "GLF0D_1", "GLTD_1")
# plausible sizes of the corrections (1 sigma of the drawn vectors); GLEP and GLTD are drawn around their values
SCALE = {"F0": 1e-8, "F1": 1e-16, "F2": 1e-24, "GLPH_1": 0.1, "GLF0_1": 1e-8, "GLF1_1": 1e-16, "GLF0D_1": 1e-8}


def flagged(values, free):
    """A {value, flag} model from a values-only dict, as ReadTimingModel's third dictionary lays it out."""
    out = {}
    for k, v in values.items():
        if isinstance(v, dict):
            out[k] = {"value": dict(v), "flag": None}
        elif k == "WAVEEPOCH":
            out[k] = {"value": v, "flag": None}
        else:
            out[k] = {"value": v, "flag": 1 if k in free else 0}
    return out


def case_models():
    a = RT.ReadTimingModel(PAR).readfulltimingmodel()[2]
    for k in ("F0", "F1"):
        a[k]["flag"] = 1
    full = json.load(open(os.path.join(HERE, "timing_model_dict.json")))
    return {"a": a,
            "b": flagged(full, ("F0", "F1", "F2") + GLITCH1_FREE),
            "c": flagged(full, ("WAVE_OM",)),
            "d": flagged(full, ("F0", "F1", "WAVE_OM"))}


def draw_pvecs(rng, keys, model):
    p = np.empty((NVEC, len(keys)))
    for i, k in enumerate(keys):
        if k.startswith("GLEP_"):
            p[:, i] = model[k]["value"] + rng.normal(0, 0.5, NVEC)
        elif k.startswith("GLTD_"):
            p[:, i] = 30.0 + rng.normal(0, 3.0, NVEC)
        elif k.startswith("WAVE"):
            p[:, i] = rng.normal(0, 0.01, NVEC)
        else:
            p[:, i] = rng.normal(0, SCALE[k], NVEC)
    p[0] = 0.0  # the all-zero vector (a free GLTD of 0 takes the GLTD == 0 rule)
    return p


def toa_sets(base, rng):
    """ToA sets of every size in SIZES: cuts of the bundled 84, and a resampling around them for 257."""
    x, y, e = (base[c].to_numpy(dtype=float) for c in ("ToA", "phase", "phase_err_cycle"))
    sets = {}
    for n in SIZES:
        if n <= x.size:
            sets[n] = (x[:n].copy(), y[:n].copy(), e[:n].copy())
        else:
            xs = np.sort(rng.uniform(x.min(), x.max(), n))
            sets[n] = (xs, rng.normal(0, 0.05, n), rng.choice(e, n))
    return sets


def jsonable(d):
    out = {}
    for k, v in d.items():
        if isinstance(v, dict):
            out[k] = jsonable(v)
        elif v is None:
            out[k] = None
        else:
            out[k] = float(v)
    return out


def wls_run_mcmc(x, y, yerr, init_parfile, keys, prior, **kw):
    """Stand-in for run_mcmc inside the reference's window walk: the weighted least-squares solution of the (linear)
    F0, F1 problem, with its analytic 1-sigma widths as the summaries' minus / plus."""
    x, y, yerr = (np.asarray(v, dtype=float) for v in (x, y, yerr))
    unit = [prior.bounds[k][1] for k in keys]
    A = np.stack([UF.model_phase_residuals(x, init_parfile, np.eye(len(keys))[i] * unit[i], keys) / unit[i]
                  for i in range(len(keys))], axis=1)
    w = 1.0 / yerr ** 2
    cov = np.linalg.inv(A.T @ (A * w[:, None]))
    sol = cov @ (A.T @ (w * (y - y.mean())))
    sig = np.sqrt(np.diag(cov))
    return None, None, {k: {"median": float(sol[i]), "minus": float(sig[i]), "plus": float(sig[i]),
                            "map": float(sol[i])} for i, k in enumerate(keys)}


def main():
    rng = np.random.default_rng(20240611)
    npz, side = {}, {"cases": {}}
    models = case_models()

    # ---- load_toas_for_fit: folded, and with two phase wraps
    tim = readtimfile(TIM, comment="C")
    base = FT.load_toas_for_fit(tim.copy(), copy.deepcopy(models["a"]))
    wraps = [58300.0, 58500.0]
    wrapped = FT.load_toas_for_fit(tim.copy(), copy.deepcopy(models["a"]), t_mjd_phasewrap=wraps, mode="add")
    for name, df in (("load", base), ("load_wrapped", wrapped)):
        for c in ("ToA", "phase", "phase_err_cycle"):
            npz[name + "_" + c] = df[c].to_numpy(dtype=float)
    npz["load_wraps"] = np.array(wraps)

    # ---- cases: key lists, injected dicts, likelihood goldens
    sets = toa_sets(base, rng)
    for name, model in models.items():
        keys = UF.list_fit_keys(model)
        pv = draw_pvecs(rng, keys, model)
        fit, full = UF.inject_free_params(copy.deepcopy(model), pv[1], keys)
        side["cases"][name] = {"model": jsonable(model), "keys": keys, "pvec": [float(v) for v in pv[1]],
                               "fit": jsonable(fit), "full": jsonable(full)}
        out = {"pvec": pv}
        max_phase = 0.0
        for n, (x, y, e) in sets.items():
            mu = np.empty((NVEC, n))
            nll = np.empty(NVEC)
            for j in range(NVEC):
                m = copy.deepcopy(model)
                fitd, fulld = UF.inject_free_params(m, pv[j], keys)
                # the largest absolute phase the evaluation forms, before the mean is taken off
                ph = np.abs(FT.Phases(x, fitd).taylorexpansion() + FT.Phases(x, fitd).glitches()) \
                    + np.abs(FT.Phases(x, fulld).waves()) + np.abs(FT.Phases(x, {**fitd, "F0": fulld["F0"]}).waves())
                max_phase = max(max_phase, float(np.max(ph)))
                mu[j] = UF.model_phase_residuals(x, m, pv[j], keys)
                nll[j] = UF.gaussian_nll(y - np.mean(y), mu[j], e)
            out.update({"x_%d" % n: x, "y_%d" % n: y, "e_%d" % n: e, "mu_%d" % n: mu, "nll_%d" % n: nll})
        out["max_abs_phase"] = np.float64(max_phase)
        print("case", name, "ndim", len(keys), "max |phase| %.3g cycles" % max_phase)
        assert max_phase <= 1e3, max_phase
        np.savez_compressed(os.path.join(HERE, "fittoas_nll_%s.npz" % name), **out)

    # ---- the reference's Nelder-Mead minimum of case (a), by the call of fit_toas.py:424
    ma = copy.deepcopy(models["a"])
    nll, p0, keys, _ = UF.make_nll(base["ToA"], base["phase"], base["phase_err_cycle"], ma)
    res = minimize(nll, p0, method="Nelder-Mead", options={"maxiter": int(1e5)})
    npz["nm_x"], npz["nm_fun"] = res.x, np.float64(res.fun)
    print("Nelder-Mead", res.x, res.fun, res.nit)

    # ---- patched .par texts: one MLE-style and one MCMC-style update of a flagged copy of 1e2259.par
    text = open(PAR).read().replace("F0     0.14328254547263483", "F0     0.14328254547263483 1") \
                           .replace("F1  -9.746993965547238e-15", "F1  -9.746993965547238e-15 1 2.5e-17")
    _, full = UF.inject_free_params(ma, res.x, keys)
    stats = {"CHI2R": 1.2345678, "NTOA": 84, "TRES": 12345.678, "CHI2R_DOF": 82}
    misc = {"START": 58136.13012457407, "FINISH": 58737.5, "TZRSITE": None, "CLK": "TT(TAI)"}
    unc = {"F0": 1.23456789e-10, "F1": 3.3e-18}
    side["par"] = {"input": text, "new_values": jsonable(full), "stats": stats, "misc": misc, "uncertainties": unc}
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "in.par"), os.path.join(tmp, "out.par")
        open(src, "w").write(text)
        RT.patch_par_values(in_path=src, out_path=dst, new_values=full)
        side["par"]["mle_values"] = open(dst).read()
        RT.patch_statistics(in_path=dst, out_path=dst, new_stats=stats)
        RT.patch_miscellaneous(in_path=dst, out_path=dst, new_misc=misc)
        side["par"]["mle_final"] = open(dst).read()
        RT.patch_par_values(in_path=src, out_path=dst, new_values=full, uncertainties=unc)
        side["par"]["mcmc_values"] = open(dst).read()
        RT.patch_statistics(in_path=dst, out_path=dst, new_stats=stats)
        RT.patch_statistics(in_path=dst, out_path=dst, new_stats=stats)  # fit_toas.py:403-404 patches twice
        RT.patch_miscellaneous(in_path=dst, out_path=dst, new_misc=misc)
        side["par"]["mcmc_final"] = open(dst).read()

        # ---- window lists of the reference's walk (fits replaced by the least-squares stand-in)
        GL.run_mcmc = wls_run_mcmc
        glitch_par = os.path.join(tmp, "glitch.par")
        glitch_lines = "GLEP_1 58400.0\nGLPH_1 0.0\nGLF0_1 1e-9\nGLF1_1 0.0\n"
        open(glitch_par, "w").write(open(PAR).read().rstrip("\n") + "\n" + glitch_lines)
        side["glitch_par_lines"] = glitch_lines
        for name, par in (("win", PAR), ("win_glitch", glitch_par)):
            df = GL.generate_local_ephemerides(TIM, par, outputfile=None)
            for c in ("TOA_MJD_ref", "TOA_MJD_ref_err", "DOF", "F0", "F1", "F0_err", "F1_err"):
                npz[name + "_" + c] = df[c].to_numpy(dtype=float)
            print(name, len(df), "windows")

    np.savez_compressed(os.path.join(HERE, "fittoas.npz"), **npz)
    with open(os.path.join(HERE, "fittoas.json"), "w") as fh:
        json.dump(side, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
