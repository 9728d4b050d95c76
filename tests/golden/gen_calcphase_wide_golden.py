"""Regenerates tests/golden/calcphase_wide.npz: the reference's calcphase / Phases (calcphase.py:20-176) run over the
whole model space, beside the same phases at 60 digits (tests/phase_reference.py).

    python tests/golden/gen_calcphase_wide_golden.py path/to/CRIMP-v2.3.0/src [--check]

``--check`` regenerates everything, compares every array with the committed file and writes nothing. All seeds are
fixed; the arrays reproduce bit for bit (the zip container carries a timestamp).

Models (each with ~1500 uniformly random times plus the special ones: every epoch and its two fp64 neighbours, the
span's ends):

* ``short``          timing_model_dict.json over MJD 58139-58146: times before PEPOCH (negative totals), before, between
                     and after both glitches, the GLTD_2 == 0 branch; |phase| < 1e5, so 32 u A < 1e-9 cycles;
* ``taylor13``       F0..F12 all non-zero, alternating signs, F_k ~ (k+1)!/T^(k+1): every term reaches >= 1e-3 cycles
                     at the edge of +-500 days;  ``taylor13_gaps``: F5 = F6 = F12 = 0;  ``taylor13_f12``: only F12;
* ``glitches32``     32 glitches, epochs not in index order, two on one epoch, GLTD of four kinds (0, ~0.01 d, ~30 d,
                     ~1e4 d), no Taylor term, so its bound is the glitch expression's own;
* ``waves64``        64 harmonics, amplitudes ~1/j, arguments up to ~6.5e3 rad, t == WAVEEPOCH;
* ``all``            taylor13's F terms, 5 of the glitches, 8 of the waves;  ``all_flags``: the same model with
                     {value, flag} entries (Phases._normalize_timdict), same arrays.

Layout, chosen to keep the file small without losing a bit of what the tests compare:
  index                JSON {name: [key of its times, name whose arrays it uses]}
  t_short, t_wide      the times (the +-500-day models share one set)
  <name>_model         the model, JSON
  <name>_hi  (4, n) f8 the 60-digit total, Taylor, glitch and wave phases rounded to fp64 (rows: phase_reference.PARTS)
  <name>_lo  (4, n) f8 mp - hi, cut to 20 significant bits (hi + lo carries mp to 2^-72 of itself)
  <name>_A   (3, n) f8 the error unit A(t) of the three parts, cut towards zero to 16 significant bits: the stored
                     bound is never wider than the exact one; A(total) is the sum of the three, formed on load
  <name>_refd (4, n) f8 the reference's total, taylorexpansion(), glitches(), waves() minus hi (exact: they lie within
                     a few ulp of hi, so the difference is representable and mostly zero)

Asserted before anything is written: the reference is within 32 u A of mp everywhere; every model parameter is
visible (zeroing it -- or, where it is zero, swapping it with a neighbouring index -- in the mp model moves the phase
by >= 1000 x the bound at >= 20 stored times; the exemptions are listed in exempt() with their reasons and asserted to
be exactly the invisible ones); every glitch epoch has times before, on and after it; ``short`` has negative totals
and its 32 u A is below the 1e-9-cycle contract. Only numbers the reference computed travel; none of its code.
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.dont_write_bytecode = True

import phase_reference as R  # noqa: E402

N_RANDOM = 1500
VISIBLE_FACTOR, VISIBLE_TIMES = 1000.0, 20
T_SPAN = 500.0                      # days either side of PEPOCH for the wide models
PEPOCH_W = 58000.0


# ------------------------------------------------------------------------------------------------ models
def zero_f():
    return {"F%d" % k: 0.0 for k in range(13)}


def model_taylor13():
    rng = np.random.default_rng(1301)
    T = T_SPAN * 86400.0
    tm = {"PEPOCH": PEPOCH_W}
    fact = 1.0
    for k in range(13):
        fact *= k + 1
        c = 4.0e6 * rng.uniform(1.0, 2.0)              # cycles reached by term k at the edge of the span
        tm["F%d" % k] = float((-1.0) ** k * c * fact / T ** (k + 1))
    return tm


def glitch_rows(n=32):
    rng = np.random.default_rng(3201)
    ep = rng.uniform(PEPOCH_W - 400.0, PEPOCH_W + 300.0, n)
    ep[16] = ep[4]                                      # GLEP_17 == GLEP_5
    assert np.any(np.diff(ep) < 0) and np.any(np.diff(ep) > 0)
    kinds = [0.0, 0.01, 30.0, 1.0e4]
    rows = []
    for j in range(n):
        td = kinds[j % 4] * (rng.uniform(0.8, 1.25) if kinds[j % 4] else 0.0)
        f0d = {0.0: 1e-7, 0.01: 1e-5, 30.0: 1e-7, 1.0e4: 1e-8}[kinds[j % 4]] * rng.uniform(0.5, 2.0)
        sg = rng.choice([-1.0, 1.0], 5)
        rows.append({"GLEP": float(ep[j]), "GLPH": float(sg[0] * rng.uniform(0.1, 0.5)),
                     "GLF0": float(sg[1] * rng.uniform(0.5, 2.0) * 1e-6), "GLF1": float(sg[2] * rng.uniform(0.5, 2.0) * 1e-14),
                     "GLF2": float(sg[3] * rng.uniform(0.5, 2.0) * 1e-21), "GLF0D": float(sg[4] * f0d), "GLTD": float(td)})
    return rows


def add_glitches(tm, rows):
    for j, r in enumerate(rows, start=1):
        for b, v in r.items():
            tm["%s_%d" % (b, j)] = v
    return tm


def wave_rows(n=64):
    rng = np.random.default_rng(6401)
    return [{"A": float(rng.choice([-1.0, 1.0]) * rng.uniform(0.7, 1.3) / j),
             "B": float(rng.choice([-1.0, 1.0]) * rng.uniform(0.7, 1.3) / j)} for j in range(1, n + 1)]


WAVEEPOCH_W, WAVE_OM_W = 57990.5, 0.2


def add_waves(tm, rows):
    tm["WAVEEPOCH"], tm["WAVE_OM"] = WAVEEPOCH_W, WAVE_OM_W
    for j, r in enumerate(rows, start=1):
        tm["WAVE%d" % j] = dict(r)
    return tm


def build_models():
    with open(os.path.join(HERE, "timing_model_dict.json")) as fh:
        short = json.load(fh)
    t13 = model_taylor13()
    gaps = dict(t13, F5=0.0, F6=0.0, F12=0.0)
    f12 = dict({"PEPOCH": PEPOCH_W}, **zero_f())
    f12["F12"] = t13["F12"]
    gl = glitch_rows()
    g32 = add_glitches(dict({"PEPOCH": PEPOCH_W}, **zero_f()), gl)
    wv = wave_rows()
    w64 = add_waves(dict(dict({"PEPOCH": PEPOCH_W}, **zero_f()), F0=0.12345678901234567, F1=-1.0e-13), wv)
    # one glitch of each GLTD kind (rows 0-3) and one of the pair that shares an epoch (row 4); harmonics 1-8
    allm = add_waves(add_glitches(dict(t13), gl[:5]), wv[:8])
    flags = {k: ({"value": v, "flag": (1 if k.startswith("F") else 0)} if isinstance(v, float) else v)
             for k, v in allm.items()}
    return {"short": short, "taylor13": t13, "taylor13_gaps": gaps, "taylor13_f12": f12, "glitches32": g32,
            "waves64": w64, "all": allm, "all_flags": flags}


# ------------------------------------------------------------------------------------------------ times
def with_neighbours(xs):
    out = []
    for x in xs:
        out += [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]
    return out


def build_times(models):
    rng = np.random.default_rng(1500)
    s = models["short"]
    sp = with_neighbours([s["PEPOCH"], s["GLEP_1"], s["GLEP_2"], s["WAVEEPOCH"]]) + [58139.0, 58146.0]
    t_short = np.concatenate([sp, rng.uniform(58139.0, 58146.0, N_RANDOM)])
    eps = [models["glitches32"]["GLEP_%d" % j] for j in range(1, 33)]
    wp = with_neighbours(eps + [PEPOCH_W, WAVEEPOCH_W]) + [PEPOCH_W - T_SPAN, PEPOCH_W + T_SPAN]
    t_wide = np.concatenate([wp, rng.uniform(PEPOCH_W - T_SPAN, PEPOCH_W + T_SPAN, N_RANDOM)])
    out = {}
    for key, t in (("t_short", t_short), ("t_wide", t_wide)):
        if t.size % 2:                                   # even length: the whole array takes the pair kernel
            t = np.append(t, rng.uniform(t.min(), t.max()))
        rng.shuffle(t)
        out[key] = np.ascontiguousarray(t, dtype=np.float64)
    return out


# ------------------------------------------------------------------------------------------------ visibility
def param_list(tm):
    keys = []
    for k, v in tm.items():
        if isinstance(v, dict):
            keys += [(k, "A"), (k, "B")]
        else:
            keys.append((k, None))
    return keys


def _get(tm, key):
    k, sub = key
    return tm[k][sub] if sub else tm[k]


def _set(tm, key, v):
    k, sub = key
    if sub:
        tm[k][sub] = v
    else:
        tm[k] = v


def _neighbours(tm, key):
    """The same parameter at the neighbouring indices (F_k+-1, GLxx_j+-1, WAVEj+-1), those the model has."""
    k, sub = key
    if k.startswith("GL") and "_" in k:
        base, j = k.rsplit("_", 1)
        cand = ["%s_%d" % (base, int(j) + d) for d in (-1, 1)]
    elif k[0] == "F" and k[1:].isdigit():
        cand = ["F%d" % (int(k[1:]) + d) for d in (-1, 1)]
    elif k.startswith("WAVE") and k[4:].isdigit():
        cand = ["WAVE%d" % (int(k[4:]) + d) for d in (-1, 1)]
    else:
        cand = []
    return [(c, sub) for c in cand if c in tm]


def perturbed(tm, key):
    """(model with ``key`` zeroed, or -- where it is zero -- swapped with the first neighbouring index that holds
    another value; the keys touched), or (None, ()) when neither changes the model."""
    new = copy.deepcopy(tm)
    v = _get(tm, key)
    if v != 0.0:
        _set(new, key, 0.0)
        return new, (key,)
    for nb in _neighbours(tm, key):
        w = _get(tm, nb)
        if w != v:
            _set(new, key, w)
            _set(new, nb, v)
            return new, (key, nb)
    return None, ()


def delta_mp(tm, new, touched, t, cache):
    """mp phase of ``new`` minus that of ``tm``: only the parts and components the touched keys enter are evaluated."""
    names = [k for k, _ in touched]
    d = [0] * len(t)

    def add(fn, **kw):
        a, b = fn(new, t, **kw)[0], fn(tm, t, **kw)[0]
        for i in range(len(t)):
            d[i] += a[i] - b[i]

    if any(k == "PEPOCH" or (k[0] == "F" and k[1:].isdigit()) for k in names):
        if "te" not in cache:
            cache["te"] = R.taylor_mp(tm, t)[0]
        a = R.taylor_mp(new, t)[0]
        for i in range(len(t)):
            d[i] += a[i] - cache["te"][i]
    gj = {int(k.rsplit("_", 1)[1]) for k in names if k.startswith("GL") and "_" in k}
    if gj:
        add(R.glitches_mp, only=gj)
    if any(k in ("WAVEEPOCH", "WAVE_OM", "F0") for k in names):
        if R.n_waves(tm):
            if "wv" not in cache:
                cache["wv"] = R.waves_mp(tm, t)[0]
            a = R.waves_mp(new, t)[0]
            for i in range(len(t)):
                d[i] += a[i] - cache["wv"][i]
    else:
        wj = {int(k[4:]) for k in names if k.startswith("WAVE") and k[4:].isdigit()}
        if wj:
            add(R.waves_mp, only=wj)
    return np.array([abs(float(x)) for x in d])


# Parameters that no perturbation of the two kinds can make visible, with the reason; asserted to be exactly the
# invisible ones. Each kind of parameter exempt in one model is visible in another.
def exempt(name, tm):
    ex = {}
    for j in range(1, R.n_glitches(tm) + 1):
        if tm.get("GLTD_%d" % j, 0.0) == 0.0:
            ex[("GLF0D_%d" % j, None)] = "multiplies the recovery term that GLTD == 0 removes (calcphase.py:115)"
    if name == "short":
        # the issue fixes this model and its 7-day span: over 6 days F3 dt^4/24 reaches 5e-10 cycles and
        # GLF2_1 ds^3/6 7e-8, below 1000 x the bound (~2.5e-7); taylor13 and glitches32 make both kinds visible
        ex[("F3", None)] = "5e-10 cycles over the 7-day span"
        ex[("GLF2_1", None)] = "7e-8 cycles over the 4 days after GLEP_1"
        ex[("GLF2_2", None)] = "zero; GLF2_1 swapped in reaches 4e-9 cycles over the 1.5 days after GLEP_2"
    fz = [tm["F%d" % k] == 0.0 for k in range(13)]
    for k in range(13):
        if fz[k] and all(fz[i] for i in (k - 1, k + 1) if 0 <= i < 13):
            ex[("F%d" % k, None)] = "zero, with zero neighbours: neither zeroing nor a swap changes the model"
    if all(fz):
        ex[("PEPOCH", None)] = "no Taylor term to shift"
    return ex


def check_visible(name, tm, t, a_total):
    thresh = VISIBLE_FACTOR * R.FACTOR * R.U * a_total
    cache, invisible, least = {}, {}, (None, np.inf)
    for key in param_list(tm):
        new, touched = perturbed(tm, key)
        if new is None:
            invisible[key] = 0
            continue
        d = delta_mp(tm, new, touched, t, cache)
        n = int(np.sum((d >= thresh) & (d > 0)))
        if n < VISIBLE_TIMES:
            invisible[key] = n
        elif n < least[1]:
            least = (key, n)
    want = exempt(name, tm)
    assert set(invisible) == set(want), (name, "invisible", invisible, "exempt", sorted(want))
    print("  visible: %d parameters, fewest times %s; exempt: %s" %
          (len(param_list(tm)) - len(invisible), least, ", ".join(k for k, _ in sorted(want)) or "none"))


# ------------------------------------------------------------------------------------------------ main
def reference_parts(ref_mod, t, tm):
    total, folded = ref_mod.calcphase(t, tm)
    ph = ref_mod.Phases(t, tm)
    te, gl, wv = ph.taylorexpansion(), ph.glitches(), ph.waves()
    assert np.array_equal(folded, total - np.floor(total))
    bc = [np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), t.shape)) for x in (total, te, gl, wv)]
    return np.vstack(bc)


def main(src, check):
    sys.path.insert(0, src)
    import crimp.calcphase as ref_mod
    models = build_models()
    times = build_times(models)
    out = {"t_short": times["t_short"], "t_wide": times["t_wide"]}
    index, table = {}, {}
    for name, tm in models.items():
        tkey = "t_short" if name == "short" else "t_wide"
        t = times[tkey]
        ref = reference_parts(ref_mod, t, tm)
        if name == "all_flags":
            assert np.array_equal(ref, out["all_hi"] + out["all_refd"]), "the {value, flag} copy moved the reference"
            index[name] = [tkey, "all"]
            out[name + "_model"] = np.array(json.dumps(tm))
            continue
        print(name, "n =", t.size)
        mpv = R.phase_mp(tm, t)
        hi, lo = zip(*(R.hi_lo(mpv[p][0]) for p in R.PARTS))
        hi, lo = np.vstack(hi), np.vstack(lo)
        a3 = np.vstack([R.mag_chopped(mpv[p][1]) for p in R.PARTS[1:]])
        refd = ref - hi
        assert np.array_equal(hi + refd, ref), "reference - hi is not exact"
        m = R.WideModel(name, tm, t, hi, lo, a3, refd)
        # --- the reference alone meets the bound
        table[name] = {p: m.ratio(m.ref[p], p) for p in R.PARTS}
        print("  reference max |err| / (u A):", {p: round(v, 2) for p, v in table[name].items()})
        assert max(table[name].values()) <= R.FACTOR, (name, table[name])
        # --- epochs and signs
        for j in range(1, R.n_glitches(tm) + 1):
            e = tm["GLEP_%d" % j]
            assert np.any(t < e) and np.any(t == e) and np.any(t > e), (name, j)
            assert np.nextafter(e, -np.inf) in t and np.nextafter(e, np.inf) in t
        if R.n_waves(tm):
            assert tm["WAVEEPOCH"] in t
            arg = R.n_waves(tm) * tm["WAVE_OM"] * np.max(np.abs(t - tm["WAVEEPOCH"]))
            print("  largest wave argument %.0f rad" % arg)
            assert name != "waves64" or 1e3 <= arg <= 1e4
        if name == "short":
            assert np.any(m.hi["total"] < 0) and np.any(t < tm["PEPOCH"])
            assert np.max(np.abs(m.hi["total"])) < 1e5
            b = R.FACTOR * R.U * np.max(m.A["total"])
            print("  32 u A <= %.3g cycles (the 1e-9-cycle contract is the weaker bound here)" % b)
            assert b < 1e-9
        if name == "taylor13":
            T = T_SPAN * 86400.0
            fact = 1.0
            for k in range(13):
                fact *= k + 1
                assert abs(tm["F%d" % k]) * T ** (k + 1) / fact >= 1e-3 and tm["F%d" % k] * (-1.0) ** k > 0
        # --- every parameter is visible
        check_visible(name, tm, t, m.A["total"])
        index[name] = [tkey, name]
        out[name + "_model"] = np.array(json.dumps(tm))
        out.update({name + "_hi": hi, name + "_lo": lo, name + "_A": a3, name + "_refd": refd})
    out["index"] = np.array(json.dumps(index))
    path = os.path.join(HERE, "calcphase_wide.npz")
    if check:
        old = np.load(path, allow_pickle=False)
        assert sorted(old.files) == sorted(out), "the set of arrays changed"
        for k, v in out.items():
            assert old[k].dtype == np.asarray(v).dtype and np.array_equal(old[k], v, equal_nan=False), k
        print("calcphase_wide.npz reproduces: %d arrays identical" % len(out))
    else:
        np.savez_compressed(path, **out)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")
    print("| model | total | Taylor | glitches | waves |")
    for name, r in table.items():
        print("| `%s` | %s |" % (name, " | ".join("%.1f" % r[p] for p in R.PARTS)))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--check"]
    if len(args) != 1:
        sys.exit(__doc__)
    main(args[0], "--check" in sys.argv[1:])
