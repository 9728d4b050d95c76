"""Regenerates tests/golden/toa_ll_wide.npz: the ToA likelihood sums, their template-shape gradients and the fitted
optimum of every template size at 60 digits (tests/likelihood_reference.py), beside the reference's own NumPy LL
(templatemodels.py:98-121, :201-226, :306-329).

    python tests/golden/gen_toa_ll_wide_golden.py path/to/CRIMP-v2.3.0/src [--check]

``--check`` regenerates everything, compares every array with the committed file and writes nothing. All seeds are
fixed. The oracle (oracle/) has to be built; only numbers the reference computed travel, none of its code.

Sums cases (one template, one photon set, 11 points each; SUMS_CASES below lists template size, photon count and
ampShift):
* Fourier K = 1..9, 12, 16, amplitudes decaying as j^-1.2, ph_j uniform over [-pi, 2 pi]; ``f7`` has interior zero
  amplitudes, ``f5`` a negative one; Cauchy with 1, 2, 5, 16 components of widths cycling through 0.02, 0.15, 1, 3;
  von Mises with 1, 3, 16 components of widths 0.04 (kappa = 625), 0.25, 1, 5; one case per model at ampShift 0.3 and 7.
* photon counts 0, 1, 2, 7, 8, 9, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1025, 4097 (both kernels' strides), 70 %
  drawn from the template, 30 % uniform; sets of >= 255 photons carry the special phases of ``specials``.
* points: phShift 0, +-bound, +-(bound - 1e-9), 1e-9 and three lattice values 0.05 k - bound at a comfortable norm
  (kind 0); one lattice value at the norm that leaves min m just positive (kind 1); one at a norm that makes the model
  negative at two photons 512 apart -- the same thread of crimp_toa_points -- or next to each other below 513 photons
  (kind 2: the reference answers -inf). Asserted: |min m| >= 1000 FACTOR u A_min at every point, the LL is -inf at
  exactly the kind-2 points, and the reference's NumPy LL is within the bound.
* stored per case: <name>_tpl (JSON), _x, _E, _pts (P, 2), _kind (P), _hi/_lo/_A (P, 8), _ll_hi/_ll_lo/_ll_A/_ll_ref
  (P), _shape_pts (the points with shape sums: one of kind 0, the kind-1 one), _sh_hi/_sh_lo/_sh_A (S, SHAPE_SUMS) and,
  von Mises, _sh0_* (S, 16): the width rows of the call without aux.

Fit cases (FIT_CASES): Fourier K = 1..16 at 600 photons, K = 3 and 8 at 4095, 4097, 8193, 8707 photons, Cauchy 1, 2, 5,
16 and von Mises 1, 3, 16 components at 600: photons drawn from the template shifted by a known 0.05..0.3 rad, exposure
N / norm. From the oracle's fit_toa optimum Newton runs in mpmath on (norm, phShift) until the 60-digit gradient is
below 1e-30. Asserted with the oracle: brutemin=True and False reach that maximum (else the next seed), the optimum is
interior to both bounds, and the two profile-LL drops that decide each 1-sigma bound are more than 1e-6 from
0.5 chi2_1(0.6827). Stored: <name>_tmpl (JSON), _x, _fit = [E, norm*, phi*, LL* hi, LL* lo, H_nn, H_np, H_pp,
A_LL, A_gn, A_gphi, phShi_LL, phShi_UL, reducedChi2] (the last three the oracle's).
"""
import json
import math
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
sys.dont_write_bytecode = True

import likelihood_reference as R  # noqa: E402

TWO_PI = 2 * math.pi
C_WID = (0.02, 0.15, 1.0, 3.0)
V_WID = (0.04, 0.25, 1.0, 5.0)
# name: (model, components, photons, ampShift)
SUMS_CASES = {
    "f1": ("fourier", 1, 4097, 1.0), "f2": ("fourier", 2, 1025, 1.0), "f3": ("fourier", 3, 513, 1.0),
    "f4": ("fourier", 4, 512, 1.0), "f5": ("fourier", 5, 511, 1.0), "f6": ("fourier", 6, 257, 1.0),
    "f7": ("fourier", 7, 256, 1.0), "f8": ("fourier", 8, 255, 1.0), "f9": ("fourier", 9, 17, 1.0),
    "f12": ("fourier", 12, 16, 1.0), "f16": ("fourier", 16, 513, 1.0),
    "f4_as03": ("fourier", 4, 15, 0.3), "f6_as7": ("fourier", 6, 9, 7.0),
    "c1": ("cauchy", 1, 1025, 1.0), "c2": ("cauchy", 2, 8, 1.0), "c5": ("cauchy", 5, 257, 1.0),
    "c16": ("cauchy", 16, 513, 1.0), "c2_as03": ("cauchy", 2, 7, 0.3), "c2_as7": ("cauchy", 2, 2, 7.0),
    "v1": ("vonmises", 1, 1, 1.0), "v3": ("vonmises", 3, 0, 1.0), "v16": ("vonmises", 16, 257, 1.0),
    "v3_as03": ("vonmises", 3, 256, 0.3), "v3_as7": ("vonmises", 3, 512, 7.0),
}
FIT_CASES = {}
for _k in range(1, 17):
    FIT_CASES["fit_f%d" % _k] = ("fourier", _k, 600)
for _k in (3, 8):
    for _n in (4095, 4097, 8193, 8707):
        FIT_CASES["fit_f%d_n%d" % (_k, _n)] = ("fourier", _k, _n)
for _k in (1, 2, 5, 16):
    FIT_CASES["fit_c%d" % _k] = ("cauchy", _k, 600)
for _k in (1, 3, 16):
    FIT_CASES["fit_v%d" % _k] = ("vonmises", _k, 600)


def seed_of(name, extra=0):
    return [sum(ord(c) * 131 ** i for i, c in enumerate(name)) % (2 ** 31), extra]


def make_template(name, model, K, amp_shift):
    rng = np.random.default_rng(seed_of(name))
    j = np.arange(1, K + 1)
    if model == "fourier":
        amp = 0.45 * j ** -1.2 * rng.uniform(0.7, 1.0, K)
        if name == "f7":
            amp[[2, 4]] = 0.0
        if name == "f5":
            amp[1] = -amp[1]
        loc = rng.uniform(-math.pi, TWO_PI, K)
        return {"model": model, "amp": amp.tolist(), "loc": loc.tolist(), "amp_shift": amp_shift}
    wset = C_WID if model == "cauchy" else V_WID
    wid = [wset[i % 4] for i in range(K)]
    amp = rng.uniform(0.5, 2.0, K) / max(1.0, K / 4.0)
    loc = rng.uniform(0.0, TWO_PI, K)
    return {"model": model, "amp": amp.tolist(), "loc": loc.tolist(), "wid": wid, "amp_shift": amp_shift}


def h_np(tpl, x, phi):
    """h = model - norm in fp64, the reference's formula."""
    from scipy.special import i0
    x = np.asarray(x, dtype=np.float64)
    h = np.zeros_like(x)
    A = tpl["amp_shift"]
    for j, (a, l) in enumerate(zip(tpl["amp"], tpl["loc"]), start=1):
        if tpl["model"] == "fourier":
            h = h + a * A * np.cos(j * 2 * np.pi * x + l - j * phi)
        elif tpl["model"] == "cauchy":
            w = tpl["wid"][j - 1]
            h = h + ((a * A) / TWO_PI) * (np.sinh(w) / (np.cosh(w) - np.cos(x - l - phi)))
        else:
            k = 1 / tpl["wid"][j - 1] ** 2
            h = h + ((a * A) / (TWO_PI * i0(k))) * np.exp(k * np.cos(x - l - phi))
    return h


def draw(tpl, n, norm, shift, rng, frac=1.0):
    """n phases (cycles for fourier, radians otherwise): ``frac`` of them from norm + h(.; shift), the rest uniform."""
    upper = 1.0 if tpl["model"] == "fourier" else TWO_PI
    nt = int(round(frac * n))
    out = np.empty(0)
    grid = norm + h_np(tpl, np.linspace(0, upper, 20001), shift)
    ymax = 1.05 * grid.max()
    while out.size < nt:
        xs = rng.uniform(0.0, upper, 4 * (nt - out.size) + 16)
        keep = rng.uniform(0.0, ymax, xs.size) < norm + h_np(tpl, xs, shift)
        out = np.concatenate([out, xs[keep]])
    out = np.concatenate([out[:nt], rng.uniform(0.0, upper, n - nt)])
    return rng.permutation(out)


def specials(tpl, phis):
    """The special phases: quarter turns, the end of the turn, 1e-12..1e-3 from 0 and 1/2, table nodes k/4096 with
    their fp64 neighbours, the ties (k + 1/2)/4096 and, Cauchy / von Mises, every peak cen_j + phShift and the point
    half a turn from it (first two components, two phShift values)."""
    t = [0.0, 0.25, 0.5, 0.75, 1.0 - 2.0 ** -53, 1.0]
    for e in (1e-12, 1e-9, 1e-6, 1e-3):
        t += [e, 1.0 - e, 0.5 - e, 0.5 + e]
    for k in (1, 1023, 2047, 2048, 3071, 4095):
        v = k / 4096.0
        t += [np.nextafter(v, 0.0), v, np.nextafter(v, 1.0), (k + 0.5) / 4096.0]
    t = np.array(t)
    if tpl["model"] == "fourier":
        return t
    t = t * TWO_PI                               # 1.0 -> 2 pi; the nodes and ties to the nearest fp64
    peaks = []
    for j in range(min(2, len(tpl["loc"]))):
        for phi in phis[:2]:
            p = (tpl["loc"][j] + phi) % TWO_PI
            peaks += [p, (p + math.pi) % TWO_PI]
    return np.concatenate([t, peaks])


def build_sums_case(name):
    model, K, n, amp_shift = SUMS_CASES[name]
    tpl = make_template(name, model, K, amp_shift)
    rng = np.random.default_rng(seed_of(name, 1))
    b = R.PH_BOUND[model]
    size = sum(abs(a) * amp_shift for a in tpl["amp"])
    comfortable = 1.25 * size + 0.1 if model == "fourier" else 0.5
    lat = [0.05 * k - b for k in (7, 63, 100)]
    phis = [0.0, b, -b, b - 1e-9, -(b - 1e-9), 1e-9] + lat
    phi_t, phi_n = 0.05 * 41 - b, 0.05 * 88 - b
    x = draw(tpl, n, comfortable, 0.1, rng, frac=0.7)
    if n >= 255:
        sp = specials(tpl, [phi_t, 0.0])
        x[1:1 + sp.size] = sp
    pts = [(comfortable, p) for p in phis]
    kind = [0] * len(pts)
    E = max(n, 1) / comfortable if model == "fourier" else max(n, 1) / (comfortable + size / TWO_PI)
    designed = []
    if n >= 1:
        xmin = x[int(np.argmin(h_np(tpl, x, phi_n)))]
        designed = [n - 1] if n == 1 else [n - 1 - 512 if n > 512 else n - 2, n - 1]
        x[designed] = xmin                       # clear of the special phases at 1..
        scale = abs(comfortable) + size
        ht = h_np(tpl, x, phi_t)
        pts.append((-ht.min() + 1e-6 * scale, phi_t))
        kind.append(1)
        pts.append((-h_np(tpl, x, phi_n).min() - 1e-3 * scale, phi_n))
        kind.append(2)
    else:
        pts += [(comfortable, phi_t), (comfortable, phi_n)]
        kind += [0, 0]
    pts = np.array(pts, dtype=np.float64)
    kind = np.array(kind, dtype=np.int8)
    res = R.points_mp(tpl, x, pts)
    P = len(pts)
    hi, lo, A = R.pack([v for r in res for v in r[0]], [a for r in res for a in r[1]], (P, 8))
    lls = []
    for p in range(P):
        if n == 0:
            lls.append((R._mp().nan, R._mp().mpf(0)))
            continue
        lls.append(R.ll_mp(tpl, n, pts[p, 0], E, res[p][0][0], res[p][1][0], res[p][0][6]))
        # the sign of the minimum is never in doubt
        mn, amn = float(res[p][0][6]), float(res[p][1][6])
        assert abs(mn) >= 1000 * R.FACTOR * R.U * amn, (name, p, mn, amn)
        assert (float(lls[-1][0]) == -np.inf) == (kind[p] == 2), (name, p, kind[p])
        if kind[p] == 2:
            neg = np.nonzero(pts[p, 0] + h_np(tpl, x, pts[p, 1]) < 0)[0]
            assert set(designed) <= set(neg.tolist()), (name, designed, neg)
    ll_hi, ll_lo, ll_A = R.pack([v[0] for v in lls], [v[1] for v in lls])
    out = {"tpl": np.array(json.dumps(tpl)), "x": x, "E": np.float64(E), "pts": pts, "kind": kind, "hi": hi,
           "lo": lo, "A": A, "ll_hi": ll_hi, "ll_lo": ll_lo, "ll_A": ll_A}
    spts = [0] if n == 0 else [2, int(np.nonzero(kind == 1)[0][0])]
    sh = [R.shape_mp(tpl, x, pts[p, 0], pts[p, 1], aux=True) for p in spts]
    out["shape_pts"] = np.array(spts, dtype=np.int64)
    out["sh_hi"], out["sh_lo"], out["sh_A"] = R.pack([v for r in sh for v in r[0]], [a for r in sh for a in r[1]],
                                                     (len(spts), R.SHAPE_SUMS))
    if model == "vonmises":
        s0 = [R.shape_mp(tpl, x, pts[p, 0], pts[p, 1], aux=False) for p in spts]
        wv = [v for r in s0 for v in r[0][6::3]]
        wa = [a for r in s0 for a in r[1][6::3]]
        out["sh0_hi"], out["sh0_lo"], out["sh0_A"] = R.pack(wv, wa, (len(spts), R.MAX_COMP))
    print("  sums case", name, model, K, n, flush=True)
    return name, out


def tmpl_dict(tpl, norm):
    """readPPtemplate's form of a template."""
    t = {"model": tpl["model"], "norm": {"value": norm, "vary": True}}
    loc = "ph" if tpl["model"] == "fourier" else "cen"
    for j, a in enumerate(tpl["amp"], start=1):
        t["amp_%d" % j] = {"value": a, "vary": False}
        t["%s_%d" % (loc, j)] = {"value": tpl["loc"][j - 1], "vary": False}
        if "wid" in tpl:
            t["wid_%d" % j] = {"value": tpl["wid"][j - 1], "vary": False}
    return t


def newton_mp(tpl, x, E, n0, p0):
    """The 60-digit maximum of LL(norm, phShift) from (n0, p0): (norm, phi, sums at the fp64 roundings of it)."""
    mp = R._mp()
    n, p = mp.mpf(float(n0)), mp.mpf(float(p0))
    for _ in range(12):
        (v, _a), = R.points_mp(tpl, x, [(n, p)])
        gn, gp = v[1] - mp.mpf(float(E)), v[2]
        if max(abs(gn), abs(gp)) < mp.mpf(10) ** -30:
            return n, p
        hnn, hnp, hpp = v[3], v[4], v[5]
        det = hnn * hpp - hnp * hnp
        n, p = n - (hpp * gn - hnp * gp) / det, p - (hnn * gp - hnp * gn) / det
    raise AssertionError("Newton did not converge")


def scan_margin(O, x, E, tarr, lo, hi, fit, res):
    """Distance from 0.5 chi2_1(0.6827) of the two profile-LL drops that decide each 1-sigma bound."""
    step = TWO_PI / res
    out = []
    for side, key in ((-1, "phShi_LL"), (1, "phShi_UL")):
        kk = int(round((fit[key] - step / 2) / step)) - 1          # the last step evaluated: the first above the level
        for k in (kk - 1, kk):
            if k < 1:
                continue
            _, o = O._profile_norm(x, E, tarr, fit["phShi"] + side * k * step, lo, hi, fit["norm"])
            out.append(abs((fit["LLmax"] - o[0]) - O.CHI2_1SIG_1DOF))
    return min(out)


def build_fit_case(name):
    from oracle import oracle as O
    model, K, n = FIT_CASES[name]
    for attempt in range(20):
        rng = np.random.default_rng(seed_of(name, 100 + attempt))
        tpl = make_template("fit_%s%d" % (model[0], K), model, K, 1.0)     # one template per size: the N variants share it
        size = sum(abs(a) for a in tpl["amp"])
        norm = 1.25 * size + 0.1 if model == "fourier" else 0.5
        shift = float(rng.uniform(0.05, 0.3))
        x = draw(tpl, n, norm, shift, rng)
        E = n / norm if model == "fourier" else n / (norm + size / TWO_PI)
        tm = tmpl_dict(tpl, norm)
        a, b = O.fit_toa(x, E, tm, brutemin=False), O.fit_toa(x, E, tm, brutemin=True)
        if abs(a["phShi"] - b["phShi"]) > 1e-8 or abs(a["norm"] - b["norm"]) > 1e-8 * a["norm"]:
            continue
        tarr = O.template_arrays(tm)
        if scan_margin(O, x, E, tarr, norm / 100.0, 500.0, a, 1000) <= 1e-6 or a["phShi_LL"] != b["phShi_LL"] or \
                a["phShi_UL"] != b["phShi_UL"]:
            continue
        ns, ps = newton_mp(tpl, x, E, a["norm"], a["phShi"])
        if abs(float(ns) - a["norm"]) > 1e-7 * a["norm"] or abs(float(ps) - a["phShi"]) > 1e-7:
            continue
        pb = R.PH_BOUND[model]
        assert norm / 100.0 < float(ns) < 500.0 and -pb + 0.5 < float(ps) < pb - 0.5
        (v, A), = R.points_mp(tpl, x, [(ns, ps)])
        ll, a_ll = R.ll_mp(tpl, n, ns, E, v[0], A[0], v[6])
        (lh,), (ll_lo,) = R.hi_lo([ll])
        fit = [E, float(ns), float(ps), lh, ll_lo, float(v[3]), float(v[4]), float(v[5]), float(a_ll),
               float(A[1]) + E, float(A[2]), a["phShi_LL"], a["phShi_UL"], a["reducedChi2"]]
        print("  fit case", name, "attempt", attempt, "norm %.6f phi %.6f" % (fit[1], fit[2]), flush=True)
        return name, {"tmpl": np.array(json.dumps(tm)), "x": x, "fit": np.array(fit, dtype=np.float64)}
    raise AssertionError("no seed gives an unambiguous fit for " + name)


def record_reference(src, out):
    """The reference's own NumPy LL at every point of every sums case; asserts it is within the bound and -inf at
    exactly the designed points."""
    sys.path.insert(0, src)
    import crimp.templatemodels as T
    cls = {"fourier": (T.Fourier, "loglikelihoodFSnormalized"), "cauchy": (T.WrappedCauchy, "loglikelihoodCAnormalized"),
           "vonmises": (T.VonMises, "loglikelihoodVMnormalized")}
    worst = {}
    for name in SUMS_CASES:
        g = {k[len(name) + 1:]: v for k, v in out.items() if k.startswith(name + "_")}
        tpl = json.loads(str(g["tpl"]))
        c = R.Case.__new__(R.Case)
        c.tpl, c.model, c.pts = tpl, tpl["model"], g["pts"]
        c.ll_hi, c.ll_lo, c.ll_A = g["ll_hi"], g["ll_lo"], g["ll_A"]
        ref = np.full(len(g["pts"]), np.nan)
        if g["x"].size:
            k, fn = cls[c.model]
            for p in range(len(g["pts"])):
                ref[p] = getattr(k(c.theta(p), g["x"]), fn)(float(g["E"]))
            assert np.array_equal(ref == -np.inf, g["kind"] == 2), (name, ref, g["kind"])
            r = c.ll_ratio(ref)
            worst[c.model] = max(worst.get(c.model, 0.0), r)
            assert r <= R.FACTOR, (name, r)
        out[name + "_ll_ref"] = ref
    print("reference LL, max |err| / (u A) per model:", {k: round(v, 2) for k, v in worst.items()})


def main(src, check):
    out = {}
    with Pool(min(24, os.cpu_count() or 1)) as pool:
        fits = pool.map_async(build_fit_case, list(FIT_CASES), chunksize=1)
        sums = pool.map_async(build_sums_case, list(SUMS_CASES), chunksize=1)
        for name, d in sums.get() + fits.get():
            out.update({name + "_" + k: v for k, v in d.items()})
    record_reference(src, out)
    out["index"] = np.array(json.dumps({"sums": list(SUMS_CASES), "fits": list(FIT_CASES)}))
    path = os.path.join(HERE, "toa_ll_wide.npz")
    if check:
        old = np.load(path, allow_pickle=False)
        assert sorted(old.files) == sorted(out), "the set of arrays changed"
        for k, v in out.items():
            v = np.asarray(v)
            assert old[k].dtype == v.dtype and np.array_equal(old[k], v, equal_nan=v.dtype.kind == "f"), k
        print("toa_ll_wide.npz reproduces: %d arrays identical" % len(out))
    else:
        np.savez_compressed(path, **out)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--check"]
    if len(args) != 1:
        sys.exit(__doc__)
    main(args[0], "--check" in sys.argv[1:])
