"""CPU checks behind tests/test_gpu_toa_ll.py: the wide ToA-likelihood fixture against the 60-digit formulas it was
made from, what it covers, the reference's recorded LL and the oracle against it (the bound is not too tight), and a
NumPy restatement of the kernels' own arithmetic with and without deliberate defects (it is not too loose).

The bound everywhere is |x - mp| <= 32 u A per sum (tests/likelihood_reference.py); the printed figures are the largest
|x - mp| / (u A) per model and sum."""
import math

import numpy as np
import pytest

import likelihood_reference as R

TWO_PI = 2 * math.pi
REDERIVED = {"fourier": ("f9", "f12", "f4_as03"), "cauchy": ("c2", "c2_as03", "c2_as7"),
             "vonmises": ("v1", "v3", "v3_as03")}


@pytest.fixture(scope="module")
def wide():
    return R.load_wide()


def test_fixture_rederives_from_the_formula(wide):
    """hi, lo and A of three cases per model -- the eight sums at every point, the LL, the shape sums with and without
    aux -- re-derive bit for bit from likelihood_reference at 60 digits."""
    sums, _ = wide
    for model, names in REDERIVED.items():
        for name in names:
            c = sums[name]
            assert c.model == model
            res = R.points_mp(c.tpl, c.x, c.pts)
            P = len(c.pts)
            hi, lo, A = R.pack([v for r in res for v in r[0]], [a for r in res for a in r[1]], (P, 8))
            for got, want, what in ((hi, c.hi, "hi"), (lo, c.lo, "lo"), (A, c.A, "A")):
                np.testing.assert_array_equal(got, want, err_msg="%s %s" % (name, what))
            if c.x.size:
                ll = [R.ll_mp(c.tpl, c.x.size, c.pts[p, 0], c.E, res[p][0][0], res[p][1][0], res[p][0][6])
                      for p in range(P)]
                for got, want in zip(R.pack([v[0] for v in ll], [v[1] for v in ll]), (c.ll_hi, c.ll_lo, c.ll_A)):
                    np.testing.assert_array_equal(got, want, err_msg=name + " LL")
            sh = [R.shape_mp(c.tpl, c.x, c.pts[p, 0], c.pts[p, 1]) for p in c.shape_pts]
            got = R.pack([v for r in sh for v in r[0]], [a for r in sh for a in r[1]], (len(sh), R.SHAPE_SUMS))
            for g, want in zip(got, (c.sh_hi, c.sh_lo, c.sh_A)):
                np.testing.assert_array_equal(g, want, err_msg=name + " shape")
            if model == "vonmises":
                s0 = [R.shape_mp(c.tpl, c.x, c.pts[p, 0], c.pts[p, 1], aux=False) for p in c.shape_pts]
                got = R.pack([v for r in s0 for v in r[0][6::3]], [a for r in s0 for a in r[1][6::3]],
                             (len(s0), R.MAX_COMP))
                for g, want in zip(got, (c.sh0_hi, c.sh0_lo, c.sh0_A)):
                    np.testing.assert_array_equal(g, want, err_msg=name + " shape without aux")


def _has(x, v):
    return bool(np.any(x == v))


def test_fixture_covers_what_it_claims(wide):
    sums, fits = wide
    by = {m: [c for c in sums.values() if c.model == m] for m in R.MODELS}
    assert sorted(len(c.tpl["amp"]) for c in by["fourier"] if c.tpl["amp_shift"] == 1.0) == \
        [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16]
    assert sorted(len(c.tpl["amp"]) for c in by["cauchy"] if c.tpl["amp_shift"] == 1.0) == [1, 2, 5, 16]
    assert sorted(len(c.tpl["amp"]) for c in by["vonmises"] if c.tpl["amp_shift"] == 1.0) == [1, 3, 16]
    for m in R.MODELS:
        assert sorted(c.tpl["amp_shift"] for c in by[m] if c.tpl["amp_shift"] != 1.0) == [0.3, 7.0]
    assert sorted(set(c.x.size for c in sums.values())) == \
        [0, 1, 2, 7, 8, 9, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1025, 4097]
    a7, a5 = sums["f7"].tpl["amp"], sums["f5"].tpl["amp"]
    assert a7[2] == 0 and a7[4] == 0 and a7[6] != 0 and sum(1 for a in a5 if a < 0) == 1
    ph = np.concatenate([c.tpl["loc"] for c in by["fourier"]])
    assert ph.min() < -0.8 * math.pi and ph.max() > 1.8 * math.pi
    assert set(w for c in by["cauchy"] for w in c.tpl["wid"]) == {0.02, 0.15, 1.0, 3.0}
    assert set(w for c in by["vonmises"] for w in c.tpl["wid"]) == {0.04, 0.25, 1.0, 5.0}
    for c in sums.values():
        n, b = c.x.size, R.PH_BOUND[c.model]
        turn = 1.0 if c.model == "fourier" else TWO_PI
        assert 8 <= len(c.pts) <= 12
        for v in (0.0, b, -b, b - 1e-9, -(b - 1e-9), 1e-9, 0.05 * 7 - b):
            assert _has(c.pts[:, 1], v), (c.name, v)
        # the three kinds of norm, the -inf set exactly the designed one
        if n:
            assert sorted(set(c.kind.tolist())) == [0, 1, 2] and np.sum(c.kind == 2) == 1
            assert np.array_equal(c.ll_hi == -np.inf, c.kind == 2) and not np.any(np.isnan(c.ll_hi))
            assert np.array_equal(c.ll_ref == -np.inf, c.kind == 2)
            mn = c.hi[:, 6]
            assert np.all(mn[c.kind == 2] < 0) and np.all(mn[c.kind != 2] > 0)
            assert np.all(np.abs(mn) >= 1000 * R.FACTOR * R.U * c.A[:, 6])
            assert np.all(mn[c.kind == 1] < 1e-4 * mn[c.kind == 0].min())
            assert np.array_equal(np.isnan(c.hi[:, 0]), c.kind == 2)
        else:
            assert np.all(c.hi[:, :6] == 0) and np.all(c.hi[:, 6] == np.inf) and np.all(c.hi[:, 7] == 0)
        if n >= 2:      # the designed negative photons share a thread of the 512- and the 256-thread kernels
            i2 = n - 1
            i1 = i2 - 512 if n > 512 else i2 - 1
            assert c.x[i1] == c.x[i2]
            p = int(np.nonzero(c.kind == 2)[0][0])
            assert c.hi[p, 6] < 0
        if n >= 255:    # the special phases
            for v in (0.0, 0.25, 0.5, 0.75, 1.0):
                assert _has(c.x, v * turn), (c.name, v)
            if c.model == "fourier":
                assert _has(c.x, 1.0 - 2.0 ** -53)
                for k in (1, 2047, 2048, 4095):
                    v = k / 4096.0
                    assert _has(c.x, v) and _has(c.x, np.nextafter(v, 0.0)) and _has(c.x, np.nextafter(v, 1.0))
                    assert _has(c.x, (k + 0.5) / 4096.0)
            else:
                p = int(np.nonzero(c.kind == 1)[0][0])
                peak = (c.tpl["loc"][0] + c.pts[p, 1]) % TWO_PI
                assert _has(c.x, peak) and _has(c.x, (peak + math.pi) % TWO_PI)
            for e in (1e-12, 1e-9, 1e-6, 1e-3):
                assert _has(c.x, e * turn) and _has(c.x, (0.5 + e) * turn) and _has(c.x, (0.5 - e) * turn)
    # fit cases: every size, the product tails, the optimum interior to both bounds
    assert sorted(f.K for f in fits.values() if f.model == "fourier" and f.x.size == 600) == list(range(1, 17))
    for k in (3, 8):
        assert sorted(f.x.size for f in fits.values() if f.model == "fourier" and f.K == k and f.x.size != 600) == \
            [4095, 4097, 8193, 8707]
    assert sorted(f.K for f in fits.values() if f.model == "cauchy") == [1, 2, 5, 16]
    assert sorted(f.K for f in fits.values() if f.model == "vonmises") == [1, 3, 16]
    for f in fits.values():
        n0 = f.tmpl["norm"]["value"]
        assert n0 / 100 * 1.5 < f.norm < 400 and abs(f.phi) < 0.5 < R.PH_BOUND[f.model]
        assert f.hnn < 0 and f.hpp < 0 and np.linalg.det(f.H) > 0


def _table(rows, title):
    print()
    for model, r in rows.items():
        print("%s %-9s max |err|/(u A): " % (title, model) + "  ".join("%s %.2f" % kv for kv in r.items()))


def _worse(rows, model, key, v):
    r = rows.setdefault(model, {})
    v = float("inf") if v != v else float(v)                 # a NaN is never the smaller figure
    r[key] = max(r.get(key, 0.0), v)


def test_reference_ll_within_bound(wide):
    sums, _ = wide
    rows = {}
    for c in sums.values():
        if c.x.size:
            _worse(rows, c.model, "LL", c.ll_ratio(c.ll_ref))
    _table(rows, "reference")
    assert max(v for r in rows.values() for v in r.values()) <= R.FACTOR, rows


def _oracle_tarr(c):
    from oracle import oracle as O
    t = {"model": c.model}
    loc = "ph" if c.model == "fourier" else "cen"
    for j, a in enumerate(c.tpl["amp"], start=1):
        t["amp_%d" % j], t["%s_%d" % (loc, j)] = a, c.tpl["loc"][j - 1]
        if c.model != "fourier":
            t["wid_%d" % j] = c.tpl["wid"][j - 1]
    return O.template_arrays(t)


def test_oracle_within_bound(wide):
    """toa_eval's LL, gradient, Hessian and minimum at every point of every case (the gradient in norm is out[1] + E,
    the minimum out[6] F: one more rounding each, of the size of the compared value)."""
    from oracle import oracle as O
    sums, fits = wide
    rows = {}
    for c in sums.values():
        if not c.x.size:
            continue
        tarr = _oracle_tarr(c)
        o = np.array([O.toa_eval(c.x, c.E, tarr, n, p, amp_shift=c.tpl["amp_shift"]) for n, p in c.pts])
        assert np.array_equal(o[:, 0] == -np.inf, c.kind == 2)
        _worse(rows, c.model, "LL", c.ll_ratio(o[:, 0]))
        F = np.array([R.norm_factor(c.tpl, n) for n in c.pts[:, 0]])
        for s, val, extra in (("q", o[:, 1] + c.E, c.E), ("h1q", o[:, 2], 0), ("mq2", o[:, 3], 0), ("mh1q2", o[:, 4], 0),
                              ("hess", o[:, 5], 0), ("min", o[:, 6] * F, np.abs(c.hi[:, 6]))):
            k = R.SUMS.index(s)
            r = R.err_ratio(val, c.hi[:, k], c.lo[:, k], c.A[:, k] + extra)
            _worse(rows, c.model, s, float(r.max()))
    _table(rows, "oracle   ")
    assert max(v for r in rows.values() for v in r.values()) <= R.FACTOR, rows
    for f in fits.values():                  # the stored optimum is the oracle's maximum
        o = O.toa_eval(f.x, f.E, O.template_arrays(f.tmpl), f.norm, f.phi)
        assert abs((o[0] - f.ll_hi) - f.ll_lo) <= R.FACTOR * R.U * f.A_ll, f.name
        step = np.linalg.solve(f.H, [o[1], o[2]])
        bound = np.linalg.norm(np.linalg.inv(f.H), 2) * R.FACTOR * R.U * math.hypot(f.A_gn, f.A_gp)
        assert abs(step[0]) <= bound + 1e-15 * f.norm and abs(step[1]) <= bound + 1e-15, (f.name, step, bound)


# ------------------------------------------------------------------------------- the kernels' arithmetic in NumPy
INV_2PI = 0.15915494309189533577
TAB = np.stack([np.cos(np.arange(4096) * (TWO_PI / 4096)), np.sin(np.arange(4096) * (TWO_PI / 4096))])


def kernel_points(tpl, x, norm, phi, defect=None):
    """crimp_toa_points' eight sums as the kernel forms them (make_tpl, tpl_coef, photon_sincos_tab, tpl_terms, the
    512 strided per-thread sums), the reciprocal as a plain division. ``defect`` plants one deliberate error."""
    from scipy.special import i0
    model, A = tpl["model"], tpl["amp_shift"]
    amp, loc = np.array(tpl["amp"]) * A, np.array(tpl["loc"])
    K = amp.size
    if defect == "drop_last":
        K -= 1
    x = np.asarray(x, dtype=np.float64)
    if defect == "skip_photon":
        x = x[:-1]
    j = np.arange(1, amp.size + 1, dtype=np.float64)
    if model == "fourier":
        d = loc - j * phi
        c0, cs = amp * np.cos(d), -amp * np.sin(d)
        if defect == "flip_b":
            cs[0] = -cs[0]
        r = x
    else:
        w = np.array(tpl["wid"])
        d = loc + phi
        c0, cs = np.cos(d), np.sin(d)
        inv = float(np.float32(INV_2PI)) if defect == "inv2pi_f32" else INV_2PI
        r = x * inv
        if model == "cauchy":
            ta, ch = (amp / TWO_PI) * np.sinh(w), np.cosh(w)
            if defect == "width_f32":
                ch = ch.astype(np.float32).astype(np.float64)
        else:
            kap = 1.0 / (w * w)
            ta = amp / (TWO_PI * i0(kap))
            if defect == "width_f32":
                kap = kap.astype(np.float32).astype(np.float64)
    k = np.rint(r * 4096.0)
    dl = (r - k / 4096.0) * TWO_PI
    d2 = dl * dl
    cd = d2 * (d2 * (1.0 / 24.0) - 0.5) + 1.0
    sd = dl * (d2 * (d2 * (1.0 / 120.0) - 1.0 / 6.0) + 1.0)
    e = TAB[:, k.astype(np.int64) & 4095]
    s1, c1 = e[1] * cd + e[0] * sd, e[0] * cd - e[1] * sd
    h, h1, h2 = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    if model == "fourier":
        tc = c1 + c1
        cj, sj, cp, sp = c1, s1, np.ones_like(x), np.zeros_like(x)
        for i in range(K):
            tj = c0[i] * cj + cs[i] * sj
            jj = float(i + 1)
            h = h + tj
            h2 = h2 - (jj if defect == "h2_weight_j" else jj * jj) * tj
            h1 = h1 + jj * (c0[i] * sj - cs[i] * cj)
            cj, sj, cp, sp = tc * cj - cp, tc * sj - sp, cj, sj
    else:
        for i in range(K):
            cu, su = c1 * c0[i] + s1 * cs[i], s1 * c0[i] - c1 * cs[i]
            if model == "cauchy":
                iD = 1.0 / (ch[i] - cu)
                v = ta[i] * iD
                h, h1, h2 = h + v, h1 + v * su * iD, h2 - v * iD * (cu - 2.0 * su * su * iD)
            else:
                v = ta[i] * np.exp(kap[i] * cu)
                h, h1, h2 = h + v, h1 + kap[i] * su * v, h2 + (-kap[i] * cu + kap[i] * kap[i] * su * su) * v
    mv = norm + h
    with np.errstate(invalid="ignore", divide="ignore"):
        q = 1.0 / mv
        terms = [np.log(mv), q, h1 * q, -(q * q), -(h1 * q * q), h2 * q - h1 * h1 * q * q]
    out = np.zeros(8)
    for s, t in enumerate(terms):
        pad = np.zeros(-(-max(t.size, 1) // 512) * 512)
        pad[:t.size] = t
        out[s] = np.sum(np.sum(pad.reshape(-1, 512), axis=0))       # per-thread strided sums, then the tree
    out[6] = mv.min() if mv.size else np.inf
    out[7] = x.size
    return out


def kernel_ll(c, s, p):
    """templatemodels._extended_ll's host assembly from the sums of point p."""
    n, N = c.pts[p, 0], s[7]
    F = R.norm_factor(c.tpl, n)
    if not s[6] / F > 0:
        return -np.inf
    if c.model == "fourier":
        return -n * c.E + N * np.log(n * c.E) + (s[0] - N * np.log(n))
    return -F * c.E / TWO_PI + N * np.log(F * c.E / TWO_PI) + (s[0] - N * np.log(F))


def _kernel_ratios(sums, defect=None, models=R.MODELS):
    rows, worst = {}, {}
    for c in sums.values():
        if c.model not in models or not c.x.size:
            continue
        s = np.array([kernel_points(c.tpl, c.x, n, p, defect) for n, p in c.pts])
        for k, name in enumerate(R.SUMS):
            r = float(R.err_ratio(s[:, k], c.hi[:, k], c.lo[:, k], c.A[:, k]).max())
            _worse(rows, c.model, name, r)
            worst[name] = max(worst.get(name, 0.0), r)
        ll = np.array([kernel_ll(c, s[p], p) for p in range(len(c.pts))])
        if defect is None:
            assert np.array_equal(ll == -np.inf, c.kind == 2), c.name
        fin = np.isfinite(ll) & np.isfinite(c.ll_hi)
        r = float(R.err_ratio(ll[fin], c.ll_hi[fin], c.ll_lo[fin], c.ll_A[fin]).max()) if fin.any() else 0.0
        _worse(rows, c.model, "LL", r)
        worst["LL"] = max(worst.get("LL", 0.0), r)
    return rows, worst


def test_kernel_arithmetic_within_bound(wide):
    """The table reduction, the Chebyshev recurrence and the strided sums, restated in NumPy, stay within the bound on
    every case, point and sum."""
    rows, worst = _kernel_ratios(wide[0])
    _table(rows, "kernel arithmetic (NumPy)")
    assert max(worst.values()) <= R.FACTOR, rows


@pytest.mark.parametrize("defect,models,sums_hit", [
    ("inv2pi_f32", ("cauchy", "vonmises"), ("lnm", "q", "h1q", "hess", "LL")),
    ("drop_last", R.MODELS, ("lnm", "q", "h1q", "mq2", "mh1q2", "hess", "min", "LL")),
    ("h2_weight_j", ("fourier",), ("hess",)),
    ("skip_photon", R.MODELS, ("lnm", "q", "mq2", "N", "LL")),
    ("width_f32", ("cauchy", "vonmises"), ("lnm", "q", "h1q", "hess", "LL")),
    ("flip_b", ("fourier",), ("lnm", "q", "h1q", "hess", "LL")),
])
def test_defects_exceed_the_bound(wide, defect, models, sums_hit):
    """1/(2 pi) in float32, the last harmonic or component dropped, h'' weighted by j, one photon left out, kappa /
    cosh w in float32, the sign of one b_j flipped: each breaks the bound, in every model it applies to and every sum
    it reaches."""
    for m in models:
        rows, worst = _kernel_ratios(wide[0], defect, (m,))
        for s in sums_hit:
            assert rows[m][s] > R.FACTOR, (defect, m, s, rows[m])
