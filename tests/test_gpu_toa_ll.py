"""The ToA likelihood kernels -- k_toa_points, every instance of k_toa_fit, k_toa_shape and the brute grid at every
template size -- against the 60-digit fixture tests/golden/toa_ll_wide.npz (tests/likelihood_reference.py; the CPU
side of the bound is tests/test_toa_ll_host.py).

Every sum has to lie within FACTOR u A = 32 u A of the 60-digit value; the printed figures are the largest
|x - mp| / (u A) per model and sum. Only the fixture and the oracle are read here."""
import math

import numpy as np
import pytest

import likelihood_reference as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu
TWO_PI = 2 * math.pi
PAD = 3          # photons of a second interval behind every case's own (an empty case sits beside a full interval)


@pytest.fixture(scope="module")
def wide():
    return R.load_wide()


def _template(c, amp_shift=None):
    from crimp_amd import ops
    return ops.make_template(c.model, c.tpl["amp"], c.tpl["loc"], c.tpl.get("wid"),
                             amp_shift=c.tpl["amp_shift"] if amp_shift is None else amp_shift)


def _padded(c):
    fill = np.full(PAD, 0.25 if c.model == "fourier" else 1.0)
    return np.concatenate([c.x, fill]), np.array([0, c.x.size, c.x.size + PAD], dtype=np.int64)


def _table(rows, title):
    print()
    for model, r in rows.items():
        print("%s %-9s max |err|/(u A): " % (title, model) + "  ".join("%s %.2f" % kv for kv in r.items()))


def _worse(rows, model, key, v):
    r = rows.setdefault(model, {})
    v = float("inf") if v != v else float(v)                 # a NaN is never the smaller figure
    r[key] = max(r.get(key, 0.0), v)


def test_toa_points_every_case_within_bound(gpu, wide):
    """crimp_toa_points at every case, point and sum: the six sums within 32 u A, min m within its own unit, N exact,
    the assembled LL finite exactly where the fixture's is; templatemodels' three likelihoods -inf exactly there and
    within the LL bound elsewhere."""
    from crimp_amd import ops, templatemodels as T
    sums, _ = wide
    ll_of = {"fourier": lambda th, x, E: T.Fourier(th, x).loglikelihoodFSnormalized(E),
             "cauchy": lambda th, x, E: T.WrappedCauchy(th, x).loglikelihoodCAnormalized(E),
             "vonmises": lambda th, x, E: T.VonMises(th, x).loglikelihoodVMnormalized(E)}
    rows, bad = {}, []
    for c in sums.values():
        x, off = _padded(c)
        P = len(c.pts)
        s = ops.toa_points(x, off, _template(c), np.zeros(P, np.int64), c.pts[:, 0].copy(), c.pts[:, 1].copy())
        assert np.array_equal(s[:, 7], np.full(P, float(c.x.size))), c.name
        for k, name in enumerate(R.SUMS[:7]):
            r = c.ratio(s[:, k], k)
            _worse(rows, c.model, name, r)
            if not r <= R.FACTOR:
                bad.append((c.name, name, r))
        if not c.x.size:
            assert np.all(s[:, :6] == 0) and np.all(s[:, 6] == np.inf)
            continue
        F = np.array([R.norm_factor(c.tpl, n) for n in c.pts[:, 0]])
        assert np.array_equal(s[:, 6] / F > 0, np.isfinite(c.ll_hi)), c.name
        ll = np.array([ll_of[c.model](c.theta(p), c.x, c.E) for p in range(P)])
        assert np.array_equal(ll == -np.inf, c.kind == 2), (c.name, ll)
        r = c.ll_ratio(ll)
        _worse(rows, c.model, "LL", r)
        if not r <= R.FACTOR:
            bad.append((c.name, "LL", r))
    _table(rows, "k_toa_points")
    assert not bad, bad


@pytest.mark.parametrize("name", ["f3", "v16"])
def test_toa_points_grouping_and_abi_edges(gpu, wide, name):
    """Calls of 1, 4, 5 and 9 points, an interval change in the middle of a group of four, unsorted pt_interval, an
    empty interval beside full ones, host arrays and device tensors, device views 8 bytes off a 16-byte boundary: all
    bit-identical to the one-point calls."""
    import torch
    from crimp_amd import ops
    c = wide[0][name]
    tpl = _template(c)
    n = c.x.size
    x = np.concatenate([c.x, c.x[:255], c.x[:7]])
    off = np.array([0, n, n, n + 255, n + 262], dtype=np.int64)           # interval 1 is empty
    iv = np.array([0, 0, 2, 2, 0, 3, 1, 0, 2], dtype=np.int64)
    good = np.nonzero(c.kind != 2)[0]
    pick = [int(good[i % good.size]) for i in range(9)]
    pn, pp = c.pts[pick, 0].copy(), c.pts[pick, 1].copy()
    one = np.stack([ops.toa_points(x, off, tpl, iv[i:i + 1], pn[i:i + 1], pp[i:i + 1])[0] for i in range(9)])
    assert np.all(one[iv == 1, :6] == 0) and np.all(one[iv == 1, 6] == np.inf) and np.all(one[iv == 1, 7] == 0)
    assert np.array_equal(one[:, 7], np.diff(off)[iv].astype(np.float64))
    assert np.array_equal(one[0], ops.toa_points(c.x, np.array([0, n]), tpl, iv[:1], pn[:1], pp[:1])[0])

    def shifted(a):                     # a device view that starts 8 bytes off a 16-byte boundary
        a = np.asarray(a)
        buf = torch.empty(a.size + 3, dtype=torch.float64 if a.dtype == np.float64 else torch.int64, device=gpu)
        k = 1 if buf.data_ptr() % 16 == 0 else 2
        v = buf[k:k + a.size]
        v.copy_(torch.as_tensor(a))
        assert v.data_ptr() % 16 == 8
        return v

    for npts in (1, 4, 5, 9):
        sl = slice(0, npts)
        host = ops.toa_points(x, off, tpl, iv[sl], pn[sl], pp[sl])
        np.testing.assert_array_equal(host, one[sl])
        dev = ops.toa_points(torch.as_tensor(x, device=gpu), torch.as_tensor(off, device=gpu), tpl,
                             torch.as_tensor(iv[sl].copy(), device=gpu), torch.as_tensor(pn[sl].copy(), device=gpu),
                             torch.as_tensor(pp[sl].copy(), device=gpu))
        np.testing.assert_array_equal(dev.cpu().numpy(), one[sl])
        odd = ops.toa_points(shifted(x), torch.as_tensor(off, device=gpu), tpl,
                             torch.as_tensor(iv[sl].copy(), device=gpu), shifted(pn[sl]), shifted(pp[sl]))
        np.testing.assert_array_equal(odd.cpu().numpy(), one[sl])
    # the last four points alone: the same groups cut differently
    np.testing.assert_array_equal(ops.toa_points(x, off, tpl, iv[5:], pn[5:], pp[5:]), one[5:])


def test_toa_shape_points_every_case_within_bound(gpu, wide):
    """crimp_toa_shape_points: all 4 + 3 x 16 sums of every case within the bound (amp, loc and wid of every
    component; the von Mises cases with aux and without), unused component slots and the Fourier wid slots exactly 0."""
    from scipy.special import i0e, i1e
    from crimp_amd import ops
    sums, _ = wide
    rows, bad = {}, []
    for c in sums.values():
        x, off = _padded(c)
        S = len(c.shape_pts)
        tpls = [_template(c)] * S
        pn, pp = c.pts[c.shape_pts, 0].copy(), c.pts[c.shape_pts, 1].copy()
        aux = None
        if c.model == "vonmises":
            k = 1.0 / np.array(c.tpl["wid"]) ** 2
            aux = np.zeros((S, R.MAX_COMP))
            aux[:, :k.size] = i1e(k) / i0e(k)
        got = ops.toa_shape_points(x, off, tpls, np.zeros(S, np.int64), pn, pp, aux=aux)
        K = len(c.tpl["amp"])
        unused = np.ones(R.SHAPE_SUMS, bool)
        unused[:4 + 3 * K] = False
        if c.model == "fourier":
            unused[6::3] = True
        assert np.all(got[:, unused] == 0) and np.all(c.sh_hi[:, unused] == 0) and np.all(c.sh_A[:, unused] == 0)
        r = R.err_ratio(got, c.sh_hi, c.sh_lo, c.sh_A)
        groups = {"lnm": r[:, 0], "min": r[:, 1], "q": r[:, 2], "hphi": r[:, 3], "amp": r[:, 4::3], "loc": r[:, 5::3],
                  "wid": r[:, 6::3]}
        if c.model == "vonmises":
            g0 = ops.toa_shape_points(x, off, tpls, np.zeros(S, np.int64), pn, pp, aux=None)
            rest = np.ones(R.SHAPE_SUMS, bool)
            rest[6::3] = False
            np.testing.assert_array_equal(g0[:, rest], got[:, rest])
            groups["wid_noaux"] = R.err_ratio(g0[:, 6::3], c.sh0_hi, c.sh0_lo, c.sh0_A)
        for key, v in groups.items():
            v = float(np.max(v))
            _worse(rows, c.model, key, v)
            if not v <= R.FACTOR:
                bad.append((c.name, key, v))
    _table(rows, "k_toa_shape")
    assert not bad, bad


def _fit_groups(fits):
    g = {}
    for f in fits.values():
        g.setdefault((f.model, f.K), []).append(f)
    return g


def _check_fit(f, r, i, brutemin, rows):
    tag = "%s brutemin=%s" % (f.name, brutemin)
    hinv = np.linalg.norm(np.linalg.inv(f.H), 2)
    slack = hinv * R.FACTOR * R.U * math.hypot(f.A_gn, f.A_gp)
    dphi, dn = abs(r["phShi"][i] - f.phi), abs(r["norm"][i] - f.norm)
    dll = abs((r["LLmax"][i] - f.ll_hi) - f.ll_lo)
    print("%-28s |dphi| %.2e (bound %.2e)  |dnorm| %.2e (bound %.2e)  |dLL|/(u A) %.2f"
          % (tag, dphi, slack + 1e-9, dn, slack + 1e-9 * f.norm, dll / (R.U * f.A_ll)))
    _worse(rows, f.model, "LLmax", dll / (R.U * f.A_ll))
    assert dphi <= slack + 1e-9, tag
    assert dn <= slack + 1e-9 * f.norm, tag
    assert dll <= R.FACTOR * R.U * f.A_ll, tag
    assert r["phShi_LL"][i] == f.phShi_LL and r["phShi_UL"][i] == f.phShi_UL, tag
    assert r["reducedChi2"][i] == pytest.approx(f.redchi2, rel=1e-6), tag


def test_toa_fit_every_instance(gpu, wide):
    """crimp_toa_fit for every template size -- the Fourier instances KF = 1..8, the run-time K = 9..16, Cauchy and von
    Mises up to 16 components, both product lengths (the N = 4095..8707 tails) -- against the 60-digit optimum: phShift
    and norm within |H^-1| (32 u A_g) plus the stopping rule's 1e-9, LLmax within the LL bound, the 1-sigma bounds the
    oracle's, reducedChi2 within 1e-6; with and (up to 8 components) without the brute start; all cases of one template
    in one batched call bit-identical to the single-interval calls."""
    from crimp_amd.toafit import ToAFitter
    rows = {}
    print()
    for (model, K), cases in _fit_groups(wide[1]).items():
        modes = (False, True) if K <= 8 else (False,)
        batch = cases if len(cases) > 1 else cases * 2
        xb = np.concatenate([f.x for f in batch])
        ob = np.concatenate([[0], np.cumsum([f.x.size for f in batch])]).astype(np.int64)
        Eb = np.array([f.E for f in batch])
        for bm in modes:
            rb = ToAFitter(xb, ob, Eb, cases[0].tmpl).fit(brutemin=bm)
            for i, f in enumerate(cases):
                r = ToAFitter(f.x, np.array([0, f.x.size]), np.array([f.E]), f.tmpl).fit(brutemin=bm)
                _check_fit(f, r, 0, bm, rows)
                for key in ("norm", "phShi", "LLmax", "phShi_LL", "phShi_UL", "reducedChi2", "ampShift"):
                    assert rb[key][i] == r[key][0], (f.name, bm, key)
        if model == "fourier" and K > 8:
            f = cases[0]
            with pytest.raises(Exception, match="at most 8 template components"):
                ToAFitter(f.x, np.array([0, f.x.size]), np.array([f.E]), f.tmpl).fit(brutemin=True)
    _table(rows, "k_toa_fit")


@pytest.mark.parametrize("K", range(1, 9))
def test_brute_grid_every_size_vs_oracle(gpu, wide, K):
    """ops.toa_grid (k_toa_grid_mf / k_toa_grid, one instance per template size) against the oracle's fp64 grid on a
    fit case's photons, with test_brute_grid_vs_oracle's tolerances and its argmax equality."""
    from crimp_amd import ops
    f = wide[1]["fit_f%d" % K]
    tarr = O.template_arrays(f.tmpl)
    tpl = ops.make_template("fourier", tarr[2], tarr[3])
    norms = np.linspace(f.tmpl["norm"]["value"] / 100.0, 500, 20)
    phis = np.arange(126) * 0.05 - np.pi
    N = f.x.size
    ln, hmin = ops.toa_grid(f.x, np.array([0, N]), tpl, norms[None, :], phis)
    ref = O.toa_grid(f.x, f.E, tarr, norms, phis)
    got = -norms[:, None] * f.E + N * np.log(norms[:, None] * f.E) + ln[0] - N * np.log(norms[:, None])
    got = np.where(hmin[0][None, :] + norms[:, None] > 0, got, -np.inf)
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(got))
    np.testing.assert_allclose(got[fin], ref[fin], rtol=2e-7, atol=0.05)
    assert np.unravel_index(np.argmax(got), got.shape) == np.unravel_index(np.argmax(ref), ref.shape)


@pytest.mark.parametrize("name", ["fit_v1", "fit_v3", "fit_c1"])
def test_brute_grid_narrow_peaks_find_the_oracles_start(gpu, wide, name):
    """k_toa_grid (fp32) on the narrowest templates -- von Mises wid 0.04 (kappa = 625, where a / (2 pi I0) is below
    fp32's range and has to be carried scaled) and Cauchy wid 0.02: finite where the oracle's fp64 grid is, and the
    same lattice maximum. The oracle's best point leads the runner-up by more than 1 in LL (asserted); the fp32 model
    is wrong by at most kappa log2(e) 2^-23 ~ 1e-4 relative per photon on the peak, under 0.06 over 600 photons."""
    from crimp_amd import ops
    f = wide[1][name]
    tarr = O.template_arrays(f.tmpl)
    tpl = ops.make_template(f.model, tarr[2], tarr[3], tarr[4])
    pb = R.PH_BOUND[f.model]
    phis = np.arange(int(math.ceil(2 * pb / 0.05))) * 0.05 - pb
    norms = np.linspace(f.tmpl["norm"]["value"] / 100.0, 500, 20)
    N = f.x.size
    ref = O.toa_grid(f.x, f.E, tarr, norms, phis)
    top = np.sort(ref[np.isfinite(ref)])[::-1]
    assert top[0] - top[1] > 1.0
    ln, hmin = ops.toa_grid(f.x, np.array([0, N]), tpl, norms[None, :], phis)
    Fn = TWO_PI * norms[:, None] + float(np.sum(tarr[2]))
    got = -Fn * f.E / TWO_PI + N * np.log(Fn * f.E / TWO_PI) + ln[0] - N * np.log(Fn)
    got = np.where(hmin[0][None, :] + norms[:, None] > 0, got, -np.inf)
    assert np.array_equal(np.isfinite(ref), np.isfinite(got))
    assert np.unravel_index(np.argmax(got), got.shape) == np.unravel_index(np.argmax(ref), ref.shape)
    assert abs(np.max(got) - top[0]) < 0.06 + 2e-7 * abs(top[0])
