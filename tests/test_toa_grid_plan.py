"""The host plan of crimp_toa_fit's brute grid (csrc/toa_grid_plan.h: plan_brute_grid) on the CPU.

`make -C crimp_amd/csrc plan-check` builds toa_grid_plan_check.cpp with the host compiler under
-fsanitize=address,undefined; every case below is one run of that program (no GPU, no preloaded library). What it
prints is held to the definitions restated here in numpy: lmfit's lattice, the pruning's soundness against the full
20-norm lattice of the extended log-likelihood, the compaction's shape, the mode bits and the histogram certificate."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crimp_amd", "csrc")
FOURIER, CAUCHY, VONMISES = 0, 1, 2
NO_MIN, PROD8, CERT = 1, 2, 4
NN_SMALL = 4

# the 1e2259 template of the benchmark's config 5 (bench.T2259)
T2259_NORM = 17.060771467236613
T2259_AMP = [1.508994969593123, 4.055594828231136, 1.4384785819368275, 0.3505348524380939, 0.19725727340744187,
             0.3483402644535841]
T2259_PH = [-0.4071967961461897, -0.8051383329477251, 0.5157949575544241, 1.9295783704947946, -0.1917798112304259,
            0.8297144204463391]


@pytest.fixture(scope="module")
def plan_check():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-s", "-B", "-C", CSRC, "plan-check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(CSRC, "build", "plan_check")


class Tpl:
    """TplDev's fields (make_tpl's folded form)."""

    def __init__(self, model, amp, loc, ch=None, kap=None):
        self.model, self.K = model, len(amp)
        self.amp, self.loc = np.asarray(amp, float), np.asarray(loc, float)
        self.ch = np.zeros(self.K) if ch is None else np.asarray(ch, float)
        self.kap = np.zeros(self.K) if kap is None else np.asarray(kap, float)

    def h(self, x, phi):
        """The template part (model - norm) [len(x), len(phi)]: x in cycles (Fourier) or radians."""
        x, phi = np.asarray(x, float)[:, None], np.asarray(phi, float)[None, :]
        out = np.zeros((x.shape[0], phi.shape[1]))
        for j in range(self.K):
            if self.model == FOURIER:
                out += self.amp[j] * np.cos(2 * np.pi * (j + 1) * x + self.loc[j] - (j + 1) * phi)
            elif self.model == CAUCHY:
                out += self.amp[j] / (self.ch[j] - np.cos(x - self.loc[j] - phi))
            else:
                out += self.amp[j] * np.exp(self.kap[j] * np.cos(x - self.loc[j] - phi))
        return out

    def period(self):
        return 1.0 if self.model == FOURIER else 2 * np.pi

    def bounds(self):
        """hmin <= h <= hmax from the components' own ranges."""
        if self.model == FOURIER:
            return -np.abs(self.amp).sum(), np.abs(self.amp).sum()
        if self.model == CAUCHY:
            return (self.amp / (self.ch + 1)).sum(), (self.amp / (self.ch - 1)).sum()
        return (self.amp * np.exp(-self.kap)).sum(), (self.amp * np.exp(self.kap)).sum()


def fourier(amp, ph, scale=1.0):
    return Tpl(FOURIER, np.asarray(amp) * scale, ph)


def cauchy(a, cen, wid):
    a, wid = np.asarray(a, float), np.asarray(wid, float)
    return Tpl(CAUCHY, a / (2 * np.pi) * np.sinh(wid), cen, ch=np.cosh(wid))


def vonmises(a, cen, wid):
    a, wid = np.asarray(a, float), np.asarray(wid, float)
    return Tpl(VONMISES, a / (2 * np.pi * np.i0(1 / wid ** 2)), cen, kap=1 / wid ** 2)


def draw(tpl, norm, shift, n, rng):
    """n photons from the density norm + h(x; shift) by rejection."""
    grid = np.linspace(0, tpl.period(), 4097)
    ymax = 1.05 * (norm + tpl.h(grid, [shift])[:, 0]).max()
    out = np.empty(0)
    while out.size < n:
        x = rng.uniform(0, tpl.period(), 4 * n + 64)
        keep = rng.uniform(0, ymax, x.size) < norm + tpl.h(x, [shift])[:, 0]
        out = np.concatenate([out, x[keep]])
    return out[:n]


def run_plan(exe, tpl, norm0, counts, expo, edges=None, mf=1, full=0, slow=0, nocert=0):
    lo, hi = norm0 / 100.0, 500.0
    pb = math.pi if tpl.model == FOURIER else 1.5 * math.pi
    w = ["%d %d" % (tpl.model, tpl.K)]
    for f in (tpl.amp, tpl.loc, tpl.ch, tpl.kap):
        w.append(" ".join(float(v).hex() if np.isfinite(v) else repr(float(v)) for v in f))
    w.append("%s %s %s" % (lo.hex(), hi.hex(), pb.hex()))
    w.append("%d" % len(counts))
    w += ["%d %s" % (n, float(e).hex()) for n, e in zip(counts, expo)]
    w.append("0" if edges is None else "%d %s" % (len(edges) - 1, " ".join(float(e).hex() for e in edges)))
    w.append("%d %d %d %d" % (mf, full, slow, nocert))
    r = subprocess.run([exe], input="\n".join(w) + "\n", capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    p = {"nrm": [], "mask": []}
    for ln in r.stdout.splitlines():
        key, *v = ln.split()
        if key in ("phi", "grid_n", "hb", "gsc"):
            p[key] = np.array([float.fromhex(t) for t in v])
        elif key == "nrm":
            p["nrm"].append([float.fromhex(t) for t in v])
        elif key == "mask":
            p["mask"].append([int(t, 16) for t in v])
        elif key == "row":
            p["row"] = np.array([int(t) for t in v], dtype=int)
        else:
            p[key] = int(v[0])
    p["nrm"] = np.array(p["nrm"])
    p["hb"], p["gsc"] = float(p["hb"][0]), float(p["gsc"][0])
    p.update(lo=lo, hi=hi, pb=pb)
    return p


def check_lattice(p, tpl):
    nphi = 126 if tpl.model == FOURIER else 189
    assert len(p["phi"]) == nphi == math.ceil(2 * p["pb"] / 0.05)
    np.testing.assert_array_equal(p["phi"], np.arange(nphi) * 0.05 + (-p["pb"]))
    np.testing.assert_array_equal(p["grid_n"], np.arange(20) * ((p["hi"] - p["lo"]) / 19.0) + p["lo"])


def candidate_ranges(p):
    """Shape of the compaction; returns every interval's (first lattice index, count)."""
    nc, g = p["nc"], p["grid_n"]
    assert nc in (2, NN_SMALL, 20) and p["nrm"].shape[1] == nc
    out = []
    for row in p["nrm"]:
        idx = [int(np.flatnonzero(g == v)[0]) for v in row]   # lattice values, bit for bit
        cnt = len(set(idx))
        assert idx[:cnt] == list(range(idx[0], idx[0] + cnt))  # contiguous, in grid order
        assert idx[cnt:] == [idx[cnt - 1]] * (nc - cnt)        # padding repeats the last
        out.append((idx[0], cnt))
    widest = max(c for _, c in out)
    assert nc == (2 if widest <= 2 else NN_SMALL if widest <= NN_SMALL else 20)
    return out


def check_pruning(p, tpl, photons, expo):
    """lmfit's brute argmax over the full lattice (norm outer, first maximum) lies among the interval's candidates."""
    for (a0, cnt), x, E in zip(candidate_ranges(p), photons, expo):
        h = tpl.h(x, p["phi"])
        ll = np.full((20, len(p["phi"])), -np.inf)
        for a, n in enumerate(p["grid_n"]):
            v = n + h
            ok = (v > 0).all(axis=0)
            ll[a, ok] = -n * E + np.log(v[:, ok]).sum(axis=0)
        assert np.isfinite(ll).any()
        best = int(np.argmax(ll.ravel())) // len(p["phi"])
        assert a0 <= best < a0 + cnt, (best, a0, cnt)


def expected_mode(p, tpl, counts, expo, mf=1, slow=0):
    """The two host-certified bits from their definitions, with the plan's own hb and scale."""
    if not (tpl.model == FOURIER and tpl.K <= 8 and mf and not slow and np.isfinite(p["hb"])):
        return 0
    hb, gsc, hhi = p["hb"], p["gsc"], tpl.bounds()[1]
    cand = p["nrm"].ravel()
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.asarray(counts, float) / np.asarray(expo, float)
        nomin = bool((cand + hb > 0).all() and (hb + r > 0.5 * r).all())
    valid = cand + hb > 0
    prod8 = bool(((cand + hhi) * gsc <= 2.0 ** 15).all() and ((cand[valid] + hb) * gsc >= 2.0 ** -15).all())
    return (NO_MIN if nomin else 0) | (PROD8 if prod8 else 0)


def check_mode(p, tpl, counts, expo, **kw):
    assert p["mode"] & 3 == expected_mode(p, tpl, counts, expo, **kw)
    if tpl.model == FOURIER and np.isfinite(p["hb"]):
        u = np.linspace(0, 1, 1 << 18, endpoint=False)
        hmin = tpl.h(u, [0.0]).min()
        lip = 2 * np.pi * (np.arange(1, tpl.K + 1) * np.abs(tpl.amp)).sum()
        assert p["hb"] <= hmin and hmin - p["hb"] <= 2 * lip / 65536 + 1e-9  # a lower bound of h, and a tight one
        m = np.abs(tpl.amp).max() * p["gsc"]
        assert math.log2(p["gsc"]).is_integer() and 1.0 <= m <= 4096.0
        assert p["gsc"] == 1.0 or not 1.0 <= np.abs(tpl.amp).max() <= 4096.0
    lazy = [int(np.argmax(np.append(row + p["hb"] > 0, True))) for row in p["nrm"]]
    if p["mode"] & 3 == PROD8:
        assert p["nlazy"] == (min(lazy) if min(lazy) < p["nc"] else 0)
    else:
        assert p["nlazy"] == 0
    if not p["mode"] & CERT:
        assert p["mask"] == [] and p["row"].size == 0
    return lazy


def check_certificate(p, tpl, edges):
    """Every set bit (lazy norm v, phi_k, bin b): the fp64 template part is <= -v - 1e-3 on every point of a 2^16-point
    phase grid that lies in bin b (its edges included), so no photon the bin can hold makes the point valid."""
    assert p["mode"] == PROD8 | CERT and len(edges) - 1 <= 64
    nint, nl, nphi = p["nrm"].shape[0], p["nlazy"], len(p["phi"])
    assert nl > 0 and p["row"].size == nint * nl
    vals = {}
    for i in range(nint):
        for z in range(nl):
            r = int(p["row"][i * nl + z])
            assert 0 <= r < len(p["mask"]) and vals.setdefault(r, p["nrm"][i, z]) == p["nrm"][i, z]
    assert sorted(vals) == list(range(len(p["mask"])))
    # h(x_g; phi_k) = sum_j amp_j cos(A_jg - B_jk) on x_g = g / 2^16, by angle addition: two small matrix products
    G = 1 << 16
    j = np.arange(1, tpl.K + 1)[:, None]
    A = 2 * np.pi * j * (np.arange(G + 1) / G)[None, :] + tpl.loc[:, None]
    B = j * p["phi"][None, :]
    H = (tpl.amp[:, None] * np.cos(B)).T @ np.cos(A) + (tpl.amp[:, None] * np.sin(B)).T @ np.sin(A)  # [nphi, G + 1]
    binmax = np.empty((nphi, len(edges) - 1))
    for b in range(len(edges) - 1):
        g0, g1 = math.floor(edges[b] * G), math.ceil(edges[b + 1] * G)
        binmax[:, b] = H[:, np.arange(g0, g1 + 1) % G].max(axis=1)
    for r, v in vals.items():
        m = np.array(p["mask"][r], dtype=np.uint64)
        assert (m != 0).all() and (m >> np.uint64(len(edges) - 1) == 0).all()
        bits = (m[:, None] >> np.arange(len(edges) - 1, dtype=np.uint64)[None, :]) & np.uint64(1)
        assert (binmax[bits == 1] <= -v - 1e-3).all()


def make_case(tpl, rates, counts, seed):
    """Intervals of counts[i] photons drawn from the template at random shifts with the mean rate rates[i] (the norm
    is the rate less the mean of h over a turn), exposure counts / rates."""
    rng = np.random.default_rng(seed)
    u = np.linspace(0, tpl.period(), 8192, endpoint=False)
    mean_h = 0.0 if tpl.model == FOURIER else tpl.h(u, [0.0]).mean()
    assert min(rates) - mean_h + tpl.h(u, [0.0]).min() >= -1e-12  # a density
    photons = [draw(tpl, r - mean_h, rng.uniform(-np.pi, np.pi), n, rng) for n, r in zip(counts, rates)]
    return photons, [n / r for n, r in zip(counts, rates)]


def full_checks(exe, tpl, norm0, rates, counts, seed, edges=None, **kw):
    photons, expo = make_case(tpl, rates, counts, seed)
    p = run_plan(exe, tpl, norm0, counts, expo, edges=edges, **kw)
    check_lattice(p, tpl)
    check_pruning(p, tpl, photons, expo)
    check_mode(p, tpl, counts, expo, mf=kw.get("mf", 1), slow=kw.get("slow", 0))
    return p, expo


T2259 = fourier(T2259_AMP, T2259_PH)
EDGES16 = np.linspace(0.0, 1.0, 17)


def test_pruning_fourier_rate_on_a_lattice_norm(plan_check):
    """Config-5-style intervals; one whose rate N/E sits on the lattice norm grid_n[1] to within 1e-12 (its candidates
    are the norm and both neighbours) and one far up the lattice."""
    g1 = 1 * ((500.0 - T2259_NORM / 100.0) / 19.0) + T2259_NORM / 100.0
    rates = [T2259_NORM, g1, T2259_NORM * 1.3, 240.0]
    assert abs(1100 / (1100 / g1) - g1) <= 1e-12
    p, _ = full_checks(plan_check, T2259, T2259_NORM, rates, [40, 1100, 3000, 300], seed=1)
    ranges = candidate_ranges(p)
    assert p["nc"] == NN_SMALL and ranges[0] == (0, 2) and ranges[1] == (0, 3)


def test_pruning_fourier_two_harmonics(plan_check):
    tpl = fourier([2.5, 0.8], [0.3, -1.1])
    p, _ = full_checks(plan_check, tpl, 12.0, [12.0, 30.0, 5.0], [40, 700, 2500], seed=2)
    assert p["nc"] == 2


def test_pruning_cauchy_and_every_norm_a_candidate(plan_check):
    """A broad Cauchy template prunes to a few norms; a narrow bright one has hmax - hmin > 500, so an interval's rate
    minus the bounds covers the whole lattice: all 20 norms are candidates."""
    tpl = cauchy([60.0, 25.0], [1.0, 4.0], [0.6, 0.9])
    p, _ = full_checks(plan_check, tpl, 20.0, [34.0, 50.0, 20.0], [40, 900, 3000], seed=3)
    assert p["nc"] in (2, NN_SMALL) and p["mode"] == 0
    narrow = cauchy([100.0], [2.0], [0.05])
    assert narrow.bounds()[1] - narrow.bounds()[0] > 500.0
    p, _ = full_checks(plan_check, narrow, 20.0, [480.0, 30.0, 100.0], [3000, 40, 500], seed=4)
    assert p["nc"] == 20 and p["mode"] == 0
    np.testing.assert_array_equal(p["nrm"], np.tile(p["grid_n"], (3, 1)))


def test_pruning_vonmises(plan_check):
    tpl = vonmises([40.0, 15.0], [0.5, 3.5], [0.7, 1.2])
    p, _ = full_checks(plan_check, tpl, 15.0, [24.0, 60.0, 15.0, 140.0], [40, 1100, 3000, 200], seed=5)
    assert p["nc"] in (2, NN_SMALL) and p["mode"] == 0


def test_full_grid_hook_gives_all_twenty(plan_check):
    counts, expo = [40, 1100, 3000], [40 / T2259_NORM, 1100 / 20.0, 3000 / 15.0]
    p = run_plan(plan_check, T2259, T2259_NORM, counts, expo, full=1)
    assert p["nc"] == 20
    np.testing.assert_array_equal(p["nrm"], np.tile(p["grid_n"], (3, 1)))
    candidate_ranges(p)
    check_mode(p, T2259, counts, expo)


def test_modes_of_the_2259_template(plan_check):
    """The 1e2259 shape reaches every host-certified mode: 3 at a rate whose candidates lie above -hb; 1 with the
    amplitudes 1000 times fainter (the coefficient scale 2^8 takes a factor past 2^15); 0 with, besides, a faint
    interval whose lowest norm is below -hb; 2 at config 5's own rate (the lowest lattice norm, norm0 / 100, is a
    candidate and invalid everywhere) and 6 with the phase histogram at hand; CRIMP_TOA_NO_CERT turns 6 into 2."""
    counts = [40, 1100, 3000]
    p, _ = full_checks(plan_check, T2259, T2259_NORM, [100.0, 110.0, 95.0], counts, seed=6)
    assert p["mode"] == NO_MIN | PROD8 and p["nlazy"] == 0
    faint = fourier(T2259_AMP, T2259_PH, 1e-3)
    p, _ = full_checks(plan_check, faint, T2259_NORM, [200.0, 210.0, 190.0], counts, seed=7)
    assert p["mode"] == NO_MIN and p["gsc"] == 256.0
    p, _ = full_checks(plan_check, faint, 0.05, [0.01, 200.0, 190.0], counts, seed=8)
    assert p["mode"] == 0
    rates = [T2259_NORM, T2259_NORM * 1.02, T2259_NORM * 0.97]
    p, _ = full_checks(plan_check, T2259, T2259_NORM, rates, counts, seed=9)
    assert p["mode"] == PROD8 and p["nlazy"] == 1 and p["nc"] == 2
    p, expo = full_checks(plan_check, T2259, T2259_NORM, rates, counts, seed=9, edges=EDGES16)
    assert p["mode"] == PROD8 | CERT and p["nlazy"] == 1
    check_certificate(p, T2259, EDGES16)
    assert len(p["mask"]) == 1 and (p["row"] == 0).all()
    p = run_plan(plan_check, T2259, T2259_NORM, counts, expo, edges=EDGES16, nocert=1)
    assert p["mode"] == PROD8 and p["mask"] == []


def test_mode_zero_where_the_fast_kernel_does_not_apply(plan_check):
    """Cauchy and von Mises (above), more than 8 components, CRIMP_TOA_GRID_SLOW, a build without the matrix-core
    kernel, a non-finite hb: mode 0, no lazy norms, no certificate, with the histogram at hand."""
    counts, rates = [40, 1100, 3000], [T2259_NORM, T2259_NORM * 1.02, T2259_NORM * 0.97]
    expo = [n / r for n, r in zip(counts, rates)]
    nine = fourier(T2259_AMP + [0.1, 0.05, 0.02], T2259_PH + [0.1, 0.2, 0.3])
    bad = fourier(T2259_AMP, [np.inf] + T2259_PH[1:])
    for tpl, kw in ((nine, {}), (T2259, {"slow": 1}), (T2259, {"mf": 0}), (bad, {})):
        p = run_plan(plan_check, tpl, T2259_NORM, counts, expo, edges=EDGES16, **kw)
        assert p["mode"] == 0 and p["nlazy"] == 0 and p["mask"] == [] and p["row"].size == 0
        candidate_ranges(p)
    assert not np.isfinite(run_plan(plan_check, bad, T2259_NORM, counts, expo)["hb"])


def test_nonuniform_lazy_counts_disable_the_certificate(plan_check):
    """One bright harmonic (hb ~ -30): an interval at rate 30 has the two lowest lattice norms lazy, one at rate 60
    only its first candidate. They get no certificate (an interval with more lazy norms than the common count would
    have evaluated norms that k_toa_grid_best, without the min, could not judge). Nor do a config-5 interval (its
    lowest norm lazy) and a brighter one (none lazy) together, though the first alone does
    (test_modes_of_the_2259_template). Intervals with the same two lazy norms each get it, for both norms (a template
    with a flat trough at -27 under a peak of 43: all 20 norms are candidates at a rate that passes the start rule)."""
    counts = [40, 1100, 2500]
    edges = np.linspace(0.0, 1.0, 65)
    tpl = fourier([30.0], [0.7])
    p, expo = full_checks(plan_check, tpl, 30.0, [30.0, 60.0, 31.0], counts, seed=10, edges=edges)
    assert check_mode(p, tpl, counts, expo) == [2, 1, 2] and p["nlazy"] == 1 and p["nc"] == NN_SMALL
    assert p["mode"] == PROD8 and p["mask"] == []
    p, expo = full_checks(plan_check, T2259, T2259_NORM, [T2259_NORM, 40.0, T2259_NORM], counts, seed=11, edges=EDGES16)
    assert check_mode(p, T2259, counts, expo) == [1, 0, 1] and p["nlazy"] == 0
    assert p["mode"] == PROD8 and p["mask"] == []
    tpl = fourier([35.0, 8.0], [0.7, 1.4])
    p, expo = full_checks(plan_check, tpl, 30.0, [58.0, 60.0, 62.0], counts, seed=12, edges=edges)
    assert check_mode(p, tpl, counts, expo) == [2, 2, 2] and p["nlazy"] == 2 and p["nc"] == 20
    assert p["mode"] == PROD8 | CERT and len(p["mask"]) == 2
    check_certificate(p, tpl, edges)
