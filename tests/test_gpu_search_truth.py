"""Every Z^2/H search path against the exact-argument truth of tests/search_reference.py, each within its own unit:
|got - truth| <= unit per checked trial. The units are derived in search_reference's docstring
from the documented arithmetic of each path; tests/test_search_reference.py holds the truth to 60-digit sums, the units'
soundness on NumPy models and the input conditions of the cases below (``CASES``, ``set_photons``), which it imports.

A case checks every trial where photons x trials x harmonics <= ``ALL_BELOW``, otherwise the stated subset
(``search_reference.checked_trials``: row edges, the centre and its neighbours, the named tile / block edges and at least 64 random
trials, in every row). Each test prints ``TRUTH <path> <case> m=.. stat=.. max|d|/unit`` and asserts the path the library
took (crimp_last_search_path) and, for the NUFFT, the plan's FFT length. The hooks (CRIMP_FIXUP_REL, CRIMP_NUFFT_*,
CRIMP_SEARCH_BUDGET_MB) are read at the start of every search, so all cases share one process.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import search_reference as R

# F0 has a full significand (f dt, and the NUFFT's centre frequency times dt, round: with 7.125 those products were
# exact and a dropped low word invisible); F0 + j 2^-k is still exact in fp64, so the grids are exact progressions
F0, STEP = 7.123456789, 2.0 ** -21
ALL_BELOW = 5.2e6
NAMES = {0: "z2", 1: "h"}


class Case:
    """Photons (pulsed_events: uniform noise plus a pulsed fraction at F0, time-sorted unless ``perm``) and a grid:
    ``nf`` trials per row centred on F0 with step ``step`` (a power of two: 'dyadic', an exact progression), or
    grid='nu' (sorted random frequencies, no progression) / 'linspace' (np.linspace, a progression to a few ulp);
    ``fd``: the 2-D rows (log10 |fdot|)."""

    def __init__(self, name, n, nf, step=STEP, span=2.0e4, seed=1, frac=0.3, fd=None, grid="dyadic", perm=False,
                 edges=()):
        self.name, self.n, self.nf, self.step, self.span, self.seed, self.frac = name, n, nf, step, span, seed, frac
        self.fd = None if fd is None else np.array(fd, dtype=np.float64)
        self.grid, self.perm, self.edges = grid, perm, tuple(edges)
        self.rows = 1 if fd is None else len(fd)

    @functools.cached_property
    def t(self):
        from crimp_amd.synth import pulsed_events
        t = pulsed_events(self.n, self.span, F0, pulsed_frac=self.frac, seed=self.seed)
        return np.random.default_rng(self.seed).permutation(t) if self.perm else t

    @property
    def t0(self):
        return (self.t[0] + self.t[-1]) / 2  # periodsearch.py:54

    @functools.cached_property
    def f(self):
        j = np.arange(self.nf) - self.nf // 2
        if self.grid == "dyadic":
            return F0 + j * self.step
        if self.grid == "linspace":
            return np.linspace(F0 - 0.013, F0 + 0.017, self.nf)
        return np.sort(F0 + np.random.default_rng(self.seed + 100).uniform(-1e-3, 1e-3, self.nf))

    @functools.cached_property
    def c2(self):
        return None if self.fd is None else R.c2_of(self.fd)

    def idx(self, m):
        """The checked flat trials: all of them within the truth budget, else the stated subset."""
        if self.n * self.nf * self.rows * m <= ALL_BELOW:
            return np.arange(self.nf * self.rows)
        nrandom = max(64, int(ALL_BELOW / (self.n * self.rows * m)) - 16)  # as many as the truth budget holds
        return R.checked_trials(self.nf, self.edges, nrandom, self.seed, self.rows)

    @functools.lru_cache(maxsize=None)
    def _truth(self, mmax):
        idx = self.idx(mmax)
        c2 = None if self.c2 is None else self.c2[idx // self.nf]
        return idx, R.Truth(self.t - self.t0, self.f[idx % self.nf], c2, mmax)

    def truth(self, m, mmax=None):
        """(idx, Truth of m harmonics); the sums of the case's largest m are computed once and shared."""
        idx, T = self._truth(mmax or m)
        return idx, (T if T.m == m else T.head(m))


# fp64 direct ------------------------------------------------------------------------------------------------
A_GROUPS = Case("fp64-257", 1000, 257, seed=11)
A_COUNTS = {nf: Case("fp64-n33-%d" % nf, 33, nf, seed=12) for nf in (1, 255, 256, 257)}
A_PHOTONS = {n: Case("fp64-n%d-65" % n, n, 65, seed=13) for n in (1, 2, 31, 33, 1000)}
A_2D = Case("fp64-2d-3x65", 1000, 65, seed=14, fd=[-9.5, -9.0, -8.7])
A_NU = Case("fp64-freq_nu-300", 1000, 300, seed=15, grid="nu")
A_PERM = Case("fp64-perm-257", 1000, 257, seed=16, perm=True)
A_PERM100 = Case("fp64-perm-100", 1000, 100, seed=16, perm=True)
A_BLOCKS = Case("fp64-blocks-16500", 33000, 16500, seed=17, edges=(8448,))
# fp64 fix-up ------------------------------------------------------------------------------------------------
B_EXACT = Case("few-exact-300", 1000, 300, seed=21)
B_EXACT_2D = Case("few-exact-2x256", 1000, 256, seed=22, fd=[-9.5, -8.7])
B_NUFFT = Case("few-nufft-100", 1000, 100, seed=23, step=2.0 ** -16)
B_NUFFT_2D = Case("few-nufft-3x64", 1000, 64, seed=24, step=2.0 ** -16, fd=[-9.5, -9.0, -8.7])
B_SPLITS = Case("few-exact-splits-256", 8200, 256, seed=25, edges=(128,))
# exact kernel: (trials, photons, m); kExTileTrials = 2048, kExChunk = 32, int32 carries every 16384 photons --------
D_CASES = {
    "256-n31": (Case("exact-256-n31", 31, 256, seed=31), 1),
    "2047-n32": (Case("exact-2047-n32", 32, 2047, seed=32, edges=(1024,)), 2),
    "2048-n33": (Case("exact-2048-n33", 33, 2048, seed=33, edges=(1024,)), 20),
    "2049-n16383": (Case("exact-2049-n16383", 16383, 2049, seed=34, edges=(1024, 2048)), 1),
    "2049-n16417": (Case("exact-2049-n16417", 16417, 2049, seed=35, edges=(1024, 2048)), 2),
    "2048-n16417": (Case("exact-2048-n16417", 16417, 2048, seed=36, edges=(1024,)), 1),
    "2048-n1000": (Case("exact-2048-n1000", 1000, 2048, seed=38, edges=(1024,)), 1),
    "2d-2x300": (Case("exact-2d-2x300", 1000, 300, seed=37, fd=[-9.5, -8.7]), 2),
}
# NUFFT: one case per FFT family (expected FFT length asserted), wraps, a linspace grid, H_20 on noise ----------------
E_CASES = {
    "64": (Case("nufft-64", 300, 64, seed=41, step=2.0 ** -16), 64),
    "700": (Case("nufft-700", 300, 700, seed=42, step=2.0 ** -18), 1024),
    "1401": (Case("nufft-1401", 300, 1401, seed=43, step=2.0 ** -19, edges=(1024,)), 2048),
    "3000": (Case("nufft-3000", 300, 3000, seed=44, step=2.0 ** -20, edges=(1024, 2048)), 4096),
    "6000": (Case("nufft-6000", 300, 6000, seed=45, step=2.0 ** -21, edges=(2048, 4096)), 8192),
    "600000": (Case("nufft-600000", 300, 600000, seed=46, step=2.0 ** -27, edges=(4096, 262144, 524288)), 1 << 20),
    "1200000": (Case("nufft-1200000", 300, 1200000, seed=47, step=2.0 ** -28, edges=(4096, 524288, 1048576)), 1 << 21),
}
E_WRAPS = {  # (m + 1) step span + 1 cells of the widest planned harmonic per FFT length: ~1, ~4, 31 of at most 32
    "none": Case("nufft-wrap0.1", 1000, 128, seed=51, step=2.0 ** -18),
    "3": Case("nufft-wrap3", 1000, 128, seed=52, step=2.0 ** -13),
    "31": Case("nufft-wrap31", 1000, 128, seed=53, step=2.0 ** -11, span=20500.0),
}
E_FEW = {n: Case("nufft-n%d-700" % n, n, 700, seed=58, step=2.0 ** -18) for n in (3, 33)}
E_LINSPACE = Case("nufft-linspace-700", 1000, 700, seed=54, grid="linspace")
E_NOISE = Case("nufft-h20-noise-240", 1000, 240, seed=55, step=2.0 ** -14, frac=0.0)
E_GATHER = Case("nufft-gather-200", 1000, 200, seed=56, step=2.0 ** -14)
E_MFMA = Case("nufft-mfma-3x64", 1000, 64, seed=57, step=2.0 ** -14, fd=[-9.5, -9.0, -8.7])

SET_SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1000)
SET_HARMONICS = (1, 5, 8, 9, 20)
# every case with the largest harmonic count its tests use: the CPU checks of tests/test_search_reference.py run on these
CASES = ([(A_GROUPS, 20), (A_2D, 7), (A_NU, 5), (A_PERM, 7), (A_PERM100, 7), (A_BLOCKS, 2), (B_EXACT, 15),
          (B_EXACT_2D, 2), (B_NUFFT, 20), (B_NUFFT_2D, 15), (B_SPLITS, 2), (E_LINSPACE, 2), (E_NOISE, 20),
          (E_GATHER, 9), (E_MFMA, 20)]
         + [(c, 15) for c in A_COUNTS.values()] + [(c, 7) for c in A_PHOTONS.values()]
         + [(c, m) for c, m in D_CASES.values()] + [(c, 2) for c, _ in E_CASES.values()]
         + [(c, 2) for c in E_WRAPS.values()] + [(c, 2) for c in E_FEW.values()])
ARGMAX_CASES = [(A_GROUPS, 20), (B_NUFFT, 20), (E_WRAPS["3"], 2), (E_WRAPS["31"], 2), (E_CASES["64"][0], 2),
                (E_CASES["700"][0], 2), (E_GATHER, 9)]


def set_photons(days=False):
    """(t, offsets, freq) of the crimp_search_sets cases: consecutive runs of one photon stream at ~5e9 s (or the same
    as MJD days), one trial frequency per set."""
    from crimp_amd.synth import pulsed_events
    off = np.concatenate([[0], np.cumsum(SET_SIZES)]).astype(np.int64)
    t = pulsed_events(int(off[-1]), 4.0e4, F0, pulsed_frac=0.3, seed=61)
    if days:
        t = 58000.0 + (t - 5.0e9) / 86400.0
    return t, off, F0 + (np.arange(len(SET_SIZES)) - 4) * 2.0 ** -17


@functools.lru_cache(maxsize=None)
def set_truth(days):
    t, off, f = set_photons(days)
    return R.truth_of_sets(t, off, f, max(SET_HARMONICS), days)


# ------------------------------------------------------------------------------------------------- running
@contextlib.contextmanager
def hooks(**env):
    """The library's environment hooks for the searches inside (restored afterwards)."""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def search(case, m, stat, precision, flags=0):
    """(powers [rows * nf], path, fix-ups, (FFT length, moments, spread form)) of one ops.search on host arrays."""
    from crimp_amd import ops, _native as N
    out = ops.search(case.t, case.t0, case.f, m, stat, log10_negfdot=case.fd, flags=flags, precision=precision)
    L = N.load()
    return out, int(L.crimp_last_search_path()), int(L.crimp_last_fixups()), N.last_nufft_plan()


def report(path, case, m, stat, got, want, unit):
    """Print and return max |got - truth| / unit; assert it is at most 1 at every checked trial."""
    assert np.isfinite(got).all()
    ratio = np.abs(got - want) / unit
    worst = int(np.argmax(ratio))
    print("TRUTH %-12s %-22s m=%-2d stat=%-2s checked=%-5d max|d|/unit=%.3e" % (path, case, m, NAMES[stat], got.size,
                                                                               ratio[worst]))
    assert ratio[worst] <= 1.0, (path, case, m, stat, worst, float(got[worst]), float(want[worst]), float(unit[worst]))
    return float(ratio[worst])


def check_fp64(case, m, stat, precision, mmax=None):
    out, path, _, _ = search(case, m, stat, precision)
    assert path == 0
    idx, T = case.truth(m, mmax)
    return report("fp64", case.name, m, stat, out[idx], T.power(stat), R.fp64_unit(T, stat))


def nufft_units(case, T, idx, stat, plan):
    j = idx % case.nf
    dev = R.nufft_grid_deviation(case.f, j)
    return R.nufft_raw_unit(T, stat, j - case.nf // 2, plan[0], plan[1], dev), dev


pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------- a. fp64 direct
@pytest.mark.parametrize("stat", [0, 1])
@pytest.mark.parametrize("m", [1, 2, 3, 7, 15, 20])
def test_fp64_direct_harmonic_groups(gpu, m, stat):
    """k_search_f64 at every group shape: m = 15 runs G = 8, 4, 2, 1 at k0 = 1, 9, 13, 15; m = 1 and m = 3 reach the
    G = 1 instance with k0 = 1 and k0 = 3; 257 trials are two blocks of kSearchBlock."""
    check_fp64(A_GROUPS, m, stat, "f64", 20)


@pytest.mark.parametrize("nf", [1, 255, 256, 257])
def test_fp64_direct_trial_counts(gpu, nf):
    for stat in (0, 1):
        check_fp64(A_COUNTS[nf], 15, stat, "f64")


@pytest.mark.parametrize("n", [1, 2, 31, 33, 1000])
def test_fp64_direct_photon_counts(gpu, n):
    for stat in (0, 1):
        check_fp64(A_PHOTONS[n], 7, stat, "f64")


@pytest.mark.parametrize("stat", [0, 1])
def test_fp64_direct_2d(gpu, stat):
    for m in (3, 7):
        check_fp64(A_2D, m, stat, "f64", 7)


def test_fp64_default_on_a_non_progression(gpu):
    """The default precision on a grid that is no progression routes to k_search_f64."""
    check_fp64(A_NU, 2, 0, None, 5)
    check_fp64(A_NU, 5, 1, None, 5)


def test_fp64_unsorted_photons(gpu):
    """A permuted photon array: precision='f64', and the default on 100 trials (the NUFFT declines unsorted photons, the
    exact rule sends fewer than 256 trials to k_search_f64)."""
    check_fp64(A_PERM, 7, 1, "f64")
    check_fp64(A_PERM100, 7, 0, None)


def plan_direct(n, nharm, count, budget):
    """search_plan.h's plan_direct restated: (chunk, splits, trials per block)."""
    def cdiv(a, b):
        return -(-a // b)
    chunk = cdiv(cdiv(n, max(1, min(64, n // 16384))), 32) * 32
    splits = cdiv(n, chunk)
    cbmax = max(256, budget // (8 * splits * 2 * nharm))
    return chunk, splits, min(count, cdiv(cdiv(count, cdiv(count, cbmax)), 256) * 256)


def test_fp64_direct_photon_splits_and_trial_blocks(gpu):
    """33000 photons x 16500 trials of Z^2_2 under CRIMP_SEARCH_BUDGET_MB=1: two photon splits and two trial blocks
    (8448 + 8052), held to the same unit; the block edge is among the checked trials."""
    c = A_BLOCKS
    assert plan_direct(c.n, 2, c.nf, 1 << 20) == (16512, 2, 8448)
    with hooks(CRIMP_SEARCH_BUDGET_MB=1):
        check_fp64(c, 2, 0, "f64")


# ------------------------------------------------------------------------------------------------- b. fp64 fix-up
@pytest.mark.parametrize("case,m,stat,precision,path", [
    (B_EXACT, 15, 1, "exact", 1), (B_EXACT, 2, 0, "exact", 1), (B_EXACT_2D, 2, 0, "exact", 1),
    (B_NUFFT, 20, 1, None, 2), (B_NUFFT, 2, 0, None, 2), (B_NUFFT_2D, 15, 0, None, 2), (B_NUFFT_2D, 2, 1, None, 2),
    (B_SPLITS, 2, 0, "exact", 1)], ids=lambda v: getattr(v, "name", None))
def test_fp64_fixup_of_every_trial(gpu, case, m, stat, precision, path):
    """CRIMP_FIXUP_REL=1e-30 flags every trial of the exact kernel and of the NUFFT, so every power is
    k_search_f64_few's (B_SPLITS: two photon splits of 4100): each within the fp64 unit."""
    with hooks(CRIMP_FIXUP_REL="1e-30"):
        out, took, fixed, _ = search(case, m, stat, precision)
    assert took == path and fixed == case.nf * case.rows
    idx, T = case.truth(m, {B_EXACT: 15, B_NUFFT: 20, B_NUFFT_2D: 15}.get(case))
    report("fp64-few", case.name, m, stat, out[idx], T.power(stat), R.fp64_unit(T, stat))


# ------------------------------------------------------------------------------------------------- c. k_search_sets
@pytest.mark.parametrize("days", [False, True], ids=["seconds", "mjd-days"])
def test_search_sets(gpu, days):
    """Sets of 1 .. 1000 photons in one call, m in {1, 5, 8, 9, 20} (m = 9: a last group of one harmonic at k0 = 9),
    both statistics, in seconds at ~5e9 and as MJD days with CRIMP_FLAG_TIME_DAYS (truth from fl(t * 86400))."""
    from crimp_amd import ops, _native as N
    t, off, f = set_photons(days)
    truths = set_truth(days)
    for m in SET_HARMONICS:
        for stat in (0, 1):
            got = ops.search_sets(t, off, f, m, stat, flags=N.FLAG_TIME_DAYS if days else 0)
            Ts = [T.head(m) for T in truths]
            want = np.array([T.power(stat)[0] for T in Ts])
            unit = np.array([R.fp64_unit(T, stat, sets=True)[0] for T in Ts])
            report("fp64-sets", "sets-days" if days else "sets-seconds", m, stat, got, want, unit)


# ------------------------------------------------------------------------------------------------- d. exact kernel
@pytest.mark.parametrize("key", list(D_CASES))
def test_exact_kernel_raw_and_default(gpu, key):
    """precision='exact' with CRIMP_FLAG_NO_FIXUP inside the certificate's bound on the truth sums (plus the argument
    and grid terms it does not know), and with the fix-up inside the default unit with at most 64 fix-ups. Z^2_1 cases of
    >= 1000 trials: the residuals normalised by the model's 1 sigma have rms <= 1."""
    from crimp_amd import _native as N
    case, m = D_CASES[key]
    for stat in ((0, 1) if m > 1 else (0,)):
        idx, T = case.truth(m)
        want = T.power(stat)
        raw, path, _, _ = search(case, m, stat, "exact", N.FLAG_NO_FIXUP)
        assert path == 1
        dev = R.exact_grid_deviation(case.f, idx % case.nf)
        assert not dev.any()  # a dyadic grid: the kernel evaluates f[j] itself
        unit, sigma = R.exact_raw_unit(T, stat, dev)
        report("exact-raw", case.name, m, stat, raw[idx], want, unit)
        if stat == 0 and m == 1 and case.nf >= 1000:
            rms = float(np.sqrt(np.mean(((raw[idx] - want) / sigma) ** 2)))
            print("TRUTH exact-raw    %-22s rms(dP/sigma_P)=%.3f over %d trials" % (case.name, rms, idx.size))
            assert rms <= 1.0
        out, path, fixed, _ = search(case, m, stat, "exact")
        assert path == 1 and fixed <= 64
        report("exact", case.name, m, stat, out[idx], want, R.default_unit(T, stat))


# ------------------------------------------------------------------------------------------------- e. NUFFT
def check_nufft(case, m, stat, nfft=None, max_nfft=None, mmax=None, spread=None, argmax=False):
    """Raw (precision='nufft', NO_FIXUP) within the NUFFT unit and the default within the default unit; returns the
    plan. ``argmax``: the default path's best trial is the truth's (cases that check every trial)."""
    from crimp_amd import _native as N
    idx, T = case.truth(m, mmax)
    want = T.power(stat)
    raw, path, _, plan = search(case, m, stat, "nufft", N.FLAG_NO_FIXUP)
    assert path == 2
    assert nfft is None or plan[0] == nfft, plan
    assert max_nfft is None or plan[0] <= max_nfft, plan
    assert spread is None or plan[2] == spread, plan
    # the plan is section 5.3's: a plan one moment short of the rule would widen the unit it is judged by
    assert plan[:2] == R.nufft_plan_rule(case.nf, stat, m, plan[2] == "gather"), plan
    unit, dev = nufft_units(case, T, idx, stat, plan)
    if case.grid == "dyadic":
        assert not dev.any()
    report("nufft-raw", case.name, m, stat, raw[idx], want, unit)
    for precision in (None, "nufft"):
        out, path, _, _ = search(case, m, stat, precision)
        assert path == 2
        report("nufft", case.name, m, stat, out[idx], want, R.default_unit(T, stat))
        if argmax:
            assert idx.size == out.size and int(np.argmax(out)) == int(np.argmax(want))
    return plan


@pytest.mark.parametrize("key", list(E_CASES))
def test_nufft_fft_families(gpu, key):
    """One plan per FFT family: n <= 2^10 (the generic row kernel), 2^11 (k_nu_rows_combine8<11>), 2^12 (k_nu_rows_iw),
    2^13 (four-step, k_nu_fft_cols), 2^20 (k_nu_cols256) and 2^21 (k_nu_cols512); Z^2_2 and H_2."""
    case, nfft = E_CASES[key]
    for stat in (0, 1):
        check_nufft(case, 2, stat, nfft=None if nfft <= 1024 else nfft, max_nfft=1024 if nfft <= 1024 else None,
                    argmax=key in ("64", "700"))


@pytest.mark.parametrize("key", ["1401", "3000"])
def test_nufft_generic_fft_kernels(gpu, key):
    """CRIMP_NUFFT_ROWS4096=0: the generic kernels at 2^11 and 2^12, held to the truth themselves."""
    case, nfft = E_CASES[key]
    with hooks(CRIMP_NUFFT_ROWS4096=0):
        check_nufft(case, 2, 0, nfft=nfft)


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_nufft_gather_lanes(gpu, lanes):
    """The cell gather at every lane width, m in {2, 8, 9}: one launch carries up to 8 harmonics, m = 9 takes two."""
    with hooks(CRIMP_NUFFT_SPREAD="gather", CRIMP_NUFFT_LANES=lanes):
        for m, stat in ((2, 0), (8, 1), (9, 0)):
            check_nufft(E_GATHER, m, stat, mmax=9, spread="gather", argmax=lanes == 1)


@pytest.mark.parametrize("m", [2, 10, 11, 20])
def test_nufft_mfma_slots(gpu, m):
    """The MFMA-slot spread on 3 rows x 64 trials: 10 harmonics per photon pass, so m = 10, 11 and 20 take 1, 2 and 2."""
    with hooks(CRIMP_NUFFT_SPREAD="mfma"):
        for stat in (0, 1):
            check_nufft(E_MFMA, m, stat, mmax=20, spread="mfma")


@pytest.mark.parametrize("key", list(E_WRAPS))
def test_nufft_cell_wraps(gpu, key):
    for stat in (0, 1):
        check_nufft(E_WRAPS[key], 2, stat, argmax=key != "none")


@pytest.mark.parametrize("n", list(E_FEW))
def test_nufft_few_photons(gpu, n):
    """3 and 33 photons on 700 trials: the truncation errors of so few photons add coherently, so the unit's N-fold
    worst case is nearly reached at the row edges and a plan one moment short exceeds it there."""
    for stat in (0, 1):
        check_nufft(E_FEW[n], 2, stat, nfft=1024)


def test_nufft_linspace_grid_term(gpu):
    """An np.linspace grid: the NUFFT evaluates f0 + j delta, a few ulp from f[j]; the unit's grid term is non-zero."""
    c = E_LINSPACE
    assert R.nufft_grid_deviation(c.f, np.arange(c.nf)).any()
    for stat in (0, 1):
        check_nufft(c, 2, stat)


def test_nufft_h20_on_noise(gpu):
    """H_20 of unpulsed photons: sum_k Z^2_k / |H| >= 50 at some trial (the cancellation DESIGN.md section 8's
    exception is about), the raw NUFFT still inside its unit there."""
    idx, T = E_NOISE.truth(20)
    assert (T.g[-1] / np.abs(T.power(1))).max() >= 50.0
    check_nufft(E_NOISE, 20, 1)


# ------------------------------------------------------------------------------------------------- f. agreement
def test_paths_agree_within_the_sum_of_their_units(gpu):
    """Two paths on one case differ by at most the sum of their units: no tolerance of its own."""
    from crimp_amd import _native as N
    case, m = E_GATHER, 9
    idx, T = case.truth(m)
    for stat in (0, 1):
        f64, p0, _, _ = search(case, m, stat, "f64")
        raw, p2, _, plan = search(case, m, stat, "nufft", N.FLAG_NO_FIXUP)
        dflt, _, _, _ = search(case, m, stat, None)
        assert (p0, p2) == (0, 2)
        u64, unu, udf = R.fp64_unit(T, stat), nufft_units(case, T, idx, stat, plan)[0], R.default_unit(T, stat)
        assert (np.abs(f64[idx] - raw[idx]) <= u64 + unu).all()
        assert (np.abs(f64[idx] - dflt[idx]) <= u64 + udf).all()
    case, m = D_CASES["2d-2x300"]
    idx, T = case.truth(m)
    for stat in (0, 1):
        f64, _, _, _ = search(case, m, stat, "f64")
        raw, p1, _, _ = search(case, m, stat, "exact", N.FLAG_NO_FIXUP)
        assert p1 == 1
        assert (np.abs(f64[idx] - raw[idx]) <= R.fp64_unit(T, stat) + R.exact_raw_unit(T, stat)[0]).all()
