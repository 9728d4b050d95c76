"""The host finish of a folded NUFFT search (csrc/search_nufft_finish.h) on the CPU.

`make -C crimp_amd/csrc nufft-finish-check` builds search_nufft_finish_check.cpp with the host compiler under
-fsanitize=address,undefined; every check below is one run of that program (no GPU, no preloaded library). A repeated
cell-gather search on a cached plan reads one block back and finishes on the host what k_ap_final and k_best_final
did on the device: the reduce of the progression check's partials, the cached plan's test clause by clause, and the
reduce of the best-trial candidates (np.argmax semantics)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crimp_amd", "csrc")
BOUND = 16.0 * 2.0 ** -52
I64MAX = 2 ** 63 - 1


@pytest.fixture(scope="module")
def exe():
    r = subprocess.run(["make", "-s", "-B", "-C", CSRC, "nufft-finish-check"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(CSRC, "build", "nufft_finish_check")


def fhex(v):
    v = float(v)
    return v.hex() if np.isfinite(v) else repr(v)


def ask(exe, text):
    """One run of the check program -> its answer lines, split."""
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def partials(exe, part):
    part = np.asarray(part, dtype=np.float64).reshape(-1, 2)
    (ans,) = ask(exe, "partials %d %s\n" % (len(part), " ".join(fhex(v) for v in part.ravel())))
    assert ans[0] == "partials"
    return float.fromhex(ans[1]), float.fromhex(ans[2])


def plan_ok(exe, nf, dev, fm, pub, expect):
    (ans,) = ask(exe, "plan %d %s\n" % (nf, " ".join(fhex(v) for v in (dev, fm, *pub, *expect))))
    assert ans[0] == "plan" and ans[1] in ("0", "1")
    return ans[1] == "1"


def best(exe, cands):
    (ans,) = ask(exe, "best %d %s\n" % (len(cands), " ".join("%s %d" % (fhex(v), i) for v, i in cands)))
    assert ans[0] == "best"
    return float(ans[1]) if "nan" in ans[1] or "inf" in ans[1] else float.fromhex(ans[1]), int(ans[2])


def test_partial_reduce_matches_numpy(exe):
    """The maxima of the check blocks' (deviation, |f|) pairs: random pairs of 1, 7, 64 and 1024 blocks against
    numpy, the empty list (0, 0), and a NaN pair, which never wins (fmax, as on the device)."""
    rng = np.random.default_rng(5)
    for nb in (1, 7, 64, 1024):
        part = np.abs(rng.standard_normal((nb, 2))) * 10.0 ** rng.integers(-20, 5, (nb, 2))
        assert partials(exe, part) == (part[:, 0].max(), part[:, 1].max())
    assert partials(exe, np.zeros((0, 2))) == (0.0, 0.0)
    part = np.array([[1e-16, 3.0], [np.nan, np.nan], [2e-16, 2.5]])
    assert partials(exe, part) == (2e-16, 3.0)


def test_plan_test_clause_by_clause(exe):
    """k_ap_final's test of a cached plan, each clause alone: a valid plan passes; a non-finite step, a zero step, a
    deviation one ulp above 16 ulp of max |f|, and each of the four scalars one ulp off fail. The step is formed as on
    the device, (f[nf-1] - f[0]) / (nf - 1)."""
    nf = 2001
    f0, flast, dt0, dtn = 3.2995, 3.3005, -1.0e5, 1.0e5 + 0.125
    d = (flast - f0) / float(nf - 1)
    fm = max(abs(f0), abs(flast))
    pub, expect = [f0, flast, dt0, dtn], [d, f0, dt0, dtn]
    lim = BOUND * fm
    assert plan_ok(exe, nf, 0.0, fm, pub, expect)
    assert plan_ok(exe, nf, lim, fm, pub, expect)                        # the bound itself holds
    assert not plan_ok(exe, nf, np.nextafter(lim, np.inf), fm, pub, expect)
    assert not plan_ok(exe, nf, np.nan, fm, pub, expect)
    # a step that is not finite (an infinite or NaN end of the grid), against a cached step that "equals" it
    assert not plan_ok(exe, nf, 0.0, np.inf, [f0, np.inf, dt0, dtn], [np.inf, f0, dt0, dtn])
    assert not plan_ok(exe, nf, 0.0, fm, [f0, np.nan, dt0, dtn], [np.nan, f0, dt0, dtn])
    # a zero step (a constant grid), against a cached step of zero
    assert not plan_ok(exe, nf, 0.0, fm, [f0, f0, dt0, dtn], [0.0, f0, dt0, dtn])
    # each scalar one ulp off, upwards and downwards: the step (through the cached value), f0, dt[0], dt[n-1]
    for q in range(4):
        for to in (np.inf, -np.inf):
            ex = list(expect)
            ex[q] = np.nextafter(ex[q], to)
            assert not plan_ok(exe, nf, 0.0, fm, pub, ex), (q, to)
    # ... and through the published values: f[nf-1] a few ulp off moves the step, f0, dt[0], dt[n-1] one ulp
    moved = [f0, np.nextafter(flast, np.inf), dt0, dtn]
    while (moved[1] - f0) / float(nf - 1) == d:
        moved[1] = np.nextafter(moved[1], np.inf)
    assert not plan_ok(exe, nf, 0.0, fm, moved, expect)
    for q in (0, 2, 3):
        pb = list(pub)
        pb[q] = np.nextafter(pb[q], np.inf)
        ex = list(expect)
        ex[0] = (pb[1] - pb[0]) / float(nf - 1)  # (the step follows f0: only the scalar under test differs)
        assert not plan_ok(exe, nf, 0.0, fm, pb, ex), q


def test_candidate_reduce_is_argmax(exe):
    """best_better's rule over the fused finalize's candidates: the largest value, ties to the lowest index wherever
    they stand in the list, a NaN above +inf, the first NaN (lowest index) of two, the empty list (-inf, INT64_MAX)
    and a single candidate; random lists against np.argmax."""
    assert best(exe, []) == (-np.inf, I64MAX)
    assert best(exe, [(2.5, 17)]) == (2.5, 17)
    assert best(exe, [(-np.inf, 3)]) == (-np.inf, 3)
    assert best(exe, [(1.0, 40), (7.0, 30), (7.0, 10), (7.0, 20), (6.0, 0)]) == (7.0, 10)
    assert best(exe, [(7.0, 10), (7.0, 30), (7.0, 20)]) == (7.0, 10)
    v, i = best(exe, [(np.inf, 1), (np.nan, 9), (np.inf, 12)])
    assert np.isnan(v) and i == 9
    v, i = best(exe, [(3.0, 0), (np.nan, 50), (np.nan, 20), (np.inf, 60)])
    assert np.isnan(v) and i == 20
    rng = np.random.default_rng(11)
    for n in (2, 256, 928):
        x = np.round(rng.standard_normal(4 * n) * 3.0)  # many ties
        # candidate b: the best of the slice b, b + n, b + 2n, ... as a block of the row pass would leave it
        cands = []
        for b in range(n):
            idx = np.arange(b, 4 * n, n)
            k = idx[np.argmax(x[idx])]
            cands.append((x[k], int(k)))
        assert best(exe, cands) == (x.max(), int(np.argmax(x)))
