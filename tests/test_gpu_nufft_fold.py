"""The folded repeat search (csrc/search_nufft.h, NuRun::fold): a cell-gather NUFFT search on a cached plan launches no
k_ap_check, k_ap_final or k_best_final. The progression check rides in its first gather launch, a failing gather wave
stores the search's epoch, and one read-back brings the flags, the plan's scalars, the check's partials and the
best-trial candidates to the host, which finishes them (csrc/search_nufft_finish.h). CRIMP_NUFFT_FOLD=0 keeps the three
launches: every result here is held to that form bit for bit, and every stale plan to a search without the plan
cache."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEP = 1.0 / 2.0e6  # a tenth of 1 / T
FD2 = np.array([-12.0, -10.5])
KEEP = []  # every device buffer of this module stays allocated: no two cases share a plan-cache key


@pytest.fixture(scope="module")
def photons():
    from crimp_amd.synth import pulsed_events
    t = pulsed_events(200_000, 2.0e5, 3.3, pulsed_frac=0.05, fdot=-2e-11, seed=17)
    return t, (t[0] + t[-1]) / 2


def grid(nf):
    return 3.3 + (np.arange(nf) - nf // 2) * STEP


def _path():
    from crimp_amd import _native as N
    return N.load().crimp_last_search_path()


def _fold(monkeypatch, on):
    if on:
        monkeypatch.delenv("CRIMP_NUFFT_FOLD", raising=False)
    else:
        monkeypatch.setenv("CRIMP_NUFFT_FOLD", "0")


def _cache(monkeypatch, on):
    if on:
        monkeypatch.delenv("CRIMP_NUFFT_PLAN_CACHE", raising=False)
    else:
        monkeypatch.setenv("CRIMP_NUFFT_PLAN_CACHE", "0")


def _search(t, t0, f, m, stat, fd, want_best):
    """-> (powers, best power or None, best index or None)"""
    from crimp_amd import ops
    if want_best:
        z, bv, bi = ops.search_best(t, t0, f, m, stat, log10_negfdot=fd)
        return z.cpu().numpy(), float(bv), int(bi)
    return ops.search(t, t0, f, m, stat, log10_negfdot=fd).cpu().numpy(), None, None


def _same(a, b, msg=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=str(msg))
    assert a[1:] == b[1:] or (a[1] != a[1] and b[1] != b[1] and a[2] == b[2]), (msg, a[1:], b[1:])


@pytest.mark.parametrize("want_best", [False, True], ids=["powers", "best"])
@pytest.mark.parametrize("rows", [1, 2])
def test_fold_same_bits_as_three_launches(gpu, photons, rows, want_best, monkeypatch):
    """Grids of 64 (the smallest the NUFFT takes), 2000, 2049 and 4097 trials per row, Z^2_1, Z^2_2 and H_5: a fresh
    search and two cached repeats with the fold, and the same three with CRIMP_NUFFT_FOLD=0 on buffers of their own (so
    that each form starts from no plan), give the same powers and best trial bit for bit; the best is np.argmax of the
    powers; every search runs the NUFFT and the repeats take their start tables from the cache."""
    import torch
    from crimp_amd import _native as N
    t_h, t0 = photons
    fd = None if rows == 1 else torch.as_tensor(FD2, device=gpu)
    for nf in (64, 2000, 2049, 4097):
        for m, stat in ((1, 0), (2, 0), (5, 1)):
            res = {}
            for fold in (True, False):
                _fold(monkeypatch, fold)
                t = torch.as_tensor(t_h, device=gpu).clone()
                f = torch.as_tensor(grid(nf), device=gpu).clone()
                KEEP.extend((t, f))
                runs = []
                for rep in range(3):
                    runs.append(_search(t, t0, f, m, stat, fd, want_best))
                    assert _path() == 2, (nf, m, stat, fold, rep)
                    built, reused = N.last_nufft_cells()
                    assert (built > 0 and reused == 0) if rep == 0 else (built == 0 and reused > 0), \
                        (nf, m, stat, fold, rep, built, reused)
                    assert N.load().crimp_last_fixups() == 0
                for r in runs[1:]:
                    _same(r, runs[0], (nf, m, stat, fold))
                res[fold] = runs[0]
            _same(res[True], res[False], (nf, m, stat))
            if want_best:
                z, bv, bi = res[True]
                assert bi == int(np.argmax(z)) and bv == z[bi], (nf, m, stat, bv, bi)


def _stale_case(monkeypatch, gpu, photons, nf, rows, want_best, edits):
    """Each edit in place between cached calls: the stale plan's search equals the search without the plan cache, path
    included. edits: (name, edit(t, f), restore) -- restore: the buffers are put back first."""
    import torch
    t_h, t0 = photons
    f_h = grid(nf)
    fd = None if rows == 1 else torch.as_tensor(FD2, device=gpu)
    t = torch.as_tensor(t_h, device=gpu).clone()
    f = torch.as_tensor(f_h, device=gpu).clone()
    KEEP.extend((t, f))
    _fold(monkeypatch, True)

    def run(cache):
        _cache(monkeypatch, cache)
        r = _search(t, t0, f, 2, 0, fd, want_best)
        return r, _path()

    first, p1 = run(True)
    again, p2 = run(True)
    assert p1 == p2 == 2
    _same(again, first)
    for name, edit, restore in edits:
        if restore:
            t.copy_(torch.as_tensor(t_h, device=gpu))
            f.copy_(torch.as_tensor(f_h, device=gpu))
            run(True)
        run(True)              # the plan of the current buffers is cached
        edit(t, f)
        got, pg = run(True)    # the stale plan: found by the host finish or a gather wave, recomputed
        ref, pr = run(False)
        assert pg == pr, (name, pg, pr)
        _same(got, ref, name)
    return t, f, run


def _edits(nf):
    def put(i, dv):
        return lambda t, f: f.__setitem__(i, f[i] + dv)
    return [("shift photons", lambda t, f: t.add_(0.37), False),
            ("rescale grid", lambda t, f: f.mul_(1.0 + 1e-7), False),
            ("swap two photons", lambda t, f: t.__setitem__(slice(1000, 1002), t[1000:1002].flip(0).clone()), False),
            ("restore order", lambda t, f: t.copy_(t.sort().values), False),
            ("non-uniform grid", put(7, 1e-9), False),
            ("f[0] alone", put(0, 1e-9), True),
            ("f[nf-1] alone", put(nf - 1, 1e-9), True),
            ("f[nf-2]", put(nf - 2, 1e-9), True)]


@pytest.mark.parametrize("want_best", [False, True], ids=["powers", "best"])
@pytest.mark.parametrize("rows", [1, 2])
def test_fold_stale_plans_redone(gpu, photons, rows, want_best, monkeypatch):
    """The five in-place edits of test_nufft_plan_cache_revalidated_on_device, then f[0] alone, f[nf-1] alone and
    f[nf-2] (only the check's deviation sees it), on a 4097-trial grid (three check blocks, the last partly filled)."""
    _stale_case(monkeypatch, gpu, photons, 4097, rows, want_best, _edits(4097))


def test_fold_stale_plan_beyond_check_block_cap(gpu, photons, monkeypatch):
    """The check rides in at most 64 blocks of 2048 trials per sweep: a grid of 133121 trials takes a second, partly
    filled sweep, and an edit there (trial 133000) is seen like any other."""
    nf = 64 * 2048 + 2048 + 1
    _stale_case(monkeypatch, gpu, photons, nf, 1, True,
                [("strided tail", lambda t, f: f.__setitem__(133000, f[133000] + 1e-9), False)])


@pytest.mark.parametrize("rows", [1, 2])
def test_fold_after_a_mismatch(gpu, photons, rows, monkeypatch):
    """After a detected mismatch the redo's plan is cached: the next two repeats reuse its start tables and equal the
    fresh result, and forty repeats in a row stay identical (every search has its own epoch, and the flag words of the
    earlier ones are still in the block)."""
    from crimp_amd import _native as N
    t, f, run = _stale_case(monkeypatch, gpu, photons, 2049, rows, True, [])
    t.add_(0.37)
    got, p = run(True)  # the stale plan, redone from a fresh one
    assert p == 2 and N.last_nufft_cells()[0] > 0
    ref, _ = run(False)
    _same(got, ref)
    for rep in range(42):
        r, p = run(True)
        assert p == 2 and N.last_nufft_cells()[0] == 0 and N.last_nufft_cells()[1] > 0, rep
        _same(r, ref, rep)
    # a mismatch only the gather sees (the scalars, the grid and the order hold; 600 photons move to the time of a
    # later one, across a cell boundary: a cell of the second harmonic holds ~250 photons) and the repeats after it
    t[5000:5600] = t[5600].clone()
    got, p = run(True)
    ref, _ = run(False)
    assert p == 2
    _same(got, ref)
    for rep in range(3):
        r, p = run(True)
        assert p == 2 and N.last_nufft_cells()[1] > 0
        _same(r, ref, rep)


def test_fold_fixup_counter(gpu):
    """The fix-up count is zeroed by the first gather launch and added to by the launches after it: with many fix-ups
    forced (CRIMP_FIXUP_REL in a child process) three repeated calls report the same count, the count of the
    three-launch form, and the same powers and best trial."""
    from conftest import ROOT
    code = ("import sys, os, numpy as np, torch; sys.path.insert(0, %r); from crimp_amd import ops, _native as N; "
            "from crimp_amd.synth import pulsed_events; "
            "t_h = pulsed_events(200000, 2.0e5, 3.3, pulsed_frac=0.05, fdot=-2e-11, seed=17); "
            "t0 = (t_h[0] + t_h[-1]) / 2; f_h = 3.3 + (np.arange(20000) - 10000) / 2.0e6; out = {}\n"
            "for mode in ('1', '0'):\n"
            "    os.environ['CRIMP_NUFFT_FOLD'] = mode\n"
            "    t = torch.as_tensor(t_h, device='cuda').clone(); f = torch.as_tensor(f_h, device='cuda').clone()\n"
            "    for rep in range(4):\n"
            "        z, bv, bi = ops.search_best(t, t0, f, 3, 1)\n"
            "        out[mode, rep] = (z.cpu().numpy(), np.array([bv, bi, N.load().crimp_last_fixups(), "
            "N.load().crimp_last_search_path(), N.last_nufft_cells()[1]]))\n"
            "np.savez(sys.argv[1], **{'z%%s%%d' %% k: v[0] for k, v in out.items()}, "
            "**{'m%%s%%d' %% k: v[1] for k, v in out.items()})") % ROOT
    with tempfile.TemporaryDirectory() as d:
        outp = os.path.join(d, "f.npz")
        subprocess.run([sys.executable, "-c", code, outp], check=True, timeout=300,
                       env=dict(os.environ, CRIMP_FIXUP_REL="1e-9"))
        r = dict(np.load(outp))
    assert r["m10"][2] > 100 and r["m10"][3] == 2  # fix-ups ran, after a NUFFT
    for mode in "10":
        for rep in range(4):
            np.testing.assert_array_equal(r["z%s%d" % (mode, rep)], r["z10"], err_msg="%s %d" % (mode, rep))
            np.testing.assert_array_equal(r["m%s%d" % (mode, rep)][:4], r["m10"][:4], err_msg="%s %d" % (mode, rep))
            assert (r["m%s%d" % (mode, rep)][4] > 0) == (rep > 0)  # the repeats ran the cached plan's tables
    assert r["m10"][1] == np.argmax(r["z10"]) and r["m10"][0] == r["z10"].max()
