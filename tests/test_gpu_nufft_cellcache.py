"""The NUFFT plan cache's cell-start tables (csrc/search_nufft.h: NuCellTab, k_nu_gather's CHECK form) and the
progression check in front of every plan (csrc/search_exact.h: k_ap_check, k_ap_final). A repeated search over the same buffers skips the
cell-start pass and gathers from the tables the first search built; its gathers verify them against the photons they
read, so whatever happens to the buffers between two calls the result is exactly a fresh search's
(CRIMP_NUFFT_PLAN_CACHE=0), kernel family included.

Shape: 20 000 photons over 2e4 s, 20 000 trials at 1 / (10 T), m = 3: ~6 photons per cell at k = 1, fewer at k = 2, 3,
so 64 consecutive photons cross many cell boundaries and sit at every lane and iteration position of the gather."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PH, SPAN, F0, M = 20_000, 2.0e4, 3.3, 3
WINDOW = range(7001, 7065)  # interior photons: neither the first nor the last, which k_ap_final compares


def _path():
    from crimp_amd import _native as N
    return N.load().crimp_last_search_path()


def _events(seed):
    from crimp_amd.synth import pulsed_events
    return pulsed_events(N_PH, SPAN, F0, pulsed_frac=0.1, seed=seed)


def _grid():
    return F0 + np.arange(-10_000, 10_000) / (10.0 * SPAN)


class _Search:
    """One photon tensor and grid on the device; run(cache) searches with or without the plan cache."""

    def __init__(self, gpu, monkeypatch, t_h, f=None):
        import torch
        self.mp = monkeypatch
        self.t = torch.as_tensor(t_h, device=gpu)
        self.f = torch.as_tensor(_grid(), device=gpu) if f is None else f
        self.t0 = (t_h[0] + t_h[-1]) / 2

    def run(self, cache):
        from crimp_amd import ops
        if cache:
            self.mp.delenv("CRIMP_NUFFT_PLAN_CACHE", raising=False)
        else:
            self.mp.setenv("CRIMP_NUFFT_PLAN_CACHE", "0")
        z = ops.search(self.t, self.t0, self.f, M, 0).cpu().numpy()
        return z, _path()


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
def test_reuse_is_exact(gpu, monkeypatch, lanes):
    """The second search reuses every table (built = 0) and equals the first and the fresh one bit for bit."""
    from crimp_amd import _native as N
    monkeypatch.setenv("CRIMP_NUFFT_LANES", str(lanes))
    s = _Search(gpu, monkeypatch, _events(101 + lanes))
    first, p1 = s.run(True)
    built, reused = N.last_nufft_cells()
    assert (built, reused) == (M, 0) and p1 == 2
    again, p2 = s.run(True)
    assert N.last_nufft_cells() == (0, M) and p2 == 2
    fresh, p3 = s.run(False)
    assert N.last_nufft_cells() == (M, 0) and p3 == 2
    np.testing.assert_array_equal(again, first)
    np.testing.assert_array_equal(again, fresh)
    # CRIMP_NUFFT_CELL_CACHE=0: the cached plan with tables rebuilt
    monkeypatch.setenv("CRIMP_NUFFT_CELL_CACHE", "0")
    rebuilt, p4 = s.run(True)
    assert N.last_nufft_cells() == (M, 0) and p4 == 2
    np.testing.assert_array_equal(rebuilt, first)


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_only_the_gather_can_see_it(gpu, monkeypatch, lanes):
    """Edits of interior photons leave the plan's scalars alone (k_ap_final passes): only the gather's own checks can
    notice that a cached table no longer fits. For every photon of the window, one edit at a time -- (a) swapped with
    its successor (disorder), (b) set equal to its successor (sorted, equal neighbours, maybe another cell), (c) moved to
    the midpoint of its neighbours (sorted, maybe another cell) -- the cached call equals the fresh one exactly."""
    import torch
    from crimp_amd import _native as N
    monkeypatch.setenv("CRIMP_NUFFT_LANES", str(lanes))
    s = _Search(gpu, monkeypatch, _events(7))
    t, orig = s.t, s.t.clone()

    def swap(i):
        t[i:i + 2] = orig[i:i + 2].flip(0)

    def equal_next(i):
        t[i] = orig[i + 1]

    def midpoint(i):
        t[i] = (orig[i - 1] + orig[i + 1]) / 2

    paths, cells = {}, {}
    for name, edit in (("swap", swap), ("equal_next", equal_next), ("midpoint", midpoint)):
        for i in WINDOW:
            t.copy_(orig)
            s.run(True)                 # the plan and tables of the original photons are cached
            edit(i)
            got, pg = s.run(True)
            cells.setdefault(name, set()).add(N.last_nufft_cells())
            ref, pr = s.run(False)
            assert pg == pr, (name, i, pg, pr)
            np.testing.assert_array_equal(got, ref, err_msg="%s at %d" % (name, i))
            paths.setdefault(name, set()).add(pg)
    # disorder takes the exact rule; sorted buffers, equal neighbours included, stay on the NUFFT
    assert paths["swap"] == {1} and paths["equal_next"] == {2} and paths["midpoint"] == {2}, paths
    # the gather is what noticed: a swap always fails its order check and the search is redone with fresh tables; of
    # the sorted edits some move the photon to another cell (redone) and some do not (the cached tables still hold)
    assert cells["swap"] == {(M, 0)}, cells
    assert cells["equal_next"] == cells["midpoint"] == {(M, 0), (0, M)}, cells
    assert torch.equal(torch.sort(orig).values, orig)


def test_other_tensor_at_the_same_address(gpu, monkeypatch):
    """A freed photon tensor's address given to another tensor of the same size, first and last value: the cache key
    and the plan's scalars match, the tables do not."""
    import torch
    a = _events(31)
    b = np.sort(np.clip(_events(32), a[0], a[-1]))
    b[0], b[-1] = a[0], a[-1]
    assert np.all(np.diff(b) >= 0) and not np.array_equal(a, b)
    s = _Search(gpu, monkeypatch, a)
    s.run(True)
    s.run(True)
    ptr = s.t.data_ptr()
    s.t = None
    s.t = torch.as_tensor(b, device=gpu)
    if s.t.data_ptr() != ptr:
        pytest.skip("the allocator gave the new tensor another address")
    got, pg = s.run(True)
    ref, pr = s.run(False)
    assert pg == pr == 2
    np.testing.assert_array_equal(got, ref)


def test_bounded_memory(gpu, monkeypatch):
    """40 searches over distinct live tensors: the cache keeps 16 plans' tables and frees or reuses the others'."""
    import torch
    from crimp_amd import _native as N
    f = torch.as_tensor(_grid(), device=gpu)
    ss = [_Search(gpu, monkeypatch, _events(200 + k), f) for k in range(40)]
    free = {}
    for k, s in enumerate(ss):
        s.run(True)
        if k + 1 in (16, 40):
            torch.cuda.synchronize()
            free[k + 1] = torch.cuda.mem_get_info()[0]
    got, pg = ss[0].run(True)  # evicted long ago
    ref, pr = ss[0].run(False)
    assert pg == pr == 2
    np.testing.assert_array_equal(got, ref)
    # one search's tables: harmonic k spans k T n delta = k n / 10 cells of the length-n FFT's grid, 8 bytes each
    nfft = N.last_nufft_plan()[0]
    one_table = 8 * sum(k * nfft // 10 + 3 for k in (1, 2, 3))
    assert free[16] - free[40] <= 16 * one_table + (64 << 20), (free, one_table)


def _predict(f):
    """The progression criterion on the host: 16 ulp of max|f| around f_0 + j delta, delta from the ends."""
    nf = len(f)
    d = (f[-1] - f[0]) / (nf - 1)
    dev = np.abs(f - (f[0] + np.arange(nf, dtype=np.float64) * d)).max()
    return bool(np.isfinite(d) and d != 0.0 and dev <= 16.0 * 2.220446049250313e-16 * np.abs(f).max())


@pytest.mark.parametrize("nf", [2, 3, 5000, 2_200_000])
def test_plan_check_sizes(gpu, nf):
    """The progression check (block partials, then their reduction) at one block (nf = 2, 3), a size that is no
    multiple of a block's 2048 trials, and more trials than one sweep of kApBlocks blocks covers. 50 calls alternate a
    progression and the same grid with one element moved by 1e-9 relative; every call takes the path the host's
    evaluation of the criterion predicts: nothing of one call's check is left standing for the next. Grids shorter
    than 256 trials reach the check only when the factorised kernel is demanded, which then refuses a grid that is no
    progression. (The reduction folded into the check's last block was measured and not adopted; this
    is the test it has to pass.)"""
    import torch
    from crimp_amd import ops, _native as N
    from crimp_amd.synth import pulsed_events
    t_h = pulsed_events(5000, 2.0e3, F0, pulsed_frac=0.1, seed=5)
    t = torch.as_tensor(t_h, device=gpu)
    t0 = (t_h[0] + t_h[-1]) / 2
    good = F0 + np.arange(nf) * (1.0e-3 / nf)
    moved = good.copy()
    moved[nf // 2] *= 1.0 + 1e-9
    grids = [(torch.as_tensor(g, device=gpu), _predict(g)) for g in (good, moved)]
    assert grids[0][1] and grids[1][1] == (nf == 2)  # (two trials are a progression whatever they are)
    force = N.FLAG_FORCE_MFMA if nf < 256 else 0
    for call in range(50):
        f, ok = grids[call % 2]
        if force and not ok:
            with pytest.raises(N.CrimpNativeError, match="not an arithmetic progression"):
                ops.search(t, t0, f, 1, 0, flags=force, precision="exact")
            continue
        ops.search(t, t0, f, 1, 0, flags=force, precision="exact")
        assert _path() == (1 if ok else 0), (nf, call, ok)
