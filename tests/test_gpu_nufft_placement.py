"""Where the NUFFT search's row passes run never changes what they compute (csrc/search_nufft.h).

The row passes give every XCD a contiguous range of rows (nu_row_of_block; CRIMP_NUFFT_ROW_MAP=linear: block b takes
row b, the map before). That only moves work: every sum keeps its operands and their order, so against the hook the
powers are equal bit for bit (torch.equal on the float64 output), the best trial (power and index) is equal, and the
fix-up list holds the same trials (those the fix-up rewrote: output != raw output). Every case runs on a fresh plan and
on the repeated call (the cached plan).

The generic row kernel (CRIMP_NUFFT_ROWS4096=0 with CRIMP_NUFFT_FINAL=separate) runs the same map and is compared with
itself under the hook bit for bit; against the radix-8 kernels it differs in rounding by design (radix-16 stages), so
that comparison holds the bound tests/test_gpu_nufft.py::test_nufft_specialised_fft_kernels_equal_generic sets for the
same pair of kernels on raw powers: 1e-10 relative at most, 1e-13 in the median.

The map moves a row only from n1 = 16 on: at n1 = 8 it is the identity ((b & 7) * 1 + (b >> 3) = b for b < 8), below
that it falls back to row b. The slice cases therefore run at n1 = 16 and 64."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F0 = 3.3


def _path():
    from crimp_amd import _native as N
    return N.load().crimp_last_search_path()


class _Case:
    """One photon tensor and grid on the device. run(env) -> what a search returns under those hooks, from a fresh
    plan and from the repeated call (the cached plan: the gather's CHECK form on the kept cell-start tables)."""

    def __init__(self, gpu, monkeypatch, t_h, f_h, nharm, stat, fd=None, first=0, count=None, nfft=None):
        import torch
        self.mp = monkeypatch
        self.t = torch.as_tensor(np.array(t_h), device=gpu)
        self.f = torch.as_tensor(f_h, device=gpu)
        self.fd = None if fd is None else torch.as_tensor(np.asarray(fd, dtype=np.float64), device=gpu)
        self.t0 = (t_h[0] + t_h[-1]) / 2
        self.nharm, self.stat, self.first, self.count, self.nfft = nharm, stat, first, count, nfft

    def _search(self, flags=0):
        from crimp_amd import ops, _native as N
        z, bv, bi = ops.search_best(self.t, self.t0, self.f, self.nharm, self.stat, self.fd, first=self.first,
                                    count=self.count, flags=flags)
        assert _path() == 2, "the search left the NUFFT"
        if self.nfft is not None:
            assert N.last_nufft_plan()[0] == self.nfft, N.last_nufft_plan()
        return z, float(bv), int(bi), int(N.load().crimp_last_fixups()), N.last_nufft_cells()

    def run(self, **env):
        from crimp_amd import _native as N
        hooks = ("CRIMP_NUFFT_ROW_MAP", "CRIMP_NUFFT_ROWS4096", "CRIMP_NUFFT_FINAL")
        for h in hooks:
            self.mp.delenv(h, raising=False)
        for k, v in env.items():
            self.mp.setenv(k, v)
        # a fresh plan whatever the cache holds for these buffers' addresses; then the cache filled; then reuse
        self.mp.setenv("CRIMP_NUFFT_PLAN_CACHE", "0")
        fresh = self._search()
        self.mp.delenv("CRIMP_NUFFT_PLAN_CACHE")
        self._search()
        again = self._search()
        raw = self._search(flags=N.FLAG_NO_FIXUP)
        assert fresh[4][1] == 0 and again[4] == raw[4] and again[4][0] == 0, (fresh[4], again[4], raw[4])
        return {"fresh": fresh, "again": again, "raw": raw}


def _same(a, b, what):
    import torch
    for call in ("fresh", "again", "raw"):
        (za, va, ia, na, _), (zb, vb, ib, nb, _) = a[call], b[call]
        assert torch.equal(za, zb), (what, call, "powers differ")
        assert (va, ia) == (vb, ib), (what, call, "best trial", (va, ia), (vb, ib))
        assert na == nb, (what, call, "fix-up count", na, nb)
    # the flagged trials as sets: those the fix-up rewrote
    fa = set(np.flatnonzero((a["again"][0] != a["raw"][0]).cpu().numpy()).tolist())
    fb = set(np.flatnonzero((b["again"][0] != b["raw"][0]).cpu().numpy()).tolist())
    assert fa == fb, (what, "flagged trials", sorted(fa ^ fb)[:8])
    # and a call's own results do not depend on where its plan came from
    assert torch.equal(a["fresh"][0], a["again"][0]), (what, "fresh vs repeated call")


# ---------------------------------------------------------------- the row passes' XCD map
@pytest.fixture(scope="module")
def pulsed():
    from crimp_amd.synth import pulsed_events
    t = pulsed_events(200_000, 2.0e5, F0, pulsed_frac=0.05, fdot=-2e-11, seed=8)
    t.setflags(write=False)
    return t


def _grid(m):
    return F0 + (np.arange(m) - m // 2) / 2.0e6


def _rows(c):
    """default (XCD map) == linear, bit for bit, with the radix-8 kernels and with the generic ones; the radix-8
    kernels against the generic ones to rounding (raw powers)."""
    lin = c.run(CRIMP_NUFFT_ROW_MAP="linear")
    new = c.run()
    _same(new, lin, "radix-8 rows")
    gen = c.run(CRIMP_NUFFT_ROWS4096="0", CRIMP_NUFFT_FINAL="separate")
    _same(gen, c.run(CRIMP_NUFFT_ROWS4096="0", CRIMP_NUFFT_FINAL="separate", CRIMP_NUFFT_ROW_MAP="linear"),
          "generic rows")
    x, y = new["raw"][0].cpu().numpy(), gen["raw"][0].cpu().numpy()
    rel = np.abs(x - y) / np.abs(y)
    assert rel.max() <= 1e-10 and np.median(rel) <= 1e-13, (rel.max(), np.median(rel))


# trials -> n: 6000 -> 2^13 (n1 = 2) and 12000 -> 2^14 (n1 = 4): the map falls back to row b; 30000 -> 2^15 (n1 = 8):
# the map is the identity; 55000 -> 2^16 (n1 = 16): the smallest n1 at which a row moves; 220000 -> 2^18 (n1 = 64)
@pytest.mark.parametrize("trials,nfft", [(6000, 1 << 13), (12000, 1 << 14), (30000, 1 << 15), (55000, 1 << 16),
                                         (220000, 1 << 18)])
@pytest.mark.parametrize("nharm,stat", [(1, 0), (3, 0), (5, 1)], ids=["Z2_1", "Z2_3", "H_5"])
def test_row_map_sizes(gpu, monkeypatch, pulsed, nharm, stat, trials, nfft):
    _rows(_Case(gpu, monkeypatch, pulsed, _grid(trials), nharm, stat, nfft=nfft))


# every slice at an n1 whose map moves rows (16 or 64)
SLICES = {
    # a non-zero first: cache lines of the outputs straddle the slice's start; 150001 trials of n = 2^18: the jhi / h
    # edges lie well inside the rows
    "first": dict(trials=440000, first=12345, count=150001, nfft=1 << 18),
    "short": dict(trials=150001, nfft=1 << 18),
    # two rows (blockIdx.y) at n1 = 16 and at n1 = 64
    "2d_n1_16": dict(trials=55000, fd=[-12.0, -11.0], nfft=1 << 16),
    "2d_n1_64": dict(trials=220000, fd=[-12.0, -11.0], nfft=1 << 18),
    # a slice that starts inside the first row and ends inside the second: two row groups, each its own plan
    "2d_partial_rows": dict(trials=220000, fd=[-12.0, -11.0], first=70001, count=300000, nfft=1 << 18),
}


@pytest.mark.parametrize("name", list(SLICES))
def test_row_map_slices(gpu, monkeypatch, pulsed, name):
    s = SLICES[name]
    _rows(_Case(gpu, monkeypatch, pulsed, _grid(s["trials"]), 3, 0, fd=s.get("fd"), first=s.get("first", 0),
                count=s.get("count"), nfft=s["nfft"]))
