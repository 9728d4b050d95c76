"""The NUFFT search's reporting hooks against the plan the CPU check program prints for the same scalars and hooks
(csrc/search_nufft_plan.h, tests/test_nufft_plan.py): what the library launched is what plan_nufft_search planned.

The inputs are exact in fp64 in any evaluation order -- photon times multiples of 2^-10 s, t0 = 2048, f0 = 3.25,
delta = 2^-21 -- so the scalars the device reads back are known here bit for bit."""
import os

import numpy as np
import pytest

from test_nufft_plan import AUTO, plan_check, run_plan  # noqa: F401 (plan_check is a fixture)

pytestmark = pytest.mark.gpu

T0, F0, DELTA = 2048.0, 3.25, 2.0 ** -21
FD = np.array([-12.0, -11.0, -10.5, -10.25])
CASES = {  # nf, rows, nharm, stat, first, count -> FFT length, spread form, row groups
    "gather_1d": ((1401, 1, 2, 0, 0, None), (1 << 11, "gather", 1)),
    "mfma_2d": ((3000, 3, 5, 1, 0, None), (1 << 12, "mfma", 1)),
    "four_step": ((5000, 1, 2, 0, 0, None), (1 << 13, "gather", 1)),
    "cut_range": ((200, 4, 2, 0, 100, 600), (None, "mfma", 3)),
}


@pytest.fixture(scope="module")
def photons():
    rng = np.random.default_rng(11)
    return np.sort(rng.integers(0, 4096 * 1024, 8000)).astype(np.float64) / 1024.0


@pytest.mark.parametrize("name", list(CASES))
def test_hooks_equal_the_checked_plan(gpu, plan_check, photons, name, monkeypatch):  # noqa: F811
    from crimp_amd import ops, _native as N
    for hook in ("CRIMP_NUFFT_SPREAD", "CRIMP_NUFFT_LANES", "CRIMP_NUFFT_ROWS4096", "CRIMP_NUFFT_FINAL"):
        monkeypatch.delenv(hook, raising=False)
    mb = int(os.environ.get("CRIMP_NUFFT_BUDGET_MB", "6144") or 0)
    budget = (mb if mb > 0 else 6144) << 20
    (nf, rows, nharm, stat, first, count), (nfft, form, ngroups) = CASES[name]
    t = photons
    f = F0 + np.arange(nf) * DELTA
    fd = FD[:rows] if rows > 1 else None
    hs = (DELTA, F0, t[0] - T0, t[-1] - T0)
    p = run_plan(plan_check, hs, t.size, nf, rows=rows, nharm=nharm, stat=stat, first=first, count=count, spread=AUTO,
                 budget=budget)
    assert p["applicable"] == 1 and len(p["groups"]) == ngroups
    assert nfft in (None, p["last_n"]) and ("gather" if p["gather"] else "mfma") == form

    z = ops.search(t, T0, f, nharm, stat, log10_negfdot=fd, first=first, count=count, flags=N.FLAG_TIME_KERNELS,
                   precision="nufft")
    assert N.load().crimp_last_search_path() == 2
    times = N.last_kernel_times()
    assert N.last_nufft_plan() == (p["last_n"], p["last_p"], form)
    work = N.last_nufft_work()
    got = [work[k] for k in ("spread_flops", "spread_bytes", "merge_bytes", "pass1_bytes", "pass2_bytes",
                             "combine_bytes", "finalize_bytes")]
    assert got == p["work"]
    assert N.last_nufft_cells() == (p["cell_tables"], 0)
    assert len(times) >= 15 and times[8:15] == [float(c) for c in p["launches"]]

    ref = ops.search(t, T0, f, nharm, stat, log10_negfdot=fd, first=first, count=count, precision="f64")
    err = np.abs(z - ref) / np.abs(ref)
    assert z.shape == ref.shape == (p["count"],)
    assert err.max() <= 1e-6, "max relative error %.3g at %d" % (err.max(), int(err.argmax()))
