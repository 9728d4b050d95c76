"""Trial blocking of the fp64 direct search and of the fp64 fix-up at a small size (otherwise reached only by the
full-size tests): the same search under the default buffer budget (one trial block) and under CRIMP_SEARCH_BUDGET_MB=1
(several) returns the same bits. The hooks are read at the start of every search (SearchHooks::from_env), so both runs
share one process; tests/test_search_plan.py::test_gpu_test_plans pins the plans named below."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_PHOTONS, F0 = 40_000, 7.123456789


@pytest.fixture(scope="module")
def photons(gpu):
    import torch
    from crimp_amd.synth import pulsed_events
    t_h = pulsed_events(N_PHOTONS, 4.0e4, F0, pulsed_frac=0.1, seed=4)
    return torch.as_tensor(t_h, device=gpu), (t_h[0] + t_h[-1]) / 2


def _grid(gpu, m):
    import torch
    return torch.as_tensor(F0 + (np.arange(m) - m // 2) / 4.0e5, device=gpu)


def test_direct_trial_blocks(gpu, photons, monkeypatch):
    """H_20 over 3000 trials by the fp64 kernel: 2 photon splits of 20000; the 1 MiB budget holds the partial sums of
    1638 trials, so the search runs as blocks of 1536 + 1464 trials where the default budget takes all 3000 at once."""
    from crimp_amd import ops, _native as N
    t, t0 = photons
    f = _grid(gpu, 3000)
    monkeypatch.delenv("CRIMP_SEARCH_BUDGET_MB", raising=False)
    h = ops.search(t, t0, f, 20, 1, precision="f64").cpu().numpy()
    assert N.load().crimp_last_search_path() == 0
    monkeypatch.setenv("CRIMP_SEARCH_BUDGET_MB", "1")
    hb = ops.search(t, t0, f, 20, 1, precision="f64").cpu().numpy()
    assert np.isfinite(h).all() and int(np.argmax(h)) == 1500
    np.testing.assert_array_equal(hb, h)


def test_fixup_trial_blocks(gpu, photons, monkeypatch):
    """H_20 over a 2048-trial progression by the exact kernel with CRIMP_FIXUP_REL=1e-30: no trial's error bound is
    within 1e-30 of its power, so all 2048 go through the fp64 fix-up (9 photon splits of 4445). The 1 MiB budget
    holds 364 trials' partial sums: 6 fix-up blocks (5 x 364 + 228) where the default budget takes one. Every
    trial then holds fp64 sums: equal to the fp64 path's up to the rounding of differently split sums (1e-12 relative,
    the bound tests/test_gpu_fullsize.py::test_trial_blocks_and_fixup holds fixed trials to; measured 6.8e-13)."""
    from crimp_amd import ops, _native as N
    t, t0 = photons
    f = _grid(gpu, 2048)
    monkeypatch.delenv("CRIMP_SEARCH_BUDGET_MB", raising=False)
    monkeypatch.setenv("CRIMP_FIXUP_REL", "1e-30")
    h = ops.search(t, t0, f, 20, 1, precision="exact").cpu().numpy()
    assert N.load().crimp_last_search_path() == 1
    assert N.load().crimp_last_fixups() == 2048
    monkeypatch.setenv("CRIMP_SEARCH_BUDGET_MB", "1")
    hb = ops.search(t, t0, f, 20, 1, precision="exact").cpu().numpy()
    assert N.load().crimp_last_fixups() == 2048
    np.testing.assert_array_equal(hb, h)
    h64 = ops.search(t, t0, f, 20, 1, precision="f64").cpu().numpy()
    rel = np.abs(h - h64) / np.abs(h64)
    print("fix-up vs fp64 path: max rel %.3e" % rel.max())
    assert rel.max() <= 1e-12
