"""Device event simulator (crimp_sim_events, csrc/sim_events.h) on the MI355X: determinism and independence of the
launch, structure of the output, Poisson statistics, pulse shapes under timing models, the simulatemodulatedlc
drop-in against the fixture recorded from the reference, and injection-recovery through measure_intervals. The
statistical bounds are those of tests/sim_reference.py (quantiles; the NumPy restatement meets them on the CPU in
tests/test_simulate_host.py); seeds are fixed, so the outcomes are deterministic."""
import ctypes

import numpy as np
import pytest

import sim_reference as R
from conftest import GOLDEN, gold, gpath

pytestmark = pytest.mark.gpu

LAM, CELL = 40.0, 4.8  # a flat 40 counts/s: lam_max * cell = 192


def flat_shape(rate=LAM, lam_max=None, bkg=0.0):
    from crimp_amd import ops
    return ops.make_sim_shape(steps=[rate], bkg=bkg, lam_max=(rate + bkg) if lam_max is None else lam_max)


def sim(shape, span, cell=CELL, tm=R.FLAT_MODEL, **kw):
    from crimp_amd import ops
    return ops.sim_events(tm, shape, R.MJD0, span, cell, **kw)


def pulsed_shape():
    from crimp_amd.simulatemodulatedlc import build_shape
    return build_shape(R.FOURIER1, phShift=0.4, bgrrate=2.0)


def test_same_seed_same_events_and_launch_independence(gpu):
    import torch
    from crimp_amd.simulatemodulatedlc import cell_count, cell_length
    shape, lam = pulsed_shape()
    cell = cell_length(lam)
    span = 20.3 * cell
    nc = cell_count(span, cell)
    assert nc == 21
    t, b, n = sim(shape, span, cell, seed=5)
    t2, b2, n2 = sim(shape, span, cell, seed=5)
    assert n == n2 == t.size == b.size and n > 1000
    assert np.array_equal(t, t2) and np.array_equal(b, b2)
    assert sim(shape, span, cell, seed=5, count_only=True) == (None, None, n)
    td, bd, nd = sim(shape, span, cell, seed=5, device=True)
    assert td.is_cuda and bd.dtype == torch.uint8 and nd == n
    assert np.array_equal(td.cpu().numpy(), t) and np.array_equal(bd.cpu().numpy(), b)
    # shards cut after cell 0, in the middle and before the last cell
    for cuts in ([0, 1, nc], [0, 10, nc], [0, nc - 1, nc], [0, 1, 10, nc - 1, nc]):
        parts = [sim(shape, span, cell, seed=5, first_cell=a, n_cells=c - a) for a, c in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), t), cuts
        assert np.array_equal(np.concatenate([p[1] for p in parts]), b), cuts
        assert sum(p[2] for p in parts) == n
    assert sim(shape, span, cell, seed=5, first_cell=nc, n_cells=-1)[2] == 0
    # cells draw from their own counter streams
    c0 = t[t < cell]
    c1 = t[(t >= cell) & (t < 2 * cell)] - cell
    assert c0.size > 20 and c1.size > 20 and not np.array_equal(c0[:20], c1[:20])
    assert np.intersect1d(np.round(c0, 9), np.round(c1, 9)).size == 0
    t3, _, _ = sim(shape, span, cell, seed=6)
    assert not np.array_equal(t3[:50], t[:50])
    # MJD and seconds outputs correspond exactly; an offset is added to the seconds
    mjd, bm, _ = sim(shape, span, cell, seed=5, days=True)
    assert np.array_equal(mjd, R.MJD0 + t / 86400.0) and np.array_equal(bm, b)
    to, _, _ = sim(shape, span, cell, seed=5, out_offset_s=5.0e9)
    assert np.array_equal(to, 5.0e9 + t)
    assert sim(shape, span, cell, seed=5, want_bkg=False)[1] is None
    # a caller's estimate of the count: enough (one native call) or not (counted, then filled) -- the same events
    for cap in (n + 100, n, 10):
        tc, bc, nc_ = sim(shape, span, cell, seed=5, cap=cap)
        assert nc_ == n and np.array_equal(tc, t) and np.array_equal(bc, b)


@pytest.mark.parametrize("cells,extra,cell", [(0, 0.5, CELL), (2, 0.0, CELL), (256, 0.3, CELL), (70000, 0.0, 0.5)])
def test_structure_across_cell_counts(gpu, cells, extra, cell):
    """Spans of less than one cell, an exact multiple, a multiple plus a sliver; 1, 2, 257 and 70 000 cells (past
    65 535 blocks and past one level of the offset scan)."""
    from crimp_amd.simulatemodulatedlc import cell_count
    span = float(cells) * cell + extra * cell
    nc = cell_count(span, cell)
    assert nc == cells + (1 if extra else 0)
    t, b, n = sim(flat_shape(), span, cell, seed=cells + 1)
    assert n == t.size and np.all(np.diff(t) >= 0.0) and t.min() >= 0.0 and t.max() < span
    assert not b.any()
    R.check_counts(n, LAM * span)
    # every cell holds its own events: the counts per cell are Poisson too
    if nc > 2:
        per = np.histogram(t, bins=np.append(np.arange(nc) * cell, span))[0]
        assert per.sum() == n
        R.check_counts(int(per[:nc // 2].sum()), LAM * cell * (nc // 2))
    mjd, _, _ = sim(flat_shape(), span, cell, seed=cells + 1, days=True)
    assert np.all(np.diff(mjd) >= 0.0) and mjd.max() <= R.MJD0 + span / 86400.0


def test_zero_rate_and_background_only(gpu):
    t, b, n = sim(flat_shape(0.0, lam_max=10.0), 500.0, 19.2, seed=1)
    assert n == 0 and t.size == 0 and b.size == 0
    t, b, n = sim(flat_shape(0.0, lam_max=10.0, bkg=10.0), 500.0, 19.2, seed=1)
    R.check_counts(n, 5000.0)
    assert b.all()


def test_gtis(gpu):
    gti, span, lam = R.gti_case()
    mjd, _, n = sim(flat_shape(), span, seed=3, gti=gti, days=True)
    R.check_gti_draw(mjd, gti, span, lam)
    s, _, _ = sim(flat_shape(), span, seed=3, gti=gti)
    assert np.array_equal(mjd, R.MJD0 + s / 86400.0)
    # the events inside the GTIs are those of the run without GTIs (a GTI only removes candidates)
    full, _, _ = sim(flat_shape(), span, seed=3, days=True)
    assert np.array_equal(full[R.in_gti(full, gti)], mjd)
    from crimp_amd import ops
    assert ops.sim_events(R.FLAT_MODEL, flat_shape(), R.MJD0, span, CELL, gti=np.zeros((0, 2)))[2] == 0


@pytest.mark.parametrize("per_cell", [20.0, 400.0])
def test_one_round_and_many_rounds_per_cell(gpu, per_cell):
    cell = per_cell / LAM
    span = 4000.0 + 0.37 * cell
    t, _, n = sim(flat_shape(), span, cell, seed=8)
    assert np.all(np.diff(t) >= 0.0) and t.max() < span
    R.check_counts(n, LAM * span)
    R.check_dispersion(t, span, 1021)


def test_cap_too_small_writes_nothing(gpu):
    from crimp_amd import _native as N, ops
    L = N.load()
    shape = flat_shape()
    m = ops._modeltm(R.FLAT_MODEL)
    n = ctypes.c_int64(0)

    def call(t, b, cap):
        return L.crimp_sim_events(ctypes.byref(m), ctypes.byref(shape), R.MJD0, 100.0, CELL, None, 0, 4, 0, -1,
                                  None if t is None else t.ctypes.data, None if b is None else b.ctypes.data, cap,
                                  ctypes.byref(n), 0.0, 0, None)
    assert call(None, None, 0) == 0
    total = n.value
    assert total > 3000
    t = np.full(total + 8, -7.0)
    b = np.full(total + 8, 9, dtype=np.uint8)
    assert call(t, b, total - 1) == -1 and n.value == total
    assert b"cap" in L.crimp_last_error()
    assert np.all(t == -7.0) and np.all(b == 9)
    assert call(t, b, total) == 0
    assert np.all(t[:total] >= 0.0) and np.all(t[total:] == -7.0) and np.all(b[total:] == 9) and not b[:total].any()


def test_argument_errors(gpu):
    from crimp_amd import ops
    from crimp_amd._native import CrimpNativeError
    ok = dict(span=100.0, cell=CELL)

    def bad(shape=None, **kw):
        a = dict(ok, **kw)
        with pytest.raises(CrimpNativeError):
            sim(flat_shape() if shape is None else shape, a.pop("span"), a.pop("cell"), **a)
    bad(span=0.0)
    bad(span=-5.0)
    bad(span=float("inf"))
    for v in (0.0, -1.0, float("nan"), float("inf")):
        bad(cell=v)
        bad(shape=flat_shape(1.0, lam_max=v))
    bad(cell=1.0e6)  # lam_max * cell_s > 65536
    bad(gti=[[R.MJD0 + 0.002, R.MJD0 + 0.003], [R.MJD0, R.MJD0 + 0.001]])       # unsorted
    bad(gti=[[R.MJD0, R.MJD0 + 0.002], [R.MJD0 + 0.001, R.MJD0 + 0.003]])       # overlapping
    bad(gti=[[R.MJD0 + 0.001, R.MJD0]])                                           # reversed
    bad(shape=ops.make_sim_shape(steps=np.zeros(0), lam_max=1.0))                 # n_steps < 1
    bad(first_cell=22)            # 21 cells
    bad(first_cell=-1)
    bad(first_cell=20, n_cells=2)
    bad(span=1.0e10, cell=1.0, shape=flat_shape(1.0))  # 1e10 cells
    assert sim(flat_shape(), 100.0, CELL, first_cell=21)[2] == 0  # the empty range at the end is allowed


def test_poisson_statistics_of_a_flat_rate(gpu):
    """~4e5 events: the count, the index of dispersion in 4096 bins (which do not divide the cells) and in the cells'
    own bins, and exactly repeated times on the MJD grid (0.63 us at MJD 58400: ~5 expected, P(>= 20) < 1e-6)."""
    span = float(2083) * CELL
    t, _, n = sim(flat_shape(), span, seed=12)
    R.check_counts(n, LAM * span)
    R.check_dispersion(t, span, 4096)
    per = np.histogram(t, bins=np.append(np.arange(2083) * CELL, span))[0]
    d = float(np.var(per, ddof=1) / np.mean(per))
    print("dispersion over the cells", d)
    assert abs(d - 1.0) <= 5.0 * np.sqrt(2.0 / 2082)
    mjd, _, _ = sim(flat_shape(), span, seed=12, days=True)
    assert np.sum(np.diff(mjd) == 0.0) < 20


@pytest.fixture(scope="module")
def cases():
    return R.shape_cases(GOLDEN)


@pytest.mark.parametrize("name", ["fourier1_0", "fourier1_1", "fourier6_par_0", "fourier6_par_1", "cauchy", "vonmises",
                                  "steps_4", "steps_95", "steps_20000", "glitch"])
def test_shapes_under_timing_models(gpu, cases, name):
    """~2e5 events folded with crimp_amd.calcphase: the 32-bin counts against the profile's exact bin integrals, the
    count and the background fraction (for the glitch model before and after the glitch)."""
    from crimp_amd.calcphase import calcphase
    from crimp_amd.simulatemodulatedlc import simulate_events
    c = cases[name]
    tm = gpath("1e2259.par") if name.startswith("fourier6_par") else c["tm"]
    shape = gpath("1e2259_template.txt") if name.startswith("fourier6_par") else c["shape"]
    tstop = R.MJD0 + c["span_s"] / 86400.0
    r = simulate_events(tm, shape, R.MJD0, tstop, phShift=c["phShift"], bgrrate=c["bkg"], seed=31)
    mjd = r["time"]
    assert np.all(np.diff(mjd) >= 0.0) and mjd.min() >= R.MJD0 and mjd.max() <= tstop
    _, folded = calcphase(mjd, tm)
    R.check_case(c, (mjd - R.MJD0) * 86400.0, r["is_bgr"], np.asarray(folded), name)
    # the seconds form of the same run, and the device-resident form
    rs = simulate_events(tm, shape, R.MJD0, tstop, phShift=c["phShift"], bgrrate=c["bkg"], seed=31, unit="s",
                         offset_s=100.0, device=True)
    assert np.array_equal(R.MJD0 + (rs["time"].cpu().numpy() - 100.0) / 86400.0, mjd)
    assert rs["n_cells"] == r["n_cells"] and rs["cell_s"] == r["cell_s"]


def test_simulatemodulatedlc_against_the_reference_fixture(gpu, capsys):
    from crimp.simulatemodulatedlc import simulatemodulatedlc
    g = gold("simlc_reference.npz")
    r = simulatemodulatedlc(float(g["freq"]), float(g["srcrate"]), float(g["exposure"]), float(g["pulsedfraction"]),
                            float(g["bgrrate"]), nbrPhaseBins=int(g["nbrPhaseBins"]), seed=2)
    assert capsys.readouterr().out == str(g["printed"])
    w, s = r["assigned_t_wBgr"], r["assigned_t_nobgr"]
    for a in (w, s):
        assert np.all(np.diff(a) >= 0.0) and a.min() >= 0.0 and a.max() < 2000.0
    assert np.all(np.isin(s, w))
    R.check_counts(s.size, 40000.0)
    R.check_counts(w.size, 44000.0)
    R.check_counts(int(g["n_nobgr"]), 40000.0)
    R.check_counts(int(g["n_wbgr"]), 44000.0)
    for a, key in ((w, "hist_wbgr"), (s, "hist_nobgr")):
        h = np.histogram((a * 0.5) % 1.0, bins=16, range=(0.0, 1.0))[0]
        R.two_sample_chi2(h, g[key], key)
    np.random.seed(4)
    a = simulatemodulatedlc(0.5, 20, 200, 0.3, 2, nbrPhaseBins=16)
    np.random.seed(4)
    b = simulatemodulatedlc(0.5, 20, 200, 0.3, 2, nbrPhaseBins=16)
    assert np.array_equal(a["assigned_t_wBgr"], b["assigned_t_wBgr"])


def test_injection_recovery_through_measure_intervals(gpu):
    """8 consecutive intervals of ~1.9e4 photons from the bundled model and template, each with its own injected
    phShift: measure_intervals(brutemin=True) returns them within 5 sigma each, pulls of RMS < 2."""
    from crimp_amd.measureToAs import measure_intervals
    from crimp_amd.simulatemodulatedlc import simulate_events
    starts, span, shifts = R.recovery_case()
    ends = starts + span / 86400.0
    times = [simulate_events(gpath("1e2259.par"), gpath("1e2259_template.txt"), a, b, phShift=sh, seed=40 + i)["time"]
             for i, (a, b, sh) in enumerate(zip(starts, ends, shifts))]
    assert all(t.size <= 20000 for t in times)
    res = measure_intervals(np.concatenate(times), gpath("1e2259.par"), gpath("1e2259_template.txt"), starts, ends,
                            np.full(8, span), brutemin=True)
    R.check_recovery(res["phShi"], res["phShi_LL"], res["phShi_UL"], shifts)
