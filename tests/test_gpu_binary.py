"""Binary orbits on the device: crimp_binary_delay (k_binary_delay) and crimp_calcphase with parts bit 3
(k_calcphase_vec<true>, k_calcphase_scalar<true>: bin_delay of csrc/binary_delay.h, then cp_one at the emission time)
against the 60-digit fixture tests/golden/calcphase_binary.npz; the fused users (k_phase_cube, k_sim_cells); the limits
of the C-ABI.

Every comparison is per element |x - mp| <= factor u A(t) with the derived factors and units of
tests/binary_reference.py (16 for the delay, 32 for the phase and its parts); the tests print the largest
|x - mp| / (u A) per model and route. Which of the pair and the scalar kernel ran follows crimp_calcphase's routing
rule (three 16-byte aligned pointers and an even n: pair), as in tests/test_gpu_calcphase.py.

On a build without binary orbits the fixture comparison fails (the orbital keys are ignored) and so does the symbol
test."""
import ctypes

import numpy as np
import pytest

import binary_reference as B
import phase_reference as R
from conftest import gpath

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 255, 256, 257, 511, 512, 513)
SENTINEL = -7.25


@pytest.fixture(scope="module")
def fixture():
    return B.load_binary()


@pytest.fixture(scope="module")
def wide():
    return R.load_wide()


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _check(m, got, row, sl, what):
    r = m.ratio(_host(got), row, sl)
    print("kernel %-13s %-28s max |err|/(u A) = %.2f" % (m.name, what, r))
    assert r <= m.factor(row), (m.name, what, r)
    return r


def test_library_exports_crimp_binary_delay(gpu):
    from crimp_amd import _native as N
    assert hasattr(N.load(), "crimp_binary_delay")
    assert "crimp_binary_delay" in N.EXPORTS


# ------------------------------------------------------------------------------------------- precision
@pytest.mark.parametrize("name", B.MODELS)
def test_delay_total_and_parts_both_kernels(gpu, fixture, name):
    """Host arrays: an even one takes the pair kernel, an odd one the scalar kernel. No element of any model is NaN
    (no lane reaches the iteration cap)."""
    from crimp_amd import ops
    from crimp_amd.binarymodels import binary_delay, emission_times
    from crimp_amd.calcphase import Phases, calcphase
    m = fixture[name]
    n = m.t.size
    assert n % 2 == 0
    print()
    tau = binary_delay(m.t, m.tm)
    assert not np.any(np.isnan(tau))
    _check(m, tau, "tau", slice(None), "crimp_binary_delay")
    _check(m, binary_delay(m.t[1:], m.tm), "tau", slice(1, None), "crimp_binary_delay odd")
    np.testing.assert_array_equal(Phases(m.t, m.tm).binarydelay(), tau)
    np.testing.assert_array_equal(emission_times(m.t, m.tm), m.t - tau / 86400.0)
    np.testing.assert_array_equal(emission_times(m.t, m.tm, unit="s"), (m.t - float(m.tm["PEPOCH"])) * 86400.0 - tau)
    tot, fol = calcphase(m.t, m.tm)                                   # even: k_calcphase_vec<true>
    assert not np.any(np.isnan(tot))
    _check(m, tot, "total", slice(None), "vec total")
    np.testing.assert_array_equal(fol, tot - np.floor(tot))
    tot1, fol1 = calcphase(m.t[1:], m.tm)                             # odd: k_calcphase_scalar<true>
    _check(m, tot1, "total", slice(1, None), "scalar total")
    np.testing.assert_array_equal(fol1, tot1 - np.floor(tot1))
    ph, ph1 = Phases(m.t, m.tm), Phases(m.t[1:], m.tm)
    for part, fn in (("te", "taylorexpansion"), ("gl", "glitches"), ("wv", "waves")):
        mask = B.PART_MASK[part]
        _check(m, ops.calcphase(m.t, m.tm, parts=mask)[0], part, slice(None), "vec parts=%d|8" % mask)
        _check(m, ops.calcphase(m.t[1:], m.tm, parts=mask)[0], part, slice(1, None), "scalar parts=%d|8" % mask)
        _check(m, np.broadcast_to(getattr(ph, fn)(), (n,)), part, slice(None), "vec Phases.%s" % fn)
        _check(m, np.broadcast_to(getattr(ph1, fn)(), (n - 1,)), part, slice(1, None), "scalar Phases.%s" % fn)


def test_parts_without_bit3_ignore_the_orbit(gpu, fixture):
    """parts = 7 through the C-ABI means what it meant: the arrival-time phase, whatever the model's tail holds."""
    from crimp_amd import ops, _native as N
    m = fixture["binary_all"]
    L = N.load()
    t = np.ascontiguousarray(m.t)
    plain = {k: v for k, v in m.tm.items() if k not in B.orbit_keys()}
    want = ops.calcphase(t, plain)[0]
    got = np.empty_like(t)
    model = ops._modeltm(m.tm)
    assert model.binary == N.BINARY_BT
    assert L.crimp_calcphase(ctypes.c_void_p(t.ctypes.data), t.size, ctypes.byref(model), 7,
                             ctypes.c_void_p(got.ctypes.data), None, 0, None) == 0
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(ops.calcphase(t, m.tm)[0], want)


@pytest.mark.parametrize("name", ("binary_all", "bt_e095"))
def test_sizes_around_one_pair_and_block_edges(gpu, fixture, name):
    """Prefixes of 1..513 times as host arrays (pair kernel when even, scalar when odd) and through a misaligned device
    view (scalar at every n), outputs inside larger sentinel-filled buffers; the same for crimp_binary_delay."""
    import torch
    from crimp_amd import ops
    m = fixture[name]
    dt = torch.as_tensor(m.t, device=gpu)
    worst = worst_tau = 0.0
    for n in SIZES:
        tot, fol = ops.calcphase(m.t[:n], m.tm)
        assert tot.shape == fol.shape == (n,)
        worst = max(worst, m.ratio(tot, "total", slice(0, n)))
        np.testing.assert_array_equal(fol, tot - np.floor(tot))
        worst_tau = max(worst_tau, m.ratio(ops.binary_delay(m.t[:n], m.tm)[0], "tau", slice(0, n)))
        for off in (2, 1):
            tin = dt[:n] if off == 2 else dt[1:1 + n]
            sl = slice(0, n) if off == 2 else slice(1, 1 + n)
            bufs = [torch.full((n + 4,), SENTINEL, dtype=torch.float64, device=gpu) for _ in range(4)]
            assert (bufs[0][off:].data_ptr() % 16 == 0) == (off == 2) and (tin.data_ptr() % 16 == 0) == (off == 2)
            ops.calcphase(tin, m.tm, total=bufs[0][off:off + n], folded=bufs[1][off:off + n])
            ops.binary_delay(tin, m.tm, delay=bufs[2][off:off + n], t_emit=bufs[3][off:off + n])
            ht, hf, hd, he = (b.cpu().numpy() for b in bufs)
            for h in (ht, hf, hd, he):
                assert np.all(h[:off] == SENTINEL) and np.all(h[off + n:] == SENTINEL), (n, off)
            worst = max(worst, m.ratio(ht[off:off + n], "total", sl))
            worst_tau = max(worst_tau, m.ratio(hd[off:off + n], "tau", sl))
            np.testing.assert_array_equal(hf[off:off + n], ht[off:off + n] - np.floor(ht[off:off + n]))
            np.testing.assert_array_equal(he[off:off + n], m.t[sl] - hd[off:off + n] / 86400.0)
    print("\nkernel %-13s sizes %s: max |err|/(u A) = %.2f (total), %.2f (tau)" % (name, SIZES, worst, worst_tau))
    assert worst <= B.FACTOR and worst_tau <= B.FACTOR_TAU


def test_empty_input_touches_nothing(gpu, fixture):
    import torch
    from crimp_amd import ops
    m = fixture["bt_e07"]
    tot, fol = ops.calcphase(np.empty(0), m.tm)
    assert tot.shape == fol.shape == (0,)
    d, e = ops.binary_delay(np.empty(0), m.tm, want_emit=True)
    assert d.shape == e.shape == (0,) and d.dtype == np.float64
    buf = torch.full((8,), SENTINEL, dtype=torch.float64, device=gpu)
    ops.binary_delay(torch.as_tensor(m.t, device=gpu)[:0], m.tm, delay=buf[2:2], t_emit=buf[4:4])
    assert bool(torch.all(buf == SENTINEL))


@pytest.mark.parametrize("name", ("bt_e07", "ell1_amxp", "binary_all"))
def test_device_tensors_three_routes(gpu, fixture, name):
    import torch
    from crimp_amd import ops
    m = fixture[name]
    n = m.t.size
    d = torch.as_tensor(m.t, device=gpu)
    print()
    for what, view, sl in (("device aligned even", d, slice(None)), ("device misaligned even", d[1:n - 1], slice(1, n - 1)),
                           ("device odd", d[:n - 1], slice(0, n - 1))):
        tot, fol = ops.calcphase(view, m.tm)
        assert tot.is_cuda and fol.is_cuda and tot.shape == view.shape
        _check(m, tot, "total", sl, what)
        ht = _host(tot)
        np.testing.assert_array_equal(_host(fol), ht - np.floor(ht))
        tau, emit = ops.binary_delay(view, m.tm, want_emit=True)
        assert tau.is_cuda and emit.is_cuda
        _check(m, tau, "tau", sl, what + " delay")


def test_short_model_meets_the_1e9_cycle_contract(gpu, fixture):
    from crimp_amd.calcphase import calcphase
    m = fixture["binary_short"]
    assert np.max(np.abs(m.hi["total"])) < 2e5 and B.FACTOR * B.U * np.max(m.A["total"]) < 1e-9
    mp_fold = (m.hi["total"] - np.floor(m.hi["total"])) + m.lo["total"]
    for t, sl in ((m.t, slice(None)), (m.t[1:], slice(1, None))):
        tot, fol = calcphase(t, m.tm)
        assert np.max(m.err(tot, "total", sl)) <= 1e-9
        d = np.abs(fol - mp_fold[sl])
        assert np.max(np.minimum(d, 1 - d)) <= 1e-9
        assert np.all((fol >= 0) & (fol <= 1))


@pytest.mark.parametrize("name", B.MODELS)
def test_fold_is_total_minus_floor_bit_for_bit(gpu, fixture, name):
    from crimp_amd import ops, _native as N
    m = fixture[name]
    for t in (m.t, m.t[1:]):
        tot, fol = ops.calcphase(t, m.tm)
        np.testing.assert_array_equal(fol, tot - np.floor(tot))
        assert np.all((fol >= 0) & (fol <= 1))
        tot2, rad = ops.calcphase(t, m.tm, flags=N.FLAG_FOLD_RADIANS)
        np.testing.assert_array_equal(tot2, tot)
        np.testing.assert_array_equal(rad, (tot - np.floor(tot)) * (2 * np.pi))


@pytest.mark.parametrize("name", ("bt_e07", "ell1_amxp", "binary_all"))
def test_nan_time_gives_nan_there_only(gpu, fixture, name):
    from crimp_amd import ops
    m = fixture[name]
    for t in (m.t, m.t[1:]):
        clean = ops.calcphase(t, m.tm)
        clean_tau = ops.binary_delay(t, m.tm, want_emit=True)
        for i in (0, 1, 300, 301, t.size - 1):
            tn = t.copy()
            tn[i] = np.nan
            keep = np.arange(t.size) != i
            tot, fol = ops.calcphase(tn, m.tm)
            assert np.isnan(tot[i]) and np.isnan(fol[i])
            np.testing.assert_array_equal(tot[keep], clean[0][keep])
            np.testing.assert_array_equal(fol[keep], clean[1][keep])
            tau, emit = ops.binary_delay(tn, m.tm, want_emit=True)
            assert np.isnan(tau[i]) and np.isnan(emit[i])
            np.testing.assert_array_equal(tau[keep], clean_tau[0][keep])
            np.testing.assert_array_equal(emit[keep], clean_tau[1][keep])


@pytest.mark.parametrize("name", ("all", "short"))
def test_unchanged_without_binary(gpu, wide, name):
    """A zero-tailed struct: parts 7 | 8 gives the bits of parts 7, on the pair and the scalar kernel."""
    from crimp_amd import ops, _native as N
    m = wide[name]
    assert ops._modeltm(m.tm).binary == N.BINARY_NONE
    for t in (m.t, m.t[1:]):
        a = ops.calcphase(t, m.tm, parts=7)
        b = ops.calcphase(t, m.tm, parts=7 | N.PART_EMISSION)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        assert m.ratio(b[0], "total", slice(m.t.size - t.size, None)) <= R.FACTOR


# ------------------------------------------------------------------------------------------- fused users
@pytest.mark.parametrize("where", ["host", "device"])
def test_fused_map_equals_calcphase_then_unfused(gpu, fixture, where):
    """The fused phase-time map of a binary model (the MAP form with Y_IS_X, the general form with a z axis; pair
    loads, and scalar loads through a misaligned view) counts exactly what calcphase followed by the unfused call
    counts."""
    import torch
    from crimp_amd import _native as N
    from crimp_amd import ops
    from crimp_amd.calcphase import calcphase
    m = fixture["binary_all"]
    rng = np.random.default_rng(5)
    t = np.sort(np.concatenate([m.t, rng.uniform(m.t.min(), m.t.max(), 20001 - m.t.size)]))   # odd: the pair tail
    z = rng.uniform(0.0, 1.0, t.size)
    te = np.linspace(t.min(), t.max(), 13)
    ze = np.array([0.0, 0.2, 0.7, 1.0])
    if where == "device":
        t, z = torch.as_tensor(t, device=gpu), torch.as_tensor(z, device=gpu)

    def host(c):
        return c.cpu().numpy() if where == "device" else c
    plain = {k: v for k, v in m.tm.items() if k not in B.orbit_keys()}
    for tt, zz in ((t, z), (t[1:], z[1:])):
        folded = calcphase(tt, m.tm)[1]
        a = host(ops.phase_cube(tt, model=m.tm, y_edges=te, nph=32, options=N.CUBE_Y_IS_X))
        b = host(ops.phase_cube(folded, y=tt, y_edges=te, nph=32))
        assert a.sum() == len(tt)
        np.testing.assert_array_equal(a, b)
        assert not np.array_equal(a, host(ops.phase_cube(tt, model=plain, y_edges=te, nph=32, options=N.CUBE_Y_IS_X)))
        a = host(ops.phase_cube(tt, model=m.tm, y=tt, y_edges=te, z=zz, z_edges=ze, nph=16))
        b = host(ops.phase_cube(folded, y=tt, y_edges=te, z=zz, z_edges=ze, nph=16))
        np.testing.assert_array_equal(a, b)


def _sim_model():
    """1e2259.par on bt_e07's orbit scaled to three orbits over the 11720 s that 2e5 events at 17.06 counts/s take:
    A1 F0 ~ 1 cycle, so the raw times are smeared over the whole pulse."""
    from crimp_amd.readtimingmodel import ReadTimingModel
    tm = ReadTimingModel(gpath("1e2259.par")).readfulltimingmodel()[0]
    span = 11720.0
    tm.update({"BINARY": "BT", "PB": span / 3.0 / 86400.0, "A1": 7.0, "ECC": 0.7, "OM": 200.0, "T0": 58400.0 - 0.01})
    return tm, 58400.0, span


def _harmonic_powers(sec, f, nh):
    ph = 2 * np.pi * np.outer(np.arange(1, nh + 1), f * sec)
    return (2.0 / sec.size) * (np.cos(ph).sum(axis=1) ** 2 + np.sin(ph).sum(axis=1) ** 2)


def test_simulated_events_follow_the_emission_phase(gpu):
    """2e5 events drawn under the orbit. Z^2_2 at the spin frequency on emission_times(...) against the raw arrival
    times: harmonic k of the raw times is the emission-time harmonic times s_k = <exp(2 pi i k f tau(t))>, the
    smearing of the orbit, computed here from the model on a uniform grid of the span (host fp64). The raw Z^2_2 has
    to sit in the 5 sigma band of a non-central chi^2_4 around sum_k (P_k - 2) |s_k|^2 + 4, and the predicted factor is
    large (the orbit destroys the raw signal). Repeats and shards are bit-identical."""
    from crimp_amd.binarymodels import binary_delay_host, emission_times
    from crimp_amd.ephemTmjd import ephemTmjd
    from crimp_amd.periodsearch import PeriodSearch
    from crimp_amd.simulatemodulatedlc import simulate_events
    tm, mjd0, span = _sim_model()
    tstop = mjd0 + span / 86400.0
    r = simulate_events(tm, gpath("1e2259_template.txt"), mjd0, tstop, seed=11)
    t = r["time"]
    assert 1.9e5 < t.size < 2.1e5 and np.all(np.diff(t) >= 0)
    r2 = simulate_events(tm, gpath("1e2259_template.txt"), mjd0, tstop, seed=11)
    assert np.array_equal(r2["time"], t) and np.array_equal(r2["is_bgr"], r["is_bgr"])
    nc = r["n_cells"]
    cuts = [0, 1, nc // 2, nc - 1, nc]
    parts = [simulate_events(tm, gpath("1e2259_template.txt"), mjd0, tstop, seed=11, first_cell=a, n_cells=b - a)["time"]
             for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts), t)
    plain = {k: v for k, v in tm.items() if k not in B.orbit_keys()}
    assert not np.array_equal(simulate_events(plain, gpath("1e2259_template.txt"), mjd0, tstop, seed=11)["time"], t)

    mid = mjd0 + 0.5 * span / 86400.0
    f = float(np.atleast_1d(ephemTmjd(mid - binary_delay_host(mid, tm) / 86400.0, tm)["freqAtTmjd"])[0])
    emit = emission_times(t, tm, unit="s")
    raw = (t - float(tm["PEPOCH"])) * 86400.0
    pe, pr = _harmonic_powers(emit, f, 2), _harmonic_powers(raw, f, 2)
    grid = mjd0 + np.linspace(0.0, span, 20001)[:-1] / 86400.0
    tau = binary_delay_host(grid, tm)
    s2 = np.array([abs(np.mean(np.exp(2j * np.pi * k * f * tau))) ** 2 for k in (1, 2)])
    lam = float(np.sum(np.maximum(pe - 2.0, 0.0) * s2))
    band = 5.0 * np.sqrt(2.0 * (4.0 + 2.0 * lam))
    factor = pe.sum() / (lam + 4.0)
    print("\nZ2_2 emission %.1f raw %.1f; |s_k|^2 = %s; predicted raw %.1f +- %.1f, factor %.1f (measured %.1f)" %
          (pe.sum(), pr.sum(), np.round(s2, 5), lam + 4.0, band, factor, pe.sum() / pr.sum()))
    assert factor > 10.0
    assert abs(pr.sum() - (lam + 4.0)) <= band
    assert pe.sum() >= pr.sum() * pe.sum() / (lam + 4.0 + band)
    # the array a user hands to PeriodSearch: the peak of a grid around f is the emission-time power
    fr = f + np.arange(-40, 41) / (20.0 * span)
    z = PeriodSearch(emit, fr, 2).ztest()
    assert abs(z[40] - pe.sum()) <= 1e-6 * pe.sum() and abs(int(np.argmax(z)) - 40) <= 2


def test_measure_intervals_on_a_binary_model_recovers_zero_shift(gpu):
    """The 8 x 1100 s intervals of the injection-recovery test on the events simulated under the orbit, no injected shift: measure_intervals (fold at the emission time) returns
    phase shifts consistent with 0 by the injection-recovery test's own criterion (5 sigma each, pulls of RMS < 2), and
    the H power is the H-test of the emission times at the emission-time spin frequency of ToA_mid."""
    import sim_reference as S
    from crimp_amd.binarymodels import binary_delay_host, emission_times
    from crimp_amd.ephemTmjd import ephemTmjd
    from crimp_amd.measureToAs import measure_intervals
    from crimp_amd.simulatemodulatedlc import simulate_events
    tm, mjd0, span = _sim_model()
    t = simulate_events(tm, gpath("1e2259_template.txt"), mjd0, mjd0 + span / 86400.0, seed=12)["time"]
    starts = mjd0 + np.arange(8) * 1100.0 / 86400.0
    ends = starts + 1100.0 / 86400.0
    res = measure_intervals(t, tm, gpath("1e2259_template.txt"), starts, ends, np.full(8, 1100.0), brutemin=True)
    S.check_recovery(res["phShi"], res["phShi_LL"], res["phShi_UL"], np.zeros(8))
    emit = emission_times(t, tm, unit="s")
    for i in range(8):
        sel = (t >= starts[i]) & (t <= ends[i])
        mid = res["ToA_mid"][i]
        assert mid == (t[sel][-1] - t[sel][0]) / 2 + t[sel][0]            # an arrival time, as without an orbit
        f = float(np.atleast_1d(ephemTmjd(mid - binary_delay_host(mid, tm) / 86400.0, tm)["freqAtTmjd"])[0])
        z = np.cumsum(_harmonic_powers(emit[sel], f, 5))
        h = np.max(z - 4.0 * np.arange(1, 6) + 4.0)
        assert abs(res["htestPow"][i] - h) <= 1e-6 * h, (i, res["htestPow"][i], h)


# ------------------------------------------------------------------------------------------- C-ABI limits
def test_capi_limits(gpu, fixture):
    from crimp_amd import ops, _native as N
    L = N.load()
    m = fixture["bt_e07"]
    t = np.ascontiguousarray(m.t[:8])
    tot, fol, dly, emi = (np.empty(8) for _ in range(4))

    def phase(model, n=8):
        return L.crimp_calcphase(ctypes.c_void_p(t.ctypes.data), n, ctypes.byref(model), 7 | N.PART_EMISSION,
                                 ctypes.c_void_p(tot.ctypes.data), ctypes.c_void_p(fol.ctypes.data), 0, None)

    def delay(model, n=8):
        return L.crimp_binary_delay(ctypes.c_void_p(t.ctypes.data), n, ctypes.byref(model),
                                    ctypes.c_void_p(dly.ctypes.data), ctypes.c_void_p(emi.ctypes.data), 0, None)

    base = ops._modeltm(m.tm)
    limit = 0.5 * base.bin_pb * 86400.0 * (1.0 - base.bin_ecc) / (2 * np.pi)
    cases = (("bin_ecc", 1.0, "ECC must be in [0, 1)"), ("bin_ecc", -0.01, "ECC must be in [0, 1)"),
             ("bin_pb", 0.0, "PB must be positive"), ("bin_a1", -1.0, "A1 must be >= 0"),
             ("bin_a1", limit * 1.001, "2 pi A1 / (PB (1 - e)) must be below 1/2"),
             ("binary", 3, "binary must be CRIMP_BINARY_NONE, CRIMP_BINARY_BT or CRIMP_BINARY_ELL1"),
             ("bin_gamma", float("nan"), "a binary parameter is not finite"))
    for call, outs in ((phase, (tot, fol)), (delay, (dly, emi))):
        for field, value, msg in cases:
            bad = N.TimingModel.from_buffer_copy(base)
            setattr(bad, field, value)
            for o in outs:
                o[:] = SENTINEL
            assert call(bad) == -1 and L.crimp_last_error().decode() == msg, (field, value)
            assert all(np.all(o == SENTINEL) for o in outs)
        assert call(base, n=-1) == -1 and L.crimp_last_error().decode() == "n < 0"
    none = N.TimingModel.from_buffer_copy(base)
    none.binary = N.BINARY_NONE
    dly[:] = SENTINEL
    assert delay(none) == -1 and L.crimp_last_error().decode() == "the model has no binary" and np.all(dly == SENTINEL)
    # the limits themselves pass and compute: just inside the contraction limit, and the fixture's own model
    ok = N.TimingModel.from_buffer_copy(base)
    ok.bin_a1 = limit * 0.998
    assert delay(ok) == 0 and not np.any(np.isnan(dly))
    assert phase(base) == 0 and delay(base) == 0
    assert m.ratio(tot, "total", slice(0, 8)) <= B.FACTOR and m.ratio(dly, "tau", slice(0, 8)) <= B.FACTOR_TAU
    # the fused users refuse the same models with the same text, and the fits refuse every orbit
    bad = N.TimingModel.from_buffer_copy(base)
    bad.bin_pb = 0.0
    with pytest.raises(N.CrimpNativeError, match="PB must be positive"):
        ops.sim_events(bad, ops.make_sim_shape(steps=np.ones(4), lam_max=2.0), 58000.0, 10.0, 1.0)
    with pytest.raises(ValueError, match="binary models are not fitted yet"):
        ops.timing_nll(t, np.zeros(8), np.ones(8), base, base, ops.fit_map(["F0"]), np.zeros((1, 1)))
