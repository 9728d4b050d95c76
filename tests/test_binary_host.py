"""Binary orbits on the host: the .par reader, the packing of crimp_timing_model, the NumPy fp64 evaluation of the
orbital delay against the 60-digit fixture (tests/binary_reference.py, tests/golden/calcphase_binary.npz), Tempo2's
first-order inverse against the exact implicit solution, and the scalar host paths (ephemIntegerRotation, the .tim
writer). No GPU."""
import ctypes
import json
import logging
import os

import numpy as np
import pytest

import binary_reference as B

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAR = os.path.join(GOLD, "1e2259.par")


@pytest.fixture(scope="module")
def fixture():
    return B.load_binary()


def _par(tmp_path, extra, name="m.par"):
    p = tmp_path / name
    p.write_text(open(PAR).read().rstrip("\n") + "\n" + extra)
    return str(p)


# ------------------------------------------------------------------------------------------- parser
def test_par_without_binary_reads_as_before(tmp_path):
    from crimp_amd.readtimingmodel import ReadTimingModel
    r = ReadTimingModel(PAR)
    assert r.readbinary() == ({}, {}, {})
    ref = json.load(open(os.path.join(GOLD, "parsed.json")))["par"]
    got = r.readfulltimingmodel()[0]
    assert list(got) == list(ref)
    for k in ref:
        assert float(got[k]) == ref[k], k


def test_reader_keys_aliases_and_case(tmp_path):
    from crimp_amd.readtimingmodel import ReadTimingModel
    p = _par(tmp_path, "BINARY bt\nPB 8.3 1 0.001\nA1 20.5 1\nE 0.7\nXDOT 3e-13\nPBDOT 2.5\nT0 57991.7\nOM 200\n"
                       "OMDOT 12\nGAMMA 0.004\n")
    vals, flags, both = ReadTimingModel(p).readbinary()
    assert vals["BINARY"] == "BT" and both["BINARY"] == {"value": "BT", "flag": None}
    assert (vals["PB"], vals["A1"], vals["ECC"], vals["A1DOT"], vals["PBDOT"]) == (8.3, 20.5, 0.7, 3e-13, 2.5)
    assert (flags["PB"], flags["A1"], flags["ECC"]) == (1, 1, 0) and both["PB"] == {"value": 8.3, "flag": 1}
    assert vals["TASC"] == 0 and vals["EPS1"] == 0 and "E" not in vals and "XDOT" not in vals
    full = ReadTimingModel(p).readfulltimingmodel()
    base = ReadTimingModel(PAR).readfulltimingmodel()
    for i in range(3):
        assert {k: v for k, v in full[i].items() if k not in vals} == base[i]
        assert list(full[i])[:len(base[i])] == list(base[i])
    p2 = _par(tmp_path, "BINARY ELL1\nPB 0.0839\nA1 0.0628\nTASC 49610\nEPS1 1e-5\nEPS2 -2e-5\n", "e.par")
    v2 = ReadTimingModel(p2).readbinary()[0]
    assert v2["BINARY"] == "ELL1" and v2["TASC"] == 49610 and v2["EPS2"] == -2e-5


def test_reader_rejects_other_models_and_warns_once(tmp_path, caplog):
    from crimp_amd.readtimingmodel import ReadTimingModel
    with pytest.raises(ValueError, match="BINARY DD is not supported: the supported binary models are BT and ELL1"):
        ReadTimingModel(_par(tmp_path, "BINARY DD\nPB 1\n")).readbinary()
    p = _par(tmp_path, "BINARY BT\nPB 1\nA1 1\nSINI 0.9\nM2 0.3\nEDOT 1e-15\n", "w.par")
    with caplog.at_level(logging.WARNING, logger="crimp_amd.readtimingmodel"):
        ReadTimingModel(p).readbinary()
    msgs = [r.getMessage() for r in caplog.records]
    assert msgs == ["binary model BT: SINI, M2, EDOT ignored (no Shapiro delay, no eccentricity derivatives)"]


def test_patch_par_values_rewrites_a_binary_key(tmp_path):
    from crimp_amd.readtimingmodel import ReadTimingModel, patch_par_values
    p = _par(tmp_path, "BINARY BT\nPB 8.3 1 0.001\nA1 20.5\n")
    out = str(tmp_path / "o.par")
    patch_par_values(p, out, new_values={"BINARY": "BT", "PB": 8.25, "A1": {"value": 21.0, "flag": 0}})
    v = ReadTimingModel(out).readbinary()[0]
    assert v["PB"] == 8.25 and v["A1"] == 21.0 and v["BINARY"] == "BT"
    assert "PB 8.25 1 0.001\n" in open(out).read()


# ------------------------------------------------------------------------------------------- limits, units, packing
def test_unit_convention_and_limits():
    from crimp_amd.binarymodels import binary_params
    base = {"PEPOCH": 58000.0, "F0": 1.0, "BINARY": "BT", "PB": 2.0, "A1": 10.0, "T0": 57990.0, "ECC": 0.1}
    p = binary_params({**base, "PBDOT": 2.5, "A1DOT": 3e-13})
    assert p["pbdot"] == 2.5 * 1e-12 and p["a1dot"] == 3e-13
    p = binary_params({**{k: v for k, v in base.items() if k != "ECC"}, "PBDOT": -4e-11, "XDOT": -70.0, "E": 0.3})
    assert p["pbdot"] == -4e-11 and p["a1dot"] == -70.0 * 1e-12 and p["ecc"] == 0.3
    assert binary_params({"PEPOCH": 1.0, "F0": 1.0}) is None
    assert binary_params({k: {"value": v, "flag": 0} for k, v in base.items()})["pb"] == 2.0
    for change, msg in (({"BINARY": "DDK"}, "BINARY DDK is not supported: the supported binary models are BT and ELL1"),
                        ({"ECC": 1.0}, r"ECC must be in \[0, 1\)"), ({"ECC": -0.1}, r"ECC must be in \[0, 1\)"),
                        ({"PB": 0.0}, "PB must be positive"), ({"A1": -1.0}, "A1 must be >= 0"),
                        ({"A1": 13000.0}, r"2 pi A1 / \(PB \(1 - e\)\) must be below 1/2"),
                        ({"ECC": 0.9995}, r"2 pi A1 / \(PB \(1 - e\)\) must be below 1/2"),
                        ({"PB": float("nan")}, "a binary parameter is not finite")):
        with pytest.raises(ValueError, match=msg):
            binary_params({**base, **change})
    # just inside the contraction limit
    a1 = 0.499 * 2.0 * 86400 * 0.9 / (2 * np.pi)
    assert binary_params({**base, "A1": a1})["a1"] == a1


def test_modeltm_packing_and_zero_tail(fixture):
    from crimp_amd import ops, _native as N
    from crimp_amd.readtimingmodel import ReadTimingModel
    plain = ops._modeltm(ReadTimingModel(PAR).readfulltimingmodel()[0])
    off = N.TimingModel.binary.offset
    raw = bytes(plain)
    assert off == N.TimingModel.wave_ab.offset + N.TimingModel.wave_ab.size
    assert raw[off:] == bytes(len(raw) - off) and plain.binary == N.BINARY_NONE
    assert ctypes.sizeof(N.TimingModel) % 8 == 0
    m = ops._modeltm(fixture["bt_full"].tm)
    o = B.orbit_values(fixture["bt_full"].tm)
    assert m.binary == N.BINARY_BT
    for k in ("pb", "pbdot", "a1", "a1dot", "t0", "ecc", "om", "omdot", "gamma"):
        assert getattr(m, "bin_" + k) == o[k], k
    assert m.bin_pbdot == 2.5e-12 and m.bin_a1dot == 3e-13 and m.bin_om == 350.0
    e = ops._modeltm(fixture["ell1_amxp"].tm)
    assert e.binary == N.BINARY_ELL1 and e.bin_t0 == fixture["ell1_amxp"].tm["TASC"] and e.bin_eps2 == -2e-5
    assert e.bin_ecc == 0.0 and e.bin_om == 0.0
    both = ops._modeltm({k: {"value": v, "flag": 0} for k, v in fixture["bt_e07"].tm.items()})
    assert bytes(both) == bytes(ops._modeltm(fixture["bt_e07"].tm))
    # the non-binary part of the struct is what it was
    nb = {k: v for k, v in fixture["binary_all"].tm.items() if k not in B.orbit_keys()}
    assert bytes(ops._modeltm(fixture["binary_all"].tm))[:off] == bytes(ops._modeltm(nb))[:off]


def test_fits_refuse_binary_models(fixture):
    import pandas as pd
    from crimp_amd import fit_toas, get_local_ephem, ops
    tm = fixture["bt_e01"].tm
    df = pd.DataFrame({"pulse_ToA": [58000.0, 58001.0], "pulse_ToA_err": [1.0, 1.0]})
    with pytest.raises(ValueError, match="binary models are not fitted yet"):
        fit_toas.load_toas_for_fit(df, tm)
    with pytest.raises(ValueError, match="binary models are not fitted yet"):
        get_local_ephem.local_ephem_windows(df, tm)
    m = ops._modeltm(tm)
    with pytest.raises(ValueError, match="binary models are not fitted yet"):
        ops._fit_args(None, None, None, None, None, [m], [m])


# ------------------------------------------------------------------------------------------- the fp64 host evaluation
@pytest.mark.parametrize("name", B.MODELS)
def test_host_delay_within_the_derived_bound(fixture, name):
    from crimp_amd.binarymodels import MAX_ITER, binary_delay_host
    m = fixture[name]
    assert m.t.size == 1024 and B.contraction(m.tm) < 0.05
    tau, its = binary_delay_host(m.t, m.tm, return_iterations=True)
    r = m.ratio(tau, "tau")
    print("\nhost %-13s tau max |err|/(u A) = %.2f   iterations mean %.2f max %d" % (name, r, its.mean(), its.max()))
    assert not np.any(np.isnan(tau))
    assert r <= B.FACTOR_TAU
    assert its.max() <= MAX_ITER // 2
    tn = m.t[:8].copy()
    tn[3] = np.nan
    tau_n = binary_delay_host(tn, m.tm)
    assert np.isnan(tau_n[3]) and np.array_equal(np.delete(tau_n, 3), np.delete(tau[:8], 3))
    assert np.array_equal(binary_delay_host(m.t[:6].reshape(2, 3), m.tm), tau[:6].reshape(2, 3))


def test_host_delay_is_zero_without_binary():
    import crimp.binarymodels
    import crimp_amd.binarymodels
    from crimp_amd.binarymodels import binary_delay_host
    assert crimp.binarymodels is crimp_amd.binarymodels          # the alias package exports the module
    assert np.array_equal(binary_delay_host(np.array([58000.0, 58001.0]), {"PEPOCH": 58000.0, "F0": 1.0}), [0.0, 0.0])


def test_iteration_cap_has_margin_up_to_e097():
    """The loop of bin_delay (its host twin: the same starter, bracket, step and stopping rule) over e in [0, 0.97],
    4096 mean anomalies with both sides of periastron down to 1e-12 revolutions, and k = 2 pi A1 / (pb (1 - e)) in
    {0, 0.25, 0.45}: every lane converges within half the cap."""
    from crimp_amd.binarymodels import MAX_ITER, binary_delay_host
    pb = 1.0
    d = np.concatenate([[0.0], np.logspace(-12, -3, 28)])
    frac = np.sort(np.concatenate([np.linspace(-0.5, 0.5, 4096 - 2 * d.size + 1), d[1:], -d]))
    t = 58000.0 + (3.0 + frac) * pb
    worst = 0
    for e in (0.0, 0.1, 0.5, 0.7, 0.9, 0.95, 0.97):
        for k in (0.0, 0.25, 0.45):
            for om in (0.0, 90.0, 217.0):
                a1 = k * pb * 86400.0 * (1 - e) / (2 * np.pi)
                tm = {"PEPOCH": 58000.0, "F0": 1.0, "BINARY": "BT", "PB": pb, "A1": a1, "ECC": e, "OM": om, "T0": 58000.0}
                tau, its = binary_delay_host(t, tm, return_iterations=True)
                assert not np.any(np.isnan(tau)), (e, k, om)
                worst = max(worst, int(its.max()))
    print("\nlargest iteration count over the sweep: %d (cap %d)" % (worst, MAX_ITER))
    assert worst <= MAX_ITER // 2


def test_tempo2_first_order_inverse_is_within_the_second_order_term(fixture):
    """Tempo2's BT model evaluates the orbit at the arrival time and inverts to first order:
    tau_T2 = D (1 - eps), eps = dD/dt = (2 pi / pb) D'(E) / (1 - e cos E). The implicit solution is
    tau = D - eps D + (eps^2 D + D^2 D_tt / 2) + O(eps^3 D), D_tt = (2 pi / pb)^2 d/dE[D' / (1 - e cos E)] / (1 - e cos E)
    (DESIGN.md 2). The two differ by at most twice that second-order term (the third order is smaller by another
    eps <= 2 pi x / (pb (1 - e)) < 0.003 here), plus the rounding bound of the fixture."""
    from crimp_amd.binarymodels import binary_delay_host
    for name in ("bt_circular", "bt_e01", "bt_e07", "bt_e095", "hmxb_wide"):     # BT with constant elements
        m = fixture[name]
        o = B.orbit_values(m.tm)
        e, pb = o["ecc"], o["pb"] * 86400.0
        M = 2 * np.pi * np.mod((m.t - o["t0"]) * 86400.0 / pb, 1.0)
        E = M.copy()
        for _ in range(200):
            E = E - (E - e * np.sin(E) - M) / (1 - e * np.cos(E))
        assert np.max(np.abs(E - e * np.sin(E) - M)) < 1e-12
        w = np.deg2rad(o["om"])
        al, be = o["a1"] * np.sin(w), o["a1"] * np.sqrt(1 - e * e) * np.cos(w)
        s, c = np.sin(E), np.cos(E)
        D, D1, D2 = al * (c - e) + be * s, be * c - al * s, -(al * c + be * s)
        k = 1.0 / (1 - e * c)
        n = 2 * np.pi / pb
        eps = n * D1 * k
        dtt = n * n * k * (D2 * k - D1 * k * k * e * s)
        t2 = D * (1 - eps)
        second = np.abs(eps * eps * D) + 0.5 * D * D * np.abs(dtt)
        ours = binary_delay_host(m.t, m.tm)
        diff = np.abs(ours - t2)
        slack = 2 * second + 64 * B.U * m.A["tau"]
        print("\n%-12s max |tau - tau_T2| = %.3g s, second-order term up to %.3g s" % (name, diff.max(), second.max()))
        assert np.all(diff <= slack)
        # and the second-order term is what separates them, not noise: it accounts for the difference to 1 %
        signed = eps * eps * D + 0.5 * D * D * dtt
        assert np.max(np.abs((ours - t2) - signed)) <= 0.01 * second.max() + 64 * B.U * m.A["tau"].max()


# ------------------------------------------------------------------------------------------- scalar host paths
def test_phase_no_waves_matches_the_fixture(fixture):
    from crimp_amd.ephemIntegerRotation import phase_no_waves
    m = fixture["binary_all"]
    got = np.array([phase_no_waves(t, m.tm) for t in m.t[:64]])
    want = (m.hi["te"][:64] + m.hi["gl"][:64]) + (m.lo["te"][:64] + m.lo["gl"][:64])
    bound = B.FACTOR * B.U * (m.A["te"][:64] + m.A["gl"][:64])
    assert np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize("name", [n for n in B.MODELS if n != "binary_all"] + ["par_e07"])
def test_integer_rotation_converges_on_binary_models(fixture, name):
    """The Newton step keeps the spin frequency as its slope; the true slope is (1 - dtau/dt) times it, within
    k = 2 pi x / (pb (1 - e)) of it, so every step leaves at most k times the phase error it started from (<= 1 cycle
    at the start). What the iteration can reach is tol_phase = 1e-10 or the phase one ulp of the MJD spans, whichever
    is larger (at MJD 58000 an ulp is 0.63 us: the resolution of the result, with or without an orbit), plus the
    rounding unit of the phase itself. So 1 + ceil(log(reach) / log(k)) steps suffice; the test finds the number
    needed per model and prints it (the worst fixture model by k is bt_e095). binary_all is left out: its glitches
    with GLTD = 0 are outside what ephemTmjd evaluates, orbit or not; par_e07 -- 1e2259.par, which has glitches, on
    bt_e07's orbit -- stands in for it."""
    import math
    import crimp_amd.ephemIntegerRotation as EI
    from crimp_amd.readtimingmodel import ReadTimingModel
    if name == "par_e07":
        tm = {**ReadTimingModel(PAR).readfulltimingmodel()[0],
              **{k: v for k, v in fixture["bt_e07"].tm.items() if k in B.orbit_keys()}}
        times = np.linspace(57900.0, 58600.0, 9) + 0.123456
        unit = [2 * abs(EI.phase_no_waves(t, tm)) for t in times]     # a sum of a few terms of the phase's own size
    else:
        m = fixture[name]
        tm, times = m.tm, m.t[::128]
        unit = (m.A["te"] + m.A["gl"])[::128]
    k = B.contraction(tm)
    f0 = abs(float(tm["F0"]))
    worst = 0
    for t, a in zip(times, unit):
        reach = max(1e-10, float(np.spacing(t)) * 86400.0 * f0) + B.FACTOR * B.U * a
        allowed = 1 + math.ceil(math.log(reach) / math.log(k))
        assert allowed < 10
        for steps in range(1, 11):
            out = EI.ephemIntegerRotation(float(t), tm, max_iter=steps)
            if abs(out["phase_residual_from_integer"]) <= reach:
                break
        assert abs(out["phase_residual_from_integer"]) <= reach and steps <= allowed, (t, steps, allowed)
        assert out["Tmjd_intRotation"] <= t
        worst = max(worst, steps)
    print("\n%-13s k = %.2e: the resolution is reached within %d Newton steps (max_iter = 10)" % (name, k, worst))


def test_tim_text_with_a_massless_orbit_is_the_non_binary_text(tmp_path):
    """A1 = 0 (and no GAMMA): tau is 0 and every expression of the host phase is the one without BINARY, so the .tim
    file is the same byte for byte."""
    from crimp_amd.timfile import phshiftTotimfile
    toas = tmp_path / "toas.txt"
    mids = [57950.123456, 58100.5, 58320.987654321]
    toas.write_text("ToA ToA_mid phShift phShift_LL phShift_UL\n" +
                    "".join("%d %r %r 0.01 0.012\n" % (i, t, 0.1 * (i - 1)) for i, t in enumerate(mids)))
    withbin = _par(tmp_path, "BINARY BT\nPB 1.7\nA1 0\nECC 0.3\nOM 40\nT0 57990.25\n")
    phshiftTotimfile(str(toas), PAR, timfile=str(tmp_path / "a"), addpn=True)
    phshiftTotimfile(str(toas), withbin, timfile=str(tmp_path / "b"), addpn=True)
    a, b = open(str(tmp_path / "a.tim"), "rb").read(), open(str(tmp_path / "b.tim"), "rb").read()
    assert a == b and a.count(b"\n") == 4
    # and with a real orbit the ToAs move
    real = _par(tmp_path, "BINARY BT\nPB 1.7\nA1 5\nECC 0.3\nOM 40\nT0 57990.25\n", "r.par")
    phshiftTotimfile(str(toas), real, timfile=str(tmp_path / "c"), addpn=True)
    assert open(str(tmp_path / "c.tim"), "rb").read() != a
