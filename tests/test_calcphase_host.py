"""CPU checks behind tests/test_gpu_calcphase.py: the wide calcphase fixture against the 60-digit formula it was made
from, the oracle against that fixture, and the packing of a timing-model dict into crimp_timing_model.

The bound everywhere is |x - mp| <= 32 u A(t) per element (tests/phase_reference.py); the printed figures are the
largest |x - mp| / (u A) per model."""
import json

import numpy as np
import pytest

import phase_reference as R
from conftest import gpath


@pytest.fixture(scope="module")
def wide():
    return R.load_wide()


def test_fixture_rederives_from_the_formula(wide):
    """hi + lo and A of a 100-point sample per model re-derive bit for bit from phase_reference at 60 digits."""
    rng = np.random.default_rng(100)
    for name, m in wide.items():
        idx = np.sort(rng.choice(m.t.size, 100, replace=False))
        mpv = R.phase_mp(m.tm, m.t[idx])
        for p in R.PARTS:
            hi, lo = R.hi_lo(mpv[p][0])
            np.testing.assert_array_equal(hi, m.hi[p][idx], err_msg="%s %s hi" % (name, p))
            np.testing.assert_array_equal(lo.astype(np.float64), m.lo[p][idx], err_msg="%s %s lo" % (name, p))
        a3 = [R.mag_chopped(mpv[p][1]).astype(np.float64) for p in R.PARTS[1:]]
        for p, a in zip(R.PARTS[1:], a3):
            np.testing.assert_array_equal(a, m.A[p][idx], err_msg="%s %s A" % (name, p))
        np.testing.assert_array_equal(a3[0] + a3[1] + a3[2], m.A["total"][idx])


def test_fixture_covers_what_it_claims(wide):
    s = wide["short"]
    assert np.any(s.hi["total"] < 0) and np.any(s.t < s.tm["PEPOCH"])
    assert R.FACTOR * R.U * np.max(s.A["total"]) < 1e-9          # the 1e-9-cycle contract is the weaker bound on short
    for name in ("short", "glitches32", "all"):
        m = wide[name]
        for j in range(1, R.n_glitches(m.tm) + 1):
            e = m.tm["GLEP_%d" % j]
            assert np.nextafter(e, -np.inf) in m.t and e in m.t and np.nextafter(e, np.inf) in m.t
    g = wide["glitches32"].tm
    ep = [g["GLEP_%d" % j] for j in range(1, 33)]
    assert R.n_glitches(g) == 32 and len(set(ep)) == 31 and ep != sorted(ep)
    td = np.array([g["GLTD_%d" % j] for j in range(1, 33)])
    for lo, hi in ((0.0, 0.0), (0.005, 0.02), (20.0, 45.0), (5e3, 2e4)):     # the four kinds of GLTD
        assert np.sum((td >= lo) & (td <= hi)) == 8
    assert R.n_waves(wide["waves64"].tm) == 64 and wide["waves64"].tm["WAVEEPOCH"] in wide["waves64"].t
    assert all(wide["taylor13"].tm["F%d" % k] != 0 for k in range(13))
    assert [k for k in range(13) if wide["taylor13_gaps"].tm["F%d" % k] == 0] == [5, 6, 12]
    assert [k for k in range(13) if wide["taylor13_f12"].tm["F%d" % k] != 0] == [12]
    assert R.plain(wide["all_flags"].tm) == wide["all"].tm and wide["all_flags"].tm != wide["all"].tm
    for m in wide.values():
        assert m.t.size % 2 == 0 and m.t.size > 1500


def test_reference_values_within_bound(wide):
    print()
    for name, m in wide.items():
        r = {p: m.ratio(m.ref[p], p) for p in R.PARTS}
        print("reference %-14s max |err|/(u A): total %.2f  taylor %.2f  glitches %.2f  waves %.2f"
              % (name, r["total"], r["te"], r["gl"], r["wv"]))
        assert max(r.values()) <= R.FACTOR, (name, r)


def test_oracle_within_bound(wide):
    from oracle import oracle as O
    print()
    for name, m in wide.items():
        r, same = {}, {}
        for p in R.PARTS:
            tot, fol = O.calcphase(m.t, m.tm, parts=R.PART_MASK[p])
            r[p] = m.ratio(tot, p)
            same[p] = bool(np.array_equal(tot, m.ref[p]))
            np.testing.assert_array_equal(fol, tot - np.floor(tot))
        print("oracle    %-14s max |err|/(u A): total %.2f  taylor %.2f  glitches %.2f  waves %.2f   "
              "bit-identical to the reference: %s" % (name, r["total"], r["te"], r["gl"], r["wv"], same))
        assert max(r.values()) <= R.FACTOR, (name, r)
    s = wide["short"]
    tot, fol = O.calcphase(s.t, s.tm)
    assert np.max(s.err(tot)) <= 1e-9 and np.all((fol >= 0) & (fol < 1))


# ------------------------------------------------------------------------------------------- ops._modeltm
@pytest.fixture()
def modeltm(monkeypatch):
    """ops._modeltm with the native library out of reach: packing is pure ctypes."""
    from crimp_amd import ops, _native as N

    def no_load(*a, **k):
        raise AssertionError("packing a timing model must not load the native library")
    monkeypatch.setattr(N, "load", no_load)
    return ops._modeltm


def _glitch(m, j):
    return [m.glitch[j][c] for c in range(7)]


def test_modeltm_packs_every_fixture_model(wide, modeltm):
    for name, mod in wide.items():
        tm = R.plain(mod.tm)
        m = modeltm(mod.tm)
        assert m.pepoch == tm["PEPOCH"] and [m.f[k] for k in range(13)] == [tm["F%d" % k] for k in range(13)]
        assert m.n_glitch == R.n_glitches(tm) and m.n_wave == R.n_waves(tm), name
        for j in range(1, m.n_glitch + 1):
            assert _glitch(m, j - 1) == [tm["GLEP_%d" % j]] + [tm["%s_%d" % (b, j)] for b in R.GLITCH_KEYS]
        for j in range(1, m.n_wave + 1):
            assert (m.wave_ab[j - 1][0], m.wave_ab[j - 1][1]) == (tm["WAVE%d" % j]["A"], tm["WAVE%d" % j]["B"])
        if m.n_wave:
            assert (m.wave_epoch, m.wave_om) == (tm["WAVEEPOCH"], tm["WAVE_OM"])
    assert modeltm(wide["glitches32"].tm).n_glitch == 32 and modeltm(wide["waves64"].tm).n_wave == 64


def test_modeltm_defaults_and_counts(modeltm):
    # calcphase.py:105-110: absent GLPH / GLF* / GLTD keys count as 0.0; absent F keys are 0.0 here too
    m = modeltm({"PEPOCH": 58000.0, "F0": 0.5, "GLEP_1": 58001.0, "GLF0_1": 1e-7, "GLEP_2": 58002.5, "GLTD_2": 3.0})
    assert m.n_glitch == 2 and m.n_wave == 0
    assert _glitch(m, 0) == [58001.0, 0.0, 1e-7, 0.0, 0.0, 0.0, 0.0]
    assert _glitch(m, 1) == [58002.5, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0]
    assert [m.f[k] for k in range(13)] == [0.5] + [0.0] * 12
    # calcphase.py:94: the count of GLEP_ keys decides, other glitch keys do not
    assert modeltm({"PEPOCH": 1.0, "GLF0_1": 1e-7}).n_glitch == 0
    # calcphase.py:135, :142: n - 2 harmonics of n WAVE* keys; the epoch and OM alone give none
    m = modeltm({"PEPOCH": 1.0, "F0": 1.0, "WAVEEPOCH": 58000.0, "WAVE_OM": 0.1})
    assert m.n_wave == 0 and (m.wave_epoch, m.wave_om) == (58000.0, 0.1)
    m = modeltm({"PEPOCH": 1.0, "F0": 1.0, "WAVEEPOCH": 58000.0, "WAVE_OM": 0.1, "WAVE1": {"A": 1.0, "B": 2.0},
                 "WAVE2": {"A": 3.0, "B": 4.0}})
    assert m.n_wave == 2 and [tuple(m.wave_ab[j]) for j in range(3)] == [(1.0, 2.0), (3.0, 4.0), (0.0, 0.0)]
    # {value, flag} entries unwrap (readtimingmodel.py:309-321)
    m = modeltm({"PEPOCH": {"value": 58000.0, "flag": 0}, "F0": {"value": 0.25, "flag": 1},
                 "GLEP_1": {"value": 58001.0, "flag": 0}, "GLPH_1": {"value": 0.5, "flag": 1}})
    assert (m.pepoch, m.f[0], m.n_glitch) == (58000.0, 0.25, 1) and _glitch(m, 0)[:2] == [58001.0, 0.5]


def test_modeltm_limits(wide, modeltm):
    g = dict(wide["glitches32"].tm)
    g["GLEP_33"] = 58000.0
    with pytest.raises(ValueError, match="at most 32 glitches"):
        modeltm(g)
    w = dict(wide["waves64"].tm)
    w["WAVE65"] = {"A": 0.1, "B": 0.1}
    with pytest.raises(ValueError, match="at most 64 wave harmonics"):
        modeltm(w)


def test_old_fixture_model_is_the_short_model(wide):
    assert wide["short"].tm == json.load(open(gpath("timing_model_dict.json")))
