"""crimp_orbit_search on the MI355X: every power against the long-double truth of
tests/orbit_search_reference.py within the unit derived there, recovery of the true (orbit, frequency) cell, bitwise
independence of the orbit slicing and the scratch cap, and the boundary of the call. The photons are drawn by thinning
from a pulsed signal in a known orbit; the shapes are the smallest that reach every edge of the plan in force (slice
length and trial chunk J read from crimp_orbit_search_plan)."""
import numpy as np
import pytest

import orbit_search_reference as OR
import search_reference as SR

pytestmark = pytest.mark.gpu


def _plan(n=1, nf=1, m=2):
    from crimp_amd import _native as N
    return N.orbit_search_plan(n, nf, m)


def _jof(m):
    return _plan(m=m)["J"]


@pytest.fixture(scope="module")
def all_cases(gpu):
    return {c.name: c for c in OR.cases(_plan()["slice"], _jof)}


@pytest.fixture(scope="module")
def powers(gpu, all_cases):
    """Every case's (power [norb, nf], best [norb, 2]) computed once."""
    from crimp_amd import ops
    out = {}
    for c in all_cases.values():
        out[c.name] = ops.orbit_search(c.t, c.tm, c.keys, c.orbits, c.freq, c.m, c.stat, fdot=c.fdot, tref=c.tref,
                                       want_best=True)
    return out


CASES = ("ell1_big_z2m2", "bt_e0_big_z2m1_fdot", "bt_e07_big_hm5_pb", "bt_e095_big_hm9_fdot_unsorted",
         "ell1_slice1_hm20", "ell1_n1_z2m2", "ell1_n255_hm5_fdot", "ell1_n257_z2m1")


def test_case_list_is_the_reference_modules(all_cases):
    assert tuple(all_cases) == CASES


# --------------------------------------------------------------------------------------------------- 1. truth
@pytest.mark.parametrize("name", CASES)
def test_powers_within_the_unit_of_the_truth(all_cases, powers, name):
    """|power - truth| <= unit on every orbit and the stated trials: checked_trials(nf, edges=(J,), nrandom=8)."""
    c = all_cases[name]
    pw = powers[name][0]
    assert pw.shape == (c.orbits.shape[0], c.nf) and np.all(np.isfinite(pw))
    trials = SR.checked_trials(c.nf, edges=(_jof(c.m),), nrandom=8)
    worst = 0.0
    for o in range(c.orbits.shape[0]):
        truth, unit = c.truth(o, trials)
        ratio = np.abs(pw[o, trials] - truth) / unit
        worst = max(worst, float(ratio.max()))
        if o == c.otrue and c.jtrue in trials:  # the unit is not vacuous: 1e-6 of the power at the signal trial
            k = int(np.flatnonzero(trials == c.jtrue)[0])
            assert unit[k] <= 1e-6 * truth[k], (name, unit[k], truth[k])
    print("%s: n %d nf %d m %d stat %d fdot %g orbits %d trials %d: max |err| / unit = %.4f"
          % (name, c.n, c.nf, c.m, c.stat, c.fdot, c.orbits.shape[0], trials.size, worst))
    assert worst <= 1.0, (name, worst)


# ------------------------------------------------------------------------------------------------ 2. recovery
@pytest.mark.parametrize("name", [n for n in CASES if n != "ell1_n1_z2m2"])  # (one photon carries no signal)
def test_argmax_is_the_true_cell(all_cases, powers, name):
    c = all_cases[name]
    pw = powers[name][0]
    o, j = np.unravel_index(int(np.argmax(pw)), pw.shape)
    assert (o, j) == (c.otrue, c.jtrue), (name, o, j, c.otrue, c.jtrue)


@pytest.mark.parametrize("name", CASES)
def test_best_is_argmax_of_every_row(powers, name):
    pw, best = powers[name]
    idx = np.argmax(pw, axis=1)
    assert np.array_equal(best[:, 1], idx.astype(np.float64))
    assert np.array_equal(best[:, 0], pw[np.arange(pw.shape[0]), idx])


def test_exact_tie_goes_to_the_lowest_index(gpu, all_cases):
    """Two identical orbits and the signal frequency listed twice: identical rows, and in each row an exact tie that
    the lowest index wins, as np.argmax."""
    from crimp_amd import ops
    c = all_cases["ell1_n257_z2m1"]
    orbits = np.concatenate([c.orbits[c.otrue:c.otrue + 1]] * 2 + [c.orbits[:3]])
    freq = np.array([c.f0 - 1e-4, c.f0, c.f0 + 1e-4, c.f0, c.f0 + 2e-4])
    pw, best = ops.orbit_search(c.t, c.tm, c.keys, orbits, freq, 2, 0, tref=c.tref, want_best=True)
    assert np.array_equal(pw[0], pw[1])
    assert np.array_equal(pw[:, 1], pw[:, 3])
    assert best[0, 1] == 1.0 and best[1, 1] == 1.0 and best[0, 0] == pw[0, 1]
    assert np.array_equal(best[:, 1], np.argmax(pw, axis=1).astype(np.float64))
    assert int(np.argmax(pw)) == 1  # of the two identical orbits the first


# ------------------------------------------------------------------------------------------------- 3. slicing
def test_first_count_pieces_equal_the_whole_call_bitwise(gpu, all_cases, powers):
    from crimp_amd import ops
    for name in ("ell1_big_z2m2", "bt_e07_big_hm5_pb"):
        c = all_cases[name]
        pw, best = powers[name]
        norb = c.orbits.shape[0]
        parts = [ops.orbit_search(c.t, c.tm, c.keys, c.orbits, c.freq, c.m, c.stat, fdot=c.fdot, tref=c.tref,
                                  first=a, count=b, want_best=True) for a, b in ((0, 1), (1, 7), (8, norb - 8))]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), pw)
        assert np.array_equal(np.concatenate([p[1] for p in parts]), best)
        # an orbit alone in its call, with no other orbit in the array
        o = c.otrue
        alone = ops.orbit_search(c.t, c.tm, c.keys, c.orbits[o:o + 1], c.freq, c.m, c.stat, fdot=c.fdot,
                                 tref=c.tref)[0]
        assert np.array_equal(alone[0], pw[o])


def test_small_scratch_cap_equals_the_whole_call_bitwise(gpu, all_cases, powers, monkeypatch):
    from crimp_amd import _native as N
    from crimp_amd import ops
    c = all_cases["ell1_big_z2m2"]
    norb = c.orbits.shape[0]
    full = N.orbit_search_plan(c.n, c.nf, c.m, c.stat, norb)
    assert full["nbatches"] == 1
    per_kb = -(-full["nslices"] * 2 * c.m * c.nf * 8 // 1024)
    for kb, batch in ((1, 1), (3 * per_kb, None)):
        monkeypatch.setenv("CRIMP_ORBIT_SCRATCH_KB", str(kb))
        p = N.orbit_search_plan(c.n, c.nf, c.m, c.stat, norb)
        assert p["nbatches"] > 1 and (batch is None or p["batch"] == batch)
        assert (p["slice"], p["nslices"], p["J"]) == (full["slice"], full["nslices"], full["J"])
        pw, best = ops.orbit_search(c.t, c.tm, c.keys, c.orbits, c.freq, c.m, c.stat, fdot=c.fdot, tref=c.tref,
                                    want_best=True)
        assert np.array_equal(pw, powers[c.name][0]) and np.array_equal(best, powers[c.name][1])


def test_sharded_orbit_search_without_a_process_group(gpu, all_cases, powers):
    from crimp_amd.sharding import sharded_orbit_search
    c = all_cases["bt_e0_big_z2m1_fdot"]
    out = sharded_orbit_search(c.t, c.tm, c.keys, c.orbits, c.freq, c.m, c.stat, fdot=c.fdot, tref=c.tref)
    assert np.array_equal(out, powers[c.name][0])


# ------------------------------------------------------------------------------------------------ 4. boundary
def test_device_times_keep_the_results_on_the_device(gpu, all_cases, powers):
    import torch
    from crimp_amd import ops
    c = all_cases["bt_e095_big_hm9_fdot_unsorted"]
    td = torch.as_tensor(c.t, device=gpu)
    pw, best = ops.orbit_search(td, c.tm, c.keys, c.orbits, c.freq, c.m, c.stat, fdot=c.fdot, tref=c.tref,
                                want_best=True)
    assert pw.is_cuda and best.is_cuda
    assert np.array_equal(pw.cpu().numpy(), powers[c.name][0]) and np.array_equal(best.cpu().numpy(), powers[c.name][1])


def test_orbitsearch_class_grid_and_best_only(gpu, all_cases, powers):
    from crimp_amd.orbitsearch import OrbitSearch
    c = all_cases["ell1_big_z2m2"]
    s = OrbitSearch(c.t, c.tm, c.freq, nbrHarm=c.m, fdot=c.fdot, tref=c.tref)
    ref = powers[c.name][0]
    assert np.array_equal(s.ztest(c.orbits, c.keys), ref)
    pw, table = s.grid("z2", **c.axes)
    shape = tuple(c.axes[k].size for k in c.keys)
    assert pw.shape == shape + (c.nf,) and np.array_equal(pw.reshape(ref.shape), ref)
    assert list(table.columns) == c.keys + ["Freq", "Power"] and len(table) == ref.shape[0]
    assert np.array_equal(table["Power"].to_numpy(), ref.max(axis=1))
    assert np.array_equal(table["Freq"].to_numpy(), c.freq[np.argmax(ref, axis=1)])
    assert np.array_equal(table[c.keys].to_numpy(), c.orbits)
    none, table2 = s.grid("z2", best_only=True, **c.axes)
    assert none is None and table2.equals(table)
    assert np.array_equal(s.best("z2", c.orbits, c.keys), powers[c.name][1])
    h = OrbitSearch(c.t, c.tm, c.freq, nbrHarm=c.m, tref=c.tref).htest(c.orbits[:2], c.keys)
    assert h.shape == (2, c.nf) and not np.array_equal(h, ref[:2])
    # the default reference epoch is PeriodSearch's
    assert OrbitSearch(c.t, c.tm, c.freq).tref == (c.t[0] + c.t[-1]) / 2


def test_searchorbit_cli(gpu, all_cases, powers, tmp_path, capsys):
    from crimp_amd import orbitsearch as S
    c = all_cases["ell1_n255_hm5_fdot"]
    np.save(tmp_path / "t.npy", c.t)
    par = tmp_path / "m.par"
    g = lambda v: "%.17g" % float(v)
    par.write_text("PSR J0001+0000\nPEPOCH 58000\nF0 401.0 1\nBINARY ELL1\n" +
                   "".join("%s %s\n" % (k, g(c.tm[k])) for k in ("PB", "A1", "TASC", "EPS1", "EPS2")))
    axes = ["-a", "TASC=%s:%s:5" % (g(c.axes["TASC"][0]), g(c.axes["TASC"][-1])),
            "-a", "A1=%s:%s:5" % (g(c.axes["A1"][0]), g(c.axes["A1"][-1]))]
    out = tmp_path / "best.txt"
    table = S.main([str(tmp_path / "t.npy"), str(par), str(out), "-fl", g(c.freq[0]), "-fh", g(c.freq[-1]),
                    "-nf", str(c.nf), "-fd=" + g(c.fdot), "-nh", str(c.m), "-s", "h"] + axes)
    assert len(table) == 25 and list(table.columns) == ["TASC", "A1", "Freq", "Power"]
    top = table.iloc[int(np.argmax(table["Power"].to_numpy()))]
    assert abs(top["TASC"] - c.tm["TASC"]) < 1e-9 and abs(top["A1"] - c.tm["A1"]) < 1e-12
    assert abs(top["Freq"] - c.f0) < 1e-9
    rows = [ln for ln in out.read_text().splitlines() if not ln.startswith("#")]
    assert len(rows) == 26 and rows[0].split() == ["TASC", "A1", "Freq", "Power"]
    assert "Best orbit of 25" in capsys.readouterr().out


def test_empty_grids_launch_nothing(gpu, all_cases):
    from crimp_amd import ops
    c = all_cases["ell1_n257_z2m1"]
    pw, best = ops.orbit_search(c.t, c.tm, c.keys, c.orbits[:0], c.freq, 2, 0, want_best=True)
    assert pw.shape == (0, c.nf) and best.shape == (0, 2)
    pw, best = ops.orbit_search(c.t, c.tm, c.keys, c.orbits, np.zeros(0), 2, 0, want_best=True)
    assert pw.shape == (c.orbits.shape[0], 0) and best.shape == (0, 2)
    pw, _ = ops.orbit_search(c.t, c.tm, c.keys, c.orbits, c.freq, 2, 0, first=3, count=0)
    assert pw.shape == (0, c.nf)


def test_inadmissible_orbit_raises_and_writes_nothing(gpu, all_cases):
    from crimp_amd import _native as N
    from crimp_amd import ops
    from crimp_amd.orbitsearch import OrbitSearch
    c = all_cases["bt_e0_big_z2m1_fdot"]
    orbits = c.orbits.copy()
    orbits[12, c.keys.index("A1")] = -1.0
    power = np.full((orbits.shape[0], c.nf), -7.0)
    best = np.full((orbits.shape[0], 2), -7.0)
    with pytest.raises(N.CrimpNativeError, match=r"orbit 12: A1 must be >= 0"):
        ops.orbit_search(c.t, c.tm, c.keys, orbits, c.freq, c.m, c.stat, power=power, best=best)
    assert np.all(power == -7.0) and np.all(best == -7.0)
    with pytest.raises(ValueError, match=r"orbit 12 .*A1 must be >= 0"):
        OrbitSearch(c.t, c.tm, c.freq).ztest(orbits, c.keys)
    # the range that leaves the orbit out is computed
    pw, _ = ops.orbit_search(c.t, c.tm, c.keys, orbits, c.freq, c.m, c.stat, first=0, count=12)
    assert pw.shape == (12, c.nf) and np.all(np.isfinite(pw))
    with pytest.raises(N.CrimpNativeError, match="orbit range"):
        ops.orbit_search(c.t, c.tm, c.keys, c.orbits, c.freq, c.m, c.stat, first=20, count=10)
    with pytest.raises(N.CrimpNativeError, match="kind does not have"):
        ops.orbit_search(c.t, c.tm, [N.ORBIT_FIELDS.index("EPS1")], c.orbits[:, :1], c.freq, c.m, c.stat)


def test_symbols_are_exported():
    from crimp_amd import _native as N
    assert "crimp_orbit_search" in N.EXPORTS and "crimp_orbit_search_plan" in N.EXPORTS
