"""Every candidate of every cell of crimp_sim_events against the documented stream (include/crimp_hip.h; DESIGN.md
5.7): counter = (cell low, cell high, round, lane), words 0-1 the gap's uniform, words 2-3 the thinning uniform.
tests/stream_reference.py replays the cells on the host -- gaps -log(u) / lam_max, the 64-lane scan in its doubling
order, candidates alive below the next cell's start and the span's end, thinned by u lam_max < S + bkg inside the
GTIs, background where u lam_max >= S -- and the device's list has to be that list: the same count, order and flags,
times within 2^-48 cell_s + 2 ulp(out_offset_s + span_s) (stream_reference.sim_tolerances derives it).

A candidate whose time is within that tolerance of its cell's or the span's end, whose MJD is within it of a GTI edge,
or (step tables) whose 60-digit phase is within 1e-9 cycles of a bin edge whose two rates decide differently, may go
either way; such candidates are counted, and the inputs are chosen so that there are none (checked on the CPU, from the
replay alone, at most 0.1 % being the cap).
"""
import functools

import numpy as np
import pytest

import phase_reference as PR
import sim_reference as R
import stream_reference as SR

SEED = 0x9E3779B97F4A7C15       # both key words set
LAM, CELL = 40.0, 4.8           # the flat rate and cell of tests/test_gpu_simulate.py: 192 candidates per cell
STEPS16 = R.step_table(16)
STEP_BKG = 1.0
STEP_LAM = float(STEPS16.max()) + STEP_BKG
STEP_CELL = 192.0 / STEP_LAM
F0F1_MODEL = {"PEPOCH": R.MJD0 - 0.01, "F0": 3.1, "F1": -1.0e-5}    # at dt ~ 900 s F1 holds ~4 of ~2700 cycles


def case(steps=(LAM,), bkg=0.0, lam_max=None, cell=CELL, cells=2.3, tm=R.FLAT_MODEL, gti=None, first_cell=0,
         n_cells=-1, days=False, seed=SEED, out_offset_s=0.0):
    steps = np.asarray(steps, dtype=np.float64)
    lam_max = float(steps.max() + bkg) if lam_max is None else lam_max
    if gti is not None:
        gti = R.MJD0 + np.asarray(gti, dtype=np.float64) * cell / 86400.0
    return dict(steps=steps, bkg=bkg, lam_max=lam_max, cell=cell, span=cells * cell, tm=tm, gti=gti,
                first_cell=first_cell, n_cells=n_cells, days=days, seed=seed, out_offset_s=out_offset_s)


CASES = {
    "flat_2.3_cells": case(),                                            # a partial last cell
    "flat_256.3_cells": case(cells=256.3),
    "flat_seed_1": case(seed=1),
    "flat_bkg_thinned": case(steps=(25.0,), bkg=10.0, lam_max=40.0, cells=5.3, out_offset_s=86400.0),
    "flat_400_per_cell": case(cell=400.0 / LAM, cells=3.37),             # seven or more rounds
    "steps16_f0": case(steps=STEPS16, bkg=STEP_BKG, cell=STEP_CELL, cells=3.3),
    "steps16_f0_f1": case(steps=STEPS16, bkg=STEP_BKG, cell=STEP_CELL, cells=3.3, tm=F0F1_MODEL),
    "two_gtis": case(cells=4.3, gti=[[0.5, 1.4], [2.2, 3.1]]),           # both end inside a cell
    "cells_3_and_4_of_8": case(cells=7.6, first_cell=3, n_cells=2),
    "days": case(cells=3.3, days=True),
}


def frac_phase(tm):
    """mjd [k] -> the fractional part of the 60-digit phase (tests/phase_reference.py), as floats."""
    plain = PR.plain(tm)
    plain = dict({"F%d" % k: 0.0 for k in range(13)}, **plain)

    def f(mjd):
        mp = PR._mp()
        val, _ = PR.taylor_mp(plain, mjd)
        return np.array([float(v - mp.floor(v)) for v in val])
    return f


@functools.lru_cache(maxsize=None)
def replayed(name):
    c = CASES[name]
    nc = int(np.ceil(c["span"] / c["cell"]))
    last = nc if c["n_cells"] < 0 else c["first_cell"] + c["n_cells"]
    return SR.sim_replay(c["seed"], c["steps"], c["bkg"], c["lam_max"], R.MJD0, c["span"], c["cell"],
                         range(c["first_cell"], last), gti=c["gti"],
                         frac_phase=frac_phase(c["tm"]) if c["steps"].size > 1 else None,
                         out_offset_s=c["out_offset_s"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_have_no_ambiguous_candidate(name):
    """From the replay alone, no device involved: what each case reaches, and that at most one of its candidates (and
    at most 0.1 %) could be decided either way by a conforming device."""
    rep, c = replayed(name), CASES[name]
    events = [o for o in rep["outcomes"] if o != {None}]
    print("%-20s candidates %6d events %6d ambiguous %d rounds %d" % (name, rep["candidates"], len(events),
                                                                     rep["ambiguous"], rep["rounds"]))
    assert rep["ambiguous"] <= 1 and rep["ambiguous"] <= 1e-3 * rep["candidates"]
    assert len(events) > 100
    flags = set().union(*events)
    if c["bkg"] > 0:
        assert {0, 1} <= flags                                    # both flags occur
        assert len(events) < 0.97 * sum(1 for s in rep["s"] if s < c["span"])  # and candidates are thinned away
    if name == "flat_400_per_cell":
        assert rep["rounds"] >= 7
    if name == "two_gtis":
        assert len(events) < 0.6 * rep["candidates"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_events_are_the_thinned_candidates_of_the_stream(gpu, name):
    from crimp_amd import ops
    c, rep = CASES[name], replayed(name)
    shape = ops.make_sim_shape(steps=c["steps"], bkg=c["bkg"], lam_max=c["lam_max"])
    t, b, n = ops.sim_events(c["tm"], shape, R.MJD0, c["span"], c["cell"], gti=c["gti"], seed=c["seed"],
                             first_cell=c["first_cell"], n_cells=c["n_cells"], days=c["days"],
                             out_offset_s=c["out_offset_s"])
    assert n == t.size == b.size
    events, amb, worst = SR.sim_match(rep, t, b, days=c["days"], out_offset_s=c["out_offset_s"])
    print("%-20s candidates %6d events %6d ambiguous %d largest |dt| / bound %.3g" % (name, rep["candidates"], events,
                                                                                     amb, worst))
    assert events == n and amb <= 1e-3 * rep["candidates"]
    if name == "cells_3_and_4_of_8":    # the same cells of the whole call
        tw, bw, _ = ops.sim_events(c["tm"], shape, R.MJD0, c["span"], c["cell"], seed=c["seed"])
        sel = (tw >= 3 * c["cell"]) & (tw < 5 * c["cell"])
        assert np.array_equal(tw[sel], t) and np.array_equal(bw[sel], b)
