"""Writes tests/golden/calcphase_binary.npz: the orbital delay and the timing-model phase at the emission time at 60
digits (tests/binary_reference.py) for nine binary models, 1024 arrival times each.

Per model ``<name>_model`` (JSON), ``<name>_t`` (fp64 MJD), ``<name>_hi`` / ``<name>_lo`` [5, n] (rows total, te, gl,
wv, tau: the 60-digit value as the nearest double and the remainder to 20 bits) and ``<name>_A`` [4, n] (te, gl, wv,
tau: the error unit, cut down to 16 bits), as calcphase_wide.npz lays its models out; ``index`` lists the names.

Each model is the smallest case where one thing can go wrong:
  bt_circular   e = 0: the Kepler part of the solve is the identity
  bt_e01, bt_e07  moderate and high eccentricity over all orbital phases
  bt_e095       times within 1e-6 revolutions of periastron on both sides, and at apastron
  bt_full       PBDOT in units of 1e-12 and A1DOT as a plain number (both unit conventions), OMDOT, GAMMA
  ell1_amxp     F0 = 401 Hz, PB = 0.0839 d, A1 = 0.0628 lt-s, 1e5 orbits after TASC: high spin times many orbits
  hmxb_wide     PB = 41.5 d, A1 = 368 lt-s, e = 0.46, P = 680 s: the largest delay
  binary_all    bt_e07's orbit with 13 Taylor terms, 32 glitches and 64 wave harmonics; times that arrive after a GLEP
                and were emitted before it; no emission time within 1e-3 s of a mask edge
  binary_short  |phase| <~ 1e5 cycles, <~ 100 orbits: the 1e-9-cycle contract

Asserted here: every model is well inside the contraction limit (2 pi A1 / (pb (1 - e)) < 1/2), mpmath finds the root
for every time (binary_reference.delay_mp), and the fp64 host evaluation is within its bound of every value.

Run from the repository root:  python tests/golden/gen_calcphase_binary_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import binary_reference as B      # noqa: E402
import phase_reference as R       # noqa: E402

N = 1024


def spin(pepoch, f0, f1=0.0, f2=0.0):
    tm = {"PEPOCH": pepoch}
    tm.update({"F%d" % k: 0.0 for k in range(13)})
    tm.update({"F0": f0, "F1": f1, "F2": f2})
    return tm


def bt(pb, a1, ecc, om, t0, **more):
    d = {"BINARY": "BT", "PB": pb, "A1": a1, "ECC": ecc, "OM": om, "T0": t0}
    d.update(more)
    return d


def models(wide):
    m = {}
    m["bt_circular"] = {**spin(58000.0, 11.2, -1.3e-13), **bt(2.1, 10.0, 0.0, 90.0, 57990.3)}
    m["bt_e01"] = {**spin(58000.0, 3.7, -2e-14), **bt(1.4, 6.5, 0.1, 45.0, 57995.1)}
    m["bt_e07"] = {**spin(58000.0, 29.6, -3.7e-10, 1e-20), **bt(8.3, 20.0, 0.7, 200.0, 57991.7)}
    m["bt_e095"] = {**spin(58000.0, 2.3, -1e-12), **bt(30.0, 50.0, 0.95, 300.0, 57800.25)}
    m["bt_full"] = {**spin(58000.0, 17.1, -4e-13), **bt(3.2, 12.0, 0.3, 350.0, 57000.125, PBDOT=2.5, A1DOT=3e-13,
                                                       OMDOT=12.0, GAMMA=0.004)}
    m["ell1_amxp"] = {**spin(58000.0, 401.0, -1e-15), "BINARY": "ELL1", "PB": 0.0839, "A1": 0.0628,
                      "TASC": 58000.0 - 1e5 * 0.0839, "EPS1": 1e-5, "EPS2": -2e-5}
    m["hmxb_wide"] = {**spin(58000.0, 1.0 / 680.0, 1e-14), **bt(41.5, 368.0, 0.46, 130.0, 57950.5)}
    full = dict(wide["all"].tm)
    for src in ("glitches32", "waves64"):       # the 32 glitches and the 64 harmonics of the wide fixture
        full.update({k: v for k, v in wide[src].tm.items() if k.startswith(("GL", "WAVE"))})
    assert R.n_glitches(full) == 32 and R.n_waves(full) == 64
    m["binary_all"] = {**full, **m["bt_e07"], **{k: v for k, v in full.items() if k == "PEPOCH" or k[0] == "F"}}
    m["binary_short"] = {**spin(58140.0, 1.0, -9.7e-15), **bt(0.01, 0.05, 0.2, 75.0, 58139.5)}
    return m


def times(name, tm, wide, rng):
    from crimp_amd.binarymodels import binary_delay_host
    if name == "binary_all":
        t = wide["all"].t
        extra = []
        for j in range(1, 33):      # arrive after GLEP_j, emitted before it: t = GLEP + tau / 2 where tau > 0
            glep = float(tm["GLEP_%d" % j])
            tau = float(binary_delay_host(np.array([glep]), tm)[0])
            if tau > 0.01:
                extra.append(glep + 0.5 * tau / 86400.0)
        assert len(extra) >= 4, extra
        t = np.concatenate([np.array(extra), t])
        tau = binary_delay_host(t, tm)
        gleps = np.array([float(tm["GLEP_%d" % j]) for j in range(1, 33)])
        edge = np.min(np.abs((t[:, None] - gleps[None, :]) * 86400.0 - tau[:, None]), axis=1)
        keep = edge > 2e-3
        assert np.all(keep[:len(extra)])
        rest = t[len(extra):][keep[len(extra):]]
        pick = np.unique(np.linspace(0, rest.size - 1, N - len(extra)).astype(int))
        assert pick.size == N - len(extra)
        return np.concatenate([t[:len(extra)], rest[pick]])
    if name == "ell1_amxp":
        t = 58000.0 + np.sort(rng.uniform(0.0, 10.0, N))
    elif name == "binary_short":
        t = 58140.0 + np.sort(rng.uniform(-0.5, 0.5, N))
    elif name == "hmxb_wide":
        t = 58000.0 + np.sort(rng.uniform(-400.0, 400.0, N))
    else:
        t = 58000.0 + np.sort(rng.uniform(-100.0, 100.0, N))
    if name == "bt_e095":
        pb, t0 = tm["PB"], tm["T0"]
        k = np.arange(5, 9)
        d = np.concatenate([[0.0], np.logspace(-12, -6, 13)])
        peri = (t0 + pb * k[:, None] + pb * np.concatenate([-d[1:], d])[None, :]).ravel()
        apo = t0 + pb * (k + 0.5)
        sp = np.concatenate([peri, apo])
        t = np.sort(np.concatenate([sp, t[:N - sp.size]]))
    t[0], t[-1] = np.floor(t[0]), np.ceil(t[-1])
    return t


def main():
    from crimp_amd.binarymodels import binary_delay_host
    wide = R.load_wide()
    rng = np.random.default_rng(20261020)
    out, index = {}, []
    for name, tm in models(wide).items():
        assert name in B.MODELS
        k = B.contraction(tm)
        assert k < 0.05, (name, k)           # well inside the 1/2 limit
        t = times(name, tm, wide, rng)
        assert t.size == N, (name, t.size)
        host, its = binary_delay_host(t, tm, return_iterations=True)
        assert np.all(np.isfinite(host))
        ref, edge = B.phase_mp(tm, t, starts=host)       # asserts the root for every time
        if name == "binary_all":
            assert min(edge) > 1e-3, min(edge)
            tau = np.array([float(v) for v in ref["tau"][0]])
            gleps = np.array([float(tm["GLEP_%d" % j]) for j in range(1, 33)])
            arr = (t[:, None] - gleps[None, :]) * 86400.0
            assert np.any((arr > 0) & (arr - tau[:, None] < 0)), "no time arrives after a GLEP it was emitted before"
        hi, lo = zip(*(R.hi_lo(ref[row][0]) for row in B.ROWS))
        a = np.vstack([R.mag_chopped(ref[row][1]) for row in B.A_ROWS])
        hi, lo = np.vstack(hi), np.vstack(lo)
        r = np.max(np.abs((host - hi[4]) - lo[4]) / (B.U * a[3]))
        print("%-13s k = %.2e  |tau| <= %.3g s  host |err|/(u A) = %.2f  iterations mean %.2f max %d" %
              (name, k, np.max(np.abs(hi[4])), r, its.mean(), its.max()))
        assert r <= B.FACTOR_TAU, (name, r)
        out[name + "_model"] = np.array(json.dumps(tm))
        out[name + "_t"] = t
        out[name + "_hi"], out[name + "_lo"], out[name + "_A"] = hi, lo, a
        index.append(name)
    assert tuple(index) == B.MODELS
    out["index"] = np.array(json.dumps(index))
    path = os.path.join(HERE, "calcphase_binary.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
