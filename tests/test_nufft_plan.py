"""The host plan of the NUFFT period search (csrc/search_nufft_plan.h: plan_nufft_search) on the CPU.

`make -C crimp_amd/csrc nufft-plan-check` builds search_nufft_plan_check.cpp with the host compiler under
-fsanitize=address,undefined; every case below is one run of that program (no GPU, no preloaded library, no
environment hook: the hooks and the budget are fields of the case). What it prints is held to the definitions restated
here in numpy: n and P per segment, the declines, the row groups and batches, the start-table layout, the gather sets,
the MFMA passes, and the work and launch counts of DESIGN.md 5.3."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crimp_amd", "csrc")
EPS, EPS_ZM = 5e-14, 5e-13
AUTO, GATHER, MFMA = 0, 1, 2
BUDGET = 6144 << 20
CLASSES = ("cellstart", "spread", "merge", "pass1", "pass2", "combine", "finalize")
SEGMENTS = [64, 100, 1401, 2048, 3000, 4096, 5000, 80000, 100000, 600000, 1000000, 1200000]


@pytest.fixture(scope="module")
def plan_check():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-s", "-B", "-C", CSRC, "nufft-plan-check"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(CSRC, "build", "nufft_plan_check")


def fhex(v):
    v = float(v)
    return v.hex() if np.isfinite(v) else repr(v)


def run_plan(exe, hs, n, nf, rows=1, nharm=2, stat=0, first=0, count=None, best=0, spread=AUTO, lanes=0, generic=0,
             separate=0, budget=BUDGET, unsorted=0):
    """One case through the check program -> the plan as a dict (groups with their cells and batches nested)."""
    count = rows * nf - first if count is None else count
    text = "%s %d\n%d %d %d %d %d %d %d %d\n%d %d %d %d %d\n" % (
        " ".join(fhex(v) for v in hs), unsorted, n, nf, rows, nharm, stat, first, count, best, spread, lanes, generic,
        separate, budget)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    p = {"groups": [], "n": n, "nf": nf, "nharm": nharm, "first": first, "count": count}
    for ln in r.stdout.splitlines():
        key, *v = ln.split()
        if key == "work":
            p["work"] = [float.fromhex(t) for t in v]
        elif key == "launches":
            p["launches"] = [int(t) for t in v]
        elif key == "group":
            g = dict(zip(("r0", "r1", "j0", "nseg", "h", "lnfft", "P", "ln1", "ln2", "fuse", "jbase", "starts_off"),
                         (int(t) for t in v[:12])))
            g.update(zip(("invfact", "s1", "fch", "fcl"), (float.fromhex(t) for t in v[12:])))
            g.update(cells=[], batches=[])
            p["groups"].append(g)
        elif key in ("gmin", "gmax", "soff"):
            p["groups"][-1][key] = [int(t) for t in v]
        elif key == "cell":
            w = [int(t) for t in v]
            p["groups"][-1]["cells"].append({"k0": w[0], "nk": w[1], "gmin": w[2::3], "span": w[3::3], "off": w[4::3]})
        elif key == "batch":
            b = dict(zip(("rb", "nrow", "tb0", "nbt", "best_base"), (int(t) for t in v)))
            b.update(sets=[], mfma=[])
            p["groups"][-1]["batches"].append(b)
        elif key == "set":
            w = [int(t) for t in v]
            names = ("k", "lanes_log2", "blk0", "gmin", "gmax", "gbase", "gcount", "soff", "woff")
            s = {nm: w[2 + i::9] for i, nm in enumerate(names)}
            s.update(nk=w[0], blocks=w[1])
            p["groups"][-1]["batches"][-1]["sets"].append(s)
        elif key == "mfma":
            w = [int(t) for t in v]
            p["groups"][-1]["batches"][-1]["mfma"].append({"k0": w[0], "gl": w[1], "ipass": w[2], "gmin": w[3::2],
                                                           "ubase": w[4::2]})
        else:
            p[key] = int(v[0])
    return p


# ---------------------------------------------------------------- the definitions, restated
def trunc(x, P):
    """2.4 (x/2)^P / P!"""
    return 2.4 * (x / 2.0) ** P / math.factorial(P)


def least_np(nseg, pmax, eps):
    """(log2 n, P): the least n P among the powers of two n >= max(nseg, 64) up to 2^24 whose edge bound is <= eps
    within pmax moments (the smaller n on a tie; no n beyond the first that needs <= 4 moments)."""
    h = nseg // 2
    edge = max(h, nseg - 1 - h)
    best = None
    for l in range(max(int(nseg - 1).bit_length(), 6), 25):
        x = math.pi * edge / 2.0 ** l
        p = next((q for q in range(1, pmax + 1) if trunc(x, q) <= eps), None)
        if p is None:
            continue
        if best is None or (p << l) < (best[1] << best[0]):
            best = (l, p)
        if p <= 4:
            break
    return best


def cells(hs, lnfft, k):
    """Unwrapped cells of dt[0], dt[n-1] for harmonic k, the kernels' arithmetic rint(k (dt s1))."""
    s1 = float(1 << lnfft) * hs[0]
    return int(np.rint(k * (hs[2] * s1))), int(np.rint(k * (hs[3] * s1)))


def occupied(gmin, gmax, lnfft, ln1):
    """(first row, rows) of the four-step view [n1][n2] the wrapped cells of [gmin, gmax] touch."""
    nfft, n1, ln2 = 1 << lnfft, 1 << ln1, lnfft - ln1
    if ln1 == 0 or gmax - gmin + 1 >= nfft:
        return 0, n1
    glo = gmin % nfft
    a0, a1 = glo >> ln2, (glo + gmax - gmin) >> ln2
    return (0, n1) if a1 - a0 + 1 >= n1 else (a0, a1 - a0 + 1)


def sizes(p, rowcap):
    """(Bmax, csmax) for the largest group."""
    bmax = csmax = 0
    for g in p["groups"]:
        nrow = min(rowcap, g["r1"] - g["r0"])
        lrow = 12 - min(g["lnfft"], 12)
        bmax = max(bmax, -(-g["P"] * nrow // (1 << lrow)) << lrow << g["lnfft"])
        csmax = max(csmax, p["nharm"] * nrow * g["nseg"])
    return bmax, csmax


HS = (1e-7, 3.0, -1000.0, 1000.0)  # delta, f0, dt[0], dt[n-1]: narrow cell ranges at every n


# ---------------------------------------------------------------- (n, P) per segment
@pytest.mark.parametrize("eps,pmax,nharm,spread", [(EPS, 24, 1, GATHER), (EPS, 16, 1, MFMA), (EPS_ZM, 24, 2, GATHER)])
def test_n_and_moments_per_segment(plan_check, eps, pmax, nharm, spread):
    for nseg in SEGMENTS:
        p = run_plan(plan_check, HS, 10000, nseg, nharm=nharm, spread=spread)
        assert p["applicable"] == 1 and len(p["groups"]) == 1
        g = p["groups"][0]
        l, P = least_np(nseg, pmax, eps)
        assert (g["lnfft"], g["P"]) == (l, P), nseg
        assert (1 << l) >= nseg and trunc(math.pi * max(nseg // 2, nseg - 1 - nseg // 2) / 2.0 ** l, P) <= eps
        assert (p["last_n"], p["last_p"], p["gather"]) == (1 << l, P, 1 if spread == GATHER else 0)
        assert g["invfact"] == 2.4 / (2.0 ** P * math.factorial(P))
        assert g["s1"] == float(1 << l) * HS[0]
        assert (g["ln2"], g["ln1"]) == (min(l, 12), l - min(l, 12))


def test_restated_and_recorded_plans(plan_check):
    got = {s: least_np(s, 24, EPS) for s in (1401, 3000, 5000, 80000, 600000, 1200000)}
    assert got == {1401: (11, 14), 3000: (12, 14), 5000: (13, 13), 80000: (17, 13), 600000: (20, 13),
                   1200000: (21, 13)}
    hs = (1e-7, 7.0, -5e5, 5e5)
    p = run_plan(plan_check, hs, 10 ** 7, 10 ** 6, nharm=2)  # config 3: Z^2_2, the cell gather
    assert (p["last_n"], p["last_p"], p["gather"]) == (1 << 20, 14, 1)
    p = run_plan(plan_check, hs, 10 ** 7, 10 ** 6, nharm=1)  # 5e-14
    assert (p["last_n"], p["last_p"]) == (1 << 20, 15)
    hs4 = (1e-8, 7.0, -5e6, 5e6)
    p = run_plan(plan_check, hs4, 10 ** 8, 10 ** 5, rows=100, nharm=20, stat=1)  # config 4: H_20, MFMA slots
    assert (p["last_n"], p["last_p"], p["gather"]) == (1 << 17, 14, 0)


# ---------------------------------------------------------------- declines
def test_declines(plan_check):
    ok = run_plan(plan_check, HS, 10000, 1401)
    assert ok["applicable"] == 1
    for hs in [(0.0,) + HS[1:], (-1e-7,) + HS[1:], (math.nan,) + HS[1:], (math.inf,) + HS[1:],
               (HS[0], math.nan) + HS[2:], (HS[0], -math.inf) + HS[2:]]:
        assert run_plan(plan_check, hs, 10000, 1401)["applicable"] == 0, hs
    assert run_plan(plan_check, HS, 10000, 1401, unsorted=1)["applicable"] == 0
    # a segment under 64 trials: a short row, or the first / last row of a cut range
    assert run_plan(plan_check, HS, 10000, 63)["applicable"] == 0
    assert run_plan(plan_check, HS, 10000, 64)["applicable"] == 1
    assert run_plan(plan_check, HS, 10000, 200, rows=3, first=137, count=463)["applicable"] == 0
    assert run_plan(plan_check, HS, 10000, 200, rows=3, first=136, count=464)["applicable"] == 1
    assert run_plan(plan_check, HS, 10000, 200, rows=3, first=0, count=463)["applicable"] == 0
    # delta = 2^-11 at n = 2^11: s1 = 1, the cell of harmonic k is k dt. Harmonics 1 .. nharm + 1 are planned.
    d = 2.0 ** -11
    glim = 2147483647 - 2048
    assert run_plan(plan_check, (d, 3.0, 0.0, 5.0), 10000, 1401, nharm=1)["groups"][0]["lnfft"] == 11
    assert run_plan(plan_check, (d, 3.0, (glim - 1) / 2 - 100, (glim - 1) / 2), 10000, 1401, nharm=1)["applicable"] == 1
    assert run_plan(plan_check, (d, 3.0, glim / 2 - 100, glim / 2), 10000, 1401, nharm=1)["applicable"] == 0
    assert run_plan(plan_check, (d, 3.0, -glim / 2, -glim / 2 + 100), 10000, 1401, nharm=1)["applicable"] == 0
    assert run_plan(plan_check, (d, 3.0, -(glim - 1) / 2, -glim / 2 + 100), 10000, 1401, nharm=1)["applicable"] == 1
    # wraps of harmonic 2: (gmax - gmin) // n + 1 <= 32
    assert run_plan(plan_check, (d, 3.0, 0.0, 32767.0), 10000, 1401, nharm=1)["applicable"] == 1
    assert run_plan(plan_check, (d, 3.0, 0.0, 32768.0), 10000, 1401, nharm=1)["applicable"] == 0
    # gmax < gmin
    assert run_plan(plan_check, (d, 3.0, 5.0, 4.0), 10000, 1401, nharm=1)["applicable"] == 0
    assert run_plan(plan_check, (d, 3.0, 5.0, 5.0), 10000, 1401, nharm=1)["applicable"] == 1


# ---------------------------------------------------------------- row groups and batches
RANGES = [  # nf, rows, first, count, spread, expected groups as (r0, r1, j0, nseg)
    (1401, 1, 0, None, AUTO, [(0, 1, 0, 1401)]),
    (300, 2, 0, None, AUTO, [(0, 2, 0, 300)]),
    (300, 20, 0, None, AUTO, [(0, 20, 0, 300)]),
    (300, 5, 0, None, GATHER, [(0, 5, 0, 300)]),
    (200, 4, 100, 600, AUTO, [(0, 1, 100, 100), (1, 3, 0, 200), (3, 4, 0, 100)]),
    (200, 4, 100, 600, GATHER, [(0, 1, 100, 100), (1, 3, 0, 200), (3, 4, 0, 100)]),
    (200, 12, 0, 2300, AUTO, [(0, 11, 0, 200), (11, 12, 0, 100)]),
    (200, 3, 70, 130, AUTO, [(0, 1, 70, 130)]),
    (200, 3, 70, 100, AUTO, [(0, 1, 70, 100)]),
]


@pytest.mark.parametrize("nf,rows,first,count,spread,want", RANGES)
def test_row_groups_and_batches(plan_check, nf, rows, first, count, spread, want):
    p = run_plan(plan_check, HS, 20000, nf, rows=rows, nharm=3, stat=1, first=first, count=count, spread=spread)
    assert p["applicable"] == 1
    count = p["count"]
    assert [(g["r0"], g["r1"], g["j0"], g["nseg"]) for g in p["groups"]] == want
    gather = p["gather"] == 1
    assert gather == (spread == GATHER or (spread == AUTO and rows <= 2))
    step = 2 if gather else 8
    seen = np.zeros(rows * nf, dtype=int)
    tb = 0
    for g in p["groups"]:
        assert (g["h"], g["jbase"]) == (g["nseg"] // 2, g["j0"] + g["nseg"] // 2)
        assert [b["rb"] for b in g["batches"]] == list(range(g["r0"], g["r1"], step))
        for b in g["batches"]:
            assert b["nrow"] == min(step, g["r1"] - b["rb"])
            # the batch's trials, in the order of the call's range
            assert (b["tb0"], b["nbt"]) == (tb, b["nrow"] * g["nseg"])
            assert b["tb0"] + first == b["rb"] * nf + g["j0"]
            tb += b["nbt"]
            for r in range(b["rb"], b["rb"] + b["nrow"]):
                seen[r * nf + g["j0"]:r * nf + g["j0"] + g["nseg"]] += 1
            assert (len(b["sets"]) > 0, len(b["mfma"]) > 0) == (gather, not gather)
    assert tb == count
    assert seen[first:first + count].tolist() == [1] * count and seen.sum() == count
    # the fused finalize: rows of 2048 and 4096 only; every batch of the other groups finalizes separately
    assert all(g["fuse"] == int(g["ln2"] >= 11) for g in p["groups"])
    assert p["separate_batches"] == sum(len(g["batches"]) for g in p["groups"] if not g["fuse"])


def test_row_shard_plans_what_the_whole_grid_plans(plan_check):
    whole = run_plan(plan_check, HS, 20000, 300, rows=20, nharm=3)
    shard = run_plan(plan_check, HS, 20000, 300, rows=20, nharm=3, first=8 * 300, count=9 * 300)
    (gw,), (gs,) = whole["groups"], shard["groups"]
    assert (gs["r0"], gs["r1"]) == (8, 17)
    for key in ("j0", "nseg", "h", "lnfft", "P", "ln1", "ln2", "fuse", "jbase", "invfact", "s1", "fch", "fcl", "gmin",
                "gmax"):
        assert gs[key] == gw[key], key
    assert whole["gather"] == shard["gather"] == 0
    # a two-row shard of a 20-row grid keeps the whole grid's spread form (MFMA slots)
    assert run_plan(plan_check, HS, 20000, 300, rows=20, nharm=3, first=300, count=600)["gather"] == 0
    # fc = f0 + (j0 + h) delta as a double-double
    from fractions import Fraction
    fc = Fraction(HS[1]) + (gw["j0"] + gw["h"]) * Fraction(HS[0])
    assert abs(Fraction(gw["fch"]) + Fraction(gw["fcl"]) - fc) <= Fraction(2.0 ** -100)


def test_fused_finalize_and_best_partials(plan_check):
    """Rows of 2048 / 4096 fuse the finalize unless a hook forbids it; the per-block best candidates follow."""
    for nf, ln1, ln2 in ((1401, 0, 11), (3000, 0, 12), (5000, 1, 12), (1000, 0, 10)):
        for generic, separate in ((0, 0), (1, 0), (0, 1)):
            p = run_plan(plan_check, HS, 20000, nf, rows=3, nharm=2, best=1, generic=generic, separate=separate)
            g = p["groups"][0]
            assert (g["ln1"], g["ln2"]) == (ln1, ln2)
            fuse = ln2 >= 11 and not generic and not separate
            assert g["fuse"] == int(fuse)
            nb = len(g["batches"])
            assert p["separate_batches"] == (0 if fuse else nb)
            assert p["best_alloc"] == max(1, 3 << ln1)
            assert p["best_count"] == ((3 << ln1) if fuse else 0)
            base = 0
            for b in g["batches"]:
                assert b["best_base"] == (base if fuse else 0)
                base += b["nrow"] << ln1
    assert run_plan(plan_check, HS, 20000, 3000, best=0)["best_alloc"] == 0


# ---------------------------------------------------------------- start tables
@pytest.mark.parametrize("nf,rows,first,count,nharm", [(1401, 1, 0, None, 2), (5000, 2, 0, None, 5),
                                                       (200, 4, 100, 600, 9), (300, 2, 100, 400, 1)])
def test_start_tables(plan_check, nf, rows, first, count, nharm):
    hs = (2.0 ** -21, 3.25, -2048.0, 2047.5)
    p = run_plan(plan_check, hs, 8000, nf, rows=rows, nharm=nharm, first=first, count=count, spread=GATHER)
    assert p["applicable"] == 1 and p["gather"] == 1
    taken = []
    tot_all, tot_max = 0, 0
    for g in p["groups"]:
        assert len(g["gmin"]) == len(g["gmax"]) == nharm + 1  # one harmonic past nharm is planned
        off = 0
        for k in range(1, nharm + 2):
            assert (g["gmin"][k - 1], g["gmax"][k - 1]) == cells(hs, g["lnfft"], k)
        for k in range(1, nharm + 1):
            size = g["gmax"][k - 1] - g["gmin"][k - 1] + 2
            assert g["soff"][k - 1] == off
            taken.append((g["starts_off"] + off, g["starts_off"] + off + size))
            off += size
        assert g["starts_off"] == tot_all
        tot_all += off
        tot_max = max(tot_max, off)
        # the cell-start launches: four harmonics each, the tables' own cells and offsets
        assert [c["k0"] for c in g["cells"]] == list(range(1, nharm + 1, 4))
        for c in g["cells"]:
            ks = range(c["k0"], min(c["k0"] + 4, nharm + 1))
            assert c["nk"] == len(ks)
            assert c["gmin"] == [g["gmin"][k - 1] for k in ks]
            assert c["span"] == [g["gmax"][k - 1] - g["gmin"][k - 1] + 1 for k in ks]
            assert c["off"] == [g["soff"][k - 1] for k in ks]
    taken.sort()
    assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:]))  # disjoint
    assert (p["starts_all"], p["starts_max"]) == (tot_all, tot_max)
    assert p["cell_tables"] == nharm * len(p["groups"])
    assert p["cell_cap"] == min(BUDGET // 32, 64 << 20)
    assert p["launches"][0] == sum(len(g["cells"]) for g in p["groups"])


# ---------------------------------------------------------------- gather sets
def lanes_rule(n, set_cells, kspan, nfft):
    ppc = n // max(1, min(kspan, nfft))
    L = 1
    while L < 4 and set_cells * 2 * L <= (1 << 20) and ppc >= 8 * L:
        L *= 2
    return L


GATHER_CASES = [  # hs, n, nf, rows, nharm, lanes hook
    ((2.0 ** -21, 3.25, -2048.0, 2047.5), 8000, 1401, 1, 2, 0),      # 2^11, few photons per cell: one lane
    ((2.0 ** -21, 3.25, -2048.0, 2047.5), 8000, 5000, 2, 3, 0),      # 2^13: cells around 0 wrap into both FFT rows
    ((2.0 ** -21, 3.25, 1000.0, 2047.5), 8000, 5000, 1, 3, 0),       # cells 4 .. 24: one FFT row of the two
    ((2.0 ** -14, 3.25, -2048.0, 2047.5), 100000, 1401, 1, 11, 0),   # wraps the grid; two sets of harmonics
    ((2.0 ** -26, 3.25, -2048.0, 2047.5), 1000000, 3000, 1, 2, 0),   # dense cells: 4 lanes
    ((2.0 ** -12, 3.25, -2048.0, 2047.5), 50000, 3000, 1, 2, 0),     # 12 photons per cell: 2 lanes
    ((2.0 ** -26, 3.25, -2048.0, 2047.5), 1000000, 3000, 1, 2, 8),   # the hook
    ((2.0 ** -26, 3.25, -2048.0, 2047.5), 1000000, 3000, 1, 2, 1),
]


def check_gather_sets(plan_check, hs, n, nf, rows, nharm, lanes):
    """Every set of the case against the definitions; returns the lane counts met."""
    p = run_plan(plan_check, hs, n, nf, rows=rows, nharm=nharm, spread=GATHER, lanes=lanes)
    assert p["applicable"] == 1
    bmax, csmax = sizes(p, 8)
    assert (p["Bmax"], p["csmax"]) == (bmax, csmax)
    assert p["gw"] == min(nharm, 8)  # the default budget holds every plane of these plans
    seen_lanes = set()
    for g in p["groups"]:
        nfft = 1 << g["lnfft"]
        assert nfft <= 1 << 13
        for b in g["batches"]:
            assert [k for s in b["sets"] for k in s["k"]] == list(range(1, nharm + 1))
            assert [s["nk"] for s in b["sets"]] == [min(8, nharm - k0 + 1) for k0 in range(1, nharm + 1, 8)]
            for s in b["sets"]:
                blocks = 0
                assert len(set(s["woff"])) == s["nk"] and s["woff"] == [j * bmax for j in range(s["nk"])]
                for j, k in enumerate(s["k"]):
                    gmin, gmax = g["gmin"][k - 1], g["gmax"][k - 1]
                    assert (s["gmin"][j], s["gmax"][j], s["soff"][j]) == (gmin, gmax, g["soff"][k - 1])
                    # every wrapped cell of [gmin, gmax] is one of the gcount cells from gbase (mod n), whole FFT rows
                    wrapped = np.unique(np.arange(gmin, gmax + 1) % nfft)
                    covered = (wrapped - s["gbase"][j]) % nfft < s["gcount"][j]
                    assert covered.all()
                    assert s["gbase"][j] % (1 << g["ln2"]) == 0 and s["gcount"][j] % (1 << g["ln2"]) == 0
                    alo, acnt = occupied(gmin, gmax, g["lnfft"], g["ln1"])
                    assert (s["gbase"][j], s["gcount"][j]) == (alo << g["ln2"], acnt << g["ln2"])
                    L = lanes or lanes_rule(n, sum(s["gcount"]), gmax - gmin + 1, nfft)
                    assert 1 << s["lanes_log2"][j] == L
                    seen_lanes.add(L)
                    assert s["blk0"][j] == blocks
                    blocks += -(-s["gcount"][j] * L // 256)
                assert s["blocks"] == blocks
    return seen_lanes


@pytest.mark.parametrize("hs,n,nf,rows,nharm,lanes", GATHER_CASES)
def test_gather_sets(plan_check, hs, n, nf, rows, nharm, lanes):
    assert check_gather_sets(plan_check, hs, n, nf, rows, nharm, lanes)


def test_gather_lanes_rule_reaches_every_width(plan_check):
    got = set()
    for case in GATHER_CASES:
        got |= check_gather_sets(plan_check, *case)
    assert got == {1, 2, 4, 8}
    # at 2^13 both FFT rows where the cells wrap around 0, one of the two for a narrow range inside a row
    p = run_plan(plan_check, GATHER_CASES[1][0], 8000, 5000, rows=2, nharm=3, spread=GATHER)
    assert p["groups"][0]["batches"][0]["sets"][0]["gcount"] == [8192] * 3
    p = run_plan(plan_check, GATHER_CASES[2][0], 8000, 5000, rows=1, nharm=3, spread=GATHER)
    assert p["groups"][0]["batches"][0]["sets"][0]["gcount"] == [4096] * 3


def test_gather_width_shrinks_under_a_small_budget(plan_check):
    hs = (2.0 ** -21, 3.25, -2048.0, 2047.5)
    full = run_plan(plan_check, hs, 8000, 3000, nharm=8, stat=1, spread=GATHER)
    bmax, csmax = sizes(full, 8)
    assert full["gw"] == 8 and len(full["groups"][0]["batches"][0]["sets"]) == 1
    for planes in (9, 8, 5, 3, 2, 1):  # a budget that holds this many planes of Bmax beside the sums
        budget = planes * bmax * 16 + csmax * 16
        p = run_plan(plan_check, hs, 8000, 3000, nharm=8, stat=1, spread=GATHER, budget=budget)
        gw = max(1, planes - 1)
        assert p["gw"] == gw
        sets = p["groups"][0]["batches"][0]["sets"]
        assert [s["nk"] for s in sets] == [min(gw, 8 - k0 + 1) for k0 in range(1, 9, gw)]
        assert p["launches"][1] == len(sets)
        assert p["cell_cap"] == min(budget // 32, 64 << 20)


# ---------------------------------------------------------------- MFMA passes
def check_mfma(p, budget):
    """The passes of every batch; returns their sizes."""
    nharm, nchunk = p["nharm"], -(-p["n"] // 1024)
    assert p["nchunk"] == nchunk and p["gather"] == 0 and p["gw"] == 1
    bmax, csmax = sizes(p, 8)
    assert (p["Bmax"], p["csmax"]) == (bmax, csmax)
    fixed = 2 * bmax * 16 + csmax * 16
    ubytes, ipass, sizes_ = 0, 0, None
    for g in p["groups"]:
        for b in g["batches"]:
            gls = [m["gl"] for m in b["mfma"]]
            assert set(gls) <= {10, 8, 6, 4, 2}
            k = 1
            for m in b["mfma"]:
                assert (m["k0"], m["ipass"]) == (k, ipass)
                k += m["gl"]
                ipass += 1
                SL = 2 * g["P"] * b["nrow"]
                need = [(g["gmax"][kk - 1] - g["gmin"][kk - 1] + 1 + nchunk) * SL for kk in range(m["k0"], m["k0"] + m["gl"])]
                assert m["gmin"] == [g["gmin"][kk - 1] for kk in range(m["k0"], m["k0"] + m["gl"])]
                assert m["ubase"] == [sum(need[:i]) for i in range(m["gl"])]  # back to back: disjoint
                SLmax = 2 * g["P"] * min(8, g["r1"] - g["r0"])
                ubytes = max(ubytes, sum(need) // SL * SLmax * 8)
            assert k - 1 in (nharm, nharm + 1)  # harmonics 1..nharm, at most one past it
            assert sizes_ in (None, gls)
            sizes_ = gls
    assert p["npass"] == ipass
    assert p["ubytes"] == ubytes
    assert max(sizes_) == 2 or ubytes + fixed <= budget
    return sizes_


@pytest.mark.parametrize("nharm,want", [(20, [10, 10]), (1, [2]), (2, [2]), (3, [4]), (5, [6]), (7, [8]), (9, [10]),
                                        (13, [10, 4]), (16, [10, 6]), (11, [10, 2])])
def test_mfma_passes(plan_check, nharm, want):
    p = run_plan(plan_check, HS, 50000, 300, rows=11, nharm=nharm, stat=1)
    assert check_mfma(p, BUDGET) == want
    assert p["launches"][1] == 2 * len(want) and p["launches"][2] == 2 * nharm and p["launches"][0] == 0


def test_mfma_passes_shrink_under_a_small_budget(plan_check):
    hs = (2.0 ** -14, 3.25, -2048.0, 2047.5)
    full = run_plan(plan_check, hs, 50000, 3000, rows=3, nharm=20, stat=1, spread=MFMA)
    assert check_mfma(full, BUDGET) == [10, 10]
    bmax, csmax = sizes(full, 8)
    fixed = 2 * bmax * 16 + csmax * 16
    got = []
    for frac in (1.0, 0.9, 0.5, 0.3, 0.05):
        budget = fixed + int(full["ubytes"] * frac)
        p = run_plan(plan_check, hs, 50000, 3000, rows=3, nharm=20, stat=1, spread=MFMA, budget=budget)
        got.append(check_mfma(p, budget))
    assert got[0] == [10, 10] and got[1] == [8, 8, 4] and got[2] == [4] * 5 and got[3] == [2] * 10 == got[4]


# ---------------------------------------------------------------- work and launch counts
def test_work_and_launches_config3(plan_check):
    """1e7 photons, 1e6 trials, Z^2_2, one row (the benchmark's config 3): DESIGN.md 5.3's formulas."""
    hs = (1e-7, 7.0, -5e5, 5e5)
    n, nf, m = 10 ** 7, 10 ** 6, 2
    p = run_plan(plan_check, hs, n, nf, nharm=m, best=1)
    (g,) = p["groups"]
    P, nfft = 14, 1 << 20
    assert (g["lnfft"], g["P"], g["ln1"], g["ln2"], g["fuse"]) == (20, P, 8, 12, 1)
    plane = 16 * P * nfft
    occ = [occupied(*cells(hs, 20, k), 20, 8)[1] for k in (1, 2)]
    assert 0 < occ[0] < occ[1] < 256  # a tenth and a fifth of the grid
    work = dict(zip(CLASSES, p["work"][:]))
    assert p["work"][4] == 509762048.0 == 2 * plane + 16 * nf + (16 * (m - 1) + 8) * nf
    assert p["launches"] == [1, 1, 0, 2, 2, 0, 0]
    assert p["work"][4] / p["launches"][4] == 254881024.0
    assert p["work"][3] == sum(plane * a // 256 + plane for a in occ)
    assert p["work"][0] == m * (40 + 5 * P) * n  # "cellstart" slot: the spread's flops
    assert p["work"][1] == sum(8 * n + 16 * P * (a << 12) for a in occ)
    assert p["work"][2] == 0 and p["work"][5] == 0 and p["work"][6] == 0
    assert (p["gw"], p["best_alloc"], p["best_count"], p["separate_batches"]) == (2, 256, 256, 0)
    del work
    for hook in ({"separate": 1}, {"generic": 1}):
        q = run_plan(plan_check, hs, n, nf, nharm=m, best=1, **hook)
        assert q["work"][4] == 2 * plane + 2 * 16 * nf
        assert q["work"][6] == 16 * m * nf + 8 * nf
        assert q["launches"] == [1, 1, 0, 2, 2, 0, 1]
        assert q["work"][:4] == p["work"][:4]
        assert (q["best_count"], q["separate_batches"]) == (0, 1)


def test_work_and_launches_mfma(plan_check):
    """A 2-D grid on the MFMA slots, two row batches: the slot bytes of every harmonic spread (one past nharm with
    its pass), merged only up to nharm."""
    hs = (2.0 ** -21, 3.25, -2048.0, 2047.5)
    n, nf, rows, m = 8000, 3000, 11, 5
    p = run_plan(plan_check, hs, n, nf, rows=rows, nharm=m, stat=1)
    (g,) = p["groups"]
    P, nfft, nchunk = g["P"], 1 << g["lnfft"], -(-n // 1024)
    assert (g["lnfft"], g["ln1"], g["fuse"]) == (12, 0, 1) and check_mfma(p, BUDGET) == [6]
    flops = sbytes = mbytes = p2 = 0
    for nrow in (8, 3):
        SL = 2 * P * nrow
        slots = [8 * SL * (g["gmax"][k - 1] - g["gmin"][k - 1] + 1 + nchunk) for k in range(1, 7)]
        flops += 512 * n * 6
        sbytes += 8 * n + sum(slots)
        mbytes += sum(slots[:m]) + m * 16 * P * nrow * nfft
        p2 += m * 16 * P * nrow * nfft + (m - 1) * 16 * nrow * nf + (16 * (m - 1) + 8) * nrow * nf
    assert p["work"] == [flops, sbytes, mbytes, 0, p2, 0, 0]
    assert p["launches"] == [0, 2, 2 * m, 0, 2 * m, 0, 0]
