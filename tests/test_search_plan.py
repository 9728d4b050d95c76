"""The host plans of the exact i8 search, the fp64 direct search and the fp64 fix-up (csrc/search_plan.h) on the CPU.

`make -C crimp_amd/csrc search-plan-check` builds search_plan_check.cpp with the host compiler under
-fsanitize=address,undefined; every case below is one run of that program (no GPU, no preloaded library, no
environment hook: the budget, the CU count and the long-splits hook are fields of the case). What it prints must equal,
number for number, the rules restated here in Python (integer arithmetic and one comparison of doubles), and the
invariants the launch side relies on are asserted directly.

The budget invariant is asserted on the block size before it is rounded up: the direct search rounds its even-sized
trial blocks up to whole 256-trial kernel blocks and the exact search to whole 2048-trial tiles, so a block's buffer may
exceed CRIMP_SEARCH_BUDGET_MB by less than one kernel block (tile) of trials (nharm 20 at 1 MiB: 3276 trials fit, the
exact search takes 4096). The fix-up does not round and holds the budget as it stands."""
import functools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "crimp_amd", "csrc")
MIB = 1 << 20
BUDGETS = (MIB, 4 * MIB, 2048 * MIB)
FOLD = 245760            # photons between the exact kernel's int64 folds (15 carry periods of 16384)
TILE = 2048              # trials per tile of the exact kernel
PHOTONS = (1, 4096, 4097, 16383, 16384, FOLD, FOLD + 1, 2 ** 27 - 1, 2 ** 27, 2 ** 28 + 5)


@pytest.fixture(scope="module")
def plan_check():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    r = subprocess.run(["make", "-s", "-B", "-C", CSRC, "search-plan-check"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(CSRC, "build", "search_plan_check")


def run_plan(exe, kind, n, nf=1, nharm=2, first=0, count=1, ncu=256, budget=2048 * MIB, long_splits=0):
    """One case through the check program -> the plan as a dict (an exact plan's blocks as a list of dicts)."""
    text = "%s %d %d %d %d %d %d %d %d\n" % (kind, n, nf, nharm, first, count, ncu, budget, long_splits)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0, text + r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    p = {}
    for ln in r.stdout.splitlines():
        key, *v = ln.split()
        if key == "block":
            names = ("bfirst", "bcount", "tf", "nt", "bpg", "chunk", "splits")
            p.setdefault("blocks", []).append(dict(zip(names, (int(t) for t in v))))
        elif key == "error":
            p["error"] = (int(v[0]), " ".join(v[1:]))
        else:
            p[key] = int(v[0])
    return p


# ---------------------------------------------------------------- the rules, restated
def cdiv(a, b):
    return -(-a // b)


def direct(n, nharm, count, budget):
    s0 = max(1, min(64, n // 16384))
    chunk = cdiv(cdiv(n, s0), 32) * 32
    splits = cdiv(n, chunk)
    cbmax = max(256, budget // (8 * splits * 2 * nharm))
    return {"chunk": chunk, "splits": splits, "cb": min(count, cdiv(cdiv(count, cdiv(count, cbmax)), 256) * 256)}


def fixup(n, nharm, budget):
    chunk = cdiv(n, max(1, min(1024, n // 4096)))
    splits = cdiv(n, chunk)
    return {"chunk": chunk, "splits": splits, "cbmax": max(1, min(65535, budget // (8 * splits * 2 * nharm)))}


def fill(n, bpg, ncu, lo, hi, max_chunk):
    """The fullest last round of bpg x splits blocks on ncu CUs among the split counts lo..hi; more splits must gain
    0.5 % (a comparison of doubles: the quotient of two integers below 2^53 rounds in Python as in C)."""
    best, best_eff = None, -1.0
    for want in range(lo, hi + 1):
        chunk = cdiv(cdiv(n, want), 32) * 32
        splits = cdiv(n, chunk)
        blocks = bpg * splits
        eff = blocks / (cdiv(blocks, ncu) * ncu)
        if (max_chunk is None or chunk <= max_chunk) and eff > best_eff + 0.005:
            best, best_eff = {"chunk": chunk, "splits": splits}, eff
    return best


@functools.lru_cache(maxsize=None)
def _split(n, bpg, ncu, long_splits):
    smax_n = max(1, min(cdiv(n, 4096), 65535))
    srounds = cdiv(8 * ncu, bpg)
    snofold = cdiv(n, FOLD)
    if not long_splits and snofold <= 65535 and bpg * snofold <= 131072:
        lo = max(1, snofold, min(srounds, smax_n))
        best = fill(n, bpg, ncu, lo, min(smax_n, lo + lo // 4 + 1), FOLD)
        if best:
            return best
    smax = max(1, min(smax_n, 8192 // bpg))
    smin = max(1, min(srounds, smax))
    return fill(n, bpg, ncu, smin, min(smax, 4 * smin), None)


def split(n, bpg, ncu, long_splits):
    return dict(_split(n, bpg, ncu, bool(long_splits)))


def tile_of(g, nf):
    """The tile of flat trial g: every grid row starts a new tile."""
    return (g // nf) * cdiv(nf, TILE) + (g % nf) // TILE


def exact(n, nf, nharm, first, count, ncu, budget, long_splits):
    nchunk = cdiv(n, 2 ** 27 - 1)
    pc = cdiv(n, nchunk)
    want = max(TILE, budget // (8 * 2 * nharm * nchunk))
    while True:
        cb = min(count, cdiv(cdiv(count, cdiv(count, want)), TILE) * TILE)
        blocks, fold_blocks, fits = [], 0, True
        for b0 in range(0, count, cb):
            k = {"bfirst": first + b0, "bcount": min(cb, count - b0)}
            k["tf"] = tile_of(k["bfirst"], nf)
            k["nt"] = tile_of(k["bfirst"] + k["bcount"] - 1, nf) - k["tf"] + 1
            k["bpg"] = cdiv(k["nt"], 4)
            fits = k["bpg"] <= 8192
            k.update(split(pc, k["bpg"], ncu, long_splits))
            if k["chunk"] > FOLD:
                fold_blocks = max(fold_blocks, k["bpg"] * k["splits"])
            blocks.append(k)
            if not fits:
                break
        if fits:
            break
        if cb <= TILE:
            return {"error": (-1, "exact search: trial block does not fit one launch")}
        want = cb // 2
    if fold_blocks > 8192:
        return {"error": (-2, "exact search: fold scratch bound")}
    return {"nchunk": nchunk, "pc": pc, "tpr": cdiv(nf, TILE), "cb": cb, "fold_blocks": fold_blocks,
            "tot_elems": 2 * nharm * cb * nchunk, "flagged_elems": count, "fold_elems": fold_blocks * 4 * 64 * 64,
            "blocks": blocks}


# ---------------------------------------------------------------- the invariants
def check_photon_splits(p, n):
    assert (p["splits"] - 1) * p["chunk"] < n <= p["splits"] * p["chunk"], (p, n)


def check_exact(p, n, nf, nharm, first, count, budget, long_splits):
    nchunk, pc, cb = p["nchunk"], p["pc"], p["cb"]
    assert pc < 2 ** 27 and nchunk * pc >= n and (nchunk - 1) * pc < n
    assert cb % TILE == 0 or cb == count
    # the budget bounds the even block size; the tile rounding adds less than one tile (the module docstring)
    assert cb == TILE or cb - (TILE - 1) <= budget // (8 * 2 * nharm * nchunk)
    assert p["tot_elems"] == 2 * nharm * cb * nchunk and p["flagged_elems"] == count
    nxt, fold_blocks = first, 0
    for k in p["blocks"]:
        assert k["bfirst"] == nxt and 1 <= k["bcount"] <= cb                       # a partition of the range
        nxt += k["bcount"]
        assert k["tf"] == tile_of(k["bfirst"], nf)
        assert k["nt"] == tile_of(nxt - 1, nf) - k["tf"] + 1
        assert k["bpg"] == cdiv(k["nt"], 4) <= 8192
        assert k["chunk"] % 32 == 0 and 1 <= k["splits"] <= 65535
        check_photon_splits(k, pc)
        if not long_splits and cdiv(pc, FOLD) * k["bpg"] <= 131072:
            assert k["chunk"] <= FOLD
        if k["chunk"] > FOLD:
            fold_blocks = max(fold_blocks, k["bpg"] * k["splits"])
    assert nxt == first + count
    assert all(k["bcount"] == cb for k in p["blocks"][:-1])
    assert p["fold_blocks"] == fold_blocks <= 8192
    assert p["fold_elems"] == fold_blocks * 4 * 64 * 64                           # <= 1 GiB of int64


def exact_case(exe, n, nf, nharm, first, count, ncu, budget, long_splits):
    p = run_plan(exe, "exact", n, nf, nharm, first, count, ncu, budget, long_splits)
    assert p == exact(n, nf, nharm, first, count, ncu, budget, long_splits)
    check_exact(p, n, nf, nharm, first, count, budget, long_splits)
    return p


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("nharm", [1, 20, 256])
def test_direct_and_fixup(plan_check, nharm):
    """The n / 16384 and n / 4096 split floors, the photon counts around them and far above, every budget."""
    for n in PHOTONS:
        for budget in BUDGETS:
            for count in (1, 255, 256, 257, 3000, 100000):
                p = run_plan(plan_check, "direct", n, nharm=nharm, count=count, budget=budget)
                assert p == direct(n, nharm, count, budget)
                check_photon_splits(p, n)
                assert p["chunk"] % 32 == 0 and p["splits"] <= 64
                cb, cap = p["cb"], budget // (8 * p["splits"] * 2 * nharm)
                assert cb % 256 == 0 or cb == count
                assert cb <= 256 or cb - 255 <= cap
                assert 1 <= cb <= count                       # blocks [b0, min(b0 + cb, count)) tile [0, count)
            p = run_plan(plan_check, "fixup", n, nharm=nharm, budget=budget)
            assert p == fixup(n, nharm, budget)
            check_photon_splits(p, n)
            assert p["splits"] <= 1024 and 1 <= p["cbmax"] <= 65535
            assert 8 * p["splits"] * 2 * nharm * p["cbmax"] <= budget or p["cbmax"] == 1


def test_gpu_test_plans(plan_check):
    """The plans tests/test_gpu_search_blocks.py relies on (40 000 photons, H_20, 1 MiB against the default): 3000
    direct trials in blocks of 1536 + 1464, 2048 fix-up trials in 6 blocks of 364."""
    assert run_plan(plan_check, "direct", 40000, nharm=20, count=3000, budget=MIB) == \
        {"chunk": 20000, "splits": 2, "cb": 1536}
    assert run_plan(plan_check, "direct", 40000, nharm=20, count=3000)["cb"] == 3000
    p = run_plan(plan_check, "fixup", 40000, nharm=20, budget=MIB)
    assert p == {"chunk": 4445, "splits": 9, "cbmax": 364} and cdiv(2048, p["cbmax"]) == 6
    assert run_plan(plan_check, "fixup", 40000, nharm=20)["cbmax"] >= 2048


@pytest.mark.parametrize("ncu", [256, 304])
@pytest.mark.parametrize("bpg", [1, 123, 8192])
def test_split_exact(plan_check, bpg, ncu):
    """Block columns against the CU count, every photon count up to one photon chunk, the fold path on and off."""
    for n in PHOTONS[:8] + (10 ** 7, 3 * 10 ** 5, 10 ** 8):
        for long_splits in (0, 1):
            p = run_plan(plan_check, "split", n, nf=bpg, ncu=ncu, long_splits=long_splits)
            assert p == split(n, bpg, ncu, long_splits), (n, bpg, ncu, long_splits)
            check_photon_splits(p, n)
            assert p["chunk"] % 32 == 0 and p["splits"] <= 65535
            assert p["splits"] <= cdiv(n, 4096)
            if not long_splits and cdiv(n, FOLD) * bpg <= 131072:
                assert p["chunk"] <= FOLD
            if p["chunk"] > FOLD:
                assert bpg * p["splits"] <= 8192


def test_split_exact_anchors(plan_check):
    """Recorded plans at 256 CUs (config 3's 123 block columns first), default and with the long-splits hook."""
    for n, bpg, default, long_ in [(10 ** 7, 123, (192320, 52), (370400, 27)),
                                   (3 * 10 ** 5, 8192, (150016, 2), (300000, 1)),
                                   (10 ** 8, 16, (240416, 416), (781280, 128)),
                                   (1, 1, (32, 1), None), (4097, 1, (2080, 2), None)]:
        p = run_plan(plan_check, "split", n, nf=bpg)
        assert (p["chunk"], p["splits"]) == default
        if long_:
            p = run_plan(plan_check, "split", n, nf=bpg, long_splits=1)
            assert (p["chunk"], p["splits"]) == long_


def test_exact_config3(plan_check):
    """Config 3 (1e7 photons, 1e6 trials, Z^2_2) at 256 CUs: one block of 489 tiles in 123 block columns, 52 splits that
    never fold; the long-splits hook gives 27 folding splits and their scratch."""
    p = exact_case(plan_check, 10 ** 7, 10 ** 6, 2, 0, 10 ** 6, 256, 2048 * MIB, 0)
    assert p["blocks"] == [dict(bfirst=0, bcount=10 ** 6, tf=0, nt=489, bpg=123, chunk=192320, splits=52)]
    assert p["fold_blocks"] == 0
    p = exact_case(plan_check, 10 ** 7, 10 ** 6, 2, 0, 10 ** 6, 256, 2048 * MIB, 1)
    assert (p["blocks"][0]["chunk"], p["blocks"][0]["splits"], p["fold_blocks"]) == (370400, 27, 123 * 27)
    # the 4 MiB budget of test_trial_blocks_and_fixup: 2e6 photons, 9e5 trials of H_20 in 63 blocks of 7 tiles
    p = exact_case(plan_check, 2 * 10 ** 6, 9 * 10 ** 5, 20, 0, 9 * 10 ** 5, 256, 4 * MIB, 0)
    assert (p["cb"], len(p["blocks"])) == (14336, 63)


@pytest.mark.parametrize("long_splits", [0, 1])
@pytest.mark.parametrize("nf", [256, 2048, 2049, 100000])
def test_exact_1d(plan_check, nf, long_splits):
    """Tile boundaries of a 1-D grid, whole and as a ragged trial range, every photon count and harmonic count."""
    for n in PHOTONS:
        for nharm, budget in ((1, 2048 * MIB), (20, MIB), (256, 4 * MIB)):
            exact_case(plan_check, n, nf, nharm, 0, nf, 256, budget, long_splits)
    for first, count in ((0, 1), (nf - 1, 1), (nf // 3, nf // 2), (1, nf - 1)):
        for ncu in (256, 304):
            exact_case(plan_check, 3 * 10 ** 6, nf, 20, first, count, ncu, MIB, long_splits)


@pytest.mark.parametrize("long_splits", [0, 1])
@pytest.mark.parametrize("budget", BUDGETS)
def test_exact_2d_ragged_rows(plan_check, budget, long_splits):
    """The grid of test_fold_path_many_ragged_trial_blocks_2d: 40 rows of 3000 trials (one full tile and a ragged
    one), a range that starts inside a row; at 1 MiB 13 blocks of 8192 trials that start at every offset of a row."""
    p = exact_case(plan_check, 3 * 10 ** 6, 3000, 8, 1234, 100000, 256, budget, long_splits)
    if budget == MIB:
        assert p["cb"] == 8192 and len(p["blocks"]) == 13
        # 2 or 3 block columns each: even the long-splits hook leaves 733 splits of 4096 photons, and nothing folds
        assert p["fold_blocks"] == 0 and all(k["bpg"] <= 3 for k in p["blocks"])
    exact_case(plan_check, 2 ** 28 + 5, 3000, 20, 1234, 100000, 304, budget, long_splits)


@pytest.mark.parametrize("long_splits", [0, 1])
def test_exact_2d_one_trial_rows(plan_check, long_splits):
    """Rows of one trial each hold one tile each: a block of count trials has count tiles, and the plan halves its
    blocks until a block's columns fit one launch (<= 8192 columns of 4 tiles)."""
    for count, budget in ((100000, 2048 * MIB), (32768, 2048 * MIB), (32769, 2048 * MIB), (100000, MIB), (5, MIB)):
        p = exact_case(plan_check, 10 ** 6, 1, 2, 7, count, 256, budget, long_splits)
        assert all(k["nt"] == k["bcount"] for k in p["blocks"])
    p = exact_case(plan_check, 10 ** 6, 1, 2, 7, 100000, 256, 2048 * MIB, long_splits)
    assert p["cb"] == 26624 and len(p["blocks"]) == 4      # 100000 -> 51200 -> 26624 trials per block
