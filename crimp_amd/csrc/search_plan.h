// search_plan.h -- the host decisions of the exact i8 search, the fp64 direct search and the fp64 fix-up (the paths
// every search falls back to; the fix-up also serves the NUFFT), as pure functions of host integers: photon splits,
// trial blocks against the buffer budget, the exact kernel's tiles and fold scratch. No HIP here: crimp_hip.hip
// launches what the plans say, and search_plan_check.cpp prints plans on the CPU for tests/test_search_plan.py.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/crimp_hip.h"

constexpr int kSearchBlock = 256;  // trials per block of the fp64 direct kernel (one lane each)
constexpr int kSearchFold = 32;    // its photon splits are whole multiples of this
constexpr int kFixBlock = 256;     // threads per (trial, split) block of the fp64 fix-up kernel

// the exact kernel's tile (search_exact.h)
constexpr int kExChunk = 32;    // photons per LDS chunk (one barrier per chunk)
constexpr int kExWaves = 4;     // waves (tiles) per block: one per SIMD
constexpr int kExBlock = 64 * kExWaves;
constexpr int kExCols = 64;     // trial columns per tile: two 32-column B fragments
constexpr int kExTileTrials = 32 * kExCols;           // trials per tile (32 rows)
// int32 headroom per photon and level (balanced digits, |top digit| <= 64): level 3 <= 2 x 49152, level 4
// <= 2 x 32768, level 5 <= 2 x 16384, level 6 <= 2 x 4096. Every kExCarry chunks (16384 photons: level 3
// reaches 1.61e9 < 2^31) the level sums are carried upward exactly (acc_L = 256 q + r, r in [0, 255]:
// acc_L <- r, acc_{L+1} += q), which leaves level 6 (never reduced) growing per period by at most 2^27 of its own
// products plus the carry from level 5 (<= (2 x 16384 x 16384 + 2^22 + 255) / 256 < 2.14e6), 1.363e8 in all; every
// kExFold chunks (CRIMP_EX_FOLD_PERIODS = 15 periods, 245760 photons: |level 6| <= 2.045e9 < 2^31 - 1) they are folded
// into the int64 running sums. (8 periods until round 4: a split of the photons then held at most 131072 photons
// without an int64 fold through global scratch, so config 3 needed 77 splits and 2.46 GB of 64-bit atomics per
// search; 15 periods halve both.)
#ifndef CRIMP_EX_FOLD_PERIODS
#define CRIMP_EX_FOLD_PERIODS 15
#endif
static_assert(CRIMP_EX_FOLD_PERIODS >= 1 && CRIMP_EX_FOLD_PERIODS <= 15, "level 6 must stay inside int32 between folds");
constexpr int kExCarry = 16384 / kExChunk;
constexpr int kExFold = CRIMP_EX_FOLD_PERIODS * kExCarry;
constexpr int kExFoldVals = 64;             // int64 running sums per lane (2 fragments x 16 result rows x Re, Im)
// int64 totals in units of 2^-36 hold |C_k| <= n exactly for n < 2^27 photons; a larger search runs its photons in
// chunks of < 2^27, each into its own totals, summed exactly by the finalize (periodsearch.py:57-71 has no limit).
constexpr int64_t kExactMaxPhotons = int64_t(1) << 27;
constexpr int64_t kExFoldMaxBlocks = 8192;  // fold scratch of one launch <= 1 GiB
constexpr int64_t kExFoldPhotons = (int64_t)kExFold * kExChunk;  // photons between int64 folds
constexpr int64_t kExNoFoldMaxBlocks = 131072;  // blocks per launch when splits need no fold scratch

inline int64_t sp_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The hooks of these paths, read from the environment at the start of every search (the tests flip them inside one
// process).
struct SearchHooks {
    // Per-trial device buffers of a search (fp64 per-split partial sums of the fp64 kernels, int64 totals of the exact
    // kernel) are bounded by this many bytes (CRIMP_SEARCH_BUDGET_MB, default 2048): a larger trial range is computed
    // in blocks of trials.
    int64_t budget = int64_t(2048) << 20;
    // Relative error the exact path and the NUFFT certify per trial before the fp64 fix-up (CRIMP_FIXUP_REL, default
    // 1e-6; a larger value is a test hook that sends more trials through the fix-up).
    double fixup_rel = 1e-6;
    bool long_splits = false;  // CRIMP_EXACT_LONG_SPLITS (set at all): the exact kernel's fold path, a test hook

    static SearchHooks from_env() {
        SearchHooks h;
        const char* e = getenv("CRIMP_SEARCH_BUDGET_MB");
        const long long mb = e ? atoll(e) : 2048;
        h.budget = (int64_t)(mb > 0 ? mb : 2048) << 20;
        e = getenv("CRIMP_FIXUP_REL");
        h.fixup_rel = e ? atof(e) : 1e-6;
        if (!(h.fixup_rel > 0.0)) h.fixup_rel = 1e-6;
        h.long_splits = getenv("CRIMP_EXACT_LONG_SPLITS") != nullptr;
        return h;
    }
};

// the fp64 kernels sum rem remaining harmonics in groups of 8, 4, 2, 1, each started from its exact phase
inline int harm_group(int rem) { return rem >= 8 ? 8 : rem >= 4 ? 4 : rem >= 2 ? 2 : 1; }

// Direct (one lane per trial) fp64 search of count trials: up to 64 photon splits of >= 16384 photons, a function of
// the photon count only; trial blocks of cb trials (whole kSearchBlocks, even-sized) whose partial sums fit the budget.
struct DirectPlan {
    int64_t chunk, splits, cb;
};
inline DirectPlan plan_direct(int64_t n, int nharm, int64_t count, int64_t budget) {
    const int64_t splits0 = std::max<int64_t>(1, std::min<int64_t>(64, n / 16384));
    const int64_t chunk = sp_cdiv(sp_cdiv(n, splits0), kSearchFold) * kSearchFold;
    const int64_t splits = sp_cdiv(n, chunk);
    const int64_t cbmax = std::max<int64_t>(kSearchBlock, budget / (8 * splits * 2 * nharm));
    const int64_t even = sp_cdiv(sp_cdiv(count, sp_cdiv(count, cbmax)), kSearchBlock) * kSearchBlock;
    return {chunk, splits, std::min<int64_t>(count, even)};
}

// fp64 fix-up, a few trials over all photons: photon splits of >= 4096 photons (up to 1024), one block per (trial,
// split), trial blocks of cbmax trials (a launch's grid.x, and partial sums within the budget).
struct FixupPlan {
    int64_t chunk, splits, cbmax;
};
inline FixupPlan plan_fixup(int64_t n, int nharm, int64_t budget) {
    const int64_t splits0 = std::max<int64_t>(1, std::min<int64_t>(1024, n / 4096));
    const int64_t chunk = sp_cdiv(n, splits0);
    const int64_t splits = sp_cdiv(n, chunk);
    return {chunk, splits, std::max<int64_t>(1, std::min<int64_t>(65535, budget / (8 * splits * 2 * nharm)))};
}

struct ExSplit {
    int64_t chunk = 0, splits = 0;
};
// Of the split counts want in [lo, hi] whose chunk is at most max_chunk, the one whose last round of bpg x splits
// blocks on ncu CUs is fullest (the fewest splits unless more gain 0.5 %); splits 0 when there is none.
inline ExSplit ex_fill(int64_t n, int64_t bpg, int64_t ncu, int64_t lo, int64_t hi, int64_t max_chunk) {
    ExSplit best;
    double best_eff = -1.0;
    for (int64_t want = lo; want <= hi; ++want) {
        const int64_t chunk = sp_cdiv(sp_cdiv(n, want), kExChunk) * kExChunk;
        const int64_t splits = sp_cdiv(n, chunk);
        const int64_t blocks = bpg * splits;
        const double eff = (double)blocks / (double)(sp_cdiv(blocks, ncu) * ncu);
        if (chunk <= max_chunk && eff > best_eff + 0.005) {
            best_eff = eff;
            best = {chunk, splits};
        }
    }
    return best;
}

// Photon splits of the exact kernel (one 256-thread block per CU) for bpg block columns: >= 4096 photons per split
// and >= 8 rounds of the device's ncu CUs, and among those counts the one whose last round of blocks is fullest
// (ex_fill): a grid of 8.2 rounds runs as long as 9. Config 3 (1e7 photons, 123 block columns, 256 CUs): the 41 splits
// of one fold period each would make 5043 blocks = 19.70 rounds; 52 splits of 192320 photons = 6396 blocks fill 24.98.
// With the long-splits hook: 27 splits of 370400 photons, 3321 blocks = 12.97 rounds (search_plan_check prints both).
inline ExSplit split_exact(int64_t n, int64_t bpg, int64_t ncu, bool long_splits) {
    const int64_t smax_n = std::max<int64_t>(1, std::min<int64_t>(sp_cdiv(n, 4096), 65535));
    const int64_t srounds = sp_cdiv(8 * ncu, bpg);
    // Preferred: splits of <= kExFoldPhotons photons, which never fold into the int64 scratch (a block's only
    // global traffic is then its final atomics, 128 KB; each intermediate fold would add 128 KB each way): the
    // counts from the smallest such up to a quarter more.
    const int64_t snofold = sp_cdiv(n, kExFoldPhotons);
    if (!long_splits && snofold <= 65535 && bpg * snofold <= kExNoFoldMaxBlocks) {
        const int64_t lo = std::max<int64_t>(1, std::max<int64_t>(snofold, std::min<int64_t>(srounds, smax_n)));
        const ExSplit s = ex_fill(n, bpg, ncu, lo, std::min<int64_t>(smax_n, lo + lo / 4 + 1), kExFoldPhotons);
        if (s.splits > 0) return s;
    }
    // else folding splits, as many blocks as the fold scratch holds at most: the counts up to 4x the smallest
    const int64_t smax = std::max<int64_t>(1, std::min<int64_t>(smax_n, kExFoldMaxBlocks / bpg));
    const int64_t smin = std::max<int64_t>(1, std::min<int64_t>(srounds, smax));
    return ex_fill(n, bpg, ncu, smin, std::min<int64_t>(smax, 4 * smin), INT64_MAX);
}

// The exact search of trials [first, first + count) of a grid of nf trials per row: one launch per trial block,
// photon chunk and harmonic.
struct ExBlock {
    int64_t bfirst, bcount;  // the block's trials [bfirst, bfirst + bcount) of the grid
    int64_t tf, nt, bpg;     // its first tile, its tiles, its block columns (kExWaves tiles each)
    int64_t chunk, splits;   // split_exact
};
struct ExactPlan {
    int err = CRIMP_OK;  // else msg says why there is no plan
    const char* msg = nullptr;
    int64_t nchunk = 0, pc = 0;  // photon chunks of pc < 2^27 (one for every search below that), each with its own totals
    int64_t tpr = 0, cb = 0;     // tiles per grid row, trials per block
    std::vector<ExBlock> blocks;
    int64_t fold_blocks = 0;  // the largest bpg * splits of the blocks whose splits fold into the int64 scratch
    int64_t tot_elems = 0, flagged_elems = 0, fold_elems = 0;  // int64 totals, flagged trial indices, fold scratch
};
inline ExactPlan exact_refused(int err, const char* msg) {
    ExactPlan p;
    p.err = err;
    p.msg = msg;
    return p;
}
inline ExactPlan plan_exact(int64_t n, int64_t nf, int nharm, int64_t first, int64_t count, int64_t ncu,
                            const SearchHooks& hooks) {
    ExactPlan p;
    const int64_t tpr = p.tpr = sp_cdiv(nf, kExTileTrials);
    const int ncomp = 2 * nharm;
    p.nchunk = sp_cdiv(n, kExactMaxPhotons - 1);
    p.pc = sp_cdiv(n, p.nchunk);
    // Trial blocks are bounded by the int64 totals buffer (the budget) and by the tiles one launch may hold
    // (<= kExFoldMaxBlocks block columns, so that a fold scratch stays <= 1 GiB: a 2-D grid's rows each start a
    // new tile, so a block of short rows holds more tiles than its trial count suggests); whole tiles.
    int64_t want = std::max<int64_t>(kExTileTrials, hooks.budget / (8 * ncomp * p.nchunk));
    for (;;) {
        p.cb = std::min<int64_t>(count, sp_cdiv(sp_cdiv(count, sp_cdiv(count, want)), kExTileTrials) * kExTileTrials);
        p.blocks.clear();
        p.fold_blocks = 0;
        bool fits = true;
        for (int64_t b0 = 0; b0 < count && fits; b0 += p.cb) {
            ExBlock k;
            k.bfirst = first + b0;
            k.bcount = std::min<int64_t>(p.cb, count - b0);
            const int64_t last = k.bfirst + k.bcount - 1;
            k.tf = (k.bfirst / nf) * tpr + (k.bfirst % nf) / kExTileTrials;
            const int64_t tl = (last / nf) * tpr + (last % nf) / kExTileTrials;
            k.nt = tl - k.tf + 1;
            k.bpg = sp_cdiv(k.nt, kExWaves);
            fits = k.bpg <= kExFoldMaxBlocks;
            const ExSplit sp = split_exact(p.pc, k.bpg, ncu, hooks.long_splits);
            k.chunk = sp.chunk;
            k.splits = sp.splits;
            if (k.chunk > kExFoldPhotons) p.fold_blocks = std::max<int64_t>(p.fold_blocks, k.bpg * k.splits);
            p.blocks.push_back(k);
        }
        if (fits) break;
        if (p.cb <= kExTileTrials) return exact_refused(CRIMP_ERR_ARG, "exact search: trial block does not fit one launch");
        want = p.cb / 2;
    }
    if (p.fold_blocks > kExFoldMaxBlocks) return exact_refused(CRIMP_ERR_HIP, "exact search: fold scratch bound");
    p.tot_elems = ncomp * p.cb * p.nchunk;
    p.flagged_elems = count;
    // fold scratch only when some block's splits are longer than one fold period; shorter splits never touch it
    p.fold_elems = p.fold_blocks * kExWaves * kExFoldVals * 64;
    return p;
}
