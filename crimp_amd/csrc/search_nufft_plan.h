// search_nufft_plan.h -- the host decisions of the NUFFT period search (search_nufft.h), as pure functions of host
// data: n and P of every row group, the spread form, the buffer sizes against the budget, the start-table layout, every
// gather set and MFMA pass, the batches' trial ranges, the fused-finalize decision, and the work and launch counts the
// search reports (plan_nufft_search). No HIP here: search_nufft.h includes this header and launches what the plan says,
// and search_nufft_plan_check.cpp prints plans on the CPU for tests/test_nufft_plan.py.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

constexpr int kNuCW = 1024;        // photons per wave chunk (256 K-groups of 4 photons)
constexpr int kNuWaves = 4;        // chunks per 256-thread block
constexpr int kNuRows = 8;         // trial-grid rows per pass (8 rows x re/im = the 16 MFMA columns)
constexpr int kNuMaxP = 16;        // moments of the MFMA spread (its 16 A rows)
constexpr int kNuGatherMaxP = 24;  // moments of the cell-gather spread (registers)
constexpr int kNuMergeG = 16;      // wrapped cells per merge block
constexpr int kNuMaxWrap = 32;     // unwrapped cells per wrapped cell (span of the photons over n)
constexpr double kNuEps = 5e-14;   // truncation bound per photon at the grid's edge (below the rounding term kNuRho)
// Z^2_m with m >= 2: 5e-13. The certificate flags a trial when its power's bound exceeds 1e-6 of the power, and Z^2_m's
// bound over its power is sum_k (2 |A_k| E + E^2) / sum_k |A_k|^2 -- at E = N (5e-13 + kNuRho) only trials whose every
// |A_k| is below ~2e-5 N are flagged (none at config 3, P 15 -> 14). Z^2_1 and H keep kNuEps: H = max_m (Z^2_m - 4m + 4)
// cancels to near 0 on noise, where a larger E flags many more trials for the fp64 fix-up (config 4: 55 at kNuEps).
constexpr double kNuEpsZm = 5e-13;

constexpr int kNuPassMax = 10;  // harmonics per MFMA spread pass (k_nu_spread<G>, G <= 10)
struct NuPass {          // one spread pass: the slot array of each harmonic k0 + kk
    int64_t gmin[kNuPassMax];   // unwrapped cell of dt[0]
    int64_t ubase[kNuPassMax];  // offset (doubles) of the harmonic's slots in U
};

// k_nu_cellstart: up to kNuCellK harmonics k0 .. k0+nk-1 per launch; harmonic k0 + j writes its table at start + off[j]
// for cells gmin[j] .. gmin[j] + span[j] - 1
constexpr int kNuCellK = 4;
struct NuCellArgs {
    int64_t gmin[kNuCellK], span[kNuCellK], off[kNuCellK];
};

constexpr int kNuGatherRows = 2;  // rows per cell-gather batch
constexpr int kNuGatherSet = 8;   // harmonics per k_nu_gather launch
struct NuGatherSet {
    int nk;
    int k[kNuGatherSet], lanes_log2[kNuGatherSet];
    int64_t blk0[kNuGatherSet + 1];                       // first block of each harmonic, then the total
    int64_t gmin[kNuGatherSet], gmax[kNuGatherSet], gbase[kNuGatherSet], gcount[kNuGatherSet];
    int64_t soff[kNuGatherSet], woff[kNuGatherSet];       // the harmonic's start table and W planes
};

// Kernel classes of a NUFFT search (timed spans and work counts): cell starts, spread (cell gather or MFMA slots),
// merge, FFT pass 1 (columns), FFT pass 2 (rows, with the moment sum), the separate moment sum (its kernel is removed:
// the slot stays in the reporting ABI and holds 0), finalize.
enum { kNuClsCellStart, kNuClsSpread, kNuClsMerge, kNuClsPass1, kNuClsPass2, kNuClsCombine, kNuClsFinalize, kNuCls };

inline int64_t nu_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// truncation bound of P Chebyshev moments per unit photon weight at x = pi |jc| / n: 2.4 (x/2)^P / P! (nu_bes);
// invfact = 2.4 / (2^P P!), so that k_nu_finalize's x^P invfact is the bound
inline double nu_trunc(double x, int P, double* invfact) {
    double f = 1.0, xp = 1.0;
    for (int p = 1; p <= P; ++p) {
        f *= 2.0 * (double)p;
        xp *= x;
    }
    *invfact = 2.4 / f;
    return 2.4 * xp / f;
}

inline int ilog2(int64_t v) {
    int l = 0;
    while ((int64_t(1) << l) < v) ++l;
    return l;
}

// The FFT input's occupied rows a in [alo, alo + acnt) (mod n1) of the four-step view [n1][n2]: the wrapped cells
// of harmonic k's unwrapped range [gmin, gmax], widened to whole rows; a single-pass FFT (n1 = 1) or a range that
// wraps the grid takes all rows. Only those rows are spread into and read by pass 1; the others are zero.
inline void nu_occupied(int64_t gmin, int64_t gmax, int lnfft, int ln1, int* alo, int* acnt) {
    const int64_t nfft = int64_t(1) << lnfft, n1 = int64_t(1) << ln1;
    const int ln2 = lnfft - ln1;
    *alo = 0;
    *acnt = (int)n1;
    if (ln1 == 0 || gmax - gmin + 1 >= nfft) return;
    const int64_t glo = gmin & (nfft - 1), ghi = glo + (gmax - gmin);  // unwrapped end
    const int64_t a0 = glo >> ln2, a1 = ghi >> ln2;
    if (a1 - a0 + 1 >= n1) return;
    *alo = (int)a0;
    *acnt = (int)(a1 - a0 + 1);
}

// The hooks of a NUFFT search, read from the environment once at the start of every search (the tests flip them inside
// one process); the budget once per process
struct NuHooks {
    enum { kAuto, kGather, kMfma };
    int spread = kAuto;           // CRIMP_NUFFT_SPREAD=gather|mfma forces a spread form
    int lanes = 0;                // CRIMP_NUFFT_LANES=1|2|4|8: lanes per cell of every gather (0: the rule's)
    bool generic_fft = false;     // CRIMP_NUFFT_ROWS4096=0: every FFT by the generic kernels (k_nu_fft_cols,
                                  // k_nu_fft_rows_combine, k_nu_finalize), the reference of the specialised ones
    bool separate_final = false;  // CRIMP_NUFFT_FINAL=separate: k_nu_finalize after every row batch, no fused finalize
    bool plan_cache_off = false;  // CRIMP_NUFFT_PLAN_CACHE=0: every search reads its plan back (A/B hook)
    bool cell_cache_off = false;  // CRIMP_NUFFT_CELL_CACHE=0: the plan is reused, its tables are rebuilt (A/B hook)
    // CRIMP_NUFFT_FOLD=0: a cached cell-gather plan keeps its k_ap_check, k_ap_final and k_best_final launches (A/B
    // hook; a launch-time choice of nufft_search, no plan field depends on it)
    bool fold_off = false;
    // CRIMP_NUFFT_ROW_MAP=linear: block b of a row pass takes row b (0), not the XCD-contiguous map (1,
    // nu_row_of_block) -- the A/B hook and the tests' reference; the results are the same bits
    int row_map = 1;
    // budget of the NUFFT path's device buffers (CRIMP_NUFFT_BUDGET_MB, default 6144): slots, FFT ping-pong, sums
    int64_t budget = int64_t(6144) << 20;
    // start tables above this many bytes are rebuilt by every search: 1/32 of the budget, 64 MB at most
    int64_t cell_cap = int64_t(64) << 20;

    bool lanes_valid() const { return lanes == 0 || lanes == 1 || lanes == 2 || lanes == 4 || lanes == 8; }
    void set_budget(int64_t bytes) {
        budget = bytes;
        cell_cap = std::min<int64_t>(bytes / 32, int64_t(64) << 20);
    }
    static NuHooks from_env() {
        static const int64_t budget_env = [] {
            const char* e = getenv("CRIMP_NUFFT_BUDGET_MB");
            const long long mb = e ? atoll(e) : 6144;
            return (int64_t)(mb > 0 ? mb : 6144) << 20;
        }();
        auto is = [](const char* name, const char* val) {
            const char* e = getenv(name);
            return e && !strcmp(e, val);
        };
        NuHooks h;
        h.spread = is("CRIMP_NUFFT_SPREAD", "gather") ? kGather : is("CRIMP_NUFFT_SPREAD", "mfma") ? kMfma : kAuto;
        const char* lanes_s = getenv("CRIMP_NUFFT_LANES");
        h.lanes = lanes_s ? atoi(lanes_s) : 0;
        h.generic_fft = is("CRIMP_NUFFT_ROWS4096", "0");
        h.separate_final = is("CRIMP_NUFFT_FINAL", "separate");
        h.plan_cache_off = is("CRIMP_NUFFT_PLAN_CACHE", "0");
        h.cell_cache_off = is("CRIMP_NUFFT_CELL_CACHE", "0");
        h.fold_off = is("CRIMP_NUFFT_FOLD", "0");
        h.row_map = is("CRIMP_NUFFT_ROW_MAP", "linear") ? 0 : 1;
        h.set_budget(budget_env);
        return h;
    }
};

// One group of rows that share their trial segment: rows [r0, r1), trials j0 .. j0+nseg-1 of each, planned on that
// segment alone (a rank's slice of a row is its own progression, so a sharded search costs its share).
struct NuPlan {
    int64_t r0 = 0, r1 = 0, j0 = 0, nseg = 0, h = 0;  // jc = j - (j0 + h) in [-h, nseg - 1 - h]
    int lnfft = 0, P = 0;
    double invfact = 1.0, s1 = 0.0, fch = 0.0, fcl = 0.0;
    std::vector<int64_t> gmin, gmax;                     // unwrapped cells of dt[0], dt[n-1] per harmonic
};

// n and P: among the powers of two n >= nseg (up to 2^24) whose edge truncation (nu_trunc) <= kNuEps within P <= pmax
// moments, the one with the least FFT work n P; false when none exists or the photons wrap the grid more than
// kNuMaxWrap times
inline bool nu_plan(NuPlan* pl, double delta, double f0, double dt0, double dtn, int nharm, int pmax, double eps) {
    // an ascending progression only: with delta < 0 the cells of the later photons come first (s1 < 0) and every
    // table below would be sized negative (a descending grid takes the exact rule)
    if (!(delta > 0.0) || !std::isfinite(delta) || !std::isfinite(f0)) return false;
    const int64_t h = pl->nseg / 2;
    pl->h = h;
    int lnfft = 0, P = 0;
    double invfact = 1.0;
    for (int l = std::max(ilog2(pl->nseg), 6); l <= 24; ++l) {
        const double x = M_PI * (double)std::max<int64_t>(h, pl->nseg - 1 - h) / (double)(int64_t(1) << l);
        int p = 1;
        while (p <= pmax && nu_trunc(x, p, &invfact) > eps) ++p;
        if (p > pmax) continue;
        if (lnfft == 0 || ((int64_t)p << l) < ((int64_t)P << lnfft)) {
            lnfft = l;
            P = p;
        }
        if (p <= 4) break;  // larger n only adds work
    }
    if (lnfft == 0) return false;
    nu_trunc(0.0, P, &invfact);
    pl->lnfft = lnfft;
    pl->P = P;
    pl->invfact = invfact;
    const int64_t nfft = int64_t(1) << lnfft;
    pl->s1 = (double)nfft * delta;
    // fc = f_0 + (j0 + h) delta in double-double (the whole grid's progression model, whatever the segment)
    const double c = (double)(pl->j0 + h);
    const double hp = c * delta, hpe = std::fma(c, delta, -hp);
    const double fch = f0 + hp, bb = fch - f0;  // TwoSum(f0, hp)
    pl->fch = fch;
    pl->fcl = ((f0 - (fch - bb)) + (hp - bb)) + hpe;
    // the kernel's arithmetic: rint(k * (dt * s1))
    const double u0 = dt0 * pl->s1, un = dtn * pl->s1;
    // The kernels convert cells with 32-bit rint (k_nu_spread, k_nu_cellstart, k_nu_gather): every cell of every
    // harmonic, one FFT length of margin included, must fit an int -- a t0 far from the photons (t0 = 0 with MJD
    // seconds) can push |G| past 2^31 although the span is small. The plan is declined then (the exact rule runs).
    const double glim = 2147483647.0 - (double)nfft;
    pl->gmin.assign((size_t)nharm, 0);
    pl->gmax.assign((size_t)nharm, 0);
    for (int k = 1; k <= nharm; ++k) {
        const double a = (double)k * u0, b = (double)k * un;
        if (!(std::fabs(a) < glim && std::fabs(b) < glim)) return false;  // NaN declines too
        pl->gmin[(size_t)(k - 1)] = (int64_t)std::rint(a);
        pl->gmax[(size_t)(k - 1)] = (int64_t)std::rint(b);
        // descending cells (a descending grid, delta < 0, or photons out of order at the ends) would size the
        // slot and start tables negative: declined
        if (pl->gmax[(size_t)(k - 1)] < pl->gmin[(size_t)(k - 1)]) return false;
        if ((pl->gmax[(size_t)(k - 1)] - pl->gmin[(size_t)(k - 1)]) / nfft + 1 > kNuMaxWrap) return false;
    }
    return true;
}

// The spread form of a grid of nrows_grid rows: the cell gather (VALU, one lane per wrapped cell) for <= kNuGatherRows
// rows, the MFMA slots otherwise (NuHooks::spread forces one, a test hook). Decided from the whole grid, so that row
// shards compute exactly what the whole grid does.
inline bool nu_gather_form(int64_t nrows_grid, const NuHooks& hooks) {
    return hooks.spread == NuHooks::kGather ? true : hooks.spread == NuHooks::kMfma ? false : nrows_grid <= kNuGatherRows;
}

// Row groups of trials [first, first + count): the first row's segment, the full rows between, the last row's
// segment, each planned (nu_plan for nharm + 1 harmonics: an MFMA spread pass may run one past nharm). False when a
// segment is shorter than 64 trials or has no plan. hs: [delta, f0, dt[0], dt[n-1]].
inline bool nu_row_groups(std::vector<NuPlan>* plans, int64_t first, int64_t count, int64_t nf, const double* hs,
                          int nharm, int pmax, double eps) {
    const int64_t r_lo = first / nf, r_hi = (first + count - 1) / nf;
    for (int64_t r = r_lo; r <= r_hi;) {
        const int64_t a = std::max<int64_t>(first, r * nf) - r * nf, b = std::min<int64_t>(first + count, (r + 1) * nf) - r * nf;
        int64_t r1 = r + 1;
        if (a == 0 && b == nf)
            while (r1 <= r_hi && std::min<int64_t>(first + count, (r1 + 1) * nf) - r1 * nf == nf) ++r1;
        NuPlan pl;
        pl.r0 = r;
        pl.r1 = r1;
        pl.j0 = a;
        pl.nseg = b - a;
        if (pl.nseg < 64 || !nu_plan(&pl, hs[0], hs[1], hs[2], hs[3], nharm + 1, pmax, eps)) return false;
        plans->push_back(std::move(pl));
        r = r1;
    }
    return true;
}

// The MFMA spread's passes, (k0, harmonics) each, and the bytes of their largest slot array. Harmonics per pass: the
// largest size in {10, 8, 6, 4, 2} (<= Gmax) the remaining harmonics fill, allowing one past nharm (its cells are
// planned, nu_row_groups): H_20 runs as 10 + 10 (two photon passes; 8 + 8 + 4 paid the per-photon phase and cis three
// times). Gmax: the largest of 10, 8, 4, 2 whose slots fit the budget beside the fixed_bytes of W, Y and the sums.
inline int64_t nu_spread_passes(std::vector<std::pair<int, int>>* passes, const std::vector<NuPlan>& plans, int nharm,
                                int64_t nchunk, int64_t fixed_bytes, int64_t budget) {
    int64_t ubytes = 0;
    for (int Gmax = 10;; Gmax = Gmax == 10 ? 8 : Gmax / 2) {  // Gmax >= 2
        passes->clear();
        ubytes = 0;
        for (int k0 = 1; k0 <= nharm;) {
            const int rem = nharm - k0 + 1;
            int gl = 2;
            for (int cand : {10, 8, 6, 4, 2})
                if (cand <= Gmax && cand <= rem + 1) {
                    gl = cand;
                    break;
                }
            for (const NuPlan& pl : plans) {
                const int64_t SLmax = 2 * (int64_t)pl.P * std::min<int64_t>(kNuRows, pl.r1 - pl.r0);
                int64_t sl = 0;
                for (int k = k0; k < k0 + gl; ++k)
                    sl += (pl.gmax[(size_t)(k - 1)] - pl.gmin[(size_t)(k - 1)] + 1 + nchunk) * SLmax;
                ubytes = std::max<int64_t>(ubytes, sl * 8);
            }
            passes->emplace_back(k0, gl);
            k0 += gl;
        }
        if (Gmax == 2 || ubytes + fixed_bytes <= budget) break;
    }
    return ubytes;
}

// ---- the whole search's plan ----
struct NuSearchShape {
    int64_t n = 0;           // photons
    int64_t nf = 0;          // trials per row of the grid
    int64_t nrows_grid = 1;  // rows of the whole grid (the spread form is the whole grid's)
    int nharm = 1, stat = 0;
    int64_t first = 0, count = 0;  // this call's trials of the fd-outer grid
    bool want_best = false;        // crimp_search_best: the fused finalize's per-block candidates need a buffer
};

struct NuMfmaPass {  // one k_nu_spread launch and the merges + FFTs of its harmonics <= nharm
    int k0 = 0, gl = 0;
    size_t ipass = 0;  // its slot table in NuSearchPlan::passes
};

// Rows [rb, rb + nrow) of a group: kNuGatherRows (cell gather) or kNuRows (MFMA slots) at most, trials
// [tb0, tb0 + nbt) of the call's range
struct NuBatch {
    int64_t rb = 0;
    int nrow = 0;
    int64_t tb0 = 0, nbt = 0;
    int64_t best_base = 0;            // the fused finalize's first per-block best candidate
    std::vector<NuGatherSet> sets;    // cell gather: one launch each (blocks: blk0[nk]); soff within the group's tables
    std::vector<NuMfmaPass> mfma;     // MFMA slots
};

struct NuCellLaunch {  // one k_nu_cellstart launch; off within the group's tables
    int k0 = 0, nk = 0;
    NuCellArgs args{};
};

struct NuGroup {
    NuPlan pl;
    int ln1 = 0, ln2 = 0;     // FFT shape: one row pass of n2 = 2^ln2 for n <= 4096, else n1 = n / 4096 columns first
    bool fuse_final = false;  // the radix-8 row kernels (rows of 2048 and 4096) finalize in the last harmonic's launch
    int64_t jbase = 0;        // the row's trial of jc = 0
    int64_t starts_off = 0;   // the group's start tables within starts_all (cell gather)
    std::vector<int64_t> soff;        // each harmonic's table within the group's
    std::vector<NuCellLaunch> cells;  // the cell-start launches
    std::vector<NuBatch> batches;
};

struct NuSearchPlan {
    bool applicable = false;  // false: the order flag is set, a segment is short or out of range (the exact rule runs)
    bool gather = false;      // the spread form: cell gather, else MFMA slots
    std::vector<NuGroup> groups;
    std::vector<NuPass> passes;  // every MFMA (group, batch, pass)'s slot table, uploaded once
    // buffer sizes for the largest group: complex elements of one W / Y plane set, harmonics per gather launch,
    // complex sums, slot bytes, photon chunks; start-table entries of the largest group and of all groups
    int64_t Bmax = 0, csmax = 0, ubytes = 0, nchunk = 0, starts_max = 0, starts_all = 0;
    int gw = 1;
    int64_t best_alloc = 0;        // per-block best candidates to allocate (0: no best trial wanted)
    int64_t best_count = 0;        // those the fused finalizes write
    int64_t separate_batches = 0;  // batches finalized by k_nu_finalize
    int64_t cell_tables = 0;       // start tables, one per group and harmonic (crimp_last_nufft_cells)
    // crimp_last_nufft_plan(): the largest FFT length, its moments
    int64_t last_n = 0;
    int last_p = 0;
    // crimp_last_nufft_work(): [0] spread fp64 flops, then HBM bytes per class 1..6 ([1] the spread's bytes; class 0,
    // the cell starts, is not counted); launches per class (a search that reuses its start tables launches no class 0)
    double work[kNuCls] = {0, 0, 0, 0, 0, 0, 0};
    int64_t launches[kNuCls] = {0, 0, 0, 0, 0, 0, 0};
};

// One gather launch of harmonics k0 .. of batch rows nrow: block ranges, cells, lanes per cell and W plane of each
inline NuGatherSet nu_gather_set(const NuGroup& g, int k0, int nk, int64_t n, int64_t Bmax, int lanes_hook) {
    const NuPlan& pl = g.pl;
    const int64_t nfft = int64_t(1) << pl.lnfft;
    NuGatherSet S{};
    S.nk = nk;
    int64_t blocks = 0, set_cells = 0;  // the set's occupied cells (threads at one lane per cell)
    for (int jj = 0; jj < nk; ++jj) {
        int alo = 0, acnt = 0;
        nu_occupied(pl.gmin[(size_t)(k0 + jj - 1)], pl.gmax[(size_t)(k0 + jj - 1)], pl.lnfft, g.ln1, &alo, &acnt);
        set_cells += (int64_t)acnt << g.ln2;
    }
    for (int jj = 0; jj < nk; ++jj) {
        const int k = k0 + jj;
        const int64_t gmin = pl.gmin[(size_t)(k - 1)], gmax = pl.gmax[(size_t)(k - 1)];
        int alo = 0, acnt = 0;
        nu_occupied(gmin, gmax, pl.lnfft, g.ln1, &alo, &acnt);
        const int64_t gbase = (int64_t)alo << g.ln2, gcount = (int64_t)acnt << g.ln2;
        // lanes per cell: doubled (up to 4) while the launch's threads stay <= 2^20 -- counted over every harmonic of
        // the set at the doubled lanes -- and each lane keeps >= 8 photons (config 3, both harmonics in one launch:
        // 0.099 ms at 2 lanes, 0.108 at 4, 0.143 at 8, profiles/r06/ab_gather_lanes.log)
        const int64_t kspan = gmax - gmin + 1;
        const int64_t ppc = n / std::max<int64_t>(1, std::min<int64_t>(kspan, nfft));
        int L = 1;
        while (L < 4 && set_cells * 2 * L <= (int64_t(1) << 20) && ppc >= 4 * 2 * L) L *= 2;
        if (lanes_hook > 0) L = lanes_hook;
        S.k[jj] = k;
        S.lanes_log2[jj] = L == 8 ? 3 : L == 4 ? 2 : L == 2 ? 1 : 0;
        S.blk0[jj] = blocks;
        blocks += nu_cdiv(gcount * L, 256);
        S.gmin[jj] = gmin;
        S.gmax[jj] = gmax;
        S.gbase[jj] = gbase;
        S.gcount[jj] = gcount;
        S.soff[jj] = g.soff[(size_t)(k - 1)];
        S.woff[jj] = (int64_t)jj * Bmax;
    }
    S.blk0[nk] = blocks;
    return S;
}

// The work and the launches of a plan, class by class. Every term is an integer below 2^53.
inline void nu_count_work(NuSearchPlan* sp, const NuSearchShape& sh) {
    double* w = sp->work;
    int64_t* c = sp->launches;
    const double n = (double)sh.n;
    for (const NuGroup& g : sp->groups) {
        const NuPlan& pl = g.pl;
        const int P = pl.P;
        const double nfft = (double)(int64_t(1) << pl.lnfft);
        // FFT + moment sum of harmonic k: the plane's occupied rows in and all out (pass 1); the moments' planes read,
        // and the sums written or (fused finalize) the earlier harmonics' sums read and the powers written (pass 2)
        auto fft = [&](const NuBatch& b, int k) {
            const double plane = 16.0 * (double)((int64_t)P * b.nrow) * nfft;  // one complex FFT buffer of the batch
            if (g.ln1 > 0) {
                int alo = 0, acnt = 0;
                nu_occupied(pl.gmin[(size_t)(k - 1)], pl.gmax[(size_t)(k - 1)], pl.lnfft, g.ln1, &alo, &acnt);
                w[kNuClsPass1] += plane * ((double)acnt / (double)(int64_t(1) << g.ln1)) + plane;
                ++c[kNuClsPass1];
            }
            const bool fin = g.fuse_final && k == sh.nharm;
            w[kNuClsPass2] += plane + (fin ? (16.0 * (sh.nharm - 1) + 8.0) * (double)b.nbt : 16.0 * (double)b.nbt);
            ++c[kNuClsPass2];
        };
        c[kNuClsCellStart] += (int64_t)g.cells.size();
        for (const NuBatch& b : g.batches) {
            for (const NuGatherSet& S : b.sets) {
                ++c[kNuClsSpread];
                for (int jj = 0; jj < S.nk; ++jj) {
                    // per photon and row: premultiplier phase + cis ~ 40 flops, then 2 FMA + 1 multiply per moment
                    w[0] += (40.0 + 5.0 * P) * n * b.nrow;
                    w[kNuClsSpread] += 8.0 * n + 16.0 * (double)P * b.nrow * (double)S.gcount[jj];
                }
                for (int jj = 0; jj < S.nk; ++jj) fft(b, S.k[jj]);
            }
            const int64_t SL = 2 * (int64_t)P * b.nrow;
            for (const NuMfmaPass& mp : b.mfma) {
                // issued: one 16x16x4 f64 MFMA (2048 flops) per 4 photons and harmonic; slots written
                ++c[kNuClsSpread];
                w[0] += 512.0 * n * mp.gl;
                w[kNuClsSpread] += 8.0 * n;
                for (int kk = 0; kk < mp.gl; ++kk) {
                    const int k = mp.k0 + kk;
                    const double slots = 8.0 * (double)SL *
                                         (double)(pl.gmax[(size_t)(k - 1)] - pl.gmin[(size_t)(k - 1)] + 1 + sp->nchunk);
                    w[kNuClsSpread] += slots;
                    if (k > sh.nharm) continue;  // spread with its pass, never merged
                    int alo = 0, acnt = 0;
                    nu_occupied(pl.gmin[(size_t)(k - 1)], pl.gmax[(size_t)(k - 1)], pl.lnfft, g.ln1, &alo, &acnt);
                    w[kNuClsMerge] += slots + 16.0 * (double)P * b.nrow * (double)((int64_t)acnt << g.ln2);
                    ++c[kNuClsMerge];
                    fft(b, k);
                }
            }
            if (!g.fuse_final) {
                w[kNuClsFinalize] += 16.0 * (double)sh.nharm * (double)b.nbt + 8.0 * (double)b.nbt;
                ++c[kNuClsFinalize];
            }
        }
    }
}

// The plan of a search over trials [first, first + count) of the fd-outer grid (nf trials per row, arithmetic
// progression). hs: [delta, f0, dt[0], dt[n-1], unsorted flag (int bits)] as grid_is_progression read them back (the
// flag only for MFMA-slot plans: a cell-gather plan checks the order in its cell-start pass).
inline NuSearchPlan plan_nufft_search(const double* hs, const NuSearchShape& sh, const NuHooks& hooks) {
    NuSearchPlan sp;
    int bad = 0;
    memcpy(&bad, hs + 4, sizeof(int));
    if (bad) return sp;
    const int nharm = sh.nharm;
    const int64_t n = sh.n, nf = sh.nf, first = sh.first, count = sh.count;
    sp.gather = nu_gather_form(sh.nrows_grid, hooks);
    std::vector<NuPlan> plans;
    if (!nu_row_groups(&plans, first, count, nf, hs, nharm, sp.gather ? kNuGatherMaxP : kNuMaxP,
                       sh.stat == 0 && nharm >= 2 ? kNuEpsZm : kNuEps))
        return sp;
    sp.applicable = true;
    sp.nchunk = nu_cdiv(n, kNuCW);
    // buffers sized for the largest group
    int64_t nb = 0;
    for (const NuPlan& pl : plans) {
        if ((int64_t(1) << pl.lnfft) > sp.last_n) {
            sp.last_n = int64_t(1) << pl.lnfft;
            sp.last_p = pl.P;
        }
        const int64_t nrow_max = std::min<int64_t>(kNuRows, pl.r1 - pl.r0);
        const int lrow = 12 - std::min(pl.lnfft, 12);
        sp.Bmax = std::max<int64_t>(sp.Bmax, (nu_cdiv((int64_t)pl.P * nrow_max, int64_t(1) << lrow) << lrow) << pl.lnfft);
        sp.csmax = std::max<int64_t>(sp.csmax, (int64_t)nharm * nrow_max * pl.nseg);
        nb += (pl.r1 - pl.r0) * (int64_t(1) << (pl.lnfft - std::min(pl.lnfft, 12)));
    }
    if (sh.want_best) sp.best_alloc = std::max<int64_t>(nb, 1);
    // cell-gather grids gather up to kNuGatherSet harmonics per launch, each into its own W planes
    if (sp.gather) {
        sp.gw = std::min(nharm, kNuGatherSet);
        while (sp.gw > 1 && (sp.gw + 1) * sp.Bmax * 16 + sp.csmax * 16 > hooks.budget) --sp.gw;
    }
    const int64_t fixed_bytes = (sp.gw + 1) * sp.Bmax * 16 + sp.csmax * 16;
    std::vector<std::pair<int, int>> passes;  // (k0, harmonics) of each MFMA spread pass
    if (!sp.gather) sp.ubytes = nu_spread_passes(&passes, plans, nharm, sp.nchunk, fixed_bytes, hooks.budget);
    for (NuPlan& plm : plans) {
        sp.groups.emplace_back();
        NuGroup& g = sp.groups.back();
        g.pl = std::move(plm);
        const NuPlan& pl = g.pl;
        g.ln2 = std::min(pl.lnfft, 12);
        g.ln1 = pl.lnfft - g.ln2;
        g.jbase = pl.j0 + pl.h;
        g.fuse_final = g.ln2 >= 11 && !hooks.generic_fft && !hooks.separate_final;
        if (sp.gather) {
            // the start tables of harmonics 1..nharm side by side, gmax - gmin + 2 entries each
            g.starts_off = sp.starts_all;
            g.soff.assign((size_t)nharm, 0);
            int64_t off = 0;
            for (int k0 = 1; k0 <= nharm; k0 += kNuCellK) {
                NuCellLaunch cl;
                cl.k0 = k0;
                cl.nk = std::min(kNuCellK, nharm - k0 + 1);
                for (int j = 0; j < cl.nk; ++j) {
                    const int k = k0 + j;
                    cl.args.gmin[j] = pl.gmin[(size_t)(k - 1)];
                    cl.args.span[j] = pl.gmax[(size_t)(k - 1)] - pl.gmin[(size_t)(k - 1)] + 1;
                    cl.args.off[j] = off;
                    g.soff[(size_t)(k - 1)] = off;
                    off += cl.args.span[j] + 1;
                }
                g.cells.push_back(cl);
            }
            sp.starts_max = std::max<int64_t>(sp.starts_max, off);
            sp.starts_all += off;
            sp.cell_tables += nharm;
        }
        const int64_t step = sp.gather ? kNuGatherRows : kNuRows;
        for (int64_t rb = pl.r0; rb < pl.r1; rb += step) {
            NuBatch b;
            b.rb = rb;
            b.nrow = (int)std::min<int64_t>(step, pl.r1 - rb);
            b.tb0 = std::max<int64_t>(first, rb * nf) - first;
            b.nbt = std::min<int64_t>(first + count, (rb + b.nrow) * nf) - first - b.tb0;
            if (sp.gather) {
                for (int k0 = 1; k0 <= nharm; k0 += sp.gw)
                    b.sets.push_back(nu_gather_set(g, k0, std::min(sp.gw, nharm - k0 + 1), n, sp.Bmax, hooks.lanes));
            } else {
                const int64_t SL = 2 * (int64_t)pl.P * b.nrow;
                for (const auto& pass : passes) {
                    NuPass ps{};
                    int64_t off = 0;
                    for (int kk = 0; kk < pass.second; ++kk) {
                        const int k = pass.first + kk;
                        ps.gmin[kk] = pl.gmin[(size_t)(k - 1)];
                        ps.ubase[kk] = off;
                        off += (pl.gmax[(size_t)(k - 1)] - pl.gmin[(size_t)(k - 1)] + 1 + sp.nchunk) * SL;
                    }
                    NuMfmaPass mp;
                    mp.k0 = pass.first;
                    mp.gl = pass.second;
                    mp.ipass = sp.passes.size();
                    b.mfma.push_back(mp);
                    sp.passes.push_back(ps);
                }
            }
            if (g.fuse_final) {
                b.best_base = sp.best_count;
                sp.best_count += (int64_t(1) << g.ln1) * b.nrow;
            } else {
                ++sp.separate_batches;
            }
            g.batches.push_back(std::move(b));
        }
    }
    nu_count_work(&sp, sh);
    return sp;
}
