// search_nufft_plan_check.cpp -- prints plan_nufft_search's plan of one case on the CPU (make nufft-plan-check builds
// it with ASan and UBSan; tests/test_nufft_plan.py checks what it prints against the definitions restated in numpy,
// tests/test_gpu_nufft_plan.py against what the library reports of the searches it ran).
//
// Case on stdin, whitespace-separated (no environment is read):
//   delta f0 dt0 dtn unsorted                     (the five read-back scalars; doubles as C99 hex floats, the flag 0 / 1)
//   n nf nrows_grid nharm stat first count best   (NuSearchShape)
//   spread lanes generic_fft separate_final budget_bytes   (NuHooks; spread 0 auto, 1 gather, 2 mfma)
// Plan on stdout, one "key values..." line each, in the plan's order (a group's lines, then its cell-start launches,
// then its batches, each followed by its gather sets or MFMA passes); doubles as C99 hex floats (exact).
#include <cinttypes>
#include <cstdio>

#include "search_nufft_plan.h"

static bool rd(double* v) { return scanf("%lf", v) == 1; }
static bool ri(long long* v) { return scanf("%lld", v) == 1; }

static void ints(const char* key, const int64_t* v, size_t n) {
    printf("%s", key);
    for (size_t i = 0; i < n; ++i) printf(" %" PRId64, v[i]);
    printf("\n");
}

int main() {
    double hs[5] = {0, 0, 0, 0, 0};
    long long sh[8], hk[5];
    for (int i = 0; i < 4; ++i)
        if (!rd(&hs[i])) return 2;
    long long unsorted = 0;
    if (!ri(&unsorted)) return 2;
    const int bad = unsorted != 0;
    std::memcpy(hs + 4, &bad, sizeof(int));
    for (long long& v : sh)
        if (!ri(&v)) return 2;
    for (long long& v : hk)
        if (!ri(&v)) return 2;
    NuSearchShape S;
    S.n = sh[0];
    S.nf = sh[1];
    S.nrows_grid = sh[2];
    S.nharm = (int)sh[3];
    S.stat = (int)sh[4];
    S.first = sh[5];
    S.count = sh[6];
    S.want_best = sh[7] != 0;
    if (S.n < 1 || S.nf < 1 || S.nrows_grid < 1 || S.nharm < 1 || S.nharm > 256 || S.first < 0 || S.count < 1 ||
        S.first + S.count > S.nrows_grid * S.nf || hk[0] < 0 || hk[0] > 2 || hk[4] < 1)
        return 2;
    NuHooks H;
    H.spread = (int)hk[0];
    H.lanes = (int)hk[1];
    H.generic_fft = hk[2] != 0;
    H.separate_final = hk[3] != 0;
    H.set_budget(hk[4]);
    if (!H.lanes_valid()) return 2;
    const NuSearchPlan P = plan_nufft_search(hs, S, H);
    printf("applicable %d\n", P.applicable ? 1 : 0);
    if (!P.applicable) return 0;
    printf("gather %d\nlast_n %" PRId64 "\nlast_p %d\n", P.gather ? 1 : 0, P.last_n, P.last_p);
    printf("Bmax %" PRId64 "\ngw %d\ncsmax %" PRId64 "\nubytes %" PRId64 "\nnchunk %" PRId64 "\n", P.Bmax, P.gw, P.csmax,
           P.ubytes, P.nchunk);
    printf("starts_max %" PRId64 "\nstarts_all %" PRId64 "\nbest_alloc %" PRId64 "\nbest_count %" PRId64 "\n",
           P.starts_max, P.starts_all, P.best_alloc, P.best_count);
    printf("separate_batches %" PRId64 "\ncell_tables %" PRId64 "\ncell_cap %" PRId64 "\n", P.separate_batches,
           P.cell_tables, H.cell_cap);
    printf("work");
    for (const double w : P.work) printf(" %a", w);
    printf("\n");
    ints("launches", P.launches, kNuCls);
    printf("row_map %d\n", H.row_map);  // NuHooks' default (no case field, no plan field depends on it)
    for (const NuGroup& g : P.groups) {
        const NuPlan& pl = g.pl;
        printf("group %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d %d %d %d %" PRId64 " %" PRId64
               " %a %a %a %a\n",
               pl.r0, pl.r1, pl.j0, pl.nseg, pl.h, pl.lnfft, pl.P, g.ln1, g.ln2, g.fuse_final ? 1 : 0, g.jbase,
               g.starts_off, pl.invfact, pl.s1, pl.fch, pl.fcl);
        ints("gmin", pl.gmin.data(), pl.gmin.size());
        ints("gmax", pl.gmax.data(), pl.gmax.size());
        ints("soff", g.soff.data(), g.soff.size());
        for (const NuCellLaunch& c : g.cells) {
            printf("cell %d %d", c.k0, c.nk);
            for (int j = 0; j < c.nk; ++j)
                printf(" %" PRId64 " %" PRId64 " %" PRId64, c.args.gmin[j], c.args.span[j], c.args.off[j]);
            printf("\n");
        }
        for (const NuBatch& b : g.batches) {
            printf("batch %" PRId64 " %d %" PRId64 " %" PRId64 " %" PRId64 "\n", b.rb, b.nrow, b.tb0, b.nbt, b.best_base);
            for (const NuGatherSet& s : b.sets) {
                printf("set %d %" PRId64, s.nk, s.blk0[s.nk]);
                for (int j = 0; j < s.nk; ++j)
                    printf(" %d %d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64, s.k[j],
                           s.lanes_log2[j], s.blk0[j], s.gmin[j], s.gmax[j], s.gbase[j], s.gcount[j], s.soff[j],
                           s.woff[j]);
                printf("\n");
            }
            for (const NuMfmaPass& m : b.mfma) {
                const NuPass& ps = P.passes[m.ipass];
                printf("mfma %d %d %zu", m.k0, m.gl, m.ipass);
                for (int j = 0; j < m.gl; ++j) printf(" %" PRId64 " %" PRId64, ps.gmin[j], ps.ubase[j]);
                printf("\n");
            }
        }
    }
    printf("npass %zu\n", P.passes.size());
    return 0;
}
