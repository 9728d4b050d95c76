// toa_grid_plan_check.cpp -- prints plan_brute_grid's plan of one case on the CPU (make plan-check builds it with
// ASan and UBSan; tests/test_toa_grid_plan.py checks what it prints against the definitions restated in numpy).
//
// Case on stdin, whitespace-separated:
//   model K   amp[K] loc[K] ch[K] kap[K]         (TplDev's fields, as make_tpl folds them)
//   lo hi pb                                     (FitCfg's norm bounds and phShift bound)
//   nint   then per interval: photons exposure
//   nbins  then nbins + 1 edges                  (nbins 0: no histogram)
//   mf_available full_grid grid_slow no_cert     (0 / 1 each)
// Plan on stdout, one "key values..." line each; doubles as C99 hex floats (exact), masks as hex integers.
#include <cinttypes>
#include <cstdio>

#include "toa_grid_plan.h"

static bool rd(double* v) { return scanf("%lf", v) == 1; }
static bool ri(long long* v) { return scanf("%lld", v) == 1; }

static void line(const char* key, const double* v, size_t n) {
    printf("%s", key);
    for (size_t i = 0; i < n; ++i) printf(" %a", v[i]);
    printf("\n");
}

int main() {
    TplDev T;
    std::memset(&T, 0, sizeof(T));
    long long model = 0, K = 0, nint = 0, nbins = 0, flag[4] = {0, 0, 0, 0};
    if (!ri(&model) || !ri(&K) || model < 0 || model > 2 || K < 1 || K > CRIMP_MAX_COMP) return 2;
    T.model = (int32_t)model;
    T.K = (int32_t)K;
    double* field[4] = {T.amp, T.loc, T.ch, T.kap};
    for (double* f : field)
        for (int j = 0; j < T.K; ++j)
            if (!rd(&f[j])) return 2;
    double lo = 0.0, hi = 0.0, pb = 0.0;
    if (!rd(&lo) || !rd(&hi) || !rd(&pb) || !ri(&nint) || nint < 1 || nint > 65535) return 2;
    std::vector<int64_t> off((size_t)nint + 1, 0);
    std::vector<double> expo((size_t)nint);
    for (long long i = 0; i < nint; ++i) {
        long long n = 0;
        if (!ri(&n) || n < 1 || !rd(&expo[(size_t)i])) return 2;
        off[(size_t)i + 1] = off[(size_t)i] + n;
    }
    if (!ri(&nbins) || nbins < 0 || nbins > 256) return 2;
    std::vector<double> edges(nbins ? (size_t)nbins + 1 : 0);
    for (double& e : edges)
        if (!rd(&e)) return 2;
    for (long long& f : flag)
        if (!ri(&f)) return 2;
    ToaHooks hooks;
    hooks.full_grid = flag[1] != 0;
    hooks.grid_slow = flag[2] != 0;
    hooks.no_cert = flag[3] != 0;
    const GridPlan P = plan_brute_grid(T, lo, hi, pb, off.data(), expo.data(), nint, nbins ? edges.data() : nullptr,
                                       (int)nbins, flag[0] != 0, hooks);
    line("phi", P.phi.data(), P.phi.size());
    line("grid_n", P.grid_n.data(), P.grid_n.size());
    printf("nc %" PRId64 "\nnlazy %" PRId64 "\nmode %d\n", P.nc, P.nlazy, P.mode);
    line("hb", &P.hb, 1);
    line("gsc", &P.gsc, 1);
    for (long long i = 0; i < nint; ++i) line("nrm", P.nrm.data() + i * P.nc, (size_t)P.nc);
    const size_t nphi = P.phi.size();
    for (size_t r = 0; r * nphi < P.mask.size(); ++r) {
        printf("mask");
        for (size_t k = 0; k < nphi; ++k) printf(" %" PRIx64, P.mask[r * nphi + k]);
        printf("\n");
    }
    printf("row");
    for (const int r : P.row) printf(" %d", r);
    printf("\n");
    return 0;
}
