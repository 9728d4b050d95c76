// search_nufft_finish_check.cpp -- runs the host finish of a folded NUFFT search (search_nufft_finish.h) on the CPU
// (make nufft-finish-check builds it with ASan and UBSan; tests/test_nufft_finish_host.py checks what it prints).
//
// Commands on stdin, whitespace-separated, any number of them; doubles as C99 hex floats (or nan, inf):
//   partials nb  dev_0 fm_0 ... dev_nb-1 fm_nb-1                 -> "partials dev fm"
//   plan nf dev fm  f0 flast dt0 dtn  delta' f0' dt0' dtn'       -> "plan 0|1"    (the primed: the cached plan's)
//   best n  v_0 i_0 ... v_n-1 i_n-1                              -> "best v i"
// One answer line per command on stdout, doubles as C99 hex floats (exact).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "search_nufft_finish.h"

static bool rd(double* v) { return scanf("%lf", v) == 1; }
static bool ri(long long* v) { return scanf("%lld", v) == 1; }

int main() {
    char cmd[16];
    while (scanf("%15s", cmd) == 1) {
        if (!strcmp(cmd, "partials")) {
            long long nb = 0;
            if (!ri(&nb) || nb < 0 || nb > (1 << 20)) return 2;
            std::vector<double> part((size_t)(2 * nb));
            for (double& v : part)
                if (!rd(&v)) return 2;
            double dev = -1.0, fm = -1.0;
            nu_finish_partials(part.data(), (int)nb, &dev, &fm);
            printf("partials %a %a\n", dev, fm);
        } else if (!strcmp(cmd, "plan")) {
            long long nf = 0;
            double dev = 0.0, fm = 0.0, pub[4], ex[4];
            if (!ri(&nf) || nf < 2 || !rd(&dev) || !rd(&fm)) return 2;
            for (double& v : pub)
                if (!rd(&v)) return 2;
            for (double& v : ex)
                if (!rd(&v)) return 2;
            printf("plan %d\n", nu_finish_plan_ok(pub, nf, dev, fm, ex) ? 1 : 0);
        } else if (!strcmp(cmd, "best")) {
            long long n = 0;
            if (!ri(&n) || n < 0 || n > (1 << 20)) return 2;
            std::vector<NuFinCand> c((size_t)n);
            for (NuFinCand& e : c) {
                long long i = 0;
                if (!rd(&e.v) || !ri(&i)) return 2;
                e.i = i;
            }
            const NuFinCand b = nu_finish_best(c.data(), n);
            printf("best %a %" PRId64 "\n", b.v, b.i);
        } else {
            return 2;
        }
    }
    return 0;
}
