// search_plan_check.cpp -- prints a plan of search_plan.h for one case on the CPU (make search-plan-check builds it
// with ASan and UBSan; tests/test_search_plan.py checks what it prints against the rules restated in Python).
//
// Case on stdin, whitespace-separated (no environment is read):
//   kind n nf nharm first count ncu budget_bytes long_splits
// kind is direct (plan_direct), fixup (plan_fixup), exact (plan_exact) or split (split_exact of n photons, with the
// block columns bpg in the nf field); every kind reads all the fields and ignores those its plan does not take.
// Plan on stdout, one "key values..." line each; an exact plan ends with one "block" line per trial block:
//   block bfirst bcount tf nt bpg chunk splits
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "search_plan.h"

static void kv(const char* key, int64_t v) { printf("%s %" PRId64 "\n", key, v); }

int main() {
    char kind[16];
    long long v[8];
    if (scanf("%15s", kind) != 1) return 2;
    for (long long& x : v)
        if (scanf("%lld", &x) != 1) return 2;
    const int64_t n = v[0], nf = v[1], first = v[3], count = v[4], ncu = v[5];
    const int nharm = (int)v[2];
    SearchHooks H;
    H.budget = v[6];
    H.long_splits = v[7] != 0;
    if (n < 1 || nf < 1 || v[2] < 1 || v[2] > 256 || first < 0 || count < 1 || ncu < 1 || H.budget < 1) return 2;
    if (!strcmp(kind, "direct")) {
        const DirectPlan P = plan_direct(n, nharm, count, H.budget);
        kv("chunk", P.chunk);
        kv("splits", P.splits);
        kv("cb", P.cb);
    } else if (!strcmp(kind, "fixup")) {
        const FixupPlan P = plan_fixup(n, nharm, H.budget);
        kv("chunk", P.chunk);
        kv("splits", P.splits);
        kv("cbmax", P.cbmax);
    } else if (!strcmp(kind, "split")) {
        const ExSplit P = split_exact(n, nf, ncu, H.long_splits);
        kv("chunk", P.chunk);
        kv("splits", P.splits);
    } else if (!strcmp(kind, "exact")) {
        const ExactPlan P = plan_exact(n, nf, nharm, first, count, ncu, H);
        if (P.err) {
            printf("error %d %s\n", P.err, P.msg);
            return 0;
        }
        kv("nchunk", P.nchunk);
        kv("pc", P.pc);
        kv("tpr", P.tpr);
        kv("cb", P.cb);
        kv("fold_blocks", P.fold_blocks);
        kv("tot_elems", P.tot_elems);
        kv("flagged_elems", P.flagged_elems);
        kv("fold_elems", P.fold_elems);
        for (const ExBlock& k : P.blocks)
            printf("block %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n",
                   k.bfirst, k.bcount, k.tf, k.nt, k.bpg, k.chunk, k.splits);
    } else {
        return 2;
    }
    return 0;
}
