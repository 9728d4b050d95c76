// orbit_search_plan_check.cpp -- prints the plan of orbit_search_plan.h for one case on the CPU (make
// orbit-search-plan-check builds it with ASan and UBSan; tests/test_orbit_search_host.py checks what it prints against
// the rules restated in Python).
//
// Case on stdin, whitespace-separated (no environment is read):
//   plan n nf nharm stat norb cap_bytes
//   orbit kind raw[0] .. raw[10]          (kind 1 BT, 2 ELL1; raw indexed by CRIMP_ORBIT_*)
// Plan on stdout, one "key values..." line each, then one "group k0 G" line per harmonic group; an orbit prints
// "ok" or "fault <text>".
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "orbit_search_plan.h"

static void kv(const char* key, int64_t v) { printf("%s %" PRId64 "\n", key, v); }

int main() {
    char kind[16];
    if (scanf("%15s", kind) != 1) return 2;
    if (!strcmp(kind, "plan")) {
        long long v[6];
        for (long long& x : v)
            if (scanf("%lld", &x) != 1) return 2;
        if (v[0] < 1 || v[1] < 1 || v[2] < 1 || v[2] > kOsMaxHarm || v[3] < 0 || v[3] > 1 || v[4] < 1 || v[5] < 1) return 2;
        const OrbitSearchPlan P = plan_orbit_search(v[0], v[1], (int)v[2], (int)v[3], v[4], v[5]);
        kv("slice", P.slice);
        kv("nslices", P.nslices);
        kv("J", P.J);
        kv("batch", P.batch);
        kv("nbatches", P.nbatches);
        kv("part_elems", P.part_elems);
        kv("grid_x", P.grid_x);
        kv("grid_y", P.grid_y);
        for (int g = 0; g < P.ngroups; ++g) printf("group %d %d\n", P.k0[g], P.G[g]);
    } else if (!strcmp(kind, "orbit")) {
        int k = 0;
        double raw[kOsMaxKeys];
        if (scanf("%d", &k) != 1) return 2;
        for (double& x : raw)
            if (scanf("%lf", &x) != 1) return 2;
        const char* why = os_orbit_fault(k, raw);
        if (why)
            printf("fault %s\n", why);
        else
            printf("ok\n");
    } else {
        return 2;
    }
    return 0;
}
