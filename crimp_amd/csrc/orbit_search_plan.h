// orbit_search_plan.h -- the host decisions of the orbit search (orbit_search.h) as pure functions of
// host numbers: the photon slices, the trial chunk and the harmonic groups of k_orbit_search, the orbit batch that
// keeps the partial sums under the scratch cap, the grid; and the limits of one orbit. No HIP here: crimp_hip.hip
// launches what the plan says, and orbit_search_plan_check.cpp prints plans on the CPU for
// tests/test_orbit_search_host.py.
//
// Determinism. power[o][j] is summed over the photons in an order fixed by the slice structure alone: slice s holds
// photons [s kOsSlice, (s + 1) kOsSlice), lane l of its workgroup photons l, l + kOsBlock, ... of the slice, the lanes
// are combined 16 at a time, then the 16 rows, then the slices in index order. The slice structure is a function of n;
// the trial chunk J and the harmonic groups (functions of m) decide which sums share a pass over the slice, never the
// order inside one sum; the batch (a function of nf, m, norb and the cap) only decides which orbits share a launch.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "../../include/crimp_hip.h"

constexpr int kOsBlock = 256;       // threads of a k_orbit_search workgroup
constexpr int kOsSlice = 3072;      // photons per slice: 12 per lane; dt (and dt^2) of a slice are 24 (48) KB of LDS
constexpr int kOsAcc = 16;          // (C, S) accumulator pairs a lane holds: J trials x G harmonics <= kOsAcc
constexpr int kOsMaxKeys = 11;      // CRIMP_ORBIT_PB .. CRIMP_ORBIT_A1DOT
constexpr int kOsMaxHarm = 256;
constexpr int kOsMaxGroups = kOsMaxHarm / 8 + 3;
constexpr int64_t kOsMaxBatch = 65535;                  // orbits of one launch (grid.y)
constexpr int64_t kOsDefaultCap = int64_t(1) << 30;     // bytes of partial sums per launch

// the remaining harmonics are summed in groups of 8, 4, 2, 1, each started from its exact phase (harm_group of
// search_plan.h; constexpr, so the kernel calls it too)
constexpr int os_harm_group(int rem) { return rem >= 8 ? 8 : rem >= 4 ? 4 : rem >= 2 ? 2 : 1; }

// The scratch cap of a call in bytes: CRIMP_ORBIT_SCRATCH_KB (default 1 GiB), read at every call (the tests flip it
// inside one process).
inline int64_t os_cap_from_env() {
    const char* e = getenv("CRIMP_ORBIT_SCRATCH_KB");
    const long long kb = e ? atoll(e) : 0;
    return kb > 0 ? (int64_t)std::min<long long>(kb, (long long)1 << 40) << 10 : kOsDefaultCap;
}

struct OrbitSearchPlan {
    int64_t slice = 0, nslices = 0;  // photons per slice and slices: from n only
    int J = 0;                       // trials per chunk: from m only
    int ngroups = 0;                 // harmonic groups: from m only
    int k0[kOsMaxGroups] = {}, G[kOsMaxGroups] = {};
    int64_t batch = 0, nbatches = 0;  // orbits per launch, launches
    int64_t part_elems = 0;           // doubles of the partial buffer [nslices][batch][2m][nf]
    int64_t grid_x = 0, grid_y = 0;   // slices x orbits of a full batch
};

// n >= 1, nf >= 1, 1 <= m <= kOsMaxHarm, norb >= 1, cap >= 1 (the caller checks). stat does not enter: both
// statistics are formed from the same sums.
inline OrbitSearchPlan plan_orbit_search(int64_t n, int64_t nf, int m, int stat, int64_t norb, int64_t cap_bytes) {
    (void)stat;
    OrbitSearchPlan p;
    p.slice = kOsSlice;
    p.nslices = (n + kOsSlice - 1) / kOsSlice;
    p.J = kOsAcc / os_harm_group(m);
    for (int k = 1; k <= m; k += p.G[p.ngroups - 1]) {
        p.k0[p.ngroups] = k;
        p.G[p.ngroups] = os_harm_group(m - k + 1);
        ++p.ngroups;
    }
    // doubles one orbit's partial sums take; beyond 2^56 no batch fits anyway and the products below stay in int64
    const double per_d = (double)p.nslices * (double)(2 * m) * (double)nf;
    const int64_t cap_elems = std::max<int64_t>(1, cap_bytes / 8);
    int64_t fit = 1;
    if (per_d < 7e16) {
        const int64_t per = p.nslices * (2 * m) * nf;
        fit = std::max<int64_t>(1, cap_elems / per);
    }
    p.batch = std::min<int64_t>(std::min<int64_t>(fit, kOsMaxBatch), norb);
    p.nbatches = (norb + p.batch - 1) / p.batch;
    p.part_elems = per_d < 7e16 ? p.nslices * (2 * m) * nf * p.batch : -1;
    p.grid_x = p.nslices;
    p.grid_y = p.batch;
    return p;
}

// The limits of crimp_binary_delay for the orbit whose raw fields (the .par's units, indexed by CRIMP_ORBIT_*) are
// raw: null when the orbit is admissible, else the text of the failed check (check_binary's texts; of_derive refuses
// the same orbits with the same expressions).
inline const char* os_orbit_fault(int kind, const double* raw) {
    const bool bt = kind == CRIMP_BINARY_BT;
    for (int k = 0; k < kOsMaxKeys; ++k)
        if (!std::isfinite(raw[k])) return "a binary parameter is not finite";
    if (!(raw[CRIMP_ORBIT_PB] > 0.0)) return "PB must be positive";
    if (!(raw[CRIMP_ORBIT_A1] >= 0.0)) return "A1 must be >= 0";
    double e = raw[CRIMP_ORBIT_ECC];
    if (bt) {
        if (!(e >= 0.0 && e < 1.0)) return "ECC must be in [0, 1)";
    } else {
        e = std::hypot(raw[CRIMP_ORBIT_EPS1], raw[CRIMP_ORBIT_EPS2]);
        if (!(e < 1.0)) return "EPS1^2 + EPS2^2 must be below 1";
    }
    if (!(2.0 * 3.141592653589793 * raw[CRIMP_ORBIT_A1] / (raw[CRIMP_ORBIT_PB] * 86400.0 * (1.0 - e)) < 0.5))
        return "2 pi A1 / (PB (1 - e)) must be below 1/2";
    return nullptr;
}
