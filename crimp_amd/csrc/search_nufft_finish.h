// Host finish of a folded NUFFT search (search_nufft.h, NuRun::fold): a repeated cell-gather search on a cached plan
// launches no progression check and no best-trial reduction of its own. The check's blocks ride in the first gather
// launch, the fused finalize leaves its per-block candidates where they are, and one read-back brings all of it to the
// host, which finishes here: the reduce of the check's partials, the cached plan's test (k_ap_final's, clause for
// clause) and the reduce of the candidates (best_better's rule, k_best_final's result).
// No HIP in this file: search_nufft_finish_check.cpp builds it for the CPU under ASan + UBSan
// (tests/test_nufft_finish_host.py).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

// The block one read-back fetches, in device memory (byte offsets):
//   0   int flags[4]      [fix-up count, legacy flag (order / stale plan), gather-failure epoch, -]
//   16  double best[2]    [power, index] where a kernel reduced the candidates (k_best_final, launch_best)
//   32  double pub[4]     f[0], f[nf-1], t[0] - t0, t[n-1] - t0, as the device forms them
//   64  double part[kNuFinChecks][2]   the check blocks' (max deviation, max |f|)
//   ..  NuFinCand cand[kNuFinCands]    the fused finalize's per-block best trials
constexpr int kNuFinChecks = 64;   // check blocks at most (64 with a loop ran 14.7 us as a launch of their own: hidden)
constexpr int kNuFinCands = 928;   // candidates finished on the host; above it k_best_final runs (block <= 16 KB)
constexpr size_t kNuFinPubOff = 32, kNuFinPartOff = 64;
constexpr size_t kNuFinCandOff = kNuFinPartOff + (size_t)kNuFinChecks * 16;
constexpr size_t kNuFinBytes = kNuFinCandOff + (size_t)kNuFinCands * 16;
static_assert(kNuFinBytes <= 16384, "the read-back block stays under 16 KB");

struct NuFinCand {  // BestCand's layout
    double v;
    int64_t i;
};

// max deviation and max |f| over the check blocks' pairs part[2 b], part[2 b + 1] (fmax: a NaN never wins, as on the
// device)
inline void nu_finish_partials(const double* part, int nb, double* dev, double* fm) {
    double d = 0.0, m = 0.0;
    for (int b = 0; b < nb; ++b) {
        d = std::fmax(d, part[2 * b]);
        m = std::fmax(m, part[2 * b + 1]);
    }
    *dev = d;
    *fm = m;
}

// k_ap_final's test of a cached plan: the step from the grid's ends finite and non-zero, the grid a progression to
// 16 ulp of max |f|, and step, f_0, dt[0], dt[n-1] equal to the values the plan was made from (expect[0..3]).
// pub: f[0], f[nf-1], dt[0], dt[n-1] as published by the device.
inline bool nu_finish_plan_ok(const double* pub, int64_t nf, double dev, double fm, const double* expect) {
    const double f0 = pub[0];
    const double d = (pub[1] - f0) / (double)(nf - 1);
    const bool ok = std::isfinite(d) && d != 0.0 && dev <= 16.0 * 2.220446049250313e-16 * fm;
    return ok && d == expect[0] && f0 == expect[1] && pub[2] == expect[2] && pub[3] == expect[3];
}

// best_better (crimp_hip.hip): the larger value, ties to the lower index, a NaN above every number
inline bool nu_finish_better(double v1, int64_t i1, double v2, int64_t i2) {
    const bool n1 = std::isnan(v1), n2 = std::isnan(v2);
    if (n1 != n2) return n1;
    if (!n1 && v1 != v2) return v1 > v2;
    return i1 < i2;
}
// k_best_final's result for the candidates: np.argmax semantics (the first NaN wins); none: (-inf, INT64_MAX)
inline NuFinCand nu_finish_best(const NuFinCand* c, int64_t n) {
    NuFinCand b = {-std::numeric_limits<double>::infinity(), INT64_MAX};
    for (int64_t k = 0; k < n; ++k)
        if (nu_finish_better(c[k].v, c[k].i, b.v, b.i)) b = c[k];
    return b;
}
