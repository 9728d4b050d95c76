// toa_grid_plan.h -- the host decisions of crimp_toa_fit's brute grid, as pure functions of host data: the lmfit
// lattice, the pruned norm candidates of every interval, the fast-kernel mode certificate, the lazy norms and the
// histogram certificate's masks (plan_brute_grid). No HIP here: crimp_hip.hip includes this header and launches what
// the plan says, and toa_grid_plan_check.cpp prints plans on the CPU for tests/test_toa_grid_plan.py.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/crimp_hip.h"

struct TplDev {
    int32_t model, K;
    double amp[CRIMP_MAX_COMP];   // amp_j * ampShift (fourier), amp_j*ampShift/(2 pi) * sinh(w) (cauchy),
                                  // amp_j*ampShift/(2 pi I0(1/w^2)) (vonmises)
    double loc[CRIMP_MAX_COMP];   // ph_j or cen_j
    double ch[CRIMP_MAX_COMP];    // cosh(wid_j) (cauchy)
    double kap[CRIMP_MAX_COMP];   // 1/wid_j^2 (vonmises)
};

constexpr int kGridKMax = 8;     // template components of the brute-grid kernels
constexpr int kGridNNSmall = 4;  // the pruned brute grid's norms per lane (crimp_toa_fit)
// mode (crimp_toa_fit's brute grid, Fourier templates on k_toa_grid_mf only): bit 0 (kGridNoMin) -- no per-phShift
// min h (the host's template bound certifies every candidate norm + h > 0); bit 1 (kGridProd8) -- log2 of products of
// eight model values (the host certified that every factor of a valid lattice point stays inside [2^-15, 2^15] after
// the coefficient scale, or k_toa_grid_best checks it where the min decides validity); bit 2 (kGridCert) -- no
// per-phShift min either: the lazy norms' points are shown invalid by the phase histogram (k_toa_grid_best with lzmask;
// crimp_toa_fit_redchi2's histogram, tpl_bin_max)
constexpr int kGridNoMin = 1, kGridProd8 = 2, kGridCert = 4;

// Bounds hmin <= h <= hmax of the template part h = model - norm over every phase and phShift
// (templatemodels.py:64-82, :166-185, :271-290 with TplDev's folded amplitudes)
inline void tpl_bounds(const TplDev& T, double* hmin, double* hmax) {
    double lo = 0.0, hi = 0.0;
    for (int j = 0; j < T.K; ++j) {
        const double a = std::fabs(T.amp[j]);
        if (T.model == CRIMP_MODEL_FOURIER) {
            lo -= a;
            hi += a;
        } else if (T.model == CRIMP_MODEL_CAUCHY) {  // a / (cosh w - cos u), cos u in [-1, 1]
            lo += T.amp[j] / (T.ch[j] + 1.0);
            hi += T.amp[j] / (T.ch[j] - 1.0);
        } else {                                     // a exp(k cos u)
            lo += T.amp[j] * std::exp(-T.kap[j]);
            hi += T.amp[j] * std::exp(T.kap[j]);
        }
    }
    *hmin = std::min(lo, hi);
    *hmax = std::max(lo, hi);
}

// A lower bound of the template part h over every phase and phShift, from the template's own shape: min over u of
// h(u) (h(x; phShift) is h shifted in phase for every model, so its minimum does not depend on phShift) sampled on
// 2^16 points per turn, less the largest change between neighbouring samples (a smooth h cannot dip further between
// two samples than it moves across one step). Tighter than tpl_bounds' -sum|amp_j| for Fourier templates.
inline double tpl_hmin_scan_uncached(const TplDev& T) {
    const int M = 1 << 16;
    double mn = INFINITY, dmax = 0.0, prev = 0.0;
    for (int i = 0; i <= M; ++i) {
        const double u = 2.0 * M_PI * (double)(i % M) / (double)M;
        double h = 0.0;
        for (int j = 0; j < T.K; ++j) {
            if (T.model == CRIMP_MODEL_FOURIER)
                h += T.amp[j] * std::cos((double)(j + 1) * u + T.loc[j]);
            else if (T.model == CRIMP_MODEL_CAUCHY)
                h += T.amp[j] / (T.ch[j] - std::cos(u - T.loc[j]));
            else
                h += T.amp[j] * std::exp(T.kap[j] * std::cos(u - T.loc[j]));
        }
        if (i > 0) dmax = std::max(dmax, std::fabs(h - prev));
        mn = std::min(mn, h);
        prev = h;
    }
    return mn - dmax - 1e-12 * (std::fabs(mn) + dmax);
}
inline double tpl_hmin_scan(const TplDev& T) {  // cached for the last template (a fit batch reuses one template)
    static TplDev last;
    static double val = 0.0;
    static bool have = false;
    if (have && std::memcmp(&last, &T, sizeof(T)) == 0) return val;
    val = tpl_hmin_scan_uncached(T);
    std::memcpy(&last, &T, sizeof(T));
    have = true;
    return val;
}

// Lazy-norm certificate (crimp_toa_fit_redchi2): per phShift phi_k of the brute lattice and histogram bin b = [e_b,
// e_{b+1}], an upper bound of the Fourier template part over every photon bin b can hold at phi_k,
// max_{x in bin} h0(x - phi_k / 2 pi) with h0(u) = sum_j amp_j cos(2 pi (j+1) u + loc_j) (k_toa_grid_mf's h): the
// largest of 8192 samples per cycle over the covering sample range plus the Lipschitz bound L / 8192,
// L = sum_j 2 pi (j+1) |amp_j|. out[k * nb + b]. Cached for the last (template, lattice, edges).
inline const std::vector<double>& tpl_bin_max(const TplDev& T, const std::vector<double>& phi, const double* edges,
                                              int nb) {
    static TplDev last;
    static std::vector<double> lphi, ledg, val;
    static bool have = false;
    std::vector<double> edg(edges, edges + nb + 1);
    if (have && std::memcmp(&last, &T, sizeof(T)) == 0 && lphi == phi && ledg == edg) return val;
    constexpr int G = 8192;
    std::vector<double> hs(G);
    double L = 0.0;
    for (int j = 0; j < T.K; ++j) L += 2.0 * M_PI * (double)(j + 1) * std::fabs(T.amp[j]);
    for (int g = 0; g < G; ++g) {
        double h = 0.0;
        for (int j = 0; j < T.K; ++j) h += T.amp[j] * std::cos(2.0 * M_PI * (double)(j + 1) * ((double)g / G) + T.loc[j]);
        hs[(size_t)g] = h;
    }
    val.assign(phi.size() * (size_t)nb, 0.0);
    for (size_t k = 0; k < phi.size(); ++k) {
        const double sh = phi[k] / (2.0 * M_PI);
        for (int b = 0; b < nb; ++b) {
            const int64_t g0 = (int64_t)std::floor((edg[(size_t)b] - sh) * G) - 1;
            const int64_t g1 = (int64_t)std::ceil((edg[(size_t)b + 1] - sh) * G) + 1;
            double mx = -INFINITY;
            for (int64_t g = g0; g <= g1; ++g) mx = std::max(mx, hs[(size_t)(((g % G) + G) % G)]);
            val[k * (size_t)nb + (size_t)b] = mx + L / G;
        }
    }
    std::memcpy(&last, &T, sizeof(T));
    lphi = phi;
    ledg = edg;
    have = true;
    return val;
}

// k_toa_grid_mf's power-of-two coefficient scale: 0 when the largest |amp_j| is in [1, 4096], otherwise the exponent
// that brings it there; *ok = false where even that is out of reach (the exponent is clamped to [-64, 20], so that
// s x 500 stays far from fp32 overflow in the kernel's products of four factors): those go to the VALU kernel.
inline int grid_mf_scale(const TplDev& T, bool* ok) {
    double m = 0.0;
    for (int j = 0; j < T.K; ++j) m = std::max(m, std::fabs(T.amp[j]));
    *ok = std::isfinite(m) && m > 0.0;
    if (!*ok) return 0;
    int e = 0;
    while (std::ldexp(m, e) < 1.0 && e < 20) ++e;
    while (std::ldexp(m, e) > 4096.0 && e > -64) --e;
    const double ms = std::ldexp(m, e);
    *ok = ms >= 1.0 && ms <= 4096.0;
    return e;
}

// The test hooks of crimp_toa_fit(_redchi2), read from the environment once at the start of every call (the tests
// flip them inside one process)
struct ToaHooks {
    bool full_grid = false;      // CRIMP_TOA_FULL_GRID: evaluate all 20 norms
    bool lattice_start = false;  // CRIMP_TOA_LATTICE_START: start the ascent at the brute lattice point itself (not at
                                 // the rate norm + parabola vertex)
    bool grid_slow = false;      // CRIMP_TOA_GRID_SLOW: always the full four-factor kernel with the min h
    bool no_cert = false;        // CRIMP_TOA_NO_CERT: no lazy-norm certificate
    bool has_mom_r = false;      // CRIMP_FIT_MOM_R: FitCfg's mom_r (0 = iterative norm profiles)
    double mom_r = 0.0;
    static ToaHooks from_env() {
        ToaHooks h;
        h.full_grid = getenv("CRIMP_TOA_FULL_GRID") != nullptr;
        h.lattice_start = getenv("CRIMP_TOA_LATTICE_START") != nullptr;
        h.grid_slow = getenv("CRIMP_TOA_GRID_SLOW") != nullptr;
        h.no_cert = getenv("CRIMP_TOA_NO_CERT") != nullptr;
        if (const char* e = getenv("CRIMP_FIT_MOM_R")) {
            h.has_mom_r = true;
            h.mom_r = atof(e);
        }
        return h;
    }
};

// What the brute grid's launches need (plan_brute_grid)
struct GridPlan {
    std::vector<double> phi;     // lmfit's phShift lattice
    std::vector<double> grid_n;  // lmfit's 20 lattice norms
    std::vector<double> nrm;     // [nint][nc] the intervals' candidate norms, compacted
    int64_t nc = 0;              // candidate norms per interval: 2, kGridNNSmall or 20
    int64_t nlazy = 0;           // leading candidates of every interval left out of the grid
    double hb = 0.0;             // lower bound of the template part (tpl_hmin_scan)
    double gsc = 1.0;            // k_toa_grid_mf's coefficient scale (grid_mf_scale)
    int mode = 0;                // kGrid* bits
    std::vector<uint64_t> mask;  // kGridCert: [distinct lazy norm][nphi] bins that show the point invalid
    std::vector<int> row;        // kGridCert: [nint][nlazy] row of mask for the interval's lazy norm
};

// lmfit brute lattices (measureToAs.py:292-295): scipy mgrid phShift = k*0.05 - bound, 20 norms
inline void plan_lattice(GridPlan& P, double lo, double hi, double pb) {
    const int64_t nphi = (int64_t)std::ceil((2.0 * pb) / (0.05 * 1.0));
    const int64_t nn = 20;
    P.phi.resize((size_t)nphi);
    for (int64_t k = 0; k < nphi; ++k) P.phi[(size_t)k] = (double)k * 0.05 + (-pb);
    P.grid_n.resize((size_t)nn);
    for (int64_t a = 0; a < nn; ++a) P.grid_n[(size_t)a] = (double)a * ((hi - lo) / (double)(nn - 1)) + lo;
}

// Pruned norm axis. At fixed phShift the extended LL is -nE + sum_i ln(n + h_i) + const (every model:
// templatemodels.py:109-121, :213-226, :318-329), strictly concave in n, with its maximum n* where
// sum_i 1/(n* + h_i) = E, so n* lies in [N/E - hmax, N/E - hmin] for any bounds hmin <= h_i <= hmax. The
// lattice maximum over the norms at that phShift is then at one of the grid norms adjacent to that
// interval: every other grid norm is strictly lower (a whole grid step, ~26 norm units, from a
// bracketing one), so the brute grid's argmax (lmfit brute, measureToAs.py:292-295) is found among them.
// Config 5 and the worked example: 2 of the 20 norms.
// [hlo, hhi]: tpl_bounds. Sets P.nc and P.nrm.
inline void plan_candidates(GridPlan& P, double hlo, double hhi, const int64_t* hoff, const double* hexp, int64_t nint,
                            bool full_grid) {
    const std::vector<double>& grid_n = P.grid_n;
    const int64_t nn = (int64_t)grid_n.size();
    std::vector<int64_t> alo((size_t)nint), acnt((size_t)nint);
    int64_t ncand = 1;
    for (int64_t i = 0; i < nint; ++i) {
        const double r = (double)(hoff[i + 1] - hoff[i]) / hexp[(size_t)i];
        const double lo_n = r - hhi, hi_n = r - hlo, eps = 1e-9 * (1.0 + std::fabs(r) + hhi - hlo);
        int64_t a0 = 0, a1 = nn - 1;
        if (std::isfinite(lo_n) && std::isfinite(hi_n) && hexp[(size_t)i] > 0.0) {
            while (a0 + 1 < nn && grid_n[(size_t)(a0 + 1)] <= lo_n - eps) ++a0;
            while (a1 > a0 && grid_n[(size_t)(a1 - 1)] >= hi_n + eps) --a1;
        }
        alo[(size_t)i] = a0;
        acnt[(size_t)i] = a1 - a0 + 1;
        ncand = std::max(ncand, a1 - a0 + 1);
    }
    if (ncand > kGridNNSmall || full_grid) {
        for (int64_t i = 0; i < nint; ++i) {
            alo[(size_t)i] = 0;
            acnt[(size_t)i] = nn;
        }
        ncand = nn;
    }
    // compacted per-interval norms: the candidates in grid order, padded by repeating the last (a repeat
    // comes later in norm-outer order, so it never wins a tie)
    const int64_t nc = ncand <= 2 ? 2 : ncand <= kGridNNSmall ? kGridNNSmall : ncand;
    P.nc = nc;
    P.nrm.resize((size_t)(nint * nc));
    for (int64_t i = 0; i < nint; ++i)
        for (int64_t c = 0; c < nc; ++c)
            P.nrm[(size_t)(i * nc + c)] = grid_n[(size_t)(alo[(size_t)i] + std::min(c, acnt[(size_t)i] - 1))];
}

// k_toa_grid_best's start rule decided by hb as the min h would decide it: hb + N/E > N/E / 2 for every interval
inline bool plan_start_rule(double hb, const int64_t* hoff, const double* hexp, int64_t nint) {
    bool ok = true;
    for (int64_t i = 0; i < nint && ok; ++i) {
        const double r = (double)(hoff[i + 1] - hoff[i]) / hexp[(size_t)i];
        ok = hb + r > 0.5 * r;
    }
    return ok;
}

// Fast brute grid (k_toa_grid_mf, Fourier): without the per-phShift min h when a lower bound hb of h keeps
// every candidate lattice point valid (norm + h > 0) and decides k_toa_grid_best's start rule as the min
// would (plan_start_rule); with log2 of products of eight model values when every
// factor s (norm + h) of a valid point stays in [2^-15, 2^15], so that a product of eight is a normal fp32:
// certified here from hb and the template's upper bound for the norms above -hb, and checked by
// k_toa_grid_best (from the min) for the others -- a lattice point there that could have underflowed sends
// the grid back to the four-factor kernel.
inline int plan_mode(const GridPlan& P, double hhi, const int64_t* hoff, const double* hexp, int64_t nint) {
    const double hb = P.hb, gsc = P.gsc;
    bool nomin = true, prod8 = true;
    for (const double nv : P.nrm) {
        nomin = nomin && nv + hb > 0.0;
        prod8 = prod8 && (nv + hhi) * gsc <= std::ldexp(1.0, 15) &&
                (nv + hb <= 0.0 || (nv + hb) * gsc >= std::ldexp(1.0, -15));
    }
    nomin = nomin && plan_start_rule(hb, hoff, hexp, nint);
    return (nomin ? kGridNoMin : 0) | (prod8 ? kGridProd8 : 0);
}

// Lazy norms: the leading candidate norms of every interval with norm + hb <= 0 are left out of the grid.
// Their lattice points are valid only where the per-phShift min h exceeds -norm; k_toa_grid_best marks the
// rest -inf, as the full grid does, and a valid one sends the grid back to the full evaluation. (Config 5:
// lmfit's lowest grid norm, norm0/100, is a candidate of every interval and invalid everywhere.)
// Returns lazy_uniform: every interval has exactly P.nlazy leading lazy norms. The certificate needs it: an
// interval with more would have evaluated norms with norm + hb <= 0 that k_toa_grid_best, without the min,
// could not judge.
inline bool plan_lazy(GridPlan& P, int64_t nint) {
    const int64_t nc = P.nc;
    int64_t nlazy = nc, zmax = 0;
    for (int64_t i = 0; i < nint; ++i) {
        int64_t z = 0;
        while (z < nc && P.nrm[(size_t)(i * nc + z)] + P.hb <= 0.0) ++z;
        nlazy = std::min(nlazy, z);
        zmax = std::max(zmax, z);
    }
    const bool lazy_uniform = zmax == nlazy;
    if (nlazy >= nc) nlazy = 0;  // every candidate lazy: evaluate them all
    P.nlazy = nlazy;
    return lazy_uniform;
}

// Lazy-norm certificate (crimp_toa_fit_redchi2, whose histogram is at hand): a lazy
// point (norm n0, phi_k) is invalid when some photon has h <= -n0; it does where a bin b holds photons and
// the template's bound over that bin at phi_k (tpl_bin_max) is <= -n0 - margin (1e-3 + 1e-5 of the
// amplitude sum and n0: it covers the kernel's fp32 h). With the start rule decided by hb too (as kGridNoMin), the
// grid then needs no min h: k_toa_grid_best marks those points -inf from the counts, and one it cannot show invalid
// reruns the grid with the min (its unsafe flag). Used only when every (lazy norm, phi_k) has such a bin: sets P.mask,
// P.row and kGridCert then.
inline void plan_certificate(GridPlan& P, const TplDev& T, int64_t nint, const double* edges, int nb) {
    const int64_t nphi = (int64_t)P.phi.size(), nc = P.nc, nlazy = P.nlazy;
    const std::vector<double>& bm = tpl_bin_max(T, P.phi, edges, nb);
    std::vector<double> vals;  // the distinct lazy norms (lattice values)
    std::vector<int> hrow((size_t)(nint * nlazy));
    for (int64_t i = 0; i < nint; ++i)
        for (int64_t z = 0; z < nlazy; ++z) {
            const double v = P.nrm[(size_t)(i * nc + z)];
            size_t r = 0;
            while (r < vals.size() && vals[r] != v) ++r;
            if (r == vals.size()) vals.push_back(v);
            hrow[(size_t)(i * nlazy + z)] = (int)r;
        }
    std::vector<uint64_t> hmask(vals.size() * (size_t)nphi, 0);
    // margin over the kernel's h: its f16 hi/lo terms and fp32 sums err by <~ 1e-6 of the amplitude
    // sum and of the norm inside the accumulators (k_toa_grid_mf), so 1e-5 of them plus 1e-3
    double asum = 0.0;
    for (int j = 0; j < T.K; ++j) asum += std::fabs(T.amp[j]);
    bool all_k = true;
    for (size_t r = 0; r < vals.size(); ++r)
        for (int64_t k = 0; k < nphi; ++k) {
            const double margin = 1e-3 + 1e-5 * (asum + std::fabs(vals[r]));
            uint64_t m = 0;
            for (int b = 0; b < nb; ++b)
                if (bm[(size_t)k * nb + b] + margin <= -vals[r]) m |= 1ull << b;
            hmask[r * (size_t)nphi + (size_t)k] = m;
            all_k = all_k && m != 0;
        }
    if (!all_k) return;
    P.mask.swap(hmask);
    P.row.swap(hrow);
    P.mode |= kGridCert;
}

// The brute grid of one crimp_toa_fit call: T and FitCfg's norm bounds [lo, hi] and phShift bound pb, the host's
// offsets[nint + 1] and exposures[nint], crimp_toa_fit_redchi2's histogram edges[nbins + 1] (nullptr: none).
// mf_available: the build has k_toa_grid_mf (CRIMP_GRID_MFMA); the fast modes exist on it only (toa_grid_partials' own
// test), so they are decided once here and a Cauchy / von Mises / K > kGridKMax fit sets up no mode state, certificate
// or unsafe readback.
inline GridPlan plan_brute_grid(const TplDev& T, double lo, double hi, double pb, const int64_t* hoff,
                                const double* hexp, int64_t nint, const double* edges, int nbins, bool mf_available,
                                const ToaHooks& hooks) {
    GridPlan P;
    plan_lattice(P, lo, hi, pb);
    double hlo = 0.0, hhi = 0.0;
    tpl_bounds(T, &hlo, &hhi);
    plan_candidates(P, hlo, hhi, hoff, hexp, nint, hooks.full_grid);
    P.hb = tpl_hmin_scan(T);
    bool mf_ok = false;
    P.gsc = std::ldexp(1.0, grid_mf_scale(T, &mf_ok));
    const bool mf_grid = T.model == CRIMP_MODEL_FOURIER && mf_available && T.K <= kGridKMax && mf_ok;
    if (mf_grid && !hooks.grid_slow && std::isfinite(P.hb)) P.mode = plan_mode(P, hhi, hoff, hexp, nint);
    bool lazy_uniform = false;
    if ((P.mode & kGridProd8) && !(P.mode & kGridNoMin)) lazy_uniform = plan_lazy(P, nint);
    if (edges && P.nlazy > 0 && lazy_uniform && P.mode == kGridProd8 && nbins <= 64 && !hooks.no_cert &&
        plan_start_rule(P.hb, hoff, hexp, nint))
        plan_certificate(P, T, nint, edges, nbins);
    return P;
}
