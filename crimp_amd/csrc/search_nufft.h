// search_nufft.h -- Z^2_m / H periodicity search by a non-uniform FFT over an arithmetic-progression trial grid
// (CRIMP_FLAG_NUFFT, PeriodSearch(..., precision="nufft")). Included by crimp_hip.hip after the exact path's host
// code (it uses Scratch, grid_is_progression's delta and fixup_search).
//
// The reference (periodsearch.py:67, :93-99, :120-121) evaluates, for every trial f_j and harmonic k,
//   A_k(f_j) = sum_i exp(2 pi i k (f_j dt_i + c2 dt_i^2))        (C_k = Re A_k, S_k = Im A_k)
// photon by photon: O(N M) per harmonic. On an arithmetic progression f_j = fc + jc delta (jc = j - h, h = nf/2,
// fc = f_0 + h delta) the sum over trials is a type-1 non-uniform DFT:
//   A_k(j) = sum_i c_i exp(2 pi i jc u_i / n),   c_i = exp(2 pi i k (fc dt_i + c2 dt_i^2)),   u_i = n k delta dt_i,
// with n a power of two >= nf. Writing u_i = g_i + e_i (g_i = rint(u_i), |e_i| <= 1/2), the sub-cell factor
// exp(2 pi i jc e_i / n) = exp(2 i z e_i), z = pi jc / n (|z| <= pi/2), is expanded in Chebyshev polynomials of
// 2 e_i (Jacobi-Anger; nu_bes): exp(2 i z e) = sum_p eps_p i^p J_p(z) T_p(2e), so with P "moments"
//   A_k(j) = sum_{p<P} eps_p i^p J_p(z) * B_p(jc mod n),   B_p(J) = sum_g b_p[g] exp(2 pi i J g / n),
//   b_p[g] = sum_{i : g_i = g (mod n)} c_i T_p(2 e_i).
// |T_p| <= 1 and |J_p(z)| <= (|z|/2)^p / p!, so |A_k error| <= 2 N sum_{p>=P} (|z|/2)^p / p! < 2.4 N (x/2)^P / P!
// with x = pi |jc| / n; P and n are chosen so that the bound is <= kNuEps at the grid's edge (16 moments at config 3;
// a Taylor expansion in e_i, bound N x^P / P!, needs 20).
// The cost is O(N m P) for the moments plus O(m P n log n) for the FFTs, against O(N M m) for the direct sum.
//
// Kernels (one pass = harmonics k0 .. k0+G-1 of up to 8 trial-grid rows):
//   k_nu_spread   photons -> per-(chunk, cell) moment sums. Each wave owns a chunk of kNuCW time-ordered photons;
//                 4 photons x 16 moments form the A operand and 4 photons x 8 rows x (re, im) of c_i the B operand
//                 of v_mfma_f64_16x16x4_f64, whose accumulator sums the photons of the current cell in fp64 (no
//                 reduction, no atomics). A cell change (photons are sorted, so cells only grow) flushes the 16 x 16
//                 tile to the cell's slot: slot(chunk c, cell G) = G - G_min + c is unique per (c, G).
//   k_nu_merge    slots -> W[batch][g]: every wrapped cell g sums its unwrapped cells G = g (mod n) and, per G, the
//                 chunks that hold it, in chunk order (deterministic), transposed to batch-major rows.
//   k_nu_cellstart, k_nu_gather   the spread of grids of <= kNuGatherRows rows: one lane per wrapped cell sums its
//                 photons' moments in registers, straight into W (no slots, no merge).
//   k_nu_fft_cols (k_nu_cols256, k_nu_cols512 for n1 = 256, 512)   pass 1 of the four-step FFT (n = n1 n2, n2 = 4096;
//                 Stockham autosort stages in LDS, positive exponent); n <= 4096 has no pass 1.
//   k_nu_fft_rows_combine (k_nu_rows_iw for n2 = 4096, k_nu_rows_combine8<11> for n = 2048)   pass 2, the rows, with
//                 the moments' Bessel-weighted sum at every trial -> (C_k, S_k) kept in registers across the moments.
//   k_nu_finalize Z^2 / H in the reference's formula order and the certificate (fix-up list, as the exact path); the
//                 last harmonic's k_nu_rows_iw / k_nu_rows_combine8 launch does it in its epilogue instead.
//
// Host: every decision that needs no device pointer -- n and P per row group, the spread form, the buffer sizes, the
// start-table layout, the gather sets and MFMA passes, the work and launch counts -- is plan_nufft_search
// (search_nufft_plan.h, no HIP, checked on the CPU by tests/test_nufft_plan.py). nufft_search walks that plan: NuRun
// holds the stream, the scratch buffers and the timed-span recorder and queues the cell starts, one gather set, one
// MFMA pass + merge, one FFT + moment sum and one finalize; the flags' single read-back, the out-of-order / mismatch
// handling and the fix-up follow. NuPlanCache keeps the plans (and start tables) of repeated searches.
#pragma once

#include "search_nufft_plan.h"  // the constants and kernel-argument structs the host plan fills (NuPass, NuCellArgs,
                                 // NuGatherSet), the plan itself (plan_nufft_search)
#include "search_nufft_finish.h"  // the read-back block of a folded search and its finish on the host

typedef double nu_f64x4 __attribute__((ext_vector_type(4)));

constexpr int kNuTile = 4096;      // complex elements per FFT block (64 KB of LDS), 16 per thread
// Rounding bound per photon for the certificate, in units of |A_k|'s scale N: c_i (cis table + fp64 polynomial,
// angle-addition over <= 8 harmonics: ~20 ulp), the MFMA's fp64 accumulation over <= 256 K-groups per cell run
// (<= 256 ulp of the run's sum of |terms|, each <= 1), the merge, the FFT (~3 log2 n ulp) and Horner (e^x ulp):
// < 4e-14 N; kept at 1e-13 N.
constexpr double kNuRho = 1e-13;

struct NuTw {            // w_n^t = hi[t >> lbits] * lo[t & (2^lbits - 1)], t in [0, n)
    const double2* lo;
    const double2* hi;
    int lbits;
    int64_t mask;        // n - 1
};

__device__ __forceinline__ double2 nu_cmul(double2 a, double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 nu_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 nu_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 nu_muli(double2 a) { return make_double2(-a.y, a.x); }  // i * a

__device__ __forceinline__ double2 nu_tw(const NuTw& T, int64_t t) {
    t &= T.mask;
    return nu_cmul(T.hi[t >> T.lbits], T.lo[t & ((int64_t(1) << T.lbits) - 1)]);
}

// e^{2 pi i x}, |x| <= 0.5 (+ a few ulp): 1024-entry table of the coarse angle and the fp64 series of the residual
// angle |theta| <= pi/1024 (omitted terms < 1e-24).
__device__ __forceinline__ double2 nu_cis(const double2* __restrict__ tab, double x) {
    const double t = rint(x * 1024.0);
    const double r = fma(t, -1.0 / 1024.0, x);  // exact
    const double th = r * 6.283185307179586476925286766559;
    const double t2 = th * th;
    const double c = fma(t2, fma(t2, fma(t2, fma(t2, 1.0 / 40320.0, -1.0 / 720.0), 1.0 / 24.0), -0.5), 1.0);
    const double s = th * fma(t2, fma(t2, fma(t2, fma(t2, 1.0 / 362880.0, -1.0 / 5040.0), 1.0 / 120.0), -1.0 / 6.0), 1.0);
    const double2 T = tab[((int)t) & 1023];
    return make_double2(T.x * c - T.y * s, T.x * s + T.y * c);
}

// e^{2 pi i x}, |x| <= 0.5 (+ a few ulp), from a 2048-entry table (the cell gather keeps it in LDS) and the residual
// series to degree 4 / 5 (|theta| <= pi/2048: omitted terms < 2e-20)
__device__ __forceinline__ double2 nu_cis2(const double2* __restrict__ tab, double x) {
    const double t = rint(x * 2048.0);
    const double r = fma(t, -1.0 / 2048.0, x);  // exact
    const double th = r * 6.283185307179586476925286766559;
    const double t2 = th * th;
    const double c = fma(t2, fma(t2, 1.0 / 24.0, -0.5), 1.0);
    const double s = th * fma(t2, fma(t2, 1.0 / 120.0, -1.0 / 6.0), 1.0);
    const double2 T = tab[((int)t) & 2047];
    return make_double2(T.x * c - T.y * s, T.x * s + T.y * c);
}

// frac(a * d) for a = ahi + alo (double-double), as hi part reduced exactly plus the product's rounding error.
// Contraction off: fused into fma(ahi, d, -rint(p)), the reduction would already hold the rounding error that pe
// adds again (a phase error of ulp(a d), ~1e-11 cycles at config-3 arguments).
__device__ __forceinline__ double nu_frac_prod(double ahi, double alo, double d) {
#pragma clang fp contract(off)
    const double p = ahi * d;
    const double pe = fma(ahi, d, -p) + alo * d;
    return (p - rint(p)) + pe;
}

// frac(c2 d^2) with d^2 = d2 + d2e (double-double), contraction off as nu_frac_prod
__device__ __forceinline__ double nu_frac_c2(double c2, double d2, double d2e) {
#pragma clang fp contract(off)
    const double qv = c2 * d2;
    const double qe = fma(c2, d2, -qv) + c2 * d2e;
    return (qv - rint(qv)) + qe;
}

// frac(k phi) for |phi| <= 1/2, the product's rounding error carried (contraction off)
__device__ __forceinline__ double nu_frac_k(double kd, double phi) {
#pragma clang fp contract(off)
    const double hk = kd * phi;
    const double hl = fma(kd, phi, -hk);
    return (hk - rint(hk)) + hl;
}

// Chebyshev-Bessel expansion of the moments' phase factor (Jacobi-Anger): for |e| <= 1/2 and theta = 2 pi jc / n,
//   e^{i theta e} = sum_p eps_p i^p J_p(theta / 2) T_p(2 e),  eps_0 = 1, eps_p = 2,
// so the spread accumulates Chebyshev moments sum c_i T_p(2 e_i) and the combine weights moment p's transform by
// eps_p i^p J_p(z), z = pi jc / n (|z| <= pi / 2). Truncating at P moments errs by <= 2 N sum_{p >= P} (|z|/2)^p / p!
// (< 2.4 N (|z|/2)^P / P! for P >= 4), against N (2|z|)^P / P! for Taylor moments e^p: 20 -> 16 moments at config 3.
// J_p(z) = (z/2)^p sum_{m < kNuBesM} y^m / (m! (m+p)!), y = -(z/2)^2 (|y| <= 0.617: the omitted terms < 4e-18 of
// J_p); the coefficients 1 / (m! (m+p)!) come from the host tables (nu_tables), read at uniform indices.
constexpr int kNuBesP = 26, kNuBesM = 12;
__device__ __forceinline__ double nu_bes_series(const double* __restrict__ bc, int p, double y) {
    const double* c = bc + p * kNuBesM;
    double f = c[kNuBesM - 1];
#pragma unroll
    for (int m = kNuBesM - 2; m >= 0; --m) f = fma(f, y, c[m]);
    return f;  // J_p(z) / (z/2)^p
}
// The combine walks the moments from P-1 down to 0 with J_p by the backward recurrence
// J_p = (2 (p+1) / z) J_p+1 - J_p+2 (stable: J_p is its minimal solution), started from J_P, J_P+1 by the series.
// z = 0 (jc = 0): J_p = 0 for p > 0 (zero start, 2/z taken as 0) and J_0 = 1 (nu_bes_w).
struct NuBes {
    double j1, j2, iz2;  // J_p+1, J_p+2, 2/z
};
__device__ __forceinline__ NuBes nu_bes_start(const double* __restrict__ bc, int P, double zh) {
    double zp = 1.0;
    for (int p = 0; p < P; ++p) zp *= zh;  // (z/2)^P
    const double y = -zh * zh;
    NuBes b;
    b.j1 = zp * nu_bes_series(bc, P, y);
    b.j2 = (zp * zh) * nu_bes_series(bc, P + 1, y);
    b.iz2 = zh != 0.0 ? 1.0 / zh : 0.0;
    return b;
}
// eps_p J_p for moment p (descending calls p = P-1 .. 0), advancing the recurrence
__device__ __forceinline__ double nu_bes_w(NuBes& b, int p, double zh) {
    double j = fma((double)(p + 1) * b.iz2, b.j1, -b.j2);
    b.j2 = b.j1;
    b.j1 = j;
    if (p == 0) return zh != 0.0 ? j : 1.0;
    return 2.0 * j;
}
// acc + w i^p v (p uniform)
__device__ __forceinline__ double2 nu_bes_acc(double2 acc, double w, double2 v, int p) {
    switch (p & 3) {
        case 0: return make_double2(fma(w, v.x, acc.x), fma(w, v.y, acc.y));
        case 1: return make_double2(fma(-w, v.y, acc.x), fma(w, v.x, acc.y));
        case 2: return make_double2(fma(-w, v.x, acc.x), fma(-w, v.y, acc.y));
        default: return make_double2(fma(w, v.y, acc.x), fma(-w, v.x, acc.y));
    }
}
// z/2 = (pi/2) jc / n for an FFT output position holding trial offset jc
__device__ __forceinline__ double nu_zh(int64_t jc, int lnfft) {
    return ldexp((double)jc, -lnfft) * 1.5707963267948966192313216916398;
}
// T_p(u), p < 32, by the doubling ladder (T_2m = 2 T_m^2 - 1, T_2m+1 = 2 T_m T_m+1 - u) -- the MFMA spread's lanes
// each need one p
__device__ __forceinline__ double nu_cheb(double u, int p) {
    double a = 1.0, b = u;  // (T_m, T_m+1), m = 0
#pragma unroll
    for (int bit = 4; bit >= 0; --bit) {
        const double ab = fma(2.0 * a, b, -u);
        if ((p >> bit) & 1) {
            b = fma(2.0 * b, b, -1.0);
            a = ab;
        } else {
            a = fma(2.0 * a, a, -1.0);
            b = ab;
        }
    }
    return a;
}

// T_p(x) = x^(p & 1) Q_p(x^2) with Q_p's monomial coefficients (exact integers), p < 16: the MFMA spread's lane
// evaluates its own T_p by a degree-7 Horner in y = x^2 (9 fp64 operations; the doubling ladder nu_cheb took ~30
// plus selects). |x| <= 1, so the rounding is at most ~sum |c| ulp: 2e-11 absolute for T_15, whose weight in the
// combine is |2 J_15(pi/2)| < 3e-14 (nu_bes); ~1e-15 for the p <= 4 moments that carry the sums.
__constant__ double kNuChebMono[16][8] = {
    {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {-1.0, 2.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {-3.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {1.0, -8.0, 8.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {5.0, -20.0, 16.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {-1.0, 18.0, -48.0, 32.0, 0.0, 0.0, 0.0, 0.0},
    {-7.0, 56.0, -112.0, 64.0, 0.0, 0.0, 0.0, 0.0},
    {1.0, -32.0, 160.0, -256.0, 128.0, 0.0, 0.0, 0.0},
    {9.0, -120.0, 432.0, -576.0, 256.0, 0.0, 0.0, 0.0},
    {-1.0, 50.0, -400.0, 1120.0, -1280.0, 512.0, 0.0, 0.0},
    {-11.0, 220.0, -1232.0, 2816.0, -2816.0, 1024.0, 0.0, 0.0},
    {1.0, -72.0, 840.0, -3584.0, 6912.0, -6144.0, 2048.0, 0.0},
    {13.0, -364.0, 2912.0, -9984.0, 16640.0, -13312.0, 4096.0, 0.0},
    {-1.0, 98.0, -1568.0, 9408.0, -26880.0, 39424.0, -28672.0, 8192.0},
    {-15.0, 560.0, -6048.0, 28800.0, -70400.0, 92160.0, -61440.0, 16384.0}};

__device__ __forceinline__ int64_t nu_readlane64(int64_t v, int lane) {
    const int lo = __builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, lane);
    const int hi = __builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), lane);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

// sortedness of dt (the spread's cells only grow along a chunk)
__global__ __launch_bounds__(256) void k_nu_sorted(const double* __restrict__ tt, double t0, int64_t n, int* __restrict__ bad) {
    int b = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 1 < n; i += (int64_t)gridDim.x * blockDim.x)
        b |= !((tt[i] - t0) <= (tt[i + 1] - t0));
    if (__any(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}

// Moments of harmonics k0 .. k0+G-1 for rows [0, nrow) of the pass (c2row points at the pass's first row).
// Lane l: photon q = l >> 4 of the K-group, A row (moment) p = l & 15, B column col = l & 15 = 2 row + (re/im).
template <int G, bool TWOD>
__global__ __launch_bounds__(256) void k_nu_spread(const double* __restrict__ tt, double t0, int64_t n, int64_t nchunk, double s1,
                                                   double fch, double fcl, const double* __restrict__ c2row, int nrow,
                                                   int k0, int P, const NuPass* __restrict__ ps,
                                                   const double2* __restrict__ tab, double* __restrict__ U,
                                                   int64_t* __restrict__ ctab, const int* __restrict__ bad) {
    if (*bad) return;  // photons out of order or a cached plan that no longer holds (k_ap_final)
    // the cis table in LDS (read twice per photon and K-group: an L2 round trip each, waited for at once), filled
    // before any wave leaves
    __shared__ double2 stab[1024];
    for (int e = threadIdx.x; e < 1024; e += 256) stab[e] = tab[e];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * kNuWaves + (threadIdx.x >> 6);
    if (c >= nchunk) return;  // wave-uniform
    const int q = lane >> 4, col = lane & 15, prow = col >> 1, reim = col & 1, pp = lane & 15;
    const bool rowok = prow < nrow, pok = pp < P;
    const double c2 = (TWOD && rowok) ? c2row[prow] : 0.0;
    double cm[8];  // this lane's T_pp in monomials of (2e)^2 (kNuChebMono); rows p >= P of D are never stored
#pragma unroll
    for (int m = 0; m < 8; ++m) cm[m] = kNuChebMono[pp][m];
    const bool odd = pp & 1;
    (void)pok;
    const int64_t i0 = c * kNuCW, i1 = i0 + kNuCW < n ? i0 + kNuCW : n;
    const int64_t SL = 2 * (int64_t)P * nrow;  // doubles per slot: [p][row][re, im]
    nu_f64x4 acc[G];
    int gcur[G];  // cells fit 32 bits (nu_plan: |G| + n < 2^31)
    {
        const double u1 = (tt[i0] - t0) * s1;
#pragma unroll
        for (int kk = 0; kk < G; ++kk) {
            acc[kk] = nu_f64x4{0.0, 0.0, 0.0, 0.0};
            gcur[kk] = (int)rint((double)(k0 + kk) * u1);
            if (lane == 0) ctab[(kk * nchunk + c) * 2] = gcur[kk];  // the chunk's first cell
        }
    }
    auto flush = [&](int kk) {
        const int64_t slot = (int64_t)gcur[kk] - ps->gmin[kk] + c;
        double* const base = U + ps->ubase[kk] + slot * SL;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = q + 4 * r;  // D row of register r
            if (p < P && rowok) base[(p * nrow + prow) * 2 + reim] = acc[kk][r];
        }
        acc[kk] = nu_f64x4{0.0, 0.0, 0.0, 0.0};
    };
    // cells the chunk's photons skip (observation gaps): their slots lie inside the chunk's cell range, which the
    // merge reads, so they are written as zeros
    auto zero_gap = [&](int kk, int64_t from, int64_t to) {
        for (int64_t cell = from + 1; cell < to; ++cell) {
            double* const base = U + ps->ubase[kk] + (cell - ps->gmin[kk] + c) * SL;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = q + 4 * r;
                if (p < P && rowok) base[(p * nrow + prow) * 2 + reim] = 0.0;
            }
        }
    };
    // past the end: the last photon's time (same cell, zero weight); the next tile's times are loaded (raw) during
    // the current one
    double tn = tt[i0 + lane < n ? i0 + lane : n - 1];
    for (int64_t ib = i0; ib < i1; ib += 64) {
        const double dv = tn - t0;
        const int64_t il = ib + 64 + lane;
        tn = tt[il < n ? il : n - 1];
#pragma unroll 1
        for (int g = 0; g < 16; ++g) {
            if (ib + 4 * g >= i1) break;  // wave-uniform
            const double d = __shfl(dv, 4 * g + q, 64);
            const bool valid = ib + 4 * g + q < i1;
            // premultiplier phase (cycles): frac(fc d) + frac(c2 d^2), in double-double, then harmonic k0
            double phi = nu_frac_prod(fch, fcl, d);
            if (TWOD) {
                const double d2 = d * d, d2e = fma(d, d, -d2);
                phi += nu_frac_c2(c2, d2, d2e);
            }
            phi -= rint(phi);
            const double2 c1 = nu_cis(stab, phi);
            double2 ck = c1;
            if (k0 > 1) ck = nu_cis(stab, nu_frac_k((double)k0, phi));
            // this lane's B column as the real part of cl: c for re lanes, (-i) c for im lanes; zero for a photon
            // past the chunk's end or a row beyond the pass (products by c1 keep it zero, and A needs no mask:
            // its rows p >= P are never stored). One select per K-group instead of per harmonic.
            double2 cl = reim ? make_double2(ck.y, -ck.x) : ck;
            if (!(valid && rowok)) cl = make_double2(0.0, 0.0);
            const double u1 = d * s1;
#pragma unroll
            for (int kk = 0; kk < G; ++kk) {
                if (kk > 0) cl = nu_cmul(cl, c1);
                const double uk = (double)(k0 + kk) * u1;
                const double gk = rint(uk);
                const double e = uk - gk;
                const double x = 2.0 * e, y = x * x;  // T_p(2e) (nu_bes) by Horner in y
                double a = cm[7];
#pragma unroll
                for (int m = 6; m >= 0; --m) a = fma(a, y, cm[m]);
                if (odd) a *= x;
                const double b = cl.x;
                const int G32 = (int)gk;  // 32-bit cells and read-lanes
                const int g0 = __builtin_amdgcn_readlane(G32, 0), g3 = __builtin_amdgcn_readlane(G32, 48);
                if (g0 == gcur[kk] && g3 == gcur[kk]) {
                    acc[kk] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[kk], 0, 0, 0);
                } else {
                    // the K-group crosses cells: photons of the current cell first, then each later cell in turn
                    const int g1 = __builtin_amdgcn_readlane(G32, 16), g2 = __builtin_amdgcn_readlane(G32, 32);
                    for (;;) {
                        if (g0 <= gcur[kk]) {
                            const double am = (G32 == gcur[kk]) ? a : 0.0;
                            acc[kk] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, b, acc[kk], 0, 0, 0);
                        }
                        if (g3 == gcur[kk]) break;
                        flush(kk);
                        const int nx = g0 > gcur[kk] ? g0 : g1 > gcur[kk] ? g1 : g2 > gcur[kk] ? g2 : g3;
                        if (nx > gcur[kk] + 1) zero_gap(kk, gcur[kk], nx);
                        gcur[kk] = nx;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int kk = 0; kk < G; ++kk) {
        flush(kk);
        if (lane == 0) ctab[(kk * nchunk + c) * 2 + 1] = gcur[kk];  // the chunk's last cell
    }
}

// ---- cell-gather spread (a pass of <= kNuGatherRows rows, one harmonic): one lane per wrapped cell ----
// start[G - gmin] = the first photon whose cell (rint(k (dt s1)), the spread's arithmetic) is >= G, for the
// unwrapped cells G in [gmin, gmax + 1]; photons are time-sorted, so cell G holds photons [start[G], start[G+1]).
// Up to kNuCellK harmonics k0 .. k0+nk-1 per launch (one read of the photon times): harmonic k0 + j writes its
// table at start + off[j] for cells gmin[j] .. gmin[j] + span[j] - 1.
// The cell gather's plans take the photon order from here too (no k_nu_sorted pass): a pair out of order sets *bad
// (the search then takes the default path) and the writes stay inside the tables (every cell is clamped to its
// harmonic's range). The tables are not zeroed: on unsorted photons the gathers read none of them (*bad).
// Photon pairs (one 16-byte load when t is 16-byte aligned, VEC), kNuCellU pairs per thread and sweep with their
// loads issued together, over at most 2048 blocks: the predecessor of a pair's first photon is the previous lane's
// second one (a shuffle; lane 0 loads it). One 8-byte load per iteration ran at ~2 TB/s, and one pair per thread
// over a grid covering the photons (19.5k short blocks at config 3) was bound by the workgroup dispatch: 35-43 us per
// 80 MB either way.
// A wave that finds a pair out of order among its photons of a sweep writes nothing for them: on sorted photons
// every wave is clean and the tables complete; on unsorted ones the search is discarded anyway (*bad), and a
// skipped wave cannot run a long write loop for a backward-then-forward jump (the gathers never read the tables).
constexpr int kNuCellU = 4;
template <bool VEC>
__global__ __launch_bounds__(256) void k_nu_cellstart(const double* __restrict__ tt, double t0, int64_t n, double s1,
                                                      int k0, int nk, NuCellArgs a, int64_t* __restrict__ start,
                                                      int* __restrict__ bad) {
    if (*bad) return;  // a cached plan that no longer holds (k_ap_final): no table is written
    const int64_t npair = (n + 1) / 2, stride = (int64_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    int b = 0;
    // block-uniform loop bound (the barrier of __syncthreads_or below)
    for (int64_t p0b = (int64_t)blockIdx.x * blockDim.x; p0b < npair; p0b += kNuCellU * stride) {
        double x0[kNuCellU], x1[kNuCellU], xl[kNuCellU];
#pragma unroll
        for (int q = 0; q < kNuCellU; ++q) {
            const int64_t pr = p0b + threadIdx.x + q * stride, i0 = 2 * pr;
            if (VEC && i0 + 1 < n) {
                const double2 v = reinterpret_cast<const double2*>(tt)[pr];
                x0[q] = v.x;
                x1[q] = v.y;
            } else {
                x0[q] = tt[i0 < n ? i0 : n - 1];
                x1[q] = tt[i0 + 1 < n ? i0 + 1 : n - 1];
            }
            xl[q] = 0.0;
            if (lane == 0) xl[q] = tt[i0 > 0 && i0 - 1 < n ? i0 - 1 : 0];  // the wave's first predecessor
        }
#pragma unroll
        for (int q = 0; q < kNuCellU; ++q) {
            const int64_t i0 = 2 * (p0b + threadIdx.x + q * stride);
            double xp = __shfl_up(x1[q], 1, 64);
            if (lane == 0) xp = xl[q];
            const double d0 = x0[q] - t0, d1 = x1[q] - t0;
            const double dp0 = i0 == 0 ? d0 : xp - t0;
            const bool v0 = i0 < n, v1 = i0 + 1 < n;
            const int ooo = (v0 && !(dp0 <= d0)) || (v1 && !(d0 <= d1));
            b |= ooo;
            // a wave that holds a pair out of order writes nothing for its photons (a vote, no block barrier: the
            // barrier cost a quarter of the pass)
            if (__any(ooo)) continue;
            // per harmonic the cells of the predecessor and of the pair's two photons, each formed once (the second
            // photon's range starts at the first one's cell); cells fit 32 bits (nu_plan checks |G| + n < 2^31): one
            // v_cvt_i32_f64 each, and 32-bit bounds
            const double up = dp0 * s1, u0 = d0 * s1, u1 = d1 * s1;
#pragma unroll
            for (int j = 0; j < kNuCellK; ++j) {
                if (j >= nk) break;
                const double kd = (double)(k0 + j);
                const int gm = (int)a.gmin[j], gl = (int)(a.gmin[j] + a.span[j] - 1);
                int64_t* st = start + a.off[j];
                const int gA = i0 == 0 ? gm - 1 : (int)rint(kd * up);
                const int gB = (int)rint(kd * u0);
                if (v0) {  // photon i0 starts the cells (gA, gB]
                    const int lo = gA + 1 > gm ? gA + 1 : gm, hi = gB < gl ? gB : gl;
                    for (int G = lo; G <= hi; ++G) st[G - gm] = i0;
                    if (i0 == n - 1) st[a.span[j]] = n;
                }
                if (v1) {  // photon i0 + 1 the cells (gB, gC]
                    const int gC = (int)rint(kd * u1);
                    const int lo = gB + 1 > gm ? gB + 1 : gm, hi = gC < gl ? gC : gl;
                    for (int G = lo; G <= hi; ++G) st[G - gm] = i0 + 1;
                    if (i0 + 1 == n - 1) st[a.span[j]] = n;
                }
            }
        }
    }
    if (__any(b) && lane == 0) atomicOr(bad, 1);
}

// L lanes per wrapped cell g sum, over its unwrapped cells G = g (mod n) and their photons in time order (lane s
// takes the cell's photons s, s + L, ...), the moments c_r T_p(2e) of rows r < nrow: b_p,r[g] = sum c_{i,r} T_p(2e_i) with
// c = e^{2 pi i k (fc dt + c2_r dt^2)}, e = k dt s1 - G, in registers; an xor butterfly over the L lanes (a fixed
// order: deterministic) completes the sums and lane s writes the moments p = s (mod L) to W[p * nrow + r][g].
// fp64 VALU throughout: per photon, row and harmonic one premultiplier phase and cis, then 3 operations per moment.
// L > 1 spreads a cell's photons over several lanes when cells are dense (many photons per cell, few cells).
// One launch serves up to kNuGatherSet harmonics (NuGatherSet: block ranges, cells, lanes per cell and W plane of
// each): the harmonics of a search share the launch's waves, so its last round of blocks is not one harmonic's tail
// (config 3 ran two launches of 1.7 and 3.4 rounds of resident waves).
// x of the lane a quad_perm DPP control picks inside each quad of lanes (two bits per lane, lane 0's first)
template <int CTRL>
__device__ __forceinline__ double nu_quad_perm(double x) {
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// CHECK: the start tables are a cached plan's (NuPlanCache::find), built from the photons an earlier search read. Every
// lane then verifies what the tables assume of the photons it weights: each sits in the lane's cell G -- the cell
// k_nu_cellstart forms, (int)rint(k (dt s1)), a product alone, so nothing contracts -- and the photons of a cell do not
// descend in index order (neighbours through a rotation inside the L-group, checked by the set's first harmonic only:
// every harmonic's cells hold every photon). The tables partition [0, n), so with every photon in the cell that owns
// it the sums are those of fresh tables, and the order is the order k_nu_cellstart demands (cells ascend with dt).
// A failing wave ORs 2 into *bad: the host drops the plan and redoes the search (nufft_search reads the flag first);
// the kernels after this one then run on W that is wrong but in bounds -- every start lies in [0, n].
// A folded search (NuFold::epoch != 0; NuRun::fold) launches nothing before its first gather, so nothing has zeroed
// *bad: the kernel takes no entry test (a stale word would stop it), and a failing wave plain-stores the search's
// epoch into bad[1] instead -- stores of one value cannot race, and a word left by an earlier search never equals
// this search's epoch. Its first launch carries ncheck leading blocks that do k_ap_check's work on the trial grid
// and leave before the cis table's fill and barrier: the lowest block indices, dispatched first, done while the
// gather's waves run. Block 0 also publishes the plan's scalars as k_ap_final forms them and zeroes the fix-up count
// bad[-1] (only later launches add to it) and the legacy flag bad[0] (nothing in a folded search reads or sets it
// before the host does). The host finishes the check from the read-back (search_nufft_finish.h).
struct NuFold {
    int epoch = 0;   // 0: not folded
    int ncheck = 0;  // leading check blocks of this launch
    const double* f = nullptr;
    int64_t nf = 0, n = 0;
    double* pub = nullptr;    // [f[0], f[nf-1], t[0] - t0, t[n-1] - t0]
    double2* part = nullptr;  // [ncheck] (max deviation, max |f|)
};
template <int R, bool TWOD, int PP, bool CHECK>  // PP >= P moments accumulated unconditionally (no per-moment selects)
__global__ __launch_bounds__(256) void k_nu_gather(const double* __restrict__ tt, double t0,
                                                   const int64_t* __restrict__ startb, int64_t nfft, double s1,
                                                   double fch, double fcl, const double* __restrict__ c2row, int nrow,
                                                   int P, const NuGatherSet S, int* __restrict__ bad,
                                                   const double2* __restrict__ tab, double2* __restrict__ Wb,
                                                   const NuFold F) {
    const bool folded = CHECK && F.epoch != 0;  // launch-uniform
    int64_t blk = blockIdx.x;
    if (folded) {
        if (blk < F.ncheck) {  // block-uniform: a check block
            const double2 r = ap_check_block(F.f, F.nf, (int)blk, F.ncheck);
            if (threadIdx.x == 0) {
                F.part[blk] = r;
                if (blk == 0) {
                    F.pub[0] = F.f[0];
                    F.pub[1] = F.f[F.nf - 1];
                    F.pub[2] = tt[0] - t0;
                    F.pub[3] = tt[F.n - 1] - t0;
                    bad[-1] = 0;
                    bad[0] = 0;
                }
            }
            return;
        }
        blk -= F.ncheck;
    } else if (*bad) {
        // photons out of order (the cell starts found it): the start tables are not filled (nothing zeroes them), so
        // no lane may read them; the search's results are discarded and the default path runs
        return;
    }
    __shared__ double2 stab[2048];  // the cis table (nu_cis2), read per photon: LDS, not L2 latency
    for (int e = threadIdx.x; e < 2048; e += 256) stab[e] = tab[e];
    __syncthreads();
    int j = 0;  // this block's harmonic (block-uniform)
    while (j + 1 < S.nk && blk >= S.blk0[j + 1]) ++j;
    const int ll = S.lanes_log2[j], L = 1 << ll;
    const int64_t tid = (blk - S.blk0[j]) * 256 + threadIdx.x;
    const int64_t idx = tid >> ll;
    const int sub = (int)(tid & (L - 1));
    if (idx >= S.gcount[j]) return;  // whole L-groups leave together (L divides 64); no barrier below
    const int64_t gmin = S.gmin[j], gmax = S.gmax[j];
    const int64_t* __restrict__ start = startb + S.soff[j];
    double2* __restrict__ W = Wb + S.woff[j];
    const int64_t g = (S.gbase[j] + idx) & (nfft - 1);  // the FFT's occupied rows only (nu_occupied)
    double ar[R][PP], ai[R][PP];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int p = 0; p < PP; ++p) ar[r][p] = ai[r][p] = 0.0;
    double c2[R];
#pragma unroll
    for (int r = 0; r < R; ++r) c2[r] = (TWOD && r < nrow) ? c2row[r] : 0.0;
    const double kd = (double)S.k[j];
    const bool order_check = CHECK && j == 0;  // block-uniform
    const int lane = threadIdx.x & 63;
    int fail = 0;
    // the photon times are prefetched raw and unconditionally (indices clamped into the cell, whose stand-ins are
    // never weighted): a load whose value entered a select or a subtraction at its issue would be waited for there;
    // the next cell's photon range is loaded during the current cell
    int64_t G = gmin + (((g - gmin) % nfft) + nfft) % nfft;
    int64_t ns0 = 0, ns1 = 0;
    if (G <= gmax) {
        ns0 = start[G - gmin];
        ns1 = start[G - gmin + 1];
    }
    for (; G <= gmax; G += nfft) {
        const int64_t i0 = ns0, i1 = ns1;
        if (G + nfft <= gmax) {
            ns0 = start[G + nfft - gmin];
            ns1 = start[G + nfft - gmin + 1];
        }
        if (i1 <= i0) continue;  // an empty cell (no clamped load below i0)
        const double Gd = (double)G;
        const int Gi = (int)G;  // cells fit 32 bits (nu_plan)
        double dlast = 0.0;     // dt of the L-group's last photon of the previous iteration
        // two photons per iteration (independent chains for the VALU; each one's terms still added in photon
        // order), their times prefetched two iterations ahead (HBM latency is several iterations of one wave)
        const int64_t il = i1 - 1;
        double dn[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) dn[q] = tt[i0 + sub + q * L < il ? i0 + sub + q * L : il];
        for (int64_t i = i0 + sub; i < i1; i += 2 * L) {
            const bool hb = i + L < i1;
            const double da = dn[0] - t0, db = (hb ? dn[1] : dn[0]) - t0;  // (no second photon: a stand-in, weight 0)
            dn[0] = dn[2];
            dn[1] = dn[3];
            dn[2] = tt[i + 4 * L < il ? i + 4 * L : il];
            dn[3] = tt[i + 5 * L < il ? i + 5 * L : il];
            const double ea = kd * (da * s1) - Gd, eb = kd * (db * s1) - Gd;
            if (CHECK) {
                // |e| clearly below 1/2 settles the cell: the product k (dt s1) the cell-start pass rounds lies within
                // 2^-23 of the unrounded one e is formed from (|cell| < 2^31), so its rint is G. Else (a cell's edge,
                // or a photon of another cell) the pass's own expression decides -- dt s1 formed again behind an
                // empty asm: were that product shared with e, the compiler would no longer fuse it into e's
                // subtraction, and the moments would differ in the last bits from the fresh plan's
                constexpr double sure = 0.5 - 0x1p-20;
                if (!(fabs(ea) < sure && (!hb || fabs(eb) < sure))) {
                    double ua = da * s1, ub = db * s1;
                    asm volatile("" : "+v"(ua), "+v"(ub));
                    fail |= (int)rint(kd * ua) != Gi || (hb && (int)rint(kd * ub) != Gi);
                }
                if (order_check) {
                    // the cell's photons of this iteration in index order: da of lanes 0 .. L-1, then db of lanes
                    // 0 .. L-1. Every lane hands (da, db) to the next lane of its L-group, the last to lane 0: a
                    // lane's predecessors are the two it receives, lane 0's are the db of the last lane from the
                    // previous iteration (kept in dlast) and that lane's da. The L-group runs its cell's iterations
                    // together, and a received value is used only where the lane it comes from holds a real photon in
                    // this iteration (a lower index than the user's).
                    // (the rotation inside pairs and quads is one DPP move per register, no LDS round trip)
                    double xa = da, xb = db;
                    if (L == 2) {
                        xa = nu_quad_perm<0xB1>(da);  // lanes 1 0 3 2
                        xb = nu_quad_perm<0xB1>(db);
                    } else if (L == 4) {
                        xa = nu_quad_perm<0x93>(da);  // lanes 3 0 1 2
                        xb = nu_quad_perm<0x93>(db);
                    } else if (L > 4) {
                        const int from = sub ? lane - 1 : lane | (L - 1);
                        xa = __shfl(da, from);
                        xb = __shfl(db, from);
                    }
                    const double preva = sub ? xa : dlast, prevb = sub ? xb : xa;
                    fail |= ((sub || i > i0) && !(preva <= da)) || (hb && !(prevb <= db));
                    dlast = xb;
                }
            }
            const double p1a = nu_frac_prod(fch, fcl, da), p1b = nu_frac_prod(fch, fcl, db);
            double d2a = 0.0, d2ea = 0.0, d2b = 0.0, d2eb = 0.0;
            if (TWOD) {
                d2a = da * da;
                d2ea = fma(da, da, -d2a);
                d2b = db * db;
                d2eb = fma(db, db, -d2b);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r < nrow) {
                    double phia = p1a, phib = p1b;
                    if (TWOD) {
                        phia += nu_frac_c2(c2[r], d2a, d2ea);
                        phib += nu_frac_c2(c2[r], d2b, d2eb);
                    }
                    phia -= rint(phia);
                    phib -= rint(phib);
                    const double2 ca = nu_cis2(stab, nu_frac_k(kd, phia));
                    double2 cb = nu_cis2(stab, nu_frac_k(kd, phib));
                    if (!hb) cb = make_double2(0.0, 0.0);
                    // Chebyshev moments T_p(2e): T_p+1 = 4e T_p - T_p-1 (nu_bes)
                    const double ua = 4.0 * ea, ub = 4.0 * eb;
                    double ta0 = 1.0, ta1 = 2.0 * ea, tb0 = 1.0, tb1 = 2.0 * eb;
#pragma unroll
                    for (int p = 0; p < PP; ++p) {
                        ar[r][p] = fma(ca.x, ta0, ar[r][p]);
                        ai[r][p] = fma(ca.y, ta0, ai[r][p]);
                        ar[r][p] = fma(cb.x, tb0, ar[r][p]);
                        ai[r][p] = fma(cb.y, tb0, ai[r][p]);
                        const double ta2 = fma(ua, ta1, -ta0), tb2 = fma(ub, tb1, -tb0);
                        ta0 = ta1;
                        ta1 = ta2;
                        tb0 = tb1;
                        tb1 = tb2;
                    }
                }
            }
        }
    }
    if (CHECK) {
        const unsigned long long failed = __ballot(fail);
        if (failed && lane == __ffsll(failed) - 1) {
            if (folded)
                bad[1] = F.epoch;
            else
                atomicOr(bad, 2);
        }
    }
    for (int o = L / 2; o > 0; o >>= 1)  // block-uniform L
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int p = 0; p < PP; ++p)
                if (p < P) {  // uniform
                    ar[r][p] += __shfl_xor(ar[r][p], o);
                    ai[r][p] += __shfl_xor(ai[r][p], o);
                }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int p = 0; p < PP; ++p)
            if (r < nrow && p < P && (p & (L - 1)) == sub)
                W[((int64_t)p * nrow + r) * nfft + g] = make_double2(ar[r][p], ai[r][p]);
}

// slots -> W[beta][g] (beta = p * nrow + row, complex), for the wrapped cells g of one block
__global__ __launch_bounds__(256) void k_nu_merge(const double* __restrict__ U, int64_t SL,
                                                  const int64_t* __restrict__ ctab, int64_t nchunk, int64_t gmin,
                                                  int64_t gmax, int64_t nfft, int64_t gbase, int64_t gcount,
                                                  double2* __restrict__ W, const int* __restrict__ bad) {
    if (*bad) return;  // the spread did not run (k_nu_spread): its slots and cell table are not written
    __shared__ int64_t rs[kNuMergeG][kNuMaxWrap];
    __shared__ int rc[kNuMergeG][kNuMaxWrap];
    __shared__ int nr[kNuMergeG];
    extern __shared__ double nu_acc[];  // [kNuMergeG][SL]
    const int64_t i0 = (int64_t)blockIdx.x * kNuMergeG;  // cells gbase + i (mod n), i < gcount: the occupied rows
    const int tid = threadIdx.x;
    if (tid < kNuMergeG) {
        const int64_t g = (gbase + i0 + tid) & (nfft - 1);
        int cnt = 0;
        if (i0 + tid < gcount) {
            int64_t Gu = gmin + (((g - gmin) % nfft) + nfft) % nfft;  // smallest unwrapped cell >= gmin, = g mod n
            for (; Gu <= gmax && cnt < kNuMaxWrap; Gu += nfft) {
                int64_t lo = 0, hi = nchunk;  // first chunk whose last cell is >= Gu
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (ctab[2 * mid + 1] < Gu)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                int len = 0;
                while (lo + len < nchunk && ctab[2 * (lo + len)] <= Gu) ++len;
                if (len > 0) {
                    rs[tid][cnt] = Gu - gmin + lo;
                    rc[tid][cnt] = len;
                    ++cnt;
                }
            }
        }
        nr[tid] = cnt;
    }
    __syncthreads();
    for (int64_t idx = tid; idx < kNuMergeG * SL; idx += 256) {
        const int t = (int)(idx / SL);
        const int64_t e = idx - t * SL;
        double v = 0.0;
        for (int r = 0; r < nr[t]; ++r)
            for (int k = 0; k < rc[t][r]; ++k) v += U[(rs[t][r] + k) * SL + e];
        nu_acc[idx] = v;
    }
    __syncthreads();
    const int64_t B = SL / 2;
    for (int64_t idx = tid; idx < kNuMergeG * B; idx += 256) {
        const int t = (int)(idx % kNuMergeG);
        const int64_t beta = idx / kNuMergeG;
        if (i0 + t < gcount) {
            const int64_t g = (gbase + i0 + t) & (nfft - 1);
            W[beta * nfft + g] = make_double2(nu_acc[t * SL + 2 * beta], nu_acc[t * SL + 2 * beta + 1]);
        }
    }
}

// Power and error bound of one trial from its harmonic sums: CS[k * nbt + t] for k < m, except that with lastv the
// last harmonic's sum is the register value `last` (the fused row pass, k_nu_rows_combine8). The same operations
// in the same order either way, so the fused and separate finalize give identical powers and flags.
__device__ __forceinline__ void nu_power(const double2* __restrict__ CS, int64_t nbt, int64_t t, int m, int stat,
                                         double nph, double E, bool lastv, double2 last, double* pout,
                                         double* eout) {
    const double w = 2.0 / nph;
    auto zk = [&](int k, double* amag) {
        const double2 a = (lastv && k == m - 1) ? last : CS[(int64_t)k * nbt + t];
        const double z = a.x * a.x + a.y * a.y;
        *amag = sqrt(z);
        return z;
    };
    double p, err;
    if (stat == CRIMP_STAT_Z2) {
        double zsum = 0.0, eb = 0.0, am;
        for (int k = 0; k < m; ++k) {
            zsum += zk(k, &am);
            eb += 2.0 * am * E + E * E;
        }
        p = zsum * w;
        err = eb * w;
    } else {
        double cum = 0.0, best = -INFINITY, ebest = 0.0, eacc = 0.0, am;
        for (int k = 0; k < m; ++k) {
            const double z = zk(k, &am);
            cum += z * w;
            eacc += (2.0 * am * E + E * E) * w;
            const double v = cum - 4.0 * (double)k;
            if (v > best) {
                best = v;
                ebest = eacc;
            }
        }
        p = best;
        err = ebest;
        cum = 0.0;
        eacc = 0.0;
        for (int k = 0; k < m; ++k) {
            const double z = zk(k, &am);
            cum += z * w;
            eacc += (2.0 * am * E + E * E) * w;
            if (cum - 4.0 * (double)k + eacc >= best - ebest) err = fmax(err, eacc);
        }
    }
    *pout = p;
    *eout = err;
}
// E = N (x^P invfact + kNuRho) at trial offset jc (nu_trunc)
__device__ __forceinline__ double nu_err_bound(int64_t jc, int64_t nfft, int P, double invfact, double nph) {
    const double x = 3.14159265358979323846 * fabs((double)jc) / (double)nfft;
    double xp = 1.0;
    for (int p = 0; p < P; ++p) xp *= x;
    return nph * (xp * invfact + kNuRho);
}

// ---- FFT: DFTs of radix 2..16 in registers (X_k = sum_j x_j w_R^{+jk}, natural order) ----
__device__ __forceinline__ void nu_dft2(double2* v) {
    const double2 a = v[0], b = v[1];
    v[0] = nu_add(a, b);
    v[1] = nu_sub(a, b);
}
__device__ __forceinline__ void nu_dft4(double2& a0, double2& a1, double2& a2, double2& a3) {
    const double2 t0 = nu_add(a0, a2), t1 = nu_sub(a0, a2), t2 = nu_add(a1, a3), t3 = nu_muli(nu_sub(a1, a3));
    a0 = nu_add(t0, t2);
    a2 = nu_sub(t0, t2);
    a1 = nu_add(t1, t3);
    a3 = nu_sub(t1, t3);
}
__device__ __forceinline__ void nu_dft4v(double2* v) { nu_dft4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void nu_dft8(double2* v) {
    double2 e[4] = {v[0], v[2], v[4], v[6]}, o[4] = {v[1], v[3], v[5], v[7]};
    nu_dft4v(e);
    nu_dft4v(o);
    const double s = 0.70710678118654752440084436210485;
    const double2 w[4] = {make_double2(1.0, 0.0), make_double2(s, s), make_double2(0.0, 1.0), make_double2(-s, s)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double2 t = k == 0 ? o[0] : k == 2 ? nu_muli(o[2]) : nu_cmul(o[k], w[k]);
        v[k] = nu_add(e[k], t);
        v[k + 4] = nu_sub(e[k], t);
    }
}
__device__ __forceinline__ void nu_dft16(double2* v) {
    double2 e[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        e[k] = v[2 * k];
        o[k] = v[2 * k + 1];
    }
    nu_dft8(e);
    nu_dft8(o);
    const double c1 = 0.92387953251128675612818318939679, s1 = 0.38268343236508977172845998403040,
                 r2 = 0.70710678118654752440084436210485;
    const double2 w[8] = {make_double2(1.0, 0.0), make_double2(c1, s1), make_double2(r2, r2), make_double2(s1, c1),
                          make_double2(0.0, 1.0), make_double2(-s1, c1), make_double2(-r2, r2), make_double2(-c1, s1)};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const double2 t = k == 0 ? o[0] : k == 4 ? nu_muli(o[4]) : nu_cmul(o[k], w[k]);
        v[k] = nu_add(e[k], t);
        v[k + 8] = nu_sub(e[k], t);
    }
}
template <int R>
__device__ __forceinline__ void nu_dft(double2* v) {
    if (R == 2) nu_dft2(v);
    else if (R == 4) nu_dft4v(v);
    else if (R == 8) nu_dft8(v);
    else nu_dft16(v);
}

// Twiddles of the in-LDS transforms (length <= 2^lt, lt = min(log2 n, 12)): w^m = e^{2 pi i m / 2^lt} as
// hi[m >> 6] * lo[m & 63], two 64-entry tables in LDS filled by fp64 sincospi at the kernel's start.
struct NuTile {
    double2 hi[64], lo[64];
};
__device__ __forceinline__ void nu_tile_init(NuTile* tw, int lt) {
    const int t = threadIdx.x;
    if (t < 128) {
        const int m = t < 64 ? t : (t - 64) << 6;
        double sv, cv;
        sincospi(ldexp((double)m, 1 - lt), &sv, &cv);  // 2 m / 2^lt
        if (t < 64)
            tw->lo[t] = make_double2(cv, sv);
        else
            tw->hi[t - 64] = make_double2(cv, sv);
    }
}
__device__ __forceinline__ double2 nu_tw_tile(const NuTile* tw, int m) { return nu_cmul(tw->hi[m >> 6], tw->lo[m & 63]); }

// v[r] *= w^r for r = 1 .. R-1: w^r as the product of w, w^2, w^4, w^8 over the bits of r (few live registers,
// product depth <= 3 after the squarings, instead of a chain of R - 2 products)
template <int R>
__device__ __forceinline__ void nu_twiddle(double2 w, double2* v) {
    double2 b[4];
    b[0] = w;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if ((1 << i) < R) b[i] = nu_cmul(b[i - 1], b[i - 1]);
#pragma unroll
    for (int r = 1; r < R; ++r) {
        double2 wr = make_double2(1.0, 0.0);
        bool first = true;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (r & (1 << i)) {
                wr = first ? b[i] : nu_cmul(wr, b[i]);
                first = false;
            }
        v[r] = nu_cmul(v[r], wr);
    }
}

// One Stockham autosort stage of radix R over 2^lc transforms of length 2^ll held in LDS at s[a*sa + cc*sc]:
// butterfly (j, cc) reads x[j + r L/R], twiddles by w_{Ns R}^{(j mod Ns) r}, and writes
// y[(j / Ns) Ns R + (j mod Ns) + r Ns]. 16 / R butterflies per thread (a tile holds <= 16 elements per thread).
template <int R>
__device__ __forceinline__ void nu_stage(double2* s, int ll, int lc, int sa, int sc, int lns, const NuTile* tw,
                                         int lt) {
    constexpr int NB = 16 / R;
    constexpr int LR = R == 2 ? 1 : R == 4 ? 2 : R == 8 ? 3 : 4;
    const int L = 1 << ll, Ns = 1 << lns;
    const int nbt = (L >> LR) << lc;
    double2 v[NB][R];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int b = threadIdx.x + 256 * k;
        if (b < nbt) {
            const int cc = b & ((1 << lc) - 1), j = b >> lc;
#pragma unroll
            for (int r = 0; r < R; ++r) v[k][r] = s[(j + (r << (ll - LR))) * sa + cc * sc];
            if (lns > 0) {
                // w_{Ns R}^{(j mod Ns)} = w_{2^lt}^{(j mod Ns) 2^lt / (Ns R)}
                nu_twiddle<R>(nu_tw_tile(tw, (j & (Ns - 1)) << (lt - lns - LR)), v[k]);
            }
            nu_dft<R>(v[k]);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const int b = threadIdx.x + 256 * k;
        if (b < nbt) {
            const int cc = b & ((1 << lc) - 1), j = b >> lc;
            const int base = ((j >> lns) << (lns + LR)) + (j & (Ns - 1));
#pragma unroll
            for (int r = 0; r < R; ++r) s[(base + r * Ns) * sa + cc * sc] = v[k][r];
        }
    }
    __syncthreads();
}

// 2^lc transforms of length 2^ll in LDS (Stockham: natural order in, natural order out)
__device__ __forceinline__ void nu_fft_lds(double2* s, int ll, int lc, int sa, int sc, const NuTile* tw, int lt) {
    int lns = 0;
    while (lns < ll) {
        const int rem = ll - lns;
        if (rem >= 4) {
            nu_stage<16>(s, ll, lc, sa, sc, lns, tw, lt);
            lns += 4;
        } else if (rem == 3) {
            nu_stage<8>(s, ll, lc, sa, sc, lns, tw, lt);
            lns += 3;
        } else if (rem == 2) {
            nu_stage<4>(s, ll, lc, sa, sc, lns, tw, lt);
            lns += 2;
        } else {
            nu_stage<2>(s, ll, lc, sa, sc, lns, tw, lt);
            lns += 1;
        }
    }
}

// pass 1 of the four-step FFT: view each batch as [n1][n2]; DFT along a of 2^lc consecutive columns b, times
// w_n^{b k1}, stored at y[k1 n2 + b]
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_nu_fft_cols(const double2* __restrict__ X, double2* __restrict__ Y,
                                                     int lnfft, int ln1, int lc, NuTw T, int alo, int acnt) {
    extern __shared__ double2 nu_s[];
    __shared__ NuTile tw;
    const int lt = lnfft < 12 ? lnfft : 12;
    nu_tile_init(&tw, lt);
    const int ln2 = lnfft - ln1, c = 1 << lc, n1 = 1 << ln1;
    const int64_t nfft = int64_t(1) << lnfft;
    const int64_t b0 = (int64_t)blockIdx.x << lc;
    const double2* x = X + (int64_t)blockIdx.y * nfft;
    double2* y = Y + (int64_t)blockIdx.y * nfft;
    for (int e = threadIdx.x; e < (n1 << lc); e += 256) {  // rows a outside [alo, alo + acnt) (mod n1) hold no cell
        const int a = e >> lc, cc = e & (c - 1);
        nu_s[e] = ((a - alo) & (n1 - 1)) < acnt ? x[((int64_t)a << ln2) + b0 + cc] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    nu_fft_lds(nu_s, ln1, lc, c, 1, &tw, lt);
    // times the inter-pass twiddles w_n^{b k1} (n1 c = 4096: 16 outputs per thread)
#pragma unroll
    for (int q = 0; q < kNuTile / 256; ++q) {
        const int e = threadIdx.x + 256 * q;
        if (e < (n1 << lc)) {
            const int k1 = e >> lc, cc = e & (c - 1);
            const int64_t b = b0 + cc;
            y[((int64_t)k1 << ln2) + b] = nu_cmul(nu_s[e], nu_tw(T, b * k1));
        }
    }
}

// k_nu_fft_cols for n1 = 256 (two radix-16 stages over 16 columns): stage 1 on the columns as loaded into registers
// (thread (j, cc): rows j + 16 r of column cc), one LDS exchange, stage 2's outputs (rows k1 = j + 16 r) twiddled and
// stored from registers: one LDS write and read instead of six. Persistent blocks walk the (batch, column block)
// groups with the next group's rows and twiddle bases loaded during the current one (the kernel is latency-bound at
// the two waves per SIMD its 64 KB of LDS allow). The inter-pass twiddle w_n^{b k1} = w_n^{b j} (w_n^{16 b})^r: two
// table values and products over the bits of r (a few ulp, as the tile twiddles).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void k_nu_cols256(
    const double2* __restrict__ X, double2* __restrict__ Y, int lnfft, NuTw T, int alo, int acnt, int64_t ngroups) {
    extern __shared__ double2 nu_s[];  // [256 rows][16 columns]
    __shared__ NuTile tw;
    nu_tile_init(&tw, 12);
    const int ln2 = lnfft - 8;
    const int64_t nfft = int64_t(1) << lnfft;
    const int cc = threadIdx.x & 15, j = threadIdx.x >> 4;
    const int64_t cpb = int64_t(1) << (ln2 - 4);  // column blocks per batch
    // the prefetch keeps the twiddle bases as their two table factors each (loaded before the rows) and multiplies
    // them at use: a product at the fetch would wait for every load issued so far, the rows' included
    double2 nv[16], tf[4];
    auto fetch = [&](int64_t grp) {  // rows outside [alo, alo + acnt) (mod 256) hold no cell
        const int64_t b = ((grp % cpb) << 4) + cc;
        const double2* x = X + (grp / cpb) * nfft + b;
        const int64_t lm = (int64_t(1) << T.lbits) - 1, tb = (b * (int64_t)j) & T.mask, ts = (b << 4) & T.mask;
        tf[0] = T.hi[tb >> T.lbits];
        tf[1] = T.lo[tb & lm];
        tf[2] = T.hi[ts >> T.lbits];
        tf[3] = T.lo[ts & lm];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int a = j + 16 * r;
            nv[r] = ((a - alo) & 255) < acnt ? x[(int64_t)a << ln2] : make_double2(0.0, 0.0);
        }
    };
    int64_t grp = blockIdx.x;
    if (grp < ngroups) fetch(grp);
    __syncthreads();  // tw
    for (; grp < ngroups; grp += gridDim.x) {
        double2 v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = nv[r];
        const double2 wb = nu_cmul(tf[0], tf[1]), ws = nu_cmul(tf[2], tf[3]);  // nu_tw's product
        const int64_t b = ((grp % cpb) << 4) + cc;
        double2* y = Y + (grp / cpb) * nfft + b;
        if (grp + gridDim.x < ngroups) fetch(grp + gridDim.x);
        nu_dft16(v);  // stage 1 (Ns = 1)
#pragma unroll
        for (int r = 0; r < 16; ++r) nu_s[((j << 4) + r) * 16 + cc] = v[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = nu_s[(j + 16 * r) * 16 + cc];
        __syncthreads();  // the next group's stage-1 writes reuse the tile
        nu_twiddle<16>(nu_tw_tile(&tw, j << 4), v);  // w_256^{j r}
        nu_dft16(v);                                 // stage 2 (Ns = 16): output rows k1 = j + 16 r
        v[0] = nu_cmul(v[0], wb);
        nu_twiddle<16>(ws, v);  // v[r] *= (w_n^{16 b})^r
#pragma unroll
        for (int r = 1; r < 16; ++r) v[r] = nu_cmul(v[r], wb);
#pragma unroll
        for (int r = 0; r < 16; ++r) y[(int64_t)(j + 16 * r) << ln2] = v[r];
    }
}

// k_nu_fft_cols for n1 = 512 (n = 2^21): groups of 8 columns (NC = 1: 128 VGPRs, two blocks
// per CU; 16 columns at 248 VGPRs and one block measured 10 % slower), 512 threads (column cc = t & 7, j = t >> 3),
// three radix-8 Stockham stages over rows j + 64 q (8 elements per thread and column: rows as loaded, stage 3's outputs
// k1 = j + 64 q stored from registers), two exchanges through a [512 rows][8 columns] tile (conflict-free without a
// swizzle: 8 consecutive lanes hold 8 consecutive columns). Persistent blocks, the next group's occupied rows loaded
// during the current one; rows by buffer loads and stores (one offset register); the inter-pass twiddle
// w_n^{b k1} = w_n^{b j} (w_n^{64 b})^q as in k_nu_cols256.
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_nu_cols512(
    const double2* __restrict__ X, double2* __restrict__ Y, int lnfft, NuTw T, int alo, int acnt, int64_t ngroups) {
    constexpr int NC = 1, C = 8;
    extern __shared__ double2 nu_s[];  // [512 rows][C columns]
    __shared__ NuTile tw;
    nu_tile_init(&tw, 9);
    const int ln2 = lnfft - 9;
    const int64_t nfft = int64_t(1) << lnfft;
    const int cc = threadIdx.x & 7, j = threadIdx.x >> 3;
    const int64_t cpb = int64_t(1) << (ln2 - 3);  // column groups per batch
    double2 nv[NC][8], tf[NC][4];
    const int voff = ((j << ln2) + cc) * 16;  // row offsets 64 q n2 16 B and column offsets 8 c 16 B: scalar
    auto fetch = [&](int64_t grp) {  // rows outside [alo, alo + acnt) (mod 512) hold no cell
        const int64_t b0 = (grp % cpb) * C;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(X + (grp / cpb) * nfft + b0), (short)0, (int)(16 << lnfft), 0x00020000);
        const int64_t lm = (int64_t(1) << T.lbits) - 1;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int64_t b = b0 + cc + 8 * c, tb = (b * (int64_t)j) & T.mask, ts = (b << 6) & T.mask;
            tf[c][0] = T.hi[tb >> T.lbits];
            tf[c][1] = T.lo[tb & lm];
            tf[c][2] = T.hi[ts >> T.lbits];
            tf[c][3] = T.lo[ts & lm];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const bool occ = ((j + 64 * q - alo) & 511) < acnt;
#pragma unroll
            for (int c = 0; c < NC; ++c)
                nv[c][q] = occ ? __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(
                                                                 rs, voff, ((64 * q << ln2) + 8 * c) * 16, 0))
                               : make_double2(0.0, 0.0);
        }
    };
    int64_t grp = blockIdx.x;
    if (grp < ngroups) fetch(grp);
    const int m2 = (j & 7) << 3;  // stage-2 twiddle w_64^{(j & 7) q} in units of w_512; stage 3: w_512^{j q}
    const int z2 = ((j >> 3) << 6) + (j & 7);
    __syncthreads();  // tw
    typedef unsigned int nu_u4 __attribute__((ext_vector_type(4)));
    for (; grp < ngroups; grp += gridDim.x) {
        double2 v[NC][8], wb[NC], ws[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[c][q] = nv[c][q];
            wb[c] = nu_cmul(tf[c][0], tf[c][1]);
            ws[c] = nu_cmul(tf[c][2], tf[c][3]);
        }
        const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(Y + (grp / cpb) * nfft + (grp % cpb) * C), (short)0, (int)(16 << lnfft), 0x00020000);
        if (grp + gridDim.x < ngroups) fetch(grp + gridDim.x);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            nu_dft8(v[c]);  // stage 1 (Ns = 1): row 8 j + q
#pragma unroll
            for (int q = 0; q < 8; ++q) nu_s[((j << 3) + q) * C + cc + 8 * c] = v[c][q];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[c][q] = nu_s[(j + 64 * q) * C + cc + 8 * c];
        }
        __syncthreads();  // the stage-2 writes reuse the tile
        const double2 t2 = nu_tw_tile(&tw, m2);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            nu_twiddle<8>(t2, v[c]);
            nu_dft8(v[c]);  // stage 2 (Ns = 8): row z2 + 8 q
#pragma unroll
            for (int q = 0; q < 8; ++q) nu_s[(z2 + 8 * q) * C + cc + 8 * c] = v[c][q];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[c][q] = nu_s[(j + 64 * q) * C + cc + 8 * c];
        }
        __syncthreads();  // the next group's stage-1 writes reuse the tile
        const double2 t3 = nu_tw_tile(&tw, j);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            nu_twiddle<8>(t3, v[c]);
            nu_dft8(v[c]);  // stage 3 (Ns = 64): output row k1 = j + 64 q
            v[c][0] = nu_cmul(v[c][0], wb[c]);
            nu_twiddle<8>(ws[c], v[c]);  // v[q] *= (w_n^{64 b})^q
#pragma unroll
            for (int q = 1; q < 8; ++q) v[c][q] = nu_cmul(v[c][q], wb[c]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(nu_u4, v[c][q]), ry, voff,
                                                       ((64 * q << ln2) + 8 * c) * 16, 0);
        }
    }
}

// Pass 2 of the FFT (or the only pass) with the moments' sum: block (k1, r) transforms row k1 (length 2^ll = n2) of
// every moment p of trial-grid row r, from p = P-1 down to 0, and keeps the Bessel-weighted sum
// A = sum_p eps_p i^p J_p(z) B_p (nu_bes; z = pi jc / n) of its 2^ll positions in registers, so the moments' transforms
// are read once and never written back; the trials' (C_k, S_k) go to CS[t], t the trial's index in the batch.
// X[beta][pos], beta = p * nrow + r, pos = k1 n2 + k2 holds J = k1 + n1 k2 (ln1 = 0: natural order), J = jc mod n.
constexpr int kNuFusedPer = kNuTile / 256;  // positions per thread
// The row k1 of block b of a row pass over n1 rows (xcd: NuHooks::row_map). A block's trials are k1 + n1 pos: the 8 or
// 16 trials of one cache line of CS, CS0 or out belong to as many consecutive k1, and consecutive blocks are dealt
// round-robin over the 8 XCDs, each with an L2 of its own -- every epilogue access would be a lone piece of a line
// whose other pieces seven other L2s hold. With n1 a multiple of 8, blocks b = x (mod 8) take the contiguous rows
// x n1/8 .. (x + 1) n1/8 - 1, so that a line's trials meet in one L2 (n1 = 8: the identity; rows move from n1 = 16 on).
// A bijection of the rows whatever the placement: b mod 8 is a label chosen for speed, and no result depends on where
// or when a block runs.
__device__ __forceinline__ unsigned nu_row_of_block(unsigned b, unsigned n1, int xcd) {
    return xcd && (n1 & 7u) == 0 ? (b & 7u) * (n1 >> 3) + (b >> 3) : b;
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1))) void k_nu_fft_rows_combine(const double2* __restrict__ X, int ll, int lnfft, int P,
                                                             int nrow, int64_t nf, int64_t jhi, int64_t h,
                                                             int64_t tbase, int64_t nbt, const double* __restrict__ bc,
                                                             double2* __restrict__ CS, int xcd) {
    extern __shared__ double2 nu_s[];
    __shared__ NuTile tw;
    const int lt = lnfft < 12 ? lnfft : 12;
    nu_tile_init(&tw, lt);
    const int64_t nfft = int64_t(1) << lnfft;
    const int L = 1 << ll, ln1 = lnfft - ll;
    const int64_t k1 = nu_row_of_block(blockIdx.x, 1u << ln1, xcd);
    const int r = blockIdx.y;
    double2 acc[kNuFusedPer], nx[kNuFusedPer];
    NuBes bs[kNuFusedPer];
    const double2* xr = X + (int64_t)r * nfft + (k1 << ll);  // moment p's row at xr + p nrow nfft
    const int64_t pstride = (int64_t)nrow * nfft;
#pragma unroll
    for (int q = 0; q < kNuFusedPer; ++q) {
        acc[q] = make_double2(0.0, 0.0);
        const int e = threadIdx.x + 256 * q;
        const int64_t J = k1 + ((int64_t)e << ln1);
        bs[q] = nu_bes_start(bc, P, nu_zh(J <= jhi ? J : J - nfft, lnfft));
        nx[q] = e < L ? xr[(int64_t)(P - 1) * pstride + e] : make_double2(0.0, 0.0);
    }
    for (int p = P - 1; p >= 0; --p) {
        // this moment's row into the tile, the next one's loads issued before the transform
        const int64_t pn = (int64_t)(p > 0 ? p - 1 : 0) * pstride;
#pragma unroll
        for (int q = 0; q < kNuFusedPer; ++q) {
            const int e = threadIdx.x + 256 * q;
            if (e < L) {
                nu_s[e] = nx[q];
                nx[q] = xr[pn + e];
            }
        }
        __syncthreads();
        nu_fft_lds(nu_s, ll, 0, 1, L, &tw, lt);
#pragma unroll
        for (int q = 0; q < kNuFusedPer; ++q) {
            const int b = threadIdx.x + 256 * q;
            if (b < L) {
                const double2 v = nu_s[b];
                const int64_t J = k1 + ((int64_t)b << ln1);
                const int64_t jc = J <= jhi ? J : J - nfft;  // positions between the two ends hold no trial
                // eps_p i^p J_p(z), z/2 = (pi/2) jc / n (nu_bes_w)
                acc[q] = nu_bes_acc(acc[q], nu_bes_w(bs[q], p, nu_zh(jc, lnfft)), v, p);
            }
        }
        __syncthreads();  // the next moment's store overwrites the tile
    }
#pragma unroll
    for (int q = 0; q < kNuFusedPer; ++q) {
        const int b = threadIdx.x + 256 * q;
        if (b >= L) continue;
        const int64_t J = k1 + ((int64_t)b << ln1);
        int64_t jc;
        if (J <= jhi)
            jc = J;
        else if (J >= nfft - h)
            jc = J - nfft;
        else
            continue;
        const int64_t t = tbase + r * nf + jc;  // (row0 + r) nf + jbase + jc - tb0
        if (t >= 0 && t < nbt) CS[t] = acc[q];
    }
}

// The radix-8 row passes (k_nu_rows_combine8<11>: rows of 2048; k_nu_rows_iw: rows of 4096): k_nu_fft_rows_combine's
// sum with 8 elements per thread, so that two waves per SIMD run. Stage 1 on the row as loaded, the last stage's outputs
// in registers for the moment sum, the stages between through two LDS tiles whose roles alternate between moments. The
// transform's arithmetic differs from nu_fft_lds's radix-16 stages in rounding only. Measured on rows of 4096
// (profiles/r06/ab_p2_probes.log, config 3): without its loads the pass takes 0.90
// of its time, without its LDS exchanges 0.85, without the transform's arithmetic 0.81, without both 0.69 -- the
// loads, exchanges and arithmetic of one block per CU overlap little; 30 % fewer VALU instructions (below) or a second
// moment's loads in flight moved it by 1-2 %, rows of 2048 with two blocks per CU by 9 % (pass 1 then needs 512-row
// columns), an L2 touch of the rows two moments ahead cost 12 % (profiles/r06/ab_p2_l2prefetch_rejected.log).
// Measured, rejected and removed: a 256-thread radix-16 form with 16 elements per thread, one wave per SIMD (0.190 vs
// 0.178 ms per config-3 search, profiles/r05/ab_r8_ilp.log); the moments in chunks, pass 1 and pass 2 of a chunk in
// turn with the partial sums carried through CS (slower at every chunk size, profiles/r06/ab_pchunk.log); n = 2^20 as
// 512 x 2048 (pass 2 0.160 vs 0.180 ms, pass 1 0.138 vs 0.115 ms per config-3 search: a wash,
// profiles/r06/ab_rows2048_cols512.log); pass 2 and the moment sum as two kernels.
// Arguments plo and accum are what is left of the moment chunks: a launch transforms moments plo .. P-1 (X holds their
// planes only, beta = (p - plo) nrow + r) and, with accum, starts from the sum CS holds instead of zero. The host
// always passes 0, 0. They stay because the register allocation hangs on them: with both folded away (accumulator
// from zero, unconditional prefetch of the next row, no rotation at the end) the compiler gives k_nu_rows_iw 256 VGPRs
// and spills 17 (with them: 252, none) and k_nu_rows_combine8<11> 236 (221).
// The last harmonic's launch may finalize (NuFinal.on): its sums stay in registers and each trial's power and
// certificate are formed there from the earlier harmonics' CS (nu_power), the fix-up list appended, and the block's
// best trial (np.argmax semantics) written to best_part for k_best_final -- no CS write, no finalize launch, no
// reduction pass over the powers.
struct NuFinal {
    int on, m, stat, Pc;           // Pc: the plan's moments P (the certificate's truncation bound)
    double nph, invfact, rel;
    int64_t tb0;                   // out index of the batch's trial 0
    double* out;
    int* nflag;
    int64_t* flagged;
    BestCand* best_part;           // per-block best (nullable)
    int64_t best_base;
    const double2* CS0;            // harmonic 0's sums of the batch (stride nbt)
};
// The row pass's epilogue: each position's sum to CS (F.on == 0), or (fused finalize, k_nu_finalize's arithmetic
// with the last harmonic from registers) each trial's power, the fix-up list and the block's best trial. Position
// q of thread t is t + TPB q of the row.
template <int TPB, int NP>
__device__ __forceinline__ void nu_rows_epilogue(const double2 (&acc)[NP], int64_t k1, int ln1, int64_t nfft,
                                                 int64_t jhi, int64_t h, int64_t tbase, int r, int64_t nf, int64_t nbt,
                                                 double2* __restrict__ CS, const NuFinal& F, double2* lds,
                                                 int pos0 = -1) {
    const int t = threadIdx.x;
    const int b0 = pos0 < 0 ? t : pos0;  // the thread's first row position (then + TPB q)
    if (!F.on) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            const int64_t J = k1 + ((int64_t)(b0 + TPB * q) << ln1);
            int64_t jc;
            if (J <= jhi)
                jc = J;
            else if (J >= nfft - h)
                jc = J - nfft;
            else
                continue;
            const int64_t tt = tbase + r * nf + jc;
            if (tt >= 0 && tt < nbt) CS[tt] = acc[q];
        }
        return;
    }
    BestCand bc_ = {-INFINITY, INT64_MAX};
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        const int64_t J = k1 + ((int64_t)(b0 + TPB * q) << ln1);
        int64_t jc;
        if (J <= jhi)
            jc = J;
        else if (J >= nfft - h)
            jc = J - nfft;
        else
            continue;
        const int64_t tt = tbase + r * nf + jc;
        if (tt < 0 || tt >= nbt) continue;
        double p, err;
        nu_power(F.CS0, nbt, tt, F.m, F.stat, F.nph, nu_err_bound(jc, nfft, F.Pc, F.invfact, F.nph), true, acc[q], &p,
                 &err);
        F.out[F.tb0 + tt] = p;
        if (!(err <= F.rel * fabs(p))) F.flagged[atomicAdd(F.nflag, 1)] = F.tb0 + tt;
        if (best_better(p, F.tb0 + tt, bc_.v, bc_.i)) bc_ = {p, F.tb0 + tt};
    }
    if (!F.best_part) return;
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(bc_.v, o);
        const int64_t i = __shfl_xor(bc_.i, o);
        if (best_better(v, i, bc_.v, bc_.i)) bc_ = {v, i};
    }
    __syncthreads();  // the tiles are free: the wave candidates go to LDS
    BestCand* red = reinterpret_cast<BestCand*>(lds);
    if ((t & 63) == 0) red[t >> 6] = bc_;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < TPB / 64; ++w)
            if (best_better(red[w].v, red[w].i, bc_.v, bc_.i)) bc_ = red[w];
        F.best_part[F.best_base + (int64_t)blockIdx.y * gridDim.x + blockIdx.x] = bc_;
    }
}

// The moment sum is carried in a rotating frame: S_p = sum_{p' >= p} eps_p' i^p' J_p'(z) v_p' as T_p = i^-p S_p,
// T_p = i T_p+1 + w_p v_p -- the product by i an exact swap and negation folded into the two fmas, no per-moment
// select of i^p -- and the Bessel recurrence as 2 J (exact), so w_p = 2 J_p is the state itself (p > 0). Every rounding
// is that of nu_bes_w / nu_bes_acc, so the sums are those of the direct form bit for bit, in ~30 % fewer VALU
// instructions. Two moments per loop iteration: the register arrays alternate between the moment in use and the next
// one's loads, the tiles between their roles (no copies). Rows by buffer loads (one offset register, the element
// offsets in a scalar register); tile element i at i + i / 8, so that every stage's element offsets are compile-time
// constants and its accesses a base plus immediates: 221 VGPRs, no spills (the xor swizzle's per-lane store addresses
// took 256 and spilled). Stride-8 stores stay conflict-free; some reads of a 16-lane group meet 2-way.
struct NuRot {
    double j1, j2, iz2;  // 2 J_p+1, 2 J_p+2 (the next moment's), 2 / z
};
// dynamic LDS of k_nu_rows_combine8<LN2>: two padded tiles
constexpr size_t nu_rows_lds(int ln2) { return 2 * ((size_t(1) << ln2) + (size_t(1) << (ln2 - 3))) * sizeof(double2); }
// LN2 = 11, the one instantiation: rows of 2048 (n = 2048, a single pass), 256 threads, one radix-4 stage (butterflies
// t and t + 1024 on v[0, 2, 4, 6] and v[1, 3, 5, 7]) then three radix-8 (Ns = 4, 32, 256), three block-wide exchanges
// per moment. Rows of 4096 take k_nu_rows_iw; this kernel's 512-thread form for them (four radix-8 stages) was
// measured slower (0.180 vs 0.171 ms per config-3 search, profiles/r06/ab_p2_iw.log) and removed.
template <int LN2>
__global__ __launch_bounds__(1 << (LN2 - 3)) __attribute__((amdgpu_waves_per_eu(2))) void k_nu_rows_combine8(
    const double2* X, int lnfft, int P, int plo, int accum, int nrow, int64_t nf, int64_t jhi, int64_t h,
    int64_t tbase, int64_t nbt, const double* __restrict__ bc, double2* __restrict__ CS, const NuFinal F) {
    constexpr int N = 1 << LN2, TPB = N / 8, NT = N + N / 8;
    constexpr int Ns2 = 4, Ns3 = 8 * Ns2;
    static_assert(LN2 == 11, "rows of 2048");
    extern __shared__ double2 nu_s[];  // [2][NT]
    __shared__ NuTile tw;
    nu_tile_init(&tw, LN2);
    const int64_t nfft = int64_t(1) << lnfft;
    const int ln1 = lnfft - LN2;
    const int64_t k1 = blockIdx.x;
    const int r = blockIdx.y;
    const int t = threadIdx.x;
    const double2* xr = X + (int64_t)r * nfft + (k1 << LN2);
    const int64_t pstride = (int64_t)nrow * nfft;
    auto load_row = [&](int pm, double2 (&dst)[8]) {  // moment pm's row: elements t + TPB q
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void*)(xr + (int64_t)pm * pstride), (short)0, N * 16, 0x00020000);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            dst[q] = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rs, t * 16, TPB * 16 * q, 0));
    };
    double2 acc[8], xa[8], xb[8];
    NuRot bs[8];
    // the frame at the top moment: T_P = i^-P S_P (S_P: the sum CS already holds at this position's trial, else 0)
    const int rP = P & 3;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        double2 a0 = make_double2(0.0, 0.0);
        const int64_t J = k1 + ((int64_t)(t + TPB * q) << ln1);
        const int64_t jc = J <= jhi ? J : J - nfft;
        if (accum) {
            const int64_t tt = tbase + r * nf + jc;
            if ((J <= jhi || J >= nfft - h) && tt >= 0 && tt < nbt) a0 = CS[tt];
        }
        acc[q] = rP == 0 ? a0 : rP == 1 ? make_double2(a0.y, -a0.x) : rP == 2 ? make_double2(-a0.x, -a0.y)
                                                                        : make_double2(-a0.y, a0.x);
        const NuBes b0 = nu_bes_start(bc, P, nu_zh(jc, lnfft));
        bs[q] = {2.0 * b0.j1, 2.0 * b0.j2, b0.iz2};
    }
    load_row(P - 1 - plo, xa);
    // stage twiddles in units of w_N (stage 4: w_N^{t q})
    const int m2 = (t & (Ns2 - 1)) * (N / (8 * Ns2)), m3 = (t & (Ns3 - 1)) * (N / (8 * Ns3)), m4 = t;
    const int z2 = (t / Ns2) * 8 * Ns2 + (t & (Ns2 - 1)), z3 = (t / Ns3) * 8 * Ns3 + (t & (Ns3 - 1));  // outputs
    // padded bases: element e = base + offset lands at e + e / 8 = (base + base / 8) + (offset + offset / 8 (+1 where
    // the stage-2 offset 4 q carries into the base's bit 3)) -- compile-time offsets
    const int w1 = 4 * t + (t >> 1), w2 = z2 + (z2 >> 3), w3 = z3 + (z3 >> 3), rd = t + (t >> 3);
    __syncthreads();  // tw
    // one moment: v (its row) through the four stages, moment p - 1's loads into nv, then the sum
    auto moment = [&](auto LAST, int p, double2 (&v)[8], double2 (&nv)[8], double2* A, double2* B) {
        constexpr bool last = decltype(LAST)::value;  // p == 0: w_0 = J_0 (1 where z = 0)
        if (p > plo) load_row(p - 1 - plo, nv);
        nu_dft4(v[0], v[2], v[4], v[6]);  // stage 1 (R 4, Ns = 1): elements 4 t + q and 4 t + 1024 + q
        nu_dft4(v[1], v[3], v[5], v[7]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            A[w1 + q] = v[2 * q];
            A[w1 + N / 2 + N / 16 + q] = v[2 * q + 1];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = A[rd + TPB * 9 / 8 * q];
        nu_twiddle<8>(nu_tw_tile(&tw, m2), v);
        nu_dft8(v);  // stage 2: element z2 + Ns2 q
#pragma unroll
        for (int q = 0; q < 8; ++q) B[w2 + Ns2 * q + (q >> 1)] = v[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = B[rd + TPB * 9 / 8 * q];
        nu_twiddle<8>(nu_tw_tile(&tw, m3), v);
        nu_dft8(v);  // stage 3: element z3 + Ns3 q
#pragma unroll
        for (int q = 0; q < 8; ++q) A[w3 + Ns3 * 9 / 8 * q] = v[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = A[rd + TPB * 9 / 8 * q];
        nu_twiddle<8>(nu_tw_tile(&tw, m4), v);
        nu_dft8(v);  // stage 4: output position t + TPB q
        const double pp1 = (double)(p + 1);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double j = fma(pp1 * bs[q].iz2, bs[q].j1, -bs[q].j2);  // 2 J_p
            bs[q].j2 = bs[q].j1;
            bs[q].j1 = j;
            double w = j;
            // w_0 = J_0, and 1 at z = 0: trial offset jc = J = 0, position 0 of row 0
            if constexpr (last) w = (q == 0 && k1 == 0 && t == 0) ? 1.0 : 0.5 * j;
            acc[q] = make_double2(fma(w, v[q].x, -acc[q].y), fma(w, v[q].y, acc[q].x));  // i T + w v
        }
    };
    // moments P-1 .. max(plo, 1) two per iteration (the first alone when their count is odd), then moment 0
    const int pend = plo > 0 ? plo : 1;
    int p = P - 1;
    double2* TA = nu_s;
    double2* TB = nu_s + NT;
    if (p >= pend && ((p - pend + 1) & 1)) {
        moment(std::false_type(), p, xa, xb, TA, TB);
        --p;
#pragma unroll
        for (int q = 0; q < 8; ++q) xa[q] = xb[q];
        double2* tt = TA;
        TA = TB;
        TB = tt;
    }
    for (; p >= pend; p -= 2) {
        moment(std::false_type(), p, xa, xb, TA, TB);
        moment(std::false_type(), p - 1, xb, xa, TB, TA);
    }
    if (plo == 0) moment(std::true_type(), 0, xa, xb, TA, TB);
    // back to S = i^plo T
    const int rl = plo & 3;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const double2 a = acc[q];
        acc[q] = rl == 0 ? a : rl == 1 ? make_double2(-a.y, a.x) : rl == 2 ? make_double2(-a.x, -a.y)
                                                                : make_double2(a.y, -a.x);
    }
    nu_rows_epilogue<TPB, 8>(acc, k1, ln1, nfft, jhi, h, tbase, r, nf, nbt, CS, F, nu_s);
}

// The 4096-element row pass with one cross-wave exchange per moment. Radix-8 decimation in frequency over the input
// digits n = 512 n3 + 64 n2 + 8 n1 + n0 (outputs k0 + 8 k1 + 64 k2 + 512 k3): stage 1 (over n3, the row as loaded:
// thread t = m = 64 n2 + 8 n1 + n0) then w_4096^(m k0); one exchange through a 64 KB tile to thread (wave k0, lane
// m' = 8 n1 + n0), whose wave reads the tile's 8 KB region k0 only; stage 2 (over n2) then w_512^(m' k1); an exchange
// inside the wave (lane 8 k1 + n0) through its own region of the tile, which no other wave reads; stage 3 (over n1)
// then w_64^(n0 k2); a second exchange inside the wave (lane 8 k1 + k2); stage 4 (over n0): outputs k3 at positions
// k0 + 8 k1 + 64 k2 + 512 k3. Two tiles alternate between moments, so one barrier per moment (the cross-wave exchange)
// suffices: a tile is written again two moments later, after every wave has passed the next moment's barrier and with
// it left the tile. Every exchange conflict-free (linear or lane-xor layouts); the wave-level exchanges wait only for
// their own stores. Moment sum as k_nu_rows_combine8 (rotating frame, doubled Bessel state, two moments per iteration).
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2))) void k_nu_rows_iw(
    const double2* X, int lnfft, int P, int plo, int accum, int nrow, int64_t nf, int64_t jhi, int64_t h,
    int64_t tbase, int64_t nbt, const double* __restrict__ bc, double2* __restrict__ CS, const NuFinal F, int xcd) {
    constexpr int N = 4096, TPB = 512;
    extern __shared__ double2 nu_s[];  // [2][4096]
    __shared__ NuTile tw;
    nu_tile_init(&tw, 12);
    const int64_t nfft = int64_t(1) << lnfft;
    const int ln1 = lnfft - 12;
    const int64_t k1b = nu_row_of_block(blockIdx.x, 1u << ln1, xcd);
    const int r = blockIdx.y;
    const int t = threadIdx.x, w = t >> 6, L = t & 63, hi3 = L >> 3, lo3 = L & 7;
    const int pos0 = w + 8 * hi3 + 64 * lo3;  // output positions pos0 + 512 q
    const double2* xr = X + (int64_t)r * nfft + (k1b << 12);
    const int64_t pstride = (int64_t)nrow * nfft;
    auto load_row = [&](int pm, double2 (&dst)[8]) {  // moment pm's row: elements t + 512 q
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc((void*)(xr + (int64_t)pm * pstride), (short)0, N * 16, 0x00020000);
#pragma unroll
        for (int q = 0; q < 8; ++q)
            dst[q] = __builtin_bit_cast(double2, __builtin_amdgcn_raw_buffer_load_b128(rs, t * 16, TPB * 16 * q, 0));
    };
    double2 acc[8], xa[8], xb[8];
    NuRot bs[8];
    const int rP = P & 3;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        double2 a0 = make_double2(0.0, 0.0);
        const int64_t J = k1b + ((int64_t)(pos0 + TPB * q) << ln1);
        const int64_t jc = J <= jhi ? J : J - nfft;
        if (accum) {
            const int64_t tt = tbase + r * nf + jc;
            if ((J <= jhi || J >= nfft - h) && tt >= 0 && tt < nbt) a0 = CS[tt];
        }
        acc[q] = rP == 0 ? a0 : rP == 1 ? make_double2(a0.y, -a0.x) : rP == 2 ? make_double2(-a0.x, -a0.y)
                                                                        : make_double2(-a0.y, a0.x);
        const NuBes b0 = nu_bes_start(bc, P, nu_zh(jc, lnfft));
        bs[q] = {2.0 * b0.j1, 2.0 * b0.j2, b0.iz2};
    }
    load_row(P - 1 - plo, xa);
    // tile offsets: cross-wave store (q 512 + n2 64 + m'), its read (k0 512 + n2 64 + m'), wave-level exchange 1 store
    // (64 n1 + 8 k1 + n0) / read (64 n1 + 8 k1 + n0, n1 = q), exchange 2 store (64 k2 + 8 k1 + (n0 ^ k2)) / read
    const int cw = 64 * w + L, cr = 512 * w + L, e1w = 512 * w + 64 * hi3 + lo3, e2w = 512 * w + 8 * hi3,
              e2r = 512 * w + 64 * lo3 + 8 * hi3;
    __syncthreads();  // tw
    auto moment = [&](auto LAST, int p, double2 (&v)[8], double2 (&nv)[8], double2* A) {
        constexpr bool last = decltype(LAST)::value;
        if (p > plo) load_row(p - 1 - plo, nv);
        nu_dft8(v);  // stage 1 (over n3): k0 = q
        nu_twiddle<8>(nu_tw_tile(&tw, t), v);
#pragma unroll
        for (int q = 0; q < 8; ++q) A[cw + 512 * q] = v[q];
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = A[cr + 64 * q];
        nu_dft8(v);  // stage 2 (over n2): k1 = q
        nu_twiddle<8>(nu_tw_tile(&tw, 8 * L), v);
#pragma unroll
        for (int q = 0; q < 8; ++q) A[e1w + 8 * q] = v[q];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own stores, before its lanes read them
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = A[cr + 64 * q];
        nu_dft8(v);  // stage 3 (over n1): k2 = q
        nu_twiddle<8>(nu_tw_tile(&tw, 64 * lo3), v);
#pragma unroll
        for (int q = 0; q < 8; ++q) A[e2w + 64 * q + (lo3 ^ q)] = v[q];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = A[e2r + (q ^ lo3)];
        nu_dft8(v);  // stage 4 (over n0): k3 = q, position pos0 + 512 q
        const double pp1 = (double)(p + 1);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const double j = fma(pp1 * bs[q].iz2, bs[q].j1, -bs[q].j2);  // 2 J_p
            bs[q].j2 = bs[q].j1;
            bs[q].j1 = j;
            double wgt = j;
            // w_0 = J_0, and 1 at z = 0: position 0 of row 0 (pos0 = 0: thread 0)
            if constexpr (last) wgt = (q == 0 && k1b == 0 && pos0 == 0) ? 1.0 : 0.5 * j;
            acc[q] = make_double2(fma(wgt, v[q].x, -acc[q].y), fma(wgt, v[q].y, acc[q].x));
        }
    };
    const int pend = plo > 0 ? plo : 1;
    int p = P - 1;
    double2* TA = nu_s;
    double2* TB = nu_s + N;
    if (p >= pend && ((p - pend + 1) & 1)) {
        moment(std::false_type(), p, xa, xb, TA);
        --p;
#pragma unroll
        for (int q = 0; q < 8; ++q) xa[q] = xb[q];
        double2* tt = TA;
        TA = TB;
        TB = tt;
    }
    for (; p >= pend; p -= 2) {
        moment(std::false_type(), p, xa, xb, TA);
        moment(std::false_type(), p - 1, xb, xa, TB);
    }
    if (plo == 0) moment(std::true_type(), 0, xa, xb, TA);
    const int rl = plo & 3;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const double2 a = acc[q];
        acc[q] = rl == 0 ? a : rl == 1 ? make_double2(-a.y, a.x) : rl == 2 ? make_double2(-a.x, -a.y)
                                                                : make_double2(a.y, -a.x);
    }
    nu_rows_epilogue<TPB, 8>(acc, k1b, ln1, nfft, jhi, h, tbase, r, nf, nbt, CS, F, nu_s, pos0);
}

// Z^2 / H of trials tb0 .. tb0+nbt-1 (flat, relative to the call's first) from CS[k][t], in the reference's formula
// order, with the certificate: |A_k error| <= E = N (2.4 (x/2)^P / P! + kNuRho), x = pi |jc| / n (invfact =
// 2.4 / (2^P P!), nu_trunc), so Z2_k = (2/N)|A_k|^2
// errs by <= (2/N)(2 |A_k| E + E^2); Z^2 sums them, H = max_k g_k takes the largest bound among the g_k that the
// errors could lift to the maximum (as k_search_finalize_exact). A trial whose bound exceeds rel |power| goes to the
// fp64 fix-up list.
__global__ __launch_bounds__(256) void k_nu_finalize(const double2* __restrict__ CS, int64_t nbt, int m, int stat,
                                                     double nph, int64_t nf, int64_t jbase, int64_t nfft, int P,
                                                     double invfact, double rel, int64_t tb0, int64_t first,
                                                     double* __restrict__ out, int* __restrict__ nflag,
                                                     int64_t* __restrict__ flagged) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nbt) return;
    const int64_t flat = tb0 + t + first;
    const int64_t jc = flat % nf - jbase;
    double p, err;
    nu_power(CS, nbt, t, m, stat, nph, nu_err_bound(jc, nfft, P, invfact, nph), false, make_double2(0.0, 0.0), &p,
             &err);
    out[tb0 + t] = p;
    if (!(err <= rel * fabs(p))) flagged[atomicAdd(nflag, 1)] = tb0 + t;
}

// ---- host ----
static int g_last_search_path = 0;  // crimp_last_search_path(): 0 fp64 direct, 1 exact, 2 nufft
static int64_t g_last_nufft_n = 0;   // crimp_last_nufft_plan(): the last NUFFT's largest FFT length, its moments,
static int g_last_nufft_p = 0;       // and its spread form (1 cell gather, 0 MFMA slots)
static int g_last_nufft_gather = 0;
// crimp_last_nufft_work(): the last NUFFT's algorithmic work (NuSearchPlan::work)
static double g_nu_work[kNuCls] = {0, 0, 0, 0, 0, 0, 0};
// crimp_last_nufft_cells(): start tables (one per row group and harmonic) the last NUFFT search built / reused
static int64_t g_last_cells_built = 0, g_last_cells_reused = 0;

// Twiddle (w_n, two-level), cis and Bessel-series tables for n = 2^lnfft, built once per device and n (long double on
// the host) and kept for the process: a search reuses them without an upload.
struct NuTables {
    NuTw T{};
    const double2* cis = nullptr;   // 1024 points per turn (k_nu_spread)
    const double2* cis2 = nullptr;  // 2048 points per turn (k_nu_gather)
    const double* bc = nullptr;     // nu_bes_series coefficients
};
static int nu_tables(hipStream_t s, int lnfft, NuTables* out) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, double2*> cache;
    const int lbits = std::min(lnfft, 11);
    const int64_t nlo = int64_t(1) << lbits, nhi = int64_t(1) << (lnfft - lbits);
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    double2* d = nullptr;
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = cache.find({dev, lnfft});
        if (it != cache.end()) {
            d = it->second;
        } else {
            std::vector<double2> h((size_t)(nlo + nhi + 1024 + kNuBesP * kNuBesM / 2 + 2048));
            const long double tp = 6.283185307179586476925286766559L;
            const long double nf = (long double)(int64_t(1) << lnfft);
            for (int64_t i = 0; i < nlo; ++i) {
                const long double a = tp * (long double)i / nf;
                h[(size_t)i] = make_double2((double)cosl(a), (double)sinl(a));
            }
            for (int64_t i = 0; i < nhi; ++i) {
                const long double a = tp * (long double)(i << lbits) / nf;
                h[(size_t)(nlo + i)] = make_double2((double)cosl(a), (double)sinl(a));
            }
            for (int i = 0; i < 1024; ++i) {
                const long double a = tp * (long double)i / 1024.0L;
                h[(size_t)(nlo + nhi + i)] = make_double2((double)cosl(a), (double)sinl(a));
            }
            // nu_bes_series coefficients 1 / (m! (m+p)!), [p][m]
            double* bco = reinterpret_cast<double*>(h.data() + nlo + nhi + 1024);
            for (int p = 0; p < kNuBesP; ++p)
                for (int m = 0; m < kNuBesM; ++m) {
                    long double f = 1.0L;
                    for (int q = 2; q <= m; ++q) f *= (long double)q;
                    for (int q = 2; q <= m + p; ++q) f *= (long double)q;
                    bco[p * kNuBesM + m] = (double)(1.0L / f);
                }
            for (int i = 0; i < 2048; ++i) {  // nu_cis2
                const long double a = tp * (long double)i / 2048.0L;
                h[(size_t)(nlo + nhi + 1024 + kNuBesP * kNuBesM / 2 + i)] = make_double2((double)cosl(a), (double)sinl(a));
            }
            HIPCHK(hipMalloc(&d, h.size() * sizeof(double2)));
            HIPCHK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(double2), hipMemcpyHostToDevice, s));
            HIPCHK(hipStreamSynchronize(s));  // h is pageable and local
            cache[{dev, lnfft}] = d;
        }
    }
    out->T.lo = d;
    out->T.hi = d + nlo;
    out->T.lbits = lbits;
    out->T.mask = (int64_t(1) << lnfft) - 1;
    out->cis = d + nlo + nhi;
    out->bc = reinterpret_cast<const double*>(d + nlo + nhi + 1024);
    out->cis2 = d + nlo + nhi + 1024 + kNuBesP * kNuBesM / 2;
    return CRIMP_OK;
}

template <bool TWOD>
static void nu_launch_spread(int G, dim3 grid, hipStream_t s, const double* tt, double t0, int64_t n, int64_t nchunk,
                             double s1,
                             double fch, double fcl, const double* c2, int nrow, int k0, int P, const NuPass* ps,
                             const double2* tab, double* U, int64_t* ctab, const int* bad) {
#define CRIMP_NS(GG) \
    k_nu_spread<GG, TWOD><<<grid, 256, 0, s>>>(tt, t0, n, nchunk, s1, fch, fcl, c2, nrow, k0, P, ps, tab, U, ctab, bad)
    if (G == 10) CRIMP_NS(10); else if (G == 8) CRIMP_NS(8); else if (G == 6) CRIMP_NS(6); else if (G == 4) CRIMP_NS(4);
    else CRIMP_NS(2);
#undef CRIMP_NS
}

template <int R, bool TWOD, bool CHECK>
static void launch_gather_r(int64_t blocks, const double* tt, double t0, const int64_t* start, int64_t nfft, double s1,
                            double fch, double fcl, const double* c2, int nrow, int P, const NuGatherSet& S,
                            int* bad, const double2* tab, double2* W, const NuFold& F, hipStream_t s) {
    const dim3 grid((unsigned)(blocks + (CHECK ? F.ncheck : 0)));
#define NU_GATHER(PPP)                                                                                               \
    k_nu_gather<R, TWOD, PPP, CHECK><<<grid, 256, 0, s>>>(tt, t0, start, nfft, s1, fch, fcl, c2, nrow, P, S, bad, tab, \
                                                          W, F)
    if (P <= 14) {  // Z^2_m (m >= 2) at config-3-like grids (kNuEpsZm)
        NU_GATHER(14);
    } else if (P <= 15) {
        NU_GATHER(15);
    } else if (P <= 16) {
        NU_GATHER(16);
    } else if (P <= 20) {
        NU_GATHER(20);
    } else {
        NU_GATHER(kNuGatherMaxP);
    }
#undef NU_GATHER
}
// check: start is a cached plan's table, validated against the photons by the gather itself (k_nu_gather, CHECK)
static void launch_gather(bool twod, bool check, int64_t blocks, const double* tt, double t0, const int64_t* start,
                          int64_t nfft, double s1, double fch, double fcl, const double* c2, int nrow, int P,
                          const NuGatherSet& S, int* bad, const double2* tab, double2* W, const NuFold& F,
                          hipStream_t s) {
#define NU_GATHER_R(RR, TD)                                                                                           \
    if (check)                                                                                                        \
        launch_gather_r<RR, TD, true>(blocks, tt, t0, start, nfft, s1, fch, fcl, c2, nrow, P, S, bad, tab, W, F, s);  \
    else                                                                                                              \
        launch_gather_r<RR, TD, false>(blocks, tt, t0, start, nfft, s1, fch, fcl, c2, nrow, P, S, bad, tab, W, F, s)
    if (twod) {
        NU_GATHER_R(kNuGatherRows, true);
    } else {
        NU_GATHER_R(1, false);
    }
#undef NU_GATHER_R
}

static int64_t nu_cus() {  // compute units of the current device (persistent grids)
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        ncu <= 0)
        ncu = 256;
    return ncu;
}

// The radix-8 row kernels' dynamic LDS (above the 64 KB default), set once per device
static int nu_rows_lds_attrs() {
    static std::mutex mu;
    static uint64_t done = 0;
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (dev >= 64 || !(done >> dev & 1)) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_nu_rows_iw),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kNuTile * (int)sizeof(double2)));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_nu_rows_combine8<11>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)nu_rows_lds(11)));
        if (dev < 64) done |= uint64_t(1) << dev;
    }
    return CRIMP_OK;
}

// ---- the plan cache ----
// A search's last plan, keyed by its buffers and shape (crimp_search reuses it on the next identical call; the device
// re-checks its scalars, k_ap_final).
struct NuSpecKey {
    const void* t;
    const void* f;
    int64_t n, nf, nfd, first, count;
    double t0;
    int nharm, stat, dev, gather;
    bool operator==(const NuSpecKey& o) const {
        return t == o.t && f == o.f && n == o.n && nf == o.nf && nfd == o.nfd && first == o.first &&
               count == o.count && t0 == o.t0 && nharm == o.nharm && stat == o.stat && dev == o.dev &&
               gather == o.gather;
    }
};
// A cell-gather plan's start tables (k_nu_cellstart), every row group's and harmonic's as plan_nufft_search lays them
// out, in device memory of the cache's own
struct NuCellTab {
    int64_t* p = nullptr;
    int64_t cap = 0, len = 0;  // int64 entries allocated / used (the sum of every group's tables)
    int dev = 0;               // the device it was allocated on
};
// Up to 16 plans, the oldest dropped first, each with its read-back scalars hs and, for a cell-gather plan under the
// cap (NuHooks::cell_cap), its start tables: built once by a search that ended clean, never written again (every index
// in them lies in [0, n] whatever the photon buffer holds later) and read by the later searches that find the entry,
// whose gathers check them against the photons (k_nu_gather, CHECK). Every search returns with its stream drained and
// calls are serialised (g_mutex), so a table is complete before any later call, on whatever stream, reads it: no
// event is needed. Memory: at most one allocation per entry (16) plus one spare -- a dropped or evicted entry's
// allocation becomes the spare, or is freed when there is one already, and a new table takes the spare when it fits.
// A search that reuses its table allocates and frees nothing.
class NuPlanCache {
  public:
    struct Hold {  // a table a search built for keeping: released unless an entry takes it (store, attach)
        NuPlanCache& c;
        NuCellTab t;
        explicit Hold(NuPlanCache& cache) : c(cache) {}
        ~Hold() { c.release(&t); }
    };
    static NuSpecKey key(const double* t, const double* f, const NuSearchShape& sh, int64_t nfd, double t0, bool gather) {
        NuSpecKey k{};
        k.t = t;
        k.f = f;
        k.n = sh.n;
        k.nf = sh.nf;
        k.nfd = nfd;
        k.first = sh.first;
        k.count = sh.count;
        k.t0 = t0;
        k.nharm = sh.nharm;
        k.stat = sh.stat;
        k.gather = gather ? 1 : 0;
        (void)hipGetDevice(&k.dev);
        return k;
    }
    // *cells: the entry's start tables (still the entry's own), none where it has none or the cell cache is off
    bool find(const NuSpecKey& k, const NuHooks& hooks, double* hs, NuCellTab* cells) const {
        *cells = NuCellTab{};
        if (hooks.plan_cache_off) return false;
        for (const Entry& e : entries_)
            if (e.key == k) {
                std::memcpy(hs, e.hs, sizeof(e.hs));
                if (!hooks.cell_cache_off) *cells = e.cells;
                return true;
            }
        return false;
    }
    // cells: the tables the search built for keeping (acquire), now the entry's; released where nothing is stored
    void store(const NuSpecKey& k, const NuHooks& hooks, const double* hs, NuCellTab* cells) {
        if (hooks.plan_cache_off) {
            release(cells);
            return;
        }
        drop(k);
        if (entries_.size() >= 16) {
            release(&entries_.front().cells);
            entries_.erase(entries_.begin());
        }
        Entry e;
        e.key = k;
        std::memcpy(e.hs, hs, sizeof(e.hs));
        e.cells = *cells;
        *cells = NuCellTab{};
        entries_.push_back(e);
    }
    // a search that ran an entry's plan without tables and built them for keeping: they become the entry's
    void attach(const NuSpecKey& k, const NuHooks& hooks, NuCellTab* cells) {
        for (Entry& e : entries_)
            if (e.key == k && !e.cells.p && !hooks.plan_cache_off) {
                e.cells = *cells;
                *cells = NuCellTab{};
                return;
            }
        release(cells);
    }
    void drop(const NuSpecKey& k) {
        for (size_t i = 0; i < entries_.size(); ++i)
            if (entries_[i].key == k) {
                release(&entries_[i].cells);
                entries_.erase(entries_.begin() + (std::ptrdiff_t)i);
                return;
            }
    }
    // room for len entries (the spare when it fits and is not more than twice too large); false: no memory, no caching
    bool acquire(NuCellTab* t, int64_t len) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (spare_.p && (spare_.dev != dev || spare_.cap < len || spare_.cap > 2 * len + (int64_t(1) << 17))) {
            (void)hipFree(spare_.p);
            spare_ = NuCellTab{};
        }
        if (spare_.p) {
            *t = spare_;
            spare_ = NuCellTab{};
        } else {
            void* p = nullptr;
            if (hipMalloc(&p, (size_t)len * sizeof(int64_t)) != hipSuccess) {
                (void)hipGetLastError();
                return false;
            }
            t->p = static_cast<int64_t*>(p);
            t->cap = len;
            t->dev = dev;
        }
        t->len = len;
        return true;
    }
    void release(NuCellTab* t) {
        if (t->p) {
            if (!spare_.p) {
                spare_ = *t;
            } else {
                (void)hipFree(t->p);
            }
        }
        *t = NuCellTab{};
    }

  private:
    struct Entry {
        NuSpecKey key;
        double hs[5];
        NuCellTab cells;  // none (p == nullptr): an MFMA-slot plan, tables above the cap, or the cell cache off
    };
    std::vector<Entry> entries_;
    NuCellTab spare_;
};
static NuPlanCache g_nu_cache;

// ---- the search ----
// Z^2 / H by NUFFT over trials [first, first + count) of the fd-outer grid (shape: nf trials per row, arithmetic
// progression with step hs[0]).
struct NuSearchIn {
    const double* t = nullptr;  // photon times (seconds); t0 the search's reference time: the kernels form dt = t - t0
    double t0 = 0.0;            // as k_search_prep does (dt and dt^2 arrays are made only for a fix-up)
    const double* freq = nullptr;
    const double* c2 = nullptr;  // the rows' fdot terms (twod)
    bool twod = false;
    NuSearchShape shape;
    NuHooks hooks;
    SearchHooks search_hooks;  // the fix-up threshold and the fix-up's budget (search_plan.h)
    const double* hs = nullptr;  // [delta, f0, dt[0], dt[n-1], unsorted flag (int bits)] (plan_nufft_search)
    double* out = nullptr;
    double* best = nullptr;  // crimp_search_best's [power, index], or nullptr
    bool timed = false, no_fixup = false;
    // [fix-up count, photons out of order (1; cell-gather plans) or a cached plan no longer valid (2), a folded
    // search's gather-failure epoch, -, best power, best index (as doubles)], zeroed or set by k_ap_final (a folded
    // search: by its first gather), read back in one transfer at the end -- the head of a block of kNuFinBytes
    // (search_nufft_finish.h) whose rest a folded search fills and reads back with it
    int* nflag = nullptr;
    // The caller ran no progression check for this cached cell-gather plan (fold_try): nufft_search folds it into the
    // first gather launch where the plan allows (NuRun::fold), and queues the check's own launches first where not
    // (*ap then is the check's device block, as grid_is_progression leaves it).
    bool fold_try = false;
    double** ap = nullptr;
    const NuCellTab* cached = nullptr;  // a cached plan's start tables, or nullptr
    NuCellTab* keep = nullptr;          // receives the tables this search built for the plan cache
};
struct NuSearchOut {
    bool applicable = false;  // false (nothing computed): unsorted photons or an out-of-range plan, the exact rule runs
    bool best_done = false;   // in.best holds the best trial
    bool mismatch = false;    // a cached plan no longer holds: the caller drops it and redoes the search
    int64_t nfixed = 0;
};

// The launches of one search, in the plan's order
struct NuRun {
    Scratch& sc;
    hipStream_t s;
    const NuSearchIn& in;
    const NuSearchPlan& sp;
    // The start tables: the cached plan's (cells_reuse: no cell-start pass, the gathers check them), or built by this
    // search -- into memory the plan cache will own (cells_keep: every group's tables side by side) when the search
    // may be stored and they are under the cap, else into scratch, one group after the other in the same place.
    bool cells_reuse = false, cells_keep = false;
    // A launch-time decision like cells_reuse (the plan is the same either way): a cached plan whose first launch is
    // a checking gather runs no k_ap_check, k_ap_final or k_best_final launch. The check rides in that gather
    // (NuFold), the best trial's candidates stay in the read-back block (best_host), and the host finishes both
    // (search_nufft_finish.h). epoch: this search's, never 0.
    bool fold = false, best_host = false;
    int epoch = 0, ncheck = 0;
    bool first_gather = true;
    double* U = nullptr;
    double2 *W = nullptr, *Y = nullptr, *CS = nullptr;
    int64_t *ctab = nullptr, *cstart = nullptr, *flagged = nullptr;
    BestCand* best_part = nullptr;  // per-block best trials of the fused finalize
    NuPass* dps = nullptr;
    NuTables tab;
    // timed spans (CRIMP_FLAG_TIME_KERNELS): the whole pipeline, then each kernel class's sum
    std::vector<hipEvent_t> ev;
    std::vector<int> evcls;  // class of the span ending at each mark (kNuCls*)

    NuRun(Scratch& sc_, hipStream_t s_, const NuSearchIn& in_, const NuSearchPlan& sp_) : sc(sc_), s(s_), in(in_), sp(sp_) {}
    ~NuRun() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    hipError_t mark() {
        if (!in.timed) return hipSuccess;
        hipEvent_t e = nullptr;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        ev.push_back(e);
        return hipEventRecord(e, s);
    }
    hipError_t span(int cls) {
        if (!in.timed) return hipSuccess;
        evcls.push_back(cls);
        return mark();
    }

    int alloc() {
        if (!sp.gather) {
            HIPCHK(sc.alloc(&U, (size_t)(sp.ubytes / 8)));
            HIPCHK(sc.alloc(&ctab, (size_t)(2 * kNuPassMax * sp.nchunk)));
        }
        if (cells_reuse)
            cstart = in.cached->p;  // read only
        else if (cells_keep)
            cstart = in.keep->p;
        else if (sp.starts_max > 0)
            HIPCHK(sc.alloc(&cstart, (size_t)sp.starts_max));
        HIPCHK(sc.alloc(&W, (size_t)(sp.Bmax * sp.gw)));
        HIPCHK(sc.alloc(&Y, (size_t)sp.Bmax));
        HIPCHK(sc.alloc(&CS, (size_t)sp.csmax));
        HIPCHK(sc.alloc(&flagged, (size_t)in.shape.count));
        if (best_host)
            best_part = reinterpret_cast<BestCand*>(reinterpret_cast<char*>(in.nflag) + kNuFinCandOff);
        else if (sp.best_alloc > 0)
            HIPCHK(sc.alloc(&best_part, (size_t)sp.best_alloc));
        if (!sp.passes.empty()) {
            HIPCHK(sc.alloc(&dps, sp.passes.size()));
            HIPCHK(hipMemcpyAsync(dps, sp.passes.data(), sp.passes.size() * sizeof(NuPass), hipMemcpyHostToDevice, s));
        }
        return CRIMP_OK;
    }

    // The group's start tables. No zeroing: on time-sorted photons every entry is written (each cell's first photon
    // writes it), and on unsorted ones the gathers read none of them (k_nu_gather exits on *bad).
    int cell_starts(const NuGroup& g, int64_t base) {
        const int64_t n = in.shape.n;
        for (const NuCellLaunch& cl : g.cells) {
            NuCellArgs ca = cl.args;
            for (int j = 0; j < cl.nk; ++j) ca.off[j] += base;
            const unsigned cb = (unsigned)std::min<int64_t>(cdiv(cdiv(n, 2), 256 * kNuCellU), 2048);
            if ((reinterpret_cast<uintptr_t>(in.t) & 15u) == 0)
                k_nu_cellstart<true><<<cb, 256, 0, s>>>(in.t, in.t0, n, g.pl.s1, cl.k0, cl.nk, ca, cstart, in.nflag + 1);
            else
                k_nu_cellstart<false><<<cb, 256, 0, s>>>(in.t, in.t0, n, g.pl.s1, cl.k0, cl.nk, ca, cstart, in.nflag + 1);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(span(kNuClsCellStart));
        return CRIMP_OK;
    }

    // one gather launch, then the FFT of each of its harmonics
    int gather_set(const NuGroup& g, const NuBatch& b, const NuGatherSet& set, int64_t base) {
        const NuPlan& pl = g.pl;
        NuGatherSet S = set;
        for (int jj = 0; jj < S.nk; ++jj) S.soff[jj] += base;
        NuFold F;
        if (fold) {
            char* blkp = reinterpret_cast<char*>(in.nflag);
            F.epoch = epoch;
            F.ncheck = first_gather ? ncheck : 0;  // the search's first launch carries the check
            F.f = in.freq;
            F.nf = in.shape.nf;
            F.n = in.shape.n;
            F.pub = reinterpret_cast<double*>(blkp + kNuFinPubOff);
            F.part = reinterpret_cast<double2*>(blkp + kNuFinPartOff);
        }
        first_gather = false;
        launch_gather(in.twod, cells_reuse, S.blk0[S.nk], in.t, in.t0, cstart, int64_t(1) << pl.lnfft, pl.s1, pl.fch,
                      pl.fcl, in.twod ? in.c2 + b.rb : nullptr, b.nrow, pl.P, S, in.nflag + 1, tab.cis2, W, F, s);
        HIPCHK(hipGetLastError());
        HIPCHK(span(kNuClsSpread));
        for (int jj = 0; jj < S.nk; ++jj) {
            const int rc = fft_combine(g, b, S.k[jj], W + S.woff[jj]);
            if (rc) return rc;
        }
        return CRIMP_OK;
    }

    // one MFMA spread launch, then the merge and the FFT of each of its harmonics <= nharm
    int mfma_pass(const NuGroup& g, const NuBatch& b, const NuMfmaPass& mp) {
        const NuPlan& pl = g.pl;
        const int64_t n = in.shape.n, nchunk = sp.nchunk, nfft = int64_t(1) << pl.lnfft;
        const int64_t SL = 2 * (int64_t)pl.P * b.nrow;
        const NuPass& ps = sp.passes[mp.ipass];
        const NuPass* dp = dps + mp.ipass;
        const dim3 grid((unsigned)cdiv(nchunk, kNuWaves));
        if (in.twod)
            nu_launch_spread<true>(mp.gl, grid, s, in.t, in.t0, n, nchunk, pl.s1, pl.fch, pl.fcl, in.c2 + b.rb, b.nrow,
                                   mp.k0, pl.P, dp, tab.cis, U, ctab, in.nflag + 1);
        else
            nu_launch_spread<false>(mp.gl, grid, s, in.t, in.t0, n, nchunk, pl.s1, pl.fch, pl.fcl, in.c2 + b.rb, b.nrow,
                                    mp.k0, pl.P, dp, tab.cis, U, ctab, in.nflag + 1);
        HIPCHK(hipGetLastError());
        HIPCHK(span(kNuClsSpread));
        for (int kk = 0; kk < mp.gl && mp.k0 + kk <= in.shape.nharm; ++kk) {
            const int k = mp.k0 + kk;
            int alo = 0, acnt = 0;
            nu_occupied(pl.gmin[(size_t)(k - 1)], pl.gmax[(size_t)(k - 1)], pl.lnfft, g.ln1, &alo, &acnt);
            const int64_t gbase = (int64_t)alo << g.ln2, gcount = (int64_t)acnt << g.ln2;
            k_nu_merge<<<(unsigned)cdiv(gcount, kNuMergeG), 256, (size_t)kNuMergeG * SL * sizeof(double), s>>>(
                U + ps.ubase[kk], SL, ctab + 2 * kk * nchunk, nchunk, ps.gmin[kk], pl.gmax[(size_t)(k - 1)], nfft, gbase,
                gcount, W, in.nflag + 1);
            HIPCHK(hipGetLastError());
            HIPCHK(span(kNuClsMerge));
            const int rc = fft_combine(g, b, k, W);
            if (rc) return rc;
        }
        return CRIMP_OK;
    }

    // Wk (moments of harmonic k, the batch's rows) -> FFT -> (C_k, S_k) of the batch's trials: columns by ln1, rows by
    // ln2, the generic kernel of each wherever no specialised one exists (or generic_fft); the last harmonic's launch of
    // a fuse_final group finalizes the batch (NuFinal)
    int fft_combine(const NuGroup& g, const NuBatch& b, int k, const double2* Wk) {
        const NuPlan& pl = g.pl;
        const NuSearchShape& sh = in.shape;
        const bool generic_fft = in.hooks.generic_fft;
        const int lnfft = pl.lnfft, P = pl.P, ln1 = g.ln1, ln2 = g.ln2;
        const size_t lds_fft = (size_t)kNuTile * sizeof(double2);
        const int64_t Bp = (int64_t)P * b.nrow;
        const double2* Z = Wk;
        if (ln1 > 0) {
            const int lcol = 12 - ln1;  // columns per block in pass 1 (n1 * c = 4096)
            int alo = 0, acnt = 0;
            nu_occupied(pl.gmin[(size_t)(k - 1)], pl.gmax[(size_t)(k - 1)], lnfft, ln1, &alo, &acnt);
            if (ln1 == 8 && !generic_fft) {
                const int64_t ngroups = Bp << (ln2 - 4);
                k_nu_cols256<<<(unsigned)std::min<int64_t>(ngroups, 2 * nu_cus()), 256, lds_fft, s>>>(
                    Wk, Y, lnfft, tab.T, alo, acnt, ngroups);
            } else if (ln1 == 9 && !generic_fft) {
                const int64_t ngroups = Bp << (ln2 - 3);
                k_nu_cols512<<<(unsigned)std::min<int64_t>(ngroups, 2 * nu_cus()), 512, lds_fft, s>>>(
                    Wk, Y, lnfft, tab.T, alo, acnt, ngroups);
            } else {
                k_nu_fft_cols<<<dim3((unsigned)(int64_t(1) << (ln2 - lcol)), (unsigned)Bp), 256, lds_fft, s>>>(
                    Wk, Y, lnfft, ln1, lcol, tab.T, alo, acnt);
            }
            HIPCHK(hipGetLastError());
            Z = Y;
            HIPCHK(span(kNuClsPass1));
        }
        NuFinal F{};
        if (g.fuse_final && k == sh.nharm) {
            F.on = 1;
            F.m = sh.nharm;
            F.stat = sh.stat;
            F.Pc = P;
            F.nph = (double)sh.n;
            F.invfact = pl.invfact;
            F.rel = in.search_hooks.fixup_rel;
            F.tb0 = b.tb0;
            F.out = in.out;
            F.nflag = in.nflag;
            F.flagged = flagged;
            F.best_part = in.best ? best_part : nullptr;
            F.best_base = b.best_base;
            F.CS0 = CS;
        }
        const dim3 g2((unsigned)(int64_t(1) << ln1), (unsigned)b.nrow);
        const int xcd = in.hooks.row_map;  // nu_row_of_block
        const int64_t jhi = pl.nseg - 1 - pl.h, tbase = b.rb * sh.nf + g.jbase - (b.tb0 + sh.first);
        double2* CSk = CS + (int64_t)(k - 1) * b.nbt;
        // plo = 0, accum = 0: all P moments in the one launch, the sum from zero (see the row kernels' comment)
        if (ln2 == 12 && !generic_fft)
            k_nu_rows_iw<<<g2, 512, 2 * lds_fft, s>>>(Z, lnfft, P, 0, 0, b.nrow, sh.nf, jhi, pl.h, tbase, b.nbt, tab.bc,
                                                      CSk, F, xcd);
        else if (ln2 == 11 && !generic_fft)
            k_nu_rows_combine8<11><<<g2, 256, nu_rows_lds(11), s>>>(Z, lnfft, P, 0, 0, b.nrow, sh.nf, jhi, pl.h, tbase,
                                                                     b.nbt, tab.bc, CSk, F);
        else
            k_nu_fft_rows_combine<<<g2, 256, lds_fft, s>>>(Z, ln2, lnfft, P, b.nrow, sh.nf, jhi, pl.h, tbase, b.nbt,
                                                           tab.bc, CSk, xcd);
        HIPCHK(hipGetLastError());
        HIPCHK(span(kNuClsPass2));
        return CRIMP_OK;
    }

    int finalize(const NuGroup& g, const NuBatch& b) {
        const NuSearchShape& sh = in.shape;
        k_nu_finalize<<<(unsigned)cdiv(b.nbt, 256), 256, 0, s>>>(CS, b.nbt, sh.nharm, sh.stat, (double)sh.n, sh.nf, g.jbase,
                                                                 int64_t(1) << g.pl.lnfft, g.pl.P, g.pl.invfact,
                                                                 in.search_hooks.fixup_rel, b.tb0, sh.first, in.out, in.nflag, flagged);
        HIPCHK(hipGetLastError());
        HIPCHK(span(kNuClsFinalize));
        return CRIMP_OK;
    }

    // every group: its tables, its start tables, then batch by batch spread -> FFT -> finalize
    int launch_all() {
        int cur_lnfft = -1;
        for (const NuGroup& g : sp.groups) {
            int rc = CRIMP_OK;
            if (g.pl.lnfft != cur_lnfft) {  // tables for this group's n (a group's first launch follows their upload)
                rc = nu_tables(s, g.pl.lnfft, &tab);
                if (rc) return rc;
                cur_lnfft = g.pl.lnfft;
            }
            if (ev.empty()) HIPCHK(mark());
            const int64_t base = cells_reuse || cells_keep ? g.starts_off : 0;
            if (sp.gather && !cells_reuse) {
                rc = cell_starts(g, base);
                if (rc) return rc;
            }
            for (const NuBatch& b : g.batches) {
                for (const NuGatherSet& S : b.sets) {
                    rc = gather_set(g, b, S, base);
                    if (rc) return rc;
                }
                for (const NuMfmaPass& mp : b.mfma) {
                    rc = mfma_pass(g, b, mp);
                    if (rc) return rc;
                }
                if (g.fuse_final) continue;
                rc = finalize(g, b);
                if (rc) return rc;
            }
        }
        return CRIMP_OK;
    }

    // the whole pipeline's ms, then the classes' ms, then their launch counts (the plan's)
    int report_times() {
        if (!in.timed) return CRIMP_OK;
        HIPCHK(hipEventSynchronize(ev.back()));
        float tot = 0.0f;
        double cls[kNuCls] = {0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipEventElapsedTime(&tot, ev.front(), ev.back()));
        for (size_t i = 1; i < ev.size(); ++i) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, ev[i - 1], ev[i]));
            cls[evcls[i - 1]] += ms;
        }
        if (g_kernel_times.empty()) g_last_kernel_ms = tot;
        g_kernel_times.push_back(tot);
        for (double v : cls) g_kernel_times.push_back(v);
        for (int c = 0; c < kNuCls; ++c)
            g_kernel_times.push_back(c == kNuClsCellStart && cells_reuse ? 0.0 : (double)sp.launches[c]);
        return CRIMP_OK;
    }
};

// a search epoch: a per-process counter that is never 0 (calls are serialised, g_mutex)
static int nu_next_epoch() {
    static uint32_t e = 0;
    if (++e == 0) ++e;
    return (int)e;
}

static int nufft_search(Scratch& sc, hipStream_t s, const NuSearchIn& in, NuSearchOut* res) {
    *res = NuSearchOut{};
    const NuSearchShape& sh = in.shape;
    const NuSearchPlan sp = plan_nufft_search(in.hs, sh, in.hooks);
    const bool cells_reuse = sp.applicable && sp.gather && in.cached && in.cached->p && in.cached->len == sp.starts_all;
    // the fold needs a checking gather as the search's first launch
    const bool fold = in.fold_try && cells_reuse && !sp.groups.empty() && !sp.groups[0].batches.empty() &&
                      !sp.groups[0].batches[0].sets.empty();
    if (in.fold_try && !fold) {  // the check's own launches, compared on the device (k_ap_final), no read-back
        NuExpect ex{};
        for (int q = 0; q < 4; ++q) ex.v[q] = in.hs[q];
        ex.on = 1;
        bool ok = false;
        const int rc = grid_is_progression(sc, s, in.freq, sh.nf, in.ap, &ok, in.t, in.t0, sh.n, nullptr, false,
                                           in.nflag, &ex);
        if (rc) return rc;
    }
    if (!sp.applicable) return CRIMP_OK;
    res->applicable = true;
    g_last_search_path = 2;
    g_last_nufft_n = sp.last_n;
    g_last_nufft_p = sp.last_p;
    g_last_nufft_gather = sp.gather ? 1 : 0;
    std::memcpy(g_nu_work, sp.work, sizeof(g_nu_work));
    g_last_cells_built = g_last_cells_reused = 0;
    {
        const int rc = nu_rows_lds_attrs();
        if (rc) return rc;
    }
    ARGCHK(in.hooks.lanes_valid(), "CRIMP_NUFFT_LANES must be 1, 2, 4 or 8");
    NuRun run(sc, s, in, sp);
    run.cells_reuse = cells_reuse;
    run.fold = fold;
    if (fold) {
        run.epoch = nu_next_epoch();
        run.ncheck = (int)std::min<int64_t>(cdiv(sh.nf, 256 * 8), kNuFinChecks);
        run.best_host = in.best && sp.separate_batches == 0 && sp.best_count > 0 && sp.best_count <= kNuFinCands;
    }
    run.cells_keep = sp.gather && !run.cells_reuse && in.keep && sp.starts_all > 0 && !in.hooks.plan_cache_off &&
                     !in.hooks.cell_cache_off && sp.starts_all * (int64_t)sizeof(int64_t) <= in.hooks.cell_cap &&
                     g_nu_cache.acquire(in.keep, sp.starts_all);
    (run.cells_reuse ? g_last_cells_reused : g_last_cells_built) = sp.cell_tables;
    int rc = run.alloc();
    if (!rc) rc = run.launch_all();
    if (!rc) rc = run.report_times();
    if (rc) return rc;
    // the best trial of the powers (crimp_search_best) rides on the same read-back; valid unless a fix-up follows
    if (in.best && !run.best_host) {
        if (sp.separate_batches == 0 && sp.best_count > 0) {  // every batch finalized in its row pass: reduce their blocks
            k_best_final<<<1, 256, 0, s>>>(run.best_part, (int)sp.best_count, reinterpret_cast<double*>(in.nflag + 4));
            HIPCHK(hipGetLastError());
        } else {
            rc = launch_best(sc, s, in.out, sh.count, reinterpret_cast<double*>(in.nflag + 4));
            if (rc) return rc;
        }
    }
    int fl[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool stale = false;
    if (fold) {
        // One read-back of the flags, the published scalars, the check's partials and the candidates; the host
        // finishes the check and the best trial (search_nufft_finish.h). A plan that fails -- k_ap_final's test, or a
        // gather wave that stored this search's epoch -- is what fl[1] & 2 is without the fold. The kernels of the
        // failed attempt have then run to completion on stale scalars: in bounds, because the start tables are the
        // cache's own with every index in [0, n] whatever the buffers hold now, and the key fixes the buffers and
        // every shape; what they wrote is overwritten by the redo from a fresh plan.
        alignas(16) static unsigned char hb[kNuFinBytes];  // (calls are serialised, g_mutex)
        const size_t bytes = run.best_host ? kNuFinCandOff + (size_t)sp.best_count * sizeof(NuFinCand)
                                           : kNuFinPartOff + (size_t)run.ncheck * 2 * sizeof(double);
        HIPCHK(d2h(s, hb, in.nflag, bytes));
        std::memcpy(fl, hb, sizeof(fl));
        double dev = 0.0, fm = 0.0;
        nu_finish_partials(reinterpret_cast<const double*>(hb + kNuFinPartOff), run.ncheck, &dev, &fm);
        stale = fl[2] == run.epoch ||
                !nu_finish_plan_ok(reinterpret_cast<const double*>(hb + kNuFinPubOff), sh.nf, dev, fm, in.hs);
        if (run.best_host) {
            const NuFinCand c = nu_finish_best(reinterpret_cast<const NuFinCand*>(hb + kNuFinCandOff), sp.best_count);
            const double bv[2] = {c.v, (double)c.i};
            std::memcpy(fl + 4, bv, sizeof(bv));
        }
    } else {
        HIPCHK(d2h(s, fl, in.nflag, (in.best ? 8 : 2) * sizeof(int)));
    }
    // photons out of order (found by the cell starts), or a cached plan that no longer holds (2, stale): nothing
    // computed, the default path (or a fresh plan) runs
    if (fl[1] || stale) {
        res->applicable = false;
        res->mismatch = stale || (fl[1] & 2) != 0;
        g_last_search_path = 0;
        return CRIMP_OK;
    }
    const int nf_h = fl[0];
    res->nfixed = nf_h;
    if (in.best && (nf_h == 0 || in.no_fixup)) {
        std::memcpy(in.best, fl + 4, 2 * sizeof(double));
        res->best_done = true;
    }
    if (nf_h == 0 || in.no_fixup) return CRIMP_OK;
    double *dt = nullptr, *dt2 = nullptr;  // the fix-up's fp64 kernel reads dt (and dt^2) arrays
    HIPCHK(sc.alloc(&dt, (size_t)sh.n));
    if (in.twod) HIPCHK(sc.alloc(&dt2, (size_t)sh.n));
    k_search_prep<<<(int)std::min<int64_t>(cdiv(sh.n, 256), 4096), 256, 0, s>>>(in.t, sh.n, in.t0, dt, dt2);
    HIPCHK(hipGetLastError());
    return fixup_search(sc, s, dt, dt2, sh.n, in.freq, sh.nf, in.c2, in.twod, sh.nharm, sh.stat, sh.first, run.flagged, nf_h,
                        in.out, in.search_hooks);
}
