// orbit_fit.h -- timing-model fits of ToAs under a binary orbit (BT, ELL1) with the orbital keys free: the batched
// Gaussian NLL and the ensemble MCMC that samples it. Not in the reference; the definition is DESIGN.md 5.9. Included by
// crimp_hip.hip after timing_fit.h: this header holds OrbitLik, the policy with which timing_fit.h's k_fit_nll and
// k_fit_mcmc (layout, summation order, move and Philox counters) fit the orbit, and k_orbit_prologue; the C-ABI
// (crimp_orbit_nll, crimp_orbit_mcmc) is in crimp_hip.hip's section 6.
//
// A problem is a set of ToAs with the full model par (its orbit B0 included) and the fit-model base of timing_fit.h. A
// parameter vector p overwrites the fit model's fields as there, and its CRIMP_FIT_SLOT_BINARY entries correct the
// orbit: field = base - p in the .par's unit (fp64, one rounding), B(p) the orbit of those numbers. Per ToA
//   tau   = bin_delay(B(p), t)
//   phase = cp_one_t<true>(fit model, t, tau) + R,   R = dtau (nu - nud dtau / 2),   dtau = tau - tau0
// tau0 = bin_delay(B0, t), nu = d phi_par / dt' and nud = d^2 phi_par / dt'^2 at the emission time of B0 are constants
// of the problem: k_orbit_prologue computes them once per call. R is the phase the par spin model accumulates between
// the emission times of B0 and B(p), as one small number. tau0 and tau come from the same machine code (of_delay is
// __noinline__) on orbits derived by the same code (of_derive), so orbital entries of 0 give dtau = 0 and R = 0 exactly.
//
// of_derive recomputes the derived fields with the expressions of make_binmodel, FMA contraction off, and checks the
// limits of crimp_binary_delay before bin_delay runs (its bracket proof rests on them): a vector outside them has
// NLL = +inf (its mu row is +inf too) and the sampler rejects it without evaluating it.
#pragma once

constexpr int kOfFields = 11;  // CRIMP_ORBIT_PB .. CRIMP_ORBIT_A1DOT
#ifndef CRIMP_OF_KEEP
#define CRIMP_OF_KEEP 4
#endif
// first-pass phases a lane keeps in registers (fit_nll's kKeep): ToAs below 64 * kOfKeep are evaluated once (0: every
// ToA twice, as the binary-free fit). 4 against 0 at P = 4096 x 84 ToAs: 62.7 -> 43.0 us (BT, e = 0.7), 44.8 -> 33.8
// us (ELL1) (profiles/orbit_fit_ab_keep.log); the values do not change, the summation order is the same.
constexpr int kOfKeep = CRIMP_OF_KEEP;

struct OFOrbit {
    int32_t kind, pad_;
    double raw[kOfFields];  // the orbit in the units of crimp_timing_model's binary block, indexed by CRIMP_ORBIT_*
};

struct OFModel {
    TFModel tf;
    OFOrbit ob;
};

// a wave's copy: the rewritten fit model, the corrected orbit and its raw fields
struct OFWave {
    CPModel m;
    BinModel b;
    double raw[kOfFields];
};
static_assert(sizeof(OFWave) % sizeof(double) == 0, "OFWave arrays are laid out in doubles");

// the kernels' form of the orbit whose raw fields are `raw` (make_binmodel, expression for expression) into *out when
// `write`; false, and nothing written, for an orbit outside the limits of crimp_binary_delay (check_binary)
__device__ __forceinline__ bool of_derive(int kind, const double* raw, BinModel* out, bool write) {
#pragma clang fp contract(off)
    const bool bt = kind == CRIMP_BINARY_BT;
    const double deg = 3.141592653589793 / 180.0;
    const double pb = raw[CRIMP_ORBIT_PB], a1 = raw[CRIMP_ORBIT_A1], ecc = raw[CRIMP_ORBIT_ECC];
    const double eps1 = raw[CRIMP_ORBIT_EPS1], eps2 = raw[CRIMP_ORBIT_EPS2];
    bool ok = true;
    for (int k = 0; k < kOfFields; ++k) ok = ok && isfinite(raw[k]);
    ok = ok && pb > 0.0 && a1 >= 0.0;
    double e = ecc;
    if (bt) {
        ok = ok && e >= 0.0 && e < 1.0;
    } else {
        e = hypot(eps1, eps2);
        ok = ok && e < 1.0;
    }
    ok = ok && 2.0 * 3.141592653589793 * a1 / (pb * 86400.0 * (1.0 - e)) < 0.5;
    if (ok && write) {
        out->kind = kind;
        out->pad_ = 0;
        out->t0 = raw[CRIMP_ORBIT_T0];
        out->pb = pb * 86400.0;
        out->pbdot = raw[CRIMP_ORBIT_PBDOT];
        out->a1dot = raw[CRIMP_ORBIT_A1DOT];
        out->a1 = a1;
        out->ecc = bt ? ecc : 0.0;
        out->s1me2 = bt ? sqrt((1.0 - ecc) * (1.0 + ecc)) : 1.0;
        out->om = bt ? raw[CRIMP_ORBIT_OM] * deg : 0.0;
        out->omdot = bt ? raw[CRIMP_ORBIT_OMDOT] * deg / (365.25 * 86400.0) : 0.0;
        out->gamma = bt ? raw[CRIMP_ORBIT_GAMMA] : 0.0;
        out->eps1 = bt ? 0.0 : eps1;
        out->eps2 = bt ? 0.0 : eps2;
        out->amp = bt ? 1.0 + ecc : 1.0 + 0.5 * (fabs(eps1) + fabs(eps2));
    }
    return ok;
}

// the wave's copy of a problem's base model and base orbit (all lanes of the wave)
__device__ __forceinline__ void of_load(OFWave* Wv, const OFModel* __restrict__ base, int lane) {
    if (lane < kOfFields) Wv->raw[lane] = base->ob.raw[lane];
    tf_load_model(&Wv->m, &base->tf, lane);
}

// parameter k (lane k's v) into the field its slot names (tf_apply_slots; a BINARY slot: base - v into the raw orbit),
// then the orbit of the raw fields. False (in every lane) for an orbit outside the limits.
__device__ __forceinline__ bool of_apply(OFWave* Wv, const OFModel* __restrict__ base, const TFMap* __restrict__ map,
                                         double v, int lane) {
#pragma clang fp contract(off)
    tf_apply_slots<true>(&Wv->m, base->tf.f0_base, map, v, lane, Wv->raw, base->ob.raw);
    const bool ok = of_derive(base->ob.kind, Wv->raw, &Wv->b, lane == 0);
    tf_wave_sync();
    return ok;
}

__device__ __noinline__ double of_delay(const BinModel* B, double t) { return bin_delay(B, t); }

// nu = d phi / dt' (Hz) and nud = d^2 phi / dt'^2 of the spin model M (all parts) at the emission time t - tau / 86400:
// the glitches active there and the wave term included
__device__ __forceinline__ void of_rates(const CPModel* __restrict__ M, double t, double tau, double* nu_out,
                                         double* nud_out) {
    double nu = 0.0, nud = 0.0;
    {
        const double dt = (t - M->pepoch) * 86400.0 - tau;
        double dn = 1.0, dm = 0.0;  // dt^k, dt^(k-1)
        for (int k = 0; k < M->nterms; ++k) {
            const double c = (double)(k + 1) * M->coef[k];
            nu += c * dn;
            nud += ((double)k * c) * dm;
            dm = dn;
            dn *= dt;
        }
    }
    for (int j = 0; j < M->n_glitch; ++j) {
        const double* g = M->glitch[j];
        const double dts = (t - g[0]) * 86400.0 - tau;
        if (dts >= 0.0) {
            const double td = g[6] * 86400.0;
            const double ex = (g[6] == 0.0) ? 0.0 : exp(-dts / td);
            nu += ((g[2] + g[3] * dts) + (0.5 * g[4]) * (dts * dts)) + g[5] * ex;
            nud += (g[3] + g[4] * dts) - ((g[6] == 0.0) ? 0.0 : g[5] * ex / td);
        }
    }
    if (M->n_wave > 0) {
        const double dw = (t - M->wave_epoch) - tau / 86400.0;
        double a1 = 0.0, a2 = 0.0;
        for (int j = 1; j <= M->n_wave; ++j) {
            const double om = j * M->wave_om, arg = om * dw, os = om / 86400.0;
            double s, c;
            sincos(arg, &s, &c);
            a1 += os * (M->wave_ab[j - 1][0] * c - M->wave_ab[j - 1][1] * s);
            a2 -= (os * os) * (M->wave_ab[j - 1][0] * s + M->wave_ab[j - 1][1] * c);
        }
        nu += M->f0 * a1;
        nud += M->f0 * a2;
    }
    *nu_out = nu;
    *nud_out = nud;
}

// The per-ToA constants of a call: block b = problem b. consts = [3][ntoa]: tau0, nu, nud.
__global__ __launch_bounds__(256) void k_orbit_prologue(const double* __restrict__ t, const int64_t* __restrict__ off,
                                                        const OFModel* __restrict__ models,
                                                        const CPModel* __restrict__ parm, int64_t ntoa,
                                                        double* __restrict__ consts) {
    __shared__ BinModel B0;
    const int64_t prob = blockIdx.x;
    const int64_t o = off[prob];
    const int n = (int)(off[prob + 1] - o);
    if (threadIdx.x == 0) of_derive(models[prob].ob.kind, models[prob].ob.raw, &B0, true);  // the host checked the limits
    __syncthreads();
    const CPModel* M = parm + prob;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double ti = t[o + i];
        const double tau0 = of_delay(&B0, ti);
        double nu, nud;
        of_rates(M, ti, tau0, &nu, &nud);
        consts[o + i] = tau0;
        consts[ntoa + o + i] = nu;
        consts[2 * ntoa + o + i] = nud;
    }
}

// a problem's ToAs and their constants
struct OFData {
    const double* a[6];  // t, y, yerr, tau0, nu, nud
};

__device__ __noinline__ double of_phase(const OFWave* Wv, double t, double tau0, double nu, double nud) {
#pragma clang fp contract(off)
    const double tau = of_delay(&Wv->b, t);
    const double d = tau - tau0;
    const double R = d * (nu - (0.5 * nud) * d);
    return cp_one_t<true>(&Wv->m, t, tau) + R;
}

// the orbit fit as k_fit_nll / k_fit_mcmc see it. A vector whose orbit is outside the limits is refused: NLL = +inf,
// its mu row +inf, and the sampler does not evaluate it.
struct OrbitLik {
    using Wave = OFWave;
    using Base = OFModel;
    using Data = OFData;
    static constexpr int kArrays = 6, kKeep = kOfKeep;
    static constexpr double kRefusedMu = INFINITY;
    static __device__ __forceinline__ void load(Wave* Wv, const Base* __restrict__ base, int lane) {
        of_load(Wv, base, lane);
    }
    static __device__ __forceinline__ bool apply(Wave* Wv, const Base* __restrict__ base,
                                                 const TFMap* __restrict__ map, double v, int lane) {
        return of_apply(Wv, base, map, v, lane);
    }
    static __device__ __forceinline__ double phase(const Wave* Wv, const Data& d, int i) {
        return of_phase(Wv, d.a[0][i], d.a[3][i], d.a[4][i], d.a[5][i]);
    }
};
