// orbit_fit.h -- timing-model fits of ToAs under a binary orbit (BT, ELL1) with the orbital keys free: the batched
// Gaussian NLL and the ensemble MCMC that samples it. Not in the reference; the definition is DESIGN.md 5.9. Included by
// crimp_hip.hip after timing_fit.h, whose layout, summation order, move and Philox counters it keeps; the C-ABI
// (crimp_orbit_nll, crimp_orbit_mcmc) is in its section 6. k_timing_nll / k_timing_mcmc are not touched.
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
// first-pass phases a lane keeps in registers: ToAs below 64 * kOfKeep are evaluated once (0: every ToA twice, as
// tf_nll). 4 against 0 at P = 4096 x 84 ToAs: 62.7 -> 43.0 us (BT, e = 0.7), 44.8 -> 33.8 us (ELL1)
// (profiles/orbit_fit_ab_keep.log); the values do not change, the summation order is the same.
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

// parameter k (lane k's v) into the field its slot names (tf_apply's three kinds; a BINARY slot: base - v into the raw
// orbit), then the orbit of the raw fields. False (in every lane) for an orbit outside the limits.
__device__ __forceinline__ bool of_apply(OFWave* Wv, const OFModel* __restrict__ base, const TFMap* __restrict__ map,
                                         double v, int lane) {
#pragma clang fp contract(off)
    CPModel* M = &Wv->m;
    const int nd = map->ndim;
    const int fp = map->f0_param;
    const double df0 = __shfl(v, fp >= 0 ? fp : 0);
    if (lane < nd) {
        const int kind = map->kind[lane], a = map->a[lane], b = map->b[lane];
        if (kind == CRIMP_FIT_SLOT_F)
            M->coef[a] = map->inv_fact[a] * v;
        else if (kind == CRIMP_FIT_SLOT_GLITCH)
            M->glitch[a][b] = v;
        else if (kind == CRIMP_FIT_SLOT_WAVE)
            M->wave_ab[a][b] = v;
        else
            Wv->raw[a] = base->ob.raw[a] - v;
    }
    if (lane == 0) M->f0 = base->tf.f0_base - (fp >= 0 ? df0 : 0.0);
    tf_wave_sync();
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
    const double *t, *y, *e, *tau0, *nu, *nud;
};

__device__ __noinline__ double of_phase(const OFWave* Wv, double t, double tau0, double nu, double nud) {
#pragma clang fp contract(off)
    const double tau = of_delay(&Wv->b, t);
    const double d = tau - tau0;
    const double R = d * (nu - (0.5 * nud) * d);
    return cp_one_t<true>(&Wv->m, t, tau) + R;
}

// tf_nll on of_phase (all lanes of one wave; the value is returned in every lane). The summation order is tf_nll's.
// The phases of the first 64 * kOfKeep ToAs stay in registers between the mean's pass and the residuals' pass; past
// them a ToA is evaluated twice, as tf_nll does.
__device__ __noinline__ double of_nll(const OFWave* Wv, const OFData d, int n, double* mu_out, int lane) {
#pragma clang fp contract(off)
    double sp = 0.0, sy = 0.0;
    double keep[kOfKeep > 0 ? kOfKeep : 1];
#pragma unroll
    for (int k = 0; k < kOfKeep; ++k) {
        const int i = lane + 64 * k;
        keep[k] = 0.0;
        if (i < n) {
            keep[k] = of_phase(Wv, d.t[i], d.tau0[i], d.nu[i], d.nud[i]);
            sp += keep[k];
            sy += d.y[i];
        }
    }
    for (int i = lane + 64 * kOfKeep; i < n; i += 64) {
        sp += of_phase(Wv, d.t[i], d.tau0[i], d.nu[i], d.nud[i]);
        sy += d.y[i];
    }
    sp = wave_sum(sp);
    sy = wave_sum(sy);
    const double mp = sp / (double)n, my = sy / (double)n;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kOfKeep; ++k) {
        const int i = lane + 64 * k;
        if (i < n) {
            const double mu = keep[k] - mp;
            const double s = d.e[i];
            const double r = ((d.y[i] - my) - mu) / s;
            acc += r * r + log((2.0 * 3.141592653589793) * (s * s));
            if (mu_out) mu_out[i] = mu;
        }
    }
    for (int i = lane + 64 * kOfKeep; i < n; i += 64) {
        const double mu = of_phase(Wv, d.t[i], d.tau0[i], d.nu[i], d.nud[i]) - mp;
        const double s = d.e[i];
        const double r = ((d.y[i] - my) - mu) / s;
        acc += r * r + log((2.0 * 3.141592653589793) * (s * s));
        if (mu_out) mu_out[i] = mu;
    }
    return 0.5 * wave_sum(acc);
}

// k_timing_nll's launch shape: block b = (problem, group of kTfNllWaves vectors)
__global__ __launch_bounds__(kTfNllWaves * 64) void k_orbit_nll(
    const double* __restrict__ t, const double* __restrict__ y, const double* __restrict__ e,
    const double* __restrict__ consts, int64_t ntoa, const int64_t* __restrict__ off,
    const OFModel* __restrict__ models, const TFMap* __restrict__ map, const double* __restrict__ pvec, int64_t P,
    int64_t groups, double* __restrict__ nll, double* __restrict__ mu) {
    __shared__ OFWave sm[kTfNllWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t prob = blockIdx.x / groups;
    const int64_t p = (blockIdx.x - prob * groups) * kTfNllWaves + wave;
    if (p >= P) return;  // no block-wide barrier below: a wave works alone
    const int nd = map->ndim;
    const int64_t o = off[prob];
    const int n = (int)(off[prob + 1] - o);
    OFWave* Wv = &sm[wave];
    of_load(Wv, models + prob, lane);
    const double v = lane < nd ? pvec[(prob * P + p) * nd + lane] : 0.0;
    const bool ok = of_apply(Wv, models + prob, map, v, lane);
    double* mo = mu ? mu + P * o + p * (int64_t)n : nullptr;
    double r = INFINITY;
    if (ok) {
        const OFData d = {t + o, y + o, e + o, consts + o, consts + ntoa + o, consts + 2 * ntoa + o};
        r = of_nll(Wv, d, n, mo, lane);
    } else if (mo) {
        for (int i = lane; i < n; i += 64) mo[i] = INFINITY;
    }
    if (lane == 0) nll[prob * P + p] = r;
}

// k_timing_mcmc on of_nll: the same walkers, halves, move, counters and outputs. The staged arrays (stage != 0) are
// the problem's ToAs and their constants, [6][n].
__global__ __launch_bounds__(kTfMcWaves * 64) void k_orbit_mcmc(
    const double* __restrict__ t, const double* __restrict__ y, const double* __restrict__ e,
    const double* __restrict__ consts, int64_t ntoa, const int64_t* __restrict__ off,
    const OFModel* __restrict__ models, const TFMap* __restrict__ map, const double* __restrict__ p0,
    const double* __restrict__ lo, const double* __restrict__ hi, int W, int64_t steps, uint64_t seed,
    int64_t first_problem, int stage, double* __restrict__ chain, double* __restrict__ logprob,
    int64_t* __restrict__ accepted) {
    extern __shared__ double of_sm[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t prob = blockIdx.x;
    const int nd = map->ndim;
    const int64_t o = off[prob];
    const int n = (int)(off[prob + 1] - o);
    double* pos = of_sm;                                             // [W][nd]
    double* lp = pos + W * nd;                                       // [W]
    long long* nacc = reinterpret_cast<long long*>(lp + W);          // [W]
    OFWave* Wv = reinterpret_cast<OFWave*>(nacc + W) + wave;         // [kTfMcWaves]
    double* st = reinterpret_cast<double*>(reinterpret_cast<OFWave*>(nacc + W) + kTfMcWaves);  // [6][n] if staged
    OFData d = {t + o, y + o, e + o, consts + o, consts + ntoa + o, consts + 2 * ntoa + o};
    if (stage) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            st[i] = d.t[i];
            st[n + i] = d.y[i];
            st[2 * n + i] = d.e[i];
            st[3 * n + i] = d.tau0[i];
            st[4 * n + i] = d.nu[i];
            st[5 * n + i] = d.nud[i];
        }
        d = {st, st + n, st + 2 * n, st + 3 * n, st + 4 * n, st + 5 * n};
    }
    for (int i = threadIdx.x; i < W * nd; i += blockDim.x) pos[i] = p0[prob * W * nd + i];
    for (int i = threadIdx.x; i < W; i += blockDim.x) nacc[i] = 0;
    const OFModel* base = models + prob;
    of_load(Wv, base, lane);
    const double blo = lane < nd ? lo[prob * nd + lane] : 0.0, bhi = lane < nd ? hi[prob * nd + lane] : 0.0;
    __syncthreads();
    // log-probability of the starting positions (outside the box, an orbit outside the limits, a non-finite value: -inf)
    for (int w = wave; w < W; w += kTfMcWaves) {
        const double x = lane < nd ? pos[w * nd + lane] : 0.0;
        const bool in = lane >= nd || (blo < x && x < bhi);
        double l = -INFINITY;
        if (__all(in) && of_apply(Wv, base, map, x, lane)) {
            l = -of_nll(Wv, d, n, nullptr, lane);
            if (!isfinite(l)) l = -INFINITY;
        }
        if (lane == 0) lp[w] = l;
    }
    __syncthreads();
    const int half = W / 2;
    const uint32_t gp = (uint32_t)(first_problem + prob);
    for (int64_t s = 0; s < steps; ++s) {
        for (int h = 0; h < 2; ++h) {
            for (int k = wave; k < half; k += kTfMcWaves) {
                const int w = 2 * k + h;
                uint32_t r[4];
                tf_philox(gp, (uint32_t)s, (uint32_t)w, 0u, seed, r);
                const double u = tf_uniform(r[0], r[1]);
                const int cw = 2 * (int)__umulhi(r[2], (uint32_t)half) + (1 - h);
                const double zr = u + 1.0;  // (a - 1) u + 1, a = 2
                const double z = zr * zr * 0.5;
                const double x = lane < nd ? pos[w * nd + lane] : 0.0;
                const double c = lane < nd ? pos[cw * nd + lane] : 0.0;
                const double q = c - (c - x) * z;
                const bool in = lane >= nd || (blo < q && q < bhi);
                const double lold = lp[w];
                double lnew = -INFINITY;
                bool ok = __all(in);
                if (ok) ok = of_apply(Wv, base, map, q, lane);  // an orbit outside the limits is not evaluated
                if (ok) {
                    lnew = -of_nll(Wv, d, n, nullptr, lane);
                    ok = isfinite(lnew);
                }
                if (ok) {
                    tf_philox(gp, (uint32_t)s, (uint32_t)w, 1u, seed, r);
                    ok = log(tf_uniform(r[0], r[1])) < (double)(nd - 1) * log(z) + lnew - lold;
                }
                if (ok) {
                    if (lane < nd) pos[w * nd + lane] = q;
                    if (lane == 0) {
                        lp[w] = lnew;
                        nacc[w] += 1;
                    }
                }
                const int64_t row = (prob * steps + s) * W + w;
                if (lane < nd) chain[row * nd + lane] = ok ? q : x;
                if (lane == 0) logprob[row] = ok ? lnew : lold;
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < W; i += blockDim.x) accepted[prob * W + i] = nacc[i];
}
