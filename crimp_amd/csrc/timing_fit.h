// timing_fit.h -- timing-model fits of ToAs: the batched Gaussian NLL of the phase residuals and the ensemble MCMC
// that samples it (utilities_fittoas.py:204-293, fit_toas.py:140-202 of the reference). Included by crimp_hip.hip
// after cp_one and wave_sum; the C-ABI (crimp_timing_nll, crimp_timing_mcmc) is in its section 6.
//
// A problem is a set of ToAs (t_mjd, y, yerr) with its fit-model base: the timing model in which every scalar that is
// not an epoch is 0 (utilities_fittoas.py:113-124). A parameter vector overwrites the model fields its slots name
// (crimp_fit_map), the wave sum is multiplied by F0_base - dF0, and the model is evaluated with cp_one -- the
// arithmetic of crimp_calcphase. mu = phases - mean(phases), NLL = gaussian_nll(y - mean(y), mu, yerr).
//
// Layout: one wave per parameter vector, lanes striding the ToAs; the rewritten model lives in LDS, one copy per wave.
// Both sums go through wave_sum in a fixed order (lane l adds ToAs l, l + 64, ... in increasing order, then the
// butterfly), so a value depends on the ToAs and the vector alone: not on P, the problem count or the launch shape.
// tf_phase and tf_nll are __noinline__: both kernels call the same machine code, so the sampler's stored
// log-probability equals -crimp_timing_nll of the stored position bit for bit.
//
// The sampler is the affine-invariant stretch move with a = 2 (emcee's default move). The ensemble is split into
// FIXED halves, the even and the odd walkers (emcee draws a fresh random split per step; both are valid, Foreman-
// Mackey et al. 2013 section 3 uses fixed halves). Deviation from the reference: a proposal whose log-probability is
// not finite (NaN included) is rejected, where emcee raises on NaN.
#pragma once

constexpr int kTfNllWaves = 4;  // k_timing_nll: parameter vectors (waves) per block
#ifndef CRIMP_TF_MC_WAVES
#define CRIMP_TF_MC_WAVES 8
#endif
constexpr int kTfMcWaves = CRIMP_TF_MC_WAVES;  // k_timing_mcmc: waves per problem

struct TFModel {
    CPModel m;       // the fit-model base in the kernels' form (parts, wave table and nterms chosen by the host)
    double f0_base;  // F0 of the full model: the wave sum is multiplied by f0_base - dF0
};

struct TFMap {
    int32_t ndim, f0_param;
    int32_t kind[CRIMP_FIT_MAX_DIM], a[CRIMP_FIT_MAX_DIM], b[CRIMP_FIT_MAX_DIM];
    double inv_fact[13];  // 1/n!, n = 1..13, formed as make_cpmodel forms them
};

__device__ __forceinline__ void tf_wave_sync() {
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

// the wave's copy of a problem's base model (all lanes of the wave)
__device__ __forceinline__ void tf_load_model(CPModel* M, const TFModel* __restrict__ base, int lane) {
    const double* src = reinterpret_cast<const double*>(&base->m);
    double* dst = reinterpret_cast<double*>(M);
    static_assert(sizeof(CPModel) % sizeof(double) == 0, "CPModel is copied in doubles");
    for (int i = lane; i < (int)(sizeof(CPModel) / sizeof(double)); i += 64) dst[i] = src[i];
    tf_wave_sync();
}

// parameter k (lane k's v) into the field its slot names; coefficients stay (1/n!) * F as calcphase.py:84 forms them
__device__ __forceinline__ void tf_apply(CPModel* M, double f0_base, const TFMap* __restrict__ map, double v,
                                         int lane) {
    const int nd = map->ndim;
    const int fp = map->f0_param;
    const double df0 = __shfl(v, fp >= 0 ? fp : 0);
    if (lane < nd) {
        const int kind = map->kind[lane], a = map->a[lane], b = map->b[lane];
        if (kind == CRIMP_FIT_SLOT_F)
            M->coef[a] = map->inv_fact[a] * v;
        else if (kind == CRIMP_FIT_SLOT_GLITCH)
            M->glitch[a][b] = v;
        else
            M->wave_ab[a][b] = v;
    }
    if (lane == 0) M->f0 = f0_base - (fp >= 0 ? df0 : 0.0);
    tf_wave_sync();
}

__device__ __noinline__ double tf_phase(const CPModel* M, double t) { return cp_one(M, t); }

// NLL of one parameter vector whose model is in M (all lanes of one wave; the value is returned in every lane).
// mu_out (may be NULL): the mean-subtracted model residuals.
__device__ __noinline__ double tf_nll(const CPModel* M, const double* t, const double* y, const double* e, int n,
                                      double* mu_out, int lane) {
#pragma clang fp contract(off)
    double sp = 0.0, sy = 0.0;
    for (int i = lane; i < n; i += 64) {
        sp += tf_phase(M, t[i]);
        sy += y[i];
    }
    sp = wave_sum(sp);
    sy = wave_sum(sy);
    const double mp = sp / (double)n, my = sy / (double)n;
    double acc = 0.0;
    for (int i = lane; i < n; i += 64) {
        const double mu = tf_phase(M, t[i]) - mp;
        const double s = e[i];
        const double r = ((y[i] - my) - mu) / s;
        acc += r * r + log((2.0 * 3.141592653589793) * (s * s));
        if (mu_out) mu_out[i] = mu;
    }
    return 0.5 * wave_sum(acc);
}

// Block b = (problem, group of kTfNllWaves vectors); wave w of it evaluates vector group * kTfNllWaves + w.
__global__ __launch_bounds__(kTfNllWaves * 64) void k_timing_nll(
    const double* __restrict__ t, const double* __restrict__ y, const double* __restrict__ e,
    const int64_t* __restrict__ off, const TFModel* __restrict__ models, const TFMap* __restrict__ map,
    const double* __restrict__ pvec, int64_t P, int64_t groups, double* __restrict__ nll, double* __restrict__ mu) {
    __shared__ CPModel sm[kTfNllWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t prob = blockIdx.x / groups;
    const int64_t p = (blockIdx.x - prob * groups) * kTfNllWaves + wave;
    if (p >= P) return;  // no block-wide barrier below: a wave works alone
    const int nd = map->ndim;
    const int64_t o = off[prob];
    const int n = (int)(off[prob + 1] - o);
    CPModel* M = &sm[wave];
    tf_load_model(M, models + prob, lane);
    const double v = lane < nd ? pvec[(prob * P + p) * nd + lane] : 0.0;
    tf_apply(M, models[prob].f0_base, map, v, lane);
    double* mo = mu ? mu + P * o + p * (int64_t)n : nullptr;
    const double r = tf_nll(M, t + o, y + o, e + o, n, mo, lane);
    if (lane == 0) nll[prob * P + p] = r;
}

// Philox4x32-10 (Salmon et al. 2011), plain C++: key = the seed, counter = (problem, step, walker, draw)
__device__ __forceinline__ void tf_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint64_t seed,
                                          uint32_t* out) {
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}
// 53 random bits -> a uniform in (0, 1]
__device__ __forceinline__ double tf_uniform(uint32_t a, uint32_t b) {
    const uint64_t k = ((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6);
    return ((double)k + 0.5) * 0x1p-53;
}

// One workgroup per problem runs every step. Walker positions, log-probabilities and acceptance counts live in LDS,
// with one model copy per wave and (stage != 0) the problem's ToAs. Per step the even walkers are updated against the
// odd ones as they stand, a barrier, then the odd against the updated even, a barrier. Walker w of the half being
// updated belongs to wave (w / 2) % kTfMcWaves, which also writes its row of chain / logprob.
__global__ __launch_bounds__(kTfMcWaves * 64) void k_timing_mcmc(
    const double* __restrict__ t, const double* __restrict__ y, const double* __restrict__ e,
    const int64_t* __restrict__ off, const TFModel* __restrict__ models, const TFMap* __restrict__ map,
    const double* __restrict__ p0, const double* __restrict__ lo, const double* __restrict__ hi, int W, int64_t steps,
    uint64_t seed, int64_t first_problem, int stage, double* __restrict__ chain, double* __restrict__ logprob,
    int64_t* __restrict__ accepted) {
    extern __shared__ double tf_sm[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t prob = blockIdx.x;
    const int nd = map->ndim;
    const int64_t o = off[prob];
    const int n = (int)(off[prob + 1] - o);
    double* pos = tf_sm;                                               // [W][nd]
    double* lp = pos + W * nd;                                         // [W]
    long long* nacc = reinterpret_cast<long long*>(lp + W);            // [W]
    CPModel* M = reinterpret_cast<CPModel*>(nacc + W) + wave;          // [kTfMcWaves]
    double* st = reinterpret_cast<double*>(reinterpret_cast<CPModel*>(nacc + W) + kTfMcWaves);  // [3][n] if staged
    const double *tt = t + o, *yy = y + o, *ee = e + o;
    if (stage) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            st[i] = tt[i];
            st[n + i] = yy[i];
            st[2 * n + i] = ee[i];
        }
        tt = st;
        yy = st + n;
        ee = st + 2 * n;
    }
    for (int i = threadIdx.x; i < W * nd; i += blockDim.x) pos[i] = p0[prob * W * nd + i];
    for (int i = threadIdx.x; i < W; i += blockDim.x) nacc[i] = 0;
    tf_load_model(M, models + prob, lane);
    const double f0b = models[prob].f0_base;
    const double blo = lane < nd ? lo[prob * nd + lane] : 0.0, bhi = lane < nd ? hi[prob * nd + lane] : 0.0;
    __syncthreads();
    // log-probability of the starting positions (a position outside the box, or a non-finite value: -inf)
    for (int w = wave; w < W; w += kTfMcWaves) {
        const double x = lane < nd ? pos[w * nd + lane] : 0.0;
        const bool in = lane >= nd || (blo < x && x < bhi);
        double l = -INFINITY;
        if (__all(in)) {
            tf_apply(M, f0b, map, x, lane);
            l = -tf_nll(M, tt, yy, ee, n, nullptr, lane);
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
                if (ok) {
                    tf_apply(M, f0b, map, q, lane);
                    lnew = -tf_nll(M, tt, yy, ee, n, nullptr, lane);
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
