// timing_fit.h -- timing-model fits of ToAs: the batched Gaussian NLL of the phase residuals and the ensemble MCMC
// that samples it (utilities_fittoas.py:204-293, fit_toas.py:140-202 of the reference). Included by crimp_hip.hip
// after cp_one, wave_sum and stretch_move.h; the C-ABI (crimp_timing_nll, crimp_timing_mcmc) is in its section 6.
//
// A problem is a set of ToAs (t_mjd, y, yerr) with its fit-model base: the timing model in which every scalar that is
// not an epoch is 0 (utilities_fittoas.py:113-124). A parameter vector overwrites the model fields its slots name
// (crimp_fit_map), the wave sum is multiplied by F0_base - dF0, and the model is evaluated with cp_one -- the
// arithmetic of crimp_calcphase. mu = phases - mean(phases), NLL = gaussian_nll(y - mean(y), mu, yerr).
//
// The two kernels, k_fit_nll<Lik> and k_fit_mcmc<Lik>, are written once for every likelihood of ToAs. A likelihood is
// a policy type Lik (static members only): the wave's LDS state (Wave), the problem's base (Base), the bundle of
// per-ToA arrays (Data: kArrays pointers), load, apply (false: the vector is refused, its NLL is +inf and its mu row
// kRefusedMu), phase, and kKeep, the first-pass phases fit_nll keeps in registers. TimingLik is here, OrbitLik in
// orbit_fit.h.
//
// Layout: one wave per parameter vector, lanes striding the ToAs; the rewritten model lives in LDS, one copy per wave.
// Both sums go through wave_sum in a fixed order (lane l adds ToAs l, l + 64, ... in increasing order, then the
// butterfly), so a value depends on the ToAs and the vector alone: not on P, the problem count or the launch shape.
// tf_phase and fit_nll<Lik> are __noinline__: both kernels call the same machine code, so the sampler's stored
// log-probability equals -crimp_timing_nll of the stored position bit for bit.
//
// The sampler is the stretch move of stretch_move.h. Deviation from the reference: a proposal whose log-probability
// is not finite (NaN included) is rejected, where emcee raises on NaN.
#pragma once

constexpr int kTfNllWaves = 4;  // k_fit_nll: parameter vectors (waves) per block
#ifndef CRIMP_TF_MC_WAVES
#define CRIMP_TF_MC_WAVES 8
#endif
constexpr int kTfMcWaves = CRIMP_TF_MC_WAVES;  // k_fit_mcmc: waves per problem

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

// parameter k (lane k's v) into the field its slot names; coefficients stay (1/n!) * F as calcphase.py:84 forms them.
// kOrbit: a slot that is none of the three spin kinds is a BINARY one, base - v into the wave's raw orbit.
template <bool kOrbit>
__device__ __forceinline__ void tf_apply_slots(CPModel* M, double f0_base, const TFMap* __restrict__ map, double v,
                                               int lane, double* raw, const double* __restrict__ raw_base) {
    const int nd = map->ndim;
    const int fp = map->f0_param;
    const double df0 = __shfl(v, fp >= 0 ? fp : 0);
    if (lane < nd) {
        const int kind = map->kind[lane], a = map->a[lane], b = map->b[lane];
        if (kind == CRIMP_FIT_SLOT_F)
            M->coef[a] = map->inv_fact[a] * v;
        else if (kind == CRIMP_FIT_SLOT_GLITCH)
            M->glitch[a][b] = v;
        else if (!kOrbit || kind == CRIMP_FIT_SLOT_WAVE)
            M->wave_ab[a][b] = v;
        else
            raw[a] = raw_base[a] - v;
    }
    if (lane == 0) M->f0 = f0_base - (fp >= 0 ? df0 : 0.0);
    tf_wave_sync();
}

__device__ __noinline__ double tf_phase(const CPModel* M, double t) { return cp_one(M, t); }

// a problem's ToAs
struct TFData {
    const double* a[3];  // t, y, yerr
};

struct TimingLik {
    using Wave = CPModel;
    using Base = TFModel;
    using Data = TFData;
    static constexpr int kArrays = 3, kKeep = 0;
    static constexpr double kRefusedMu = 0.0;  // no vector is refused
    static __device__ __forceinline__ void load(Wave* M, const Base* __restrict__ base, int lane) {
        tf_load_model(M, base, lane);
    }
    static __device__ __forceinline__ bool apply(Wave* M, const Base* __restrict__ base,
                                                 const TFMap* __restrict__ map, double v, int lane) {
        tf_apply_slots<false>(M, base->f0_base, map, v, lane, nullptr, nullptr);
        return true;
    }
    static __device__ __forceinline__ double phase(const Wave* M, const Data& d, int i) {
        return tf_phase(M, d.a[0][i]);
    }
};

// one ToA's term of the NLL
__device__ __forceinline__ double fit_term(double y, double my, double mu, double s) {
#pragma clang fp contract(off)
    const double r = ((y - my) - mu) / s;
    return r * r + log((2.0 * 3.141592653589793) * (s * s));
}

// NLL of one parameter vector whose model is in Wv (all lanes of one wave; the value is returned in every lane).
// mu_out (may be NULL): the mean-subtracted model residuals. The phases of the first 64 * kKeep ToAs stay in registers
// between the mean's pass and the residuals' pass; past them a ToA is evaluated twice. The summation order does not
// depend on kKeep.
template <class Lik>
__device__ __noinline__ double fit_nll(const typename Lik::Wave* Wv, const typename Lik::Data d, int n, double* mu_out,
                                       int lane) {
#pragma clang fp contract(off)
    constexpr int kKeep = Lik::kKeep;
    const double *y = d.a[1], *e = d.a[2];
    double sp = 0.0, sy = 0.0;
    double keep[kKeep > 0 ? kKeep : 1];
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
        const int i = lane + 64 * k;
        keep[k] = 0.0;
        if (i < n) {
            keep[k] = Lik::phase(Wv, d, i);
            sp += keep[k];
            sy += y[i];
        }
    }
    for (int i = lane + 64 * kKeep; i < n; i += 64) {
        sp += Lik::phase(Wv, d, i);
        sy += y[i];
    }
    sp = wave_sum(sp);
    sy = wave_sum(sy);
    const double mp = sp / (double)n, my = sy / (double)n;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
        const int i = lane + 64 * k;
        if (i < n) {
            const double mu = keep[k] - mp;
            acc += fit_term(y[i], my, mu, e[i]);
            if (mu_out) mu_out[i] = mu;
        }
    }
    for (int i = lane + 64 * kKeep; i < n; i += 64) {
        const double mu = Lik::phase(Wv, d, i) - mp;
        acc += fit_term(y[i], my, mu, e[i]);
        if (mu_out) mu_out[i] = mu;
    }
    return 0.5 * wave_sum(acc);
}

// Block b = (problem, group of kTfNllWaves vectors); wave w of it evaluates vector group * kTfNllWaves + w. d: the
// arrays of all problems, problem i's ToAs from off[i].
template <class Lik>
__global__ __launch_bounds__(kTfNllWaves * 64) void k_fit_nll(
    typename Lik::Data d, const int64_t* __restrict__ off, const typename Lik::Base* __restrict__ models,
    const TFMap* __restrict__ map, const double* __restrict__ pvec, int64_t P, int64_t groups,
    double* __restrict__ nll, double* __restrict__ mu) {
    __shared__ typename Lik::Wave sm[kTfNllWaves];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t prob = blockIdx.x / groups;
    const int64_t p = (blockIdx.x - prob * groups) * kTfNllWaves + wave;
    if (p >= P) return;  // no block-wide barrier below: a wave works alone
    const int nd = map->ndim;
    const int64_t o = off[prob];
    const int n = (int)(off[prob + 1] - o);
    typename Lik::Wave* Wv = &sm[wave];
    Lik::load(Wv, models + prob, lane);
    const double v = lane < nd ? pvec[(prob * P + p) * nd + lane] : 0.0;
    const bool ok = Lik::apply(Wv, models + prob, map, v, lane);
    double* mo = mu ? mu + P * o + p * (int64_t)n : nullptr;
    double r = INFINITY;
    if (ok) {
#pragma unroll
        for (int k = 0; k < Lik::kArrays; ++k) d.a[k] += o;
        r = fit_nll<Lik>(Wv, d, n, mo, lane);
    } else if (mo) {
        for (int i = lane; i < n; i += 64) mo[i] = Lik::kRefusedMu;
    }
    if (lane == 0) nll[prob * P + p] = r;
}

// One workgroup per problem runs every step. Walker positions, log-probabilities and acceptance counts live in LDS,
// with one Lik::Wave per wave and (stage != 0) the problem's kArrays arrays, [kArrays][n]; else they are read from
// global memory. Per step the even walkers are updated against the odd ones as they stand, a barrier, then the odd
// against the updated even, a barrier. Walker w of the half being updated belongs to wave (w / 2) % kTfMcWaves, which
// also writes its row of chain / logprob. A vector outside the box or refused by Lik::apply is not evaluated.
template <class Lik>
__global__ __launch_bounds__(kTfMcWaves * 64) void k_fit_mcmc(
    typename Lik::Data d, const int64_t* __restrict__ off, const typename Lik::Base* __restrict__ models,
    const TFMap* __restrict__ map, const double* __restrict__ p0, const double* __restrict__ lo,
    const double* __restrict__ hi, int W, int64_t steps, uint64_t seed, int64_t first_problem, int stage,
    double* __restrict__ chain, double* __restrict__ logprob, int64_t* __restrict__ accepted) {
    using Wave = typename Lik::Wave;
    extern __shared__ double tf_sm[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t prob = blockIdx.x;
    const int nd = map->ndim;
    const int64_t o = off[prob];
    const int n = (int)(off[prob + 1] - o);
    double* pos = tf_sm;                                               // [W][nd]
    double* lp = pos + W * nd;                                         // [W]
    long long* nacc = reinterpret_cast<long long*>(lp + W);            // [W]
    Wave* Wv = reinterpret_cast<Wave*>(nacc + W) + wave;               // [kTfMcWaves]
    double* st = reinterpret_cast<double*>(reinterpret_cast<Wave*>(nacc + W) + kTfMcWaves);  // [kArrays][n] if staged
#pragma unroll
    for (int k = 0; k < Lik::kArrays; ++k) d.a[k] += o;
    if (stage) {
        const typename Lik::Data g = d;  // in global memory
#pragma unroll
        for (int k = 0; k < Lik::kArrays; ++k) d.a[k] = st + k * n;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
#pragma unroll
            for (int k = 0; k < Lik::kArrays; ++k) st[k * n + i] = g.a[k][i];
        }
    }
    for (int i = threadIdx.x; i < W * nd; i += blockDim.x) pos[i] = p0[prob * W * nd + i];
    for (int i = threadIdx.x; i < W; i += blockDim.x) nacc[i] = 0;
    const typename Lik::Base* base = models + prob;
    Lik::load(Wv, base, lane);
    const double blo = lane < nd ? lo[prob * nd + lane] : 0.0, bhi = lane < nd ? hi[prob * nd + lane] : 0.0;
    __syncthreads();
    // log-probability of the starting positions (outside the box, refused, or a non-finite value: -inf)
    for (int w = wave; w < W; w += kTfMcWaves) {
        const double x = lane < nd ? pos[w * nd + lane] : 0.0;
        const bool in = lane >= nd || (blo < x && x < bhi);
        double l = -INFINITY;
        if (__all(in) && Lik::apply(Wv, base, map, x, lane)) {
            l = -fit_nll<Lik>(Wv, d, n, nullptr, lane);
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
                int cw;
                const double z = sm_draw(seed, gp, s, w, half, h, &cw);
                const double x = lane < nd ? pos[w * nd + lane] : 0.0;
                const double c = lane < nd ? pos[cw * nd + lane] : 0.0;
                bool in;
                const double q = sm_propose(x, c, z, blo, bhi, lane >= nd, &in);
                const double lold = lp[w];
                double lnew = -INFINITY;
                bool ok = __all(in);
                if (ok) ok = Lik::apply(Wv, base, map, q, lane);
                if (ok) {
                    lnew = -fit_nll<Lik>(Wv, d, n, nullptr, lane);
                    ok = isfinite(lnew);
                }
                if (ok) ok = sm_accept(seed, gp, s, w, nd, z, lnew, lold);
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
