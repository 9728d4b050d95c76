// photon_fit.h -- photon-domain timing fits: the unbinned template likelihood of every photon folded with a corrected
// timing model, for P correction vectors at once, and the ensemble sampler of it. Not in the reference.
// Included by crimp_hip.hip after cp_one, TplDev / tpl_coef / photon_sincos_tab / tpl_terms, wave_sum / wave_min and
// stretch_move.h; the host plan is photon_fit_plan.h, the C-ABI (crimp_photon_nll, crimp_photon_mcmc) is in
// crimp_hip.hip's section 6.
//
//   delta_i(p) = cp_one(photon fit model of p, t_i)      (= Phi(t_i; par) - Phi(t_i; par - p), photon_fit_plan.h)
//   u_i        = x_i - delta_i(p) - PHOFF                (cycles; x_i the folded phase under par)
//   NLL(p)     = n ln(norm) - sum_i ln m(u_i),  m = norm + h;   +inf when some m(u_i) <= 0
//
// Layout: grid (photon tiles, groups of kPfWaves vectors). A block stages its tile's t and x in LDS with the sin/cos
// table and the template's coefficient rows; each wave owns one vector, its model copy in LDS, and strides the tile:
// lane l adds photons l, l + 64, ... of the tile in increasing order, then the butterfly. One (sum ln m, min m) pair is
// written per (vector, tile); pf_reduce adds a vector's pairs over the tiles the same way (lane l tiles l, l + 64, ...,
// then the butterfly). So a value depends on the photons, the vector and kPfTile alone: not on P, on how vectors fall
// into groups, or on who asked. The sampler launches this same kernel for its proposals and calls the same
// __noinline__ pf_reduce, so its stored log-probability equals -crimp_photon_nll of the stored position bit for bit.
#pragma once

#include "photon_fit_plan.h"

constexpr int kPfStepWaves = 8;  // k_photon_step: waves of its one block

struct PFLds {
    double2 tab[kSinTab];  // photon_sincos_tab's table, copied from the call's global one
    double t[kPfTile], x[kPfTile];
    double coef[2][CRIMP_MAX_COMP];  // tpl_coef at phShift 0
    CPModel m[kPfWaves];
};
static_assert(sizeof(PFLds) <= 128 * 1024, "k_photon_nll's LDS");

__global__ __launch_bounds__(256) void k_photon_table(double2* __restrict__ tab) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < kSinTab) {
        double sv, cv;
        sincospi((double)i * (2.0 / kSinTab), &sv, &cv);
        tab[i] = make_double2(cv, sv);
    }
}

// a vector's entries (lane k holds entry k) into the wave's model copy: Fn and glitch amplitudes into their slots, the
// wave coefficients (F0 - dF0) dA_j + dF0 A_j(par) with lane j forming harmonic j's pair
__device__ __forceinline__ void pf_apply(CPModel* M, const PFMap* __restrict__ map, double v, int lane) {
    const int nd = map->ndim, fp = map->f0_param;
    const double s0 = __shfl(v, fp >= 0 ? fp : 0);
    const double df0 = fp >= 0 ? s0 : 0.0;
    if (lane < nd) {
        const int kind = map->kind[lane], a = map->a[lane], b = map->b[lane];
        if (kind == CRIMP_FIT_SLOT_F)
            M->coef[a] = map->inv_fact[a] * v;
        else if (kind == CRIMP_FIT_SLOT_GLITCH)
            M->glitch[a][b] = v;
    }
    if (map->use_waves) {
        static_assert(CRIMP_MAX_WAVE == 64, "one lane per wave harmonic");
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int idx = map->wave_param[lane][s];
            const double sv = __shfl(v, idx >= 0 ? idx : 0);
            const double da = idx >= 0 ? sv : 0.0;
            if (lane < M->n_wave) M->wave_ab[lane][s] = photon_wave_coef(map->f0_par, map->wave_par[lane][s], df0, da);
        }
    }
    tf_wave_sync();
}

// Block (tile, group); wave w of it evaluates vector group * kPfWaves + w on the tile's photons. active (may be NULL):
// vectors with active[p] == 0 are skipped and their pairs left as they are (the sampler's out-of-box proposals).
// pvec rows have D = ndim + phoff entries. delta (may be NULL): [P][n].
__global__ __launch_bounds__(kPfWaves * 64) void k_photon_nll(
    const double* __restrict__ t, const double* __restrict__ x, int64_t n, const CPModel* __restrict__ base,
    const PFMap* __restrict__ map, const TplDev* __restrict__ T, const double2* __restrict__ gtab, double norm,
    const double* __restrict__ pvec, const int32_t* __restrict__ active, int64_t P, double* __restrict__ psum,
    double* __restrict__ pmin, double* __restrict__ delta) {
    extern __shared__ double2 pf_sm[];
    PFLds& S = *reinterpret_cast<PFLds*>(pf_sm);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t tile = blockIdx.x, tiles = gridDim.x;
    const int64_t i0 = tile * kPfTile;
    const int cnt = (int)(n - i0 < kPfTile ? n - i0 : kPfTile);
    const int model = T->model, K = T->K;
    for (int i = tid; i < kSinTab; i += kPfWaves * 64) S.tab[i] = gtab[i];
    for (int i = tid; i < cnt; i += kPfWaves * 64) {
        S.t[i] = t[i0 + i];
        S.x[i] = x[i0 + i];
    }
    if (tid < K) tpl_coef(T, tid, 0.0, S.coef[0][tid], S.coef[1][tid]);
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.y * kPfWaves + wave;
    if (p >= P) return;  // no block-wide barrier below: a wave works alone
    if (active && !active[p]) return;
    const int nd = map->ndim, D = nd + map->phoff;
    CPModel* M = &S.m[wave];
    {
        const double* src = reinterpret_cast<const double*>(base);
        double* dst = reinterpret_cast<double*>(M);
        for (int i = lane; i < (int)(sizeof(CPModel) / sizeof(double)); i += 64) dst[i] = src[i];
        tf_wave_sync();
    }
    const double v = lane < D ? pvec[p * D + lane] : 0.0;
    const double sv = __shfl(v, nd < 64 ? nd : 0);
    const double phoff = map->phoff ? sv : 0.0;
    pf_apply(M, map, v, lane);
    double* dout = delta ? delta + p * n + i0 : nullptr;
    double acc = 0.0, mn = INFINITY;
    for (int i = lane; i < cnt; i += 64) {
        const double d = cp_one(M, S.t[i]);
        const double u = (S.x[i] - d) - phoff;
        double s1, c1, h, h1, h2;
        photon_sincos_tab(CRIMP_MODEL_FOURIER, S.tab, u, s1, c1);  // u in cycles for every template model
        tpl_terms(T, model, K, S.coef[0], S.coef[1], s1, c1, h, h1, h2);
        const double mv = norm + h;
        acc += log(mv);
        mn = fmin(mn, mv);
        if (dout) dout[i] = d;
    }
    acc = wave_sum(acc);
    mn = wave_min(mn);
    if (lane == 0) {
        psum[p * tiles + tile] = acc;
        pmin[p * tiles + tile] = mn;
    }
}

// NLL of one vector from its pairs (all lanes of one wave; the value is returned in every lane)
__device__ __noinline__ double pf_reduce(const double* psum, const double* pmin, int64_t tiles, int64_t n, double norm,
                                         int lane) {
#pragma clang fp contract(off)
    double s = 0.0, m = INFINITY;
    for (int64_t k = lane; k < tiles; k += 64) {
        s += psum[k];
        m = fmin(m, pmin[k]);
    }
    s = wave_sum(s);
    m = wave_min(m);
    const double v = (double)n * log(norm) - s;
    return m > 0.0 ? v : INFINITY;
}

__global__ __launch_bounds__(256) void k_photon_reduce(const double* __restrict__ psum, const double* __restrict__ pmin,
                                                       int64_t tiles, int64_t n, double norm, int64_t P,
                                                       double* __restrict__ nll) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    const double r = pf_reduce(psum + p * tiles, pmin + p * tiles, tiles, n, norm, lane);
    if (lane == 0) nll[p] = r;
}

// The sampler's state and outputs (device memory all)
struct PFMc {
    const double *p0, *lo, *hi;  // [W][D], [D], [D]
    double *pos, *lp;            // walkers [W][D], their log-probabilities [W]
    long long* nacc;             // [W]
    double *prop, *pz;           // the half's proposals [W/2][D] and their z
    int32_t* act;                // [W]: proposal k is inside the box (mode 0: walker w's start is)
    const double *psum, *pmin;   // the pairs k_photon_nll wrote for the proposals, [.][tiles]
    int64_t tiles, n;
    double norm;
    int32_t W, D;
    uint64_t seed;
    double *chain, *logprob;     // [steps][W][D], [steps][W]
    int64_t* accepted;           // [W]
};

// the stretch proposals of half h at step s (stretch_move.h's move and random stream, problem index 0)
__device__ __forceinline__ void pf_propose(const PFMc& A, int64_t s, int h, int wave, int lane) {
    const int D = A.D, half = A.W / 2;
    const double blo = lane < D ? A.lo[lane] : 0.0, bhi = lane < D ? A.hi[lane] : 0.0;
    for (int k = wave; k < half; k += kPfStepWaves) {
        const int w = 2 * k + h;
        int cw;
        const double z = sm_draw(A.seed, 0u, s, w, half, h, &cw);
        const double x = lane < D ? A.pos[w * D + lane] : 0.0;
        const double c = lane < D ? A.pos[cw * D + lane] : 0.0;
        bool in;
        const double q = sm_propose(x, c, z, blo, bhi, lane >= D, &in);
        const bool ok = __all(in);
        if (lane < D) A.prop[k * D + lane] = q;
        if (lane == 0) {
            A.pz[k] = z;
            A.act[k] = ok ? 1 : 0;
        }
    }
}

// One block, between the likelihood launches of a chain.
//   mode 0: the walkers take p0; act[w] = the start is inside the box.            (then k_photon_nll on pos, W vectors)
//   mode 1: lp[w] of the starts (outside the box or not finite: -inf); proposals of (0, 0).      (then on prop, W / 2)
//   mode 2: accept or reject the proposals of (s, h), write that half's rows of chain / logprob; then the proposals
//           of the next half-step, or (last) the acceptance counts.
__global__ __launch_bounds__(kPfStepWaves * 64) void k_photon_step(PFMc A, int mode, int64_t s, int h, int last) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int W = A.W, D = A.D, half = W / 2;
    if (mode == 0) {
        const double blo = lane < D ? A.lo[lane] : 0.0, bhi = lane < D ? A.hi[lane] : 0.0;
        for (int w = wave; w < W; w += kPfStepWaves) {
            const double x = lane < D ? A.p0[w * D + lane] : 0.0;
            const bool in = lane >= D || (blo < x && x < bhi);
            const bool ok = __all(in);
            if (lane < D) A.pos[w * D + lane] = x;
            if (lane == 0) {
                A.act[w] = ok ? 1 : 0;
                A.nacc[w] = 0;
            }
        }
        return;
    }
    if (mode == 1) {
        for (int w = wave; w < W; w += kPfStepWaves) {
            double l = -INFINITY;
            if (A.act[w]) {
                l = -pf_reduce(A.psum + w * A.tiles, A.pmin + w * A.tiles, A.tiles, A.n, A.norm, lane);
                if (!isfinite(l)) l = -INFINITY;
            }
            if (lane == 0) A.lp[w] = l;
        }
        __syncthreads();
        pf_propose(A, 0, 0, wave, lane);
        return;
    }
    for (int k = wave; k < half; k += kPfStepWaves) {
        const int w = 2 * k + h;
        const double lold = A.lp[w];
        const double z = A.pz[k];
        const double x = lane < D ? A.pos[w * D + lane] : 0.0;
        const double q = lane < D ? A.prop[k * D + lane] : 0.0;
        double lnew = -INFINITY;
        bool ok = A.act[k] != 0;
        if (ok) {
            lnew = -pf_reduce(A.psum + k * A.tiles, A.pmin + k * A.tiles, A.tiles, A.n, A.norm, lane);
            ok = isfinite(lnew);
        }
        if (ok) ok = sm_accept(A.seed, 0u, s, w, D, z, lnew, lold);
        if (ok) {
            if (lane < D) A.pos[w * D + lane] = q;
            if (lane == 0) {
                A.lp[w] = lnew;
                A.nacc[w] += 1;
            }
        }
        const int64_t row = s * W + w;
        if (lane < D) A.chain[row * D + lane] = ok ? q : x;
        if (lane == 0) A.logprob[row] = ok ? lnew : lold;
    }
    __syncthreads();
    if (last) {
        for (int i = threadIdx.x; i < W; i += blockDim.x) A.accepted[i] = A.nacc[i];
    } else {
        pf_propose(A, s + h, 1 - h, wave, lane);
    }
}
