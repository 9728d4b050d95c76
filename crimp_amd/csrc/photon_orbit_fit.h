// photon_orbit_fit.h -- photon-domain timing fits under a binary orbit (BT, ELL1) with the orbital keys free: the
// unbinned template likelihood of every photon for P correction vectors at once, and its ensemble sampler. Not in the
// reference; the definition is DESIGN.md 5.11. Included by crimp_hip.hip after photon_fit.h and orbit_fit.h, whose
// parts it joins: photon_fit.h's tile / pair layout, pf_apply, pf_reduce and k_photon_step, orbit_fit.h's of_derive,
// of_delay, of_rates and of_phase. The host plan is photon_orbit_fit_plan.h, the C-ABI (crimp_photon_orbit_nll,
// crimp_photon_orbit_mcmc) is in crimp_hip.hip's section 6.
//
//   tau_i      = bin_delay(B(p), t_i),   dtau_i = tau_i - tau0_i
//   delta_i(p) = cp_one_t<true>(photon fit model of p, t_i, tau_i) + dtau_i (nu_i - nud_i dtau_i / 2)
//   u_i        = x_i - delta_i(p) - PHOFF
//   NLL(p)     = n ln(norm) - sum_i ln m(u_i),   +inf when some m(u_i) <= 0
//
// tau0 = bin_delay(B0, t), nu and nud (of_rates of par's spin model at the emission time of B0) are constants of the
// photons: k_photon_orbit_prologue writes them once per call, 24 B per photon. B(p) is B0 with field = base - v on
// every BINARY entry, derived per wave by of_derive; a vector it refuses writes the pair (0, -inf) -- NLL = +inf in
// pf_reduce -- and a delta row of +inf, and runs no solve. tau0 and tau come from the same machine code (of_delay) on
// orbits derived by the same code, so orbital entries of 0 give dtau = 0 and R = 0 exactly. A photon whose solve
// reaches kBinMaxIter has a NaN delay: its tile's minimum is set to -inf, so the NLL is +inf and never NaN.
//
// Layout and ownership are k_photon_nll's: grid (photon tiles, groups of kPfWaves vectors), one wave per vector, lane l
// taking photons l, l + 64, ... of the tile in increasing order, then the butterfly; one (sum ln m, min m) pair per
// (vector, tile) in k_photon_nll's scratch layout, so k_photon_reduce, pf_reduce and k_photon_step serve unchanged and
// a value depends on the photons, the vector and kPfTile alone.
//
// The constants of a tile. CRIMP_POF_STAGE = 1 (the default) stages tau0, nu, nud in LDS beside t and x: POFLds is
// 129 KB, past PFLds' 128 KB but under gfx950's 160 KiB per workgroup, and one block per CU either way. 0 reads them
// from global memory where a lane needs them (each is read by the block's eight waves; POFLds is then 105 KB). Staged
// measured 3.5 % faster at 1e6 photons x 256 vectors (BT 9.78 against 10.13 / 10.14 ms, ELL1 7.62 against 7.91 / 7.92
// ms, the two builds alternating in one session).
#pragma once

#include "photon_orbit_fit_plan.h"

#ifndef CRIMP_POF_STAGE
#define CRIMP_POF_STAGE 1
#endif

static_assert(kPofFields == kOfFields, "POFOrbit is OFOrbit's layout");
static_assert(sizeof(POFOrbit) == sizeof(OFOrbit), "POFOrbit is OFOrbit's layout");

struct POFLds {
    double2 tab[kSinTab];  // photon_sincos_tab's table, copied from the call's global one
    double t[kPfTile], x[kPfTile];
#if CRIMP_POF_STAGE
    double c[3][kPfTile];  // tau0, nu, nud of the tile
#endif
    double coef[2][CRIMP_MAX_COMP];  // tpl_coef at phShift 0
    OFWave w[kPfWaves];              // per wave: the photon fit model, B(p), its raw fields
};
static_assert(sizeof(POFLds) <= 160 * 1024, "k_photon_orbit_nll's LDS (gfx950: 160 KiB per workgroup)");

// The per-photon constants of a call: consts = [3][n]: tau0, nu, nud. Each block derives B0 into LDS.
__global__ __launch_bounds__(256) void k_photon_orbit_prologue(const double* __restrict__ t, int64_t n,
                                                               const POFOrbit ob, const CPModel* __restrict__ parm,
                                                               double* __restrict__ consts) {
    __shared__ BinModel B0;
    if (threadIdx.x == 0) of_derive(ob.kind, ob.raw, &B0, true);  // the host checked the limits
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double ti = t[i];
        const double tau0 = of_delay(&B0, ti);
        double nu, nud;
        of_rates(parm, ti, tau0, &nu, &nud);
        consts[i] = tau0;
        consts[n + i] = nu;
        consts[2 * n + i] = nud;
    }
}

// Block (tile, group); wave w of it evaluates vector group * kPfWaves + w on the tile's photons. active (may be NULL):
// vectors with active[p] == 0 are skipped and their pairs left as they are (the sampler's out-of-box proposals).
// pvec rows have D = ndim + phoff entries. delta (may be NULL): [P][n].
__global__ __launch_bounds__(kPfWaves * 64) void k_photon_orbit_nll(
    const double* __restrict__ t, const double* __restrict__ x, const double* __restrict__ consts, int64_t n,
    const CPModel* __restrict__ base, const POFOrbit ob, const PFMap* __restrict__ map, const TplDev* __restrict__ T,
    const double2* __restrict__ gtab, double norm, const double* __restrict__ pvec, const int32_t* __restrict__ active,
    int64_t P, double* __restrict__ psum, double* __restrict__ pmin, double* __restrict__ delta) {
    extern __shared__ double2 pof_sm[];
    POFLds& S = *reinterpret_cast<POFLds*>(pof_sm);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t tile = blockIdx.x, tiles = gridDim.x;
    const int64_t i0 = tile * kPfTile;
    const int cnt = (int)(n - i0 < kPfTile ? n - i0 : kPfTile);
    const int model = T->model, K = T->K;
    for (int i = tid; i < kSinTab; i += kPfWaves * 64) S.tab[i] = gtab[i];
    for (int i = tid; i < cnt; i += kPfWaves * 64) {
        S.t[i] = t[i0 + i];
        S.x[i] = x[i0 + i];
#if CRIMP_POF_STAGE
        for (int k = 0; k < 3; ++k) S.c[k][i] = consts[k * n + i0 + i];
#endif
    }
    if (tid < K) tpl_coef(T, tid, 0.0, S.coef[0][tid], S.coef[1][tid]);
    __syncthreads();
    const int64_t p = (int64_t)blockIdx.y * kPfWaves + wave;
    if (p >= P) return;  // no block-wide barrier below: a wave works alone
    if (active && !active[p]) return;
    const int nd = map->ndim, D = nd + map->phoff;
    OFWave* Wv = &S.w[wave];
    {
        const double* src = reinterpret_cast<const double*>(base);
        double* dst = reinterpret_cast<double*>(&Wv->m);
        for (int i = lane; i < (int)(sizeof(CPModel) / sizeof(double)); i += 64) dst[i] = src[i];
        if (lane < kOfFields) Wv->raw[lane] = ob.raw[lane];
        tf_wave_sync();
    }
    const double v = lane < D ? pvec[p * D + lane] : 0.0;
    const double sv = __shfl(v, nd < 64 ? nd : 0);
    const double phoff = map->phoff ? sv : 0.0;
    pf_apply(&Wv->m, map, v, lane);
    bool ok;
    {
#pragma clang fp contract(off)
        if (lane < nd && map->kind[lane] == CRIMP_FIT_SLOT_BINARY) {
            const int a = map->a[lane];
            Wv->raw[a] = ob.raw[a] - v;
        }
        tf_wave_sync();
        ok = of_derive(ob.kind, Wv->raw, &Wv->b, lane == 0);
        tf_wave_sync();
    }
    double* dout = delta ? delta + p * n + i0 : nullptr;
    if (!ok) {  // the same in every lane: an orbit outside the limits, refused before any solve
        if (dout)
            for (int i = lane; i < cnt; i += 64) dout[i] = INFINITY;
        if (lane == 0) {
            psum[p * tiles + tile] = 0.0;
            pmin[p * tiles + tile] = -INFINITY;
        }
        return;
    }
    double acc = 0.0, mn = INFINITY;
    for (int i = lane; i < cnt; i += 64) {
#if CRIMP_POF_STAGE
        const double tau0 = S.c[0][i], nu = S.c[1][i], nud = S.c[2][i];
#else
        const double tau0 = consts[i0 + i], nu = consts[n + i0 + i], nud = consts[2 * n + i0 + i];
#endif
        const double d = of_phase(Wv, S.t[i], tau0, nu, nud);
        const double u = (S.x[i] - d) - phoff;
        double s1, c1, h, h1, h2;
        photon_sincos_tab(CRIMP_MODEL_FOURIER, S.tab, u, s1, c1);  // u in cycles for every template model
        tpl_terms(T, model, K, S.coef[0], S.coef[1], s1, c1, h, h1, h2);
        const double mv = norm + h;
        acc += log(mv);
        mn = fmin(mn, mv == mv ? mv : -INFINITY);  // an unconverged solve (NaN): the NLL is +inf
        if (dout) dout[i] = d;
    }
    acc = wave_sum(acc);
    mn = wave_min(mn);
    if (lane == 0) {
        psum[p * tiles + tile] = acc;
        pmin[p * tiles + tile] = mn;
    }
}
