// photon_fit_plan.h -- the host decisions of crimp_photon_nll / crimp_photon_mcmc, as pure functions of host data: the
// launch shape and its limits (plan_photon_launch) and the "photon fit model" with its parameter map
// (plan_photon_model), refusals included. No HIP here: crimp_hip.hip includes this header and launches what the plan
// says, and photon_fit_plan_check.cpp prints plans on the CPU for tests/test_photon_fit_host.py.
//
// The photon fit model is the timing model whose cp_one is delta(p) = Phi(t; par) - Phi(t; par - p), a phase of size
// |delta| and not a difference of two ~1e6-cycle phases. The phase is linear in every admitted key, so the model is
// `par` with every linear amplitude (F*, GLPH / GLF0 / GLF1 / GLF2 / GLF0D, WAVE A/B) 0 and every shape value (PEPOCH,
// GLEP, GLTD, WAVEEPOCH, WAVE_OM) kept; a vector's entries overwrite their slots. The wave sum of the full model is
// F0 * sum_j A_j s_j, bilinear in (F0, A): its difference under par -> par - p is the wave sum with coefficients
// (F0 - dF0) dA_j + dF0 A_j(par) and multiplier 1 (PFMap::f0_par, wave_par, wave_param), exact in the cross term.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/crimp_hip.h"

#ifndef CRIMP_PF_TILE
#define CRIMP_PF_TILE 1024
#endif
constexpr int kPfTile = CRIMP_PF_TILE;  // photons per block; a value depends on it (the summation order), on nothing else
constexpr int kPfWaves = 8;             // parameter vectors (waves) per block
static_assert(kPfTile >= 64 && kPfTile % 64 == 0 && kPfTile <= 4096, "the tile is a whole number of wave strides");

struct PFMap {
    int32_t ndim, f0_param;  // map entries; the entry that is F0, or -1
    int32_t phoff;           // 1: a vector has ndim + 1 entries, the last one PHOFF (cycles)
    int32_t use_waves;       // 0: no wave key and no F0 free, the wave sum is skipped
    int32_t kind[CRIMP_FIT_MAX_DIM], a[CRIMP_FIT_MAX_DIM], b[CRIMP_FIT_MAX_DIM];
    double inv_fact[13];                      // 1/n!, n = 1..13, formed as make_cpmodel forms them
    int32_t wave_param[CRIMP_MAX_WAVE][2];    // the entry that is WAVEj A / B, or -1
    double f0_par;                            // F0 of par
    double wave_par[CRIMP_MAX_WAVE][2];       // WAVEj A / B of par
};

struct PFLaunch {
    int64_t tiles = 0, groups = 0;  // grid (tiles, groups) of k_photon_nll
    int64_t partials = 0;           // (sum log m, min m) pairs of scratch: P * tiles
};

// The launch shape of P vectors over n photons, or the text of the limit it declines (nullptr: fine)
inline const char* plan_photon_launch(int64_t n, int64_t P, PFLaunch* L) {
    if (n < 1) return "n < 1";
    if (n > (int64_t(1) << 40)) return "too many photons for one call";
    if (P < 1 || P > (int64_t)65535 * kPfWaves) return "P out of range";
    L->tiles = (n + kPfTile - 1) / kPfTile;
    L->groups = (P + kPfWaves - 1) / kPfWaves;
    if (L->tiles > 2147483647LL) return "too many photons for one call";
    L->partials = P * L->tiles;
    if (L->partials > (int64_t(1) << 31)) return "too many partial sums for one launch";
    return nullptr;
}

// The photon fit model of (par, map, phoff): `fit` is what make_cpmodel takes, *parts and *nterms what the kernel
// evaluates of it (Taylor terms up to the highest free Fn, glitches up to the last free one, waves when use_waves).
// Returns the CRIMP_ERR_ARG text of a refusal, or nullptr. map->branch and map->f0_param are not read.
// orbit_fields (plan_photon_orbit_model; else null): par may carry an orbit and CRIMP_FIT_SLOT_BINARY slots are
// admitted; the mask of the orbit fields they name is returned there, and par's binary block is not read.
inline const char* plan_photon_model(const crimp_timing_model* par, const crimp_fit_map* map, int32_t phoff,
                                     crimp_timing_model* fit, PFMap* dm, int32_t* parts, int32_t* nterms,
                                     uint32_t* orbit_fields = nullptr) {
    if (par == nullptr || map == nullptr) return "null argument";
    if (phoff != 0 && phoff != 1) return "phoff must be 0 or 1";
    if (map->ndim < 1 || map->ndim > CRIMP_FIT_MAX_DIM - phoff) return "ndim must be 1..CRIMP_FIT_MAX_DIM - phoff";
    if (orbit_fields == nullptr && par->binary != CRIMP_BINARY_NONE) return "binary models are not fitted yet";
    if (orbit_fields) *orbit_fields = 0;
    if (par->n_glitch < 0 || par->n_glitch > CRIMP_MAX_GLITCH) return "n_glitch out of range";
    if (par->n_wave < 0 || par->n_wave > CRIMP_MAX_WAVE) return "n_wave out of range";
    std::memset(dm, 0, sizeof(*dm));
    dm->ndim = map->ndim;
    dm->f0_param = -1;
    dm->phoff = phoff;
    double fact = 1.0;
    for (int k = 0; k < 13; ++k) {
        fact *= (double)(k + 1);
        dm->inv_fact[k] = 1.0 / fact;
    }
    for (int j = 0; j < CRIMP_MAX_WAVE; ++j) dm->wave_param[j][0] = dm->wave_param[j][1] = -1;
    int top_f = 0, top_gl = -1;
    bool wave_free = false;
    for (int k = 0; k < map->ndim; ++k) {
        const crimp_fit_slot& sl = map->slot[k];
        if (sl.kind == CRIMP_FIT_SLOT_F) {
            if (sl.index < 0 || sl.index > 12) return "slot names an F term outside F0..F12";
            top_f = std::max(top_f, sl.index + 1);
            if (sl.index == 0) dm->f0_param = k;
        } else if (sl.kind == CRIMP_FIT_SLOT_GLITCH) {
            if (sl.index < 0 || sl.index >= CRIMP_MAX_GLITCH || sl.sub < 0 || sl.sub > 6)
                return "slot names a glitch field outside the model";
            if (sl.index >= par->n_glitch) return "slot names a glitch outside the model";
            if (sl.sub == 0) return "GLEP is not fitted to photons";
            if (sl.sub == 6) return "GLTD is not fitted to photons";
            top_gl = std::max(top_gl, sl.index);
        } else if (sl.kind == CRIMP_FIT_SLOT_WAVE) {
            if (sl.index < 0 || sl.index >= CRIMP_MAX_WAVE || sl.sub < 0 || sl.sub > 1)
                return "slot names a wave field outside the model";
            if (sl.index >= par->n_wave) return "slot names a wave harmonic outside the model";
            dm->wave_param[sl.index][sl.sub] = k;
            wave_free = true;
        } else if (sl.kind == CRIMP_FIT_SLOT_BINARY && orbit_fields != nullptr) {
            if (sl.index < 0 || sl.index > CRIMP_ORBIT_A1DOT)
                return "slot names an orbit field outside CRIMP_ORBIT_PB..CRIMP_ORBIT_A1DOT";
            if (*orbit_fields >> sl.index & 1u) return "two slots name one orbit field";
            *orbit_fields |= 1u << sl.index;
        } else {
            return "unknown slot kind";
        }
        dm->kind[k] = sl.kind;
        dm->a[k] = sl.index;
        dm->b[k] = sl.kind == CRIMP_FIT_SLOT_F ? 0 : sl.sub;
    }
    dm->use_waves = par->n_wave > 0 && (wave_free || dm->f0_param >= 0);
    dm->f0_par = par->f[0];
    std::memcpy(dm->wave_par, par->wave_ab, sizeof(dm->wave_par));
    std::memset(fit, 0, sizeof(*fit));
    fit->pepoch = par->pepoch;
    fit->n_glitch = top_gl + 1;
    for (int j = 0; j < fit->n_glitch; ++j) {
        fit->glitch[j][0] = par->glitch[j][0];
        fit->glitch[j][6] = par->glitch[j][6];
    }
    if (dm->use_waves) {
        fit->n_wave = par->n_wave;
        fit->wave_epoch = par->wave_epoch;
        fit->wave_om = par->wave_om;
    }
    *parts = (top_f > 0 ? 1 : 0) | (top_gl >= 0 ? 2 : 0) | (dm->use_waves ? 4 : 0);
    *nterms = std::max(top_f, 1);
    return nullptr;
}

// the wave coefficient of one harmonic and side for a vector whose F0 and WAVE entries are df0 and da
#ifdef __HIPCC__
__host__ __device__
#endif
inline double photon_wave_coef(double f0_par, double a_par, double df0, double da) {
    return (f0_par - df0) * da + df0 * a_par;
}
