// photon_orbit_fit_plan.h -- the host decisions of crimp_photon_orbit_nll / crimp_photon_orbit_mcmc, as pure functions
// of host data: plan_photon_orbit_model is plan_photon_model (photon_fit_plan.h) for a model that must carry an orbit,
// with CRIMP_FIT_SLOT_BINARY slots admitted and the base orbit held to the limits of crimp_binary_delay. The launch
// shape is plan_photon_launch's. No HIP here: crimp_hip.hip includes this header through photon_orbit_fit.h, and
// photon_orbit_fit_plan_check.cpp prints plans on the CPU for tests/test_photon_orbit_host.py.
#pragma once

#include "photon_fit_plan.h"

constexpr int kPofFields = CRIMP_ORBIT_A1DOT + 1;  // CRIMP_ORBIT_PB .. CRIMP_ORBIT_A1DOT

// par's orbit in the units of crimp_timing_model's binary block, indexed by CRIMP_ORBIT_* (orbit_fit.h's OFOrbit)
struct POFOrbit {
    int32_t kind, pad_;
    double raw[kPofFields];
};

// the limits of crimp_binary_delay on a model's orbit, with its texts (crimp_hip.hip: check_binary); nullptr: inside
inline const char* plan_orbit_limits(const crimp_timing_model* m) {
    if (m->binary != CRIMP_BINARY_BT && m->binary != CRIMP_BINARY_ELL1)
        return "binary must be CRIMP_BINARY_NONE, CRIMP_BINARY_BT or CRIMP_BINARY_ELL1";
    const bool bt = m->binary == CRIMP_BINARY_BT;
    if (!(std::isfinite(m->bin_pb) && std::isfinite(m->bin_pbdot) && std::isfinite(m->bin_a1) &&
          std::isfinite(m->bin_a1dot) && std::isfinite(m->bin_t0) && std::isfinite(m->bin_ecc) &&
          std::isfinite(m->bin_om) && std::isfinite(m->bin_omdot) && std::isfinite(m->bin_gamma) &&
          std::isfinite(m->bin_eps1) && std::isfinite(m->bin_eps2)))
        return "a binary parameter is not finite";
    if (!(m->bin_pb > 0.0)) return "PB must be positive";
    if (!(m->bin_a1 >= 0.0)) return "A1 must be >= 0";
    double e = m->bin_ecc;
    if (bt) {
        if (!(e >= 0.0 && e < 1.0)) return "ECC must be in [0, 1)";
    } else {
        e = std::hypot(m->bin_eps1, m->bin_eps2);
        if (!(e < 1.0)) return "EPS1^2 + EPS2^2 must be below 1";
    }
    if (!(2.0 * 3.141592653589793 * m->bin_a1 / (m->bin_pb * 86400.0 * (1.0 - e)) < 0.5))
        return "2 pi A1 / (PB (1 - e)) must be below 1/2";
    return nullptr;
}

// plan_photon_model's outputs, and *orbit = par's orbit. BINARY entries of the map keep their place in a vector:
// dm->kind[k] = CRIMP_FIT_SLOT_BINARY, dm->a[k] = the CRIMP_ORBIT_* field. Returns the CRIMP_ERR_ARG text of a
// refusal, or nullptr.
inline const char* plan_photon_orbit_model(const crimp_timing_model* par, const crimp_fit_map* map, int32_t phoff,
                                           crimp_timing_model* fit, PFMap* dm, int32_t* parts, int32_t* nterms,
                                           POFOrbit* orbit) {
    if (par == nullptr || map == nullptr) return "null argument";
    if (par->binary == CRIMP_BINARY_NONE) return "the model has no binary";
    uint32_t fields = 0;
    if (const char* e = plan_photon_model(par, map, phoff, fit, dm, parts, nterms, &fields)) return e;
    if (const char* e = plan_orbit_limits(par)) return e;
    constexpr uint32_t bt_only = 1u << CRIMP_ORBIT_ECC | 1u << CRIMP_ORBIT_OM | 1u << CRIMP_ORBIT_OMDOT |
                                 1u << CRIMP_ORBIT_GAMMA;
    constexpr uint32_t ell1_only = 1u << CRIMP_ORBIT_EPS1 | 1u << CRIMP_ORBIT_EPS2;
    if (fields & (par->binary == CRIMP_BINARY_BT ? ell1_only : bt_only))
        return "slot names an orbit field the model's kind does not have";
    std::memset(orbit, 0, sizeof(*orbit));
    orbit->kind = par->binary;
    double* r = orbit->raw;
    r[CRIMP_ORBIT_PB] = par->bin_pb;
    r[CRIMP_ORBIT_A1] = par->bin_a1;
    r[CRIMP_ORBIT_T0] = par->bin_t0;
    r[CRIMP_ORBIT_ECC] = par->bin_ecc;
    r[CRIMP_ORBIT_OM] = par->bin_om;
    r[CRIMP_ORBIT_OMDOT] = par->bin_omdot;
    r[CRIMP_ORBIT_GAMMA] = par->bin_gamma;
    r[CRIMP_ORBIT_EPS1] = par->bin_eps1;
    r[CRIMP_ORBIT_EPS2] = par->bin_eps2;
    r[CRIMP_ORBIT_PBDOT] = par->bin_pbdot;
    r[CRIMP_ORBIT_A1DOT] = par->bin_a1dot;
    return nullptr;
}
