// photon_orbit_fit_plan_check.cpp -- prints the host plan of one crimp_photon_orbit_nll case on the CPU (make
// photon-orbit-plan-check builds it with ASan and UBSan; tests/test_photon_orbit_host.py checks what it prints against
// the definitions restated in Python).
//
// Case on stdin, whitespace-separated (no environment is read; doubles in any form scanf's %lf takes):
//   n P phoff
//   pepoch f0 binary n_glitch n_wave wave_epoch wave_om
//   the orbit, 11 numbers in CRIMP_ORBIT_* order: PB A1 T0|TASC ECC OM OMDOT GAMMA EPS1 EPS2 PBDOT A1DOT
//   n_glitch rows of 7 (GLEP GLPH GLF0 GLF1 GLF2 GLF0D GLTD), then n_wave rows of 2 (A B)
//   ndim, then ndim slots (kind index sub)
//   one vector of ndim + phoff entries
// Plan on stdout, one "key values..." line each; doubles as C99 hex floats (exact). A refusal prints "error <text>"
// alone (the model's before the launch shape's, as the C-ABI's prologue orders them).
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "photon_orbit_fit_plan.h"

static bool rd(double* v) { return scanf("%lf", v) == 1; }
static bool ri(long long* v) { return scanf("%lld", v) == 1; }

int main() {
    long long n, P, phoff, binary, ngl, nwv, ndim;
    crimp_timing_model par;
    std::memset(&par, 0, sizeof(par));
    if (!ri(&n) || !ri(&P) || !ri(&phoff)) return 2;
    if (!rd(&par.pepoch) || !rd(&par.f[0]) || !ri(&binary) || !ri(&ngl) || !ri(&nwv) || !rd(&par.wave_epoch) ||
        !rd(&par.wave_om))
        return 2;
    if (ngl < 0 || ngl > CRIMP_MAX_GLITCH || nwv < 0 || nwv > CRIMP_MAX_WAVE) return 2;
    par.binary = (int32_t)binary;
    par.n_glitch = (int32_t)ngl;
    par.n_wave = (int32_t)nwv;
    double* const field[kPofFields] = {&par.bin_pb,    &par.bin_a1,   &par.bin_t0,   &par.bin_ecc,   &par.bin_om,   &par.bin_omdot,
                                       &par.bin_gamma, &par.bin_eps1, &par.bin_eps2, &par.bin_pbdot, &par.bin_a1dot};
    for (double* f : field)
        if (!rd(f)) return 2;
    for (long long j = 0; j < ngl; ++j)
        for (int c = 0; c < 7; ++c)
            if (!rd(&par.glitch[j][c])) return 2;
    for (long long j = 0; j < nwv; ++j)
        for (int c = 0; c < 2; ++c)
            if (!rd(&par.wave_ab[j][c])) return 2;
    if (!ri(&ndim)) return 2;
    crimp_fit_map map;
    std::memset(&map, 0, sizeof(map));
    map.ndim = (int32_t)ndim;
    const long long nslot = std::min<long long>(std::max<long long>(ndim, 0), CRIMP_FIT_MAX_DIM);
    for (long long k = 0; k < nslot; ++k) {
        long long a, b, c;
        if (!ri(&a) || !ri(&b) || !ri(&c)) return 2;
        map.slot[k].kind = (int32_t)a;
        map.slot[k].index = (int32_t)b;
        map.slot[k].sub = (int32_t)c;
    }
    std::vector<double> vec((size_t)(nslot + (phoff == 1 ? 1 : 0)), 0.0);
    for (double& v : vec)
        if (!rd(&v)) return 2;

    crimp_timing_model fit;
    PFMap dm;
    POFOrbit ob;
    int32_t parts = 0, nterms = 0;
    if (const char* e = plan_photon_orbit_model(&par, &map, (int32_t)phoff, &fit, &dm, &parts, &nterms, &ob)) {
        printf("error %s\n", e);
        return 0;
    }
    PFLaunch L;
    if (const char* e = plan_photon_launch(n, P, &L)) {
        printf("error %s\n", e);
        return 0;
    }
    printf("tile %d\nwaves %d\n", kPfTile, kPfWaves);
    printf("tiles %" PRId64 "\ngroups %" PRId64 "\npartials %" PRId64 "\n", L.tiles, L.groups, L.partials);
    printf("parts %d\nnterms %d\nuse_waves %d\nf0_param %d\nD %d\n", parts, nterms, dm.use_waves, dm.f0_param,
           dm.ndim + dm.phoff);
    printf("fit_pepoch %a\nfit_n_glitch %d\nfit_n_wave %d\nfit_binary %d\n", fit.pepoch, fit.n_glitch, fit.n_wave,
           fit.binary);
    printf("orbit_kind %d\n", ob.kind);
    // the corrected orbit of the vector, as the kernel forms it: base - v on every BINARY entry
    std::vector<double> raw(ob.raw, ob.raw + kPofFields);
    for (int k = 0; k < dm.ndim; ++k) {
        printf("slot %d %d %d %d\n", k, dm.kind[k], dm.a[k], dm.b[k]);
        if (dm.kind[k] == CRIMP_FIT_SLOT_BINARY) raw[(size_t)dm.a[k]] = ob.raw[dm.a[k]] - vec[(size_t)k];
    }
    for (int k = 0; k < kPofFields; ++k) printf("orbit %d %a %a\n", k, ob.raw[k], raw[(size_t)k]);
    if (dm.use_waves) {
        const double df0 = dm.f0_param >= 0 ? vec[(size_t)dm.f0_param] : 0.0;
        for (int j = 0; j < fit.n_wave; ++j) {
            double co[2];
            for (int s = 0; s < 2; ++s) {
                const int idx = dm.wave_param[j][s];
                co[s] = photon_wave_coef(dm.f0_par, dm.wave_par[j][s], df0, idx >= 0 ? vec[(size_t)idx] : 0.0);
            }
            printf("wave_coef %d %a %a\n", j, co[0], co[1]);
        }
    }
    return 0;
}
