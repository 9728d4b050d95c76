// stretch_move.h -- what every ensemble sampler of the library shares: Philox4x32-10 with the 53-bit uniform (the event
// simulator draws from them too) and the affine-invariant stretch move with a = 2 (emcee's default move), written once
// as the draw, the proposal of a lane and the acceptance test. Included by crimp_hip.hip before timing_fit.h.
//
// The ensemble is split into FIXED halves, the even and the odd walkers (emcee draws a fresh random split per step;
// both are valid, Foreman-Mackey et al. 2013 section 3 uses fixed halves). Walker w of half h (w = 2 k + h) at step s
// of global problem gp reads two Philox blocks, counter = (gp, s, w, draw): draw 0 gives z and the partner, draw 1 the
// uniform of the acceptance test. k_fit_mcmc (timing_fit.h) and k_photon_step (photon_fit.h) are the callers; the
// functions carry no fp-contract pragma, as their callers carry none.
#pragma once

// Philox4x32-10 (Salmon et al. 2011), plain C++: key = the seed
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

// the stretch factor z of walker w = 2 k + h and *cw, its partner among the `half` walkers of the other half
__device__ __forceinline__ double sm_draw(uint64_t seed, uint32_t gp, int64_t s, int w, int half, int h, int* cw) {
    uint32_t r[4];
    tf_philox(gp, (uint32_t)s, (uint32_t)w, 0u, seed, r);
    const double u = tf_uniform(r[0], r[1]);
    *cw = 2 * (int)__umulhi(r[2], (uint32_t)half) + (1 - h);
    const double zr = u + 1.0;  // (a - 1) u + 1, a = 2
    return zr * zr * 0.5;
}

// a lane's entry of the proposal from the walker's x and the partner's c; *in: inside the open box (blo, bhi), or a
// lane past the D entries
__device__ __forceinline__ double sm_propose(double x, double c, double z, double blo, double bhi, bool past,
                                             bool* in) {
    const double q = c - (c - x) * z;
    *in = past || (blo < q && q < bhi);
    return q;
}

// the acceptance test of a proposal with D entries whose log-probability lnew is finite
__device__ __forceinline__ bool sm_accept(uint64_t seed, uint32_t gp, int64_t s, int w, int D, double z, double lnew,
                                          double lold) {
    uint32_t r[4];
    tf_philox(gp, (uint32_t)s, (uint32_t)w, 1u, seed, r);
    return log(tf_uniform(r[0], r[1])) < (double)(D - 1) * log(z) + lnew - lold;
}
