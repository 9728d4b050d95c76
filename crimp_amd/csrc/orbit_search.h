// orbit_search.h -- the Z^2_m / H search over a grid of binary orbits (BT, ELL1), fused on the device: the kernels of
// crimp_orbit_search. Not in the reference; the definition is DESIGN.md 5.10. Included by crimp_hip.hip after
// orbit_fit.h (of_derive, OFOrbit) and binary_delay.h (bin_delay); the host plan is orbit_search_plan.h and the C-ABI
// is in crimp_hip.hip's section 6.
//
// k_orbit_search: workgroup (slice s, orbit o of the batch). The workgroup builds B_o once: the base orbit's raw
// fields with the keyed ones replaced by row o of `orbits`, derived by of_derive (the expressions of make_binmodel)
// into LDS, where every lane reads it (one address: a broadcast). Phase A: lane l solves bin_delay for photons l, l + 256, ... of the slice and
// writes dt = fl(fl((t - tref) 86400) - tau) (and fl(dt dt) with an fdot) to LDS: a photon is solved once per orbit.
// Phase B: for every harmonic group (k0, G) and every chunk of J trials a lane runs over the same photons of the slice
// (consecutive lanes read consecutive LDS addresses) with the arithmetic of k_search_f64 -- ph = f d or
// fma(f, d, c2 d^2), ph - rint(ph), fp64 sincospi, the harmonics of the group by fused angle addition, fp64
// lane-private sums --, then the 16 lanes of a DPP row are added in a fixed order (os_row_sum), the 16 rows of the
// workgroup in index order, and the sums stored to part[slice][orbit][comp][trial]. Every lane works at nf = 1 as at
// nf = 64. J x G <= kOsAcc keeps the accumulators in registers. A lane whose bin_delay reaches kBinMaxIter has dt =
// NaN, which makes every sum of that orbit NaN: no loop waits on convergence.
//
// k_orbit_search_finalize: workgroup o adds the slices in index order and forms Z^2_m / H as k_search_finalize does;
// with `best` it also writes the orbit's best (power, trial), np.argmax semantics (best_better).
#pragma once

#include "orbit_search_plan.h"

struct OSArgs {
    OFOrbit base;              // the base orbit's kind and raw fields
    int32_t col[kOfFields];    // the column of `orbits` that replaces field k, or -1
    int32_t nkeys;
    double tref, c2;           // MJD; 0.5 fdot
    int32_t nharm, pad_;
};

template <int CTRL>
__device__ __forceinline__ double os_dpp(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
// the sum of the 16 lanes of a DPP row, in every lane of the row, in one order: neighbours (quad_perm [1, 0, 3, 2]),
// pairs ([2, 3, 0, 1]), the quads of a half row (row_half_mirror), the halves (row_mirror). All 64 lanes are active.
__device__ __forceinline__ double os_row_sum(double v) {
    v += os_dpp<0xB1>(v);
    v += os_dpp<0x4E>(v);
    v += os_dpp<0x141>(v);
    v += os_dpp<0x140>(v);
    return v;
}

// harmonics k0 .. k0 + G - 1 of every trial over the cnt photons of the slice in sd, into part (the slice's and the
// orbit's [2m][nf] block)
template <int G, int J, bool TWOD>
__device__ __forceinline__ void os_group(const double (*sd)[kOsSlice], int cnt, const double* __restrict__ freq,
                                         int64_t nf, double c2, int k0, double (*red)[2 * kOsAcc],
                                         double* __restrict__ part) {
    static_assert(G * J <= kOsAcc, "the accumulators of a chunk stay in registers");
    const int tid = threadIdx.x;
    const double kf = (double)k0;
    for (int64_t j0 = 0; j0 < nf; j0 += J) {
        const int jn = (int)(nf - j0 < J ? nf - j0 : J);
        double f[J], C[J][G], S[J][G];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            f[j] = freq[j0 + (j < jn ? j : jn - 1)];
#pragma unroll
            for (int k = 0; k < G; ++k) C[j][k] = S[j][k] = 0.0;
        }
        for (int p = tid; p < cnt; p += kOsBlock) {
            const double d = sd[0][p];
            const double d2 = TWOD ? sd[TWOD ? 1 : 0][p] : 0.0;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (j < jn) {
                    const double ph = TWOD ? fma(f[j], d, c2 * d2) : f[j] * d;
                    double s1 = 0.0, c1 = 1.0, s, c;
                    if (G > 1) sincospi(2.0 * (ph - rint(ph)), &s1, &c1);
                    if (k0 == 1 && G > 1) {
                        s = s1;
                        c = c1;
                    } else {
                        const double pk = ph * kf;
                        sincospi(2.0 * (pk - rint(pk)), &s, &c);
                    }
                    C[j][0] += c;
                    S[j][0] += s;
#pragma unroll
                    for (int k = 1; k < G; ++k) {
                        const double cn = fma(c, c1, -s * s1);
                        const double sn = fma(s, c1, c * s1);
                        c = cn;
                        s = sn;
                        C[j][k] += c;
                        S[j][k] += s;
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (j < jn) {
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const double cr = os_row_sum(C[j][k]), sr = os_row_sum(S[j][k]);
                    if ((tid & 15) == 0) {
                        red[tid >> 4][2 * (j * G + k)] = cr;
                        red[tid >> 4][2 * (j * G + k) + 1] = sr;
                    }
                }
            }
        }
        __syncthreads();
        if (tid < 2 * G * jn) {
            double v = 0.0;
#pragma unroll
            for (int w = 0; w < kOsBlock / 16; ++w) v += red[w][tid];
            const int j = tid / (2 * G), r = tid - j * (2 * G);
            part[(int64_t)(2 * (k0 - 1) + r) * nf + j0 + j] = v;
        }
        __syncthreads();
    }
}

template <int J, bool TWOD>
__global__ __launch_bounds__(kOsBlock) void k_orbit_search(const double* __restrict__ t, int64_t n, const OSArgs A,
                                                           const double* __restrict__ orbits,
                                                           const double* __restrict__ freq, int64_t nf,
                                                           double* __restrict__ part) {
    __shared__ double sraw[kOfFields];
    __shared__ BinModel sB;
    __shared__ double sd[TWOD ? 2 : 1][kOsSlice];
    __shared__ double red[kOsBlock / 16][2 * kOsAcc];
    const int tid = threadIdx.x;
    const int64_t slice = blockIdx.x, o = blockIdx.y, ob = gridDim.y;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < kOfFields; ++k) {
            const int c = A.col[k];
            sraw[k] = c >= 0 ? orbits[o * A.nkeys + c] : A.base.raw[k];
        }
        of_derive(A.base.kind, sraw, &sB, true);  // the host checked the limits
    }
    __syncthreads();
    const BinModel* B = &sB;
    const int64_t i0 = slice * kOsSlice;
    const int cnt = (int)(n - i0 < kOsSlice ? n - i0 : kOsSlice);
    // phase A
    for (int p = tid; p < cnt; p += kOsBlock) {
#pragma clang fp contract(off)
        const double ti = t[i0 + p];
        const double tau = bin_delay(B, ti);
        const double a = (ti - A.tref) * 86400.0;
        const double d = a - tau;
        sd[0][p] = d;
        if (TWOD) sd[TWOD ? 1 : 0][p] = d * d;
    }
    __syncthreads();
    // phase B
    const int m = A.nharm;
    double* pb = part + ((slice * ob + o) * (int64_t)(2 * m)) * nf;
    for (int k0 = 1, G; k0 <= m; k0 += G) {
        G = os_harm_group(m - k0 + 1);
        if (J * 8 <= kOsAcc && G == 8)
            os_group<(J * 8 <= kOsAcc ? 8 : 1), J, TWOD>(sd, cnt, freq, nf, A.c2, k0, red, pb);
        else if (J * 4 <= kOsAcc && G == 4)
            os_group<(J * 4 <= kOsAcc ? 4 : 1), J, TWOD>(sd, cnt, freq, nf, A.c2, k0, red, pb);
        else if (J * 2 <= kOsAcc && G == 2)
            os_group<(J * 2 <= kOsAcc ? 2 : 1), J, TWOD>(sd, cnt, freq, nf, A.c2, k0, red, pb);
        else
            os_group<1, J, TWOD>(sd, cnt, freq, nf, A.c2, k0, red, pb);
    }
}

// part[nslices][ob][2m][nf] -> power[ob][nf] (may be null) and best[ob][2] (may be null); workgroup o = orbit o
__global__ __launch_bounds__(256) void k_orbit_search_finalize(const double* __restrict__ part, int64_t ob,
                                                               int64_t nslices, int64_t nf, int m, int stat, double n,
                                                               double* __restrict__ power, double* __restrict__ best) {
    const int64_t o = blockIdx.x;
    const int ncomp = 2 * m;
    const double w = 2.0 / n;
    BestCand cand = {-INFINITY, INT64_MAX};
    for (int64_t j = threadIdx.x; j < nf; j += blockDim.x) {
        double zsum = 0.0, cum = 0.0, top = -INFINITY;
        for (int k = 0; k < m; ++k) {
            double c = 0.0, s = 0.0;
            for (int64_t sp = 0; sp < nslices; ++sp) {
                const double* q = part + ((sp * ob + o) * ncomp + 2 * k) * nf + j;
                c += q[0];
                s += q[nf];
            }
            const double z = c * c + s * s;
            if (stat == CRIMP_STAT_Z2) {
                zsum += z;
            } else {
                cum += z * w;
                const double v = cum - 4.0 * (double)k;
                top = (v > top || v != v) ? v : top;  // (a NaN stays: an orbit with an unconverged lane reads NaN)
            }
        }
        const double v = (stat == CRIMP_STAT_Z2) ? zsum * w : top;
        if (power) power[o * nf + j] = v;
        if (best_better(v, j, cand.v, cand.i)) cand = {v, j};
    }
    if (best) {
        cand = best_block_reduce(cand);
        if (threadIdx.x == 0) {
            best[2 * o] = cand.v;
            best[2 * o + 1] = (double)cand.i;
        }
    }
}
