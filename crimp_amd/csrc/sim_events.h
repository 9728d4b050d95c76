// sim_events.h -- event simulator: photon arrival times of an inhomogeneous Poisson process whose rate follows a
// pulse profile under a timing model (replaces simulatemodulatedlc.py:19-96 of the reference, a binned sinusoid at
// constant frequency drawn from NumPy's global RNG, and the host generators of crimp_amd/synth.py). Included by
// crimp_hip.hip after cp_one, TplDev / tpl_coef / photon_sincos / tpl_terms and stretch_move.h (tf_philox, tf_uniform);
// the C-ABI (crimp_sim_events) is in its section 6.
//
// The process: on [mjd_start, mjd_start + span_s / 86400), inside the union of the half-open GTIs when given,
//   lambda(t) = S(frac(phi(t))) + b   counts/s,
// phi(t) = cp_one at the event's MJD (the arithmetic of crimp_calcphase), S a template (norm + the template part of
// k_toa_points at phShift) or a table of n rates, one per phase bin [k/n, (k+1)/n).
//
// Layout: time is cut into cells of cell_s seconds anchored at mjd_start, one wave (a 64-thread block) per cell.
// Candidates are a homogeneous process of rate lam_max >= lambda: every lane draws an Exp(1) / lam_max gap, a
// fixed-order inclusive scan over the wave turns 64 gaps into 64 arrival times after the running time, and rounds
// repeat until the running time passes the cell's end (restarting at a cell's start is exact: the process has no
// memory). A candidate at t survives if it lies in a GTI and u * lam_max < lambda(t); with u * lam_max < S it is a
// source event, otherwise a background event. Survivors are compacted in order by the ballot's prefix popcount, so a
// cell's events come out time-sorted and cells follow each other in time: no sort and no Poisson sampler.
//
// Random numbers: Philox4x32-10, key = seed, counter = (cell lo, cell hi, round, lane); one call gives the gap's
// uniform (53 bits) and the acceptance uniform. A cell's events depend on (seed, inputs, cell_s, cell index) alone:
// not on the grid, on which cells a call covers or on what else is in the launch.
//
// Two passes over the same counter streams: k_sim_cells<false> counts the survivors of every cell, a two-level int64
// exclusive scan (k_sim_tile_sums, k_sim_scan_top, k_sim_scan_apply) over the counts and one trailing zero turns them
// into offsets and the total, and k_sim_cells<true> regenerates the cells and stores times and the optional
// background mask at offset + rank. Plain vector stores; no atomics.
#pragma once

constexpr int kSimLdsSteps = 512;   // a step table of at most this many rates is copied to LDS by every wave
constexpr int kSimScanBlock = 256;  // threads of the scan kernels
constexpr int kSimScanItems = 4;    // cells per thread
constexpr int kSimScanTile = kSimScanBlock * kSimScanItems;

struct SimArgs {
    int32_t kind, n_steps;  // CRIMP_SIM_TEMPLATE | CRIMP_SIM_STEPS
    TplDev T;
    double norm, ph_shift, bkg;
    double lam_max, inv_lam;
    double mjd_start, span_s, cell_s, out_offset_s;
    int64_t first_cell, ngti;
    uint64_t seed;
    int32_t days;
};
static_assert(sizeof(CPArgs<true>) + sizeof(SimArgs) + 64 <= 4096,
              "the timing model and the shape ride in the kernel arguments (4 KB limit)");

// mjd inside some [start, stop) of the sorted, disjoint GTIs
__device__ __forceinline__ bool sim_in_gti(const double* __restrict__ gti, int64_t ngti, double mjd) {
    int64_t a = 0, b = ngti;  // first interval whose stop is past mjd
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (gti[2 * m + 1] <= mjd) a = m + 1; else b = m;
    }
    return a < ngti && gti[2 * a] <= mjd;
}

// One block of 64 threads (one wave) per cell. FILL = false: cnt[cell] = survivors; FILL = true: the same cell again,
// times to t_out[off[cell] + rank], background flags to bkg_out (may be NULL); off has one entry more than there are
// cells (the total).
// BIN: the rate follows the template at the phase of the emission time (the orbit stays in the kernel arguments).
template <bool FILL, bool BIN>
__global__ __launch_bounds__(64) void k_sim_cells(const CPArgs<BIN> Mv, const SimArgs A, const double* __restrict__ steps,
                                                  const double* __restrict__ gti, int64_t* __restrict__ cnt,
                                                  const int64_t* __restrict__ off, double* __restrict__ t_out,
                                                  uint8_t* __restrict__ bkg_out) {
    __shared__ double coef[2][CRIMP_MAX_COMP];
    __shared__ double tab[kSimLdsSteps];
    // the model arrives in the kernel arguments (no upload) and is read from LDS: 14 VGPRs fewer than reading it
    // from the arguments, and a third wave per SIMD for the fill pass
    __shared__ CPModel Ms;
    static_assert(sizeof(CPModel) % sizeof(double) == 0, "CPModel is copied to LDS in 8-byte words");
    const int lane = threadIdx.x;
    {
        const char* src = reinterpret_cast<const char*>(&Mv.m);
        char* dst = reinterpret_cast<char*>(&Ms);
        for (int i = lane; i < (int)(sizeof(CPModel) / sizeof(double)); i += 64)
            __builtin_memcpy(dst + 8 * i, src + 8 * i, 8);
    }
    const CPModel* M = &Ms;
    const int64_t rel = blockIdx.x;
    const uint64_t cell = (uint64_t)(A.first_cell + rel);
    const bool tpl = A.kind == CRIMP_SIM_TEMPLATE;
    const bool lds_steps = !tpl && A.n_steps <= kSimLdsSteps;
    if (tpl) {
        if (lane < A.T.K) tpl_coef(&A.T, lane, A.ph_shift, coef[0][lane], coef[1][lane]);
    } else if (lds_steps) {
        for (int i = lane; i < A.n_steps; i += 64) tab[i] = steps[i];
    }
    __syncthreads();
    const double start = (double)cell * A.cell_s;
    const double end = fmin((double)(cell + 1) * A.cell_s, A.span_s);  // the next cell's start, or the span's end
    // a cell no GTI touches has no survivors: skip its candidates (the same result as rejecting each of them)
    bool dead = false;
    if (A.ngti > 0) {
        const double lo = A.mjd_start + start / 86400.0, hi = A.mjd_start + end / 86400.0;
        int64_t a = 0, b = A.ngti;
        while (a < b) {
            const int64_t m = (a + b) >> 1;
            if (gti[2 * m + 1] <= lo) a = m + 1; else b = m;
        }
        dead = a >= A.ngti || gti[2 * a] > hi;
    }
    int64_t n_acc = 0;
    const int64_t o = FILL ? off[rel] : 0;
    const int64_t o_end = FILL ? off[rel + 1] : 0;  // the fill pass never stores past the cell's counted share
    double base = 0.0;
    for (uint32_t round = 0; !dead; ++round) {
        uint32_t r[4];
        tf_philox((uint32_t)cell, (uint32_t)(cell >> 32), round, (uint32_t)lane, A.seed, r);
        double x = -log(tf_uniform(r[0], r[1])) * A.inv_lam;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {  // inclusive scan, the same order in every launch
            const double y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        const double offs = base + x;
        const double s = start + offs;
        bool ok = false, isb = false;
        if (s < end) {
            const double mjd = A.mjd_start + s / 86400.0;
            if (A.ngti == 0 || sim_in_gti(gti, A.ngti, mjd)) {
                const double ph = cp_args_one<BIN>(M, Mv, mjd);
                const double fr = ph - floor(ph);
                double S;
                if (tpl) {
                    double s1, c1, h, h1, h2;
                    photon_sincos(A.T.model, A.T.model == CRIMP_MODEL_FOURIER ? fr : fr * 6.283185307179586476925, s1,
                                  c1);
                    tpl_terms(&A.T, A.T.model, A.T.K, coef[0], coef[1], s1, c1, h, h1, h2);
                    S = A.norm + h;
                } else {
                    int k = (int)(fr * (double)A.n_steps);
                    k = k < A.n_steps ? k : A.n_steps - 1;  // frac = 1 after rounding
                    k = k > 0 ? k : 0;                      // (a NaN phase)
                    S = lds_steps ? tab[k] : steps[k];
                }
                const double v = tf_uniform(r[2], r[3]) * A.lam_max;
                ok = v < S + A.bkg;
                isb = !(v < S);
            }
        }
        const unsigned long long mask = __ballot(ok);
        const int64_t at = o + n_acc + __popcll(mask & ((1ull << lane) - 1ull));
        if (FILL && ok && at < o_end) {
            t_out[at] = A.days ? A.mjd_start + s / 86400.0 : A.out_offset_s + s;
            if (bkg_out) bkg_out[at] = isb ? 1 : 0;
        }
        n_acc += __popcll(mask);
        base = __shfl(offs, 63);
        if (!(start + base < end)) break;  // the same value in every lane
    }
    if (!FILL && lane == 0) cnt[rel] = n_acc;
}

// exclusive scan of one value per thread over a block of kSimScanBlock threads; *total = the block's sum
__device__ __forceinline__ int64_t sim_block_scan(int64_t v, int64_t* sh, int64_t* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < kSimScanBlock; d <<= 1) {
        const int64_t a = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += a;
        __syncthreads();
    }
    *total = sh[kSimScanBlock - 1];
    const int64_t ex = sh[tid] - v;
    __syncthreads();
    return ex;
}

// level 1: sums[tile] = the sum of the tile's counts
__global__ __launch_bounds__(kSimScanBlock) void k_sim_tile_sums(const int64_t* __restrict__ cnt, int64_t n,
                                                                 int64_t* __restrict__ sums) {
    __shared__ int64_t sh[kSimScanBlock];
    const int64_t i0 = (int64_t)blockIdx.x * kSimScanTile + (int64_t)threadIdx.x * kSimScanItems;
    int64_t v = 0;
#pragma unroll
    for (int q = 0; q < kSimScanItems; ++q)
        if (i0 + q < n) v += cnt[i0 + q];
    int64_t total;
    (void)sim_block_scan(v, sh, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// level 2 (one block): sums -> their exclusive scan in place
__global__ __launch_bounds__(kSimScanBlock) void k_sim_scan_top(int64_t* __restrict__ sums, int64_t nb) {
    __shared__ int64_t sh[kSimScanBlock];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += kSimScanBlock) {
        const int64_t i = b0 + threadIdx.x;
        const int64_t v = i < nb ? sums[i] : 0;
        int64_t total;
        const int64_t ex = sim_block_scan(v, sh, &total);
        if (i < nb) sums[i] = carry + ex;
        carry += total;
    }
}

// counts -> offsets in place: the tile's offset plus the exclusive scan inside the tile
__global__ __launch_bounds__(kSimScanBlock) void k_sim_scan_apply(int64_t* cnt, int64_t n,
                                                                  const int64_t* __restrict__ sums) {
    __shared__ int64_t sh[kSimScanBlock];
    const int64_t i0 = (int64_t)blockIdx.x * kSimScanTile + (int64_t)threadIdx.x * kSimScanItems;
    int64_t c[kSimScanItems];
    int64_t v = 0;
#pragma unroll
    for (int q = 0; q < kSimScanItems; ++q) {
        c[q] = i0 + q < n ? cnt[i0 + q] : 0;
        v += c[q];
    }
    int64_t total;
    int64_t run = sums[blockIdx.x] + sim_block_scan(v, sh, &total);
#pragma unroll
    for (int q = 0; q < kSimScanItems; ++q) {
        if (i0 + q < n) cnt[i0 + q] = run;
        run += c[q];
    }
}
