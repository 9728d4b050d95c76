// phase_cube.h -- fold-and-bin in one pass: the (y, z, phase) count cube behind the pulse-profile maps of plot_pps.py
// (phase-energy :139-152, phase-time :204-215, the time x energy grid of profiles :288-333, before / after :447-479).
// Included by crimp_hip.hip after section 3 (CPModel, cp_one) and the runtime helpers.
//
// Every photon is placed on three axes by exact comparisons against the edges the host passes (np.histogramdd with
// explicit edges: bin = searchsorted(edges, v, 'right') - 1, the last edge closed unless the axis is OPEN_LAST, NaN and
// values outside dropped) and counted into cell iy * S + zoff[iz] + b. The phase is x itself, or -- with a timing
// model -- calcphase's folded value of the time x, formed by the same cp_one and the same tot - floor(tot) as
// k_calcphase_vec, so that a fused call counts exactly what crimp_calcphase followed by an unfused call counts.
//
// Two lookups, both exact. An axis whose edges the host found near-uniform (cube_axis_uniform: numpy.linspace's are)
// takes k_binphases' form: the estimate (v - first) * nb / (last - first), then one step down or up against the two
// edges beside it -- two independent LDS reads. Any other axis (log-spaced energies) takes a binary search of
// ceil(log2(nb + 1)) steps. A thread bins its four photons of a sweep side by side and without branches, so that their
// LDS round trips overlap; the first form, one after the other with early exits, ran 0.54 ms per 1e8 photons without
// the fold, almost all of it LDS latency.
//
// Counting: u32 cells in LDS, R copies of the cube per block (R a power of two, as many as fit kCubeLdsCells, at most
// one per thread), thread tid adds to copy tid & (R - 1). Time-sorted photons put a whole wave into one time row and a
// small cube has few cells anyway, so one copy per block (or per wave) would serialise the lanes of one ds_add on the
// same address; the copies spread them, and the odd copy stride puts the same cell of neighbouring copies on different
// banks. Each block adds its non-zero cells to the zeroed int64 cube once. Integer sums: no split over blocks and no
// atomic order can change a count. A cube of more than CRIMP_CUBE_LDS_BINS cells is counted with global 64-bit atomics.
#pragma once

constexpr int kCubeBlock = 256;
constexpr int kCubeLdsCells = CRIMP_CUBE_LDS_BINS + 1;  // + 1: the copy stride is the cell count made odd
constexpr int kCubeMaxBlocks = 2048;                    // about 8 blocks per CU, grid-stride beyond
constexpr int kCubeK = 4;                               // photons a thread bins side by side

struct CubeDims {
    int32_t ny, nz;        // bins of the y and z axes (1 for an absent axis)
    int32_t has_y, has_z;  // the axis has values and edges (has_y also with y_is_x)
    int32_t y_is_x;        // y = x: the time axis of a fused phase-time map, read once
    int32_t S;             // phase bins of all z columns together = zoff[nz]
    int32_t cells;         // ny * S
    int32_t nph_edges;     // S + nz
    int32_t stride, R;     // LDS copies: R cubes of `stride` u32 cells (R = 0: global atomics)
    int32_t open_y, open_z, open_p;
    int32_t fused;         // x holds MJD times, folded with the model
    int32_t uni_y, uni_z, uni_p;     // the axis takes the estimate-and-step lookup (uni_p: every column does)
    int32_t it_y, it_z, it_p;        // binary-search steps otherwise: ceil(log2(nb + 1)), the largest column's for it_p
    double sc_y, sc_z;     // nb / (last - first) of the y and z axes
};

// dynamic LDS of k_phase_cube: [y edges | z edges | phase edges | per-column nb / (last - first)] doubles,
// zoff[nz + 1] ints, then the R * stride cells
static size_t cube_lds_bytes(const CubeDims& D) {
    const size_t nd = (size_t)(D.has_y ? D.ny + 1 : 0) + (size_t)(D.has_z ? D.nz + 1 : 0) + (size_t)D.nph_edges +
                      (size_t)D.nz;
    return nd * sizeof(double) + (size_t)(D.nz + 1) * sizeof(int32_t) + (size_t)D.R * D.stride * sizeof(uint32_t);
}
static_assert((size_t)(2 * (CRIMP_CUBE_MAX_BINS + 1) + CRIMP_CUBE_MAX_PH_EDGES + CRIMP_CUBE_MAX_BINS) * 8 +
                      (size_t)(CRIMP_CUBE_MAX_BINS + 1) * 4 + (size_t)kCubeLdsCells * 4 <= 65536,
              "k_phase_cube's edge tables and cells must fit 64 KB of LDS");

static double cube_axis_scale(const double* e, int nb) { return (double)nb / (e[nb] - e[0]); }

// The estimate of a value's bin, as the device forms it (host and device: one subtraction, one product, no contraction
// possible between them).
__host__ __device__ __forceinline__ int cube_estimate(double v, double first, double scale, int nb) {
    const int idx = (int)((v - first) * scale);
    return idx < nb ? (idx < 0 ? 0 : idx) : nb - 1;
}

// True when one step from the estimate always reaches the bin: the estimate of every edge e[i] is i - 1 or i (the last
// edge's nb - 1). The estimate does not decrease with v, so for e[i] <= v < e[i + 1] it lies in [i - 1, i + 1].
static bool cube_axis_uniform(const double* e, int nb) {
    const double scale = cube_axis_scale(e, nb);
    if (!std::isfinite(scale) || !(scale > 0.0)) return false;
    for (int i = 0; i <= nb; ++i) {
        const int est = cube_estimate(e[i], e[0], scale, nb);
        if (est > i || est < i - 1) return false;
    }
    return true;
}

static int cube_search_steps(int nb) {
    int it = 0;
    while ((1 << it) < nb + 1) ++it;
    return it;
}

// Bins of K values on one axis, side by side: idx[k] = largest i with e[i] <= v[k] (np.searchsorted(e, v, 'right') - 1),
// a value on the last edge in the last bin; ok[k] cleared for a value outside [e[0], e[nb]], a NaN, or -- open_last --
// a value on the last edge. e, nb, scale may differ per k (the phase axis: the photon's z column).
template <int K>
__device__ __forceinline__ void cube_bins(const double* (&e)[K], const int (&nb)[K], const double (&scale)[K],
                                          const double (&first)[K], const double (&last)[K], bool uniform, int iters,
                                          bool open_last, const double (&v)[K], int (&idx)[K], bool (&ok)[K]) {
    double w[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const bool in = v[k] >= first[k] && v[k] <= last[k];  // a NaN fails both
        ok[k] = ok[k] && in && !(open_last && v[k] == last[k]);
        w[k] = in ? v[k] : first[k];
    }
    if (uniform) {
        double a[K], b[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            idx[k] = cube_estimate(w[k], first[k], scale[k], nb[k]);
            a[k] = e[k][idx[k]];
            b[k] = e[k][idx[k] + 1];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int down = w[k] < a[k] ? 1 : 0;
            const int up = (idx[k] != nb[k] - 1 && w[k] >= b[k]) ? 1 : 0;
            idx[k] += up - down;  // (never both: a < b)
        }
    } else {
        int lo[K], hi[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            lo[k] = 0;
            hi[k] = nb[k];
        }
        for (int it = 0; it < iters; ++it) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int mid = (lo[k] + hi[k] + 1) >> 1;  // lo == hi: mid = lo, e[lo] <= w holds, nothing moves
                const bool le = e[k][mid] <= w[k];
                lo[k] = le ? mid : lo[k];
                hi[k] = le ? hi[k] : mid - 1;
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) idx[k] = lo[k] < nb[k] ? lo[k] : nb[k] - 1;
    }
}

// Two photons per thread and sweep with 16-byte loads (VEC: every array 16-byte aligned; the odd last photon is
// counted by one thread), two sweeps' loads issued together and their four photons binned side by side (a photon that
// is not there is a NaN, which every axis drops); a grid of at most kCubeMaxBlocks blocks strides over the list, so
// that the per-block set-up (edges into LDS, cells zeroed) and merge are paid a few thousand times.
// MAP: the shape of a profile or a phase-time map, fixed at compile time -- no z axis, near-uniform y (if any) and
// phase edges, LDS counting -- so that its loop carries neither the binary searches nor the column and atomic
// choices (the kernel is bound by its instruction count: 0.444 ms for the fused 32 x 12 map in the general form).
// BIN: the model carries a binary orbit and the fused phase is the one at the emission time (crimp_calcphase's
// parts 7 | 8); BIN = false is the kernel of a build without orbits.
template <bool VEC, bool MAP, bool BIN>
__global__ __launch_bounds__(kCubeBlock) void k_phase_cube(const double* __restrict__ x, const double* __restrict__ y,
                                                           const double* __restrict__ z, int64_t n,
                                                           const CPArgs<BIN> Mv,
                                                           const double* __restrict__ tables,
                                                           const int32_t* __restrict__ zoff_g, const CubeDims D,
                                                           unsigned long long* __restrict__ counts) {
    extern __shared__ double cube_sm[];
    constexpr int K = kCubeK;
    const CPModel* M = &Mv.m;
    const int tid = threadIdx.x;
    const bool has_z = MAP ? false : D.has_z != 0, lds = MAP ? true : D.R != 0;
    const bool uni_y = MAP ? true : D.uni_y != 0, uni_p = MAP ? true : D.uni_p != 0;
    const int nye = D.has_y ? D.ny + 1 : 0, nze = has_z ? D.nz + 1 : 0;
    double* ye = cube_sm;
    double* ze = ye + nye;
    double* pe = ze + nze;
    double* psc = pe + D.nph_edges;
    int32_t* zoff = reinterpret_cast<int32_t*>(psc + D.nz);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(zoff + D.nz + 1);
    const int ntab = nye + nze + D.nph_edges + D.nz;
    for (int i = tid; i < ntab; i += kCubeBlock) cube_sm[i] = tables[i];
    for (int i = tid; i <= D.nz; i += kCubeBlock) zoff[i] = zoff_g[i];
    for (int i = tid; i < D.R * D.stride; i += kCubeBlock) cnt[i] = 0;
    __syncthreads();
    uint32_t* mine = cnt + (size_t)(tid & (D.R - 1)) * D.stride;  // (R = 0: unused)
    const double yfirst = D.has_y ? ye[0] : 0.0, ylast = D.has_y ? ye[D.ny] : 0.0;
    const double zfirst = has_z ? ze[0] : 0.0, zlast = has_z ? ze[D.nz] : 0.0;
    const double pfirst0 = pe[0], plast0 = pe[zoff[1]], psc0 = psc[0];  // column 0: the only one without a z axis
    const int pnb0 = zoff[1];
    const double qnan = __builtin_nan("");

    auto count = [&](const double (&xv)[K], const double (&yv)[K], const double (&zv)[K]) {
        bool ok[K];
        int iy[K], iz[K], b[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            ok[k] = true;
            iy[k] = 0;
            iz[k] = 0;
        }
        if (D.has_y) {
            const double* e[K];
            int nb[K];
            double sc[K], fi[K], la[K];
#pragma unroll
            for (int k = 0; k < K; ++k) e[k] = ye, nb[k] = D.ny, sc[k] = D.sc_y, fi[k] = yfirst, la[k] = ylast;
            cube_bins<K>(e, nb, sc, fi, la, uni_y, D.it_y, D.open_y, yv, iy, ok);
        }
        if (has_z) {
            const double* e[K];
            int nb[K];
            double sc[K], fi[K], la[K];
#pragma unroll
            for (int k = 0; k < K; ++k) e[k] = ze, nb[k] = D.nz, sc[k] = D.sc_z, fi[k] = zfirst, la[k] = zlast;
            cube_bins<K>(e, nb, sc, fi, la, D.uni_z, D.it_z, D.open_z, zv, iz, ok);
        }
        double ph[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            ph[k] = xv[k];
            if (D.fused) {
                const double tot = cp_args_one<BIN>(M, Mv, xv[k]);
                ph[k] = tot - floor(tot);  // k_calcphase_vec's folded value
            }
        }
        int o[K];
        {
            const double* e[K];
            int nb[K];
            double sc[K], fi[K], la[K];
#pragma unroll
            for (int k = 0; k < K; ++k) e[k] = pe, nb[k] = pnb0, sc[k] = psc0, fi[k] = pfirst0, la[k] = plast0, o[k] = 0;
            if (has_z) {
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    o[k] = zoff[iz[k]];
                    nb[k] = zoff[iz[k] + 1] - o[k];
                    e[k] = pe + o[k] + iz[k];
                    sc[k] = psc[iz[k]];
                }
#pragma unroll
                for (int k = 0; k < K; ++k) fi[k] = e[k][0], la[k] = e[k][nb[k]];
            }
            cube_bins<K>(e, nb, sc, fi, la, uni_p, D.it_p, D.open_p, ph, b, ok);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (ok[k]) {
                const int cell = iy[k] * D.S + o[k] + b[k];
                if (lds)
                    atomicAdd(&mine[cell], 1u);
                else
                    atomicAdd(&counts[cell], 1ull);
            }
        }
    };
    const int64_t stride = (int64_t)gridDim.x * kCubeBlock;
    if (VEC) {
        const double2* x2 = reinterpret_cast<const double2*>(x);
        const double2* y2 = reinterpret_cast<const double2*>(y);
        const double2* z2 = reinterpret_cast<const double2*>(z);
        const int64_t npair = n / 2;
        const double2 none = make_double2(qnan, qnan);
        for (int64_t i = (int64_t)blockIdx.x * kCubeBlock + tid; i < npair; i += 2 * stride) {
            const int64_t j = i + stride;
            const bool two = j < npair;
            const double2 xa = x2[i], xb = two ? x2[j] : none;
            const double2 ya = D.y_is_x ? xa : (y2 ? y2[i] : none), yb = D.y_is_x ? xb : (y2 && two ? y2[j] : none);
            const double2 za = z2 ? z2[i] : none, zb = z2 && two ? z2[j] : none;
            const double xv[K] = {xa.x, xa.y, xb.x, xb.y}, yv[K] = {ya.x, ya.y, yb.x, yb.y};
            const double zv[K] = {za.x, za.y, zb.x, zb.y};
            count(xv, yv, zv);
        }
        if ((n & 1) && blockIdx.x == 0 && tid == 0) {
            const double xl = x[n - 1];
            const double xv[K] = {xl, qnan, qnan, qnan};
            const double yv[K] = {D.y_is_x ? xl : (y ? y[n - 1] : qnan), qnan, qnan, qnan};
            const double zv[K] = {z ? z[n - 1] : qnan, qnan, qnan, qnan};
            count(xv, yv, zv);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * kCubeBlock + tid; i < n; i += K * stride) {
            double xv[K], yv[K], zv[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int64_t j = i + k * stride;
                const bool in = j < n;
                xv[k] = in ? x[j] : qnan;
                yv[k] = D.y_is_x ? xv[k] : (y && in ? y[j] : qnan);
                zv[k] = z && in ? z[j] : qnan;
            }
            count(xv, yv, zv);
        }
    }
    if (lds) {
        __syncthreads();
        for (int c = tid; c < D.cells; c += kCubeBlock) {
            unsigned long long sum = 0;
            for (int r = 0; r < D.R; ++r) sum += cnt[(size_t)r * D.stride + c];
            if (sum) atomicAdd(&counts[c], sum);
        }
    }
}

// the LDS copies of a cube of `cells` cells: (stride, R), R = 0 above CRIMP_CUBE_LDS_BINS
static void cube_copies(int cells, int32_t* stride, int32_t* R) {
    *stride = cells | 1;
    *R = 0;
    if (cells > CRIMP_CUBE_LDS_BINS) return;
    int r = 1;
    while (2 * r <= kCubeBlock && (int64_t)(2 * r) * *stride <= kCubeLdsCells) r *= 2;
    *R = r;
}

// k_phase_cube's MAP form applies
static bool cube_is_map(const CubeDims& D) {
    return !D.has_z && D.uni_p && (!D.has_y || D.uni_y) && D.R > 0;
}
