/*
 * crimp_hip.h -- C-ABI of the MI355X-native CRIMP photon hot path (libcrimp_hip.so).
 *
 * The reference (georgeyounes/CRIMP v2.3.0) is pure Python with no FFI; its
 * "operator API" is the Python functions listed per entry point below. Each entry
 * point replaces the NumPy inner loops of one of them; the Python drop-ins in
 * crimp_amd/ keep the reference signatures and call these through ctypes.
 *
 * Conventions (all entry points):
 *   - return 0 (CRIMP_OK) or a negative status; crimp_last_error() gives the text
 *     (thread-local, valid until the next call on the same thread);
 *   - every buffer is caller-owned; with CRIMP_FLAG_DEVICE_PTRS all array
 *     arguments are device pointers on the current HIP device, otherwise they are
 *     host pointers and the library stages them through device memory itself;
 *   - `stream` is a hipStream_t (NULL = the null stream); kernels are queued on it
 *     and every call returns with that stream drained (host staging copies are
 *     blocking), so results are ready on return -- CRIMP_FLAG_SYNC is accepted and
 *     implied;
 *   - calls are serialised process-wide, all devices together (one internal mutex:
 *     the scratch pool and the measurement hooks are shared); the ctypes layer
 *     releases the GIL around them, so threads driving different devices queue.
 */
#ifndef CRIMP_HIP_H
#define CRIMP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRIMP_OK 0
#define CRIMP_ERR_ARG (-1)
#define CRIMP_ERR_HIP (-2)
#define CRIMP_ERR_NODEV (-3)

#define CRIMP_FLAG_DEVICE_PTRS 1u  /* array arguments are device pointers */
#define CRIMP_FLAG_SYNC 2u         /* synchronise the stream before returning */
/* Periodicity-search precision. Default: the NUFFT (search_nufft.h) on arithmetic-progression grids (ascending)
 * of >= 64 trials per row segment with time-sorted photons and a plan in range -- every trial certified within 1e-6
 * relative by a truncation bound, the uncertified ones recomputed in fp64 (crimp_last_fixups()). Where the NUFFT
 * declines: the exact i8-MFMA kernel on progressions of >= 256 trials (per-term error ~1e-9, integer sums; trials
 * whose 10-sigma bound cannot place them within 1e-6 relative are recomputed in fp64), the fp64 kernel otherwise.
 * crimp_last_search_path() says which ran. Tested within 1e-6 of the reference on every checked trial; the
 * reference's own fp64 argument rounding (~1e-6 of a noise-level H_20) is the floor of any fp64 implementation
 * (DESIGN.md section 8). */
#define CRIMP_FLAG_FORCE_MFMA 8u   /* search: fail unless a factorised kernel (NUFFT, or exact i8 MFMA at any row
                                    * length) applies */
#define CRIMP_FLAG_TIME_KERNELS 128u /* search / calcphase: time the kernels with hipEvents (crimp_last_kernel_ms) */
#define CRIMP_FLAG_F64 256u         /* search: fp64 kernel on every grid */
#define CRIMP_FLAG_NO_FIXUP 1024u   /* search (diagnostic): the exact kernel's / the NUFFT's raw powers, without the
                                       fp64 fix-up of the trials their error bound cannot certify (crimp_last_fixups
                                       counts them) */
/* Bits 4, 16 and 512 selected the fp32 "fast" search (round 1-4), retired in round 5: slower than the default exact
 * path and only within 1e-6 of the grid's mean power. A search call that sets any of them fails with CRIMP_ERR_ARG. */
#define CRIMP_FLAG_RETIRED_FAST (4u | 16u | 512u)
#define CRIMP_FLAG_ASYNC 2048u     /* crimp_search_sets with device pointers: return once the kernel is queued, without
                                     * draining the stream (the caller synchronises it before reading out) */

#define CRIMP_FLAG_NUFFT 4096u     /* search: the default routing, asked for explicitly (the NUFFT wherever it applies,
                                    * the exact rule otherwise); kept for callers of rounds 5 and earlier */
#define CRIMP_FLAG_EXACT 8192u     /* search: no NUFFT -- the exact i8-MFMA kernel on progressions of >= 256 trials,
                                    * the fp64 kernel otherwise (the default of rounds 1-5) */

#define CRIMP_FLAG_TIME_DAYS 16384u    /* crimp_search_sets: t in days (MJD); the kernel forms t * 86400 seconds as
                                        * measureToAs.py:211 does on the host (the same fp64 multiply) */
#define CRIMP_FLAG_FOLD_RADIANS 32768u /* crimp_calcphase: the folded phase times 2 pi (radians), the host's
                                        * `folded * (2 * np.pi)` of measureToAs.py:195, :200 in the same multiply */

#define CRIMP_STAT_Z2 0 /* Z^2_m  (periodsearch.py:57-71, :73-106) */
#define CRIMP_STAT_H 1  /* H-test (periodsearch.py:109-125)         */

#define CRIMP_MODEL_FOURIER 0  /* templatemodels.py:24-121, x in cycles  */
#define CRIMP_MODEL_CAUCHY 1   /* templatemodels.py:124-226, x in rad    */
#define CRIMP_MODEL_VONMISES 2 /* templatemodels.py:229-329, x in rad    */

#define CRIMP_MAX_GLITCH 32
#define CRIMP_MAX_WAVE 64
#define CRIMP_MAX_COMP 16

#define CRIMP_BINARY_NONE 0
#define CRIMP_BINARY_BT 1    /* Blandford & Teukolsky 1976 */
#define CRIMP_BINARY_ELL1 2  /* Lange et al. 2001 */
#define CRIMP_PART_EMISSION 8 /* crimp_calcphase parts bit 3: the requested parts at the emission time of a binary model */

/* Values of a .par timing model as calcphase consumes them
 * (readtimingmodel.py:212-233; calcphase.py:73-149). */
typedef struct crimp_timing_model {
    double pepoch;                          /* PEPOCH (MJD) */
    double f[13];                           /* F0..F12; absent ones 0 */
    int32_t n_glitch;                       /* glitches 1..n (count of GLEP_ keys, calcphase.py:94) */
    double glitch[CRIMP_MAX_GLITCH][7];     /* GLEP, GLPH, GLF0, GLF1, GLF2, GLF0D, GLTD */
    int32_t n_wave;                         /* WAVE harmonics used = (#WAVE* keys) - 2 (calcphase.py:142) */
    double wave_epoch, wave_om;             /* WAVEEPOCH (MJD), WAVE_OM (rad/day) */
    double wave_ab[CRIMP_MAX_WAVE][2];      /* WAVEj A, B */
    /* The binary orbit (not in the reference). A zero-filled tail is "no binary". Angles as in the .par. */
    int32_t binary;                         /* CRIMP_BINARY_NONE | _BT | _ELL1 */
    double bin_pb;                          /* PB (days) */
    double bin_pbdot, bin_a1dot;            /* PBDOT, A1DOT|XDOT, dimensionless (the 1e-12 unit convention applied) */
    double bin_a1;                          /* A1 (light-seconds) */
    double bin_t0;                          /* T0 (BT) or TASC (ELL1), MJD */
    double bin_ecc, bin_om, bin_omdot;      /* BT: ECC, OM (deg), OMDOT (deg/yr of 365.25 d) */
    double bin_gamma;                       /* BT: GAMMA (s) */
    double bin_eps1, bin_eps2;              /* ELL1: EPS1, EPS2 */
} crimp_timing_model;

/* A pulse-profile template (readPPtemplate.py:15-166) with its fixed shape. */
typedef struct crimp_template {
    int32_t model;                   /* CRIMP_MODEL_* */
    int32_t ncomp;                   /* harmonics / components, 1..CRIMP_MAX_COMP */
    double amp[CRIMP_MAX_COMP];      /* amp_j */
    double loc[CRIMP_MAX_COMP];      /* ph_j (fourier) or cen_j (cauchy, vonmises) */
    double wid[CRIMP_MAX_COMP];      /* wid_j (cauchy, vonmises) */
    double i0[CRIMP_MAX_COMP];       /* scipy.special.i0(1/wid_j^2) (vonmises) */
    double amp_shift;                /* ampShift (1 unless varied) */
} crimp_template;

/* Library identification. */
int crimp_version(void);
const char* crimp_last_error(void);
/* Duration (ms, hipEvents on the call's stream) of the harmonic-sum kernels of the last crimp_search, or of
 * the kernel of the last crimp_calcphase, made with CRIMP_FLAG_TIME_KERNELS; -1 if none. Measurement hook for
 * bench.py, not in the reference. */
double crimp_last_kernel_ms(void);
/* All timed spans of the last call made with CRIMP_FLAG_TIME_KERNELS (ms, in order: crimp_search -> the
 * harmonic-sum kernels; crimp_calcphase -> the kernel; crimp_toa_fit -> the brute grid, the fit kernel); writes
 * up to cap values, returns how many there are. Measurement hook for bench.py, not in the reference. */
int crimp_last_kernel_times(double* ms, int32_t cap);
/* Trials of the last crimp_search (default precision) whose power was recomputed by the fp64 fix-up. */
int64_t crimp_last_fixups(void);
/* Kernel family of the last crimp_search: 0 fp64 direct, 1 exact i8 MFMA, 2 NUFFT. With
 * CRIMP_FLAG_TIME_KERNELS a NUFFT search's crimp_last_kernel_times are: the whole pipeline, then the summed ms of its
 * seven kernel classes (cell starts, spread, merge, FFT pass 1, FFT pass 2, separate moment sum, finalize), then their
 * launch counts. The separate moment sum's kernel is removed (pass 2 always forms the sum): its slot stays, so that the
 * layout does not change, and reports 0. Measurement hook for tests and bench.py, not in the reference. */
int crimp_last_search_path(void);
/* The plan of the last NUFFT search: its (largest) FFT length n, moments P, and spread form (1 = cell gather, one lane
 * per wrapped cell on the VALU; 0 = MFMA slots). Measurement hook for bench.py, not in the reference. */
int crimp_last_nufft_plan(int64_t* fft_length, int32_t* moments, int32_t* gather);
/* The last NUFFT search's algorithmic work, up to cap of: [0] the spread's fp64 flops, then HBM bytes of [1] the
 * spread, [2] merge, [3] FFT pass 1, [4] FFT pass 2 (with the moment sum), [5] the removed separate moment sum (always
 * 0, kept for the layout), [6] finalize; returns 7. For bench.py's rooflines, not in the reference. */
int crimp_last_nufft_work(double* work, int32_t cap);
/* Cell-start tables (one per row group and harmonic of a cell-gather plan) the last NUFFT search built with
 * k_nu_cellstart / took from the plan cache (a repeated search over the same buffers: its gathers check them against
 * the photons). Both 0 for an MFMA-slot plan. Measurement hook for tests and bench.py, not in the reference. */
int crimp_last_nufft_cells(int64_t* built, int64_t* reused);
/* Brute-grid norms evaluated per phShift by the last crimp_toa_fit with CRIMP_TOA_BRUTE (the pruned candidates of
 * lmfit's 20-norm lattice, padded to 2, 4 or 20, less the lazy norms the eight-factor grid leaves out; 0 without a
 * brute grid). Measurement hook for bench.py's
 * algorithmic work count, not in the reference. */
int64_t crimp_last_toa_grid_norms(void);
/* The form of the last crimp_toa_fit's brute grid (Fourier templates): bit 0 -- no per-phShift min of the template
 * part (the template's bound certified every candidate lattice point valid), bit 1 -- log2 of products of eight model
 * values instead of four (every factor certified inside [2^-15, 2^15]); 0 = the full kernel. Measurement hook for
 * bench.py, not in the reference. */
int64_t crimp_last_toa_grid_fast(void);
/* Frees the library's idle cached device scratch on every device (not in the reference). */
int crimp_release_scratch(void);
int crimp_device_count(int32_t* count);

/* calcphase(timeMJD, timMod) -> (total, folded)   [calcphase.py:152-176]
 * parts: bit0 Taylor expansion (:73-85), bit1 glitches (:87-126), bit2 waves (:128-149);
 * 7 = calcphase(). folded may be NULL. n == 0 succeeds without touching anything, and t_mjd and total may then be
 * NULL as well (the data pointer of an empty array). A NaN time gives NaN in total and folded whenever bit0 is set,
 * with every F term zero too (the reference's 0 * NaN).
 * parts bit 3 (CRIMP_PART_EMISSION): with a model whose ``binary`` is set, every requested part is evaluated at the
 * emission time t - tau / 86400, tau the orbital delay of crimp_binary_delay, which enters each part in seconds after
 * the epoch difference; the glitch masks are taken at the emission time. Without the bit, or without a
 * binary, the call is the one above, bit for bit. A model with a binary outside the limits of crimp_binary_delay is
 * CRIMP_ERR_ARG whatever the parts. */
int crimp_calcphase(const double* t_mjd, int64_t n, const crimp_timing_model* model, int32_t parts,
                    double* total, double* folded, uint32_t flags, void* stream);

/* The orbital (Roemer) delay of a binary model, not in the reference: delay_s[i] = tau, the root of
 * tau = D(t - tau / 86400), D the BT or ELL1 delay of the emission time; t_emit_mjd (may be NULL) =
 * t - tau / 86400 rounded once. The orbit and the light-travel equation are solved together by a bracketed Newton
 * iteration with a compile-time cap; a lane that reaches the cap gives NaN, and so does a NaN time. n == 0 touches
 * nothing. CRIMP_ERR_ARG, each with its own text and nothing written: binary not _BT / _ELL1, PB <= 0, A1 < 0, ECC
 * outside [0, 1) (ELL1: EPS1^2 + EPS2^2 >= 1), 2 pi A1 / (PB 86400 (1 - e)) >= 1/2 (beyond it the equation need not
 * have one root), a non-finite value. */
int crimp_binary_delay(const double* t_mjd, int64_t n, const crimp_timing_model* model, double* delay_s,
                       double* t_emit_mjd, uint32_t flags, void* stream);

/* PeriodSearch(time, freq, nbrHarm).ztest()/.htest()/.twod_ztest(freq_dot)
 *   [periodsearch.py:40-125]
 * t: photon times (s) [n]; t0: (t[0]+t[n-1])/2 as periodsearch.py:54 (passed explicitly so that
 * shards of one search share it); freq [nf] (Hz); log10_negfdot [nfd] or NULL (1-D); the trial
 * grid is fd-outer/f-inner (periodsearch.py:264-278) and this call computes flat trials
 * [first, first+count) of it into out[count]. stat = CRIMP_STAT_Z2 or CRIMP_STAT_H (the latter
 * over the 2-D grid is this library's extension). Precision: the CRIMP_FLAG_F64 / _NUFFT notes
 * above; the kernel is chosen from the whole grid (nf, nfd, progression), not from [first, count), so a sharded
 * search computes every trial exactly as an unsharded one -- except that the NUFFT (the default) plans each row
 * segment of [first, count) on its own (a shard of a row is its own progression, so it costs its share): whole rows are
 * bit-identical, a cut row agrees within the plans' ~1e-13 error. */
int crimp_search(const double* t, int64_t n, double t0, const double* freq, int64_t nf,
                 const double* log10_negfdot, int64_t nfd, int32_t nharm, int32_t stat, int64_t first,
                 int64_t count, double* out, uint32_t flags, void* stream);

/* crimp_search and the best trial of its powers in one call: out[count] as crimp_search, best[0] = the largest of
 * out, best[1] = its index within [first, first+count) as a double (np.argmax semantics, as crimp_best), best a host
 * pointer. A NUFFT search reads the best trial back with its fix-up count (one stream sync less than crimp_search +
 * crimp_best; sharding.sharded_search(gather='best')). */
int crimp_search_best(const double* t, int64_t n, double t0, const double* freq, int64_t nf,
                      const double* log10_negfdot, int64_t nfd, int32_t nharm, int32_t stat, int64_t first,
                      int64_t count, double* out, double* best, uint32_t flags, void* stream);

/* Best trial of a power array x[n] (crimp_search's out): best[0] = max, best[1] = its index as a double (exact:
 * n <= 2^53), np.argmax semantics -- ties to the lowest index, NaN above every number   [the maximum the
 * reference's callers take of PeriodSearch's powers; sharding.sharded_search(gather='best')]. best is a host
 * pointer; with CRIMP_FLAG_DEVICE_PTRS x is device memory (else host, staged). One stream sync. */
int crimp_best(const double* x, int64_t n, double* best, uint32_t flags, void* stream);

/* Many one-trial searches at once: for every set i, PeriodSearch(t[offsets[i]:offsets[i+1]], [freq[i]],
 * nbrHarm).htest() / .ztest()   [periodsearch.py:40-125 as measureToAs.py:210-212 calls it per ToA interval;
 * t0 = (first + last)/2 of each set, :54]. t in seconds; out[nset]. fp64 (the reference's precision). */
int crimp_search_sets(const double* t, const int64_t* offsets, int64_t nset, const double* freq, int32_t nharm,
                      int32_t stat, double* out, uint32_t flags, void* stream);

/* Fourier|WrappedCauchy|VonMises(theta, x).loglikelihood{FS,CA,VM}normalized(exposure) and its
 * (norm, phShift) derivatives at arbitrary points   [templatemodels.py:98-121, 201-226, 306-329].
 * x: folded phases of all intervals concatenated, interval i = x[offsets[i] : offsets[i+1]]
 * (cycles for fourier, radians otherwise). Point p is (pt_interval[p], pt_norm[p], pt_phi[p]).
 * out[p*8 + 0..7] = { sum ln(norm + h), sum q, sum h' q, -sum q^2, -sum h' q^2,
 *                     sum (h'' q - h'^2 q^2), min(norm + h), N }   with q = 1/(norm + h),
 * h = model - norm, primes = d/dphShift. fp64 throughout. Host assembles the reference LL. */
int crimp_toa_points(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                     const int64_t* pt_interval, const double* pt_norm, const double* pt_phi, int64_t npts,
                     double* out, uint32_t flags, void* stream);

/* lmfit 'brute' grid of measureToA_* (measureToAs.py:292-295, defineinitialfitparam :698-806):
 * for every interval i, norm a, phShift b:
 *   lnsum[(i*nnorm + a)*nphi + b] = sum_photons ln(norm[i*nnorm+a] + h(x; phi[b]))
 *   hmin[i*nphi + b]              = min_photons h(x; phi[b])
 * fp32 model + logarithm, fp64 accumulation; a Fourier template's part on the f16 matrix cores with every fp32
 * factor split hi + lo (fp32-level products), the likelihood part on the VALU. */
int crimp_toa_grid(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                   const double* norm, int64_t nnorm, const double* phi, int64_t nphi, double* lnsum,
                   double* hmin, uint32_t flags, void* stream);

#define CRIMP_TOA_BRUTE 1      /* crimp_toa_fit options: lmfit brute start (measureToAs.py:292-295, -bm) */
#define CRIMP_TOA_VARY_AMPS 2  /* ampShift free in [0.01, 100] after the first fit (measureToAs.py:305-312, -va) */

/* measureToA_fourier / _cauchy / _vonmises(tempModPP, phases, exposure, phShiftRes=res, brutemin=...,
 * varyAmps=...) for every interval at once, readvaryparam=False   [measureToAs.py:254-693, :698-806]:
 * optional lmfit brute start (20 norms in [norm0/100, 500] x phShift = k*0.05 - bound), the extended-LL
 * maximum in (norm, phShift) -- and ampShift with CRIMP_TOA_VARY_AMPS --, and the 1-sigma scan in steps of
 * 2pi/res with the other free parameters re-profiled at each step. One workgroup per interval runs the
 * whole fit on the device (csrc/toa_fit.h).
 * out[i*8 + 0..6] = { norm, phShift, LLmax, phShift_LL, phShift_UL, likelihood evaluations, ampShift }.
 * The reduced chi2 (:385-393) is crimp_toa_redchi2 on these records (or crimp_toa_fit_redchi2: both at once). */
int crimp_toa_fit(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                  const double* exposure, double norm0, int32_t ph_shift_res, int32_t options, double* out,
                  uint32_t flags, void* stream);

/* Extended-LL sums with template-shape gradients, for fits that free template parameters
 * (readvaryparam, measureToAs.py:727-801 with the likelihoods of templatemodels.py:98-121, 201-226,
 * 306-329). Point p is interval pt_interval[p] with its own template tpls[p] (ampShift applied),
 * norm pt_norm[p] and phShift pt_phi[p]; aux[p*CRIMP_MAX_COMP + j] = I1(k)/I0(k), k = 1/wid_j^2
 * (vonmises; may be NULL otherwise). With m = norm + h the model at a photon:
 * out[p*CRIMP_SHAPE_SUMS + ...] = { sum ln m, min m, sum 1/m, sum (dh/dphShift)/m,
 *     then for j < CRIMP_MAX_COMP: sum (dh/damp_j)/m, sum (dh/dloc_j)/m, sum (dh/dwid_j)/m }
 * (loc = ph_j or cen_j; unused components and the Fourier wid terms are 0). fp64. */
#define CRIMP_SHAPE_SUMS (4 + 3 * CRIMP_MAX_COMP)
int crimp_toa_shape_points(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpls,
                           const double* aux, const int64_t* pt_interval, const double* pt_norm,
                           const double* pt_phi, int64_t npts, double* out, uint32_t flags, void* stream);

/* redChi2 of every fitted interval   [measureToAs.py:385-393 (Fourier), :530-538, :675-683; binphases.py:9-39]:
 * the binned profile (np.histogram with edges[nbins+1] = numpy.linspace(0, upper, nbins+1), upper 1 (Fourier, cycles)
 * or 2 pi) against the template curve at centers[nbins] with the interval's fitted norm, phShift and ampShift from
 * records[i*8 + 0, 1, 6] (crimp_toa_fit's records): out[i] = sum_b (model_b - rate_b)^2 / err_b^2 / (nbins - nfree),
 * rate = cts / (E_i / nbins), err = sqrt(cts) / (E_i / nbins). fp64. */
int crimp_toa_redchi2(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                      const double* exposure, const double* records, const double* edges, const double* centers,
                      int32_t nbins, int32_t nfree, double* out, uint32_t flags, void* stream);

/* crimp_toa_fit and crimp_toa_redchi2 in one call (the whole measureToA_* of every interval, :254-393): the same
 * records in out[i*8 + 0..6] and the same redchi2[i]. The histogram needs only the photons, so it runs on a second
 * stream beside the brute grid and the fits (with CRIMP_FLAG_TIME_KERNELS: after them). */
int crimp_toa_fit_redchi2(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                          const double* exposure, double norm0, int32_t ph_shift_res, int32_t options,
                          const double* edges, const double* centers, int32_t nbins, int32_t nfree, double* out,
                          double* redchi2, uint32_t flags, void* stream);

/* binphases(phases, nbrBins) counts per interval   [binphases.py:9-39]:
 * np.histogram(x, bins=edges) semantics with edges[nbins+1] (numpy.linspace). counts[i*nbins+b]. */
int crimp_binphases(const double* x, const int64_t* offsets, int64_t nint, const double* edges, int32_t nbins,
                    int64_t* counts, uint32_t flags, void* stream);

/* The count cube behind the pulse-profile maps of plot_pps.py: np.histogram2d(phases, energies | times, bins=[...])
 * (:149, :214), the per-tile binphases of the time x energy grid (:319-333) and of the before / after windows
 * (:469-477), folding and binning in one pass when a timing model is given (not in the reference: calcphase, then
 * the histogram on its output).
 *   x[n]: folded phases (model == NULL; cycles or radians, the phase edges decide), or MJD times (model != NULL)
 *         whose phase is calcphase's `folded` (parts = 7, cycles), formed exactly as crimp_calcphase forms it: a fused
 *         call gives the counts of crimp_calcphase followed by an unfused call.
 *   y[n] with y_edges[ny + 1], z[n] with z_edges[nz + 1]: the two other axes. A NULL y (z) is an axis of one bin that
 *         takes every photon: ny (nz) must be 1, the edges are ignored. CRIMP_CUBE_Y_IS_X: y = x (y must be NULL).
 *   nph[nz]: phase bins of every z column (plotting_pp_grid's nbrbins, :277); ph_edges: the columns' nph[j] + 1 edges
 *         concatenated (sum of nph[j] + 1 <= CRIMP_CUBE_MAX_PH_EDGES).
 *   counts[iy * S + zoff[iz] + b], zoff = prefix sum of nph, S = zoff[nz]; int64, zeroed by the call.
 * Bin rule of every axis (np.histogramdd with explicit edges): bin = np.searchsorted(edges, v, 'right') - 1; v equal
 * to the last edge counts in the last bin unless the axis's OPEN_LAST option is set; a value outside the edges or a NaN
 * drops the photon. Exact comparisons against the edges as passed; edges strictly ascending and finite
 * (else CRIMP_ERR_ARG). The edges, nph and the model are host pointers always; x, y, z and counts follow
 * CRIMP_FLAG_DEVICE_PTRS. CRIMP_FLAG_TIME_KERNELS times the kernel (crimp_last_kernel_ms). n == 0 gives zeros. */
#define CRIMP_CUBE_Y_OPEN_LAST 1  /* y axis: last bin [e, e') like the others (plot_pps.py:325), not numpy's closed last bin */
#define CRIMP_CUBE_Z_OPEN_LAST 2  /* the same for the z axis */
#define CRIMP_CUBE_Y_IS_X      4  /* y = x (time axis of a fused phase-time map): x is read once */
#define CRIMP_CUBE_PH_OPEN_LAST 8 /* the same for the phase axis: a phase equal to the last edge is dropped */
#define CRIMP_CUBE_MAX_BINS 1024  /* per axis */
#define CRIMP_CUBE_MAX_PH_EDGES 2048 /* phase edges of all z columns together */
#define CRIMP_CUBE_LDS_BINS 4096  /* largest cube (cells) counted in LDS; above it, global atomics */
int crimp_phase_cube(const double* x, int64_t n, const crimp_timing_model* model,
                     const double* y, const double* y_edges, int32_t ny,
                     const double* z, const double* z_edges, int32_t nz,
                     const double* ph_edges, const int32_t* nph,
                     int64_t* counts, int32_t options, uint32_t flags, void* stream);

/* Timing-model fits of ToAs   [utilities_fittoas.py:204-293, fit_toas.py:140-202] (csrc/timing_fit.h).
 *
 * model_phase_residuals (utilities_fittoas.py:269-293) evaluates a *fit model* -- every scalar that is not an epoch 0,
 * every free parameter equal to its pvec entry, PEPOCH / fixed GLEP_* / WAVEEPOCH / WAVE_OM kept -- and takes from the
 * *full model* the F0 that multiplies the wave sum (F0_base - dF0) and, when no wave key is free, the WAVE A/B values.
 * The host describes that with two models per problem and one map shared by all problems of a call:
 *   fit_base[i]:  the fit model with every free parameter 0 (its WAVE A/B: the .par values);
 *   wave_base[i]: supplies F0_base (f[0]) and, with CRIMP_FIT_WAVES_FIXED, n_wave / WAVEEPOCH / WAVE_OM / WAVE A/B;
 *   map->branch:  which of the reference's three branches applies;
 *   map->slot[k]: the field parameter k overwrites; map->f0_param: the index of the F0 parameter, or -1.
 * The models and the map are host pointers always; the arrays follow CRIMP_FLAG_DEVICE_PTRS. */
#define CRIMP_FIT_MAX_DIM 32
#define CRIMP_FIT_WAVES_FIXED 0 /* no wave key free: Taylor + glitches of the fit model, waves of the full model */
#define CRIMP_FIT_WAVES_ONLY 1  /* every key is a wave key: the wave sum alone */
#define CRIMP_FIT_WAVES_MIXED 2 /* both: Taylor + glitches + the fit model's waves */
#define CRIMP_FIT_SLOT_F 0      /* index = n of Fn, 0..12 */
#define CRIMP_FIT_SLOT_GLITCH 1 /* index = glitch (0-based), sub = 0..6: GLEP, GLPH, GLF0, GLF1, GLF2, GLF0D, GLTD */
#define CRIMP_FIT_SLOT_WAVE 2   /* index = harmonic (0-based), sub = 0 (A) or 1 (B) */
typedef struct crimp_fit_slot {
    int32_t kind, index, sub;
} crimp_fit_slot;
typedef struct crimp_fit_map {
    int32_t ndim;     /* 1..CRIMP_FIT_MAX_DIM */
    int32_t branch;   /* CRIMP_FIT_WAVES_* */
    int32_t f0_param; /* k with slot[k] = F0, or -1 */
    crimp_fit_slot slot[CRIMP_FIT_MAX_DIM];
} crimp_fit_map;

/* gaussian_nll(y - mean(y), model_phase_residuals(x, parfile, pvec, keys), yerr) of nprob problems x P vectors in
 * one launch   [utilities_fittoas.py:204-210, :236-239, :269-293]. Problem i's ToAs are [offsets[i], offsets[i+1]) of
 * t_mjd / y / yerr (at least one each); pvec[nprob][P][ndim]; nll[nprob][P]; mu (may be NULL) = the mean-subtracted
 * model residuals, problem i's at mu + P * offsets[i], [P][n_i]. A value depends on its ToAs and its vector alone (fixed
 * summation order): not on P, nprob or the launch shape. CRIMP_ERR_ARG: an empty problem, ndim outside
 * 1..CRIMP_FIT_MAX_DIM, a slot that names a field outside some problem's model. */
int crimp_timing_nll(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets, int64_t nprob,
                     const crimp_timing_model* fit_base, const crimp_timing_model* wave_base,
                     const crimp_fit_map* map, const double* pvec, int64_t P, double* nll, double* mu,
                     uint32_t flags, void* stream);

/* emcee.EnsembleSampler(W, ndim, log_probability).run_mcmc(p0, steps) of nprob problems in one launch
 * [fit_toas.py:140-163]: the affine-invariant stretch move, a = 2, log-probability = box prior (Prior.log_prior:
 * strict inequalities, +-inf = no bound on that side) - the NLL above, from the same device function as
 * crimp_timing_nll (logprob equals -crimp_timing_nll(chain) bit for bit). One workgroup per problem runs all steps.
 * The ensemble is split into fixed even / odd halves; each half is updated against the other as it stands:
 * proposal c - (c - x) z, z = ((a-1)u + 1)^2 / a, accepted when log u' < (ndim-1) log z + lp_new - lp_old; a proposal
 * outside the box is rejected without evaluating it, and so is one whose log-probability is not finite (the reference
 * lets emcee raise on NaN). Random numbers: Philox4x32-10, key = seed, counter = (first_problem + i, step, walker,
 * draw): a chain depends on the seed, the problem's global index and its own data, not on the rest of the launch.
 * Key = (seed's low 32 bits, its high 32 bits); the index and the step enter by their low 32 bits. A 53-bit uniform of
 * two output words is U(a, b) = (((a >> 5) << 26 | (b >> 6)) + 0.5) 2^-53 in fp64, in (0, 1]. Walker w = 2 k + h of
 * half h reads draw 0 for u = U(word 0, word 1) and its partner, walker 2 floor(word 2 * (W / 2) / 2^32) + (1 - h) of
 * the other half, and draw 1 for u' = U(word 0, word 1). tests/stream_reference.py restates this on the host and
 * tests/test_gpu_sampler_replay.py holds every decision of the three samplers to it.
 * p0[nprob][W][ndim]; lo, hi [nprob][ndim]; W even, 2 ndim <= W <= 256; steps >= 1.
 * chain[nprob][steps][W][ndim], logprob[nprob][steps][W], accepted[nprob][W] (accepted moves per walker). */
int crimp_timing_mcmc(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets,
                      int64_t nprob, const crimp_timing_model* fit_base, const crimp_timing_model* wave_base,
                      const crimp_fit_map* map, const double* p0, const double* lo, const double* hi, int32_t W,
                      int64_t steps, uint64_t seed, int64_t first_problem, double* chain, double* logprob,
                      int64_t* accepted, uint32_t flags, void* stream);

/* Timing-model fits of ToAs under a binary orbit, the orbital keys free (not in the reference; csrc/orbit_fit.h,
 * DESIGN.md 5.9). crimp_timing_nll / _mcmc refuse a model with an orbit and a CRIMP_FIT_SLOT_BINARY slot; these two
 * calls are the same fits with par[i], the full model of problem i with its binary block, beside the two bases (whose
 * own binary blocks are not read).
 *
 * A CRIMP_FIT_SLOT_BINARY slot (index = CRIMP_ORBIT_*, sub not read) corrects a field of par's orbit as
 * inject_free_params corrects every ordinary key: field(p) = par's field - p, in the unit of crimp_timing_model's
 * binary block (days, light-seconds, MJD, degrees, degrees / yr; PBDOT and A1DOT dimensionless), the fp64 difference.
 * With B0 the orbit of par, B(p) the corrected one, tau_B(t) the delay crimp_binary_delay defines and phi_M(t') the
 * spin phase of model M at the emission time t', the model residual of ToA i before the mean is subtracted is
 *   m_i(p) = phi_fit(p)(teF_i) + R_i(p),   R_i(p) = phi_par(te0_i) - phi_par(teF_i),
 *   te0 = t - tau_B0(t) / 86400,   teF = t - tau_B(p)(t) / 86400,
 * phi_fit(p) the fit model of crimp_timing_nll (same branches, F0_base - dF0 and wave_base), evaluated at the emission
 * time of the corrected orbit. R is evaluated as one small phase, dtau (nu - nud dtau / 2) with dtau = tau_B(p) -
 * tau_B0 and nu, nud the first two derivatives of phi_par at te0 (glitches active there and waves included), computed
 * once per call; the dropped term is |phi_par'''| |dtau|^3 / 6. A ToA with a glitch epoch of par between te0 and teF
 * is outside the contract. mu = m - mean(m); NLL = gaussian_nll(y - mean(y), mu, yerr). With no BINARY slot, or with
 * every orbital entry 0, R is exactly 0: the spin fit under the fixed orbit.
 * A vector whose corrected orbit is outside the limits of crimp_binary_delay (a non-finite field included) is
 * inadmissible: NLL = +inf, its mu row +inf, and the sampler rejects it without evaluating it, as it rejects a
 * proposal outside the box.
 * CRIMP_ERR_ARG of both calls, nothing written: the texts of crimp_timing_nll / _mcmc; "the model has no binary";
 * a base orbit outside the limits (the texts of crimp_binary_delay); "slot names an orbit field the model's kind does
 * not have" (ECC, OM, OMDOT, GAMMA under ELL1; EPS1, EPS2 under BT); "slot names an orbit field outside
 * CRIMP_ORBIT_PB..CRIMP_ORBIT_A1DOT"; "two slots name one orbit field". */
#define CRIMP_FIT_SLOT_BINARY 3 /* index = CRIMP_ORBIT_* (crimp_orbit_* and crimp_photon_orbit_* only) */
#define CRIMP_ORBIT_PB 0
#define CRIMP_ORBIT_A1 1
#define CRIMP_ORBIT_T0 2 /* T0 (BT) or TASC (ELL1) */
#define CRIMP_ORBIT_ECC 3
#define CRIMP_ORBIT_OM 4
#define CRIMP_ORBIT_OMDOT 5
#define CRIMP_ORBIT_GAMMA 6
#define CRIMP_ORBIT_EPS1 7
#define CRIMP_ORBIT_EPS2 8
#define CRIMP_ORBIT_PBDOT 9
#define CRIMP_ORBIT_A1DOT 10

/* crimp_timing_nll with par[nprob]: the same arrays, outputs and independence of the launch shape. */
int crimp_orbit_nll(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets, int64_t nprob,
                    const crimp_timing_model* par, const crimp_timing_model* fit_base,
                    const crimp_timing_model* wave_base, const crimp_fit_map* map, const double* pvec, int64_t P,
                    double* nll, double* mu, uint32_t flags, void* stream);

/* crimp_timing_mcmc with par[nprob]: the same move, halves, Philox counters, first_problem and outputs; logprob equals
 * -crimp_orbit_nll(chain) bit for bit, and no inadmissible vector enters a chain. */
int crimp_orbit_mcmc(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets, int64_t nprob,
                     const crimp_timing_model* par, const crimp_timing_model* fit_base,
                     const crimp_timing_model* wave_base, const crimp_fit_map* map, const double* p0,
                     const double* lo, const double* hi, int32_t W, int64_t steps, uint64_t seed,
                     int64_t first_problem, double* chain, double* logprob, int64_t* accepted, uint32_t flags,
                     void* stream);

/* ---- orbit search: Z^2_m / H over a grid of binary orbits (not in the reference)
 * For orbit o of orbits[norb][nkeys] (host, row-major): B_o is base's orbit with field keys[q] (CRIMP_ORBIT_*, each
 * at most once, valid for base's kind) replaced by orbits[o][q], an absolute value in the unit of crimp_timing_model's
 * binary block; derived as crimp_binary_delay derives base's. With tau = the delay crimp_binary_delay defines,
 *   dt_i = fl(fl((t_i - tref_mjd) 86400) - tau_{B_o}(t_i)),   ph = freq[j] dt + (0.5 fdot) dt^2   (cycles)
 *   power[o - first][j] = Z^2_nharm (CRIMP_STAT_Z2) or H (CRIMP_STAT_H) of C_k = sum_i cos 2 pi k ph, S_k (sin), n,
 * in the formula order of crimp_search's fp64 path, for orbits [first, first + count). best[o - first] = (the largest
 * power of the row, its trial index as a double), np.argmax semantics (the lowest index wins a tie, a NaN wins). power
 * or best may be NULL (not both unless count or nf is 0). base's spin keys are not read. A photon whose delay
 * iteration reaches its cap makes its orbit's powers NaN.
 * power[o][j] does not depend on norb, first, count or the scratch cap: the photons are summed in an order fixed by n.
 * t_mjd, power and best follow CRIMP_FLAG_DEVICE_PTRS; base, keys, orbits and freq are host pointers always.
 * CRIMP_FLAG_TIME_KERNELS times the search and finalize kernels together (crimp_last_kernel_ms). count == 0 or
 * nf == 0 launches nothing. Partial sums of a launch are bounded by CRIMP_ORBIT_SCRATCH_KB (default 1 GiB): more
 * orbits run in batches.
 * CRIMP_ERR_ARG, nothing launched or written: n < 1; nf, norb < 0; [first, first + count) outside [0, norb]; nharm
 * outside [1, 256]; stat; nkeys outside [0, 11]; "key ... is not a CRIMP_ORBIT_* field", "two keys name one orbit
 * field", "key names an orbit field the model's kind does not have"; "the model has no binary"; a non-finite freq,
 * fdot or tref; and "orbit <index>: <text>" for the first orbit of the range outside the limits of
 * crimp_binary_delay (its texts). */
int crimp_orbit_search(const double* t_mjd, int64_t n, const crimp_timing_model* base, double tref_mjd,
                       const int32_t* keys, int32_t nkeys, const double* orbits, int64_t norb, const double* freq,
                       int64_t nf, double fdot, int32_t nharm, int32_t stat, int64_t first, int64_t count,
                       double* power, double* best, uint32_t flags, void* stream);

/* The plan crimp_orbit_search takes for these sizes under the scratch cap in force (no device needed):
 * out[0..5] = photons per slice, slices, trials per chunk J, orbits per launch, launches, bytes of partial sums. */
int crimp_orbit_search_plan(int64_t n, int64_t nf, int32_t nharm, int32_t stat, int64_t norb, int64_t* out);

/* Photon-domain timing fits (not in the reference; csrc/photon_fit.h).
 *
 * The vector p corrects the model as inject_free_params does, full(p) = par - p on every free key, and its likelihood
 * is the unbinned template likelihood of the photons folded with full(p):
 *   delta_i = Phi(t_i; par) - Phi(t_i; full(p))   (cycles; evaluated as one small phase, never as a difference)
 *   u_i     = x_i - delta_i - PHOFF               (x_i: the folded phase of t_i under par, cycles for every template)
 *   NLL(p)  = -sum_i ln(m(u_i) / norm), m = norm + the template part (templatemodels.py:64-82, :166-185, :271-290);
 *             +inf when some m(u_i) <= 0.
 * par is the full model (one problem per call); map->slot names the free keys (map->branch and map->f0_param are not
 * read). Admitted slots are the ones in which the phase is linear: CRIMP_FIT_SLOT_F, CRIMP_FIT_SLOT_GLITCH with sub
 * 1..5 (GLPH, GLF0, GLF1, GLF2, GLF0D) and CRIMP_FIT_SLOT_WAVE. phoff = 1 appends a free phase offset PHOFF (cycles)
 * as the last entry of every vector: D = ndim + phoff entries. norm (> 0) and tpl->amp_shift are fixed. par, map and
 * tpl are host pointers always; the arrays follow CRIMP_FLAG_DEVICE_PTRS. CRIMP_FLAG_TIME_KERNELS times the kernels
 * of a call together (crimp_last_kernel_ms).
 * CRIMP_ERR_ARG of both calls, nothing written: "n < 1"; a slot outside the model ("slot names ..."); a refused slot
 * ("GLEP is not fitted to photons", "GLTD is not fitted to photons"); "ndim must be 1..CRIMP_FIT_MAX_DIM - phoff";
 * "binary models are not fitted yet"; a bad template (crimp_toa_points' texts); "norm must be positive". */

/* Photons per tile of the kernels' fixed summation order (a compile-time constant of the library). */
int crimp_photon_tile(void);

/* NLL of P vectors over n photons in one launch: pvec[P][D], nll[P], delta (may be NULL) [P][n] = delta_i of every
 * vector. A value depends on the photons, its vector and crimp_photon_tile() alone: not on P or the launch shape. */
int crimp_photon_nll(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                     const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                     const double* pvec, int64_t P, double* nll, double* delta, uint32_t flags, void* stream);

/* The ensemble sampler of crimp_timing_mcmc (same move, halves, box prior, rejections and Philox counters, problem
 * index 0) on log-probability = box prior - the NLL above; logprob equals -crimp_photon_nll(chain) bit for bit. The
 * walkers live on the device and the whole chain is queued at once: per half-step one likelihood launch for that
 * half's proposals and one small accept/update launch. p0[W][D]; lo, hi [D]; W even, 2 D <= W <= 256; steps >= 1.
 * chain[steps][W][D], logprob[steps][W], accepted[W]. */
int crimp_photon_mcmc(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                      const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                      const double* p0, const double* lo, const double* hi, int32_t W, int64_t steps, uint64_t seed,
                      double* chain, double* logprob, int64_t* accepted, uint32_t flags, void* stream);

/* Photon-domain timing fits under a binary orbit, the orbital keys free (not in the reference;
 * csrc/photon_orbit_fit.h). crimp_photon_nll / _mcmc refuse a model with an orbit; these two calls take
 * the same arguments with par carrying its binary block, and map may hold CRIMP_FIT_SLOT_BINARY slots, which correct
 * par's orbit as in crimp_orbit_nll: field(p) = par's field - p in the unit of crimp_timing_model's binary block, the
 * fp64 difference. With B0 the orbit of par, B(p) the corrected one and tau_B(t) the delay of crimp_binary_delay,
 *   te0 = t - tau_B0(t) / 86400,   teF = t - tau_B(p)(t) / 86400,   dtau = tau_B(p)(t) - tau_B0(t)
 *   delta_i = phi_pf(p)(teF_i) + R_i,   R_i = dtau_i (nu_i - nud_i dtau_i / 2)
 *   u_i = x_i - delta_i - PHOFF,   NLL as crimp_photon_nll defines it,
 * phi_pf(p) the photon fit model of crimp_photon_nll (every linear amplitude of par 0, the free ones their entries,
 * the wave cross term exact) at the emission time of the corrected orbit, nu and nud the first two derivatives of par's
 * spin phase at te0 (glitches active there and waves included), computed with tau_B0 once per call. x_i is the folded
 * phase of t_i under par at the emission time (crimp_calcphase with CRIMP_PART_EMISSION). delta_i equals Phi(t_i; par)
 * - Phi(t_i; full(p)) up to the dropped |phi_par'''| |dtau|^3 / 6; a photon with a glitch epoch of par between te0 and
 * teF is outside the contract. With no BINARY slot, or every orbital entry 0, R is exactly 0.
 * A vector whose corrected orbit is outside the limits of crimp_binary_delay (a non-finite field included) is
 * inadmissible: NLL = +inf, its delta row +inf, no solve is run for it and the sampler rejects it as it rejects a
 * proposal outside the box. A photon whose delay iteration reaches its cap makes the NLL +inf.
 * CRIMP_ERR_ARG of both calls, nothing written: the texts of crimp_photon_nll / _mcmc but "binary models are not
 * fitted yet"; "the model has no binary"; a base orbit outside the limits (the texts of crimp_binary_delay); "slot
 * names an orbit field outside CRIMP_ORBIT_PB..CRIMP_ORBIT_A1DOT"; "two slots name one orbit field"; "slot names an
 * orbit field the model's kind does not have" (ECC, OM, OMDOT, GAMMA under ELL1; EPS1, EPS2 under BT).
 * CRIMP_FLAG_TIME_KERNELS times the kernel of the per-photon constants with the others. */

/* crimp_photon_nll under an orbit: the same arrays, outputs and independence of P and the launch shape. */
int crimp_photon_orbit_nll(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                           const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                           const double* pvec, int64_t P, double* nll, double* delta, uint32_t flags, void* stream);

/* crimp_photon_mcmc under an orbit: the same move, halves, box prior, Philox counters and outputs; logprob equals
 * -crimp_photon_orbit_nll(chain) bit for bit, and no inadmissible vector enters a chain. */
int crimp_photon_orbit_mcmc(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                            const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                            const double* p0, const double* lo, const double* hi, int32_t W, int64_t steps,
                            uint64_t seed, double* chain, double* logprob, int64_t* accepted, uint32_t flags,
                            void* stream);

/* Interval selection of measureToAs (measureToAs.py:168-182): TIME[(TIME >= start) & (TIME <= end)] per ToA interval
 * (:173-174) and its first / last photon (ToA_mid, :182).
 * crimp_is_sorted: *unsorted = 1 if some t[i+1] < t[i] (or a NaN), else 0 (host int; t host or device per flags).
 * crimp_select_intervals: on time-sorted t, lo[i] = np.searchsorted(t, starts[i], "left"), count[i] =
 *   max(np.searchsorted(t, ends[i], "right") - lo[i], 0) (0 for a NaN bound), first_last[2i], [2i+1] = the
 *   interval's first and last time (NaN if empty; may be NULL) -- the mask's photons on sorted times.
 * crimp_gather_ranges: out[offsets[i] + j] = t[lo[i] + j] for j < offsets[i+1] - offsets[i] (offsets[0] = 0; every
 *   range inside t[0, n)): the intervals' photons concatenated, as measureToAs.py's per-interval selections. */
int crimp_is_sorted(const double* t, int64_t n, int32_t* unsorted, uint32_t flags, void* stream);
int crimp_select_intervals(const double* t, int64_t n, const double* starts, const double* ends, int64_t nint,
                           int64_t* lo, int64_t* count, double* first_last, uint32_t flags, void* stream);
int crimp_gather_ranges(const double* t, int64_t n, const int64_t* lo, const int64_t* offsets, int64_t nint,
                        double* out, uint32_t flags, void* stream);

/* Event simulator   [simulatemodulatedlc.py:19-96: the binned sinusoid at constant frequency drawn from NumPy's global
 * RNG, :64-79 its per-bin Poisson counts and uniform phases, :88-92 its flat background; and this build's host
 * generators crimp_amd/synth.py pulsed_events / template_phases] (csrc/sim_events.h).
 *
 * Events on [mjd_start, mjd_start + span_s / 86400), restricted to the union of the half-open GTIs [start, stop) when
 * given, form an inhomogeneous Poisson process of rate lambda(t) = S(frac(phi(t))) + bkg counts/s: phi(t) is what
 * crimp_calcphase computes for that MJD (parts = 7), S the source shape --
 *   CRIMP_SIM_TEMPLATE: norm + the template part of `tpl` at ph_shift (amp_shift in tpl), the model value of
 *     templatemodels.py:64-82, :166-185, :271-290 as crimp_toa_points forms it (x in cycles for Fourier, radians
 *     otherwise; the fit's sign of phShift: crimp_toa_fit on simulated events returns ph_shift);
 *   CRIMP_SIM_STEPS: steps[k] on the phase bin [k / n_steps, (k + 1) / n_steps)  (simulatemodulatedlc.py:64-79).
 * lam_max is the caller's bound: S + bkg <= lam_max at every phase (the library thins candidates of rate lam_max and
 * trusts it). Time is cut into cells of cell_s seconds anchored at mjd_start; the events of a cell depend on (seed,
 * model, shape, mjd_start, span_s, cell_s, GTIs, the cell's index) alone, so the calls over [first_cell, first_cell +
 * n_cells) of any partition concatenate to the whole list bit for bit (n_cells = -1: every cell from first_cell on).
 * Random numbers: Philox4x32-10, key = seed (low word, high word), counter = (cell low, cell high, round, lane) with
 * 64 lanes per round. Words 0-1 give the lane's gap -log(U(word 0, word 1)) / lam_max (U: the 53-bit uniform of
 * crimp_timing_mcmc), words 2-3 the thinning uniform u = U(word 2, word 3). A round's 64 gaps are summed by an
 * inclusive scan in doubling order (distances 1, 2, ..., 32) onto the running time, which starts at 0 in every cell;
 * a candidate at s = cell * cell_s + that sum counts while s < min((cell + 1) * cell_s, span_s), survives inside the
 * GTIs when u lam_max < S + bkg, and rounds follow until the running time passes the cell's end
 * (tests/stream_reference.py replays it; tests/test_gpu_simulate_replay.py holds every candidate to the replay).
 *   t_out == NULL: the count pass alone, *n_out = the number of events. Otherwise cap < that number fails with
 *   CRIMP_ERR_ARG (nothing written, *n_out still set); else t_out[n] non-decreasing = out_offset_s + seconds since
 *   mjd_start, or the MJD mjd_start + s / 86400 with CRIMP_FLAG_TIME_DAYS; bkg_out[n] (may be NULL) = 1 for a
 *   background event (u lam_max >= S), 0 for a source event.
 * model, shape and n_out are host pointers always; shape->steps, gti, t_out and bkg_out follow CRIMP_FLAG_DEVICE_PTRS.
 * gti[ngti][2] MJD, sorted and disjoint (NULL / 0: the whole span). CRIMP_FLAG_TIME_KERNELS times the count pass, the
 * scan and the fill pass together (crimp_last_kernel_ms). CRIMP_ERR_ARG: span_s <= 0, a non-finite or non-positive
 * lam_max or cell_s, lam_max * cell_s > 65536, unsorted or overlapping GTIs, n_steps < 1, a cell range outside the
 * span's cells, more than 2^31 - 1 cells. */
#define CRIMP_SIM_TEMPLATE 0
#define CRIMP_SIM_STEPS 1
typedef struct crimp_sim_shape {
    int32_t kind;         /* CRIMP_SIM_TEMPLATE | CRIMP_SIM_STEPS */
    int32_t n_steps;      /* steps: number of rates */
    crimp_template tpl;   /* template */
    double norm;          /* template: norm (counts/s) */
    double ph_shift;      /* template: phShift (rad) */
    const double* steps;  /* steps: n_steps rates (counts/s) */
    double bkg;           /* flat background b >= 0 (counts/s) */
    double lam_max;       /* bound of S + bkg */
} crimp_sim_shape;
int crimp_sim_events(const crimp_timing_model* model, const crimp_sim_shape* shape, double mjd_start, double span_s,
                     double cell_s, const double* gti, int64_t ngti, uint64_t seed, int64_t first_cell,
                     int64_t n_cells, double* t_out, uint8_t* bkg_out, int64_t cap, int64_t* n_out,
                     double out_offset_s, uint32_t flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CRIMP_HIP_H */
