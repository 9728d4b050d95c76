// crimp_hip.hip -- MI355X (gfx950) kernels + C-ABI for CRIMP's photon hot path.
//
// Entry points are declared (with the reference routine each replaces) in
// include/crimp_hip.h. Layout of this file:
//   1. runtime helpers (errors, stream-ordered scratch, staging of host buffers)
//   2. fp32 sin/cos in revolutions (polynomial and hardware v_sin/v_cos)
//   3. calcphase            -- HBM-bound fp64 phase folding
//   4. periodicity search   -- exact i8-MFMA kernel (search_exact.h, default), NUFFT (search_nufft.h,
//                              opt-in), fp64 kernel, finalize
//   5. ToA likelihood scan  -- fp64 point evaluator, fp32 brute grid, binning
//   6. C-ABI
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <chrono>
#include <type_traits>
#include <vector>

#include "../../include/crimp_hip.h"
#include "search_plan.h"  // the host plans of the exact / fp64 searches and the constants they share with the kernels

#define CRIMP_VERSION 2

// ============================================================== 1. runtime helpers
static thread_local std::string g_err;
static std::mutex g_mutex;

// CRIMP_FLAG_TIME_KERNELS: hipEvents around the timed spans of the last call (ms): the harmonic-sum kernels of a
// search, the calcphase kernel, the brute-grid and the fit kernels of crimp_toa_fit
static double g_last_kernel_ms = -1.0;
static std::vector<double> g_kernel_times;
// trials of the last crimp_search recomputed by the fp64 fix-up (exact path)
static int64_t g_last_fixups = 0;
static int64_t g_last_grid_norms = 0;  // brute-grid norms evaluated per phShift by the last crimp_toa_fit
static int64_t g_last_grid_fast = 0;   // the last crimp_toa_fit's brute-grid mode (kGridNoMin | kGridProd8 bits)
struct KernelTimer {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    bool on;
    KernelTimer(hipStream_t st, bool enable) : s(st), on(enable) {
        if (on && (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess)) on = false;
    }
    void start() {
        if (on) (void)hipEventRecord(a, s);
    }
    void stop() {
        if (!on) return;
        (void)hipEventRecord(b, s);
        float ms = -1.0f;
        if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) {
            if (g_kernel_times.empty()) g_last_kernel_ms = ms;
            g_kernel_times.push_back(ms);
        }
    }
    ~KernelTimer() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

static int set_err(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return set_err(CRIMP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

#define ARGCHK(cond, msg)                                                                          \
    do {                                                                                           \
        if (!(cond)) return set_err(CRIMP_ERR_ARG, msg);                                           \
    } while (0)

// CRIMP_DEBUG=1: poison every scratch allocation with 0xFF (NaN) bytes before use.
static int debug_level() {
    static int lvl = -1;
    if (lvl < 0) {
        const char* e = getenv("CRIMP_DEBUG");
        lvl = e ? atoi(e) : 0;
    }
    return lvl;
}

// Device scratch: a small caching allocator (hipMalloc'd blocks reused across calls). Every
// entry point synchronises its stream before returning and calls are serialised by g_mutex, so
// a block handed back at the end of a call is idle when the next call takes it. The idle blocks
// of a device are freed when hipMalloc fails (then the allocation is retried once) or when the
// cached bytes would pass CRIMP_SCRATCH_CAP_MB (default 8192), and by crimp_release_scratch().
struct Block {
    void* p;
    size_t bytes;
    int dev;
    bool busy;
};
static std::vector<Block> g_blocks;

static size_t scratch_cap_bytes() {
    static size_t cap = 0;
    if (cap == 0) {
        const char* e = getenv("CRIMP_SCRATCH_CAP_MB");
        const long long mb = e ? atoll(e) : 8192;
        cap = (size_t)(mb > 0 ? mb : 8192) << 20;
    }
    return cap;
}

// frees the idle blocks of device `dev` (all devices for dev < 0)
static void release_idle_blocks(int dev) {
    std::vector<Block> keep;
    for (const Block& b : g_blocks) {
        if (!b.busy && (dev < 0 || b.dev == dev)) {
            (void)hipFree(b.p);
        } else {
            keep.push_back(b);
        }
    }
    g_blocks.swap(keep);
}

struct Scratch {
    hipStream_t s;
    int dev = 0;
    std::vector<void*> held;
    explicit Scratch(hipStream_t st) : s(st) { (void)hipGetDevice(&dev); }
    ~Scratch() {
        // an error return may leave kernels of this call queued on the stream: drain it before the blocks
        // they may still write become reusable (a no-op on the normal path, which returns drained)
        if (!held.empty()) (void)hipStreamSynchronize(s);
        for (void* p : held)
            for (Block& b : g_blocks)
                if (b.p == p) b.busy = false;
    }
    template <typename T>
    hipError_t alloc(T** out, size_t count) {
        const size_t bytes = (std::max<size_t>(count * sizeof(T), 16) + 255) & ~size_t(255);
        size_t pick = (size_t)-1, cached = 0;
        for (size_t i = 0; i < g_blocks.size(); ++i) {
            const Block& b = g_blocks[i];
            cached += b.bytes;
            if (!b.busy && b.dev == dev && b.bytes >= bytes && b.bytes <= 2 * bytes + (1u << 20) &&
                (pick == (size_t)-1 || b.bytes < g_blocks[pick].bytes))
                pick = i;
        }
        if (pick == (size_t)-1) {
            if (cached + bytes > scratch_cap_bytes()) release_idle_blocks(dev);
            void* p = nullptr;
            hipError_t e = hipMalloc(&p, bytes);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                release_idle_blocks(dev);
                e = hipMalloc(&p, bytes);
                if (e != hipSuccess) return e;
            }
            g_blocks.push_back(Block{p, bytes, dev, false});
            pick = g_blocks.size() - 1;
        }
        g_blocks[pick].busy = true;
        held.push_back(g_blocks[pick].p);
        *out = static_cast<T*>(g_blocks[pick].p);
        if (debug_level() > 0) return hipMemset(g_blocks[pick].p, 0xFF, g_blocks[pick].bytes);
        return hipSuccess;
    }
};

// Host staging uses blocking copies: inputs are copied before any kernel of the call is queued,
// outputs after the stream has drained.
template <typename T>
static hipError_t stage_in(Scratch& sc, const T* src, size_t count, bool dev, const T** out) {
    if (dev || src == nullptr || count == 0) {
        *out = src;
        return hipSuccess;
    }
    T* d = nullptr;
    hipError_t e = sc.alloc(&d, count);
    if (e != hipSuccess) return e;
    *out = d;
    return hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice);
}

template <typename T>
static hipError_t stage_out(Scratch& sc, T* dst, size_t count, bool dev, T** out) {
    if (dev || dst == nullptr) {
        *out = dst;
        return hipSuccess;
    }
    return sc.alloc(out, count);
}

template <typename T>
static hipError_t copy_back(hipStream_t s, T* host, const T* devp, size_t count, bool dev) {
    if (dev || host == nullptr || count == 0) return hipSuccess;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    return hipMemcpy(host, devp, count * sizeof(T), hipMemcpyDeviceToHost);
}

// blocking host <-> device copies of small host-side tables
static hipError_t h2d(void* d, const void* h, size_t bytes) { return hipMemcpy(d, h, bytes, hipMemcpyHostToDevice); }

// Page-locked staging of a call's small host->device uploads (crimp_toa_fit: template, lattice, candidate norms,
// certificate masks): copied into one hipHostMalloc'd buffer and queued with hipMemcpyAsync on the call's stream, so
// the host does not wait for each pageable copy (~290 us of setup before the first kernel, profiles/r04). Calls are
// serialised by g_mutex and drain their stream before returning, so the buffer is free again at the next call.
struct PinnedStage {
    char* p = nullptr;
    size_t cap = 0, used = 0;
};
static PinnedStage g_pin;
static void pin_begin(size_t bytes) {
    g_pin.used = 0;
    if (g_pin.cap >= bytes || bytes > (size_t(64) << 20)) return;  // (huge batches: the blocking copies past the cap)
    if (g_pin.p) (void)hipHostFree(g_pin.p);
    g_pin.p = nullptr;
    g_pin.cap = 0;
    const size_t cap = std::max<size_t>(bytes, size_t(1) << 20);
    if (hipHostMalloc(reinterpret_cast<void**>(&g_pin.p), cap, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        g_pin.p = nullptr;  // no staging: h2d_async falls back to the blocking copy
        return;
    }
    g_pin.cap = cap;
}
static hipError_t h2d_async(hipStream_t s, void* d, const void* h, size_t bytes) {
    const size_t need = (bytes + 255) & ~size_t(255);
    if (!g_pin.p || g_pin.used + need > g_pin.cap) return h2d(d, h, bytes);
    char* q = g_pin.p + g_pin.used;
    g_pin.used += need;
    std::memcpy(q, h, bytes);
    return hipMemcpyAsync(d, q, bytes, hipMemcpyHostToDevice, s);
}
// Device -> host after the stream's queued work. Small reads (flags, counts, grid scalars: the routing readbacks
// of a search) go through a page-locked per-thread buffer with one async copy and one stream sync: a blocking
// pageable hipMemcpy of a few bytes after the sync cost ~30 us per readback (rocprofv3 sys-trace, profiles/r05).
static hipError_t d2h(hipStream_t s, void* h, const void* d, size_t bytes) {
    constexpr size_t kSmall = 16384;  // (a folded NUFFT search's read-back block, search_nufft_finish.h)
    thread_local void* pin = nullptr;
    if (bytes <= kSmall) {
        if (!pin && hipHostMalloc(&pin, kSmall, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            pin = nullptr;
        }
        if (pin) {
            hipError_t e = hipMemcpyAsync(pin, d, bytes, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) return e;
            std::memcpy(h, pin, bytes);
            return hipSuccess;
        }
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return e;
    return hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost);
}

static hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// The prologue of every computing entry point: calls are serialised by g_mutex for their whole length, the pointer
// and timing flags decoded, the kernel-time record of the previous call cleared when this one is timed. kKeepTimes:
// the entries that record no kernel times (crimp_best and the interval selection) leave the last record standing.
struct Call {
    enum Times { kResetTimes, kKeepTimes };
    std::lock_guard<std::mutex> lk;
    const bool dev, timed;  // CRIMP_FLAG_DEVICE_PTRS, CRIMP_FLAG_TIME_KERNELS
    const hipStream_t s;
    Call(uint32_t flags, void* stream, Times times = kResetTimes)
        : lk(g_mutex), dev(flags & CRIMP_FLAG_DEVICE_PTRS), timed(flags & CRIMP_FLAG_TIME_KERNELS),
          s(as_stream(stream)) {
        if (timed && times == kResetTimes) {
            g_kernel_times.clear();
            g_last_kernel_ms = -1.0;
        }
    }
};

// offsets[n + 1] on the host: offsets[0] >= 0 and non-decreasing, or increasing where strict (every span holds
// something); otherwise CRIMP_ERR_ARG with the entry's own text. *max_span: the largest span.
static int check_offsets(const std::vector<int64_t>& h, bool strict, const char* msg, int64_t* max_span = nullptr) {
    int64_t m = 0;
    ARGCHK(h[0] >= 0, msg);
    for (size_t i = 0; i + 1 < h.size(); ++i) {
        ARGCHK(strict ? h[i + 1] > h[i] : h[i + 1] >= h[i], msg);
        m = std::max(m, h[i + 1] - h[i]);
    }
    if (max_span) *max_span = m;
    return CRIMP_OK;
}
// the table copied from the caller's device or host pointer (the stream drained once), then checked
static int read_offsets(const Call& c, const int64_t* offsets, int64_t n, bool strict, const char* msg,
                        std::vector<int64_t>* h, int64_t* max_span = nullptr) {
    h->resize((size_t)n + 1);
    if (c.dev)
        HIPCHK(d2h(c.s, h->data(), offsets, h->size() * sizeof(int64_t)));
    else
        std::memcpy(h->data(), offsets, h->size() * sizeof(int64_t));
    return check_offsets(*h, strict, msg, max_span);
}

// Several small tables of the caller's to the host with one stream drain: async reads into the page-locked staging
// buffer (pin_begin) where they fit, blocking copies otherwise; plain copies from host pointers. Empty reads are
// skipped.
struct HostRead {
    void* dst;
    const void* src;
    size_t bytes;
};
static hipError_t read_list(const Call& c, std::initializer_list<HostRead> reads) {
    const auto slot = [](size_t bytes) { return (bytes + 255) & ~size_t(255); };
    size_t need = 0;
    for (const HostRead& r : reads) need += slot(r.bytes);
    const bool pinned = c.dev && g_pin.p && need <= g_pin.cap;
    if (c.dev && !pinned) {
        const hipError_t e = hipStreamSynchronize(c.s);
        if (e != hipSuccess) return e;
    }
    char* q = g_pin.p;
    for (const HostRead& r : reads) {
        if (r.bytes == 0) continue;
        hipError_t e = hipSuccess;
        if (pinned)
            e = hipMemcpyAsync(q, r.src, r.bytes, hipMemcpyDeviceToHost, c.s);
        else if (c.dev)
            e = hipMemcpy(r.dst, r.src, r.bytes, hipMemcpyDeviceToHost);
        else
            std::memcpy(r.dst, r.src, r.bytes);
        if (e != hipSuccess) return e;
        if (pinned) q += slot(r.bytes);
    }
    if (!pinned) return hipSuccess;
    const hipError_t e = hipStreamSynchronize(c.s);
    if (e != hipSuccess) return e;
    q = g_pin.p;
    for (const HostRead& r : reads) {
        if (r.bytes) std::memcpy(r.dst, q, r.bytes);
        q += slot(r.bytes);
    }
    return hipSuccess;
}

static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ============================================================== 2. sin/cos in revolutions
// r in [-0.5, 0.5] revolutions -> sin(2*pi*r), cos(2*pi*r).
// Polynomial form: quarter-turn reduction y = r - q/4 (exact), |y| <= 1/8, Taylor series of
// sin/cos(2*pi*y) to degree 9/10 (truncation < 2e-9), then an exact quadrant rotation.
__device__ __forceinline__ void sincos_rev_poly(float r, float& s, float& c) {
    const float q = __builtin_rintf(4.0f * r);
    const float y = __builtin_fmaf(-0.25f, q, r);
    const float y2 = y * y;
    const float S1 = 6.28318530717958647692f, S3 = -41.3417022403997f, S5 = 81.6052492760750f,
                S7 = -76.7058597530613f, S9 = 42.0587782776566f;
    const float C2 = -19.7392088021787f, C4 = 64.9393940226683f, C6 = -85.4568172844813f,
                C8 = 60.2446397079094f, C10 = -26.4262625987960f;
    float sp = __builtin_fmaf(y2, S9, S7);
    sp = __builtin_fmaf(y2, sp, S5);
    sp = __builtin_fmaf(y2, sp, S3);
    sp = __builtin_fmaf(y2, sp, S1);
    sp *= y;
    float cp = __builtin_fmaf(y2, C10, C8);
    cp = __builtin_fmaf(y2, cp, C6);
    cp = __builtin_fmaf(y2, cp, C4);
    cp = __builtin_fmaf(y2, cp, C2);
    cp = __builtin_fmaf(y2, cp, 1.0f);
    const int iq = ((int)q) & 3;
    const float s_a = (iq & 1) ? cp : sp;
    const float c_a = (iq & 1) ? sp : cp;
    s = (iq & 2) ? -s_a : s_a;
    c = ((iq + 1) & 2) ? -c_a : c_a;
}

#include "binary_delay.h"

// ============================================================== 3. calcphase
struct CPModel {
    double pepoch;
    double coef[13];  // (1/n!) * F_{n-1}, exactly as calcphase.py:84 forms it
    int32_t nterms;   // highest n with a non-zero coefficient, at least 1 (make_cpmodel)
    int32_t parts;
    int32_t n_glitch;
    int32_t n_wave;
    double glitch[CRIMP_MAX_GLITCH][7];
    double wave_epoch, wave_om, f0;
    double wave_ab[CRIMP_MAX_WAVE][2];
};
static_assert(sizeof(CPModel) + 64 <= 4096, "CPModel is passed by value in the kernel arguments (4 KB limit)");

// The model as a kernel argument. BIN = false is CPModel alone, the layout and the code of a build without binary
// orbits; BIN = true appends the orbit, and the kernel's phase is the one at the emission time (parts bit 3).
template <bool BIN>
struct CPArgs;
template <>
struct CPArgs<false> {
    CPModel m;
};
template <>
struct CPArgs<true> {
    CPModel m;
    BinModel b;
};
static_assert(sizeof(CPArgs<false>) == sizeof(CPModel), "the non-binary kernels take CPModel as before");
static_assert(sizeof(CPArgs<true>) % 8 == 0 && sizeof(CPArgs<true>) + 64 <= 4096,
              "the model and the orbit ride in the kernel arguments (4 KB limit)");

// BIN: tau (s) is the orbital delay of t, and every part is evaluated at the emission time t - tau / 86400. tau
// enters each part in seconds after the epoch difference -- never through an emission MJD rounded to a double, which
// would cost up to 0.3 us * F0 -- and the glitch masks are taken at the emission time.
template <bool BIN>
__device__ __forceinline__ double cp_one_t(const CPModel* __restrict__ M, double t, double tau) {
    double te = 0.0;
    if (M->parts & 1) {
        // calcphase.py:80-85: te = sum_{n=1}^{13} coef_n * dt**n, summed in increasing n.
        const double dt = BIN ? (t - M->pepoch) * 86400.0 - tau : (t - M->pepoch) * 86400.0;
        double dn = dt;
        const int nt = M->nterms;
        for (int k = 0; k < nt; ++k) {
            te += M->coef[k] * dn;
            dn *= dt;
        }
    }
    double gl = 0.0;
    if (M->parts & 2) {
        // calcphase.py:98-124
        for (int j = 0; j < M->n_glitch; ++j) {
            const double* g = M->glitch[j];
            if (BIN) {
                const double dts = (t - g[0]) * 86400.0 - tau;
                if (dts >= 0.0) {
                    const double td = g[6] * 86400.0;
                    const double ex = (g[6] == 0.0) ? 0.0 : td * (1.0 - exp(-dts / td));
                    gl += (((g[1] + g[2] * dts) + (0.5 * g[3]) * (dts * dts)) +
                           ((1.0 / 6.0) * g[4]) * (dts * dts * dts)) + g[5] * ex;
                }
            } else if (t >= g[0]) {
                const double dts = (t - g[0]) * 86400.0;
                const double ex = (g[6] == 0.0) ? 0.0 : (g[6] * 86400.0) * (1.0 - exp(-(t - g[0]) / g[6]));
                gl += (((g[1] + g[2] * dts) + (0.5 * g[3]) * (dts * dts)) + ((1.0 / 6.0) * g[4]) * (dts * dts * dts)) +
                      g[5] * ex;
            }
        }
    }
    double wv = 0.0;
    if ((M->parts & 4) && M->n_wave > 0) {
        // calcphase.py:138-149
        const double dw = BIN ? (t - M->wave_epoch) - tau / 86400.0 : (t - M->wave_epoch);
        for (int j = 1; j <= M->n_wave; ++j) {
            const double arg = (j * M->wave_om) * dw;
            wv += (M->wave_ab[j - 1][0] * sin(arg)) + (M->wave_ab[j - 1][1] * cos(arg));
        }
        wv *= M->f0;
    }
    return te + gl + wv;
}

__device__ __forceinline__ double cp_one(const CPModel* __restrict__ M, double t) { return cp_one_t<false>(M, t, 0.0); }

// the phase of a kernel argument: cp_one, or (BIN) cp_one at the emission time of the model's orbit
template <bool BIN>
__device__ __forceinline__ double cp_args_one(const CPModel* __restrict__ M, const CPArgs<BIN>& A, double t) {
    if constexpr (BIN) {
        return cp_one_t<true>(M, t, bin_delay(&A.b, t));
    } else {
        return cp_one_t<false>(M, t, 0.0);
    }
}

// Two photons per thread, 16-byte loads and stores (24 B of HBM traffic per photon; non-temporal loads and
// stores measured the same, profiles/r1_final/ab_cos6_nt.log). One pair per thread over a
// grid that covers the array (up to 2^28 pairs per sweep): 5.5-5.6 TB/s at 1e8 photons, against 4.6-5.1 TB/s
// for a 4096-block grid-stride loop with 1, 2 or 4 loads in flight per thread (profiles/r1_s4/calcphase_ab.log).
template <bool BIN>
__global__ __launch_bounds__(256) void k_calcphase_vec(const double2* __restrict__ t, int64_t npair,
                                                       const CPArgs<BIN> Mv, double2* __restrict__ total,
                                                       double2* __restrict__ folded, double fscale) {
    const CPModel* M = &Mv.m;  // the model rides in the kernel arguments (no upload, no copy to the stack)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npair; i += (int64_t)gridDim.x * blockDim.x) {
        const double2 tv = t[i];
        double2 tot;
        tot.x = cp_args_one<BIN>(M, Mv, tv.x);
        tot.y = cp_args_one<BIN>(M, Mv, tv.y);
        total[i] = tot;
        if (folded) {
            double2 fo;
            fo.x = (tot.x - floor(tot.x)) * fscale;  // fscale 1 (cycles) or 2 pi (measureToAs.py:195, :200)
            fo.y = (tot.y - floor(tot.y)) * fscale;
            folded[i] = fo;
        }
    }
}

template <bool BIN>
__global__ __launch_bounds__(256) void k_calcphase_scalar(const double* __restrict__ t, int64_t n,
                                                          const CPArgs<BIN> Mv, double* __restrict__ total,
                                                          double* __restrict__ folded, double fscale) {
    const CPModel* M = &Mv.m;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double tot = cp_args_one<BIN>(M, Mv, t[i]);
        total[i] = tot;
        if (folded) folded[i] = (tot - floor(tot)) * fscale;
    }
}

// ============================================================== 4. periodicity search
// Three paths compute the per-trial harmonic sums C_k, S_k (periodsearch.py:67-69, :93-99, :120-121):
//   k_search_exact (search_exact.h, the default for arithmetic-progression grids): i8 MFMA, exact integer sums;
//   the NUFFT (search_nufft.h, opt-in CRIMP_FLAG_NUFFT, progressions of time-sorted photons): fp64 moments on
//                   the f64 matrix cores, fp64 FFT, fp64 Horner sums;
//   k_search_f64   (any grid; the default when the grid is not a progression or has < 256 trials, and the
//                   fix-up of trials the exact and NUFFT paths cannot certify): fp64 throughout.
// dt[i] = t[i] - t0 (periodsearch.py: self.time - self.t0); dt2 = dt*dt for the 2-D grid.
__global__ __launch_bounds__(256) void k_search_prep(const double* __restrict__ t, int64_t n, double t0,
                                                     double* __restrict__ dt, double* __restrict__ dt2) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double d = t[i] - t0;
        dt[i] = d;
        if (dt2) dt2[i] = d * d;
    }
}

// Direct kernels: one lane per trial, every photon of its split broadcast to the wave through the scalar
// path. Trial t of the launch is flat grid index first + (tidx ? tidx[t] : t). part layout: [split][2m][count]
// (C_k at 2(k-1), S_k at 2(k-1)+1). kSearchBlock, kSearchFold: search_plan.h.

__device__ __forceinline__ int64_t trial_index(const int64_t* __restrict__ tidx, int64_t first, int64_t t) {
    return first + (tidx ? tidx[t] : t);
}

// fp64 kernel: the reference's arithmetic precision end to end. fp64 phase reduced to a centred fractional
// cycle r, fp64 sincospi(2r) for harmonic k0 of the group, harmonics k0+1 .. k0+G-1 by fp64 angle addition,
// fp64 sums. Every term differs from np.cos(2*k*pi*f*(t-t0)) (periodsearch.py:67) by the fp64 rounding of the
// phase argument only.
template <int G, bool TWOD>
__global__ __launch_bounds__(kSearchBlock) void k_search_f64(
    const double* __restrict__ dt, const double* __restrict__ dt2, int64_t n, int64_t chunk,
    const double* __restrict__ freq, int64_t nf, const double* __restrict__ c2row, int64_t first,
    const int64_t* __restrict__ tidx, int64_t count, int k0, int ncomp, double* __restrict__ part) {
    const int64_t t = (int64_t)blockIdx.x * kSearchBlock + threadIdx.x;
    const int64_t split = blockIdx.y;
    const int64_t g = trial_index(tidx, first, t < count ? t : count - 1);
    const int64_t row = TWOD ? g / nf : 0;
    const double f = freq[g - row * nf];
    const double c2 = TWOD ? c2row[row] : 0.0;
    const double kf = (double)k0;
    const int64_t i0 = split * chunk;
    const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    double C[G], S[G];
#pragma unroll
    for (int k = 0; k < G; ++k) C[k] = S[k] = 0.0;
#pragma unroll 2
    for (int64_t i = i0; i < i1; ++i) {
        const double d = dt[i];
        const double ph = TWOD ? fma(f, d, c2 * dt2[i]) : f * d;
        double s1 = 0.0, c1 = 1.0, s, c;
        if (G > 1) sincospi(2.0 * (ph - rint(ph)), &s1, &c1);
        if (k0 == 1 && G > 1) {
            s = s1;
            c = c1;
        } else {
            const double pk = ph * kf;
            sincospi(2.0 * (pk - rint(pk)), &s, &c);
        }
        C[0] += c;
        S[0] += s;
#pragma unroll
        for (int k = 1; k < G; ++k) {
            const double cn = fma(c, c1, -s * s1);
            const double sn = fma(s, c1, c * s1);
            c = cn;
            s = sn;
            C[k] += c;
            S[k] += s;
        }
    }
    if (t < count) {
#pragma unroll
        for (int k = 0; k < G; ++k) {
            const int comp = 2 * (k0 - 1 + k);
            part[(split * ncomp + comp) * count + t] = C[k];
            part[(split * ncomp + comp + 1) * count + t] = S[k];
        }
    }
}

// Z^2 = sum_k (C_k^2 + S_k^2) * (2/n)            (periodsearch.py:67-69)
// H   = max_k (cumsum_k[(C^2+S^2)(2/n)] - 4(k-1)) (periodsearch.py:120-123)
// from fp64 per-split partial sums; out[map ? map[t] : t].
__global__ __launch_bounds__(256) void k_search_finalize(const double* __restrict__ part, int64_t count, int splits,
                                                         int m, int stat, double n, const int64_t* __restrict__ map,
                                                         double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const int ncomp = 2 * m;
    double zsum = 0.0, cum = 0.0, best = -INFINITY;
    const double w = 2.0 / n;
    for (int k = 0; k < m; ++k) {
        double c = 0.0, s = 0.0;
        for (int sp = 0; sp < splits; ++sp) {
            c += part[((int64_t)sp * ncomp + 2 * k) * count + t];
            s += part[((int64_t)sp * ncomp + 2 * k + 1) * count + t];
        }
        const double z = c * c + s * s;
        if (stat == CRIMP_STAT_Z2) {
            zsum += z;
        } else {
            cum += z * w;
            const double v = cum - 4.0 * (double)k;
            best = v > best ? v : best;
        }
    }
    out[map ? map[t] : t] = (stat == CRIMP_STAT_Z2) ? zsum * w : best;
}

#include "mfma_drain.h"
#include "f16_split.h"
#include "search_exact.h"

// ============================================================== 5. ToA likelihood scan
#include "toa_grid_plan.h"  // TplDev, the brute grid's host plan (plan_brute_grid) and its constants

constexpr int kPtsPerGroup = 4;
#ifndef CRIMP_PTS_BLOCK
#define CRIMP_PTS_BLOCK 512
#endif
constexpr int kPtsBlock = CRIMP_PTS_BLOCK;  // = kFitBlock: the device fit driver strides and reduces as k_toa_points

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

// Point coefficients of component j at phShift phi:
//   fourier   c0 = A cos(ph_j - j phi), c1 = -A sin(ph_j - j phi)
//   cauchy/vm c0 = cos(cen_j + phi),    c1 = sin(cen_j + phi)
__device__ __forceinline__ void tpl_coef(const TplDev* __restrict__ T, int j, double phi, double& c0, double& c1) {
    if (T->model == CRIMP_MODEL_FOURIER) {
        const double d = T->loc[j] - (double)(j + 1) * phi;
        c0 = T->amp[j] * cos(d);
        c1 = -T->amp[j] * sin(d);
    } else {
        const double d = T->loc[j] + phi;
        c0 = cos(d);
        c1 = sin(d);
    }
}

// sin/cos of a photon's phase: x in cycles (fourier) or radians (cauchy, von Mises)
__device__ __forceinline__ void photon_sincos(int model, double xv, double& s1, double& c1) {
    if (model == CRIMP_MODEL_FOURIER)
        sincospi(2.0 * xv, &s1, &c1);
    else
        sincos(xv, &s1, &c1);
}

// The same sin/cos from a 4096-entry fp64 table in LDS (k_toa_points and the fit kernels; CRIMP_FIT_TABLE=0 keeps
// the library sincospi / sincos): r = x in turns (x / 2 pi for radians), k = rint(4096 r), delta = 2 pi (r - k / 4096)
// (the subtraction is exact), |delta| <= pi / 4096, cos/sin(delta) by their Taylor series to delta^4 / delta^5
// (truncation < 3e-22), rotated by the table entry: ~2 ulp, against ~30 fp64 operations of the library call.
#ifndef CRIMP_FIT_TABLE
#define CRIMP_FIT_TABLE 1
#endif
constexpr int kSinTab = 4096;
__device__ __forceinline__ void sintab_fill(double2* tab) {
    for (int i = threadIdx.x; i < kSinTab; i += blockDim.x) {
        double sv, cv;
        sincospi((double)i * (2.0 / kSinTab), &sv, &cv);
        tab[i] = make_double2(cv, sv);
    }
    __syncthreads();
}
__device__ __forceinline__ void photon_sincos_tab(int model, const double2* __restrict__ tab, double xv, double& s1,
                                                  double& c1) {
    const double r = (model == CRIMP_MODEL_FOURIER) ? xv : xv * 0.15915494309189533577;
    const double k = rint(r * (double)kSinTab);
    const double d = fma(-k, 1.0 / kSinTab, r) * 6.283185307179586476925;
    const double d2 = d * d;
    const double cd = fma(d2, fma(d2, 1.0 / 24.0, -0.5), 1.0);
    const double sd = d * fma(d2, fma(d2, 1.0 / 120.0, -1.0 / 6.0), 1.0);
    const double2 e = tab[(int)(int64_t)k & (kSinTab - 1)];
    s1 = fma(e.y, cd, e.x * sd);
    c1 = fma(e.x, cd, -(e.y * sd));
}

// 1/v for the likelihood sums: v_rcp_f64 and two Newton steps (5 fp64 operations instead of the ~10 of a correctly
// rounded division; measured equal to 1/v on 2^24 values, one step alone 11 ulps, v_rcp_f64 alone 2^-24.6:
// profiles/r06/mb_rcp.txt). The fit kernels and k_toa_points use the same, so the device-driven and the
// host-driven fits sum identical terms.
__device__ __forceinline__ double lk_rcp(double v) {
    double r = __builtin_amdgcn_rcp(v);
    r = fma(fma(-v, r, 1.0), r, r);
    return fma(fma(-v, r, 1.0), r, r);
}

// h = model - norm at one photon and its first two phShift derivatives h1, h2 (templatemodels.py:64-82,
// :166-185, :271-290), from the photon's (s1, c1) and one point's coefficient rows c0[], cs[].
__device__ __forceinline__ void tpl_terms(const TplDev* __restrict__ T, int model, int K, const double* c0,
                                          const double* cs, double s1, double c1, double& h, double& h1,
                                          double& h2) {
    h = 0.0;
    h1 = 0.0;
    h2 = 0.0;
    if (model == CRIMP_MODEL_FOURIER) {
        // cos, sin of harmonic j+1 by the Chebyshev recurrence c_{j+1} = 2 c_1 c_j - c_{j-1} (one fma each instead of
        // the four operations of an angle addition; error <= ~K^2 ulp)
        const double tc = c1 + c1;
        double cj = c1, sj = s1, cp = 1.0, sp = 0.0;
        for (int j = 0; j < K; ++j) {
            const double al = c0[j], be = cs[j];
            const double tj = fma(al, cj, be * sj);
            const double jj = (double)(j + 1);
            h += tj;
            h2 = fma(-(jj * jj), tj, h2);
            h1 = fma(jj, fma(al, sj, -(be * cj)), h1);
            const double cn = fma(tc, cj, -cp), sn = fma(tc, sj, -sp);
            cp = cj;
            sp = sj;
            cj = cn;
            sj = sn;
        }
    } else {
        for (int j = 0; j < K; ++j) {
            const double C = c0[j], S = cs[j];
            const double cu = c1 * C + s1 * S;  // cos(x - cen - phi)
            const double su = s1 * C - c1 * S;  // sin(x - cen - phi)
            if (model == CRIMP_MODEL_CAUCHY) {
                const double iD = 1.0 / (T->ch[j] - cu);
                const double v = T->amp[j] * iD;  // amp' = a*sinh(w)
                const double dvdu = -v * su * iD;
                const double d2 = -v * iD * (cu - 2.0 * su * su * iD);
                h += v;
                h1 -= dvdu;
                h2 += d2;
            } else {
                const double kp = T->kap[j];
                const double v = T->amp[j] * exp(kp * cu);
                h += v;
                h1 += kp * su * v;
                h2 += (-kp * cu + kp * kp * su * su) * v;
            }
        }
    }
}

// The Fourier branch of tpl_terms for a template size fixed at compile time (the device fit kernel): the same
// per-photon operation order, coefficient rows held in registers, the harmonic loop unrolled.
template <int KF>
__device__ __forceinline__ void tpl_terms_fourier(const double (&al)[KF], const double (&be)[KF], double s1, double c1,
                                                  double& h, double& h1, double& h2) {
    // harmonic 1 starts the sums (not 0 + term: three adds per photon fewer, the same values up to the sign of zero)
    const double tc = c1 + c1;
    double cj = c1, sj = s1, cp = 1.0, sp = 0.0;
#pragma unroll
    for (int j = 0; j < KF; ++j) {
        const double tj = fma(al[j], cj, be[j] * sj);
        const double jj = (double)(j + 1);
        if (j == 0) {
            h = tj;
            h2 = -tj;
            h1 = fma(al[0], sj, -(be[0] * cj));
        } else {
            h += tj;
            h2 = fma(-(jj * jj), tj, h2);
            h1 = fma(jj, fma(al[j], sj, -(be[j] * cj)), h1);
        }
        if (j + 1 < KF) {
            const double cn = fma(tc, cj, -cp), sn = fma(tc, sj, -sp);
            cp = cj;
            sp = sj;
            cj = cn;
            sj = sn;
        }
    }
}

// h alone (no phShift derivatives), bit-identical to tpl_terms_fourier's h
template <int KF>
__device__ __forceinline__ void tpl_value_fourier(const double (&al)[KF], const double (&be)[KF], double s1, double c1,
                                                  double& h) {
    const double tc = c1 + c1;
    double cj = c1, sj = s1, cp = 1.0, sp = 0.0;
#pragma unroll
    for (int j = 0; j < KF; ++j) {
        const double tj = fma(al[j], cj, be[j] * sj);
        h = j == 0 ? tj : h + tj;
        if (j + 1 < KF) {
            const double cn = fma(tc, cj, -cp), sn = fma(tc, sj, -sp);
            cp = cj;
            sp = sj;
            cj = cn;
            sj = sn;
        }
    }
}

// One block per group of <= 4 points of one interval; lanes stride the photons. fp64.
// Coefficient table per point (LDS): fourier  a_j = A cos(ph_j - j phi), b_j = -A sin(ph_j - j phi)
//                                    cauchy/vm a_j = cos(cen_j + phi),   b_j = sin(cen_j + phi)
__global__ __launch_bounds__(kPtsBlock) void k_toa_points(const double* __restrict__ x,
                                                          const int64_t* __restrict__ offsets,
                                                          const TplDev* __restrict__ T,
                                                          const int64_t* __restrict__ grp_int,
                                                          const int64_t* __restrict__ grp_first,
                                                          const int32_t* __restrict__ grp_np,
                                                          const double* __restrict__ pt_norm,
                                                          const double* __restrict__ pt_phi, double* __restrict__ out) {
    __shared__ double coef[kPtsPerGroup][2][CRIMP_MAX_COMP];
    __shared__ double red[kPtsBlock / 64][kPtsPerGroup][8];
#if CRIMP_FIT_TABLE
    __shared__ double2 stab[kSinTab];
    sintab_fill(stab);
#endif
    const int gi = blockIdx.x;
    const int64_t iv = grp_int[gi];
    const int64_t p0 = grp_first[gi];
    const int np = grp_np[gi];
    const int model = T->model, K = T->K;
    const int tid = threadIdx.x;
    if (tid < kPtsPerGroup * K) {
        const int p = tid / K, j = tid % K;
        const double phi = p < np ? pt_phi[p0 + p] : 0.0;
        tpl_coef(T, j, phi, coef[p][0][j], coef[p][1][j]);
    }
    __syncthreads();
    double nrm[kPtsPerGroup];
#pragma unroll
    for (int p = 0; p < kPtsPerGroup; ++p) nrm[p] = p < np ? pt_norm[p0 + p] : 1.0;
    double acc[kPtsPerGroup][7];
#pragma unroll
    for (int p = 0; p < kPtsPerGroup; ++p) {
#pragma unroll
        for (int q = 0; q < 6; ++q) acc[p][q] = 0.0;
        acc[p][6] = INFINITY;
    }
    const int64_t a = offsets[iv], b = offsets[iv + 1];
    for (int64_t i = a + tid; i < b; i += kPtsBlock) {
        double s1, c1;
#if CRIMP_FIT_TABLE
        photon_sincos_tab(model, stab, x[i], s1, c1);
#else
        photon_sincos(model, x[i], s1, c1);
#endif
#pragma unroll
        for (int p = 0; p < kPtsPerGroup; ++p) {
            if (p >= np) break;
            double h, h1, h2;
            tpl_terms(T, model, K, coef[p][0], coef[p][1], s1, c1, h, h1, h2);
            const double mv = nrm[p] + h;
            const double q = lk_rcp(mv);
            acc[p][0] += log(mv);
            acc[p][1] += q;
            acc[p][2] += h1 * q;
            acc[p][3] -= q * q;
            acc[p][4] -= h1 * q * q;
            acc[p][5] += h2 * q - h1 * h1 * q * q;
            acc[p][6] = fmin(acc[p][6], mv);
        }
    }
    const int wid = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int p = 0; p < kPtsPerGroup; ++p) {
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const double v = wave_sum(acc[p][q]);
            if (lane == 0) red[wid][p][q] = v;
        }
        const double v = wave_min(acc[p][6]);
        if (lane == 0) red[wid][p][6] = v;
    }
    __syncthreads();
    if (tid < kPtsPerGroup * 7) {
        const int p = tid / 7, q = tid % 7;
        if (p < np) {
            double v = red[0][p][q];
            for (int w = 1; w < kPtsBlock / 64; ++w) v = (q == 6) ? fmin(v, red[w][p][q]) : v + red[w][p][q];
            out[(p0 + p) * 8 + q] = v;
            if (q == 0) out[(p0 + p) * 8 + 7] = (double)(b - a);
        }
    }
}

// Brute grid (fp32 model and log2, fp64 fold every 32 photons). One lane per phShift value,
// photons of a 128-photon tile broadcast from LDS; NN norms per lane. The fp32 adds, multiplies and FMAs run
// as packed pairs (v_pk_add/mul/fma_f32: two lane-ops per issue, the only way to the f32 VALU peak) -- the
// template over photon pairs, the norm products over norm pairs -- with each lane's operation order unchanged,
// so the sums are bit-identical to the scalar form.
constexpr int kGridBlock = 128;
constexpr int kGridNN = 20;
constexpr int kGridProd = 4;
constexpr int64_t kGridTarget = 16384;  // brute-grid blocks per launch (toa_grid_partials)
static_assert(kGridNN % 2 == 0 && kGridProd == 4, "norm pairs; photons in two pairs per product");
#ifndef CRIMP_GRID_MFMA
#define CRIMP_GRID_MFMA 1  // Fourier brute grid on the f16 matrix cores (k_toa_grid_mf)
#endif
#ifndef CRIMP_GRID_PPL
#define CRIMP_GRID_PPL 2
#endif
constexpr int kGridPPL = CRIMP_GRID_PPL;  // phShift values per lane of the pruned grid (k_toa_grid)

typedef float f32x2 __attribute__((ext_vector_type(2)));

// MODEL and (Fourier) the template size KF are template arguments: registers only for the model's own coefficients,
// no per-harmonic branches; KF = 0 reads K from the template at run time. NN (even, <= kGridNN) norms per lane:
// the device fit evaluates only the norms that can hold each phShift's maximum (crimp_toa_fit), usually 2.
// PPL phShift values per lane (1 or 2; the block has kGridBlock / PPL threads and always covers kGridBlock phShift
// values): with 2, every broadcast basis read feeds twice the FMAs. Each (phShift, norm) sum is formed in the same
// operation order whatever PPL, so the sums are bit-identical.
template <int KMAX, int MODEL, int KF, int NN, int PPL>
__global__ __launch_bounds__(kGridBlock) __attribute__((amdgpu_waves_per_eu(4))) void k_toa_grid(const double* __restrict__ x,
                                                         const int64_t* __restrict__ offsets,
                                                         const TplDev* __restrict__ T, const double* __restrict__ norm,
                                                         int nnorm, int a0, int na, const double* __restrict__ phi,
                                                         int nphi, int64_t chunk, int nint,
                                                         double* __restrict__ lnsum, double* __restrict__ hmin) {
    constexpr int TB = kGridBlock / PPL;  // threads per block
    // bas[pair][2j (+1)] = {photon 2 pair, photon 2 pair + 1}: cos / sin of harmonic j+1 (Fourier) or of the phase
    // (j = 0, other models). A photon pair's whole basis is 16 K contiguous bytes, read by broadcast ds_read_b128
    // (cos and sin of one harmonic for both photons) at immediate offsets from one address per pair.
    __shared__ __attribute__((aligned(16))) f32x2 bas[kGridBlock / 2][2 * KMAX];
    float* const basf = reinterpret_cast<float*>(&bas[0][0]);
    auto bset = [&](int photon, int row, float v) { basf[((photon >> 1) * 2 * KMAX + row) * 2 + (photon & 1)] = v; };
    auto bget = [&](int photon, int row) { return basf[((photon >> 1) * 2 * KMAX + row) * 2 + (photon & 1)]; };
    const int tid = threadIdx.x;
    const int64_t iv = blockIdx.y;
    const int64_t split = blockIdx.z;
    constexpr int model = MODEL;
    const int K = KF > 0 ? KF : T->K;
    int bphi[PPL];
    float ca[PPL][KMAX], cb[PPL][KMAX], amp[KMAX], chj[KMAX], kpj[KMAX];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        bphi[p] = blockIdx.x * kGridBlock + p * TB + tid;
        const double ph = phi[bphi[p] < nphi ? bphi[p] : nphi - 1];
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            ca[p][j] = cb[p][j] = 0.0f;
            if (p == 0) amp[j] = chj[j] = kpj[j] = 0.0f;
            if (j < K) {
                if (model == CRIMP_MODEL_FOURIER) {
                    const double d = T->loc[j] - (double)(j + 1) * ph;
                    ca[p][j] = (float)(T->amp[j] * cos(d));
                    cb[p][j] = (float)(-T->amp[j] * sin(d));
                } else {
                    const double d = T->loc[j] + ph;
                    ca[p][j] = (float)cos(d);
                    cb[p][j] = (float)sin(d);
                    if (p == 0) {
                        amp[j] = (float)T->amp[j];
                        chj[j] = (float)T->ch[j];
                        kpj[j] = (float)(T->kap[j] * 1.4426950408889634);  // exp(k*cu) = exp2(k*log2e*cu)
                        // von Mises: a / (2 pi I0(k)) is below fp32's range from k ~ 80 (wid < 0.11) and the whole
                        // template would read 0: carry a exp(k) / (2 pi I0(k)) = O(a sqrt k) with exp(k (cu - 1))
                        if (model == CRIMP_MODEL_VONMISES && T->amp[j] != 0.0)
                            amp[j] = (float)copysign(exp(log(fabs(T->amp[j])) + T->kap[j]), T->amp[j]);
                    }
                }
            }
        }
    }
    f32x2 nr[NN / 2];
#pragma unroll
    for (int a = 0; a < NN; ++a) nr[a / 2][a % 2] = (a < na) ? (float)norm[iv * nnorm + a0 + a] : 1.0f;
    double acc[PPL][NN];
    float hmn[PPL];
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        hmn[p] = INFINITY;
#pragma unroll
        for (int a = 0; a < NN; ++a) acc[p][a] = 0.0;
    }
    const int64_t beg = offsets[iv] + split * chunk;
    const int64_t end = std::min<int64_t>(offsets[iv + 1], beg + chunk);
    for (int64_t base = beg; base < end; base += kGridBlock) {
        const int cnt = (int)std::min<int64_t>(kGridBlock, end - base);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PPL; ++q) {
            const int ph_i = tid + q * TB;  // photon of the tile this thread fills
            if (ph_i < cnt) {
                const double xv = x[base + ph_i];
                double rv = (model == CRIMP_MODEL_FOURIER) ? xv : xv * 0.15915494309189533577;  // cycles
                rv -= rint(rv);
                float s1, c1;
                sincos_rev_poly((float)rv, s1, c1);
                if (model == CRIMP_MODEL_FOURIER) {
                    float cj = c1, sj = s1;
#pragma unroll
                    for (int j = 0; j < KMAX; ++j) {
                        bset(ph_i, 2 * j, cj);
                        bset(ph_i, 2 * j + 1, sj);
                        const float cn = __builtin_fmaf(cj, c1, -sj * s1);
                        sj = __builtin_fmaf(sj, c1, cj * s1);
                        cj = cn;
                    }
                } else {
                    bset(ph_i, 0, c1);
                    bset(ph_i, 1, s1);
                }
            }
        }
        __syncthreads();
        auto hval = [&](int p, int i) {
            float h = 0.0f;
            if (model == CRIMP_MODEL_FOURIER) {
#pragma unroll
                for (int j = 0; j < KMAX; ++j)
                    if (j < K) h = __builtin_fmaf(ca[p][j], bget(i, 2 * j), __builtin_fmaf(cb[p][j], bget(i, 2 * j + 1), h));
            } else {
                const float cx = bget(i, 0), sx = bget(i, 1);
#pragma unroll
                for (int j = 0; j < KMAX; ++j) {
                    if (j < K) {
                        const float cu = __builtin_fmaf(cx, ca[p][j], sx * cb[p][j]);
                        if (model == CRIMP_MODEL_CAUCHY)
                            h += amp[j] * __builtin_amdgcn_rcpf(chj[j] - cu);
                        else
                            h += amp[j] * __builtin_amdgcn_exp2f(__builtin_fmaf(kpj[j], cu, -kpj[j]));
                    }
                }
            }
            return h;
        };
        // photons i, i+1 (i even) for every phShift of the lane: the Fourier template as packed FMAs, same order per
        // photon as hval; one basis read serves all PPL phShifts
        auto hval2 = [&](int i, f32x2 (&h)[PPL]) {
            if (model == CRIMP_MODEL_FOURIER) {
#pragma unroll
                for (int p = 0; p < PPL; ++p) h[p] = f32x2{0.0f, 0.0f};
#pragma unroll
                for (int j = 0; j < KMAX; ++j)
                    if (j < K) {
                        const f32x2 cj = bas[i >> 1][2 * j], sj = bas[i >> 1][2 * j + 1];   // i is even
#pragma unroll
                        for (int p = 0; p < PPL; ++p)
                            h[p] = __builtin_elementwise_fma(f32x2{ca[p][j], ca[p][j]}, cj,
                                                             __builtin_elementwise_fma(f32x2{cb[p][j], cb[p][j]}, sj, h[p]));
                    }
            } else {
#pragma unroll
                for (int p = 0; p < PPL; ++p) h[p] = f32x2{hval(p, i), hval(p, i + 1)};
            }
        };
        for (int i0 = 0; i0 < cnt; i0 += 32) {
            f32x2 pa[PPL][NN / 2];
#pragma unroll
            for (int p = 0; p < PPL; ++p)
#pragma unroll
                for (int a = 0; a < NN / 2; ++a) pa[p][a] = f32x2{0.0f, 0.0f};
            const int i1 = std::min(cnt, i0 + 32);
            int i = i0;
            // log2 of a product of kGridProd model values instead of kGridProd logs (v_log issues at quarter
            // rate): one photon costs an add and a multiply per norm plus 1/kGridProd of a log and an add.
            // Four factors of (norm + h) <= 2^31 cannot overflow fp32; the product adds <= 3 roundings.
            for (; i + kGridProd <= i1; i += kGridProd) {
                f32x2 h01[PPL], h23[PPL];
                hval2(i, h01);
                hval2(i + 2, h23);
#pragma unroll
                for (int p = 0; p < PPL; ++p) {
                    hmn[p] = fminf(fminf(fminf(fminf(hmn[p], h01[p].x), h01[p].y), h23[p].x), h23[p].y);
#pragma unroll
                    for (int b = 0; b < NN / 2; ++b) {
                        f32x2 pr = nr[b] + h01[p].x;
                        pr *= nr[b] + h01[p].y;
                        pr *= nr[b] + h23[p].x;
                        pr *= nr[b] + h23[p].y;
                        pa[p][b] += f32x2{__builtin_amdgcn_logf(pr.x), __builtin_amdgcn_logf(pr.y)};
                    }
                }
            }
            for (; i < i1; ++i) {
#pragma unroll
                for (int p = 0; p < PPL; ++p) {
                    const float h = hval(p, i);
                    hmn[p] = fminf(hmn[p], h);
#pragma unroll
                    for (int b = 0; b < NN / 2; ++b) {
                        const f32x2 pr = nr[b] + h;
                        pa[p][b] += f32x2{__builtin_amdgcn_logf(pr.x), __builtin_amdgcn_logf(pr.y)};
                    }
                }
            }
#pragma unroll
            for (int p = 0; p < PPL; ++p)
#pragma unroll
                for (int a = 0; a < NN; ++a) acc[p][a] += (double)pa[p][a / 2][a % 2];
        }
    }
#pragma unroll
    for (int p = 0; p < PPL; ++p) {
        if (bphi[p] < nphi) {
#pragma unroll
            for (int a = 0; a < NN; ++a)
                if (a < na) lnsum[((split * nint + iv) * nnorm + a0 + a) * nphi + bphi[p]] = acc[p][a];
            if (a0 == 0) hmin[(split * nint + iv) * nphi + bphi[p]] = (double)hmn[p];
        }
    }
}

// Brute grid of a Fourier template on the f16 matrix cores (the default for Fourier templates of <= 8 harmonics;
// CRIMP_GRID_MFMA=0 builds the VALU kernel above for them too). The template part of every (photon, phShift)
// point is a product of the photon's basis (cos jx, sin jx) and the phShift's coefficients (a_j, b_j):
// h = sum_j a_j cos jx + b_j sin jx, i.e. one (32 photons x 2K) . (2K x 32 phShifts) matrix product per tile. Each
// fp32 factor is carried as hi + lo f16 (f16_split.h split_xy; |x - hi - lo| <= 2^-22 |x|) and the four exact
// products hi.hi, hi.lo, lo.hi, lo.lo of each term fill K = 8 per harmonic of v_mfma_f32_32x32x16_f16 (two harmonics
// per instruction, fp32 accumulation). The VALU is left with the likelihood part: per point and evaluated norm an
// add, 3/4 of a multiply and 1/4 of a v_log_f32 (log2 of products of 4 photons, as k_toa_grid), and the min -- or,
// on crimp_toa_fit's certified modes, 7/8 of a multiply and 1/8 of a log (PROD 8), no add (CIN: the accumulators
// start at the norm) and no min (HMIN false).
// Block: 4 waves, wave w owns the 32 phShift columns 128 bx + 32 w + (lane & 31); a kGmTile-photon tile's A fragments
// (per photon and harmonic 16 bytes: hi, hi, lo, lo of cos then of sin) are built once per tile in LDS by the whole
// block. MFMA result i of lane l is photon (i & 3) + 8 (i >> 2) + 4 (l >> 5) of the 32-photon chunk, phShift column
// l & 31, so each lane multiplies 4 consecutive photons per group; the two lane halves' sums of a column are added
// (half 0 + half 1) at the end. fp64 folds every 32-photon chunk; deterministic, not bit-identical to k_toa_grid.
// Scale: the coefficients and the norms enter multiplied by s = 2^se (grid_mf_scale: the largest amplitude brought into
// [1, 4096] when it lies outside), so that faint templates keep the split's 2^-22 relative accuracy (a lo part below
// 2^-14 would be an f16 subnormal) and bright ones cannot overflow f16; every factor norm + h is then s (norm + h)
// exactly, so the log2 sums lose se per photon (subtracted exactly at the end) and min h is hmn / s. se = 0 (the
// amplitudes already in range, e.g. the bundled template) is the unscaled kernel, bit for bit.
// Tile: CRIMP_GM_TILE photons per LDS tile, built by the block's 256 threads -- 256: one thread per photon computes all
// of its harmonics (one sin/cos and one recurrence per photon); 128 (round 3): two threads per photon, each storing
// half of the harmonics but running the recurrence up to its own. Each photon row has one spare 16-byte slot
// (kGmPad): the 16 lanes of a b128 read pass take 16 consecutive rows, whose start banks are then 16 distinct
// multiples of 4 (row strides of 3, 5, 7, 9 slots for K <= 2, 4, 6, 8; without the pad 2, 4, 6, 8 slots put 2-8 rows
// on the same banks).
#ifndef CRIMP_GM_TILE
#define CRIMP_GM_TILE 256
#endif
#ifndef CRIMP_GM_PAD
#define CRIMP_GM_PAD 1
#endif
// CRIMP_GM_CIN: with one evaluated norm on the eight-factor kernel, the MFMA accumulators start at s norm instead of 0,
// so the matrix cores return the factors s (norm + h) themselves (no add per point; the min h is then
// min(s (norm + h)) - s norm, exact in fp64). The factor is the MFMA's fp32 sum with the norm inside instead of
// fl(norm + fl(h)): rounding-level changes of the lattice LL, held to the full kernel's brute argmax by the tests.
#ifndef CRIMP_GM_CIN
#define CRIMP_GM_CIN 1
#endif
// CRIMP_GM_PREF: each thread loads its photon of the next tile right after building the current one, so the global
// load's latency passes under the current tile's chunks instead of stalling every wave of the block at the build.
// (1.85 -> 1.82 ms per 1250 config-5 grids, profiles/r04/ab_toa_pipe.log.) Measured, rejected and removed: a wave
// issuing the next chunk's MFMAs before the VALU work on the current chunk's results (1.88 ms, the same log): the
// five resident waves per SIMD already overlap one wave's MFMAs with another's VALU work.
#ifndef CRIMP_GM_PREF
#define CRIMP_GM_PREF 1
#endif
constexpr int kGmTile = CRIMP_GM_TILE, kGmPad = CRIMP_GM_PAD;
static_assert(kGmTile == 128 || kGmTile == 256, "k_toa_grid_mf: one or two of the block's 256 threads per photon");
static_assert(kGridBlock == 32 * 4, "k_toa_grid_mf: 4 waves of 32 phShift columns cover a block's kGridBlock columns");
// HMIN: track min h per phShift (the public crimp_toa_grid; the device fit skips it when the template's lower bound
// already keeps every evaluated norm + h positive, k_toa_grid_best then takes that bound). PROD: model values per log2
// (4, or 8 when the host has checked that a product of eight factors stays a normal fp32, grid_prod8_ok): the min is
// ~29 % and the logs ~15 % of the likelihood part's VALU.
template <int KF, int NN, bool HMIN = true, int PROD = 4>
__global__ __launch_bounds__(256) void k_toa_grid_mf(const double* __restrict__ x, const int64_t* __restrict__ offsets,
                                                     const TplDev* __restrict__ T, const double* __restrict__ norm,
                                                     int nnorm, int a0, int na, const double* __restrict__ phi, int nphi,
                                                     int64_t chunk, int nint, int se, int a_first,
                                                     double* __restrict__ lnsum, double* __restrict__ hmin) {
    constexpr int NM = (KF + 1) / 2;  // MFMAs per 32-photon chunk (two harmonics each)
    __shared__ __attribute__((aligned(16))) u32x4 afr[kGmTile][2 * NM + kGmPad];  // [photon][harmonic]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, hk = lane >> 5;
    const int64_t iv = blockIdx.y, split = blockIdx.z;
    const int bphi = blockIdx.x * kGridBlock + 32 * wv + (lane & 31);
    const double sc = ldexp(1.0, se);
    // B fragments: the lane's phShift coefficients of harmonics 2m + hk + 1 (zero past K)
    f16x8 bf[NM];
    {
        const double ph = phi[bphi < nphi ? bphi : nphi - 1];
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            const int j = 2 * m + hk;
            float ca = 0.0f, cb = 0.0f;
            if (j < KF) {
                const double d = T->loc[j] - (double)(j + 1) * ph;
                ca = (float)(T->amp[j] * cos(d) * sc);
                cb = (float)(-T->amp[j] * sin(d) * sc);
            }
            uint32_t dh, dl;
            split_xy<false>(ca, cb, dh, dl);
            const uint32_t wc = (dh & 0xffffu) | (dl << 16), ws = (dh >> 16) | (dl & 0xffff0000u);
            const u32x4 w = {wc, wc, ws, ws};
            bf[m] = __builtin_bit_cast(f16x8, w);
        }
    }
    // PROD 4: the norms in pairs (f32x2 over two norms); PROD 8: one norm at a time over photon pairs (f32x2 over two
    // photons), so that an odd number of norms (a single one after k_toa_grid_best's lazy norms) costs no dead lane
    constexpr int NP = NN > 1 ? NN / 2 : 1;
    constexpr bool CIN = CRIMP_GM_CIN && PROD == 8 && NN == 1;
    f32x2 nr[NP];
    float nrs[NN];
#pragma unroll
    for (int a = 0; a < NN; ++a) {
        nrs[a] = (a < na) ? (float)(norm[iv * nnorm + a0 + a] * sc) : 1.0f;
        nr[a / 2][a % 2] = nrs[a];
    }
    if (NN == 1) nr[0][1] = 1.0f;
    double acc[NN];
#pragma unroll
    for (int a = 0; a < NN; ++a) acc[a] = 0.0;
    float hmn = INFINITY;
    const int64_t beg = offsets[iv] + split * chunk;
    const int64_t end = std::min<int64_t>(offsets[iv + 1], beg + chunk);
    const int pt = tid & (kGmTile - 1);  // this thread's photon of a tile
    double xpre = (CRIMP_GM_PREF && beg + pt < end) ? x[beg + pt] : 0.0;
    for (int64_t base = beg; base < end; base += kGmTile) {
        const int cnt = (int)std::min<int64_t>(kGmTile, end - base);
        __syncthreads();
        {   // A fragments: thread (photon p = tid % kGmTile, part g = tid / kGmTile) builds harmonics [g JP, (g+1) JP)
            constexpr int JP = kGmTile == 256 ? 2 * NM : 4;
            const int p = pt, g = kGmTile == 256 ? 0 : tid >> 7;
            float c1 = 1.0f, s1 = 0.0f;
            if (p < cnt) {
                double rv = CRIMP_GM_PREF ? xpre : x[base + p];
                rv -= rint(rv);
                sincos_rev_poly((float)rv, s1, c1);
            }
            if (CRIMP_GM_PREF) xpre = base + kGmTile + p < end ? x[base + kGmTile + p] : 0.0;
            float cj = c1, sj = s1;
#pragma unroll
            for (int j = 0; j < 2 * NM; ++j) {
                if (j >= JP * g && j < JP * g + JP) {
                    uint32_t dh, dl;
                    split_xy<false>(cj, sj, dh, dl);
                    // {hi, hi}, {lo, lo} of cos (low halves of dh, dl), then of sin (high halves): one v_perm each
                    afr[p][j] = u32x4{__builtin_amdgcn_perm(dh, dh, 0x01000100u), __builtin_amdgcn_perm(dl, dl, 0x01000100u),
                                      __builtin_amdgcn_perm(dh, dh, 0x03020302u), __builtin_amdgcn_perm(dl, dl, 0x03020302u)};
                }
                const float cn = __builtin_fmaf(cj, c1, -sj * s1);
                sj = __builtin_fmaf(sj, c1, cj * s1);
                cj = cn;
            }
        }
        __syncthreads();
        // one 32-photon chunk's template part (32 photons x the wave's 32 phShift columns) on the matrix cores
        auto chunk_mfma = [&](int q0) -> f32x16 {
            f32x16 h = {};
            if constexpr (CIN) {
#pragma unroll
                for (int r = 0; r < 16; ++r) h[r] = nrs[0];
            }
#pragma unroll
            for (int m = 0; m < NM; ++m) {
                const f16x8 av = __builtin_bit_cast(f16x8, afr[q0 + (lane & 31)][2 * m + hk]);
                h = __builtin_amdgcn_mfma_f32_32x32x16_f16(av, bf[m], h, 0, 0, 0);
            }
            return h;
        };
        // the likelihood part of one chunk on the VALU (hv: the chunk's MFMA results)
        auto chunk_valu = [&](const f32x16& hv, int q0) {
            if constexpr (PROD == 8) {
                // photon pairs: per norm, the 16 factors norm + h of the lane's chunk as 8 f32x2, multiplied down a tree
                // to two products of eight (even and odd photons), one v_log_f32 each
                f32x2 pl[NN];
#pragma unroll
                for (int b = 0; b < NN; ++b) pl[b] = f32x2{0.0f, 0.0f};
                if (q0 + 32 <= cnt) {
                    if constexpr (HMIN) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) hmn = fminf(hmn, hv[r]);
                    }
#pragma unroll
                    for (int b = 0; b < NN; ++b) {
                        const f32x2 n2 = f32x2{nrs[b], nrs[b]};
                        f32x2 f[8];
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            f[k] = f32x2{hv[2 * k], hv[2 * k + 1]};
                            if constexpr (!CIN) f[k] += n2;
                        }
                        f[0] *= f[1];
                        f[2] *= f[3];
                        f[4] *= f[5];
                        f[6] *= f[7];
                        f[0] *= f[2];
                        f[4] *= f[6];
                        f[0] *= f[4];
                        pl[b] += f32x2{__builtin_amdgcn_logf(f[0].x), __builtin_amdgcn_logf(f[0].y)};
                    }
                } else {  // the tile's last, partial chunk: photons past cnt contribute a factor 1 (products of four)
#pragma unroll
                    for (int gi = 0; gi < 4; ++gi) {
                        float pr[NN];
#pragma unroll
                        for (int b = 0; b < NN; ++b) pr[b] = 1.0f;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = q0 + r + 8 * gi + 4 * hk;
                            if (row < cnt) {
                                const float h = hv[4 * gi + r];
                                if constexpr (HMIN) hmn = fminf(hmn, h);
#pragma unroll
                                for (int b = 0; b < NN; ++b) pr[b] *= CIN ? h : nrs[b] + h;
                            }
                        }
#pragma unroll
                        for (int b = 0; b < NN; ++b) pl[b].x += __builtin_amdgcn_logf(pr[b]);
                    }
                }
#pragma unroll
                for (int a = 0; a < NN; ++a) acc[a] += (double)pl[a].x + (double)pl[a].y;
                return;
            }
            f32x2 pa[NP];
#pragma unroll
            for (int b = 0; b < NP; ++b) pa[b] = f32x2{0.0f, 0.0f};
            if (q0 + 32 <= cnt) {
#pragma unroll
                for (int gi = 0; gi < 4; ++gi) {
                    if constexpr (HMIN) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) hmn = fminf(hmn, hv[4 * gi + r]);
                    }
#pragma unroll
                    for (int b = 0; b < NP; ++b) {
                        f32x2 pr = nr[b] + hv[4 * gi];
#pragma unroll
                        for (int r = 1; r < 4; ++r) pr *= nr[b] + hv[4 * gi + r];
                        pa[b] += f32x2{__builtin_amdgcn_logf(pr.x), __builtin_amdgcn_logf(pr.y)};
                    }
                }
            } else {  // the tile's last, partial chunk: photons past cnt contribute a factor 1
#pragma unroll
                for (int gi = 0; gi < 4; ++gi) {
                    f32x2 pr[NP];
#pragma unroll
                    for (int b = 0; b < NP; ++b) pr[b] = f32x2{1.0f, 1.0f};
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = q0 + r + 8 * gi + 4 * hk;
                        if (row < cnt) {
                            const float h = hv[4 * gi + r];
                            if constexpr (HMIN) hmn = fminf(hmn, h);
#pragma unroll
                            for (int b = 0; b < NP; ++b) pr[b] *= nr[b] + h;
                        }
                    }
#pragma unroll
                    for (int b = 0; b < NP; ++b)
                        pa[b] += f32x2{__builtin_amdgcn_logf(pr[b].x), __builtin_amdgcn_logf(pr[b].y)};
                }
            }
#pragma unroll
            for (int a = 0; a < NN; ++a) acc[a] += (double)pa[a / 2][a % 2];
        };
        for (int q0 = 0; q0 < cnt; q0 += 32) chunk_valu(chunk_mfma(q0), q0);
    }
    // the column's two lane halves: half 0 + half 1
#pragma unroll
    for (int a = 0; a < NN; ++a) {
        const double o = __shfl_xor(acc[a], 32);
        acc[a] = hk == 0 ? acc[a] + o : o + acc[a];
    }
    hmn = fminf(hmn, __shfl_xor(hmn, 32));
    if (se != 0) {  // every photon's factor carried s = 2^se: log2 s per photon of the split, exactly
        const double drop = (double)se * (double)(end > beg ? end - beg : 0);
#pragma unroll
        for (int a = 0; a < NN; ++a) acc[a] -= drop;
    }
    if (hk == 0 && bphi < nphi) {
#pragma unroll
        for (int a = 0; a < NN; ++a)
            if (a < na) lnsum[((split * nint + iv) * nnorm + a0 + a) * nphi + bphi] = acc[a];
        // the first evaluated norm block writes the min (a_first: past toa_grid_partials' lazy norms)
        if (HMIN && a0 == a_first)
            hmin[(split * nint + iv) * nphi + bphi] = ldexp(CIN ? (double)hmn - (double)nrs[0] : (double)hmn, -se);
    }
}

// np.histogram(x, bins=edges) for uniform edges (numpy/lib/_histograms_impl.py semantics).
// Per-interval phase histogram (np.histogram semantics, binphases.py). Block (iv, y) of a (nint, ns) grid counts
// photons offsets[iv] + 256 y + tid + k 256 ns into one LDS histogram per wave (4-way fewer LDS atomic collisions
// than one per block, the bins being few), then adds its bins to the zeroed int64 counts: integer sums, so the split
// into ns blocks per interval cannot change a count. (One 256-thread block per interval with one shared histogram:
// 0.6 ms for config 5's 1250 x 1e5 photons, ~1.7 TB/s.)
constexpr int kBinWaves = 4;
constexpr int kBinRegs = 16;
__global__ __launch_bounds__(64 * kBinWaves) void k_binphases(const double* __restrict__ x,
                                                              const int64_t* __restrict__ offsets,
                                                              const double* __restrict__ edges, int nb,
                                                              unsigned long long* __restrict__ counts) {
    __shared__ unsigned int cnt[kBinWaves][256];
    __shared__ double se[257];
    const int64_t iv = blockIdx.x;
    const int tid = threadIdx.x, w = tid >> 6;
    for (int b = tid; b < kBinWaves * 256; b += blockDim.x) cnt[b >> 8][b & 255] = 0;
    for (int b = tid; b <= nb; b += blockDim.x) se[b] = edges[b];
    __syncthreads();
    const double first = se[0], last = se[nb];
    const double scale = (double)nb / (last - first);
    // np.histogram's bin: the estimate floor((v - first) / (last - first) * nb), then its two corrections against the
    // edges (v below its left edge: one down; at or above its right edge, unless the last bin: one up). Any estimate
    // within one bin of the true one ends on the same bin, so the product with the reciprocal (a few ulps from numpy's
    // quotient) gives numpy's counts without an fp64 division per photon.
    auto bin = [&](double v) -> int {
        int idx = (int)((v - first) * scale);
        idx = idx < nb ? idx : nb - 1;
        if (v < se[idx]) idx -= 1;
        if (idx != nb - 1 && v >= se[idx + 1]) idx += 1;
        return idx;
    };
    const int64_t stride = (int64_t)blockDim.x * gridDim.y;
    const int64_t beg = offsets[iv] + (int64_t)blockIdx.y * blockDim.x + tid, end = offsets[iv + 1];
    if (nb <= kBinRegs) {
        // up to kBinRegs bins (measuretoas' default 15): per-thread 8-bit counters, bins 0-7 in lo and 8-15 in hi
        // (one shift and a 64-bit add per photon), moved to 32-bit registers every 32 iterations of two photons (a
        // byte holds 64 at most), added to the wave's LDS histogram once at the end
        uint32_t rc[kBinRegs];
#pragma unroll
        for (int b = 0; b < kBinRegs; ++b) rc[b] = 0;
        uint64_t lo = 0, hi = 0;
        int pend = 0;
        auto count = [&](double v) {
            if (!(v >= first && v <= last)) return;
            const int idx = bin(v);
            const uint64_t one = 1ull << (8 * (idx & 7));
            lo += idx < 8 ? one : 0ull;
            hi += idx < 8 ? 0ull : one;
        };
        auto flush = [&]() {
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                rc[b] += (uint32_t)(lo >> (8 * b)) & 0xffu;
                rc[b + 8] += (uint32_t)(hi >> (8 * b)) & 0xffu;
            }
            lo = hi = 0;
            pend = 0;
        };
        for (int64_t i = beg; i < end; i += 2 * stride) {
            const double v0 = x[i];
            const double v1 = i + stride < end ? x[i + stride] : NAN;
            count(v0);
            count(v1);
            if (++pend == 32) flush();
        }
        flush();
#pragma unroll
        for (int b = 0; b < kBinRegs; ++b)
            if (rc[b]) atomicAdd(&cnt[w][b], rc[b]);
    } else {
        for (int64_t i = beg; i < end; i += stride) {
            const double v = x[i];
            if (v >= first && v <= last) atomicAdd(&cnt[w][bin(v)], 1u);
        }
    }
    __syncthreads();
    for (int b = tid; b < nb; b += blockDim.x) {
        unsigned long long c = 0;
#pragma unroll
        for (int k = 0; k < kBinWaves; ++k) c += cnt[k][b];
        if (c) atomicAdd(&counts[iv * nb + b], c);
    }
}

// photon splits per interval for k_binphases: about 8 blocks per CU over the whole call, at least 4096 photons per block
static int64_t bin_splits(int64_t ntot, int64_t nint) {
    const int64_t per = (ntot + nint - 1) / nint;
    return std::max<int64_t>(1, std::min<int64_t>({(2048 + nint - 1) / nint, (per + 4095) / 4096, 65535}));
}

// redChi2 of every fitted interval on the device (measureToAs.py:385-393 and the Cauchy / von Mises copies): against
// binphases' histogram (k_binphases, np.histogram semantics) the best-fit template curve at the bin centres;
// chi2 = sum_b (model_b - rate_b)^2 / err_b^2 with rate = cts / (E / nbins), err = sqrt(cts) / (E / nbins) (numpy's
// division: an empty bin gives inf, or nan where the model is 0 too), summed in bin order, redChi2 = chi2 / (nbins -
// nfree). One 64-thread block per interval; rec = the fit records (norm [0], phShift [1], ampShift [6]).
__global__ __launch_bounds__(64) void k_toa_chi2(const unsigned long long* __restrict__ counts, const TplDev T,
                                                 const double* __restrict__ expo, const double* __restrict__ rec,
                                                 const double* __restrict__ centers, int nb, int nfree,
                                                 double* __restrict__ out) {
    __shared__ double term[256];
    const int64_t iv = blockIdx.x;
    const double n = rec[iv * 8], ph = rec[iv * 8 + 1], A = rec[iv * 8 + 6];
    const double w = expo[iv] / (double)nb;
    for (int b = threadIdx.x; b < nb; b += 64) {
        const double xx = centers[b];
        double y = n;  // toafit.ToAFitter.curve: fourseries / wrapcauchy / vonmises (templatemodels.py:64-82, :166-185,
                       // :271-290); Fourier by angle subtraction as the host formed it
        for (int j = 0; j < T.K; ++j) {
            if (T.model == CRIMP_MODEL_FOURIER) {
                const double ang = (double)(j + 1) * 2.0 * M_PI * xx + T.loc[j], bph = (double)(j + 1) * ph;
                y = y + T.amp[j] * A * (cos(ang) * cos(bph) + sin(ang) * sin(bph));
            } else if (T.model == CRIMP_MODEL_CAUCHY) {
                y = y + T.amp[j] * A / (T.ch[j] - cos(xx - T.loc[j] - ph));
            } else {
                y = y + T.amp[j] * A * exp(T.kap[j] * cos(xx - T.loc[j] - ph));
            }
        }
        const double c = (double)counts[iv * nb + b];
        const double rate = c / w, err = sqrt(c) / w;
        term[b] = ((y - rate) * (y - rate)) / (err * err);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double chi2 = 0.0;
        for (int b = 0; b < nb; ++b) chi2 += term[b];
        out[iv] = chi2 / (double)(nb - nfree);
    }
}

// Many independent one-trial searches (measureToAs.py:210-212: PeriodSearch(TIME_toa*86400, [f(ToA_mid)], 5).htest()
// per interval): set i is t[offsets[i] : offsets[i+1]] with its own t0 = (t[first] + t[last])/2 (periodsearch.py:54)
// and trial frequency freq[i]. One block per set; fp64 as k_search_f64 (harmonic groups of 8 from exact phases,
// fp64 angle addition inside a group), block-reduced fp64 sums, statistic in the reference's formula order.
constexpr int kSetBlock = 256;
__global__ __launch_bounds__(kSetBlock) void k_search_sets(const double* __restrict__ t,
                                                           const int64_t* __restrict__ offsets,
                                                           const double* __restrict__ freq, int m, int stat,
                                                           double tscale, double* __restrict__ out) {
#pragma clang fp contract(off)  // t * tscale rounded before the subtraction, as the host's TIME_toa * 86400
    __shared__ double red[kSetBlock / 64][16];
    const int64_t set = blockIdx.x;
    const int64_t a = offsets[set], b = offsets[set + 1];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // tscale 1 (seconds) or 86400 (days: the reference's TIME_toa * 86400, measureToAs.py:211, in the same multiply)
    const double t0 = (t[a] * tscale + t[b - 1] * tscale) / 2;
    const double f = freq[set];
    const double w = 2.0 / (double)(b - a);
    double zsum = 0.0, cum = 0.0, best = -INFINITY;
    for (int k0 = 1; k0 <= m; k0 += 8) {
        const int G = m - k0 + 1 < 8 ? m - k0 + 1 : 8;
        double C[8], S[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) C[k] = S[k] = 0.0;
        for (int64_t i = a + tid; i < b; i += kSetBlock) {
            const double ph = f * (t[i] * tscale - t0);
            double s1, c1, s, c;
            sincospi(2.0 * (ph - rint(ph)), &s1, &c1);
            if (k0 == 1) {
                s = s1;
                c = c1;
            } else {
                const double pk = ph * (double)k0;
                sincospi(2.0 * (pk - rint(pk)), &s, &c);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k < G) {
                    C[k] += c;
                    S[k] += s;
                    const double cn = fma(c, c1, -s * s1);
                    s = fma(s, c1, c * s1);
                    c = cn;
                }
            }
        }
        for (int k = 0; k < G; ++k) {
            const double cw = wave_sum(C[k]), sw = wave_sum(S[k]);
            if (lane == 0) {
                red[wid][2 * k] = cw;
                red[wid][2 * k + 1] = sw;
            }
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < G; ++k) {
                double c = 0.0, s = 0.0;
                for (int q = 0; q < kSetBlock / 64; ++q) {
                    c += red[q][2 * k];
                    s += red[q][2 * k + 1];
                }
                const double z = c * c + s * s;
                if (stat == CRIMP_STAT_Z2) {
                    zsum += z;
                } else {
                    cum += z * w;
                    const double v = cum - 4.0 * (double)(k0 - 1 + k);
                    best = v > best ? v : best;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) out[set] = (stat == CRIMP_STAT_Z2) ? zsum * w : best;
}

// fp64 fix-up of a few trials over many photons (the exact path's flagged trials): block (t, split) sums the
// harmonics k0 .. k0+G-1 of trial tidx[t] over photons of its split with fp64 sincospi of the exact phase of k0 and
// fp64 angle addition (as k_search_f64), reduced across the block in a fixed order into part[split][2m][count].
template <int G, bool TWOD>
__global__ __launch_bounds__(kFixBlock) void k_search_f64_few(
    const double* __restrict__ dt, const double* __restrict__ dt2, int64_t n, int64_t chunk,
    const double* __restrict__ freq, int64_t nf, const double* __restrict__ c2row, int64_t first,
    const int64_t* __restrict__ tidx, int64_t count, int k0, int ncomp, double* __restrict__ part) {
    __shared__ double red[kFixBlock / 64][2 * G];
    const int64_t t = blockIdx.x;
    const int64_t split = blockIdx.y;
    const int64_t g = first + tidx[t];
    const int64_t row = TWOD ? g / nf : 0;
    const double f = freq[g - row * nf];
    const double c2 = TWOD ? c2row[row] : 0.0;
    const int64_t i0 = split * chunk;
    const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    double C[G], S[G];
#pragma unroll
    for (int k = 0; k < G; ++k) C[k] = S[k] = 0.0;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kFixBlock) {
        const double ph = TWOD ? fma(f, dt[i], c2 * dt2[i]) : f * dt[i];
        double s1 = 0.0, c1 = 1.0, s, c;
        if (G > 1) sincospi(2.0 * (ph - rint(ph)), &s1, &c1);
        if (k0 == 1 && G > 1) {
            s = s1;
            c = c1;
        } else {
            const double pk = ph * (double)k0;
            sincospi(2.0 * (pk - rint(pk)), &s, &c);
        }
#pragma unroll
        for (int k = 0; k < G; ++k) {
            C[k] += c;
            S[k] += s;
            const double cn = fma(c, c1, -s * s1);
            s = fma(s, c1, c * s1);
            c = cn;
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        const double cw = wave_sum(C[k]), sw = wave_sum(S[k]);
        if (lane == 0) {
            red[wid][2 * k] = cw;
            red[wid][2 * k + 1] = sw;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * G) {
        double v = 0.0;
        for (int w = 0; w < kFixBlock / 64; ++w) v += red[w][threadIdx.x];
        part[(split * ncomp + 2 * (k0 - 1) + threadIdx.x) * count + t] = v;
    }
}

#include "toa_fit.h"
#include "toa_shape.h"
#include "phase_cube.h"
#include "stretch_move.h"
#include "timing_fit.h"
#include "orbit_fit.h"
#include "sim_events.h"
#include "photon_fit.h"
#include "photon_orbit_fit.h"

// ============================================================== 6. C-ABI
// A second stream per device for crimp_toa_fit's overlapped halves (created once, kept for the process)
static hipStream_t aux_stream() {
    static hipStream_t st[64] = {};
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return nullptr;
    if (!st[d] && hipStreamCreateWithFlags(&st[d], hipStreamNonBlocking) != hipSuccess) st[d] = nullptr;
    return st[d];
}

extern "C" double crimp_last_kernel_ms(void) { return g_last_kernel_ms; }

extern "C" int crimp_last_kernel_times(double* ms, int32_t cap) {
    const int n = (int)g_kernel_times.size();
    for (int i = 0; i < n && i < cap; ++i) ms[i] = g_kernel_times[(size_t)i];
    return n;
}

extern "C" int crimp_version(void) { return CRIMP_VERSION; }

extern "C" int64_t crimp_last_fixups(void) { return g_last_fixups; }
extern "C" int64_t crimp_last_toa_grid_norms(void) { return g_last_grid_norms; }
extern "C" int64_t crimp_last_toa_grid_fast(void) { return g_last_grid_fast; }

extern "C" int crimp_release_scratch(void) {
    std::lock_guard<std::mutex> lk(g_mutex);
    release_idle_blocks(-1);
    return CRIMP_OK;
}

extern "C" const char* crimp_last_error(void) { return g_err.c_str(); }

extern "C" int crimp_device_count(int32_t* count) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (count) *count = (e == hipSuccess) ? n : 0;
    if (e != hipSuccess) return set_err(CRIMP_ERR_NODEV, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    return CRIMP_OK;
}

static int finish(hipStream_t s, uint32_t flags) {
    (void)flags;
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));  // every call returns with its stream drained (scratch reuse)
    return CRIMP_OK;
}

// the kernels' form of a timing model (crimp_calcphase and the fused crimp_phase_cube share it, coefficient for
// coefficient)
static void make_cpmodel(const crimp_timing_model* model, int32_t parts, CPModel* out) {
    CPModel& hm = *out;
    hm.pepoch = model->pepoch;
    hm.nterms = 0;
    double fact = 1.0;
    for (int k = 0; k < 13; ++k) {
        fact *= (double)(k + 1);
        hm.coef[k] = (1.0 / fact) * model->f[k];
        if (model->f[k] != 0.0) hm.nterms = k + 1;
    }
    // with every F zero the first term stays: 0 * dt adds nothing to a finite time and carries a NaN time into the
    // total as the reference's 0 * NaN does (no comparison t >= GLEP is true for a NaN, so the glitch sum alone is 0)
    if (hm.nterms == 0) hm.nterms = 1;
    hm.parts = parts;
    hm.n_glitch = model->n_glitch;
    std::memcpy(hm.glitch, model->glitch, sizeof(hm.glitch));
    hm.n_wave = model->n_wave;
    hm.wave_epoch = model->wave_epoch;
    hm.wave_om = model->wave_om;
    hm.f0 = model->f[0];
    std::memcpy(hm.wave_ab, model->wave_ab, sizeof(hm.wave_ab));
}

// the limits of a model's binary orbit (include/crimp_hip.h: crimp_binary_delay); none set is fine
static int check_binary(const crimp_timing_model* m) {
    if (m->binary == CRIMP_BINARY_NONE) return CRIMP_OK;
    ARGCHK(m->binary == CRIMP_BINARY_BT || m->binary == CRIMP_BINARY_ELL1,
           "binary must be CRIMP_BINARY_NONE, CRIMP_BINARY_BT or CRIMP_BINARY_ELL1");
    const bool bt = m->binary == CRIMP_BINARY_BT;
    ARGCHK(std::isfinite(m->bin_pb) && std::isfinite(m->bin_pbdot) && std::isfinite(m->bin_a1) &&
               std::isfinite(m->bin_a1dot) && std::isfinite(m->bin_t0) && std::isfinite(m->bin_ecc) &&
               std::isfinite(m->bin_om) && std::isfinite(m->bin_omdot) && std::isfinite(m->bin_gamma) &&
               std::isfinite(m->bin_eps1) && std::isfinite(m->bin_eps2), "a binary parameter is not finite");
    ARGCHK(m->bin_pb > 0.0, "PB must be positive");
    ARGCHK(m->bin_a1 >= 0.0, "A1 must be >= 0");
    double e = m->bin_ecc;
    if (bt) {
        ARGCHK(e >= 0.0 && e < 1.0, "ECC must be in [0, 1)");
    } else {
        e = std::hypot(m->bin_eps1, m->bin_eps2);
        ARGCHK(e < 1.0, "EPS1^2 + EPS2^2 must be below 1");
    }
    ARGCHK(2.0 * 3.141592653589793 * m->bin_a1 / (m->bin_pb * 86400.0 * (1.0 - e)) < 0.5,
           "2 pi A1 / (PB (1 - e)) must be below 1/2");
    return CRIMP_OK;
}

// the kernels' form of the orbit (angles in radians, PB in seconds)
static void make_binmodel(const crimp_timing_model* m, BinModel* out) {
    const bool bt = m->binary == CRIMP_BINARY_BT;
    const double deg = 3.141592653589793 / 180.0;
    BinModel& b = *out;
    b = BinModel{};
    b.kind = m->binary;
    b.t0 = m->bin_t0;
    b.pb = m->bin_pb * 86400.0;
    b.pbdot = m->bin_pbdot;
    b.a1dot = m->bin_a1dot;
    b.a1 = m->bin_a1;
    b.ecc = bt ? m->bin_ecc : 0.0;
    b.s1me2 = bt ? std::sqrt((1.0 - m->bin_ecc) * (1.0 + m->bin_ecc)) : 1.0;
    b.om = bt ? m->bin_om * deg : 0.0;
    b.omdot = bt ? m->bin_omdot * deg / (365.25 * 86400.0) : 0.0;
    b.gamma = bt ? m->bin_gamma : 0.0;
    b.eps1 = bt ? 0.0 : m->bin_eps1;
    b.eps2 = bt ? 0.0 : m->bin_eps2;
    b.amp = bt ? 1.0 + m->bin_ecc : 1.0 + 0.5 * (std::fabs(m->bin_eps1) + std::fabs(m->bin_eps2));
}

// a call evaluates at the emission time: the caller asked for it (parts bit 3) and the model has an orbit
static bool wants_binary(const crimp_timing_model* m, int32_t parts) {
    return (parts & CRIMP_PART_EMISSION) && m->binary != CRIMP_BINARY_NONE;
}

extern "C" int crimp_calcphase(const double* t_mjd, int64_t n, const crimp_timing_model* model, int32_t parts,
                               double* total, double* folded, uint32_t flags, void* stream) {
    ARGCHK(n >= 0, "n < 0");
    // n == 0 takes null arrays: an empty torch tensor's data pointer is null
    ARGCHK(model != nullptr && ((total != nullptr && t_mjd != nullptr) || n == 0), "null argument");
    ARGCHK(model->n_glitch >= 0 && model->n_glitch <= CRIMP_MAX_GLITCH, "n_glitch out of range");
    ARGCHK(model->n_wave >= 0 && model->n_wave <= CRIMP_MAX_WAVE, "n_wave out of range");
    if (const int rc = check_binary(model)) return rc;
    if (n == 0) return CRIMP_OK;
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    const bool bin = wants_binary(model, parts);
    CPArgs<false> hm{};
    make_cpmodel(model, parts, &hm.m);
    CPArgs<true> hb{};
    if (bin) {
        hb.m = hm.m;
        make_binmodel(model, &hb.b);
    }
    {
        Scratch sc(s);
        const double* dt = nullptr;
        double *dtot = nullptr, *dfol = nullptr;
        HIPCHK(stage_in(sc, t_mjd, (size_t)n, dev, &dt));
        HIPCHK(stage_out(sc, total, (size_t)n, dev, &dtot));
        HIPCHK(stage_out(sc, folded, (size_t)n, dev, &dfol));
        const bool vec = ((reinterpret_cast<uintptr_t>(dt) | reinterpret_cast<uintptr_t>(dtot) |
                           reinterpret_cast<uintptr_t>(dfol)) & 15u) == 0 && (n % 2 == 0);
        const int blocks = (int)std::min<int64_t>(cdiv(vec ? n / 2 : n, 256), int64_t(1) << 20);
        KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
        kt.start();
        // CRIMP_FLAG_FOLD_RADIANS: the folded phase times 2 pi, the host's `folded * (2 * np.pi)` of the Cauchy and
        // von Mises fits (measureToAs.py:195, :200) in the same fp64 multiply
        const double fscale = (flags & CRIMP_FLAG_FOLD_RADIANS) ? 2.0 * 3.141592653589793 : 1.0;
        if (vec && bin)
            k_calcphase_vec<true><<<blocks, 256, 0, s>>>(reinterpret_cast<const double2*>(dt), n / 2, hb,
                                                           reinterpret_cast<double2*>(dtot),
                                                           reinterpret_cast<double2*>(dfol), fscale);
        else if (vec)
            k_calcphase_vec<false><<<blocks, 256, 0, s>>>(reinterpret_cast<const double2*>(dt), n / 2, hm,
                                                            reinterpret_cast<double2*>(dtot),
                                                            reinterpret_cast<double2*>(dfol), fscale);
        else if (bin)
            k_calcphase_scalar<true><<<blocks, 256, 0, s>>>(dt, n, hb, dtot, dfol, fscale);
        else
            k_calcphase_scalar<false><<<blocks, 256, 0, s>>>(dt, n, hm, dtot, dfol, fscale);
        HIPCHK(hipGetLastError());
        kt.stop();
        HIPCHK(copy_back(s, total, dtot, (size_t)n, dev));
        HIPCHK(copy_back(s, folded, dfol, (size_t)n, dev));
    }
    return finish(s, flags);
}

extern "C" int crimp_binary_delay(const double* t_mjd, int64_t n, const crimp_timing_model* model, double* delay_s,
                                  double* t_emit_mjd, uint32_t flags, void* stream) {
    ARGCHK(n >= 0, "n < 0");
    ARGCHK(model != nullptr && ((delay_s != nullptr && t_mjd != nullptr) || n == 0), "null argument");
    ARGCHK(model->binary != CRIMP_BINARY_NONE, "the model has no binary");
    if (const int rc = check_binary(model)) return rc;
    if (n == 0) return CRIMP_OK;
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    BinModel hb{};
    make_binmodel(model, &hb);
    {
        Scratch sc(s);
        const double* dt = nullptr;
        double *dd = nullptr, *de = nullptr;
        HIPCHK(stage_in(sc, t_mjd, (size_t)n, dev, &dt));
        HIPCHK(stage_out(sc, delay_s, (size_t)n, dev, &dd));
        HIPCHK(stage_out(sc, t_emit_mjd, (size_t)n, dev, &de));
        const int blocks = (int)std::min<int64_t>(cdiv(n, 256), int64_t(1) << 20);
        KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
        kt.start();
        k_binary_delay<<<blocks, 256, 0, s>>>(dt, n, hb, dd, de);
        HIPCHK(hipGetLastError());
        kt.stop();
        HIPCHK(copy_back(s, delay_s, dd, (size_t)n, dev));
        HIPCHK(copy_back(s, t_emit_mjd, de, (size_t)n, dev));
    }
    return finish(s, flags);
}

// The instance K<G, TWOD> of an fp64 kernel (k_search_f64, k_search_f64_few) for a harmonic group G of harm_group
#define CRIMP_F64_KERNEL(K, G, TWOD)                                                                \
    ((TWOD) ? ((G) == 8 ? K<8, true> : (G) == 4 ? K<4, true> : (G) == 2 ? K<2, true> : K<1, true>) \
            : ((G) == 8 ? K<8, false> : (G) == 4 ? K<4, false> : (G) == 2 ? K<2, false> : K<1, false>))

// Direct (one lane per trial) fp64 search over trials first + (tidx ? tidx[t] : t), t < count, of any grid, into
// out[t] (or out[tidx[t]] with scatter): plan_direct's photon splits and trial blocks.
static int direct_search(Scratch& sc, hipStream_t s, const double* dt, const double* dt2, int64_t n,
                         const double* freq, int64_t nf, const double* c2, bool twod, int nharm, int stat,
                         int64_t first, const int64_t* tidx, int64_t count, double* out, bool scatter,
                         KernelTimer* kt, const SearchHooks& hooks) {
    const DirectPlan P = plan_direct(n, nharm, count, hooks.budget);
    const int ncomp = 2 * nharm;
    double* part = nullptr;
    HIPCHK(sc.alloc(&part, (size_t)(P.splits * ncomp * P.cb)));
    if (kt) kt->start();
    for (int64_t b0 = 0; b0 < count; b0 += P.cb) {
        const int64_t bc = std::min<int64_t>(P.cb, count - b0);
        const int64_t* bt = tidx ? tidx + b0 : nullptr;
        const int64_t bfirst = tidx ? first : first + b0;
        dim3 grid((unsigned)cdiv(bc, kSearchBlock), (unsigned)P.splits);
        for (int k0 = 1, G; k0 <= nharm; k0 += G) {
            G = harm_group(nharm - k0 + 1);
            CRIMP_F64_KERNEL(k_search_f64, G, twod)<<<grid, kSearchBlock, 0, s>>>(dt, dt2, n, P.chunk, freq, nf, c2, bfirst,
                                                                                   bt, bc, k0, ncomp, part);
            HIPCHK(hipGetLastError());
        }
        if (kt && b0 + P.cb >= count) kt->stop();
        k_search_finalize<<<(unsigned)cdiv(bc, 256), 256, 0, s>>>(part, bc, (int)P.splits, nharm, stat, (double)n,
                                                                 scatter ? bt : nullptr, scatter ? out : out + b0);
        HIPCHK(hipGetLastError());
    }
    return CRIMP_OK;
}

// fp64 fix-up of the trials first + tidx[t] (t < count), a few trials over all photons: plan_fixup's photon splits, one
// block per (trial, split), the splits combined by k_search_finalize into out[tidx[t]].
static int fixup_search(Scratch& sc, hipStream_t s, const double* dt, const double* dt2, int64_t n, const double* freq,
                        int64_t nf, const double* c2, bool twod, int nharm, int stat, int64_t first,
                        const int64_t* tidx, int64_t count, double* out, const SearchHooks& hooks) {
    const FixupPlan P = plan_fixup(n, nharm, hooks.budget);
    const int ncomp = 2 * nharm;
    double* part = nullptr;
    HIPCHK(sc.alloc(&part, (size_t)(P.splits * ncomp * std::min<int64_t>(count, P.cbmax))));
    for (int64_t b0 = 0; b0 < count; b0 += P.cbmax) {
        const int64_t bc = std::min<int64_t>(P.cbmax, count - b0);
        dim3 grid((unsigned)bc, (unsigned)P.splits);
        for (int k0 = 1, G; k0 <= nharm; k0 += G) {
            G = harm_group(nharm - k0 + 1);
            CRIMP_F64_KERNEL(k_search_f64_few, G, twod)<<<grid, kFixBlock, 0, s>>>(dt, dt2, n, P.chunk, freq, nf, c2, first,
                                                                                    tidx + b0, bc, k0, ncomp, part);
            HIPCHK(hipGetLastError());
        }
        k_search_finalize<<<(unsigned)cdiv(bc, 256), 256, 0, s>>>(part, bc, (int)P.splits, nharm, stat, (double)n,
                                                                 tidx + b0, out);
        HIPCHK(hipGetLastError());
    }
    return CRIMP_OK;
}

// Best trial of a power array, np.argmax semantics (periodsearch.py's callers take the maximum and its index): the
// largest value, ties to the lowest index, a NaN above every number (the first NaN wins). k_best_blocks reduces
// grid-stride slices (eight loads in flight per thread) to one candidate per block, k_best_final the candidates.
struct BestCand {
    double v;
    int64_t i;
};
static_assert(sizeof(BestCand) == 16, "NuFinCand (search_nufft_finish.h) mirrors BestCand");
__device__ __forceinline__ bool best_better(double v1, int64_t i1, double v2, int64_t i2) {
    const bool n1 = isnan(v1), n2 = isnan(v2);
    if (n1 != n2) return n1;
    if (!n1 && v1 != v2) return v1 > v2;
    return i1 < i2;
}
__device__ __forceinline__ BestCand best_block_reduce(BestCand c) {
    for (int o = 32; o > 0; o >>= 1) {
        const double v = __shfl_xor(c.v, o);
        const int64_t i = __shfl_xor(c.i, o);
        if (best_better(v, i, c.v, c.i)) c = {v, i};
    }
    __shared__ BestCand red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    c = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
        if (best_better(red[w].v, red[w].i, c.v, c.i)) c = red[w];
    return c;
}
constexpr int kBestBlocks = 1024;
__global__ __launch_bounds__(256) void k_best_blocks(const double* __restrict__ x, int64_t n, BestCand* __restrict__ part) {
    constexpr int U = 8;
    BestCand c = {-INFINITY, INT64_MAX};
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j0 < n; j0 += U * stride) {
        double v[U];
#pragma unroll
        for (int q = 0; q < U; ++q) v[q] = x[j0 + q * stride < n ? j0 + q * stride : n - 1];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t j = j0 + q * stride;
            if (j < n && best_better(v[q], j, c.v, c.i)) c = {v[q], j};
        }
    }
    c = best_block_reduce(c);
    if (threadIdx.x == 0) part[blockIdx.x] = c;
}
__global__ __launch_bounds__(256) void k_best_final(const BestCand* __restrict__ part, int nb, double* __restrict__ out) {
    BestCand c = {-INFINITY, INT64_MAX};
    for (int b = threadIdx.x; b < nb; b += blockDim.x)
        if (best_better(part[b].v, part[b].i, c.v, c.i)) c = part[b];
    c = best_block_reduce(c);
    if (threadIdx.x == 0) {
        out[0] = c.v;
        out[1] = (double)c.i;
    }
}

// the best trial of x[n] (device) into dout[0..1] (device): k_best_blocks + k_best_final on the stream, no sync
static int launch_best(Scratch& sc, hipStream_t s, const double* x, int64_t n, double* dout) {
    BestCand* part = nullptr;
    HIPCHK(sc.alloc(&part, (size_t)kBestBlocks));
    const int nb = (int)std::min<int64_t>(cdiv(n, 256 * 8), kBestBlocks);
    k_best_blocks<<<nb, 256, 0, s>>>(x, n, part);
    HIPCHK(hipGetLastError());
    k_best_final<<<1, 256, 0, s>>>(part, nb, dout);
    HIPCHK(hipGetLastError());
    return CRIMP_OK;
}

// Arithmetic-progression check of the (device) frequency grid: 16 ulp of max|f| (k_ap_check, k_ap_final). Writes
// delta into ap[0] on the device (read by the factorised kernels) and returns whether the grid qualifies. With nu_t
// (a NUFFT search) the NUFFT's own checks -- photon order (k_nu_sorted, MFMA-slot plans only) and the plan's
// scalars (k_ap_final) -- are queued with it and read back in the same transfer: nu_hs = [delta, f0, dt[0],
// dt[n-1], unsorted flag]. No memset: k_ap_check zeroes the order flag, k_ap_final writes the rest.
static int grid_is_progression(Scratch& sc, hipStream_t s, const double* freq, int64_t nf, double** ap, bool* ok,
                               const double* nu_t = nullptr, double t0 = 0.0, int64_t n = 0, double* nu_hs = nullptr,
                               bool nu_sorted_check = true, int* nuflags = nullptr, const NuExpect* ex = nullptr);
#include "search_nufft.h"
static int grid_is_progression(Scratch& sc, hipStream_t s, const double* freq, int64_t nf, double** ap, bool* ok,
                               const double* nu_t, double t0, int64_t n, double* nu_hs, bool nu_sorted_check,
                               int* nuflags, const NuExpect* ex) {
    *ok = false;
    // info: [delta, max deviation, max |f|, NUFFT: delta, f_0, dt[0], dt[n-1], order flag (int bits)], then the
    // block partials of k_ap_check
    double* info = nullptr;
    HIPCHK(sc.alloc(&info, 8 + 2 * kApBlocks));
    *ap = info;
    if (nf < 2) return CRIMP_OK;
    double2* part = reinterpret_cast<double2*>(info + 8);
    int* order = reinterpret_cast<int*>(info + 7);
    const int nb = (int)std::min<int64_t>(cdiv(nf, 256 * 8), kApBlocks);
    k_ap_check<<<nb, 256, 0, s>>>(freq, nf, part, nu_t ? order : nullptr);
    HIPCHK(hipGetLastError());
    if (nu_t && nu_sorted_check)
        k_nu_sorted<<<(unsigned)std::min<int64_t>(cdiv(n, 256), 2048), 256, 0, s>>>(nu_t, t0, n, order);
    NuExpect none{};
    k_ap_final<<<1, 256, 0, s>>>(freq, nf, part, nb, info, nu_t, t0, n, info + 3, order, ex ? *ex : none, nuflags);
    HIPCHK(hipGetLastError());
    if (ex && ex->on) {  // a cached NUFFT plan runs on: no read-back, the device checks the plan (nuflags[1])
        *ok = true;
        return CRIMP_OK;
    }
    double h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(d2h(s, h, info, (nu_t ? 8 : 3) * sizeof(double)));
    *ok = std::isfinite(h[0]) && h[0] != 0.0 && h[1] <= 16.0 * 2.220446049250313e-16 * h[2];
    if (nu_t) std::memcpy(nu_hs, h + 3, 5 * sizeof(double));
    return CRIMP_OK;
}

// Default path: the exact integer-MFMA kernel (search_exact.h) over an arithmetic-progression grid, then the
// fp64 fix-up of the trials whose power is too small for the kernel's error bound (k_search_finalize_exact).
// plan_exact (search_plan.h) decides the photon chunks, the trial blocks and every launch's photon splits.
static int exact_search(Scratch& sc, hipStream_t s, const double* dt, const double* dt2, int64_t n, const double* freq,
                        int64_t nf, const double* c2, const double* ap, bool twod, int nharm, int stat, int64_t first,
                        int64_t count, double* out, KernelTimer* kt, int64_t* nfixed, bool no_fixup,
                        const SearchHooks& hooks) {
    static const int64_t ncu = nu_cus();  // once per process
    const ExactPlan P = plan_exact(n, nf, nharm, first, count, ncu, hooks);
    if (P.err) return set_err(P.err, P.msg);
    const int64_t nchunk = P.nchunk, pc = P.pc;
    const auto kernel = twod ? k_search_exact<true> : k_search_exact<false>;
    const int ncomp = 2 * nharm;
    unsigned long long* tot = nullptr;
    long long* fold = nullptr;
    int64_t* flagged = nullptr;
    int* nflag = nullptr;
    HIPCHK(sc.alloc(&tot, (size_t)P.tot_elems));
    HIPCHK(sc.alloc(&flagged, (size_t)P.flagged_elems));
    HIPCHK(sc.alloc(&nflag, 1));
    if (P.fold_elems > 0) HIPCHK(sc.alloc(&fold, (size_t)P.fold_elems));
    HIPCHK(hipMemsetAsync(nflag, 0, sizeof(int), s));
    const double sigc = std::sqrt((double)n) * 1e-9;  // standard deviation of the error of C_k (search_exact.h)
    if (kt) kt->start();
    for (size_t bi = 0; bi < P.blocks.size(); ++bi) {
        const ExBlock& k = P.blocks[bi];
        const int64_t b0 = k.bfirst - first;
        const int64_t cstride = (int64_t)ncomp * k.bcount;  // one chunk's totals
        HIPCHK(hipMemsetAsync(tot, 0, (size_t)(cstride * nchunk) * sizeof(unsigned long long), s));
        dim3 grid((unsigned)k.bpg, (unsigned)k.splits);
        for (int64_t pch = 0; pch < nchunk; ++pch) {
            const int64_t p0 = pch * pc, np_ = std::min<int64_t>(pc, n - p0);
            unsigned long long* tc = tot + pch * cstride;
            for (int h = 1; h <= nharm; ++h) {
                kernel<<<grid, kExBlock, 0, s>>>(dt + p0, dt2 ? dt2 + p0 : nullptr, np_, k.chunk, freq, nf, c2, ap, k.tf,
                                                 k.nt, P.tpr, k.bfirst, k.bcount, h, tc, fold);
                HIPCHK(hipGetLastError());
            }
        }
        if (kt && bi + 1 == P.blocks.size()) kt->stop();
        k_search_finalize_exact<<<(unsigned)cdiv(k.bcount, 256), 256, 0, s>>>(
            reinterpret_cast<const long long*>(tot), k.bcount, nharm, stat, (double)n, sigc, hooks.fixup_rel, b0,
            out + b0, nflag, flagged, (int)nchunk, cstride);
        HIPCHK(hipGetLastError());
    }
    int nf_h = 0;
    HIPCHK(d2h(s, &nf_h, nflag, sizeof(int)));
    *nfixed = nf_h;
    if (nf_h == 0 || no_fixup) return CRIMP_OK;
    return fixup_search(sc, s, dt, dt2, n, freq, nf, c2, twod, nharm, stat, first, flagged, nf_h, out, hooks);
}

extern "C" int crimp_best(const double* x, int64_t n, double* best, uint32_t flags, void* stream) {
    ARGCHK(n >= 1, "need at least one value");
    ARGCHK(x != nullptr && best != nullptr, "null argument");
    ARGCHK(n <= (int64_t(1) << 53), "n above 2^53 (the index is returned as a double)");
    const Call call(flags, stream, Call::kKeepTimes);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    {
        Scratch sc(s);
        const double* dx = nullptr;
        HIPCHK(stage_in(sc, x, (size_t)n, dev, &dx));
        double* dout = nullptr;
        HIPCHK(sc.alloc(&dout, 2));
        const int rc = launch_best(sc, s, dx, n, dout);
        if (rc) return rc;
        HIPCHK(d2h(s, best, dout, 2 * sizeof(double)));
    }
    return finish(s, flags);
}

extern "C" int crimp_last_search_path(void) { return g_last_search_path; }

extern "C" int crimp_last_nufft_plan(int64_t* fft_length, int32_t* moments, int32_t* gather) {
    if (fft_length) *fft_length = g_last_nufft_n;
    if (moments) *moments = g_last_nufft_p;
    if (gather) *gather = g_last_nufft_gather;
    return CRIMP_OK;
}

extern "C" int crimp_last_nufft_cells(int64_t* built, int64_t* reused) {
    if (built) *built = g_last_cells_built;
    if (reused) *reused = g_last_cells_reused;
    return CRIMP_OK;
}

extern "C" int crimp_last_nufft_work(double* work, int32_t cap) {
    for (int i = 0; i < kNuCls && i < cap; ++i) work[i] = g_nu_work[i];
    return kNuCls;
}

static int search_impl(const double* t, int64_t n, double t0, const double* freq, int64_t nf,
                       const double* log10_negfdot, int64_t nfd, int32_t nharm, int32_t stat, int64_t first,
                       int64_t count, double* out, uint32_t flags, void* stream, double* best);

extern "C" int crimp_search(const double* t, int64_t n, double t0, const double* freq, int64_t nf,
                            const double* log10_negfdot, int64_t nfd, int32_t nharm, int32_t stat, int64_t first,
                            int64_t count, double* out, uint32_t flags, void* stream) {
    return search_impl(t, n, t0, freq, nf, log10_negfdot, nfd, nharm, stat, first, count, out, flags, stream, nullptr);
}

extern "C" int crimp_search_best(const double* t, int64_t n, double t0, const double* freq, int64_t nf,
                                 const double* log10_negfdot, int64_t nfd, int32_t nharm, int32_t stat, int64_t first,
                                 int64_t count, double* out, double* best, uint32_t flags, void* stream) {
    ARGCHK(best != nullptr, "null argument");
    ARGCHK(count >= 1, "the best trial of an empty range");
    ARGCHK(count <= (int64_t(1) << 53), "count above 2^53 (the index is returned as a double)");
    return search_impl(t, n, t0, freq, nf, log10_negfdot, nfd, nharm, stat, first, count, out, flags, stream, best);
}

static int search_impl(const double* t, int64_t n, double t0, const double* freq, int64_t nf,
                       const double* log10_negfdot, int64_t nfd, int32_t nharm, int32_t stat, int64_t first,
                       int64_t count, double* out, uint32_t flags, void* stream, double* best) {
    ARGCHK(n >= 1, "need at least one photon (periodsearch.py:54 reads time[0], time[-1])");
    ARGCHK(nf >= 1, "need at least one trial frequency");
    ARGCHK(nharm >= 1 && nharm <= 256, "nbrHarm must be in 1..256");
    ARGCHK(stat == CRIMP_STAT_Z2 || stat == CRIMP_STAT_H, "unknown statistic");
    ARGCHK(t != nullptr && freq != nullptr && out != nullptr, "null argument");
    const bool twod = log10_negfdot != nullptr && nfd > 0;
    const int64_t total = (twod ? nfd : 1) * nf;
    ARGCHK(first >= 0 && count >= 0 && first + count <= total, "trial range outside the grid");
    const bool f64 = flags & CRIMP_FLAG_F64;
    const bool exact_only = flags & CRIMP_FLAG_EXACT;
    ARGCHK(!(flags & CRIMP_FLAG_RETIRED_FAST), "the fp32 fast search path (flag bits 4, 16, 512) was retired: slower and "
                                                "less precise than the default path");
    ARGCHK(!((flags & CRIMP_FLAG_NUFFT) && f64), "CRIMP_FLAG_NUFFT excludes CRIMP_FLAG_F64");
    ARGCHK(!(exact_only && (f64 || (flags & CRIMP_FLAG_NUFFT))), "CRIMP_FLAG_EXACT excludes CRIMP_FLAG_F64 and _NUFFT");
    // the NUFFT is tried first unless a precision flag excludes it (CRIMP_FLAG_NUFFT asks for the default explicitly)
    const bool nufft = !f64 && !exact_only;
    if (count == 0) return CRIMP_OK;
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    g_last_fixups = 0;
    {
        Scratch sc(s);
        const double *dtm = nullptr, *dfr = nullptr;
        double* dout = nullptr;
        HIPCHK(stage_in(sc, t, (size_t)n, dev, &dtm));
        HIPCHK(stage_in(sc, freq, (size_t)nf, dev, &dfr));
        HIPCHK(stage_out(sc, out, (size_t)count, dev, &dout));
        // fdot term per row, formed on the host exactly as periodsearch.py:95: 0.5*(-1*10**fd)
        double* dc2 = nullptr;
        if (twod) {
            std::vector<double> fdh((size_t)nfd), c2h((size_t)nfd);
            if (dev) {
                HIPCHK(d2h(s, fdh.data(), log10_negfdot, nfd * sizeof(double)));
            } else {
                std::memcpy(fdh.data(), log10_negfdot, nfd * sizeof(double));
            }
            for (int64_t r = 0; r < nfd; ++r) c2h[r] = 0.5 * (-1.0 * std::pow(10.0, fdh[r]));
            HIPCHK(sc.alloc(&dc2, (size_t)nfd));
            HIPCHK(h2d(dc2, c2h.data(), nfd * sizeof(double)));
        }
        // dt = t - t0 (and dt^2) for the exact / fp64 kernels; the NUFFT forms dt in its kernels and skips this
        double *ddt = nullptr, *ddt2 = nullptr;
        auto prep = [&]() -> hipError_t {
            hipError_t e = sc.alloc(&ddt, (size_t)n);
            if (e == hipSuccess && twod) e = sc.alloc(&ddt2, (size_t)n);
            if (e != hipSuccess) return e;
            k_search_prep<<<(int)std::min<int64_t>(cdiv(n, 256), 4096), 256, 0, s>>>(dtm, n, t0, ddt, ddt2);
            return hipGetLastError();
        };
        if (!nufft) HIPCHK(prep());

        // Routing by properties of the whole grid (not of this call's trial range), so that every shard of a
        // sharded search takes the kernel an unsharded search takes:
        //   default (and CRIMP_FLAG_NUFFT): the NUFFT for progressions of >= 64 trials per row (per shard segment),
        //            time-sorted photons and a plan within range (nu_plan); where it declines, the exact rule below;
        //   exact:   exact i8 kernel for progressions of >= 256 trials per row (any length with FORCE_MFMA), fp64
        //            kernel otherwise (a 2-D grid of short rows would fill its 2048-trial tiles with dead columns);
        //   f64:     fp64 kernel.
        KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
        const bool exact_grid = nf >= 256 || (flags & CRIMP_FLAG_FORCE_MFMA);
        bool progression = false;
        double* ap = nullptr;
        double nu_hs[5] = {0, 0, 0, 0, 0};
        int rc = CRIMP_OK;
        bool done = false, best_done = false;
        const bool nu_try = nufft && nf >= 64;
        int* nuflags = nullptr;  // the NUFFT's device flags (fix-up count, photon order / plan check, best trial)
        // (the head of the block a folded search reads back in one transfer, search_nufft_finish.h)
        if (nu_try) HIPCHK(sc.alloc(&nuflags, kNuFinBytes / sizeof(int)));
        NuSearchIn nu;
        nu.t = dtm;
        nu.t0 = t0;
        nu.freq = dfr;
        nu.c2 = dc2;
        nu.twod = twod;
        nu.shape.n = n;
        nu.shape.nf = nf;
        nu.shape.nrows_grid = twod ? nfd : 1;
        nu.shape.nharm = nharm;
        nu.shape.stat = stat;
        nu.shape.first = first;
        nu.shape.count = count;
        nu.shape.want_best = best != nullptr;
        nu.hooks = NuHooks::from_env();
        nu.search_hooks = SearchHooks::from_env();
        nu.hs = nu_hs;
        nu.out = dout;
        nu.best = best;
        nu.timed = flags & CRIMP_FLAG_TIME_KERNELS;
        nu.no_fixup = (flags & CRIMP_FLAG_NO_FIXUP) != 0;
        nu.nflag = nuflags;
        const bool gather_form = nu_gather_form(nu.shape.nrows_grid, nu.hooks);
        // A repeated search over the same buffers reuses its last plan (NuPlanCache::find): the progression check and
        // the plan's scalars are recomputed on the device and compared there (k_ap_final), every NUFFT kernel that
        // reads photon-derived tables exits if they differ, and the host, reading the result flags anyway at the
        // end, redoes the search from a fresh plan -- one host round trip per search instead of two.
        // A cell-gather plan's start tables are kept with it: the repeated search skips the cell-start pass too, and
        // its gathers check the tables against the photons they read (k_nu_gather, CHECK; the same flag and redo).
        const NuSpecKey key = NuPlanCache::key(dtm, dfr, nu.shape, twod ? nfd : 0, t0, gather_form);
        NuPlanCache::Hold cells(g_nu_cache);
        nu.keep = &cells.t;
        bool spec_mismatch = false;
        // One attempt: the progression check, the search, then what the plan cache keeps of it. From the cache entry
        // (from_cache; nothing runs without one) the check compares on the device and reads nothing back; without it
        // the check reads the plan's scalars back, for the exact rule too.
        auto nu_attempt = [&](bool from_cache) -> int {
            NuExpect ex{};
            NuCellTab cached;
            if (from_cache) {
                if (!g_nu_cache.find(key, nu.hooks, nu_hs, &cached)) return CRIMP_OK;
                for (int q = 0; q < 4; ++q) ex.v[q] = nu_hs[q];
                ex.on = 1;
                ex.check_order = gather_form ? 0 : 1;
            }
            progression = false;
            // A cached cell-gather plan with its start tables launches no check here: it rides in the search's first
            // gather launch and the host finishes it from the search's read-back (nufft_search, NuRun::fold), or
            // nufft_search queues these launches itself where the plan turns out to have no checking gather first.
            nu.fold_try = from_cache && gather_form && cached.p && !nu.hooks.fold_off;
            nu.ap = &ap;
            int r = CRIMP_OK;
            if (nu.fold_try)
                progression = true;
            else
                r = grid_is_progression(sc, s, dfr, nf, &ap, &progression, nufft ? dtm : nullptr, t0, n, nu_hs,
                                        !gather_form, nuflags, from_cache ? &ex : nullptr);
            if (r) return r;
            if (!progression || !nu_try) return CRIMP_OK;  // the exact rule
            nu.cached = from_cache ? &cached : nullptr;
            NuSearchOut res;
            r = nufft_search(sc, s, nu, &res);
            if (r) return r;
            done = res.applicable;  // else: unsorted photons, no plan, or a cached plan that no longer holds
            best_done = res.best_done;
            if (done) g_last_fixups = res.nfixed;
            if (!from_cache) {  // ended clean (the order flag read back as 0): the plan and its tables are kept
                if (done) g_nu_cache.store(key, nu.hooks, nu_hs, &cells.t);
                return CRIMP_OK;
            }
            if (done && cells.t.p) g_nu_cache.attach(key, nu.hooks, &cells.t);  // (an entry stored without tables)
            g_nu_cache.release(&cells.t);
            spec_mismatch = res.mismatch;
            if (spec_mismatch) g_nu_cache.drop(key);
            // not done and no mismatch: photons out of order under a still-valid progression (the exact rule)
            return CRIMP_OK;
        };
        if (nu_try) rc = nu_attempt(true);
        if (rc) return rc;
        if (!done && (!progression || spec_mismatch) && !f64 && (exact_grid || nu_try)) rc = nu_attempt(false);
        if (rc) return rc;
        const bool factorised = !done && progression && exact_grid;
        if ((flags & CRIMP_FLAG_FORCE_MFMA) && !done && !factorised)
            return set_err(CRIMP_ERR_ARG, "factorised search not applicable (grid is not an arithmetic progression)");
        if (nufft && !done) HIPCHK(prep());  // the NUFFT did not apply: the exact / fp64 kernels read dt
        if (done) {
        } else if (factorised) {
            g_last_search_path = 1;
            int64_t nfix = 0;
            rc = exact_search(sc, s, ddt, ddt2, n, dfr, nf, dc2, ap, twod, nharm, stat, first, count, dout, &kt, &nfix,
                              (flags & CRIMP_FLAG_NO_FIXUP) != 0, nu.search_hooks);
            g_last_fixups = nfix;
        } else {
            g_last_search_path = 0;
            rc = direct_search(sc, s, ddt, ddt2, n, dfr, nf, dc2, twod, nharm, stat, first, nullptr, count, dout,
                               false, &kt, nu.search_hooks);
        }
        if (rc) return rc;
        if (best && !best_done) {  // the exact / fp64 paths, or a NUFFT whose fix-up rewrote powers after its read-back
            double* db = nullptr;
            HIPCHK(sc.alloc(&db, 2));
            rc = launch_best(sc, s, dout, count, db);
            if (rc) return rc;
            HIPCHK(d2h(s, best, db, 2 * sizeof(double)));
        }
        HIPCHK(copy_back(s, out, dout, (size_t)count, dev));
    }
    return finish(s, flags);
}

extern "C" int crimp_search_sets(const double* t, const int64_t* offsets, int64_t nset, const double* freq,
                                 int32_t nharm, int32_t stat, double* out, uint32_t flags, void* stream) {
    ARGCHK(nset >= 0, "nset < 0");
    ARGCHK(nharm >= 1 && nharm <= 256, "nbrHarm must be in 1..256");
    ARGCHK(stat == CRIMP_STAT_Z2 || stat == CRIMP_STAT_H, "unknown statistic");
    ARGCHK(t != nullptr && offsets != nullptr && freq != nullptr && out != nullptr, "null argument");
    ARGCHK(nset <= 2147483647LL, "too many sets");
    if (nset == 0) return CRIMP_OK;
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    std::vector<int64_t> hoff;
    const int rc = read_offsets(call, offsets, nset, true, "every set needs photons (periodsearch.py:54 reads time[0])",
                                &hoff);
    if (rc) return rc;
    {
        Scratch sc(s);
        const double *dt = nullptr, *df = nullptr;
        const int64_t* doff = nullptr;
        double* dout = nullptr;
        HIPCHK(stage_in(sc, t, (size_t)hoff[nset], dev, &dt));
        HIPCHK(stage_in(sc, offsets, (size_t)nset + 1, dev, &doff));
        HIPCHK(stage_in(sc, freq, (size_t)nset, dev, &df));
        HIPCHK(stage_out(sc, out, (size_t)nset, dev, &dout));
        k_search_sets<<<(unsigned)nset, kSetBlock, 0, s>>>(dt, doff, df, nharm, stat,
                                                           (flags & CRIMP_FLAG_TIME_DAYS) ? 86400.0 : 1.0, dout);
        HIPCHK(hipGetLastError());
        HIPCHK(copy_back(s, out, dout, (size_t)nset, dev));
        // CRIMP_FLAG_ASYNC: with device pointers the call stages nothing and takes no scratch block (a block handed
        // back while the kernel still ran could be given to another call on another stream), so it may return with
        // the kernel queued
        if (dev && (flags & CRIMP_FLAG_ASYNC) && sc.held.empty()) return CRIMP_OK;
    }
    return finish(s, flags);
}

static int make_tpl(const crimp_template* tpl, TplDev* T) {
    ARGCHK(tpl != nullptr, "null template");
    ARGCHK(tpl->ncomp >= 1 && tpl->ncomp <= CRIMP_MAX_COMP, "ncomp out of range");
    ARGCHK(tpl->model >= 0 && tpl->model <= 2, "unknown template model");
    std::memset(T, 0, sizeof(*T));
    T->model = tpl->model;
    T->K = tpl->ncomp;
    const double twopi = 6.283185307179586476925286766559;
    for (int j = 0; j < tpl->ncomp; ++j) {
        const double a = tpl->amp[j] * tpl->amp_shift;
        T->loc[j] = tpl->loc[j];
        if (tpl->model == CRIMP_MODEL_FOURIER) {
            T->amp[j] = a;
        } else if (tpl->model == CRIMP_MODEL_CAUCHY) {
            T->amp[j] = (a / twopi) * std::sinh(tpl->wid[j]);
            T->ch[j] = std::cosh(tpl->wid[j]);
        } else {
            T->amp[j] = a / (twopi * tpl->i0[j]);
            T->kap[j] = 1.0 / (tpl->wid[j] * tpl->wid[j]);
        }
    }
    return CRIMP_OK;
}

extern "C" int crimp_toa_points(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                                const int64_t* pt_interval, const double* pt_norm, const double* pt_phi, int64_t npts,
                                double* out, uint32_t flags, void* stream) {
    ARGCHK(nint >= 1 && npts >= 0, "bad sizes");
    ARGCHK(x != nullptr && offsets != nullptr && pt_interval != nullptr && pt_norm != nullptr && pt_phi != nullptr &&
               out != nullptr,
           "null argument");
    TplDev T;
    int rc = make_tpl(tpl, &T);
    if (rc) return rc;
    if (npts == 0) return CRIMP_OK;
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    // groups of <= 4 consecutive points sharing an interval (host needs the interval ids)
    std::vector<int64_t> pint((size_t)npts), hoff;
    if (dev)
        HIPCHK(d2h(s, pint.data(), pt_interval, npts * sizeof(int64_t)));
    else
        std::memcpy(pint.data(), pt_interval, npts * sizeof(int64_t));
    rc = read_offsets(call, offsets, nint, false, "offsets must be non-decreasing", &hoff);
    if (rc) return rc;
    std::vector<int64_t> gint, gfirst;
    std::vector<int32_t> gnp;
    for (int64_t p = 0; p < npts;) {
        ARGCHK(pint[p] >= 0 && pint[p] < nint, "point interval out of range");
        int64_t q = p + 1;
        while (q < npts && q - p < kPtsPerGroup && pint[q] == pint[p]) ++q;
        gint.push_back(pint[p]);
        gfirst.push_back(p);
        gnp.push_back((int32_t)(q - p));
        p = q;
    }
    const int64_t ng = (int64_t)gint.size();
    {
        Scratch sc(s);
        const double *dx = nullptr, *dn = nullptr, *dp = nullptr;
        const int64_t* doff = nullptr;
        double* dout = nullptr;
        HIPCHK(stage_in(sc, x, (size_t)hoff[nint], dev, &dx));
        HIPCHK(stage_in(sc, offsets, (size_t)nint + 1, dev, &doff));
        HIPCHK(stage_in(sc, pt_norm, (size_t)npts, dev, &dn));
        HIPCHK(stage_in(sc, pt_phi, (size_t)npts, dev, &dp));
        HIPCHK(stage_out(sc, out, (size_t)npts * 8, dev, &dout));
        TplDev* dT = nullptr;
        int64_t *dgi = nullptr, *dgf = nullptr;
        int32_t* dgn = nullptr;
        HIPCHK(sc.alloc(&dT, 1));
        HIPCHK(sc.alloc(&dgi, (size_t)ng));
        HIPCHK(sc.alloc(&dgf, (size_t)ng));
        HIPCHK(sc.alloc(&dgn, (size_t)ng));
        HIPCHK(h2d(dT, &T, sizeof(T)));
        HIPCHK(h2d(dgi, gint.data(), ng * sizeof(int64_t)));
        HIPCHK(h2d(dgf, gfirst.data(), ng * sizeof(int64_t)));
        HIPCHK(h2d(dgn, gnp.data(), ng * sizeof(int32_t)));
        k_toa_points<<<(unsigned)ng, kPtsBlock, 0, s>>>(dx, doff, dT, dgi, dgf, dgn, dn, dp, dout);
        HIPCHK(hipGetLastError());
        HIPCHK(copy_back(s, out, dout, (size_t)npts * 8, dev));
        HIPCHK(hipStreamSynchronize(s));  // host vectors above are read by queued copies
    }
    return finish(s, flags);
}

// Per-split brute-grid partial sums (k_toa_grid) for nint <= 65535 intervals of at most maxn photons:
// pl[((split*nint + i)*nnorm + a)*nphi + b] (log2 sums), ph[(split*nint + i)*nphi + b] (min h).
// mode: crimp_toa_fit's fast brute-grid modes (the kGrid* bits, toa_grid_plan.h; Fourier templates on
// k_toa_grid_mf only); kGridNoMin and kGridCert leave *ph = nullptr.
// a_first: the lazy norms [0, a_first) of every interval are not evaluated (their lnsum entries are left unwritten;
// k_toa_grid_best knows them invalid from the min, or has the grid rerun in full)
static int toa_grid_partials(Scratch& sc, hipStream_t s, const double* dx, const int64_t* doff, const TplDev* dT,
                             const TplDev& T, const double* dnrm, int64_t nnorm, const double* dphi, int64_t nphi,
                             int64_t nint, int64_t maxn, double** pl, double** ph, int64_t* splits_out,
                             int mode = 0, int* mode_out = nullptr, int64_t a_first = 0) {
    const int model = T.model, K = T.K;
    bool mf_ok = false;
    const int se = grid_mf_scale(T, &mf_ok);
    const int64_t pblocks = cdiv(nphi, kGridBlock);
    // photon splits: aim at kGridTarget blocks (2 waves each; 4 waves/SIMD fit, 2048 resident blocks), so
    // that the last round of waves is a small part of the launch (config 5: 1250 intervals x 14 splits = 8.5
    // rounds; targets of 12288..32768 blocks measured within 1 %, profiles/r02/ab_toa_target.log), splits of
    // >= 1024 photons
    int64_t splits = std::max<int64_t>(1, std::min<int64_t>(cdiv(kGridTarget, pblocks * nint),
                                                            cdiv(std::max<int64_t>(maxn, 1), 1024)));
    splits = std::min<int64_t>(splits, 65535);
    int64_t chunk = cdiv(std::max<int64_t>(maxn, 1), splits);
    chunk = cdiv(chunk, kGridBlock) * kGridBlock;
    splits = cdiv(std::max<int64_t>(maxn, 1), chunk);
    HIPCHK(sc.alloc(pl, (size_t)(splits * nint * nnorm * nphi)));
    const bool mf = model == CRIMP_MODEL_FOURIER && CRIMP_GRID_MFMA && K <= kGridKMax && mf_ok;
    if (!mf) mode = 0;
    if (!(mode & kGridProd8)) a_first = 0;  // lazy norms only on the eight-factor kernel (its caller checks them)
    if (!(mode & kGridProd8)) mode &= ~kGridCert;
    if (mode_out) *mode_out = mode;
    const bool hm = !(mode & (kGridNoMin | kGridCert)), p8 = mode & kGridProd8;
    if (!hm)
        *ph = nullptr;
    else
        HIPCHK(sc.alloc(ph, (size_t)(splits * nint * nphi)));
    dim3 grid((unsigned)pblocks, (unsigned)nint, (unsigned)splits);
    // norms per lane: 2 or kGridNNSmall for a pruned grid (crimp_toa_fit; 1 left after its lazy norms, on the eight-
    // factor kernel), otherwise kGridNN per launch
    const int64_t neval = nnorm - a_first;
    const int nn = (neval == 1 && mf && (mode & kGridProd8)) ? 1 : neval <= 2 ? 2 : neval <= kGridNNSmall ? kGridNNSmall
                                                                                                       : kGridNN;
    for (int64_t a0 = a_first; a0 < nnorm; a0 += nn) {
        const int na = (int)std::min<int64_t>(nn, nnorm - a0);
#define CRIMP_LG1(MD, KK, NNV, PP) k_toa_grid<kGridKMax, MD, KK, NNV, PP><<<grid, kGridBlock / PP, 0, s>>>(dx, doff, dT, dnrm, \
                                                          (int)nnorm, (int)a0, na, dphi, (int)nphi, chunk, (int)nint, *pl, *ph)
#define CRIMP_LG(MD, KK) do { if (nn == 2) CRIMP_LG1(MD, KK, 2, kGridPPL); \
                              else if (nn == kGridNNSmall) CRIMP_LG1(MD, KK, kGridNNSmall, kGridPPL); \
                              else CRIMP_LG1(MD, KK, kGridNN, 1); } while (0)
        if (mf) {
#define CRIMP_LM2(KK, NNV, HM, PR) k_toa_grid_mf<KK, NNV, HM, PR><<<grid, 256, 0, s>>>(dx, doff, dT, dnrm, (int)nnorm, \
                                                        (int)a0, na, dphi, (int)nphi, chunk, (int)nint, se, (int)a_first, \
                                                        *pl, *ph)
#define CRIMP_LM1(KK, NNV) do { \
        if (!hm && p8) CRIMP_LM2(KK, NNV, false, 8); \
        else if (p8) CRIMP_LM2(KK, NNV, true, 8); \
        else if (!hm) CRIMP_LM2(KK, NNV, false, 4); \
        else CRIMP_LM2(KK, NNV, true, 4); } while (0)
#define CRIMP_LM(KK) do { if (nn == 1) { if (hm) CRIMP_LM2(KK, 1, true, 8); else CRIMP_LM2(KK, 1, false, 8); } \
                          else if (nn == 2) CRIMP_LM1(KK, 2); else if (nn == kGridNNSmall) CRIMP_LM1(KK, kGridNNSmall); \
                          else CRIMP_LM1(KK, kGridNN); } while (0)
            switch (K) {
                case 1: CRIMP_LM(1); break;
                case 2: CRIMP_LM(2); break;
                case 3: CRIMP_LM(3); break;
                case 4: CRIMP_LM(4); break;
                case 5: CRIMP_LM(5); break;
                case 6: CRIMP_LM(6); break;
                case 7: CRIMP_LM(7); break;
                default: CRIMP_LM(8); break;
            }
#undef CRIMP_LM
#undef CRIMP_LM1
#undef CRIMP_LM2
        } else if (model == CRIMP_MODEL_FOURIER) {
            switch (K) {
                case 1: CRIMP_LG(CRIMP_MODEL_FOURIER, 1); break;
                case 2: CRIMP_LG(CRIMP_MODEL_FOURIER, 2); break;
                case 3: CRIMP_LG(CRIMP_MODEL_FOURIER, 3); break;
                case 4: CRIMP_LG(CRIMP_MODEL_FOURIER, 4); break;
                case 5: CRIMP_LG(CRIMP_MODEL_FOURIER, 5); break;
                case 6: CRIMP_LG(CRIMP_MODEL_FOURIER, 6); break;
                case 7: CRIMP_LG(CRIMP_MODEL_FOURIER, 7); break;
                default: CRIMP_LG(CRIMP_MODEL_FOURIER, 8); break;
            }
        } else if (model == CRIMP_MODEL_CAUCHY) {
            CRIMP_LG(CRIMP_MODEL_CAUCHY, 0);
        } else {
            CRIMP_LG(CRIMP_MODEL_VONMISES, 0);
        }
#undef CRIMP_LG
#undef CRIMP_LG1
        HIPCHK(hipGetLastError());
    }
    *splits_out = splits;
    return CRIMP_OK;
}

// crimp_toa_fit_redchi2's binned part: np.histogram edges and bin centres (binphases), free parameters, output
struct RedChi2Req {
    const double *edges, *centers;
    int32_t nbins, nfree;
    double* out;
};

struct EventGuard {  // an event destroyed on every return path (destruction waits for nothing unless wait is set)
    hipEvent_t e = nullptr;
    bool wait = false;  // synchronise before destroying: the event marks work that uses scratch blocks of this call
    ~EventGuard() {
        if (e && wait) (void)hipEventSynchronize(e);
        if (e) (void)hipEventDestroy(e);
    }
};

// CRIMP_TOA_HOST_TRACE=1 (diagnostic): host-side phase times of each crimp_toa_fit(_redchi2) call on stderr
struct HostTrace {
    bool on;
    std::chrono::steady_clock::time_point t0, last;
    std::string line;
    HostTrace() : on(getenv("CRIMP_TOA_HOST_TRACE") != nullptr) {
        if (on) t0 = last = std::chrono::steady_clock::now();
    }
    void mark(const char* what) {
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        char b[96];
        snprintf(b, sizeof(b), " %s %.1f", what, std::chrono::duration<double, std::micro>(t - last).count());
        line += b;
        last = t;
    }
    ~HostTrace() {
        if (on) fprintf(stderr, "toa host trace (us):%s total %.1f\n", line.c_str(),
                        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
};

// measureToAs.py:715-725 / :757-771 (readvaryparam=False) and :320-376
static FitCfg toa_fit_cfg(const crimp_template* tpl, const TplDev& T, double norm0, int32_t ph_shift_res,
                          const ToaHooks& hooks) {
    FitCfg C;
    C.lo = norm0 / 100.0;
    C.hi = 500.0;
    C.pb = T.model == CRIMP_MODEL_FOURIER ? M_PI : 1.5 * M_PI;
    C.step = (2.0 * M_PI) / (double)ph_shift_res;
    C.kcap = (double)ph_shift_res / 2.0;
    C.sum_amp = 0.0;
    for (int j = 0; j < tpl->ncomp; ++j) C.sum_amp += tpl->amp[j] * tpl->amp_shift;
    C.amp_lo = T.model == CRIMP_MODEL_FOURIER ? 0.01 : 0.0;                                  // :308, :461, :605
    C.amp_hi = T.model == CRIMP_MODEL_FOURIER ? 100.0 : T.model == CRIMP_MODEL_CAUCHY ? INFINITY : 500.0;
    C.mom_r = hooks.has_mom_r ? hooks.mom_r : kMomR;
    return C;
}

// The launches of one crimp_toa_fit call over its staged inputs and uploaded plan, on the caller's stream
struct ToaFitRun {
    Scratch& sc;
    hipStream_t s;
    bool timed;
    const TplDev& T;
    const FitCfg& C;
    const std::vector<int64_t>& hoff;
    int64_t nint;
    const GridPlan* plan;    // nullptr: no brute grid
    const EventGuard& ebin;  // the auxiliary stream's histogram has finished (kGridCert reads its counts)
    int lattice_start = 0;
    bool vary_amps = false;
    int nbins = 0;
    const double *dx = nullptr, *de = nullptr;
    const int64_t* doff = nullptr;
    TplDev* dT = nullptr;
    double *dout = nullptr, *dstart = nullptr, *dphi = nullptr, *dnrm = nullptr;
    double* hcache = nullptr;  // per-photon template part for the iterative norm profiles of the 1-sigma scan (only
                               // the CRIMP_FIT_MOMENTS=0 build caches it; the moment profile needs none)
    int* dunsafe = nullptr;    // k_toa_grid_best: a valid lattice point whose min factor is below 2^-15 / s, or of a
                               // lazy norm
    uint64_t* dlzmask = nullptr;
    int* dlzrow = nullptr;
    unsigned long long* dcnt = nullptr;

    // the plan's tables through the page-locked staging buffer, and the cleared unsafe flag
    int upload_plan() {
        const GridPlan& P = *plan;
        HIPCHK(sc.alloc(&dphi, P.phi.size()));
        HIPCHK(sc.alloc(&dnrm, P.nrm.size()));
        HIPCHK(h2d_async(s, dphi, P.phi.data(), P.phi.size() * sizeof(double)));
        HIPCHK(h2d_async(s, dnrm, P.nrm.data(), P.nrm.size() * sizeof(double)));
        if (P.mode & kGridCert) {
            HIPCHK(sc.alloc(&dlzmask, P.mask.size()));
            HIPCHK(sc.alloc(&dlzrow, P.row.size()));
            HIPCHK(h2d_async(s, dlzmask, P.mask.data(), P.mask.size() * sizeof(uint64_t)));
            HIPCHK(h2d_async(s, dlzrow, P.row.data(), P.row.size() * sizeof(int)));
        }
        HIPCHK(sc.alloc(&dunsafe, 1));
        HIPCHK(hipMemsetAsync(dunsafe, 0, sizeof(int), s));
        return CRIMP_OK;
    }

    // brute grid of every interval (k_toa_grid_mf / k_toa_grid + k_toa_grid_best)
    int brute(int md) {
        const GridPlan& P = *plan;
        const int64_t nc = P.nc, nphi = (int64_t)P.phi.size();
        for (int64_t i0 = 0; i0 < nint; i0 += 65535) {
            const int64_t nb = std::min<int64_t>(65535, nint - i0);
            int64_t maxn = 0;
            for (int64_t i = i0; i < i0 + nb; ++i) maxn = std::max(maxn, hoff[i + 1] - hoff[i]);
            double *pl = nullptr, *ph = nullptr;
            int64_t splits = 0;
            int ran = 0;
            const int64_t lz = (md & kGridProd8) ? P.nlazy : 0;
            const int r2 = toa_grid_partials(sc, s, dx, doff + i0, dT, T, dnrm + i0 * nc, nc, dphi, nphi, nb, maxn, &pl,
                                             &ph, &splits, md, &ran, lz);
            if (r2) return r2;
            g_last_grid_fast = ran;
            g_last_grid_norms = nc - ((ran & kGridProd8) ? lz : 0);  // the lazy norms are not evaluated
            const bool cert = ran & kGridCert;
            if (cert && ebin.e) HIPCHK(hipStreamWaitEvent(s, ebin.e, 0));  // the histogram's counts
            k_toa_grid_best<<<(unsigned)nb, 256, 0, s>>>(pl, ph, dnrm + i0 * nc, dphi, doff + i0, de + i0, (int)nc,
                                                        (int)nphi, (int)nb, (int)splits, T.model, C.sum_amp,
                                                        P.grid_n[0], C.lo, C.hi, lattice_start, P.hb,
                                                        (ran & kGridProd8) ? P.gsc : 0.0,
                                                        (ran & kGridProd8) ? (int)lz : 0, dunsafe,
                                                        cert ? dlzmask : nullptr, cert ? dlzrow + i0 * lz : nullptr,
                                                        cert ? dcnt + i0 * nbins : nullptr, cert ? nbins : 0,
                                                        dstart + 2 * i0);
            HIPCHK(hipGetLastError());
        }
        return CRIMP_OK;
    }

    // the fit kernel over every interval
    void fit() {
        if (vary_amps) {
            k_toa_fit_amp<<<(unsigned)nint, kFitBlock, 0, s>>>(dx, doff, dT, de, dstart, C, dout);
            return;
        }
#define CRIMP_LF(MD, KK) k_toa_fit<MD, KK><<<(unsigned)nint, kFitBlock, 0, s>>>(dx, doff, dT, de, dstart, C, dout, hcache)
        if (T.model == CRIMP_MODEL_FOURIER) {
            switch (T.K) {  // the template size at compile time (0: read at run time)
                case 1: CRIMP_LF(CRIMP_MODEL_FOURIER, 1); break;
                case 2: CRIMP_LF(CRIMP_MODEL_FOURIER, 2); break;
                case 3: CRIMP_LF(CRIMP_MODEL_FOURIER, 3); break;
                case 4: CRIMP_LF(CRIMP_MODEL_FOURIER, 4); break;
                case 5: CRIMP_LF(CRIMP_MODEL_FOURIER, 5); break;
                case 6: CRIMP_LF(CRIMP_MODEL_FOURIER, 6); break;
                case 7: CRIMP_LF(CRIMP_MODEL_FOURIER, 7); break;
                case 8: CRIMP_LF(CRIMP_MODEL_FOURIER, 8); break;
                default: CRIMP_LF(CRIMP_MODEL_FOURIER, 0); break;
            }
        } else if (T.model == CRIMP_MODEL_CAUCHY) {
            CRIMP_LF(CRIMP_MODEL_CAUCHY, 0);
        } else {
            CRIMP_LF(CRIMP_MODEL_VONMISES, 0);
        }
#undef CRIMP_LF
    }

    // Brute grid, then fits, in sequence on the caller's stream. Measured, rejected and removed: the intervals in two
    // halves on two streams, the second half's grid beside the first half's fits (config 5: 6.1 vs 5.7 ms per 1250
    // intervals, profiles/r04/toa_breakdown.log) -- each half's fit runs 1.2 rounds of the resident workgroups and its
    // grid half as many blocks, so the tails grow, not shrink
    int all(int md) {
        KernelTimer kg(s, timed);  // brute grid: k_toa_grid(_mf) + k_toa_grid_best
        kg.start();
        if (plan) {
            const int r2 = brute(md);
            if (r2) return r2;
            kg.stop();
        }
        KernelTimer kf(s, timed);  // the fit kernel
        kf.start();
        fit();
        HIPCHK(hipGetLastError());
        kf.stop();
        return CRIMP_OK;
    }
};

// redChi2's histogram on the auxiliary stream, beside the grid and the fits; *ebin marks its end
static int toa_hist_aux(hipStream_t s, const double* dx, const int64_t* doff, const double* dedg, int nbins, int64_t nint,
                        int64_t ntot, unsigned long long* dcnt, EventGuard* ebin) {
    hipStream_t s1 = aux_stream();
    if (!s1) return set_err(CRIMP_ERR_HIP, "cannot create the auxiliary stream");
    EventGuard e0;
    HIPCHK(hipEventCreateWithFlags(&e0.e, hipEventDisableTiming));
    HIPCHK(hipEventRecord(e0.e, s));
    HIPCHK(hipStreamWaitEvent(s1, e0.e, 0));
    k_binphases<<<dim3((unsigned)nint, (unsigned)bin_splits(ntot, nint)), 64 * kBinWaves, 0, s1>>>(dx, doff, dedg, nbins,
                                                                                                  dcnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventCreateWithFlags(&ebin->e, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ebin->e, s1));
    return CRIMP_OK;
}

// crimp_toa_fit(_redchi2): the inputs staged, the brute grid planned on the host (plan_brute_grid) and its tables
// uploaded, the grid and the fits launched (ToaFitRun), rerun with the full kernel where a runtime certificate failed,
// then redChi2 from the final records
static int toa_fit_impl(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                        const double* exposure, double norm0, int32_t ph_shift_res, int32_t options, double* out,
                        uint32_t flags, void* stream, const RedChi2Req* rq) {
    ARGCHK(nint >= 1, "bad sizes");
    ARGCHK(ph_shift_res >= 1, "phShiftRes must be >= 1");
    ARGCHK(norm0 > 0.0, "template norm must be positive");
    ARGCHK(x != nullptr && offsets != nullptr && exposure != nullptr && out != nullptr, "null argument");
    ARGCHK(nint <= 2147483647LL, "too many intervals");
    TplDev T;
    int rc = make_tpl(tpl, &T);
    if (rc) return rc;
    const bool brutemin = options & CRIMP_TOA_BRUTE;
    if (brutemin) ARGCHK(T.K <= kGridKMax, "brute grid supports at most 8 template components");
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    const ToaHooks hooks = ToaHooks::from_env();
    HostTrace ht;
    g_last_grid_norms = 0;
    g_last_grid_fast = 0;
    // the host's copies of the offsets, exposures and (crimp_toa_fit_redchi2) histogram edges: one stream drain for all
    std::vector<int64_t> hoff((size_t)nint + 1);
    std::vector<double> hexp((size_t)nint), hedg(rq ? (size_t)rq->nbins + 1 : 0);
    pin_begin((size_t)65536 + (size_t)nint * 340 + hedg.size() * 8);
    HIPCHK(read_list(call, {{hoff.data(), offsets, hoff.size() * sizeof(int64_t)},
                            {hexp.data(), exposure, hexp.size() * sizeof(double)},
                            {hedg.data(), rq ? rq->edges : nullptr, hedg.size() * sizeof(double)}}));
    rc = check_offsets(hoff, true, "every ToA interval needs photons (measureToAs.py:182 fails on an empty one)");
    if (rc) return rc;
    g_pin.used = 0;  // the reads are in the host's vectors: the staging buffer starts over for the uploads
    ht.mark("offsets");
    const FitCfg C = toa_fit_cfg(tpl, T, norm0, ph_shift_res, hooks);
    {
        Scratch sc(s);
        // destroyed before sc releases its blocks: on an error return between the histogram's launch on the
        // auxiliary stream and the caller stream's wait for it, dcnt stays held until the histogram has finished
        EventGuard ebin;
        ebin.wait = true;
        GridPlan plan;
        ToaFitRun R{sc, s, call.timed, T, C, hoff, nint, brutemin ? &plan : nullptr, ebin};
        R.lattice_start = hooks.lattice_start;
        R.vary_amps = options & CRIMP_TOA_VARY_AMPS;
        HIPCHK(stage_in(sc, x, (size_t)hoff[nint], dev, &R.dx));
        HIPCHK(stage_in(sc, offsets, (size_t)nint + 1, dev, &R.doff));
        HIPCHK(stage_in(sc, exposure, (size_t)nint, dev, &R.de));
        HIPCHK(stage_out(sc, out, (size_t)nint * 8, dev, &R.dout));
        // redChi2's histogram (crimp_toa_fit_redchi2) needs only the photons: it runs on the auxiliary stream beside
        // the brute grid and the fits, in the partly empty last round of the fit's workgroups (timed calls: on this
        // stream before the grid's timer starts, so that the kernel times stay those of the grid and the fit alone).
        // The brute grid's lazy-norm certificate reads it too (kGridCert).
        const double *dedg = nullptr, *dcen = nullptr;
        double* dred = nullptr;
        if (rq) {
            R.nbins = rq->nbins;
            HIPCHK(stage_in(sc, rq->edges, (size_t)rq->nbins + 1, dev, &dedg));
            HIPCHK(stage_in(sc, rq->centers, (size_t)rq->nbins, dev, &dcen));
            HIPCHK(stage_out(sc, rq->out, (size_t)nint, dev, &dred));
            HIPCHK(sc.alloc(&R.dcnt, (size_t)(nint * rq->nbins)));
            HIPCHK(hipMemsetAsync(R.dcnt, 0, (size_t)(nint * rq->nbins) * sizeof(unsigned long long), s));
            if (call.timed) {
                k_binphases<<<dim3((unsigned)nint, (unsigned)bin_splits(hoff[nint], nint)), 64 * kBinWaves, 0, s>>>(
                    R.dx, R.doff, dedg, rq->nbins, R.dcnt);
                HIPCHK(hipGetLastError());
            }
        }
        ht.mark("stage+hist");
        HIPCHK(sc.alloc(&R.dT, 1));
        HIPCHK(h2d_async(s, R.dT, &T, sizeof(T)));
        HIPCHK(sc.alloc(&R.dstart, (size_t)(2 * nint)));
        std::vector<double> hstart;
        if (brutemin) {
            plan = plan_brute_grid(T, C.lo, C.hi, C.pb, hoff.data(), hexp.data(), nint, rq ? hedg.data() : nullptr,
                                   rq ? rq->nbins : 0, CRIMP_GRID_MFMA, hooks);
            g_last_grid_norms = plan.nc;
            rc = R.upload_plan();
            if (rc) return rc;
        } else {  // Nelder-Mead starts from the template (norm0, phShift 0) (measureToAs.py:301)
            hstart.resize((size_t)(2 * nint));
            for (int64_t i = 0; i < nint; ++i) {
                hstart[(size_t)(2 * i)] = norm0;
                hstart[(size_t)(2 * i + 1)] = 0.0;
            }
            HIPCHK(h2d_async(s, R.dstart, hstart.data(), 2 * nint * sizeof(double)));
        }
        if (!R.vary_amps && !CRIMP_FIT_MOMENTS) HIPCHK(sc.alloc(&R.hcache, (size_t)hoff[nint]));
        ht.mark("setup");
        if (rq && !call.timed) {
            // launched here, once the grid's uploads are queued: launched with the staging above, its blocks held every
            // CU while the uploads' copy kernels waited for one (the grid started ~180 us late, rocprofv3 trace)
            rc = toa_hist_aux(s, R.dx, R.doff, dedg, rq->nbins, nint, hoff[nint], R.dcnt, &ebin);
            if (rc) return rc;
        }
        rc = R.all(plan.mode);
        if (rc) return rc;
        ht.mark("launch");
        if (brutemin && (plan.mode & kGridProd8) && !(plan.mode & kGridNoMin)) {
            // the runtime half of the certificates (eight factors, lazy norms): a flagged lattice point reruns the
            // grid and the fits with the full four-factor kernel
            int unsafe = 0;
            HIPCHK(d2h(s, &unsafe, R.dunsafe, sizeof(int)));
            if (unsafe) {
                rc = R.all(plan.mode & ~(kGridProd8 | kGridCert));
                if (rc) return rc;
            }
        }
        ht.mark("unsafe");
        if (rq) {  // redChi2 from the final records
            if (ebin.e) HIPCHK(hipStreamWaitEvent(s, ebin.e, 0));
            k_toa_chi2<<<(unsigned)nint, 64, 0, s>>>(R.dcnt, T, R.de, R.dout, dcen, rq->nbins, rq->nfree, dred);
            HIPCHK(hipGetLastError());
            HIPCHK(copy_back(s, rq->out, dred, (size_t)nint, dev));
        }
        HIPCHK(copy_back(s, out, R.dout, (size_t)nint * 8, dev));
        HIPCHK(hipStreamSynchronize(s));
        ht.mark("chi2+sync");
    }
    return finish(s, flags);
}

extern "C" int crimp_toa_fit(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                             const double* exposure, double norm0, int32_t ph_shift_res, int32_t options, double* out,
                             uint32_t flags, void* stream) {
    return toa_fit_impl(x, offsets, nint, tpl, exposure, norm0, ph_shift_res, options, out, flags, stream, nullptr);
}

extern "C" int crimp_toa_fit_redchi2(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                                     const double* exposure, double norm0, int32_t ph_shift_res, int32_t options,
                                     const double* edges, const double* centers, int32_t nbins, int32_t nfree,
                                     double* out, double* redchi2, uint32_t flags, void* stream) {
    ARGCHK(nbins >= 1 && nbins <= 256, "bad sizes (nbins must be 1..256)");
    ARGCHK(edges != nullptr && centers != nullptr && redchi2 != nullptr, "null argument");
    const RedChi2Req rq{edges, centers, nbins, nfree, redchi2};
    return toa_fit_impl(x, offsets, nint, tpl, exposure, norm0, ph_shift_res, options, out, flags, stream, &rq);
}

extern "C" int crimp_toa_grid(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                              const double* norm, int64_t nnorm, const double* phi, int64_t nphi, double* lnsum,
                              double* hmin, uint32_t flags, void* stream) {
    ARGCHK(nint >= 1 && nnorm >= 1 && nphi >= 1, "bad sizes");
    ARGCHK(nphi <= (1 << 24) && nnorm <= (1 << 20), "grid too large");
    ARGCHK(x != nullptr && offsets != nullptr && norm != nullptr && phi != nullptr && lnsum != nullptr &&
               hmin != nullptr,
           "null argument");
    TplDev T;
    int rc = make_tpl(tpl, &T);
    if (rc) return rc;
    ARGCHK(T.K <= kGridKMax, "brute grid supports at most 8 template components");
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    std::vector<int64_t> hoff;
    int64_t maxn = 0;
    rc = read_offsets(call, offsets, nint, false, "offsets must be non-decreasing", &hoff, &maxn);
    if (rc) return rc;
    {
        Scratch sc(s);
        const double *dx = nullptr, *dnrm = nullptr, *dphi = nullptr;
        const int64_t* doff = nullptr;
        HIPCHK(stage_in(sc, x, (size_t)hoff[nint], dev, &dx));
        HIPCHK(stage_in(sc, offsets, (size_t)nint + 1, dev, &doff));
        HIPCHK(stage_in(sc, norm, (size_t)(nint * nnorm), dev, &dnrm));
        HIPCHK(stage_in(sc, phi, (size_t)nphi, dev, &dphi));
        ARGCHK(nint <= 65535, "at most 65535 intervals per brute-grid call");
        TplDev* dT = nullptr;
        HIPCHK(sc.alloc(&dT, 1));
        HIPCHK(h2d(dT, &T, sizeof(T)));
        double *pl = nullptr, *ph = nullptr;
        int64_t splits = 0;
        rc = toa_grid_partials(sc, s, dx, doff, dT, T, dnrm, nnorm, dphi, nphi, nint, maxn, &pl, &ph, &splits);
        if (rc) return rc;
        // combine splits on the host in a fixed order (deterministic)
        std::vector<double> hl((size_t)(splits * nint * nnorm * nphi)), hh((size_t)(splits * nint * nphi));
        HIPCHK(d2h(s, hl.data(), pl, hl.size() * sizeof(double)));
        HIPCHK(d2h(s, hh.data(), ph, hh.size() * sizeof(double)));
        const int64_t L = nint * nnorm * nphi, H = nint * nphi;
        std::vector<double> rl((size_t)L), rh((size_t)H);
        for (int64_t k = 0; k < L; ++k) {
            double v = 0.0;
            for (int64_t sp = 0; sp < splits; ++sp) v += hl[(size_t)(sp * L + k)];
            rl[(size_t)k] = v * 0.69314718055994530942;  // log2 -> ln
        }
        for (int64_t k = 0; k < H; ++k) {
            double v = INFINITY;
            for (int64_t sp = 0; sp < splits; ++sp) v = std::min(v, hh[(size_t)(sp * H + k)]);
            rh[(size_t)k] = v;
        }
        if (dev) {
            HIPCHK(h2d(lnsum, rl.data(), L * sizeof(double)));
            HIPCHK(h2d(hmin, rh.data(), H * sizeof(double)));
            HIPCHK(hipStreamSynchronize(s));
        } else {
            std::memcpy(lnsum, rl.data(), L * sizeof(double));
            std::memcpy(hmin, rh.data(), H * sizeof(double));
        }
    }
    return finish(s, flags);
}

extern "C" int crimp_toa_shape_points(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpls,
                                      const double* aux, const int64_t* pt_interval, const double* pt_norm,
                                      const double* pt_phi, int64_t npts, double* out, uint32_t flags, void* stream) {
    ARGCHK(nint >= 1 && npts >= 0, "bad sizes");
    ARGCHK(x != nullptr && offsets != nullptr && tpls != nullptr && pt_interval != nullptr && pt_norm != nullptr &&
               pt_phi != nullptr && out != nullptr,
           "null argument");
    ARGCHK(npts <= 2147483647LL, "too many points");
    if (npts == 0) return CRIMP_OK;
    // templates and point intervals are host arrays (checked here); photons, norms, phases and out may be device
    for (int64_t p = 0; p < npts; ++p) {
        ARGCHK(tpls[p].ncomp >= 1 && tpls[p].ncomp <= CRIMP_MAX_COMP, "ncomp out of range");
        ARGCHK(tpls[p].model >= 0 && tpls[p].model <= 2, "unknown template model");
        ARGCHK(pt_interval[p] >= 0 && pt_interval[p] < nint, "point interval out of range");
    }
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    std::vector<int64_t> hoff;
    const int rc = read_offsets(call, offsets, nint, false, "offsets must be non-decreasing", &hoff);
    if (rc) return rc;
    {
        Scratch sc(s);
        const double *dx = nullptr, *dn = nullptr, *dp = nullptr;
        const int64_t* doff = nullptr;
        double* dout = nullptr;
        HIPCHK(stage_in(sc, x, (size_t)hoff[nint], dev, &dx));
        HIPCHK(stage_in(sc, offsets, (size_t)nint + 1, dev, &doff));
        HIPCHK(stage_in(sc, pt_norm, (size_t)npts, dev, &dn));
        HIPCHK(stage_in(sc, pt_phi, (size_t)npts, dev, &dp));
        HIPCHK(stage_out(sc, out, (size_t)npts * kShapeSums, dev, &dout));
        crimp_template* dT = nullptr;
        int64_t* dpi = nullptr;
        double* daux = nullptr;
        HIPCHK(sc.alloc(&dT, (size_t)npts));
        HIPCHK(sc.alloc(&dpi, (size_t)npts));
        HIPCHK(h2d(dT, tpls, npts * sizeof(crimp_template)));
        HIPCHK(h2d(dpi, pt_interval, npts * sizeof(int64_t)));
        if (aux != nullptr) {
            HIPCHK(sc.alloc(&daux, (size_t)npts * CRIMP_MAX_COMP));
            HIPCHK(h2d(daux, aux, npts * CRIMP_MAX_COMP * sizeof(double)));
        }
        // one launch per run of points sharing a model (the kernel is specialised per model)
        for (int64_t p0 = 0; p0 < npts;) {
            int64_t p1 = p0 + 1;
            while (p1 < npts && tpls[p1].model == tpls[p0].model) ++p1;
            const unsigned nb = (unsigned)(p1 - p0);
            const double* da = daux != nullptr ? daux + p0 * CRIMP_MAX_COMP : nullptr;
            if (tpls[p0].model == CRIMP_MODEL_FOURIER)
                k_toa_shape<CRIMP_MODEL_FOURIER><<<nb, kShapeBlock, 0, s>>>(dx, doff, dT + p0, da, dpi + p0, dn + p0,
                                                                            dp + p0, dout + p0 * kShapeSums);
            else if (tpls[p0].model == CRIMP_MODEL_CAUCHY)
                k_toa_shape<CRIMP_MODEL_CAUCHY><<<nb, kShapeBlock, 0, s>>>(dx, doff, dT + p0, da, dpi + p0, dn + p0,
                                                                           dp + p0, dout + p0 * kShapeSums);
            else
                k_toa_shape<CRIMP_MODEL_VONMISES><<<nb, kShapeBlock, 0, s>>>(dx, doff, dT + p0, da, dpi + p0, dn + p0,
                                                                             dp + p0, dout + p0 * kShapeSums);
            p0 = p1;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(copy_back(s, out, dout, (size_t)npts * kShapeSums, dev));
        HIPCHK(hipStreamSynchronize(s));
    }
    return finish(s, flags);
}

extern "C" int crimp_toa_redchi2(const double* x, const int64_t* offsets, int64_t nint, const crimp_template* tpl,
                                 const double* exposure, const double* records, const double* edges,
                                 const double* centers, int32_t nbins, int32_t nfree, double* out, uint32_t flags,
                                 void* stream) {
    ARGCHK(nint >= 1 && nbins >= 1 && nbins <= 256, "bad sizes (nbins must be 1..256)");
    ARGCHK(x != nullptr && offsets != nullptr && exposure != nullptr && records != nullptr && edges != nullptr &&
               centers != nullptr && out != nullptr, "null argument");
    ARGCHK(nint <= 2147483647LL, "too many intervals");
    TplDev T;
    int rc = make_tpl(tpl, &T);
    if (rc) return rc;
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    int64_t ntot = 0;
    if (dev)
        HIPCHK(d2h(s, &ntot, offsets + nint, sizeof(int64_t)));
    else
        ntot = offsets[nint];
    {
        Scratch sc(s);
        const double *dx = nullptr, *de = nullptr, *dc = nullptr, *dexp = nullptr, *drec = nullptr;
        const int64_t* doff = nullptr;
        double* dout = nullptr;
        unsigned long long* dcnt = nullptr;
        HIPCHK(stage_in(sc, x, (size_t)ntot, dev, &dx));
        HIPCHK(stage_in(sc, offsets, (size_t)nint + 1, dev, &doff));
        HIPCHK(stage_in(sc, exposure, (size_t)nint, dev, &dexp));
        HIPCHK(stage_in(sc, records, (size_t)nint * 8, dev, &drec));
        HIPCHK(stage_in(sc, edges, (size_t)nbins + 1, dev, &de));
        HIPCHK(stage_in(sc, centers, (size_t)nbins, dev, &dc));
        HIPCHK(stage_out(sc, out, (size_t)nint, dev, &dout));
        HIPCHK(sc.alloc(&dcnt, (size_t)(nint * nbins)));
        HIPCHK(hipMemsetAsync(dcnt, 0, (size_t)(nint * nbins) * sizeof(unsigned long long), s));
        const int64_t ns = bin_splits(ntot, nint);
        KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
        kt.start();
        k_binphases<<<dim3((unsigned)nint, (unsigned)ns), 64 * kBinWaves, 0, s>>>(dx, doff, de, nbins, dcnt);
        k_toa_chi2<<<(unsigned)nint, 64, 0, s>>>(dcnt, T, dexp, drec, dc, nbins, nfree, dout);
        HIPCHK(hipGetLastError());
        kt.stop();
        HIPCHK(copy_back(s, out, dout, (size_t)nint, dev));
    }
    return finish(s, flags);
}

extern "C" int crimp_binphases(const double* x, const int64_t* offsets, int64_t nint, const double* edges,
                               int32_t nbins, int64_t* counts, uint32_t flags, void* stream) {
    ARGCHK(nint >= 1 && nbins >= 1 && nbins <= 256, "bad sizes (nbins must be 1..256)");
    ARGCHK(x != nullptr && offsets != nullptr && edges != nullptr && counts != nullptr, "null argument");
    ARGCHK(nint <= 2147483647LL, "too many intervals");
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    int64_t ntot = 0;
    if (dev)
        HIPCHK(d2h(s, &ntot, offsets + nint, sizeof(int64_t)));
    else
        ntot = offsets[nint];
    {
        Scratch sc(s);
        const double *dx = nullptr, *de = nullptr;
        const int64_t* doff = nullptr;
        int64_t* dc = nullptr;
        HIPCHK(stage_in(sc, x, (size_t)ntot, dev, &dx));
        HIPCHK(stage_in(sc, offsets, (size_t)nint + 1, dev, &doff));
        HIPCHK(stage_in(sc, edges, (size_t)nbins + 1, dev, &de));
        HIPCHK(stage_out(sc, counts, (size_t)(nint * nbins), dev, &dc));
        const int64_t ns = bin_splits(ntot, nint);
        HIPCHK(hipMemsetAsync(dc, 0, (size_t)(nint * nbins) * sizeof(int64_t), s));
        k_binphases<<<dim3((unsigned)nint, (unsigned)ns), 64 * kBinWaves, 0, s>>>(
            dx, doff, de, nbins, reinterpret_cast<unsigned long long*>(dc));
        HIPCHK(hipGetLastError());
        HIPCHK(copy_back(s, counts, dc, (size_t)(nint * nbins), dev));
    }
    return finish(s, flags);
}

// edges[nb + 1] finite and strictly ascending (np.histogramdd's own demand)
static bool cube_edges_ok(const double* e, int nb) {
    for (int i = 0; i <= nb; ++i)
        if (!std::isfinite(e[i]) || (i > 0 && !(e[i] > e[i - 1]))) return false;
    return true;
}

extern "C" int crimp_phase_cube(const double* x, int64_t n, const crimp_timing_model* model, const double* y,
                                const double* y_edges, int32_t ny, const double* z, const double* z_edges, int32_t nz,
                                const double* ph_edges, const int32_t* nph, int64_t* counts, int32_t options,
                                uint32_t flags, void* stream) {
    ARGCHK(n >= 0 && n <= (int64_t(1) << 40), "n out of range");
    ARGCHK(counts != nullptr && ph_edges != nullptr && nph != nullptr && (x != nullptr || n == 0), "null argument");
    ARGCHK((options & ~(CRIMP_CUBE_Y_OPEN_LAST | CRIMP_CUBE_Z_OPEN_LAST | CRIMP_CUBE_Y_IS_X |
                        CRIMP_CUBE_PH_OPEN_LAST)) == 0, "unknown option bits");
    ARGCHK(ny >= 1 && ny <= CRIMP_CUBE_MAX_BINS && nz >= 1 && nz <= CRIMP_CUBE_MAX_BINS,
           "ny and nz must be 1..CRIMP_CUBE_MAX_BINS");
    const bool y_is_x = options & CRIMP_CUBE_Y_IS_X;
    ARGCHK(!(y_is_x && y != nullptr), "CRIMP_CUBE_Y_IS_X takes y = NULL");
    const bool has_y = y != nullptr || y_is_x, has_z = z != nullptr;
    ARGCHK(has_y || ny == 1, "y == NULL is an axis of one bin: ny must be 1");
    ARGCHK(has_z || nz == 1, "z == NULL is an axis of one bin: nz must be 1");
    ARGCHK(!has_y || y_edges != nullptr, "y_edges missing");
    ARGCHK(!has_z || z_edges != nullptr, "z_edges missing");
    ARGCHK(!has_y || cube_edges_ok(y_edges, ny), "y_edges must be finite and strictly ascending");
    ARGCHK(!has_z || cube_edges_ok(z_edges, nz), "z_edges must be finite and strictly ascending");
    std::vector<int32_t> zoff((size_t)nz + 1, 0);
    for (int j = 0; j < nz; ++j) {
        ARGCHK(nph[j] >= 1 && nph[j] <= CRIMP_CUBE_MAX_BINS, "nph must be 1..CRIMP_CUBE_MAX_BINS");
        zoff[(size_t)j + 1] = zoff[(size_t)j] + nph[j];
        ARGCHK(zoff[(size_t)j + 1] + j + 1 <= CRIMP_CUBE_MAX_PH_EDGES, "more than CRIMP_CUBE_MAX_PH_EDGES phase edges");
        ARGCHK(cube_edges_ok(ph_edges + zoff[(size_t)j] + j, nph[j]), "ph_edges must be finite and strictly ascending");
    }
    if (model != nullptr) {
        ARGCHK(model->n_glitch >= 0 && model->n_glitch <= CRIMP_MAX_GLITCH, "n_glitch out of range");
        ARGCHK(model->n_wave >= 0 && model->n_wave <= CRIMP_MAX_WAVE, "n_wave out of range");
        if (const int rc = check_binary(model)) return rc;
    }
    CubeDims D{};
    D.ny = ny;
    D.nz = nz;
    D.has_y = has_y;
    D.has_z = has_z;
    D.y_is_x = y_is_x;
    D.S = zoff[(size_t)nz];
    D.cells = ny * D.S;
    D.nph_edges = D.S + nz;
    cube_copies(D.cells, &D.stride, &D.R);
    D.open_y = (options & CRIMP_CUBE_Y_OPEN_LAST) != 0;
    D.open_z = (options & CRIMP_CUBE_Z_OPEN_LAST) != 0;
    D.open_p = (options & CRIMP_CUBE_PH_OPEN_LAST) != 0;
    D.fused = model != nullptr;
    // the lookup of every axis: estimate-and-step where the edges allow it (numpy.linspace's do), else a binary search
    std::vector<double> psc((size_t)nz);
    D.uni_y = has_y && cube_axis_uniform(y_edges, ny);
    D.uni_z = has_z && cube_axis_uniform(z_edges, nz);
    D.sc_y = has_y ? cube_axis_scale(y_edges, ny) : 0.0;
    D.sc_z = has_z ? cube_axis_scale(z_edges, nz) : 0.0;
    D.it_y = cube_search_steps(ny);
    D.it_z = cube_search_steps(nz);
    D.uni_p = 1;
    D.it_p = 0;
    for (int j = 0; j < nz; ++j) {
        const double* e = ph_edges + zoff[(size_t)j] + j;
        psc[(size_t)j] = cube_axis_scale(e, nph[j]);
        D.uni_p = D.uni_p && cube_axis_uniform(e, nph[j]);
        D.it_p = std::max(D.it_p, cube_search_steps(nph[j]));
    }
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    // a model with an orbit is folded at the emission time (crimp_calcphase's parts 7 | 8)
    const bool bin = model != nullptr && wants_binary(model, 7 | CRIMP_PART_EMISSION);
    CPArgs<false> hm{};
    if (model) make_cpmodel(model, 7, &hm.m);
    CPArgs<true> hb{};
    if (bin) {
        hb.m = hm.m;
        make_binmodel(model, &hb.b);
    }
    {
        Scratch sc(s);
        const double *dx = nullptr, *dy = nullptr, *dz = nullptr;
        int64_t* dc = nullptr;
        HIPCHK(stage_out(sc, counts, (size_t)D.cells, dev, &dc));
        HIPCHK(hipMemsetAsync(dc, 0, (size_t)D.cells * sizeof(int64_t), s));
        if (n > 0) {
            HIPCHK(stage_in(sc, x, (size_t)n, dev, &dx));
            HIPCHK(stage_in(sc, y, (size_t)n, dev, &dy));
            HIPCHK(stage_in(sc, z, (size_t)n, dev, &dz));
            // the edge tables in the kernel's LDS order, and the column offsets: one small upload each
            std::vector<double> tab;
            if (has_y) tab.insert(tab.end(), y_edges, y_edges + ny + 1);
            if (has_z) tab.insert(tab.end(), z_edges, z_edges + nz + 1);
            tab.insert(tab.end(), ph_edges, ph_edges + D.nph_edges);
            tab.insert(tab.end(), psc.begin(), psc.end());
            double* dtab = nullptr;
            int32_t* dzoff = nullptr;
            HIPCHK(sc.alloc(&dtab, tab.size()));
            HIPCHK(sc.alloc(&dzoff, zoff.size()));
            pin_begin((tab.size() * sizeof(double) + 255 + zoff.size() * sizeof(int32_t) + 255));
            HIPCHK(h2d_async(s, dtab, tab.data(), tab.size() * sizeof(double)));
            HIPCHK(h2d_async(s, dzoff, zoff.data(), zoff.size() * sizeof(int32_t)));
            const bool vec = ((reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dy) |
                               reinterpret_cast<uintptr_t>(dz)) & 15u) == 0;
            const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(vec ? n / 2 : n, kCubeBlock),
                                                                             kCubeMaxBlocks));
            const size_t lds = cube_lds_bytes(D);
            KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
            kt.start();
            if (bin) {
                auto kern = vec ? (cube_is_map(D) ? k_phase_cube<true, true, true> : k_phase_cube<true, false, true>)
                                : (cube_is_map(D) ? k_phase_cube<false, true, true> : k_phase_cube<false, false, true>);
                kern<<<blocks, kCubeBlock, lds, s>>>(dx, dy, dz, n, hb, dtab, dzoff, D,
                                                     reinterpret_cast<unsigned long long*>(dc));
            } else {
                auto kern = vec ? (cube_is_map(D) ? k_phase_cube<true, true, false> : k_phase_cube<true, false, false>)
                                : (cube_is_map(D) ? k_phase_cube<false, true, false>
                                                  : k_phase_cube<false, false, false>);
                kern<<<blocks, kCubeBlock, lds, s>>>(dx, dy, dz, n, hm, dtab, dzoff, D,
                                                     reinterpret_cast<unsigned long long*>(dc));
            }
            HIPCHK(hipGetLastError());
            kt.stop();
        }
        HIPCHK(copy_back(s, counts, dc, (size_t)D.cells, dev));
    }
    return finish(s, flags);
}

// ---- timing-model fits of ToAs (timing_fit.h)
// the kernels' form of the per-problem models and of the map, with every check of crimp_timing_nll / _mcmc on them.
// orbit_fields (crimp_orbit_nll / _mcmc; else null): BINARY slots are admitted, the mask of the orbit fields they name
// is returned there, and the bases' binary blocks are not read.
static int tf_prepare(const int64_t* h_off, int64_t nprob, const crimp_timing_model* fit_base,
                      const crimp_timing_model* wave_base, const crimp_fit_map* map, std::vector<TFModel>* models,
                      TFMap* dm, uint32_t* orbit_fields = nullptr) {
    ARGCHK(nprob >= 1 && nprob <= (int64_t(1) << 24), "nprob out of range");
    ARGCHK(fit_base != nullptr && wave_base != nullptr && map != nullptr, "null argument");
    ARGCHK(map->ndim >= 1 && map->ndim <= CRIMP_FIT_MAX_DIM, "ndim must be 1..CRIMP_FIT_MAX_DIM");
    ARGCHK(map->branch >= CRIMP_FIT_WAVES_FIXED && map->branch <= CRIMP_FIT_WAVES_MIXED, "unknown branch");
    ARGCHK(map->f0_param >= -1 && map->f0_param < map->ndim, "f0_param out of range");
    *dm = TFMap{};
    if (orbit_fields) *orbit_fields = 0;
    dm->ndim = map->ndim;
    dm->f0_param = map->f0_param;
    double fact = 1.0;
    for (int k = 0; k < 13; ++k) {
        fact *= (double)(k + 1);
        dm->inv_fact[k] = 1.0 / fact;
    }
    int top_f = 0, top_gl = -1, top_wv = -1;
    for (int k = 0; k < map->ndim; ++k) {
        const crimp_fit_slot& sl = map->slot[k];
        if (sl.kind == CRIMP_FIT_SLOT_F) {
            ARGCHK(sl.index >= 0 && sl.index <= 12, "slot names an F term outside F0..F12");
            top_f = std::max(top_f, sl.index + 1);
        } else if (sl.kind == CRIMP_FIT_SLOT_GLITCH) {
            ARGCHK(sl.index >= 0 && sl.index < CRIMP_MAX_GLITCH && sl.sub >= 0 && sl.sub <= 6,
                   "slot names a glitch field outside the model");
            top_gl = std::max(top_gl, sl.index);
        } else if (sl.kind == CRIMP_FIT_SLOT_WAVE) {
            ARGCHK(sl.index >= 0 && sl.index < CRIMP_MAX_WAVE && sl.sub >= 0 && sl.sub <= 1,
                   "slot names a wave field outside the model");
            ARGCHK(map->branch != CRIMP_FIT_WAVES_FIXED, "a wave slot with CRIMP_FIT_WAVES_FIXED");
            top_wv = std::max(top_wv, sl.index);
        } else if (sl.kind == CRIMP_FIT_SLOT_BINARY) {
            ARGCHK(orbit_fields != nullptr, "a BINARY slot: crimp_orbit_nll and crimp_orbit_mcmc fit the orbit");
            ARGCHK(sl.index >= 0 && sl.index < kOfFields,
                   "slot names an orbit field outside CRIMP_ORBIT_PB..CRIMP_ORBIT_A1DOT");
            ARGCHK(!(*orbit_fields >> sl.index & 1u), "two slots name one orbit field");
            *orbit_fields |= 1u << sl.index;
        } else {
            return set_err(CRIMP_ERR_ARG, "unknown slot kind");
        }
        ARGCHK(k != map->f0_param || (sl.kind == CRIMP_FIT_SLOT_F && sl.index == 0), "f0_param is not an F0 slot");
        dm->kind[k] = sl.kind;
        dm->a[k] = sl.index;
        dm->b[k] = sl.kind == CRIMP_FIT_SLOT_F ? 0 : sl.sub;
    }
    models->resize((size_t)nprob);
    for (int64_t i = 0; i < nprob; ++i) {
        const crimp_timing_model &fm = fit_base[i], &wm = wave_base[i];
        ARGCHK(h_off[i + 1] - h_off[i] <= (int64_t(1) << 30), "a problem has too many ToAs");
        ARGCHK(fm.n_glitch >= 0 && fm.n_glitch <= CRIMP_MAX_GLITCH, "n_glitch out of range");
        ARGCHK(fm.n_wave >= 0 && fm.n_wave <= CRIMP_MAX_WAVE && wm.n_wave >= 0 && wm.n_wave <= CRIMP_MAX_WAVE,
               "n_wave out of range");
        ARGCHK(orbit_fields != nullptr || (fm.binary == CRIMP_BINARY_NONE && wm.binary == CRIMP_BINARY_NONE),
               "binary models are not fitted yet");
        ARGCHK(top_gl < fm.n_glitch, "slot names a glitch outside the model");
        ARGCHK(top_wv < fm.n_wave, "slot names a wave harmonic outside the model");
        TFModel& tm = (*models)[(size_t)i];
        make_cpmodel(&fm, map->branch == CRIMP_FIT_WAVES_ONLY ? 4 : 7, &tm.m);
        tm.m.nterms = std::max(tm.m.nterms, top_f);
        if (map->branch == CRIMP_FIT_WAVES_FIXED) {  // utilities_fittoas.py:283: the full model's waves
            tm.m.n_wave = wm.n_wave;
            tm.m.wave_epoch = wm.wave_epoch;
            tm.m.wave_om = wm.wave_om;
            std::memcpy(tm.m.wave_ab, wm.wave_ab, sizeof(tm.m.wave_ab));
        }
        tm.f0_base = wm.f[0];
        tm.m.f0 = wm.f[0];
    }
    return CRIMP_OK;
}

// offsets on the host (the checks and the LDS plan need the ToA counts)
static int tf_host_offsets(const Call& c, const int64_t* offsets, int64_t nprob, std::vector<int64_t>* h) {
    ARGCHK(offsets != nullptr && nprob >= 1 && nprob <= (int64_t(1) << 24), "nprob out of range");
    const int rc = read_offsets(c, offsets, nprob, true, "a problem has no ToAs", h);
    if (rc) return rc;
    ARGCHK((*h)[0] == 0, "offsets[0] must be 0");
    return CRIMP_OK;
}

// What a ToA-fit call holds after its host checks, binary-free (TimingLik) or under an orbit (OrbitLik): the offsets,
// the problems' models in the kernels' form, the map and (the orbit's calls) the par spin models of the prologue
template <class Lik>
struct FitCall {
    std::vector<int64_t> h_off;
    std::vector<typename Lik::Base> models;
    std::vector<CPModel> parm;
    TFMap dm;
};
template <class Lik>
constexpr bool kFitOrbit = std::is_same<Lik, OrbitLik>::value;

static int fit_prepare(const Call& call, const int64_t* offsets, int64_t nprob, const crimp_timing_model*,
                       const crimp_timing_model* fit_base, const crimp_timing_model* wave_base,
                       const crimp_fit_map* map, FitCall<TimingLik>* c) {
    const int rc = tf_host_offsets(call, offsets, nprob, &c->h_off);
    if (rc != CRIMP_OK) return rc;
    return tf_prepare(c->h_off.data(), nprob, fit_base, wave_base, map, &c->models, &c->dm);
}

// the orbit's calls: par is required (checked before the offsets are read), BINARY slots are admitted
static int fit_prepare(const Call& call, const int64_t* offsets, int64_t nprob, const crimp_timing_model* par,
                       const crimp_timing_model* fit_base, const crimp_timing_model* wave_base,
                       const crimp_fit_map* map, FitCall<OrbitLik>* c) {
    ARGCHK(par != nullptr, "null argument");
    int rc = tf_host_offsets(call, offsets, nprob, &c->h_off);
    if (rc != CRIMP_OK) return rc;
    std::vector<TFModel> tf;
    uint32_t fields = 0;
    rc = tf_prepare(c->h_off.data(), nprob, fit_base, wave_base, map, &tf, &c->dm, &fields);
    if (rc != CRIMP_OK) return rc;
    constexpr uint32_t bt_only = 1u << CRIMP_ORBIT_ECC | 1u << CRIMP_ORBIT_OM | 1u << CRIMP_ORBIT_OMDOT |
                                 1u << CRIMP_ORBIT_GAMMA;
    constexpr uint32_t ell1_only = 1u << CRIMP_ORBIT_EPS1 | 1u << CRIMP_ORBIT_EPS2;
    c->models.resize((size_t)nprob);
    c->parm.resize((size_t)nprob);
    for (int64_t i = 0; i < nprob; ++i) {
        const crimp_timing_model& pm = par[i];
        ARGCHK(pm.binary != CRIMP_BINARY_NONE, "the model has no binary");
        rc = check_binary(&pm);
        if (rc != CRIMP_OK) return rc;
        ARGCHK(!(fields & (pm.binary == CRIMP_BINARY_BT ? ell1_only : bt_only)),
               "slot names an orbit field the model's kind does not have");
        ARGCHK(pm.n_glitch >= 0 && pm.n_glitch <= CRIMP_MAX_GLITCH, "n_glitch out of range");
        ARGCHK(pm.n_wave >= 0 && pm.n_wave <= CRIMP_MAX_WAVE, "n_wave out of range");
        OFModel& m = c->models[(size_t)i];
        m.tf = tf[(size_t)i];
        m.ob = OFOrbit{};
        m.ob.kind = pm.binary;
        double* r = m.ob.raw;
        r[CRIMP_ORBIT_PB] = pm.bin_pb;
        r[CRIMP_ORBIT_A1] = pm.bin_a1;
        r[CRIMP_ORBIT_T0] = pm.bin_t0;
        r[CRIMP_ORBIT_ECC] = pm.bin_ecc;
        r[CRIMP_ORBIT_OM] = pm.bin_om;
        r[CRIMP_ORBIT_OMDOT] = pm.bin_omdot;
        r[CRIMP_ORBIT_GAMMA] = pm.bin_gamma;
        r[CRIMP_ORBIT_EPS1] = pm.bin_eps1;
        r[CRIMP_ORBIT_EPS2] = pm.bin_eps2;
        r[CRIMP_ORBIT_PBDOT] = pm.bin_pbdot;
        r[CRIMP_ORBIT_A1DOT] = pm.bin_a1dot;
        make_cpmodel(&pm, 7, &c->parm[(size_t)i]);
    }
    return CRIMP_OK;
}

// The device side of a call: the arrays of all problems as the kernels take them, the offsets, the models and the map
template <class Lik>
struct FitDev {
    typename Lik::Data d{};
    const int64_t* off = nullptr;
    typename Lik::Base* mod = nullptr;
    TFMap* map = nullptr;
    CPModel* par = nullptr;  // the orbit's calls: the prologue's models, and the constants it writes
    double* consts = nullptr;
};

// the device copies of a FitCall; for the orbit also the room of the per-ToA constants, the arrays d.a[3..5]
template <class Lik>
static hipError_t fit_upload(Scratch& sc, const FitCall<Lik>& c, size_t ntoa, FitDev<Lik>* D) {
    hipError_t e;
    if ((e = sc.alloc(&D->mod, c.models.size())) != hipSuccess) return e;
    if ((e = sc.alloc(&D->map, 1)) != hipSuccess) return e;
    if ((e = h2d(D->mod, c.models.data(), c.models.size() * sizeof(typename Lik::Base))) != hipSuccess) return e;
    if ((e = h2d(D->map, &c.dm, sizeof(TFMap))) != hipSuccess) return e;
    if constexpr (kFitOrbit<Lik>) {
        if ((e = sc.alloc(&D->par, c.parm.size())) != hipSuccess) return e;
        if ((e = sc.alloc(&D->consts, 3 * ntoa)) != hipSuccess) return e;
        if ((e = h2d(D->par, c.parm.data(), c.parm.size() * sizeof(CPModel))) != hipSuccess) return e;
        for (int k = 0; k < 3; ++k) D->d.a[3 + k] = D->consts + (size_t)k * ntoa;
    }
    return hipSuccess;
}

// the launches before a call's kernel: the orbit's per-ToA constants (part of a call's timed cost)
template <class Lik>
static hipError_t fit_prologue(hipStream_t s, int64_t nprob, size_t ntoa, const FitDev<Lik>& D) {
    if constexpr (kFitOrbit<Lik>)
        k_orbit_prologue<<<(unsigned)nprob, 256, 0, s>>>(D.d.a[0], D.off, D.mod, D.par, (int64_t)ntoa, D.consts);
    return hipGetLastError();
}

// crimp_timing_nll and crimp_orbit_nll (par: the orbit's call alone)
template <class Lik>
static int fit_nll_call(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets,
                        int64_t nprob, const crimp_timing_model* par, const crimp_timing_model* fit_base,
                        const crimp_timing_model* wave_base, const crimp_fit_map* map, const double* pvec, int64_t P,
                        double* nll, double* mu, uint32_t flags, void* stream) {
    ARGCHK(t_mjd != nullptr && y != nullptr && yerr != nullptr && pvec != nullptr && nll != nullptr, "null argument");
    ARGCHK(P >= 1 && P <= (int64_t(1) << 24), "P out of range");
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    FitCall<Lik> c;
    const int rc = fit_prepare(call, offsets, nprob, par, fit_base, wave_base, map, &c);
    if (rc != CRIMP_OK) return rc;
    const int64_t groups = cdiv(P, kTfNllWaves);
    ARGCHK(nprob * groups <= (int64_t(1) << 30), "too many parameter vectors for one launch");
    const size_t ntoa = (size_t)c.h_off[(size_t)nprob], nd = (size_t)c.dm.ndim;
    {
        Scratch sc(s);
        FitDev<Lik> D;
        const double* dp = nullptr;
        double *dnll = nullptr, *dmu = nullptr;
        HIPCHK(stage_in(sc, t_mjd, ntoa, dev, &D.d.a[0]));
        HIPCHK(stage_in(sc, y, ntoa, dev, &D.d.a[1]));
        HIPCHK(stage_in(sc, yerr, ntoa, dev, &D.d.a[2]));
        HIPCHK(stage_in(sc, offsets, (size_t)nprob + 1, dev, &D.off));
        HIPCHK(stage_in(sc, pvec, (size_t)nprob * (size_t)P * nd, dev, &dp));
        HIPCHK(stage_out(sc, nll, (size_t)nprob * (size_t)P, dev, &dnll));
        HIPCHK(stage_out(sc, mu, (size_t)P * ntoa, dev, &dmu));
        HIPCHK(fit_upload(sc, c, ntoa, &D));
        KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
        kt.start();
        HIPCHK(fit_prologue(s, nprob, ntoa, D));
        k_fit_nll<Lik><<<(unsigned)(nprob * groups), kTfNllWaves * 64, 0, s>>>(D.d, D.off, D.mod, D.map, dp, P, groups,
                                                                               dnll, dmu);
        HIPCHK(hipGetLastError());
        kt.stop();
        HIPCHK(copy_back(s, nll, dnll, (size_t)nprob * (size_t)P, dev));
        HIPCHK(copy_back(s, mu, dmu, (size_t)P * ntoa, dev));
    }
    return finish(s, flags);
}

// crimp_timing_mcmc and crimp_orbit_mcmc (par: the orbit's call alone)
template <class Lik>
static int fit_mcmc_call(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets,
                         int64_t nprob, const crimp_timing_model* par, const crimp_timing_model* fit_base,
                         const crimp_timing_model* wave_base, const crimp_fit_map* map, const double* p0,
                         const double* lo, const double* hi, int32_t W, int64_t steps, uint64_t seed,
                         int64_t first_problem, double* chain, double* logprob, int64_t* accepted, uint32_t flags,
                         void* stream) {
    ARGCHK(t_mjd != nullptr && y != nullptr && yerr != nullptr && p0 != nullptr && lo != nullptr && hi != nullptr &&
               chain != nullptr && logprob != nullptr && accepted != nullptr, "null argument");
    ARGCHK(map != nullptr && map->ndim >= 1 && map->ndim <= CRIMP_FIT_MAX_DIM, "ndim must be 1..CRIMP_FIT_MAX_DIM");
    ARGCHK(W >= 2 && W % 2 == 0 && W <= 256 && W >= 2 * map->ndim, "walkers: even, >= 2 ndim and <= 256");
    ARGCHK(steps >= 1 && steps <= (int64_t(1) << 31), "steps out of range");
    ARGCHK(first_problem >= 0 && first_problem + nprob <= (int64_t(1) << 32), "first_problem out of range");
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    FitCall<Lik> c;
    const int rc = fit_prepare(call, offsets, nprob, par, fit_base, wave_base, map, &c);
    if (rc != CRIMP_OK) return rc;
    const size_t ntoa = (size_t)c.h_off[(size_t)nprob], nd = (size_t)c.dm.ndim, w = (size_t)W;
    int64_t nmax = 0;
    for (int64_t i = 0; i < nprob; ++i) nmax = std::max(nmax, c.h_off[(size_t)i + 1] - c.h_off[(size_t)i]);
    // LDS: positions, log-probabilities, counts, one Lik::Wave per wave; the per-ToA arrays too when the largest
    // problem's fit, else they are read from global memory
    constexpr size_t kLdsCap = 128 * 1024;
    size_t lds = (w * nd + 2 * w) * sizeof(double) + kTfMcWaves * sizeof(typename Lik::Wave);
    const int stage = lds + Lik::kArrays * (size_t)nmax * sizeof(double) <= kLdsCap;
    if (stage) lds += Lik::kArrays * (size_t)nmax * sizeof(double);
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_fit_mcmc<Lik>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCap));
    const size_t rows = (size_t)nprob * (size_t)steps * w;
    {
        Scratch sc(s);
        FitDev<Lik> D;
        const double *dp0 = nullptr, *dlo = nullptr, *dhi = nullptr;
        double *dchain = nullptr, *dlp = nullptr;
        int64_t* dacc = nullptr;
        HIPCHK(stage_in(sc, t_mjd, ntoa, dev, &D.d.a[0]));
        HIPCHK(stage_in(sc, y, ntoa, dev, &D.d.a[1]));
        HIPCHK(stage_in(sc, yerr, ntoa, dev, &D.d.a[2]));
        HIPCHK(stage_in(sc, offsets, (size_t)nprob + 1, dev, &D.off));
        HIPCHK(stage_in(sc, p0, (size_t)nprob * w * nd, dev, &dp0));
        HIPCHK(stage_in(sc, lo, (size_t)nprob * nd, dev, &dlo));
        HIPCHK(stage_in(sc, hi, (size_t)nprob * nd, dev, &dhi));
        HIPCHK(stage_out(sc, chain, rows * nd, dev, &dchain));
        HIPCHK(stage_out(sc, logprob, rows, dev, &dlp));
        HIPCHK(stage_out(sc, accepted, (size_t)nprob * w, dev, &dacc));
        HIPCHK(fit_upload(sc, c, ntoa, &D));
        KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
        kt.start();
        HIPCHK(fit_prologue(s, nprob, ntoa, D));
        k_fit_mcmc<Lik><<<(unsigned)nprob, kTfMcWaves * 64, lds, s>>>(D.d, D.off, D.mod, D.map, dp0, dlo, dhi, (int)W,
                                                                      steps, seed, first_problem, stage, dchain, dlp,
                                                                      dacc);
        HIPCHK(hipGetLastError());
        kt.stop();
        HIPCHK(copy_back(s, chain, dchain, rows * nd, dev));
        HIPCHK(copy_back(s, logprob, dlp, rows, dev));
        HIPCHK(copy_back(s, accepted, dacc, (size_t)nprob * w, dev));
    }
    return finish(s, flags);
}

extern "C" int crimp_timing_nll(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets,
                                int64_t nprob, const crimp_timing_model* fit_base,
                                const crimp_timing_model* wave_base, const crimp_fit_map* map, const double* pvec,
                                int64_t P, double* nll, double* mu, uint32_t flags, void* stream) {
    return fit_nll_call<TimingLik>(t_mjd, y, yerr, offsets, nprob, nullptr, fit_base, wave_base, map, pvec, P, nll, mu,
                                   flags, stream);
}

extern "C" int crimp_timing_mcmc(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets,
                                 int64_t nprob, const crimp_timing_model* fit_base,
                                 const crimp_timing_model* wave_base, const crimp_fit_map* map, const double* p0,
                                 const double* lo, const double* hi, int32_t W, int64_t steps, uint64_t seed,
                                 int64_t first_problem, double* chain, double* logprob, int64_t* accepted,
                                 uint32_t flags, void* stream) {
    return fit_mcmc_call<TimingLik>(t_mjd, y, yerr, offsets, nprob, nullptr, fit_base, wave_base, map, p0, lo, hi, W,
                                    steps, seed, first_problem, chain, logprob, accepted, flags, stream);
}

extern "C" int crimp_orbit_nll(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets,
                               int64_t nprob, const crimp_timing_model* par, const crimp_timing_model* fit_base,
                               const crimp_timing_model* wave_base, const crimp_fit_map* map, const double* pvec,
                               int64_t P, double* nll, double* mu, uint32_t flags, void* stream) {
    return fit_nll_call<OrbitLik>(t_mjd, y, yerr, offsets, nprob, par, fit_base, wave_base, map, pvec, P, nll, mu,
                                  flags, stream);
}

extern "C" int crimp_orbit_mcmc(const double* t_mjd, const double* y, const double* yerr, const int64_t* offsets,
                                int64_t nprob, const crimp_timing_model* par, const crimp_timing_model* fit_base,
                                const crimp_timing_model* wave_base, const crimp_fit_map* map, const double* p0,
                                const double* lo, const double* hi, int32_t W, int64_t steps, uint64_t seed,
                                int64_t first_problem, double* chain, double* logprob, int64_t* accepted,
                                uint32_t flags, void* stream) {
    return fit_mcmc_call<OrbitLik>(t_mjd, y, yerr, offsets, nprob, par, fit_base, wave_base, map, p0, lo, hi, W, steps,
                                   seed, first_problem, chain, logprob, accepted, flags, stream);
}

// ---- orbit search (orbit_search.h; its finalize kernel takes the best trial as crimp_best does, so the header
// follows BestCand)
#include "orbit_search.h"

extern "C" int crimp_orbit_search_plan(int64_t n, int64_t nf, int32_t nharm, int32_t stat, int64_t norb, int64_t* out) {
    ARGCHK(out != nullptr, "null argument");
    ARGCHK(n >= 1 && nf >= 1 && norb >= 1, "n, nf, norb < 1");
    ARGCHK(nharm >= 1 && nharm <= kOsMaxHarm, "nharm outside [1, 256]");
    ARGCHK(stat == CRIMP_STAT_Z2 || stat == CRIMP_STAT_H, "stat must be CRIMP_STAT_Z2 or CRIMP_STAT_H");
    const OrbitSearchPlan P = plan_orbit_search(n, nf, nharm, stat, norb, os_cap_from_env());
    out[0] = P.slice;
    out[1] = P.nslices;
    out[2] = P.J;
    out[3] = P.batch;
    out[4] = P.nbatches;
    out[5] = P.part_elems < 0 ? -1 : P.part_elems * 8;
    return CRIMP_OK;
}

template <bool TWOD>
static void launch_orbit_search(int J, dim3 grid, hipStream_t s, const double* t, int64_t n, const OSArgs& A,
                                const double* orbits, const double* freq, int64_t nf, double* part) {
    switch (J) {
        case 2: k_orbit_search<2, TWOD><<<grid, kOsBlock, 0, s>>>(t, n, A, orbits, freq, nf, part); break;
        case 4: k_orbit_search<4, TWOD><<<grid, kOsBlock, 0, s>>>(t, n, A, orbits, freq, nf, part); break;
        case 8: k_orbit_search<8, TWOD><<<grid, kOsBlock, 0, s>>>(t, n, A, orbits, freq, nf, part); break;
        default: k_orbit_search<16, TWOD><<<grid, kOsBlock, 0, s>>>(t, n, A, orbits, freq, nf, part); break;
    }
}

extern "C" int crimp_orbit_search(const double* t_mjd, int64_t n, const crimp_timing_model* base, double tref_mjd,
                                  const int32_t* keys, int32_t nkeys, const double* orbits, int64_t norb,
                                  const double* freq, int64_t nf, double fdot, int32_t nharm, int32_t stat,
                                  int64_t first, int64_t count, double* power, double* best, uint32_t flags,
                                  void* stream) {
    ARGCHK(n >= 1, "n < 1");
    ARGCHK(nf >= 0 && norb >= 0, "nf or norb < 0");
    ARGCHK(first >= 0 && count >= 0 && first <= norb && count <= norb - first, "orbit range outside [0, norb]");
    ARGCHK(nharm >= 1 && nharm <= kOsMaxHarm, "nharm outside [1, 256]");
    ARGCHK(stat == CRIMP_STAT_Z2 || stat == CRIMP_STAT_H, "stat must be CRIMP_STAT_Z2 or CRIMP_STAT_H");
    ARGCHK(nkeys >= 0 && nkeys <= kOsMaxKeys, "nkeys outside [0, 11]");
    ARGCHK(base != nullptr && t_mjd != nullptr && (keys != nullptr || nkeys == 0), "null argument");
    ARGCHK(base->binary == CRIMP_BINARY_BT || base->binary == CRIMP_BINARY_ELL1, "the model has no binary");
    ARGCHK(std::isfinite(tref_mjd) && std::isfinite(fdot), "tref or fdot is not finite");
    OSArgs A{};
    A.base.kind = base->binary;
    {
        double* r = A.base.raw;
        r[CRIMP_ORBIT_PB] = base->bin_pb;
        r[CRIMP_ORBIT_A1] = base->bin_a1;
        r[CRIMP_ORBIT_T0] = base->bin_t0;
        r[CRIMP_ORBIT_ECC] = base->bin_ecc;
        r[CRIMP_ORBIT_OM] = base->bin_om;
        r[CRIMP_ORBIT_OMDOT] = base->bin_omdot;
        r[CRIMP_ORBIT_GAMMA] = base->bin_gamma;
        r[CRIMP_ORBIT_EPS1] = base->bin_eps1;
        r[CRIMP_ORBIT_EPS2] = base->bin_eps2;
        r[CRIMP_ORBIT_PBDOT] = base->bin_pbdot;
        r[CRIMP_ORBIT_A1DOT] = base->bin_a1dot;
    }
    for (int k = 0; k < kOfFields; ++k) A.col[k] = -1;
    constexpr uint32_t bt_only = 1u << CRIMP_ORBIT_ECC | 1u << CRIMP_ORBIT_OM | 1u << CRIMP_ORBIT_OMDOT |
                                 1u << CRIMP_ORBIT_GAMMA;
    constexpr uint32_t ell1_only = 1u << CRIMP_ORBIT_EPS1 | 1u << CRIMP_ORBIT_EPS2;
    for (int q = 0; q < nkeys; ++q) {
        const int k = keys[q];
        ARGCHK(k >= 0 && k < kOfFields, "key " + std::to_string(q) + " is not a CRIMP_ORBIT_* field");
        ARGCHK(A.col[k] < 0, "two keys name one orbit field");
        ARGCHK(!((1u << k) & (base->binary == CRIMP_BINARY_BT ? ell1_only : bt_only)),
               "key names an orbit field the model's kind does not have");
        A.col[k] = q;
    }
    A.nkeys = nkeys;
    A.tref = tref_mjd;
    A.c2 = 0.5 * fdot;
    A.nharm = nharm;
    if (count == 0 || nf == 0) return CRIMP_OK;
    ARGCHK(freq != nullptr && (orbits != nullptr || nkeys == 0) && (power != nullptr || best != nullptr),
           "null argument");
    for (int64_t j = 0; j < nf; ++j) ARGCHK(std::isfinite(freq[j]), "a trial frequency is not finite");
    // every orbit of the range against the limits of crimp_binary_delay, before anything is launched
    for (int64_t o = first; o < first + count; ++o) {
        double raw[kOfFields];
        for (int k = 0; k < kOfFields; ++k) raw[k] = A.col[k] >= 0 ? orbits[o * nkeys + A.col[k]] : A.base.raw[k];
        if (const char* why = os_orbit_fault(A.base.kind, raw))
            return set_err(CRIMP_ERR_ARG, "orbit " + std::to_string(o) + ": " + why);
    }
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    const OrbitSearchPlan P = plan_orbit_search(n, nf, nharm, stat, count, os_cap_from_env());
    ARGCHK(P.part_elems > 0 && P.nslices <= 0x7fffffff, "orbit search: the partial sums of one orbit do not fit");
    const bool twod = fdot != 0.0;
    {
        Scratch sc(s);
        const double *dt = nullptr, *dfreq = nullptr, *dorb = nullptr;
        double *dpow = nullptr, *dbest = nullptr, *part = nullptr;
        HIPCHK(stage_in(sc, t_mjd, (size_t)n, dev, &dt));
        HIPCHK(stage_in(sc, freq, (size_t)nf, false, &dfreq));
        if (nkeys > 0) HIPCHK(stage_in(sc, orbits + first * nkeys, (size_t)(count * nkeys), false, &dorb));
        HIPCHK(stage_out(sc, power, (size_t)(count * nf), dev, &dpow));
        HIPCHK(stage_out(sc, best, (size_t)(2 * count), dev, &dbest));
        HIPCHK(sc.alloc(&part, (size_t)P.part_elems));
        KernelTimer kt(s, call.timed);
        kt.start();
        for (int64_t b0 = 0; b0 < count; b0 += P.batch) {
            const int64_t ob = std::min<int64_t>(P.batch, count - b0);
            const dim3 grid((unsigned)P.nslices, (unsigned)ob);
            const double* borb = dorb ? dorb + b0 * nkeys : nullptr;
            if (twod)
                launch_orbit_search<true>(P.J, grid, s, dt, n, A, borb, dfreq, nf, part);
            else
                launch_orbit_search<false>(P.J, grid, s, dt, n, A, borb, dfreq, nf, part);
            HIPCHK(hipGetLastError());
            k_orbit_search_finalize<<<(unsigned)ob, 256, 0, s>>>(part, ob, P.nslices, nf, nharm, stat, (double)n,
                                                                 dpow ? dpow + b0 * nf : nullptr,
                                                                 dbest ? dbest + 2 * b0 : nullptr);
            HIPCHK(hipGetLastError());
        }
        kt.stop();
        HIPCHK(copy_back(s, power, dpow, (size_t)(count * nf), dev));
        HIPCHK(copy_back(s, best, dbest, (size_t)(2 * count), dev));
    }
    return finish(s, flags);
}

// ---- photon-domain timing fits (photon_fit.h), binary-free or under an orbit (photon_orbit_fit.h)
// What a call holds after its one prologue: the plan's launch shape, the photon fit model, its map and the template;
// the orbit's calls also par's orbit and par's spin model (the prologue kernel's rates)
struct PFCall {
    PFLaunch L;
    CPModel base;
    PFMap map;
    TplDev T;
    bool orbit = false;
    POFOrbit ob;
    CPModel parm;
};

// every check of a call that does not need the device, and the host plan (photon_fit_plan.h; orbit: the two
// crimp_photon_orbit_* calls, photon_orbit_fit_plan.h)
static int pf_prologue(int64_t n, const crimp_timing_model* par, const crimp_fit_map* map, const crimp_template* tpl,
                       double norm, int32_t phoff, int64_t P, bool orbit, PFCall* c) {
    crimp_timing_model fit;
    int32_t parts = 0, nterms = 1;
    c->orbit = orbit;
    if (const char* e = orbit ? plan_photon_orbit_model(par, map, phoff, &fit, &c->map, &parts, &nterms, &c->ob)
                              : plan_photon_model(par, map, phoff, &fit, &c->map, &parts, &nterms))
        return set_err(CRIMP_ERR_ARG, e);
    if (const int rc = make_tpl(tpl, &c->T)) return rc;
    ARGCHK(std::isfinite(norm) && norm > 0.0, "norm must be positive");
    if (const char* e = plan_photon_launch(n, P, &c->L)) return set_err(CRIMP_ERR_ARG, e);
    make_cpmodel(&fit, parts, &c->base);
    c->base.nterms = nterms;
    c->base.f0 = 1.0;  // the wave coefficients carry F0 (photon_wave_coef)
    if (orbit) make_cpmodel(par, 7, &c->parm);
    return CRIMP_OK;
}

// the device copies every launch of a call reads; the orbit's calls also the room of the per-photon constants
struct PFDev {
    CPModel* base = nullptr;
    PFMap* map = nullptr;
    TplDev* T = nullptr;
    double2* tab = nullptr;
    double *psum = nullptr, *pmin = nullptr;
    CPModel* parm = nullptr;
    double* consts = nullptr;  // [3][n]: tau0, nu, nud
};
static int pf_upload(Scratch& sc, hipStream_t s, const PFCall& c, int64_t n, PFDev* d) {
    if (c.orbit) {
        HIPCHK(sc.alloc(&d->parm, 1));
        HIPCHK(sc.alloc(&d->consts, 3 * (size_t)n));
        HIPCHK(h2d(d->parm, &c.parm, sizeof(CPModel)));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_photon_orbit_nll),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(POFLds)));
    }
    HIPCHK(sc.alloc(&d->base, 1));
    HIPCHK(sc.alloc(&d->map, 1));
    HIPCHK(sc.alloc(&d->T, 1));
    HIPCHK(sc.alloc(&d->tab, (size_t)kSinTab));
    HIPCHK(sc.alloc(&d->psum, (size_t)c.L.partials));
    HIPCHK(sc.alloc(&d->pmin, (size_t)c.L.partials));
    HIPCHK(h2d(d->base, &c.base, sizeof(CPModel)));
    HIPCHK(h2d(d->map, &c.map, sizeof(PFMap)));
    HIPCHK(h2d(d->T, &c.T, sizeof(TplDev)));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_photon_nll), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)sizeof(PFLds)));
    k_photon_table<<<kSinTab / 256, 256, 0, s>>>(d->tab);
    HIPCHK(hipGetLastError());
    return CRIMP_OK;
}

extern "C" int crimp_photon_tile(void) { return kPfTile; }

// the orbit's per-photon constants, once per call (nothing for a binary-free call); part of a call's timed cost
static void pf_launch_prologue(hipStream_t s, const PFCall& c, const PFDev& d, const double* dt, int64_t n) {
    if (c.orbit)
        k_photon_orbit_prologue<<<(unsigned)std::min<int64_t>(cdiv(n, 256), int64_t(1) << 20), 256, 0, s>>>(
            dt, n, c.ob, d.parm, d.consts);
}

// the likelihood kernel of a call on P vectors: (sum ln m, min m) pairs into d.psum / d.pmin
static void pf_launch_nll(hipStream_t s, const PFCall& c, const PFDev& d, const double* dt, const double* dx,
                          int64_t n, double norm, const double* pvec, const int32_t* active, int64_t P,
                          double* delta) {
    const dim3 grid((unsigned)c.L.tiles, (unsigned)cdiv(P, kPfWaves));
    if (c.orbit)
        k_photon_orbit_nll<<<grid, kPfWaves * 64, sizeof(POFLds), s>>>(dt, dx, d.consts, n, d.base, c.ob, d.map, d.T,
                                                                      d.tab, norm, pvec, active, P, d.psum, d.pmin,
                                                                      delta);
    else
        k_photon_nll<<<grid, kPfWaves * 64, sizeof(PFLds), s>>>(dt, dx, n, d.base, d.map, d.T, d.tab, norm, pvec,
                                                                active, P, d.psum, d.pmin, delta);
}

// crimp_photon_nll and (orbit) crimp_photon_orbit_nll
static int photon_nll_call(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                           const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                           const double* pvec, int64_t P, double* nll, double* delta, uint32_t flags, void* stream,
                           bool orbit) {
    ARGCHK(t_mjd != nullptr && x != nullptr && pvec != nullptr && nll != nullptr, "null argument");
    PFCall c;
    if (const int rc = pf_prologue(n, par, map, tpl, norm, phoff, P, orbit, &c)) return rc;
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    const size_t D = (size_t)(c.map.ndim + c.map.phoff);
    {
        Scratch sc(s);
        const double *dt = nullptr, *dx = nullptr, *dp = nullptr;
        double *dnll = nullptr, *ddel = nullptr;
        PFDev d;
        HIPCHK(stage_in(sc, t_mjd, (size_t)n, dev, &dt));
        HIPCHK(stage_in(sc, x, (size_t)n, dev, &dx));
        HIPCHK(stage_in(sc, pvec, (size_t)P * D, dev, &dp));
        HIPCHK(stage_out(sc, nll, (size_t)P, dev, &dnll));
        HIPCHK(stage_out(sc, delta, (size_t)P * (size_t)n, dev, &ddel));
        if (const int rc = pf_upload(sc, s, c, n, &d)) return rc;
        KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
        kt.start();
        pf_launch_prologue(s, c, d, dt, n);
        pf_launch_nll(s, c, d, dt, dx, n, norm, dp, nullptr, P, ddel);
        HIPCHK(hipGetLastError());
        k_photon_reduce<<<(unsigned)cdiv(P, 4), 256, 0, s>>>(d.psum, d.pmin, c.L.tiles, n, norm, P, dnll);
        HIPCHK(hipGetLastError());
        kt.stop();
        HIPCHK(copy_back(s, nll, dnll, (size_t)P, dev));
        HIPCHK(copy_back(s, delta, ddel, (size_t)P * (size_t)n, dev));
    }
    return finish(s, flags);
}

extern "C" int crimp_photon_nll(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                                const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                                const double* pvec, int64_t P, double* nll, double* delta, uint32_t flags,
                                void* stream) {
    return photon_nll_call(t_mjd, x, n, par, map, tpl, norm, phoff, pvec, P, nll, delta, flags, stream, false);
}

extern "C" int crimp_photon_orbit_nll(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                                      const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                                      const double* pvec, int64_t P, double* nll, double* delta, uint32_t flags,
                                      void* stream) {
    return photon_nll_call(t_mjd, x, n, par, map, tpl, norm, phoff, pvec, P, nll, delta, flags, stream, true);
}

// crimp_photon_mcmc and (orbit) crimp_photon_orbit_mcmc
static int photon_mcmc_call(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                            const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                            const double* p0, const double* lo, const double* hi, int32_t W, int64_t steps,
                            uint64_t seed, double* chain, double* logprob, int64_t* accepted, uint32_t flags,
                            void* stream, bool orbit) {
    ARGCHK(t_mjd != nullptr && x != nullptr && p0 != nullptr && lo != nullptr && hi != nullptr && chain != nullptr &&
               logprob != nullptr && accepted != nullptr, "null argument");
    PFCall c;
    if (const int rc = pf_prologue(n, par, map, tpl, norm, phoff, W >= 1 ? W : 1, orbit, &c)) return rc;
    const int32_t D = c.map.ndim + c.map.phoff;
    ARGCHK(W >= 2 && W % 2 == 0 && W <= 256 && W >= 2 * D, "walkers: even, >= 2 ndim and <= 256");
    ARGCHK(steps >= 1 && steps <= (int64_t(1) << 31), "steps out of range");
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    const size_t w = (size_t)W, nd = (size_t)D, rows = (size_t)steps * w;
    {
        Scratch sc(s);
        const double *dt = nullptr, *dx = nullptr;
        PFDev d;
        PFMc A{};
        HIPCHK(stage_in(sc, t_mjd, (size_t)n, dev, &dt));
        HIPCHK(stage_in(sc, x, (size_t)n, dev, &dx));
        HIPCHK(stage_in(sc, p0, w * nd, dev, &A.p0));
        HIPCHK(stage_in(sc, lo, nd, dev, &A.lo));
        HIPCHK(stage_in(sc, hi, nd, dev, &A.hi));
        HIPCHK(stage_out(sc, chain, rows * nd, dev, &A.chain));
        HIPCHK(stage_out(sc, logprob, rows, dev, &A.logprob));
        HIPCHK(stage_out(sc, accepted, w, dev, &A.accepted));
        if (const int rc = pf_upload(sc, s, c, n, &d)) return rc;
        HIPCHK(sc.alloc(&A.pos, w * nd));
        HIPCHK(sc.alloc(&A.lp, w));
        HIPCHK(sc.alloc(&A.nacc, w));
        HIPCHK(sc.alloc(&A.prop, w * nd));
        HIPCHK(sc.alloc(&A.pz, w));
        HIPCHK(sc.alloc(&A.act, w));
        A.psum = d.psum;
        A.pmin = d.pmin;
        A.tiles = c.L.tiles;
        A.n = n;
        A.norm = norm;
        A.W = W;
        A.D = D;
        A.seed = seed;
        const int64_t half = W / 2;
        KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
        kt.start();
        // the whole chain is queued here; the host waits once, in finish()
        pf_launch_prologue(s, c, d, dt, n);
        k_photon_step<<<1, kPfStepWaves * 64, 0, s>>>(A, 0, 0, 0, 0);
        pf_launch_nll(s, c, d, dt, dx, n, norm, A.pos, A.act, W, nullptr);
        k_photon_step<<<1, kPfStepWaves * 64, 0, s>>>(A, 1, 0, 0, 0);
        HIPCHK(hipGetLastError());
        for (int64_t st = 0; st < steps; ++st)
            for (int h = 0; h < 2; ++h) {
                pf_launch_nll(s, c, d, dt, dx, n, norm, A.prop, A.act, half, nullptr);
                k_photon_step<<<1, kPfStepWaves * 64, 0, s>>>(A, 2, st, h, st + 1 == steps && h == 1);
            }
        HIPCHK(hipGetLastError());
        kt.stop();
        HIPCHK(copy_back(s, chain, A.chain, rows * nd, dev));
        HIPCHK(copy_back(s, logprob, A.logprob, rows, dev));
        HIPCHK(copy_back(s, accepted, A.accepted, w, dev));
    }
    return finish(s, flags);
}

extern "C" int crimp_photon_mcmc(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                                 const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                                 const double* p0, const double* lo, const double* hi, int32_t W, int64_t steps,
                                 uint64_t seed, double* chain, double* logprob, int64_t* accepted, uint32_t flags,
                                 void* stream) {
    return photon_mcmc_call(t_mjd, x, n, par, map, tpl, norm, phoff, p0, lo, hi, W, steps, seed, chain, logprob,
                            accepted, flags, stream, false);
}

extern "C" int crimp_photon_orbit_mcmc(const double* t_mjd, const double* x, int64_t n, const crimp_timing_model* par,
                                       const crimp_fit_map* map, const crimp_template* tpl, double norm, int32_t phoff,
                                       const double* p0, const double* lo, const double* hi, int32_t W, int64_t steps,
                                       uint64_t seed, double* chain, double* logprob, int64_t* accepted,
                                       uint32_t flags, void* stream) {
    return photon_mcmc_call(t_mjd, x, n, par, map, tpl, norm, phoff, p0, lo, hi, W, steps, seed, chain, logprob,
                            accepted, flags, stream, true);
}


// ============================================================== 7. interval selection (measureToAs.py:168-182)
// The photons of a ToA interval are TIME[(TIME >= start) & (TIME <= end)] (measureToAs.py:173-174); on time-sorted
// photons (event files are) that is the range [lower_bound(start), upper_bound(end)) -- two binary searches per
// interval instead of a pass over all photons per interval. crimp_is_sorted decides which applies.
__global__ __launch_bounds__(256) void k_unsorted(const double* __restrict__ t, int64_t n, int* __restrict__ flag) {
    constexpr int U = 4;  // pairs per thread and sweep, loads issued together
    int b = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 + 1 < n; i0 += U * stride) {
        double a[U], c[U];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t i = i0 + q * stride;
            a[q] = t[i + 1 < n ? i : 0];
            c[q] = t[i + 1 < n ? i + 1 : 0];
        }
#pragma unroll
        for (int q = 0; q < U; ++q)
            if (i0 + q * stride + 1 < n) b |= !(a[q] <= c[q]);  // a NaN is out of order, as np.all(T[1:] >= T[:-1])
    }
    if (__any(b) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}

// lo[i] = first photon with t >= starts[i] (np.searchsorted side="left"), count[i] = photons up to the last with
// t <= ends[i] (side="right") less lo[i], at least 0; first_last[2i], [2i+1] = t of the interval's first and last
// photon (NaN when it holds none). A NaN bound selects nothing, as the reference's mask.
__global__ __launch_bounds__(256) void k_select_intervals(const double* __restrict__ t, int64_t n,
                                                          const double* __restrict__ starts,
                                                          const double* __restrict__ ends, int64_t nint,
                                                          int64_t* __restrict__ lo, int64_t* __restrict__ count,
                                                          double* __restrict__ first_last) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nint) return;
    const double s = starts[i], e = ends[i];
    int64_t a = 0, b = n;
    while (a < b) {  // lower bound of s
        const int64_t m = (a + b) >> 1;
        if (t[m] < s) a = m + 1; else b = m;
    }
    const int64_t l = a;
    b = n;
    while (a < b) {  // upper bound of e, from l
        const int64_t m = (a + b) >> 1;
        if (t[m] <= e) a = m + 1; else b = m;
    }
    const int64_t c = (s == s && e == e && a > l) ? a - l : 0;
    lo[i] = l;
    count[i] = c;
    if (first_last) {
        first_last[2 * i] = c > 0 ? t[l] : NAN;
        first_last[2 * i + 1] = c > 0 ? t[l + c - 1] : NAN;
    }
}

// out[offsets[i] + j] = t[lo[i] + j], j < offsets[i+1] - offsets[i]: the intervals' photons concatenated
__global__ __launch_bounds__(256) void k_gather_ranges(const double* __restrict__ t, const int64_t* __restrict__ lo,
                                                       const int64_t* __restrict__ offsets, double* __restrict__ out) {
    const int64_t i = blockIdx.x;
    const int64_t o = offsets[i], len = offsets[i + 1] - o;
    const double* src = t + lo[i];
    for (int64_t j = threadIdx.x; j < len; j += blockDim.x) out[o + j] = src[j];
}

extern "C" int crimp_is_sorted(const double* t, int64_t n, int32_t* unsorted, uint32_t flags, void* stream) {
    ARGCHK(n >= 0, "n < 0");
    ARGCHK(unsorted != nullptr && (t != nullptr || n == 0), "null argument");
    *unsorted = 0;
    if (n < 2) return CRIMP_OK;
    const Call call(flags, stream, Call::kKeepTimes);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    {
        Scratch sc(s);
        const double* dt = nullptr;
        int* dflag = nullptr;
        HIPCHK(stage_in(sc, t, (size_t)n, dev, &dt));
        HIPCHK(sc.alloc(&dflag, 1));
        HIPCHK(hipMemsetAsync(dflag, 0, sizeof(int), s));
        k_unsorted<<<(unsigned)std::min<int64_t>(cdiv(n, 256 * 4), 2048), 256, 0, s>>>(dt, n, dflag);
        HIPCHK(hipGetLastError());
        int h = 0;
        HIPCHK(d2h(s, &h, dflag, sizeof(int)));
        *unsorted = h ? 1 : 0;
    }
    return finish(s, flags);
}

extern "C" int crimp_select_intervals(const double* t, int64_t n, const double* starts, const double* ends,
                                      int64_t nint, int64_t* lo, int64_t* count, double* first_last, uint32_t flags,
                                      void* stream) {
    ARGCHK(n >= 0 && nint >= 0, "negative size");
    ARGCHK((t != nullptr || n == 0) && (nint == 0 || (starts && ends && lo && count)), "null argument");
    if (nint == 0) return CRIMP_OK;
    const Call call(flags, stream, Call::kKeepTimes);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    {
        Scratch sc(s);
        const double *dt = nullptr, *ds = nullptr, *de = nullptr;
        int64_t *dlo = nullptr, *dc = nullptr;
        double* dfl = nullptr;
        HIPCHK(stage_in(sc, t, (size_t)n, dev, &dt));
        HIPCHK(stage_in(sc, starts, (size_t)nint, dev, &ds));
        HIPCHK(stage_in(sc, ends, (size_t)nint, dev, &de));
        HIPCHK(stage_out(sc, lo, (size_t)nint, dev, &dlo));
        HIPCHK(stage_out(sc, count, (size_t)nint, dev, &dc));
        if (first_last) HIPCHK(stage_out(sc, first_last, (size_t)(2 * nint), dev, &dfl));
        k_select_intervals<<<(unsigned)cdiv(nint, 256), 256, 0, s>>>(dt, n, ds, de, nint, dlo, dc, dfl);
        HIPCHK(hipGetLastError());
        HIPCHK(copy_back(s, lo, dlo, (size_t)nint, dev));
        HIPCHK(copy_back(s, count, dc, (size_t)nint, dev));
        if (first_last) HIPCHK(copy_back(s, first_last, dfl, (size_t)(2 * nint), dev));
    }
    return finish(s, flags);
}

extern "C" int crimp_gather_ranges(const double* t, int64_t n, const int64_t* lo, const int64_t* offsets,
                                   int64_t nint, double* out, uint32_t flags, void* stream) {
    ARGCHK(n >= 0 && nint >= 0, "negative size");
    ARGCHK(nint <= 2147483647LL, "too many intervals");
    ARGCHK(nint == 0 || (t && lo && offsets && out), "null argument");
    if (nint == 0) return CRIMP_OK;
    const Call call(flags, stream, Call::kKeepTimes);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    // the ranges are checked on the host against the photon array before any copy is queued
    std::vector<int64_t> hlo((size_t)nint), hoff((size_t)nint + 1);
    if (dev) {
        HIPCHK(d2h(s, hlo.data(), lo, (size_t)nint * sizeof(int64_t)));
        HIPCHK(d2h(s, hoff.data(), offsets, ((size_t)nint + 1) * sizeof(int64_t)));
    } else {
        std::memcpy(hlo.data(), lo, (size_t)nint * sizeof(int64_t));
        std::memcpy(hoff.data(), offsets, ((size_t)nint + 1) * sizeof(int64_t));
    }
    ARGCHK(hoff[0] == 0, "offsets[0] must be 0");
    for (int64_t i = 0; i < nint; ++i) {
        const int64_t len = hoff[(size_t)i + 1] - hoff[(size_t)i];
        ARGCHK(len >= 0 && hlo[(size_t)i] >= 0 && hlo[(size_t)i] + len <= n, "a range lies outside the photon array");
    }
    const int64_t total = hoff[(size_t)nint];
    {
        Scratch sc(s);
        const double* dt = nullptr;
        const int64_t *dlo = nullptr, *doff = nullptr;
        double* dout = nullptr;
        HIPCHK(stage_in(sc, t, (size_t)n, dev, &dt));
        HIPCHK(stage_in(sc, lo, (size_t)nint, dev, &dlo));
        HIPCHK(stage_in(sc, offsets, (size_t)nint + 1, dev, &doff));
        HIPCHK(stage_out(sc, out, (size_t)total, dev, &dout));
        k_gather_ranges<<<(unsigned)nint, 256, 0, s>>>(dt, dlo, doff, dout);
        HIPCHK(hipGetLastError());
        HIPCHK(copy_back(s, out, dout, (size_t)total, dev));
    }
    return finish(s, flags);
}

// ============================================================== 8. event simulator (sim_events.h)
extern "C" int crimp_sim_events(const crimp_timing_model* model, const crimp_sim_shape* shape, double mjd_start,
                                double span_s, double cell_s, const double* gti, int64_t ngti, uint64_t seed,
                                int64_t first_cell, int64_t n_cells, double* t_out, uint8_t* bkg_out, int64_t cap,
                                int64_t* n_out, double out_offset_s, uint32_t flags, void* stream) {
    ARGCHK(model != nullptr && shape != nullptr && n_out != nullptr, "null argument");
    *n_out = 0;
    ARGCHK(model->n_glitch >= 0 && model->n_glitch <= CRIMP_MAX_GLITCH, "n_glitch out of range");
    ARGCHK(model->n_wave >= 0 && model->n_wave <= CRIMP_MAX_WAVE, "n_wave out of range");
    if (const int rc = check_binary(model)) return rc;
    ARGCHK(std::isfinite(mjd_start) && std::isfinite(out_offset_s), "mjd_start and out_offset_s must be finite");
    ARGCHK(std::isfinite(span_s) && span_s > 0.0, "span_s must be positive and finite");
    ARGCHK(std::isfinite(cell_s) && cell_s > 0.0, "cell_s must be positive and finite");
    ARGCHK(std::isfinite(shape->lam_max) && shape->lam_max > 0.0, "lam_max must be positive and finite");
    ARGCHK(shape->lam_max * cell_s <= 65536.0, "lam_max * cell_s > 65536: shorten the cells");
    ARGCHK(std::isfinite(shape->bkg) && shape->bkg >= 0.0, "the background rate must be finite and >= 0");
    ARGCHK(shape->kind == CRIMP_SIM_TEMPLATE || shape->kind == CRIMP_SIM_STEPS, "unknown shape kind");
    ARGCHK(ngti >= 0 && (ngti == 0 || gti != nullptr), "ngti < 0 or a null GTI table");
    ARGCHK(cap >= 0 || t_out == nullptr, "cap < 0");
    SimArgs A{};
    A.kind = shape->kind;
    if (shape->kind == CRIMP_SIM_TEMPLATE) {
        const int rc = make_tpl(&shape->tpl, &A.T);
        if (rc != CRIMP_OK) return rc;
        ARGCHK(std::isfinite(shape->norm) && std::isfinite(shape->ph_shift), "norm and ph_shift must be finite");
    } else {
        ARGCHK(shape->n_steps >= 1 && shape->steps != nullptr, "a step shape needs n_steps >= 1 rates");
        A.n_steps = shape->n_steps;
    }
    // cells: the smallest count whose cells cover [0, span_s), every cell starting inside the span
    const double ncd = std::ceil(span_s / cell_s);
    ARGCHK(ncd < 2147483648.0, "more than 2^31 - 1 cells: lengthen the cells");
    int64_t nc = std::max<int64_t>((int64_t)ncd, 1);
    while (nc > 1 && (double)(nc - 1) * cell_s >= span_s) --nc;
    while ((double)nc * cell_s < span_s) ++nc;
    ARGCHK(nc <= 2147483647LL, "more than 2^31 - 1 cells: lengthen the cells");
    ARGCHK(first_cell >= 0 && first_cell <= nc, "first_cell outside the span's cells");
    if (n_cells < 0) n_cells = nc - first_cell;
    ARGCHK(first_cell + n_cells <= nc, "the cell range ends outside the span's cells");
    A.norm = shape->norm;
    A.ph_shift = shape->ph_shift;
    A.bkg = shape->bkg;
    A.lam_max = shape->lam_max;
    A.inv_lam = 1.0 / shape->lam_max;
    A.mjd_start = mjd_start;
    A.span_s = span_s;
    A.cell_s = cell_s;
    A.out_offset_s = out_offset_s;
    A.first_cell = first_cell;
    A.ngti = ngti;
    A.seed = seed;
    A.days = (flags & CRIMP_FLAG_TIME_DAYS) ? 1 : 0;
    const Call call(flags, stream);
    const bool dev = call.dev;
    hipStream_t s = call.s;
    if (ngti > 0) {  // the table is checked on the host before anything is queued
        std::vector<double> hg((size_t)ngti * 2);
        if (dev)
            HIPCHK(d2h(s, hg.data(), gti, hg.size() * sizeof(double)));
        else
            std::memcpy(hg.data(), gti, hg.size() * sizeof(double));
        for (int64_t i = 0; i < ngti; ++i) {
            ARGCHK(hg[2 * i] <= hg[2 * i + 1], "a GTI ends before it starts (or holds a NaN)");
            ARGCHK(i == 0 || hg[2 * i - 1] <= hg[2 * i], "the GTIs must be sorted and disjoint");
        }
    }
    if (n_cells == 0) return CRIMP_OK;  // an empty cell range: no events, every argument checked all the same
    // with an orbit the rate follows the shape at the phase of the emission time (parts 7 | 8); the Jacobian
    // 1 - dtau/dt of the rate, below 2 pi x / pb, is ignored
    const bool bin = wants_binary(model, 7 | CRIMP_PART_EMISSION);
    CPArgs<false> hm{};
    make_cpmodel(model, 7, &hm.m);
    CPArgs<true> hb{};
    if (bin) {
        hb.m = hm.m;
        make_binmodel(model, &hb.b);
    }
    {
        Scratch sc(s);
        const double *dgti = nullptr, *dsteps = nullptr;
        HIPCHK(stage_in(sc, gti, (size_t)ngti * 2, dev, &dgti));
        if (A.kind == CRIMP_SIM_STEPS) HIPCHK(stage_in(sc, shape->steps, (size_t)A.n_steps, dev, &dsteps));
        const int64_t n1 = n_cells + 1;  // the counts and one trailing zero: the scan leaves the total there
        const int64_t tiles = cdiv(n1, kSimScanTile);
        int64_t *dcnt = nullptr, *dsums = nullptr;
        HIPCHK(sc.alloc(&dcnt, (size_t)n1));
        HIPCHK(sc.alloc(&dsums, (size_t)tiles));
        KernelTimer kt(s, flags & CRIMP_FLAG_TIME_KERNELS);
        kt.start();
        HIPCHK(hipMemsetAsync(dcnt + n_cells, 0, sizeof(int64_t), s));
        if (bin)
            k_sim_cells<false, true><<<(unsigned)n_cells, 64, 0, s>>>(hb, A, dsteps, dgti, dcnt, nullptr, nullptr,
                                                                      nullptr);
        else
            k_sim_cells<false, false><<<(unsigned)n_cells, 64, 0, s>>>(hm, A, dsteps, dgti, dcnt, nullptr, nullptr,
                                                                       nullptr);
        HIPCHK(hipGetLastError());
        k_sim_tile_sums<<<(unsigned)tiles, kSimScanBlock, 0, s>>>(dcnt, n1, dsums);
        k_sim_scan_top<<<1, kSimScanBlock, 0, s>>>(dsums, tiles);
        k_sim_scan_apply<<<(unsigned)tiles, kSimScanBlock, 0, s>>>(dcnt, n1, dsums);
        HIPCHK(hipGetLastError());
        int64_t total = 0;
        HIPCHK(d2h(s, &total, dcnt + n_cells, sizeof(int64_t)));
        *n_out = total;
        if (t_out == nullptr) {
            kt.stop();
            return finish(s, flags);
        }
        if (cap < total) kt.stop();  // the count pass and the scan ran: their time is reported as on the count-only path
        ARGCHK(cap >= total, "cap is smaller than the number of events (nothing written)");
        double* dt = nullptr;
        uint8_t* db = nullptr;
        HIPCHK(stage_out(sc, t_out, (size_t)total, dev, &dt));
        HIPCHK(stage_out(sc, bkg_out, (size_t)total, dev, &db));
        if (total > 0) {
            if (bin)
                k_sim_cells<true, true><<<(unsigned)n_cells, 64, 0, s>>>(hb, A, dsteps, dgti, nullptr, dcnt, dt, db);
            else
                k_sim_cells<true, false><<<(unsigned)n_cells, 64, 0, s>>>(hm, A, dsteps, dgti, nullptr, dcnt, dt, db);
            HIPCHK(hipGetLastError());
        }
        kt.stop();
        HIPCHK(copy_back(s, t_out, dt, (size_t)total, dev));
        HIPCHK(copy_back(s, bkg_out, db, (size_t)total, dev));
    }
    return finish(s, flags);
}
