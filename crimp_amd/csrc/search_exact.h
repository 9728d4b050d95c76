// search_exact.h -- the default periodicity-search kernel: factorised harmonic sums on the i8 matrix cores
// with EXACT integer accumulation (MI355X / gfx950).
//
// Trial grid: an arithmetic progression f_j = f_0 + j*delta (fd-outer rows for the 2-D grid). A tile of
// 2048 trials j = c0 + 64a + b (a in 0..31, b in 0..63) factorises (periodsearch.py:67, :93-98, :120):
//     exp(2 pi i k (f_j dt + c2 dt^2)) = U_a * V_b,   U_a = exp(2 pi i k (f_{c0+64a} dt + c2 dt^2)),
//                                                   V_b = exp(2 pi i k (b delta) dt),
// so C_k + i S_k of the tile is the complex matrix product sum_photons U_a V_b.
//
// Numerics (why this is the default): the phase is fp64 (as the reference's argument), reduced to table
// units t = phase * kExTab turns; cos/sin come from a 4096-entry LDS table of fp64 values plus a short
// fp32 rotation by the residual angle (|theta| <= pi/4096), and are emitted directly as 2^30 fixed-point
// integers (error <= ~1.3 units = 1.2e-9). Each integer is split into four balanced base-256 digits
// (d3 2^24 + d2 2^16 + d1 2^8 + d0, d_i in [-128, 127], |d3| <= 64) packed in one dword by two
// integer ops: digits(y) = (y + 0x808080) ^ 0x808080. A product U.V = sum_{i,j} d_i e_j 2^{8(i+j)} is
// accumulated per digit LEVEL L = i+j in int32 (exact), levels 3..6 kept (the dropped levels 0..2 contribute
// < 5e-14 per photon): the A operand holds U's digits in natural order, the B operand V's digits byte-reversed,
// so one dword pair dots to level 3 and A >> 8 to level 4 (dense v_mfma_i32_32x32x32_i8); levels 5 and 6 have
// A bytes (d2, d3, 0, 0) and (d3, 0, 0, 0) and run on the 2:4-sparse v_smfmac_i32_32x32x64_i8, two quads per
// instruction. The level sums are carried exactly between levels every 16384 photons and folded into int64
// (acc3 + acc4 << 8 + acc5 << 16 + acc6 << 24, units of 2^-36) every 131072; each block adds its int64 totals to
// the global per-trial totals with 64-bit integer atomics: integer sums are exact and order-independent, so the
// result does not depend on photon splits, trial blocking or sharding, and the only errors are the 2^30
// roundings of U and V (per-term ~1e-9, against ~1e-7 for fp32 sin/cos).
//
// Layout: one 256-thread block per CU (4 waves, one per SIMD, one 32 x 64 tile each) per group of 4 consecutive
// tiles and photon split; the 256 int32 accumulators of a wave live in AGPRs (ex_mfma). Per chunk of 32 photons
// the block stages dt in LDS, all 256 threads compute the tile-independent V digits for the 4 tiles (32 photons x
// 64 b, stored per photon pair and column as B fragments {rev Vr, rev -Vi} / {rev Vi, rev Vr}), and every wave
// computes its own U digits in registers: lane (a, h) holds photons 4q+2h, 4q+2h+1 of quad q ({Ur, Ui} of each:
// 16 bytes = the K slice of one i8 MFMA). A software pipeline over quad pairs (below) interleaves all of it with
// the 24 matrix instructions of each pair.
#include <type_traits>

#include "search_plan.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// the tile's shape and the carry / fold periods (kExChunk .. kExFoldVals) are in search_plan.h: the host plan needs them
constexpr int kExTab = 4096;    // sin/cos table entries per turn
constexpr int kExQuads = kExChunk / 4;
constexpr int kExItems = kExChunk * kExCols / kExBlock;  // V items per thread and chunk (= kExQuads)
static_assert(kExItems == kExQuads, "one V item per pipeline group");
constexpr int kExDtSlots = 4;   // photon-time ring: chunks c-1 (being retired) .. c+2
constexpr double kExUnit = 1.4551915228366852e-11;  // 2^-36: value of one unit of the int64 totals

struct ExEntry {
    int32_t sk, ck;  // rint(sin, cos(2 pi k / T) * 2^30) + 0x808080 - 0x4B400000: the fp32 rounding bias of ex_end and
                     // the digit bias of ex_digits folded in
    float s1, c1;    // sin, cos(2 pi k / T) * 2^30 * (2 pi / T): the residual rotation's first-order coefficients
};

// t in table units (turns * kExTab) -> the digit dwords of (cos, sin) * 2^30 (ex_digits of the rounded integers),
// in two halves so that the table read of one photon can be issued ahead of the arithmetic of another.
// x = 2 pi (k + y) / T, |y| <= 1/2: sin x = s_k + c_k sin(th) + s_k (cos(th) - 1) with th = 2 pi y / T, and to
// 2^30 units  sin x * 2^30 = S_k + y (C1 - u S1),  cos x * 2^30 = C_k - y (S1 + u C1),  u = (pi / T) y,
// (C1, S1 = (c_k, s_k) 2^30 2 pi / T); the dropped th^3/6 term is <= 0.08 units at the cell edge.
struct ExArg {
    uint32_t idx;  // table index
    float y;       // residual in table steps, |y| <= 1/2
};
// Floating-point contraction is spelled out here (contract off, explicit fma) so that the digits -- and the exact
// integer sums -- are a function of the source alone: with hipcc's default contraction the choice between
// fma(a, b, -kf) and rint(a b) - kf depended on the schedule, and a build without the ex_ready fences returned
// different (equally accurate) sums (profiles/r04/ab_fences.log).
__device__ __forceinline__ ExArg ex_begin(double t) {
#pragma clang fp contract(off)
    const double M = 6755399441055744.0;  // 1.5 * 2^52: low mantissa bits of t + M = rint(t) (|t| < 2^51)
    const double tm = t + M;
    const double kf = tm - M;
    return ExArg{(uint32_t)__double2loint(tm) & (kExTab - 1), (float)(t - kf)};  // t - kf is exact
}
// the same for the phase t = a * b taken from the exact product: index from fma(a, b, M), residual fma(a, b, -kf)
__device__ __forceinline__ ExArg ex_begin_prod(double a, double b) {
#pragma clang fp contract(off)
    const double M = 6755399441055744.0;
    const double tm = __builtin_fma(a, b, M);
    const double kf = tm - M;
    return ExArg{(uint32_t)__double2loint(tm) & (kExTab - 1), (float)__builtin_fma(a, b, -kf)};
}
// -> digit dwords of cos (dc) and sin (ds), in two halves (ex_end_a: the rotation terms, ex_end_b: the digits)
struct ExRot { float ts, tc; };
__device__ __forceinline__ ExRot ex_end_a(const ExEntry& e, float y) {
    const float u = y * (3.14159265358979323846f / (float)kExTab);
    return ExRot{__builtin_fmaf(-u, e.s1, e.c1), __builtin_fmaf(u, e.c1, e.s1)};
}
// |value| < 2^22: the low mantissa bits of fma(y, t, 1.5 * 2^23) are rint(y t) + 0x400000
__device__ __forceinline__ uint32_t ex_end_s(const ExEntry& e, float y, float ts) {
    return ((uint32_t)e.sk + __float_as_uint(__builtin_fmaf(y, ts, 12582912.0f))) ^ 0x00808080u;
}
__device__ __forceinline__ uint32_t ex_end_c(const ExEntry& e, float y, float tc) {
    return ((uint32_t)e.ck + __float_as_uint(__builtin_fmaf(-y, tc, 12582912.0f))) ^ 0x00808080u;
}
__device__ __forceinline__ void ex_end_b(const ExEntry& e, float y, ExRot r, uint32_t& dc, uint32_t& ds) {
    ds = ex_end_s(e, y, r.ts);
    dc = ex_end_c(e, y, r.tc);
}
__device__ __forceinline__ void ex_end(const ExEntry& e, float y, uint32_t& dc, uint32_t& ds) {
    ex_end_b(e, y, ex_end_a(e, y), dc, ds);
}
__device__ __forceinline__ void ex_sincos_digits(const ExEntry* __restrict__ tab, double t, uint32_t& dc,
                                                 uint32_t& ds) {
    const ExArg g = ex_begin(t);
    ex_end(tab[g.idx], g.y, dc, ds);
}
__device__ __forceinline__ ExEntry ex_entry(int i) {
    double s, c;
    sincospi((double)i * (2.0 / kExTab), &s, &c);
    const double w = 1073741824.0 * (6.283185307179586476925 / kExTab);
    ExEntry e;
    e.s1 = (float)(s * w);
    e.c1 = (float)(c * w);
    e.sk = (int32_t)((uint32_t)(int32_t)rint(s * 1073741824.0) + 0x00808080u - 0x4B400000u);
    e.ck = (int32_t)((uint32_t)(int32_t)rint(c * 1073741824.0) + 0x00808080u - 0x4B400000u);
    return e;
}

// digit dword of -y from the digit dword of y: -y's balanced digits are the negated digits (with carries),
// recomputed from the integer: y = (d ^ 0x808080) - 0x808080
// ((0x808080 - y) ^ 0x808080 with y = (d ^ 0x808080) - 0x808080) = ((~(d ^ 0x808080) + 0x1010101) ^ 0x808080): an
// xor-add and an xor (v_xad_u32, v_xor_b32)
__device__ __forceinline__ uint32_t ex_neg_digits(uint32_t d) {
    uint32_t x;  // hipcc does not form v_xad_u32 with two literal constants (one may be an SGPR, the other a VGPR)
    asm("v_xad_u32 %0, %1, %2, %3" : "=v"(x) : "v"(d), "s"(0xFF7F7F7Fu), "v"(0x01010101u));
    return x ^ 0x00808080u;
}


// Issue-order control for the pipelined photon loop. The MFMAs are volatile inline asm, so they keep their
// program order with respect to each other, to LDS accesses and to the empty asm fences below; hipcc only moves
// VALU work between them:
//   ex_ready(x): x is computed before this point (pins a piece of work before the next MFMA);
//   ex_open(x):  x is redefined here (work that depends on x starts after this point);
//   ex_keep(x):  x's registers stay allocated until here. A quad's operands are kept until two MFMAs of the
//                next group have issued, so no register an MFMA reads is rewritten within 64 cycles of its issue
//                (the matrix pipe issues one 32x32x32 i8 MFMA per 32 cycles; mfma_drain.h for why it matters).
// Operands are ready one whole group ahead, results are read only after mfma_drain(); hipcc inserts the LDS
// waits (s_waitcnt) for the asm operands.
// The wave's 16 int32 accumulator tiles live in AGPRs for the whole kernel, outside the compiler's register
// model: tile m (level m >> 2, fragment (m >> 1) & 1, Re/Im m & 1) is a[16m : 16m + 15]. Only these asm helpers
// touch AGPRs, so the accumulators never move. Every MFMA statement lists all 256 AGPRs as clobbers (and
// ex_acc_zero's clobber makes the code object reserve them): hipcc may then keep no value of its own in an AGPR
// across any MFMA, so under register pressure it spills to scratch -- visible, and rejected by the no-scratch test
// -- instead of allocating AGPRs. Without the clobbers (CRIMP_EX_AGPR_CLOBBERS=0) the build without the ex_open
// fences parks the 64-bit photon-time address of fetch_dt in a0:a1, tile 0's MFMAs overwrite it and the next
// global_load faults (profiles/r03/ab_search_no_open_fences_rejected_fault.log; tools/agpr_check.py flags it on the
// CPU). The cost is one s_nop 0 per chunk's MFMA sequence. tools/isa_hazards.py and tools/agpr_check.py check
// the built code.
#ifndef CRIMP_EX_AGPR_CLOBBERS
#define CRIMP_EX_AGPR_CLOBBERS 1
#endif
// every AGPR, as a clobber of each MFMA statement (below)
#define EX_ALL_AGPRS \
    "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", "a10", "a11", "a12", "a13", "a14", "a15", \
    "a16", "a17", "a18", "a19", "a20", "a21", "a22", "a23", "a24", "a25", "a26", "a27", "a28", "a29", "a30", "a31", \
    "a32", "a33", "a34", "a35", "a36", "a37", "a38", "a39", "a40", "a41", "a42", "a43", "a44", "a45", "a46", "a47", \
    "a48", "a49", "a50", "a51", "a52", "a53", "a54", "a55", "a56", "a57", "a58", "a59", "a60", "a61", "a62", "a63", \
    "a64", "a65", "a66", "a67", "a68", "a69", "a70", "a71", "a72", "a73", "a74", "a75", "a76", "a77", "a78", "a79", \
    "a80", "a81", "a82", "a83", "a84", "a85", "a86", "a87", "a88", "a89", "a90", "a91", "a92", "a93", "a94", "a95", \
    "a96", "a97", "a98", "a99", "a100", "a101", "a102", "a103", "a104", "a105", "a106", "a107", "a108", "a109", "a110", "a111", \
    "a112", "a113", "a114", "a115", "a116", "a117", "a118", "a119", "a120", "a121", "a122", "a123", "a124", "a125", "a126", "a127", \
    "a128", "a129", "a130", "a131", "a132", "a133", "a134", "a135", "a136", "a137", "a138", "a139", "a140", "a141", "a142", "a143", \
    "a144", "a145", "a146", "a147", "a148", "a149", "a150", "a151", "a152", "a153", "a154", "a155", "a156", "a157", "a158", "a159", \
    "a160", "a161", "a162", "a163", "a164", "a165", "a166", "a167", "a168", "a169", "a170", "a171", "a172", "a173", "a174", "a175", \
    "a176", "a177", "a178", "a179", "a180", "a181", "a182", "a183", "a184", "a185", "a186", "a187", "a188", "a189", "a190", "a191", \
    "a192", "a193", "a194", "a195", "a196", "a197", "a198", "a199", "a200", "a201", "a202", "a203", "a204", "a205", "a206", "a207", \
    "a208", "a209", "a210", "a211", "a212", "a213", "a214", "a215", "a216", "a217", "a218", "a219", "a220", "a221", "a222", "a223", \
    "a224", "a225", "a226", "a227", "a228", "a229", "a230", "a231", "a232", "a233", "a234", "a235", "a236", "a237", "a238", "a239", \
    "a240", "a241", "a242", "a243", "a244", "a245", "a246", "a247", "a248", "a249", "a250", "a251", "a252", "a253", "a254", "a255"
// CRIMP_EX_PRE_NOP=N (A/B only): every MFMA statement starts with s_nop N, N + 1 wait states after whatever
// hipcc issued before it
#ifdef CRIMP_EX_PRE_NOP
#define EX_STR2(x) #x
#define EX_STR(x) EX_STR2(x)
#define EX_PRE "s_nop " EX_STR(CRIMP_EX_PRE_NOP) "\n\t"
#else
#define EX_PRE ""
#endif
#if !CRIMP_EX_AGPR_CLOBBERS
#undef EX_ALL_AGPRS
#define EX_ALL_AGPRS
#endif
template <int M>
__device__ __forceinline__ void ex_mfma(const i32x4& a, const i32x4& b) {
    asm volatile(EX_PRE "v_mfma_i32_32x32x32_i8 a[%c2:%c3], %0, %1, a[%c2:%c3]" ::"v"(a), "v"(b), "i"(16 * M),
                 "i"(16 * M + 15) : EX_ALL_AGPRS);
}
template <int M>
__device__ __forceinline__ void ex_smfma(const i32x4& a, const i32x8& b, int idx) {
    asm volatile(EX_PRE "v_smfmac_i32_32x32x64_i8 a[%c3:%c4], %0, %1, %2" ::"v"(a), "v"(b), "v"(idx), "i"(16 * M),
                 "i"(16 * M + 15) : EX_ALL_AGPRS);
}
template <int R>
__device__ __forceinline__ int ex_acc_read(std::integral_constant<int, R>) {
    int x;
    asm volatile("v_accvgpr_read_b32 %0, a%c1" : "=v"(x) : "i"(R));
    return x;
}
template <int R>
__device__ __forceinline__ void ex_acc_write(std::integral_constant<int, R>, int x) {
    asm volatile("v_accvgpr_write_b32 a%c0, %1" ::"i"(R), "v"(x));
}
template <int N, typename F>
__device__ __forceinline__ void ex_static_for(F&& f) {
    if constexpr (N > 0) {
        ex_static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}
template <int M, int R>
using ex_areg = std::integral_constant<int, 16 * M + R>;
__device__ __forceinline__ void ex_acc_zero() {
    asm volatile("v_accvgpr_write_b32 a255, 0" ::: "a255");
    ex_static_for<255>([&](auto r) { asm volatile("v_accvgpr_write_b32 a%c0, 0" ::"i"(decltype(r)::value)); });
}
// A/B switches of the fence analysis: CRIMP_EX_OPEN=0 / CRIMP_EX_READY=0 build the kernel without
// the ex_open / ex_ready fences. Without ex_ready, hipcc computes an MFMA's operands right before it (2 wait
// states after the writing VALU, where the fenced build leaves >= 16): tools/isa_hazards.py rejects that build.
#ifndef CRIMP_EX_OPEN
#define CRIMP_EX_OPEN 1
#endif
// CRIMP_EX_EARLY_OPEN=1: every ex_open that pins a piece to its MFMA gap is issued before the MFMA that opens the gap
// instead of after it, and the ones whose input was computed in the same gap are dropped: hipcc pads one wait state
// (s_nop 0) between an asm statement's outputs and the next VALU reading them, and with the MFMA between the two
// there is no such VALU
#ifndef CRIMP_EX_EARLY_OPEN
#define CRIMP_EX_EARLY_OPEN 0
#endif
#ifndef CRIMP_EX_READY
#define CRIMP_EX_READY 1
#endif
__device__ __forceinline__ void ex_keep(const i32x4& x) { asm volatile("" ::"v"(x)); }
__device__ __forceinline__ void ex_keep(const i32x8& x) { asm volatile("" ::"v"(x)); }
#if CRIMP_EX_READY
__device__ __forceinline__ void ex_ready(const i32x4& x) { asm volatile("" ::"v"(x)); }
__device__ __forceinline__ void ex_ready(uint32_t x, float y) { asm volatile("" ::"v"(x), "v"(y)); }
__device__ __forceinline__ void ex_ready(uint32_t x, uint32_t y) { asm volatile("" ::"v"(x), "v"(y)); }
__device__ __forceinline__ void ex_ready(float x, float y) { asm volatile("" ::"v"(x), "v"(y)); }
__device__ __forceinline__ void ex_ready(uint32_t x) { asm volatile("" ::"v"(x)); }
#else
__device__ __forceinline__ void ex_ready(const i32x4&) {}
__device__ __forceinline__ void ex_ready(uint32_t, float) {}
__device__ __forceinline__ void ex_ready(uint32_t, uint32_t) {}
__device__ __forceinline__ void ex_ready(float, float) {}
__device__ __forceinline__ void ex_ready(uint32_t) {}
#endif
#if CRIMP_EX_OPEN == 2  // A/B: a scheduling barrier instead of the opaque redefinition (no VGPR output, no pad)
__device__ __forceinline__ void ex_open(double&) { __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ void ex_open(i32x4&) { __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ void ex_open(float&) { __builtin_amdgcn_sched_barrier(0); }
__device__ __forceinline__ void ex_open(uint32_t&, uint32_t&) { __builtin_amdgcn_sched_barrier(0); }
#elif CRIMP_EX_OPEN
__device__ __forceinline__ void ex_open(double& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void ex_open(i32x4& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void ex_open(float& x) { asm volatile("" : "+v"(x)); }
__device__ __forceinline__ void ex_open(uint32_t& x, uint32_t& y) { asm volatile("" : "+v"(x), "+v"(y)); }
#else
__device__ __forceinline__ void ex_open(double&) {}
__device__ __forceinline__ void ex_open(i32x4&) {}
__device__ __forceinline__ void ex_open(float&) {}
__device__ __forceinline__ void ex_open(uint32_t&, uint32_t&) {}
#endif

// level-4 operand: every digit dword shifted right by one byte (logical: the top byte becomes 0)
typedef unsigned ex_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ i32x4 ex_shr8(i32x4 a) { return (i32x4)((ex_u32x4)a >> 8u); }

__device__ __forceinline__ int64_t ex_level_sum(int a3, int a4, int a5, int a6) {
    return (int64_t)a3 + ((int64_t)a4 << 8) + ((int64_t)a5 << 16) + ((int64_t)a6 << 24);
}

template <bool TWOD>
__global__ __launch_bounds__(kExBlock, 1) void k_search_exact(
    const double* __restrict__ dt, const double* __restrict__ dt2, int64_t n, int64_t chunk,
    const double* __restrict__ freq, int64_t nf, const double* __restrict__ c2row, const double* __restrict__ apinfo,
    int64_t tile_first, int64_t ntiles, int64_t tiles_per_row, int64_t first, int64_t count, int kh,
    unsigned long long* __restrict__ tot, long long* __restrict__ fold) {
    __shared__ ExEntry tab[kExTab + 1];                      // 64 KB; entry kExTab: cos = sin = 0 (dead photons)
    // B fragments per photon pair and column b: two chunk buffers of kExChunk / 2 pairs, a ring of kExChunk pairs
    __shared__ uint4 vre[kExChunk][kExCols];                 // {rev Vr, rev -Vi} of the pair's two photons
    __shared__ uint4 vim[kExChunk][kExCols];                 // {rev Vi, rev Vr}
    __shared__ double sdt[kExDtSlots * kExChunk];            // photon times: a ring of four chunks
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < kExTab; i += kExBlock) tab[i] = ex_entry(i);
    if (tid == 0) {  // digits of exactly 0 whatever the residual: the biased zero integers, no rotation terms
        const int32_t z = (int32_t)(0x00808080u - 0x4B400000u);
        tab[kExTab] = ExEntry{z, z, 0.0f, 0.0f};
    }
    const double kT = (double)kh * (double)kExTab;
    const int64_t T = (int64_t)blockIdx.x * kExWaves + wv;  // this wave's tile; waves past the end only produce V
    const bool active = T < ntiles;                          // wave-uniform
    const int64_t gt = tile_first + (active ? T : 0);
    const int64_t frow = gt / tiles_per_row;
    const int64_t c0 = (gt - frow * tiles_per_row) * kExTileTrials;
    const int ar = lane & 31, h = lane >> 5;
    const int64_t ca = c0 + kExCols * ar;                    // U row a: trial c0 + 64 a
    const double fa = freq[ca < nf ? ca : nf - 1] * kT;
    const double c2 = TWOD ? c2row[frow] * kT : 0.0;
    const int pb = tid & (kExCols - 1);                      // producer: V_b for b = pb, photons (tid >> 6) + 4 s
    const int pp = tid / kExCols;
    const int ppu = __builtin_amdgcn_readfirstlane(pp);      // = pp: the wave's index, made visibly uniform
    const double gbv = (double)pb * apinfo[0] * kT;
    const int64_t split = blockIdx.y;
    const int64_t i0 = split * chunk;
    const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    const int nch = (int)((i1 - i0 + kExChunk - 1) / kExChunk);

    // photon times: thread tid < kExChunk loads photon tid of chunk c into a register one chunk before storing it
    // into the ring, three chunks ahead of its use, so that no wave waits on global memory in the photon loop
    auto fetch_dt = [&](int c, double& v) {
        const int64_t i = i0 + (int64_t)c * kExChunk + tid;
        const bool ok = tid < kExChunk && c < nch && i < i1;
        v = ok ? dt[i] : 0.0;
    };
    auto store_dt = [&](int c, double v) {
        if (tid < kExChunk) sdt[(c % kExDtSlots) * kExChunk + tid] = v;
    };
    auto nlive_of = [&](int c) -> int {
        const int64_t rest = i1 - (i0 + (int64_t)c * kExChunk);
        return rest < 0 ? 0 : (rest > kExChunk ? kExChunk : (int)rest);
    };
    // V items: item (chunk cj, index s) is photon pp + 4 s of chunk cj (so quad s) at column pb, stored as B
    // fragment halves; photons past the split get V = 0, so that their products vanish
    uint2* const wre = reinterpret_cast<uint2*>(&vre[pp >> 1][pb]) + (pp & 1);
    uint2* const wim = reinterpret_cast<uint2*>(&vim[pp >> 1][pb]) + (pp & 1);
    constexpr int kPairU2 = kExCols * 2;               // uint2 per photon pair row
    struct VItem { double d; ExArg g; ExEntry e; ExRot r; uint32_t dc, dsn, rc, rs, rn; };
    // item (chunk cj, index s): all indices wave-uniform (scalar arithmetic), s a compile-time constant
    auto v_read = [&](int cj, int s, VItem& it) { it.d = sdt[(cj & (kExDtSlots - 1)) * kExChunk + pp + 4 * s]; };
    // a photon past the split (pp + 4 s >= nlive: wave-uniform) reads the zero entry, so its V digits are 0
    auto v_begin = [&](VItem& it, int s, int nlive) {
        it.g = ex_begin_prod(gbv, it.d);
        it.g.idx = ppu + 4 * s < nlive ? it.g.idx : (uint32_t)kExTab;
    };
    auto v_table = [&](VItem& it) { it.e = tab[it.g.idx]; };
    auto v_post = [&](VItem& it) {  // B fragment dwords: byte-reversed digits of Vr, Vi, -Vi
        it.rc = __builtin_bswap32(it.dc);
        it.rs = __builtin_bswap32(it.dsn);
        it.rn = __builtin_bswap32(ex_neg_digits(it.dsn));
    };
    auto v_write = [&](VItem& it, int cj, int s) {
        // photon pp + 4 s of buffer cj & 1 = pair (pp >> 1) + 2 s + (cj & 1) kExChunk / 2
        const int o = ((cj & 1) * (kExChunk / 2) + 2 * s) * kPairU2;
        wre[o] = make_uint2(it.rc, it.rn);
        wim[o] = make_uint2(it.rs, it.rc);
    };
    auto produce = [&](int cj, int s) {  // one whole item, outside the pipeline
        VItem it;
        v_read(cj, s, it);
        v_begin(it, s, nlive_of(cj));
        v_table(it);
        ex_end(it.e, it.g.y, it.dc, it.dsn);
        v_post(it);
        v_write(it, cj, s);
    };

    // int32 level sums of the wave's 32 x 64 tile: AGPR tiles [level][fragment][Re, Im] (ex_mfma)
    ex_acc_zero();
    // the block's running int64 sums between folds: per lane in global scratch (coalesced, written and read
    // by the same lane), so that they take no registers inside the photon loop
    long long* const fs =
        fold + (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kExWaves + wv) * (kExFoldVals * 64) + lane;
    const int comp = 2 * (kh - 1);

    // ---- software pipeline over quad PAIRS (8 photons). Pair group (c, p) issues the 24 MFMAs of quads 2p, 2p+1
    // of chunk c -- levels 3 and 4 dense, one v_mfma_i32_32x32x32_i8 per quad, tile fragment and Re/Im; levels 5
    // and 6 on the 2:4-sparse v_smfmac_i32_32x32x64_i8, one per fragment and Re/Im for both quads (their A bytes
    // are (d2, d3, 0, 0) and (d3, 0, 0, 0), so the sparse form loses nothing and does the two quads' K = 64 in
    // one instruction: 24 matrix instructions per pair instead of 32, tools/mb_power.hip for the energy) -- on
    // operands prepared during the previous pair group. In the gaps between them it finishes U of the next pair
    // (table entries read one group earlier), starts U of the pair after (phase, table reads), reads the next
    // pair's B fragments and the photon times of the pair three ahead, and computes two V items. Every piece is
    // pinned to its MFMA gap by ex_open / ex_ready, and no LDS read is consumed within 3 MFMAs of its issue. The
    // block's one barrier per chunk sits in pair group 3, before its read of the next chunk's first B fragments:
    // by then the V items and photon times every wave reads next are written (four MFMAs earlier, so the barrier's
    // LDS drain is free) and the buffers it overwrites next are read, so the pipeline runs across chunks.
    //
    // Sparse operand layout (tools/mb_smfmac_layout.hip, profiles/r02/smfmac_layout.txt): the instruction's
    // logical K = 64 is [B lane-half 0 bytes 0..15 | half 1 bytes 0..15 | half 0 bytes 16..31 | half 1 bytes
    // 16..31], and A lane-half h's 16 compressed bytes cover K 32h .. 32h+31. With B = {quad 2p's dense fragment,
    // quad 2p+1's} the K order is (quad 0 half 0, quad 0 half 1, quad 1 half 0, quad 1 half 1), so lane-half 0 needs
    // quad 0's level digits of both halves and lane-half 1 quad 1's: one v_permlane32_swap per compressed dword.
    struct ExOps {                 // one pair's MFMA operands
        i32x4 A3[2];               // dense level 3 per quad: U digits (level 4, the digits >> 8, is formed in the
                                   // group that uses it)
        i32x4 A5, A6;              // sparse levels 5, 6: compressed (d2, d3) / (d3, 0) per dword, lane-swapped
        i32x8 b[2][2];             // B [fragment][Re, Im] = {quad 2p, quad 2p+1}
    };
    struct ExPend { ExEntry e[4]; ExArg g[4]; };  // the next pair's table entries: photon 2 quad + i of the lane
    struct ExDt { double2 d[2]; };                // a pair's photon times, per quad
    // photon times of quad q of chunk c (q may run into the next chunks: the slots form a ring)
    auto read_dt = [&](int c, int q, double2& d) {
        const int i = ((c % kExDtSlots) * kExChunk + 4 * q) & (kExDtSlots * kExChunk - 1);
        d = *reinterpret_cast<const double2*>(&sdt[i + 2 * h]);
    };
    auto read_dt_pair = [&](int c, int p, ExDt& D) {
        read_dt(c, 2 * p, D.d[0]);
        read_dt(c, 2 * p + 1, D.d[1]);
    };
    // the phase in table units; the 2-D grid's dt^2 is formed here as d * d, bit-identical to the dt2 array
    auto begin1 = [&](double d) -> ExArg {
#pragma clang fp contract(off)
        return TWOD ? ex_begin(__builtin_fma(fa, d, c2 * (d * d))) : ex_begin_prod(fa, d);
    };
    // B fragments of pair p of chunk c (p = kExQuads / 2 is pair 0 of chunk c+1)
    auto read_b = [&](int c, int p, ExOps& o) {
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            uint4 r[2], m[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int pr = (((c & 1) * kExQuads + 2 * p + i) * 2 + h) & (kExChunk - 1);
                r[i] = vre[pr][32 * f + ar];
                m[i] = vim[pr][32 * f + ar];
            }
            o.b[f][0] = i32x8{(int)r[0].x, (int)r[0].y, (int)r[0].z, (int)r[0].w,
                              (int)r[1].x, (int)r[1].y, (int)r[1].z, (int)r[1].w};
            o.b[f][1] = i32x8{(int)m[0].x, (int)m[0].y, (int)m[0].z, (int)m[0].w,
                              (int)m[1].x, (int)m[1].y, (int)m[1].z, (int)m[1].w};
        }
    };
    // Pieces of the pipeline, each pinned to one MFMA gap (ex_open on its input at the start, ex_ready on its output
    // at the end). U photon i of a pair = photon i & 1 of the lane's two in quad i >> 1 -> digit dwords
    // a[quad][Ur, Ui of photon 0, then of photon 1].
    constexpr bool kEarly = CRIMP_EX_EARLY_OPEN;
    auto u_a = [&](ExPend& P, int i) -> ExRot {
        if constexpr (!kEarly) ex_open(P.g[i].y);
        const ExRot r = ex_end_a(P.e[i], P.g[i].y);
        ex_ready(r.ts, r.tc);
        return r;
    };
    auto u_s = [&](ExPend& P, int i, ExRot& r, uint32_t (&a)[2][4]) {
        if constexpr (!kEarly) ex_open(r.ts);
        a[i >> 1][2 * (i & 1) + 1] = ex_end_s(P.e[i], P.g[i].y, r.ts);
        ex_ready(a[i >> 1][2 * (i & 1) + 1]);
    };
    auto u_c = [&](ExPend& P, int i, ExRot& r, uint32_t (&a)[2][4]) {
        if constexpr (!kEarly) ex_open(r.tc);
        a[i >> 1][2 * (i & 1)] = ex_end_c(P.e[i], P.g[i].y, r.tc);
        ex_ready(a[i >> 1][2 * (i & 1)]);
    };
    auto item_begin = [&](VItem& it, int s, int nlive) {
        if constexpr (!kEarly) ex_open(it.d);
        v_begin(it, s, nlive);
        ex_ready(it.g.idx, it.g.y);
    };
    auto item_a = [&](VItem& it) {
        if constexpr (!kEarly) ex_open(it.g.y);
        it.r = ex_end_a(it.e, it.g.y);
        ex_ready(it.r.ts, it.r.tc);
    };
    auto item_s = [&](VItem& it) {
        if constexpr (!kEarly) ex_open(it.r.ts);
        it.dsn = ex_end_s(it.e, it.g.y, it.r.ts);
        ex_ready(it.dsn);
    };
    auto item_c = [&](VItem& it) {
        if constexpr (!kEarly) ex_open(it.r.tc);
        it.dc = ex_end_c(it.e, it.g.y, it.r.tc);
        ex_ready(it.dc);
    };
    auto item_post = [&](VItem& it) {
        if constexpr (!kEarly) ex_open(it.dc, it.dsn);
        v_post(it);
        ex_ready(it.rc, it.rs);
        ex_ready(it.rn);
    };
    auto u_begin = [&](double& d) -> ExArg {
        if constexpr (!kEarly) ex_open(d);
        const ExArg g = begin1(d);
        ex_ready(g.idx, g.y);
        return g;
    };
    const int kIdx = 0x44444444;  // sparse index: every group's two values at positions 0, 1
#define EX_LO(v) __builtin_shufflevector(v, v, 0, 1, 2, 3)
#define EX_HI(v) __builtin_shufflevector(v, v, 4, 5, 6, 7)
    // one pair group; X = this pair's operands, Y = the previous pair's (kept 2 MFMAs past their last reader,
    // then overwritten with the next pair's); P = table entries of pair +1 (in) / +2 (out); D = photon times of
    // pair +2 (in) / +3 (out); I0, I1 = V items (photon time read one group earlier; on exit the next group's).
    // Gap k = the gap after matrix instruction k; VALU per gap ~6 (the pieces above: begin 6, a 3, s 3, c 3).
    auto pgroup = [&](ExOps& X, ExOps& Y, ExPend& P, ExDt& D, VItem& I0, VItem& I1, int c, int p, int nl1,
                      int nl2, bool sync) {
        // this group's items: (c+1, 2p+2), (c+1, 2p+3) for p < 3, (c+2, 0), (c+2, 1) for p = 3; next group's
        const int icj = p + 1 < kExQuads / 2 ? c + 1 : c + 2, is = (2 * p + 2) % kExItems;
        const int ncj = p + 2 < kExQuads / 2 ? c + 1 : c + 2, ns = (2 * p + 4) % kExItems;
        const int inl = p + 1 < kExQuads / 2 ? nl1 : nl2;
        ExArg g[4];
        uint32_t a[2][4];
        ExRot r[4];
        // (kEarly: each piece's input opened before the MFMA that starts its gap; EO = early open)
#define EO(...) do { if constexpr (kEarly) ex_open(__VA_ARGS__); } while (0)
        EO(D.d[0].x);
        ex_mfma<0>(X.A3[0], EX_LO(X.b[0][0]));
        g[0] = u_begin(D.d[0].x);                                // gap 0
        EO(D.d[0].y);
        ex_mfma<1>(X.A3[0], EX_LO(X.b[0][1]));
        // operands are kept allocated two MFMAs past their last reader (three with the early opens, whose missing
        // pads shorten the gaps: tools/isa_hazards.py's 64-issue-cycle rule)
#define EK(...) do { if constexpr (!kEarly) ex_keep(__VA_ARGS__); } while (0)
#define EK3(...) do { if constexpr (kEarly) ex_keep(__VA_ARGS__); } while (0)
        EK(Y.A6);  // read by the previous group's last MFMAs
        EK(Y.b[1][0]);
        EK(Y.b[1][1]);
        g[1] = u_begin(D.d[0].y);                                // gap 1
        EO(D.d[1].x);
        ex_mfma<2>(X.A3[0], EX_LO(X.b[1][0]));
        EK3(Y.A6);
        EK3(Y.b[1][0]);
        EK3(Y.b[1][1]);
        if (sync) __syncthreads();  // the chunk's barrier: after the previous group's V writes, before this read
        read_b(c, p + 1, Y);                                     // gap 2: consumed in the next group
        g[2] = u_begin(D.d[1].x);
        EO(D.d[1].y);
        ex_mfma<3>(X.A3[0], EX_LO(X.b[1][1]));
        g[3] = u_begin(D.d[1].y);                                // gap 3
        read_dt_pair(c, p + 3, D);                               //        consumed in the next group
        EO(I0.d);
        ex_mfma<0>(X.A3[1], EX_HI(X.b[0][0]));
        item_begin(I0, is, inl);                                 // gap 4
        ex_mfma<1>(X.A3[1], EX_HI(X.b[0][1]));
        EK(X.A3[0]);
        v_table(I0);                                             // gap 5
        if constexpr (!kEarly) ex_open(X.A3[0]);
        const i32x4 A40 = ex_shr8(X.A3[0]);
        ex_ready(A40);
        EO(I1.d);
        ex_mfma<2>(X.A3[1], EX_HI(X.b[1][0]));
        EK3(X.A3[0]);
        item_begin(I1, is + 1, inl);                             // gap 6
        ex_mfma<3>(X.A3[1], EX_HI(X.b[1][1]));
        v_table(I1);                                             // gap 7
        if constexpr (!kEarly) ex_open(X.A3[1]);
        const i32x4 A41 = ex_shr8(X.A3[1]);
        ex_ready(A41);
        EO(P.g[0].y);
        ex_mfma<4>(A40, EX_LO(X.b[0][0]));
        r[0] = u_a(P, 0);                                        // gap 8
        u_s(P, 0, r[0], a);
        EO(r[0].tc);
        EO(I0.g.y);
        ex_mfma<5>(A40, EX_LO(X.b[0][1]));
        EK(X.A3[1]);
        u_c(P, 0, r[0], a);                                      // gap 9
        item_a(I0);
        EO(P.g[1].y);
        ex_mfma<6>(A40, EX_LO(X.b[1][0]));
        EK3(X.A3[1]);
        r[1] = u_a(P, 1);                                        // gap 10
        u_s(P, 1, r[1], a);
        EO(r[1].tc);
        EO(I1.g.y);
        ex_mfma<7>(A40, EX_LO(X.b[1][1]));
        u_c(P, 1, r[1], a);                                      // gap 11
        item_a(I1);
        EO(P.g[2].y);
        ex_mfma<4>(A41, EX_HI(X.b[0][0]));
        r[2] = u_a(P, 2);                                        // gap 12
        u_s(P, 2, r[2], a);
        EO(r[2].tc);
        EO(I0.r.ts);
        ex_mfma<5>(A41, EX_HI(X.b[0][1]));
        EK(A40);
        u_c(P, 2, r[2], a);                                      // gap 13
        item_s(I0);
        EO(P.g[3].y);
        ex_mfma<6>(A41, EX_HI(X.b[1][0]));
        EK3(A40);
        r[3] = u_a(P, 3);                                        // gap 14
        u_s(P, 3, r[3], a);
        EO(r[3].tc);
        EO(I0.r.tc);
        ex_mfma<7>(A41, EX_HI(X.b[1][1]));
        u_c(P, 3, r[3], a);                                      // gap 15
        item_c(I0);
        // the next pair's operands: dense digits, compressed level-5/6 bytes (lane-swapped below)
        uint32_t c5[2][2], c6[2][2];
        EO(a[0][0], a[0][1]);
        EO(a[0][2], a[0][3]);
        EO(a[1][0], a[1][1]);
        EO(a[1][2], a[1][3]);
        EO(I1.r.ts);
        ex_smfma<8>(X.A5, X.b[0][0], kIdx);
#pragma unroll
        for (int qd = 0; qd < 2; ++qd) {                         // gap 16
            if constexpr (!kEarly) {
                ex_open(a[qd][0], a[qd][1]);
                ex_open(a[qd][2], a[qd][3]);
            }
            Y.A3[qd] = i32x4{(int)a[qd][0], (int)a[qd][1], (int)a[qd][2], (int)a[qd][3]};
#pragma unroll
            for (int w = 0; w < 2; ++w)
                c5[qd][w] = __builtin_amdgcn_perm(a[qd][2 * w + 1], a[qd][2 * w], 0x07060302u);  // d2, d3 of each
            ex_ready(c5[qd][0], c5[qd][1]);
        }
        ex_ready(Y.A3[0]);
        ex_ready(Y.A3[1]);
        item_s(I1);
        EO(I1.r.tc);
        ex_smfma<9>(X.A5, X.b[0][1], kIdx);
        EK(A41);
#pragma unroll
        for (int qd = 0; qd < 2; ++qd) {                         // gap 17
#pragma unroll
            for (int w = 0; w < 2; ++w)
                c6[qd][w] = __builtin_amdgcn_perm(a[qd][2 * w + 1], a[qd][2 * w], 0x0C070C03u);  // d3, 0 of each
            ex_ready(c6[qd][0], c6[qd][1]);
        }
        item_c(I1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // the table entries of pair +2: consumed in the next group
            P.e[i] = tab[g[i].idx];
            P.g[i] = g[i];
        }

        ex_smfma<10>(X.A5, X.b[1][0], kIdx);
        EK3(A41);
        {                                                        // gap 18
            uint32_t s5[2][2], s6[2][2];
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                const auto t5 = __builtin_amdgcn_permlane32_swap(c5[0][w], c5[1][w], false, false);
                const auto t6 = __builtin_amdgcn_permlane32_swap(c6[0][w], c6[1][w], false, false);
                s5[0][w] = t5[0];
                s5[1][w] = t5[1];
                s6[0][w] = t6[0];
                s6[1][w] = t6[1];
            }
            Y.A5 = i32x4{(int)s5[0][0], (int)s5[0][1], (int)s5[1][0], (int)s5[1][1]};
            Y.A6 = i32x4{(int)s6[0][0], (int)s6[0][1], (int)s6[1][0], (int)s6[1][1]};
        }
        ex_ready(Y.A5);
        ex_ready(Y.A6);
        EO(I0.dc, I0.dsn);
        ex_smfma<11>(X.A5, X.b[1][1], kIdx);
        item_post(I0);                                           // gap 19
        EO(I1.dc, I1.dsn);
        ex_smfma<12>(X.A6, X.b[0][0], kIdx);
        item_post(I1);                                           // gap 20
        ex_smfma<13>(X.A6, X.b[0][1], kIdx);
        EK(X.A5);
        v_write(I0, icj, is);                                    // gap 21
        v_write(I1, icj, is + 1);
        ex_smfma<14>(X.A6, X.b[1][0], kIdx);
        EK3(X.A5);
        v_read(ncj, ns, I0);                                     // gap 22: the next group's items
        v_read(ncj, ns + 1, I1);
        ex_smfma<15>(X.A6, X.b[1][1], kIdx);
#undef EO
#undef EK
#undef EK3
        ex_keep(X.b[0][0]);
        ex_keep(X.b[0][1]);
    };
#undef EX_LO
#undef EX_HI

    double pre = 0.0, v = 0.0;
#pragma unroll
    for (int c = 0; c < kExDtSlots - 1; ++c) {
        fetch_dt(c, v);
        store_dt(c, v);
    }
    fetch_dt(kExDtSlots - 1, pre);
    __syncthreads();  // table + the first three chunks' times
#pragma unroll
    for (int s = 0; s < kExItems; ++s) produce(0, s);  // chunk 0
    produce(1, 0);                                      // and the first two items of chunk 1
    produce(1, 1);
    ExOps X, Y;
    ExPend P;
    ExDt D;
    VItem I0, I1;
    if (active) {  // pipeline prologue: U of pair 0, table entries of pair 1, photon times of pair 2, V items (1, 2..3)
        ExDt D0;
        read_dt_pair(0, 0, D0);
        uint32_t a[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const ExArg g = begin1((i & 1) ? D0.d[i >> 1].y : D0.d[i >> 1].x);
            ex_end(tab[g.idx], g.y, a[i >> 1][2 * (i & 1)], a[i >> 1][2 * (i & 1) + 1]);
        }
        uint32_t c5[2][2], c6[2][2];
#pragma unroll
        for (int qd = 0; qd < 2; ++qd) {
            X.A3[qd] = i32x4{(int)a[qd][0], (int)a[qd][1], (int)a[qd][2], (int)a[qd][3]};
#pragma unroll
            for (int w = 0; w < 2; ++w) {
                c5[qd][w] = __builtin_amdgcn_perm(a[qd][2 * w + 1], a[qd][2 * w], 0x07060302u);
                c6[qd][w] = __builtin_amdgcn_perm(a[qd][2 * w + 1], a[qd][2 * w], 0x0C070C03u);
            }
        }
        uint32_t s5[2][2], s6[2][2];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const auto t5 = __builtin_amdgcn_permlane32_swap(c5[0][w], c5[1][w], false, false);
            const auto t6 = __builtin_amdgcn_permlane32_swap(c6[0][w], c6[1][w], false, false);
            s5[0][w] = t5[0];
            s5[1][w] = t5[1];
            s6[0][w] = t6[0];
            s6[1][w] = t6[1];
        }
        X.A5 = i32x4{(int)s5[0][0], (int)s5[0][1], (int)s5[1][0], (int)s5[1][1]};
        X.A6 = i32x4{(int)s6[0][0], (int)s6[0][1], (int)s6[1][0], (int)s6[1][1]};
        read_dt_pair(0, 1, D);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            P.g[i] = begin1((i & 1) ? D.d[i >> 1].y : D.d[i >> 1].x);
            P.e[i] = tab[P.g[i].idx];
        }
        read_dt_pair(0, 2, D);
        v_read(1, 2, I0);
        v_read(1, 3, I1);
    }
    __syncthreads();
    if (active) {
        read_b(0, 0, X);
        Y = X;
    }
    for (int c = 0; c < nch; ++c) {
        // chunk c+3's times (fetched one chunk ago) into the slot of chunk c-1, read by every wave before the last
        // barrier
        store_dt(c + kExDtSlots - 1, pre);
        fetch_dt(c + kExDtSlots, pre);
        const int nl1 = nlive_of(c + 1), nl2 = nlive_of(c + 2);
        if (active) {
            pgroup(X, Y, P, D, I0, I1, c, 0, nl1, nl2, false);
            pgroup(Y, X, P, D, I0, I1, c, 1, nl1, nl2, false);
            pgroup(X, Y, P, D, I0, I1, c, 2, nl1, nl2, false);
            pgroup(Y, X, P, D, I0, I1, c, 3, nl1, nl2, true);
            const bool fold_now = (c + 1) % kExFold == 0 || c + 1 == nch;
            if (!fold_now && (c + 1) % kExCarry == 0) {
                mfma_drain();
                ex_static_for<4>([&](auto fx) {  // fragment, Re/Im
                    constexpr int t = decltype(fx)::value;
                    ex_static_for<16>([&](auto rr) {
                        constexpr int r = decltype(rr)::value;
                        int l0 = ex_acc_read(ex_areg<t, r>{}), l1 = ex_acc_read(ex_areg<4 + t, r>{});
                        int l2 = ex_acc_read(ex_areg<8 + t, r>{}), l3 = ex_acc_read(ex_areg<12 + t, r>{});
                        l1 += l0 >> 8;  // floor division by 256
                        l0 &= 255;
                        l2 += l1 >> 8;
                        l1 &= 255;
                        l3 += l2 >> 8;
                        l2 &= 255;
                        ex_acc_write(ex_areg<t, r>{}, l0);
                        ex_acc_write(ex_areg<4 + t, r>{}, l1);
                        ex_acc_write(ex_areg<8 + t, r>{}, l2);
                        ex_acc_write(ex_areg<12 + t, r>{}, l3);
                    });
                });
                mfma_operand_guard();
            }
            if (fold_now) {
                mfma_drain();
                const bool first_fold = c + 1 <= kExFold, last = c + 1 == nch;
                // opaque copies of the lane's scratch pointer and trial index: the addresses derived from them
                // must be formed here, not hoisted out of the photon loop
                long long* fp = fs;
                int64_t cl = c0 + ar - first + frow * nf;
                int64_t lim = nf - c0 - ar;  // trial c0 + 64 a + 32 f + ar is in the grid iff 64 a + 32 f < lim
                asm volatile("" : "+v"(fp), "+v"(cl), "+v"(lim));
                ex_static_for<2>([&](auto ff) {
                    constexpr int f = decltype(ff)::value;
                    ex_static_for<16>([&](auto rr) {
                        constexpr int r = decltype(rr)::value;
                        long long re = ex_level_sum(ex_acc_read(ex_areg<2 * f, r>{}), ex_acc_read(ex_areg<4 + 2 * f, r>{}),
                                                    ex_acc_read(ex_areg<8 + 2 * f, r>{}), ex_acc_read(ex_areg<12 + 2 * f, r>{}));
                        long long im = ex_level_sum(ex_acc_read(ex_areg<2 * f + 1, r>{}), ex_acc_read(ex_areg<5 + 2 * f, r>{}),
                                                    ex_acc_read(ex_areg<9 + 2 * f, r>{}), ex_acc_read(ex_areg<13 + 2 * f, r>{}));
                        long long* const fr = fp + (f * 32 + r) * 64;
                        long long* const fi = fp + (f * 32 + 16 + r) * 64;
                        if (!first_fold) {
                            re += *fr;
                            im += *fi;
                        }
                        if (!last) {
                            *fr = re;
                            *fi = im;
                        } else {
                            // D[row a][col] of fragment f: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 h;
                            // trial c0 + 64 a + 32 f + col, output slot o = frow * nf + trial - first
                            const int ra = (r & 3) + 8 * (r >> 2) + 4 * h;
                            const int64_t off = kExCols * ra + 32 * f;
                            const int64_t o = cl + off;
                            if (off < lim && o >= 0 && o < count) {
                                atomicAdd(&tot[(int64_t)comp * count + o], (unsigned long long)re);
                                atomicAdd(&tot[(int64_t)(comp + 1) * count + o], (unsigned long long)im);
                            }
                        }
                    });
                });
                ex_acc_zero();
                mfma_operand_guard();
            }
        } else {  // waves without a tile only produce V items, on the same barrier schedule
            for (int s = 2; s < kExItems; ++s) produce(c + 1, s);
            __syncthreads();
            produce(c + 2, 0);
            produce(c + 2, 1);
        }
    }
}

// Statistic from the exact totals (periodsearch.py:67-69 and :120-123 in the reference's formula order), and
// the fix-up list: trials whose power is too small for the kernel's error bound to guarantee 1e-6 relative.
// Error model: per term of U.V (2^30 roundings of both factors, fp32 residual rotation) |e| <= 3e-9, rms <= 1e-9,
// independent across photons and harmonics, so C_k and S_k carry errors of standard deviation
// sc = sqrt(N) 1e-9 and Z2_k = (2/N)(C^2 + S^2) one of (4/N) sc sqrt(C^2 + S^2) (+ (2/N) 2 sc^2 bias). A sum of
// harmonics i <= k (Z2, and H's cumulative g_k = sum_{i<=k} Z2_i - 4(k-1)) has standard deviation
// (4/N) sc sqrt(sum_{i<=k} (C_i^2 + S_i^2)); the bound is kappa = 10 of them plus the bias. H = max_k g_k moves
// by at most the bound of any g_k that can reach the maximum (g_k + err_k >= H - err_k*), so only those count.
// nchunk > 1 (searches of >= 2^27 photons): the photons ran in chunks of < 2^27, each into its own int64 totals
// (tot + c * chunk_stride, exact per chunk); their sum is formed exactly as 32-bit halves summed in int64 (each
// half-sum < nchunk 2^32) and converted once.
__device__ __forceinline__ double ex_total(const long long* __restrict__ tot, int64_t idx, int nchunk,
                                           int64_t chunk_stride) {
    if (nchunk == 1) return (double)tot[idx] * kExUnit;
    long long hi = 0, lo = 0;
    for (int c = 0; c < nchunk; ++c) {
        const long long v = tot[(int64_t)c * chunk_stride + idx];
        hi += v >> 32;                 // arithmetic shift: v = hi 2^32 + lo, 0 <= lo < 2^32
        lo += v & 0xffffffffLL;
    }
    return ((double)hi * 4294967296.0 + (double)lo) * kExUnit;
}

__global__ __launch_bounds__(256) void k_search_finalize_exact(const long long* __restrict__ tot, int64_t count, int m,
                                                               int stat, double n, double sc, double rel, int64_t tbase,
                                                               double* __restrict__ out, int* __restrict__ nflag,
                                                               int64_t* __restrict__ flagged, int nchunk,
                                                               int64_t chunk_stride) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const double w = 2.0 / n, kappa = 10.0;
    const double lin = kappa * 2.0 * w * sc, quad = w * 2.0 * (kappa * sc) * (kappa * sc);
    auto zk = [&](int k) {
        const double c = ex_total(tot, (int64_t)(2 * k) * count + t, nchunk, chunk_stride);
        const double s = ex_total(tot, (int64_t)(2 * k + 1) * count + t, nchunk, chunk_stride);
        return c * c + s * s;
    };
    double p, err;
    if (stat == CRIMP_STAT_Z2) {
        double zsum = 0.0;
        for (int k = 0; k < m; ++k) zsum += zk(k);
        p = zsum * w;
        err = lin * sqrt(zsum) + m * quad;
    } else {
        double cum = 0.0, raw = 0.0, best = -INFINITY, ebest = 0.0;
        for (int k = 0; k < m; ++k) {
            const double z = zk(k);
            cum += z * w;
            raw += z;
            const double v = cum - 4.0 * (double)k;
            if (v > best) {
                best = v;
                ebest = lin * sqrt(raw) + (k + 1) * quad;
            }
        }
        p = best;
        err = ebest;
        cum = 0.0;
        raw = 0.0;
        for (int k = 0; k < m; ++k) {  // every g_k that the errors could lift to the maximum
            const double z = zk(k);
            cum += z * w;
            raw += z;
            const double ek = lin * sqrt(raw) + (k + 1) * quad;
            if (cum - 4.0 * (double)k + ek >= best - ebest) err = fmax(err, ek);
        }
    }
    out[t] = p;
    if (!(err <= rel * fabs(p))) flagged[atomicAdd(nflag, 1)] = tbase + t;
}

// arithmetic-progression check on the device: |f_j - (f_0 + j delta)| <= 16 ulp(max|f|), delta from the ends.
// Each block writes its (max deviation, max |f|) to part[blockIdx] (plain stores: same-address atomics from every
// block serialise at L2); k_ap_final reduces them. One pass of eight loads in flight per thread over up to
// kApBlocks blocks: the whole 8 MB of a 1e6-trial grid is in flight at once (64 blocks with a loop: 14.7 us).
constexpr int kApBlocks = 1024;
// block b of nb of the check (256 threads): k_ap_check's body, and the check blocks that ride in a cached NUFFT
// search's first gather launch (k_nu_gather, NuFold). Thread 0 returns the block's pair.
__device__ __forceinline__ double2 ap_check_block(const double* __restrict__ f, int64_t nf, int b, int nb) {
    const double f0 = f[0];
    const double d = (f[nf - 1] - f0) / (double)(nf - 1);
    double dev = 0.0, fm = 0.0;
    constexpr int U = 8;
    const int64_t stride = (int64_t)nb * 256;
    for (int64_t j0 = (int64_t)b * 256 + threadIdx.x; j0 < nf; j0 += U * stride) {
        double v[U];
#pragma unroll
        for (int q = 0; q < U; ++q) v[q] = f[j0 + q * stride < nf ? j0 + q * stride : nf - 1];
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int64_t j = j0 + q * stride;
            if (j < nf) {
                dev = fmax(dev, fabs(v[q] - (f0 + (double)j * d)));
                fm = fmax(fm, fabs(v[q]));
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        dev = fmax(dev, __shfl_xor(dev, o));
        fm = fmax(fm, __shfl_xor(fm, o));
    }
    __shared__ double red[2][4];
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = dev;
        red[1][threadIdx.x >> 6] = fm;
    }
    __syncthreads();
    dev = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
    fm = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
    return make_double2(dev, fm);
}
__global__ __launch_bounds__(256) void k_ap_check(const double* __restrict__ f, int64_t nf, double2* __restrict__ part,
                                                  int* __restrict__ zero) {
    const double2 r = ap_check_block(f, nf, (int)blockIdx.x, (int)gridDim.x);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = r;
        if (blockIdx.x == 0 && zero) *zero = 0;  // the NUFFT's order flag (k_nu_sorted ORs into it afterwards)
    }
}

// info[0] = delta, info[1] = max deviation, info[2] = max |f| (doubles); with tt (a NUFFT search) also the plan's
// scalars nu[0..3] = delta, f_0, t[0] - t0, t[n-1] - t0 -- one read-back for all of them -- and the NUFFT's flags
// nuflags[0] = 0 (fix-up count), nuflags[1] = 0, or 2 when the search runs a cached plan (ex.on) whose scalars, photon
// order (order, MFMA-slot plans) or progression no longer hold: every NUFFT kernel that reads photon-derived tables
// then exits, and the host redoes the search from a fresh plan.
struct NuExpect {
    double v[4];       // delta, f_0, t[0] - t0, t[n-1] - t0 the cached plan was made from
    int on;            // a cached plan is running
    int check_order;   // its spread reads photons in order (k_nu_sorted ran into *order)
};
__global__ __launch_bounds__(256) void k_ap_final(const double* __restrict__ f, int64_t nf,
                                                  const double2* __restrict__ part, int nb, double* __restrict__ info,
                                                  const double* __restrict__ tt, double t0, int64_t n,
                                                  double* __restrict__ nu, const int* __restrict__ order,
                                                  NuExpect ex, int* __restrict__ nuflags) {
    double dev = 0.0, fm = 0.0;
    for (int b = threadIdx.x; b < nb; b += blockDim.x) {
        dev = fmax(dev, part[b].x);
        fm = fmax(fm, part[b].y);
    }
    for (int o = 32; o > 0; o >>= 1) {
        dev = fmax(dev, __shfl_xor(dev, o));
        fm = fmax(fm, __shfl_xor(fm, o));
    }
    __shared__ double red[2][4];
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = dev;
        red[1][threadIdx.x >> 6] = fm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double f0 = f[0];
        const double d = (f[nf - 1] - f0) / (double)(nf - 1);
        dev = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
        fm = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
        info[0] = d;
        info[1] = dev;
        info[2] = fm;
        if (tt) {
            const double a0 = tt[0] - t0, a1 = tt[n - 1] - t0;
            nu[0] = d;
            nu[1] = f0;
            nu[2] = a0;
            nu[3] = a1;
            if (nuflags) {
                int m = 0;
                if (ex.on) {
                    const bool ok = isfinite(d) && d != 0.0 && dev <= 16.0 * 2.220446049250313e-16 * fm;
                    m = !(ok && d == ex.v[0] && f0 == ex.v[1] && a0 == ex.v[2] && a1 == ex.v[3] &&
                          (!ex.check_order || *order == 0));
                }
                nuflags[0] = 0;
                nuflags[1] = m ? 2 : 0;
            }
        }
    }
}
