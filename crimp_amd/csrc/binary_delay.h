// The orbital delay of a binary model (BT, ELL1): bin_delay, and the kernel of crimp_binary_delay. Included by
// crimp_hip.hip before section 3 (CPModel, cp_one); the C-ABI is in its section 6.
//
// Definition. t is a barycentric arrival time (MJD). tau (s) is the root of tau = D(t - tau / 86400),
// D(t') the orbital delay of the emission time t':
//   tt0 = (t' - T0|TASC) 86400,  pb = PB 86400,  orbits = tt0 / pb - PBDOT (tt0 / pb)^2 / 2,  x = A1 + A1DOT tt0
//   BT:    M = 2 pi frac(orbits),  E - e sin E = M,  w = OM + OMDOT tt0,
//          D = x sin w (cos E - e) + (x sqrt(1 - e^2) cos w + GAMMA) sin E
//   ELL1:  P = 2 pi frac(orbits),  D = x (sin P + EPS2 / 2 sin 2P - EPS1 / 2 cos 2P)
//
// Solve. The orbit and the light-travel equation are one equation in the eccentric anomaly at emission (ELL1: in the
// orbital phase P, with e = 0):
//   g(E) = E - e sin E - M(tta - D(E)) = 0,   tta = (t - T0) 86400,   tau = D(E)
//   g'(E) = 1 - e cos E + (2 pi / pb) (1 - PBDOT tt0 / pb) D'(E)
// so every iteration costs one fp64 sincos, not a Kepler solve inside an outer fixed point. The whole orbits
// n = rint(orbits(tta)) are fixed before the loop and M = 2 pi (orbits - n) is formed in revolutions first, so E and
// every sincos argument of the loop stay within [-pi - e - r, pi + e + r] (r below). x and w depend on tau through
// A1DOT and OMDOT only: they are formed from the previous iterate's tau (a fixed point of ratio <= |A1DOT|, |OMDOT|
// x), and once more from the final tau before the value is returned. sin w, cos w come from one sincos of the angle
// at arrival and the rotation by OMDOT tau (< 1e-4 rad: its series to the 4th power is exact to fp64).
//
// Bound on the loop. The host admits a model only with k = 2 pi A1 / (pb (1 - e)) < 1/2 (crimp_binary_delay), so
// |M'(E)| <= (2 pi / pb)|D'| <= k (1 - e) and g' >= (1 - e)(1 - k) > 0: g is increasing and has one root, inside
// [Ma - e - r, Ma + e + r] with Ma = M(tta) and r = (2 pi / pb)(x (1 + e) + |GAMMA|) the most the light travel moves M.
// That interval is the starting bracket. Each iteration evaluates g at E, moves the bracket end of g's sign to E,
// and takes the Newton step unless it leaves the bracket, in which case it takes the midpoint: the bracket always
// holds the root, so E cannot run away, and a midpoint step at least halves the bracket. From the starter
// E0 = Ma + e sin Ma / sqrt(1 - 2 e cos Ma + e^2) (within ~e^3 of Kepler's root, the light travel adds <= k) Newton's
// quadratic phase starts at once except next to periastron at high e, where g' ~ 1 - e makes the first steps
// overshoot; there the bracket ends of both signs are set within two steps and Newton converges from the convex
// side. The host twin of this loop (crimp_amd/binarymodels.py: binary_delay_host, the same starter, bracket and
// stopping rule) counts at most 12 iterations over e in [0, 0.97] x 4096 mean anomalies (periastron +- 1e-12 rev
// among them) x k in {0, 0.25, 0.45} x three OM, and at most 5 on the fixture models (tests/test_binary_host.py
// asserts <= kBinMaxIter / 2); kBinMaxIter = 32 is more than twice the count. A lane that has not converged at the cap returns NaN: no loop waits on convergence.
//
// Stopping rule. A Newton step |dE| <= 2^-31 is accepted: the step's own error is <= g''/(2 g') dE^2 <= e / ((1 - e)
// (1 - k)) 2^-62 < 2e-17 rad for e <= 0.97, and tau = D(E) + D'(E) dE + D''(E) dE^2 / 2 at the new E without another
// sincos (the cubic term is < x 2^-93).
#pragma once

struct BinModel {
    int32_t kind;  // CRIMP_BINARY_BT | CRIMP_BINARY_ELL1
    int32_t pad_;
    double t0;              // T0 | TASC (MJD)
    double pb;              // PB * 86400 (s)
    double pbdot, a1dot;    // dimensionless
    double a1;              // light-seconds
    double ecc, s1me2;      // BT: e, sqrt(1 - e^2); ELL1: 0, 1
    double om, omdot;       // BT: rad, rad/s
    double gamma;           // BT: s
    double eps1, eps2;      // ELL1
    double amp;             // |D| <= x amp + |gamma|: 1 + e (BT), 1 + (|EPS1| + |EPS2|) / 2 (ELL1)
};
static_assert(sizeof(BinModel) % 8 == 0, "BinModel follows CPModel in the kernel arguments");

constexpr int kBinMaxIter = 32;
constexpr double kBinTwoPi = 6.283185307179586476925;
constexpr double kBinTol = 4.656612873077392578125e-10;  // 2^-31

// D, D', D'' at the eccentric anomaly (orbital phase) whose sine and cosine are s, c, for the emission time
// tt = tta - tau (s since T0|TASC); sw, cw: sin and cos of OM + OMDOT tta
__device__ __forceinline__ void bin_orbit(const BinModel* __restrict__ B, bool bt, double tt, double tau, double sw,
                                          double cw, double s, double c, double& D, double& D1, double& D2) {
    const double x = B->a1 + B->a1dot * tt;
    if (bt) {
        // w = (OM + OMDOT tta) - OMDOT tau: rotate by d = OMDOT tau
        const double d = B->omdot * tau, d2 = d * d;
        const double sd = d * (1.0 - d2 * (1.0 / 6.0)), cd = 1.0 - 0.5 * d2 * (1.0 - d2 * (1.0 / 12.0));
        const double so = sw * cd - cw * sd, co = cw * cd + sw * sd;
        const double al = x * so, be = (x * B->s1me2) * co + B->gamma;
        D = al * (c - B->ecc) + be * s;
        D1 = be * c - al * s;
        D2 = -(al * c + be * s);
    } else {
        const double s2 = 2.0 * s * c, c2 = (c - s) * (c + s);
        const double h1 = 0.5 * B->eps1, h2 = 0.5 * B->eps2;
        D = x * ((s + h2 * s2) - h1 * c2);
        D1 = x * ((c + B->eps2 * c2) + B->eps1 * s2);
        D2 = -x * ((s + (4.0 * h2) * s2) - (4.0 * h1) * c2);
    }
}

// tau (s) of the arrival time t (MJD); NaN for a NaN time and for a lane that reaches kBinMaxIter. *iters (may be
// null): the iterations taken.
__device__ __forceinline__ double bin_delay(const BinModel* __restrict__ B, double t, int* iters = nullptr) {
    const bool bt = B->kind == CRIMP_BINARY_BT;
    const double e = B->ecc;
    const double tta = (t - B->t0) * 86400.0;
    const double ua = tta / B->pb;
    const double oa = ua - (0.5 * B->pbdot) * (ua * ua);
    const double n = rint(oa);
    const double Ma = kBinTwoPi * (oa - n);
    double sw = 0.0, cw = 1.0;
    if (bt) sincos(B->om + B->omdot * tta, &sw, &cw);
    double s, c;
    sincos(Ma, &s, &c);
    double E = Ma + e * s / sqrt((1.0 - 2.0 * e * c) + e * e);  // e = 0: Ma; else the root is >= 1 - e > 0
    // the starting bracket [Ma - e - r, Ma + e + r], r with a margin over its roundings
    const double span = e + 1.0001 * (kBinTwoPi / B->pb) * (fabs(B->a1 + B->a1dot * tta) * B->amp + fabs(B->gamma)) + 1e-12;
    double lo = Ma - span, hi = Ma + span;
    double tau = 0.0, res = __builtin_nan("");
    int it = 0;
    for (; it < kBinMaxIter; ++it) {
        sincos(E, &s, &c);
        double D, D1, D2;
        bin_orbit(B, bt, tta - tau, tau, sw, cw, s, c, D, D1, D2);
        const double tt = tta - D;
        const double u = tt / B->pb;
        const double M = kBinTwoPi * ((u - (0.5 * B->pbdot) * (u * u)) - n);
        const double g = (E - e * s) - M;
        const double gp = (1.0 - e * c) + (kBinTwoPi / B->pb) * (1.0 - B->pbdot * u) * D1;
        tau = D;
        if (g > 0.0) hi = E; else lo = E;
        double dE = -g / gp;
        const bool newton = E + dE >= lo && E + dE <= hi;
        if (!newton) dE = 0.5 * (lo + hi) - E;
        E += dE;
        // accepted: a small Newton step; a bracket closed to a few ulp; a NaN time (every comparison is false), which
        // leaves here at once with a NaN result
        if (!(fabs(dE) > kBinTol) && (newton || !(hi - lo > 1e-15 * (1.0 + fabs(E))))) {
            tau = D + dE * (D1 + 0.5 * dE * D2);
            bin_orbit(B, bt, tta - tau, tau, sw, cw, s, c, D, D1, D2);  // x and w at the final emission time
            res = D + dE * (D1 + 0.5 * dE * D2);
            ++it;
            break;
        }
    }
    if (iters) *iters = it;
    return res;
}

// crimp_binary_delay: one grid-stride kernel; t_emit may be null
__global__ __launch_bounds__(256) void k_binary_delay(const double* __restrict__ t, int64_t n, const BinModel Bv,
                                                      double* __restrict__ delay, double* __restrict__ t_emit) {
    const BinModel* B = &Bv;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double ti = t[i];
        const double tau = bin_delay(B, ti);
        delay[i] = tau;
        if (t_emit) t_emit[i] = ti - tau / 86400.0;
    }
}
