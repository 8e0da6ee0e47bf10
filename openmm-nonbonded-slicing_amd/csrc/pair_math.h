// pair_math.h -- arithmetic helpers shared by the pair kernels (direct.hip) and the per-atom table kernels (atom_table.h, atomenergy.hip, atomforce.hip).
#pragma once
#include "snb_internal.h"

namespace snb {

// ---- math helpers -------------------------------------------------------------------------------
__device__ inline float rsq(float x) { return __builtin_amdgcn_rsqf(x); }
// double: the hardware estimate (v_rsq_f64, ~2^-27) refined by two Newton steps -- about a third of the instructions of 1.0 / sqrt(x),
// which runs its own refinements for the square root and again for the division; relative error < 1e-15 (tests hold 1e-12 on forces)
__device__ inline double rsq(double x) {
    double y = __builtin_amdgcn_rsq(x);
    y = y * (1.5 - 0.5 * x * y * y);
    y = y * (1.5 - 0.5 * x * y * y);
    return y;
}
__device__ inline float fexp(float x) { return __expf(x); }
__device__ inline double fexp(double x) { return exp(x); }
// erfc(ar) given e = exp(-ar^2).  Single precision: Abramowitz & Stegun 7.1.26 (max abs error 1.5e-7), the
// same approximation the reference GPU path uses (coulombLennardJones.cc:18-23); double: libm.
__device__ inline float erfcFromExp(float ar, float e) {
    float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ar);
    return (0.254829592f + (-0.284496736f + (1.421413741f + (-1.453152027f + 1.061405429f * t) * t) * t) * t) * t * e;
}
__device__ inline double erfcFromExp(double ar, double) { return erfc(ar); }
// exp(-alpha^2 r^2): single precision folds log2(e) into the constant and issues one v_exp_f32
__device__ inline float expNegAlpha2R2(float a2l2e, float, float r2) { return __builtin_amdgcn_exp2f(-a2l2e * r2); }
__device__ inline double expNegAlpha2R2(double, double alpha, double r2) { return exp(-alpha * alpha * r2); }
__device__ inline double erfOf(float ar, float) { return (double)erff(ar); }
__device__ inline double erfOf(double ar, double) { return erf(ar); }
// The Ewald exclusion correction's radial factor  g(x) = erf(x) - (2/sqrt(pi)) x exp(-x^2),  x = alpha r.  For small x the two terms
// cancel to 0.752 x^3: in float, any error of erf (1.5e-7 absolute for Abramowitz & Stegun 7.1.26, an ulp for erff) is divided by x^2
// there -- excluded partners a few picometres apart (a Drude particle on its core) were off by kJ/mol/nm.  Below x = 0.5 the series
// (4/sqrt(pi)) x^3 sum_n (-1)^n x^(2n) / (n! (2n+3)), seven terms (truncation < 1e-7 relative), takes its place; double keeps libm erf.
__device__ inline float exclusionG(float x, float e, double erfv) {
    if (x < 0.5f) {
        const float x2 = x * x;
        const float s = 1.0f / 3 - x2 * (1.0f / 5 - x2 * (1.0f / 14 - x2 * (1.0f / 54 - x2 * (1.0f / 264 - x2 * (1.0f / 1560 - x2 * (1.0f / 10800))))));
        return 2.2567583341910252f * x * x2 * s;
    }
    return (float)erfv - x * e * 1.1283791670955126f;
}
__device__ inline double exclusionG(double x, double e, double erfv) { return erfv - x * e * 1.1283791670955126; }
// The LJPME part of the exclusion correction: the radial factors  h3(y) = 1 - e (1 + y + y^2/2)  of the energy and  h4(y) = h3(y) - e y^3/6
// of the force, y = (alpha_d r)^2, e = exp(-y).  They cancel to y^3/6 and y^4/24: in float the rounding of the bracket (1e-7 absolute) is
// divided by y^4/24, 8 % of the force factor at alpha_d r = 0.25 and all of it at 0.125.  Below y = 1 the identity
// 1 = e exp(y) gives  h4 = e sum_{k >= 4} y^k / k!  with every term positive, here to k = 13 (truncation 24 y^10 / 14! < 3e-10 relative),
// and h3 = h4 + e y^3/6; double keeps the closed form on libm's exp.
__device__ inline void dispersionExclusion(float y, float e, float& h3, float& h4) {
    const float y2 = y * y, y3 = y2 * y;
    if (y < 1.0f) {
        float p = 1.0f + y * (1.0f / 13);
#pragma unroll
        for (int k = 12; k >= 5; k--) p = 1.0f + y * (1.0f / k) * p;
        h4 = e * (y2 * y2 * (1.0f / 24)) * p;
        h3 = h4 + e * (y3 * (1.0f / 6));
        return;
    }
    h3 = 1.0f - e * (1.0f + y + 0.5f * y2);
    h4 = 1.0f - e * (1.0f + y + 0.5f * y2 + y3 * (1.0f / 6));
}
__device__ inline void dispersionExclusion(double y, double e, double& h3, double& h4) {
    const double y2 = y * y;
    h3 = 1.0 - e * (1.0 + y + 0.5 * y2);
    h4 = 1.0 - e * (1.0 + y + 0.5 * y2 + y2 * y * (1.0 / 6.0));
}

__device__ inline void ldsAdd(float* p, float v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void ldsAdd(double* p, double v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ inline void gAdd(float* p, float v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void gAdd(double* p, double v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline double waveSum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ inline int sliceOf(int a, int b) { return a > b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; }

template <typename Real> __device__ inline void wrapDelta(Real& dx, Real& dy, Real& dz, const Real* box, const Real* inv) {
    // OpenMM ReferenceForce::getDeltaRPeriodic (triclinic form)
    Real s = floor(dz * inv[2] + Real(0.5)); dx -= s * box[6]; dy -= s * box[7]; dz -= s * box[8];
    s = floor(dy * inv[1] + Real(0.5)); dx -= s * box[3]; dy -= s * box[4];
    s = floor(dx * inv[0] + Real(0.5)); dx -= s * box[0];
}

// The sorted coordinates are box-wrapped per atom (imageOffset = wrapped - user).  Non-periodic exceptions
// (periodicExceptions == false, ReferenceSlicedLJCoulombIxn.cpp:461-464) need the user's own coordinates back.
template <typename Real> __device__ inline void unwrapDelta(Real& dx, Real& dy, Real& dz, const Real* off, int i, int j) {
    dx -= off[3 * i] - off[3 * j]; dy -= off[3 * i + 1] - off[3 * j + 1]; dz -= off[3 * i + 2] - off[3 * j + 2];
}

}  // namespace snb
