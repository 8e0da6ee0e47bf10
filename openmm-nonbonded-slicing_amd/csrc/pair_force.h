// pair_force.h -- the raw forces of a tile pair, a 1-4 exception and an Ewald exclusion correction, once: what the per-atom force table
// (atomforce.hip) adds under its own keys and the per-slice virial (virial.hip, section 4.14) contracts with the
// pair's own delta.
#pragma once
#include "snb_internal.h"
#include "pair_math.h"
#include <type_traits>

namespace snb {

// Force factors of the pair (i, j), every lambda 1, as the forces instantiation of tileSteps (direct.hip) forms them: the force on i is
// fC * delta (Coulomb) + fLJ * delta (vdW), delta = r_i - r_j (returned in dx, dy, dz).  Double precision takes the Ewald and dispersion
// factors from the polynomials of the forces kernels where the guard keeps them (p.ewUsePoly), else and in single precision from erfcFromExp / fexp.  Returns whether the pair is inside the cutoff.
template <typename Real, int MC, bool WRAP>
__device__ __forceinline__ bool pairForces(const DirectParams<Real>& p, const typename Vec<Real>::T4 pi, const typename Vec<Real>::T2 sei, const Real qi, const Real c6i,
                                           const typename Vec<Real>::T4 xj, const typename Vec<Real>::T2 sj2, Real& dx, Real& dy, Real& dz, Real& fC, Real& fLJ) {
    dx = pi.x - xj.x; dy = pi.y - xj.y; dz = pi.z - xj.z;
    if (WRAP) wrapDelta<Real>(dx, dy, dz, p.box, p.invBoxDiag);
    const Real r2 = dx * dx + dy * dy + dz * dz;
    const Real invR = rsq(r2);
    const Real r = r2 * invR;
    const bool include = MC == MC_NOCUTOFF ? true : (r2 < p.cutoff2);
    // Lennard-Jones (sigeps holds sigma/2 and 2 sqrt(eps))
    const Real sig = sei.x + sj2.x;
    Real s2 = sig * invR; s2 *= s2;
    const Real s6 = s2 * s2 * s2;
    const Real es6 = sei.y * sj2.y * s6;
    fLJ = es6 * (Real(12) * s6 - Real(6));
    if (MC == MC_LJPME && std::is_same<Real, double>::value && (p.ewUsePoly & SNB_POLY_DISPERSION)) {
        const Real t = r2 * p.ewScale - Real(1);
        Real gd = p.dispPoly[SNB_DISP_DEG_F64];
#pragma unroll
        for (int k = SNB_DISP_DEG_F64 - 1; k >= 0; k--) gd = gd * t + p.dispPoly[k];
        const Real c6 = c6i * (Real(8) * sj2.x * sj2.x * sj2.x * sj2.y);
        fLJ += Real(6) * c6 * gd * r2;
    } else if (MC == MC_LJPME) {
        const Real dar2 = p.alphaD * p.alphaD * r2;
        const Real dar4 = dar2 * dar2, dar6 = dar4 * dar2;
        const Real invR2 = invR * invR;
        const Real c6 = c6i * (Real(8) * sj2.x * sj2.x * sj2.x * sj2.y);
        const Real coef = invR2 * invR2 * invR2 * c6;
        const Real expd = fexp(-dar2);
        const Real dpre = Real(1) + dar2 + Real(0.5) * dar4 + dar6 * Real(1.0 / 6.0);
        fLJ += Real(6) * coef * (Real(1) - expd * dpre);
    } else if (MC != MC_NOCUTOFF) {
        if (p.useSwitch && r > p.switchDist) {
            const Real tt = (r - p.switchDist) * p.invSwitchWidth;
            const Real sw = Real(1) + tt * tt * tt * (Real(-10) + tt * (Real(15) - tt * Real(6)));
            const Real dsw = tt * tt * (Real(-30) + tt * (Real(60) - tt * Real(30))) * p.invSwitchWidth;
            fLJ = fLJ * sw - es6 * (s6 - Real(1)) * dsw * r;
        }
    }
    const Real qq = qi * xj.w;
    if ((MC == MC_EWALD || MC == MC_LJPME) && std::is_same<Real, double>::value && (p.ewUsePoly & SNB_POLY_FORCE)) {
        const Real t = r2 * p.ewScale - Real(1);
        Real bt = p.ewPoly[SNB_EW_DEG_F64];
#pragma unroll
        for (int k = SNB_EW_DEG_F64 - 1; k >= 0; k--) bt = bt * t + p.ewPoly[k];
        fC = qq * (invR - r2 * bt);
    } else if (MC == MC_EWALD || MC == MC_LJPME) {
        const Real ar = p.alpha * r;
        const Real ex = expNegAlpha2R2(p.alpha2l2e, p.alpha, r2);
        fC = qq * invR * (erfcFromExp(ar, ex) + ar * ex * Real(1.1283791670955126));
    } else if (MC == MC_RF) fC = qq * (invR - Real(2) * p.krf * r2);
    else fC = qq * invR;
    const Real invR2 = invR * invR;
    fC *= invR2; fLJ *= invR2;
    return include;
}

// the force table's contributions to the shared walkers (atom_table.h): six values per pair, Coulomb x y z and vdW x y z of the force on
// the i-end; the partner's end takes the opposite force
struct PairForce {
    static constexpr int NV = 6, UNROLL = 2, J_SIGN = -1;
    template <typename Real, int MC, bool WRAP>
    static __device__ __forceinline__ bool eval(const DirectParams<Real>& p, const typename Vec<Real>::T4 pi, const typename Vec<Real>::T2 sei, const Real qi, const Real c6i,
                                                const typename Vec<Real>::T4 xj, const typename Vec<Real>::T2 sj2, Real* v) {
        Real dx, dy, dz, fC, fLJ;
        const bool include = pairForces<Real, MC, WRAP>(p, pi, sei, qi, c6i, xj, sj2, dx, dy, dz, fC, fLJ);
        v[0] = fC * dx; v[1] = fC * dy; v[2] = fC * dz; v[3] = fLJ * dx; v[4] = fLJ * dy; v[5] = fLJ * dz;
        return include;
    }
    // 1-4 exceptions: the forces of exceptionsBody (direct.hip) with every lambda 1
    template <typename Real, typename Par> static __device__ __forceinline__ void exception(const Par par, const Real dx, const Real dy, const Real dz, const Real invR, const Real s6, double* v) {
        const Real invR2 = invR * invR;
        const double fC = par.z * invR * invR2, fL = par.y * (Real(12) * s6 - Real(6)) * s6 * invR2;
        v[0] = fC * dx; v[1] = fC * dy; v[2] = fC * dz; v[3] = fL * dx; v[4] = fL * dy; v[5] = fL * dz;
    }
    // Ewald exclusion corrections: the forces of exclusionAtomsBody (direct.hip) with every lambda 1, formed in double from the stored
    // coordinates and charges
    template <typename Real>
    static __device__ __forceinline__ void exclusion(const PairListParams<Real>& p, const Real qa, const Real qb, const typename Vec<Real>::T2 sei, const int b, const Real dx, const Real dy, const Real dz, double* v) {
        const double ddx = dx, ddy = dy, ddz = dz;
        const double r2 = ddx * ddx + ddy * ddy + ddz * ddz;
        const double rd = sqrt(r2), invR = 1.0 / rd;
        const double x = p.alpha64 * rd;
        const double qqd = (double)qa * (double)qb * SNB_ONE_4PI_EPS0;
        const double erfv = erf(x);
#pragma unroll
        for (int c = 0; c < 6; c++) v[c] = 0;
        if (erfv > 1e-6) {
            const double f = -qqd * invR * invR * invR * exclusionG(x, exp(-x * x), erfv);
            v[0] = f * ddx; v[1] = f * ddy; v[2] = f * ddz;
        }
        if (p.ljpme) {
            const auto sej = p.sigeps[b];
            const double c6i = 8.0 * (double)sei.x * (double)sei.x * (double)sei.x * (double)sei.y;
            const double c6 = c6i * (8.0 * (double)sej.x * (double)sej.x * (double)sej.x * (double)sej.y);
            const double ad = (double)p.alphaD;
            const double dar2 = ad * ad * r2, dar4 = dar2 * dar2, dar6 = dar4 * dar2;
            const double invR2 = invR * invR;
            const double f = 6.0 * c6 * invR2 * invR2 * invR2 * invR2 * (1.0 - exp(-dar2) * (1.0 + dar2 + 0.5 * dar4 + dar6 * (1.0 / 6.0)));
            v[3] = f * ddx; v[4] = f * ddy; v[5] = f * ddz;
        }
    }
};

}  // namespace snb
