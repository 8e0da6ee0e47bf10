// pair_energy.h -- the raw energies of a tile pair, a 1-4 exception and an Ewald exclusion correction, once: what the per-atom energy table
// (atomenergy.hip) and the group-pair matrix (grouppairs.hip, section 4.13) add under their own keys.
#pragma once
#include "snb_internal.h"
#include "pair_math.h"

namespace snb {

// raw pair energies of (i, j) as the energy instantiation of tileSteps (direct.hip) forms them; returns whether the pair is inside the cutoff
template <typename Real, int MC, bool WRAP>
__device__ __forceinline__ bool pairEnergies(const DirectParams<Real>& p, const typename Vec<Real>::T4 pi, const typename Vec<Real>::T2 sei, const Real qi, const Real c6i,
                                             const typename Vec<Real>::T4 xj, const typename Vec<Real>::T2 sj2, Real& eC, Real& eLJ) {
    Real dx = pi.x - xj.x, dy = pi.y - xj.y, dz = pi.z - xj.z;
    if (WRAP) wrapDelta<Real>(dx, dy, dz, p.box, p.invBoxDiag);
    const Real r2 = dx * dx + dy * dy + dz * dz;
    const Real invR = rsq(r2);
    const Real r = r2 * invR;
    const bool include = MC == MC_NOCUTOFF ? true : (r2 < p.cutoff2);
    // Lennard-Jones (sigeps holds sigma/2 and 2 sqrt(eps))
    const Real sig = sei.x + sj2.x;
    Real s2 = sig * invR; s2 *= s2;
    const Real s6 = s2 * s2 * s2;
    eLJ = sei.y * sj2.y * s6 * (s6 - Real(1));
    if (MC == MC_LJPME) {      // multiplicative grid term + potential shifts
        const Real dar2 = p.alphaD * p.alphaD * r2, dar4 = dar2 * dar2;
        const Real invR2 = invR * invR;
        const Real c6 = c6i * (Real(8) * sj2.x * sj2.x * sj2.x * sj2.y);
        const Real coef = invR2 * invR2 * invR2 * c6;
        const Real expd = fexp(-dar2);
        const Real epre = Real(1) + dar2 + Real(0.5) * dar4;
        Real sg2 = sig * sig; const Real sg6 = sg2 * sg2 * sg2 * p.invCut6;
        eLJ += coef * (Real(1) - expd * epre) + sei.y * sj2.y * (Real(1) - sg6) * sg6 - c6 * p.multShift6;
    } else if (MC != MC_NOCUTOFF) {
        if (p.useSwitch && r > p.switchDist) {
            const Real tt = (r - p.switchDist) * p.invSwitchWidth;
            eLJ *= Real(1) + tt * tt * tt * (Real(-10) + tt * (Real(15) - tt * Real(6)));
        }
    }
    const Real qq = qi * xj.w;
    if ((MC == MC_EWALD || MC == MC_LJPME) && sizeof(Real) == 4 && (p.ewUsePoly & SNB_POLY_ENERGY)) {
        // single precision: qq (1/r - Et(r^2)), Et = erf(ar)/r as the degree-13 polynomial of the packed energy kernels -- the error of the
        // Abramowitz & Stegun erfc is one-signed and an atom's column sums thousands of pairs whose direct and reciprocal parts cancel
        const Real t = r2 * p.ewScale - Real(1);
        Real et = p.ewPolyE[13];
#pragma unroll
        for (int k = 12; k >= 0; k--) et = et * t + p.ewPolyE[k];
        eC = qq * (invR - et);
    } else if (MC == MC_EWALD || MC == MC_LJPME) {
        const Real ar = p.alpha * r;
        eC = qq * invR * erfcFromExp(ar, expNegAlpha2R2(p.alpha2l2e, p.alpha, r2));
    } else if (MC == MC_RF) eC = qq * (invR + p.krf * r2 - p.crf);
    else eC = qq * invR;
    return include;
}

// the energy contributions to the shared walkers (atom_table.h) and to the group-pair kernel: two values per pair, Coulomb and vdW
struct PairEnergy {
    static constexpr int NV = 2, UNROLL = 4, J_SIGN = 1;
    template <typename Real, int MC, bool WRAP>
    static __device__ __forceinline__ bool eval(const DirectParams<Real>& p, const typename Vec<Real>::T4 pi, const typename Vec<Real>::T2 sei, const Real qi, const Real c6i,
                                                const typename Vec<Real>::T4 xj, const typename Vec<Real>::T2 sj2, Real* v) {
        return pairEnergies<Real, MC, WRAP>(p, pi, sei, qi, c6i, xj, sj2, v[0], v[1]);
    }
    // 1-4 exceptions: the energies of exceptionsBody (direct.hip)
    template <typename Real, typename Par> static __device__ __forceinline__ void exception(const Par par, const Real dx, const Real dy, const Real dz, const Real invR, const Real s6, double* v) {
        v[0] = par.z * invR; v[1] = par.y * (s6 - Real(1)) * s6;
    }
    // Ewald exclusion corrections: the energies of exclusionAtomsBody (direct.hip; formed in double as there)
    template <typename Real>
    static __device__ __forceinline__ void exclusion(const PairListParams<Real>& p, const Real qa, const Real qb, const typename Vec<Real>::T2 sei, const int b, const Real dx, const Real dy, const Real dz, double* v) {
        const double rd = sqrt((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);
        const double qqd = (double)qa * (double)qb * SNB_ONE_4PI_EPS0;
        const double erfv = erf(p.alpha64 * rd);
        v[0] = erfv > 1e-6 ? -qqd * erfv / rd : -p.alpha64 * 1.1283791670955126 * qqd;
        v[1] = 0;
        if (p.ljpme) {
            const Real r2 = dx * dx + dy * dy + dz * dz;
            const Real invR = Real(1) / sqrt(r2);
            const auto sej = p.sigeps[b];
            const Real c6i = Real(8) * sei.x * sei.x * sei.x * sei.y;
            const Real c6 = c6i * (Real(8) * sej.x * sej.x * sej.x * sej.y);
            const Real dar2 = p.alphaD * p.alphaD * r2;
            const Real invR2 = invR * invR;
            Real h3, h4;
            dispersionExclusion(dar2, fexp(-dar2), h3, h4);
            v[1] = (double)(c6 * invR2 * invR2 * invR2 * h3);
        }
    }
};

}  // namespace snb
