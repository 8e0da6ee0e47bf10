// The polynomials of the pair kernels' direct-space Ewald terms as a pure host function: plain numbers in, coefficients, measured
// residuals and the decision whether each polynomial may be used out.  No HIP.  Engine::buildEwaldPoly calls fitEwaldPolys and uploads
// the coefficients; tests/ewald_fit_check.cpp calls it without a GPU.
//
// Three entire functions of r^2 are fitted over [0, rmax^2], rmax = cutoff + list padding + 0.02, as monomials in t = 2 r^2 / rmax^2 - 1:
//   Bt(r^2) = [erf(ar) - 2ar/sqrt(pi) e^{-(ar)^2}] / r^3      force factor: [erfc(ar)/r + 2a/sqrt(pi) e^{-(ar)^2}] / r^2 = 1/r^3 - Bt
//                                                             degree 11 in the single-precision kernels, 16 in double
//   Et(r^2) = erf(ar) / r                                     pair energy qq (1/r - Et) of the single-precision kernels, degree 13
//   Gd(r^2) = ad^8 e^{-x} sum_k x^k / (k+4)!, x = (ad r)^2    LJPME dispersion force 6 c6 r^2 Gd of the double-precision kernels, degree 17
// The degrees are fixed, and the truncation error depends on z = a * rmax alone and grows fast with it (Bt, degree 11: 1.5e-7 of Bt(0)
// at z = 2.94, 2.3e-5 at z = 4.05), so a polynomial is used only where its measured residual passes the guard below; elsewhere the
// kernels take their analytic branch.
//
// The guard.  Residuals are taken at kGuardRadii radii in (0, cutoff] against the exact function, the polynomial evaluated as the kernel
// does it: float coefficients, float t = r^2 * scale - 1 and float FMA Horner for degrees 11 and 13, double for 16 and 17.  err* is the
// largest |polynomial - exact|.  A polynomial is used where
//   force       pairF = max r |dBt| <= bar / (2 K)          K r |dBt| is the force error of the reference pair |qi qj| = 1 e^2: at most
//                                                           half the parity bar (3.6e-6 nm^-2 in single precision, 3.6e-8 in double)
//   dispersion  pairD = max r |dGd| <= bar / (12 c6)        6 c6 r |dGd|, c6 = 4 eps sigma^6 of the reference pair sigma = 0.4 nm, eps = 1 kJ/mol
//   energy      sysE  = max |dEt|   <= 1.5e-7 / cutoff      no worse than the analytic branch, erfc(ar)/r with the A&S 7.1.26 erfc
//                                                           (|d erfc| <= 1.5e-7, r <= cutoff)
// bar = 1e-3 kJ/mol/nm in single and mixed precision, 1e-5 in double: the parity tolerances, which max(|F|, 1) makes absolute below
// |F| = 1.  sysE is the error of the polynomial itself -- the float coefficients, evaluated exactly -- and leaves out the rounding of
// the float Horner steps that errE contains (about 3 ulp of Et(0), 4e-7 at alpha = 2.6283): 1.5e-7 is likewise the error of the A&S
// formula and not of its float evaluation, either branch then subtracts from or multiplies with a float 1/r >= 1/cutoff that rounds as
// coarsely, and what the energy polynomial is there for is a pair-energy error that does not keep one sign over 6e7 pairs
// (direct.hip tileStepsPacked), which rounding does not produce.  The forces are held to pairF in full kernel arithmetic.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

namespace snb {

constexpr int kEwaldFitLJPME = 5;      // (snb_method SNB_LJPME: the only method with a dispersion polynomial; engine.hip asserts the value)
constexpr int kEwDegF32 = 11, kEwDegF64 = 16, kEwDegE = 13, kDispDegF64 = 17, kGuardRadii = 16384;
constexpr double kFitPi = 3.14159265358979323846, kFitCoulomb = 138.935456, kRefC6 = 4.0 * 1.0 * 0.4 * 0.4 * 0.4 * 0.4 * 0.4 * 0.4;
constexpr double kBarF32 = 1e-3, kBarF64 = 1e-5, kErfcAbsErr = 1.5e-7;
enum { kPolyForce = 1, kPolyEnergy = 2, kPolyDispersion = 4 };      // bits of EwaldFit::use and of snb_stats.ewald_poly_mask

// the exact functions, in double (the series take over where the closed forms cancel)
inline double ewaldBt(double a, double r2) {
    const double r = std::sqrt(r2), z = a * r;
    if (z < 2e-2) return a * a * a * (4.0 / (3.0 * std::sqrt(kFitPi))) * (1.0 - 0.6 * z * z + (3.0 / 14.0) * z * z * z * z - (1.0 / 18.0) * z * z * z * z * z * z);
    return (std::erf(z) - 2.0 * z / std::sqrt(kFitPi) * std::exp(-z * z)) / (r2 * r);
}
inline double ewaldEt(double a, double r2) {
    const double r = std::sqrt(r2), z = a * r;
    if (z < 1e-3) return a * (2.0 / std::sqrt(kFitPi)) * (1.0 - z * z / 3.0 + z * z * z * z / 10.0);
    return std::erf(z) / r;
}
inline double ewaldGd(double ad, double r2) {
    const double x = ad * ad * r2;
    double sum = 0, term = 1.0 / 24.0;      // sum_k x^k / (k+4)!
    for (int k = 0; k < 60; k++) { sum += term; term *= x / (k + 5); if (term < 1e-18 * sum) break; }
    return std::pow(ad, 8.0) * std::exp(-x) * sum;
}

// Chebyshev interpolant of f(r^2) over [0, r2max] at 96 nodes, truncated at `deg`, as monomial coefficients in t = 2 r^2/r2max - 1
template <typename Fn> void chebyshevToMonomial(Fn f, int deg, double r2max, double* out) {
    const int M = 96;
    std::vector<double> c(deg + 1);
    for (int k = 0; k <= deg; k++) {
        double acc = 0;
        for (int j = 0; j < M; j++) { const double x = std::cos(kFitPi * (j + 0.5) / M); acc += f(0.5 * (x + 1.0) * r2max) * std::cos(kFitPi * k * (j + 0.5) / M); }
        c[k] = acc * 2.0 / M;
    }
    c[0] *= 0.5;
    // T_0 = 1, T_1 = x, T_{k+1} = 2 x T_k - T_{k-1}
    std::vector<double> Tm(deg + 1, 0.0), Tc(deg + 1, 0.0), Tn(deg + 1, 0.0);
    Tm[0] = 1; if (deg >= 1) Tc[1] = 1;
    for (int i = 0; i <= deg; i++) out[i] = 0;
    out[0] += c[0];
    if (deg >= 1) for (int i = 0; i <= deg; i++) out[i] += c[1] * Tc[i];
    for (int k = 2; k <= deg; k++) {
        for (int i = 0; i <= deg; i++) Tn[i] = (i > 0 ? 2.0 * Tc[i - 1] : 0.0) - Tm[i];
        for (int i = 0; i <= deg; i++) { out[i] += c[k] * Tn[i]; Tm[i] = Tc[i]; Tc[i] = Tn[i]; }
    }
}

// the polynomial as a kernel of arithmetic T evaluates it: coefficients, scale, t and every Horner step (one FMA each) rounded to T
template <typename T> double evalKernelPoly(const double* coef, int deg, double r2max, double r2) {
    const T scale = (T)(2.0 / r2max), t = std::fma((T)r2, scale, (T)-1);
    T v = (T)coef[deg];
    for (int k = deg - 1; k >= 0; k--) v = std::fma(v, t, (T)coef[k]);
    return (double)v;
}

struct EwaldFit {
    double ewPoly[21] = {0}, ewPolyE[14] = {0}, dispPoly[21] = {0}, r2max = 1;      // what the engine uploads (ewPoly: degree degF)
    int degF = 0;
    double errF = 0, errE = 0, errD = 0;      // measured residuals over (0, cutoff], in the kernel's arithmetic (errD: 0 without LJPME)
    double pairF = 0, pairD = 0, sysE = 0;    // what the guard looks at: max r |dBt|, max r |dGd|, max |dEt| of the float coefficients evaluated exactly
    double limF = 0, limD = 0, limE = 0;      // ... and its limits for the three
    int use = 0;                              // kPolyForce | kPolyEnergy | kPolyDispersion: the polynomials that pass the guard
};

// Real: the arithmetic of the pair kernel (float: single and mixed precision; double)
template <typename Real> EwaldFit fitEwaldPolys(double alpha, double alphaD, double cutoff, double rmax, int method) {
    constexpr bool f32 = sizeof(Real) == 4;
    EwaldFit fit;
    fit.r2max = rmax * rmax; fit.degF = f32 ? kEwDegF32 : kEwDegF64;
    const bool disp = method == kEwaldFitLJPME;
    chebyshevToMonomial([&](double r2) { return ewaldBt(alpha, r2); }, fit.degF, fit.r2max, fit.ewPoly);
    chebyshevToMonomial([&](double r2) { return ewaldEt(alpha, r2); }, kEwDegE, fit.r2max, fit.ewPolyE);
    if (disp) chebyshevToMonomial([&](double r2) { return ewaldGd(alphaD, r2); }, kDispDegF64, fit.r2max, fit.dispPoly);
    double cf[kEwDegE + 1];      // the float coefficients of Et, for sysE
    for (int k = 0; k <= kEwDegE; k++) cf[k] = (double)(float)fit.ewPolyE[k];
    for (int i = 1; i <= kGuardRadii; i++) {
        const double r = cutoff * i / kGuardRadii, r2 = r * r;
        const double dF = std::fabs(evalKernelPoly<Real>(fit.ewPoly, fit.degF, fit.r2max, r2) - ewaldBt(alpha, r2));
        fit.errF = std::max(fit.errF, dF); fit.pairF = std::max(fit.pairF, r * dF);
        fit.errE = std::max(fit.errE, std::fabs(evalKernelPoly<float>(fit.ewPolyE, kEwDegE, fit.r2max, r2) - ewaldEt(alpha, r2)));
        fit.sysE = std::max(fit.sysE, std::fabs(evalKernelPoly<double>(cf, kEwDegE, fit.r2max, r2) - ewaldEt(alpha, r2)));
        if (disp) { const double dD = std::fabs(evalKernelPoly<double>(fit.dispPoly, kDispDegF64, fit.r2max, r2) - ewaldGd(alphaD, r2)); fit.errD = std::max(fit.errD, dD); fit.pairD = std::max(fit.pairD, r * dD); }
    }
    const double bar = f32 ? kBarF32 : kBarF64;
    fit.limF = 0.5 * bar / kFitCoulomb;
    fit.limD = 0.5 * bar / (6.0 * kRefC6);
    fit.limE = kErfcAbsErr / cutoff;
    if (fit.pairF <= fit.limF) fit.use |= kPolyForce;
    if (fit.sysE <= fit.limE) fit.use |= kPolyEnergy;
    if (disp && fit.pairD <= fit.limD) fit.use |= kPolyDispersion;
    return fit;
}

}  // namespace snb
