// Stand-alone driver of the Ewald polynomial fit (csrc/ewald_fit.h) for tests/test_ewald_fit_cpu.py.  No GPU, no HIP; built with ASan + UBSan.
//
//   ewald_fit_check alpha alpha_d cutoff padding method precision      (method: snb_method; precision: 0 single / mixed, 1 double)
//
// prints one "name value ..." line per item:
//   coefF / coefE / coefD   the monomial coefficients the engine uploads (%.17g), use, degF
//   errF errE errD pairF sysE pairD   the residuals the header reports, limF limE limD the guard's limits
//   indep_errF ... indep_pairD        the same six residuals from this file's own evaluation: the exact functions in long double
//                                     (erfl, expl) at kIndepRadii radii in [0.05, cutoff], the polynomials by this file's own Horner loop
#include "ewald_fit.h"

#include <cstdio>
#include <cstdlib>

static const int kIndepRadii = 4001;
static const long double kSqrtPi = 1.77245385090551602729816748334L;

static long double exactBt(long double a, long double r) { const long double z = a * r; return (erfl(z) - 2.0L * z / kSqrtPi * expl(-z * z)) / (r * r * r); }
static long double exactEt(long double a, long double r) { return erfl(a * r) / r; }
static long double exactGd(long double ad, long double r) {      // [1 - e^{-x} (1 + x + x^2/2 + x^3/6)] / r^8 (direct.hip: the fexp form is 6 c6 r^2 times this)
    const long double x = ad * ad * r * r;
    if (x < 0.5L) {      // the bracket cancels: x^4 e^{-x} sum_k x^k / (k+4)!
        long double sum = 0, term = 1.0L / 24.0L;
        for (int k = 0; k < 40; k++) { sum += term; term *= x / (k + 5); }
        return powl(ad, 8.0L) * expl(-x) * sum;
    }
    return (1.0L - expl(-x) * (1.0L + x + x * x / 2.0L + x * x * x / 6.0L)) / powl(r, 8.0L);
}
// float coefficients, float t and float FMA Horner, as the single-precision kernels
static long double hornerF32(const double* c, int deg, double r2max, long double r2) {
    const float scale = (float)(2.0 / r2max), t = fmaf((float)r2, scale, -1.0f);
    float v = (float)c[deg];
    for (int k = deg - 1; k >= 0; k--) v = fmaf(v, t, (float)c[k]);
    return v;
}
static long double hornerF64(const double* c, int deg, double r2max, long double r2) {
    const double scale = 2.0 / r2max, t = fma((double)r2, scale, -1.0);
    double v = c[deg];
    for (int k = deg - 1; k >= 0; k--) v = fma(v, t, c[k]);
    return v;
}
// the float coefficients, everything else exact
static long double hornerExact(const double* c, int deg, double r2max, long double r2) {
    const long double t = r2 * (2.0L / (long double)r2max) - 1.0L;
    long double v = (float)c[deg];
    for (int k = deg - 1; k >= 0; k--) v = v * t + (long double)(float)c[k];
    return v;
}

static void printCoef(const char* name, const double* c, int n) {
    printf("%s", name);
    for (int i = 0; i < n; i++) printf(" %.17g", c[i]);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: %s alpha alpha_d cutoff padding method precision\n", argv[0]); return 2; }
    const double alpha = atof(argv[1]), alphaD = atof(argv[2]), cutoff = atof(argv[3]), padding = atof(argv[4]);
    const int method = atoi(argv[5]), precision = atoi(argv[6]);
    if (!(alpha > 0) || !(cutoff > 0) || padding < 0 || (precision != 0 && precision != 1)) { fprintf(stderr, "bad arguments\n"); return 2; }
    const double rmax = cutoff + padding + 0.02;      // (Engine::buildEwaldPoly)
    const snb::EwaldFit fit = precision == 0 ? snb::fitEwaldPolys<float>(alpha, alphaD, cutoff, rmax, method) : snb::fitEwaldPolys<double>(alpha, alphaD, cutoff, rmax, method);
    printCoef("coefF", fit.ewPoly, fit.degF + 1); printCoef("coefE", fit.ewPolyE, 14); printCoef("coefD", fit.dispPoly, snb::kDispDegF64 + 1);
    printf("degF %d\nuse %d\nr2max %.17g\n", fit.degF, fit.use, fit.r2max);
    printf("errF %.17g\nerrE %.17g\nerrD %.17g\npairF %.17g\nsysE %.17g\npairD %.17g\n", fit.errF, fit.errE, fit.errD, fit.pairF, fit.sysE, fit.pairD);
    printf("limF %.17g\nlimE %.17g\nlimD %.17g\n", fit.limF, fit.limE, fit.limD);

    const bool disp = method == snb::kEwaldFitLJPME;
    long double errF = 0, errE = 0, errD = 0, pairF = 0, sysE = 0, pairD = 0;
    for (int i = 0; i < kIndepRadii; i++) {
        const long double r = 0.05L + ((long double)cutoff - 0.05L) * i / (kIndepRadii - 1), r2 = r * r;
        const long double pF = precision == 0 ? hornerF32(fit.ewPoly, fit.degF, fit.r2max, r2) : hornerF64(fit.ewPoly, fit.degF, fit.r2max, r2);
        const long double dF = fabsl(pF - exactBt(alpha, r));
        errF = std::max(errF, dF); pairF = std::max(pairF, r * dF);
        errE = std::max(errE, fabsl(hornerF32(fit.ewPolyE, snb::kEwDegE, fit.r2max, r2) - exactEt(alpha, r)));
        sysE = std::max(sysE, fabsl(hornerExact(fit.ewPolyE, snb::kEwDegE, fit.r2max, r2) - exactEt(alpha, r)));
        if (disp) { const long double dD = fabsl(hornerF64(fit.dispPoly, snb::kDispDegF64, fit.r2max, r2) - exactGd(alphaD, r)); errD = std::max(errD, dD); pairD = std::max(pairD, r * dD); }
    }
    printf("indep_errF %.17Lg\nindep_errE %.17Lg\nindep_errD %.17Lg\nindep_pairF %.17Lg\nindep_sysE %.17Lg\nindep_pairD %.17Lg\n", errF, errE, errD, pairF, sysE, pairD);
    return 0;
}
