// CPU driver of csrc/pme_sizes.h (tests/test_subset_census.py builds it with g++ under ASan + UBSan and runs it; no GPU, nothing loaded
// into python).  It sweeps nx in 20 .. 260, 1 .. 64 subsets, both arithmetics and the budgets the tests use, and holds the header against
// the kernel's own carve-up of its dynamic LDS (pme.hip k_convolveX: two buffers [nx][nsub][NB] of complex values, nx roots of unity, a
// line [nx][NB] of the reciprocal-space kernel), written out here with std::complex.  Then it prints, for the mesh lines the subset-count
// census runs, the columns per work-group and the request: "row <nx> <nsub> <realBytes> <budgetKB> <NB> <total>".
#include <complex>
#include <cstdio>
#include <cstdlib>

#include "pme_sizes.h"

using namespace snb;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "FAILED %s: ", #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

template <typename Real> static size_t kernelBytes(int nx, int nsub, int NB) {
    const size_t A = (size_t)nx * nsub * NB * sizeof(std::complex<Real>);      // A, and B behind it
    return 2 * A + (size_t)nx * sizeof(std::complex<Real>) + (size_t)nx * NB * sizeof(Real);
}

static size_t staticBytes() { return (512 / 64) * 4 * sizeof(double); }      // s_red of k_convolveX at 512 threads (half of it at 256)

template <typename Real> static void sweep(size_t deviceLimit) {
    const int budgets[3] = {16, 32, 72};
    for (int nx = 20; nx <= 260; nx++)
        for (int nsub = 1; nsub <= 64; nsub++) {
            const bool accepted = convLdsFits(nx, nsub, sizeof(Real), deviceLimit);
            CHECK(accepted == (kernelBytes<Real>(nx, nsub, 1) + staticBytes() <= deviceLimit), "nx %d nsub %d", nx, nsub);
            for (int b = 0; b < 3; b++) {
                const ConvLds c = convLds(nx, nsub, sizeof(Real), budgets[b]);
                CHECK(c.NB == 1 || c.NB == 2 || c.NB == 4 || c.NB == 8, "nx %d nsub %d budget %d: NB %d", nx, nsub, budgets[b], c.NB);
                CHECK(c.total == kernelBytes<Real>(nx, nsub, c.NB), "nx %d nsub %d budget %d: %zu against %zu", nx, nsub, budgets[b], c.total, kernelBytes<Real>(nx, nsub, c.NB));
                CHECK(c.perCol * c.NB + (size_t)nx * sizeof(std::complex<Real>) == c.total, "nx %d nsub %d", nx, nsub);
                // the largest of 8, 4, 2, 1 whose columns fit the budget; 1 when none does
                CHECK(c.NB == 1 || c.perCol * c.NB <= (size_t)budgets[b] * 1024, "nx %d nsub %d budget %d", nx, nsub, budgets[b]);
                CHECK(c.NB == 8 || c.perCol * 2 * c.NB > (size_t)budgets[b] * 1024, "nx %d nsub %d budget %d", nx, nsub, budgets[b]);
                // what is launched fits the device, beside the kernel's static LDS, exactly when the guard accepts (every budget here, with the roots of unity, is below the limit)
                CHECK((c.total + staticBytes() <= deviceLimit) == accepted, "nx %d nsub %d budget %d: request %zu, limit %zu, accepted %d", nx, nsub, budgets[b], c.total, deviceLimit, (int)accepted);
            }
        }
}

static int firstRefused(int nx, size_t realBytes, size_t limit) {
    int n = 1;
    while (convLdsFits(nx, n, realBytes, limit)) n++;
    return n;
}

int main() {
    const size_t limit = 160 * 1024;      // LDS of a gfx950 compute unit; the engine asks the device
    sweep<float>(limit);
    sweep<double>(limit);
    // double precision, one column per work-group: past 160 KB at 42 subsets on a 120 mesh, at 28 on a 180 mesh
    CHECK(firstRefused(120, 8, limit) == 42, "%d", firstRefused(120, 8, limit));
    CHECK(firstRefused(180, 8, limit) == 28, "%d", firstRefused(180, 8, limit));
    CHECK(!convLdsFits(180, 32, 8, limit) && convLdsFits(180, 32, 4, limit), "the engine the GPU test expects to be refused");
    CHECK(staticBytes() == kConvStaticLds && convLdsNeed(180, 32, 8) == 188896, "%zu", convLdsNeed(180, 32, 8));
    // a request that fits alone but not beside the static part: double precision, nx = 105, 48 subsets, 163 800 + 256 bytes
    CHECK(convLdsTotal(105, 48, 8, 1) == 163800 && !convLdsFits(105, 48, 8, limit) && convLdsFits(105, 47, 8, limit), "static LDS");
    // pair lists: 16 bytes per slice, at most 48 KB -- 77 subsets; the packed pair kernel's 16-bit slice is far above
    long long maxSub = 0;
    for (long long n = 1; n <= 400; n++) {
        const long long S = n * (n + 1) / 2;
        CHECK(pairListLds(S) == (size_t)(2 * S) * sizeof(double), "%lld", n);
        if (pairListLdsFits(S)) { CHECK(maxSub == n - 1, "not monotonic at %lld", n); maxSub = n; CHECK(S <= 65535, "%lld", S); }
    }
    CHECK(maxSub == 77, "%lld", maxSub);
    // the mesh lines of the census: Coulomb nx = 40, dispersion nx = 24, 3 .. 20 subsets, budgets 72 (default), 32, 16
    const int nxs[2] = {40, 24}, budgets[3] = {72, 32, 16};
    for (int m = 0; m < 2; m++)
        for (int nsub = 3; nsub <= 20; nsub++)
            for (size_t rb = 4; rb <= 8; rb += 4)
                for (int b = 0; b < 3; b++) {
                    const ConvLds c = convLds(nxs[m], nsub, rb, budgets[b]);
                    printf("row %d %d %zu %d %d %zu\n", nxs[m], nsub, rb, budgets[b], c.NB, c.total);
                }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("OK\n");
    return 0;
}
