// pme_plan.h -- the host-side planner of the reciprocal path: which kernel runs for a mesh, with how much LDS, how many threads and how
// many work-groups.  Pure functions of integers, the element size (4: single and mixed precision, 8: double) and the switches; no HIP.
// engine.hip sizes buffers and prints the SNB_VERBOSE mesh line from them, the launchers of pme.hip take their geometry from them (same
// functions, same inputs: every decision is written once), tests/pme_plan_check.cpp runs them on the CPU for the mesh census.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>

#include "switches.h"

#if defined(__HIPCC__)
#define SNB_PLAN_HD __host__ __device__
#else
#define SNB_PLAN_HD
#endif

namespace snb {

struct PmePlanDims {
    int nx, ny, nz, nzc;      // nzc = nz/2+1
    int nfx, nfy, nfz;        // number of radix factors per axis
    int fx[16], fy[16], fz[16];
    int rx1, rx2, ry1, ry2, rz1, rz2;   // two-pass register-FFT split n = r1*r2 per axis (0 = use the staged Stockham path)
    int px1, px2, py1, py2;             // plane path (pme.hip k_planeXY): splits of the x and y axes into radices it has pass bodies for (0 = none)
};

// ---- the instantiated (R1, R2) pairs ----------------------------------------------------------------------------------------------------
#ifndef SNB_FFT_120
// the split of a 120-point line, measured on c3 (round 3, A/B through SNB_LIB_PATH): 8 x 15 (rounds 1-2) x kernel 53.2 us, inverse z 16.3,
// merge + forward z 29.8, y pass 21.3; 10 x 12: 49.7 / 14.8 / 28.2 / 21.6 (the 15-point pass has only nb x 8 tasks for a work-group's 512
// threads and the most registers); 12 x 10: y pass 28.1; 15 x 8: x kernel 85.4
#define SNB_FFT_120(X) X(10, 12)
#endif
// The kernels are instantiated per (R1, R2) pair (inlining every radix into one runtime switch made them allocate 248 VGPRs);
// sizes outside this list use the staged Stockham path (R1 = 0).
#define SNB_FFT_PAIRS(X) X(6, 7) X(6, 9) X(8, 8) X(8, 10) X(9, 10) X(8, 12) X(10, 10) X(9, 12) SNB_FFT_120(X) X(8, 16) X(12, 12) X(10, 16) X(12, 15) X(12, 16) X(15, 16) X(16, 16)
// Plane path (k_planeXY + k_fftZInvMix): single precision, a square mesh plane that fits LDS with its row padding, an instantiated
// two-pass split, at most 8 held subsets, and the own-atoms spreader's merge kernel in front (it writes the plane-major spectrum).
#define SNB_PLANE_PAIRS(X) X(6, 7) X(6, 9) X(8, 8) X(8, 10) X(9, 10) X(8, 12) X(10, 10) X(9, 12) X(10, 12) X(8, 16)
// the radices the run-time plane kernel has pass bodies for
#define SNB_PLANE_RADICES(X) X(5) X(6) X(7) X(8) X(9) X(10) X(12) X(15) X(16)

inline bool factorize(int n, int* factors, int* nf) {
    int k = 0;
    while (n % 4 == 0) { factors[k++] = 4; n /= 4; }
    while (n % 2 == 0) { factors[k++] = 2; n /= 2; }
    while (n % 3 == 0) { factors[k++] = 3; n /= 3; }
    while (n % 5 == 0) { factors[k++] = 5; n /= 5; }
    while (n % 7 == 0) { factors[k++] = 7; n /= 7; }
    while (n % 11 == 0) { factors[k++] = 11; n /= 11; }      // 11 and 13: the reference's GPU FFT is legal up to 13-smooth sizes
    while (n % 13 == 0) { factors[k++] = 13; n /= 13; }      // (platforms/common/include/FFT3DFactory.h:45-47)
    *nf = k;
    return n == 1 && k <= 16;
}

// plane path: n = r1 * r2 with both factors among the radices k_planeXY has pass bodies for, r1 <= r2, the most balanced pair; the
// pairs with a kernel of their own (SNB_PLANE_PAIRS) first
inline bool splitPlane(int n, int* r1, int* r2) {
#define X(A, B) if (n == (A) * (B)) { *r1 = A; *r2 = B; return true; }
    SNB_PLANE_PAIRS(X)
#undef X
    const int radices[] = {
#define X(A) A,
        SNB_PLANE_RADICES(X)
#undef X
    };
    int best = 0;
    for (int a : radices) for (int b : radices) if (a <= b && a * b == n && a > best) { best = a; *r1 = a; *r2 = b; }
    if (best) return true;
    *r1 = *r2 = 0;
    return false;
}

// n = r1 * r2 for one of the instantiated (R1, R2) pairs; false (and 0, 0) if n is not in the list
inline bool splitTwoPass(int n, int* r1, int* r2) {
#define X(A, B) if (n == (A) * (B)) { *r1 = A; *r2 = B; return true; }
    SNB_FFT_PAIRS(X)
#undef X
    *r1 = *r2 = 0;
    return false;
}
inline bool isFftPair(int r1, int r2) {
#define X(A, B) if (r1 == A && r2 == B) return true;
    SNB_FFT_PAIRS(X)
#undef X
    return false;
}

inline int legalGridSize(int n) {
    if (n < 6) n = 6;
    for (;; n++) {
        int f[32], nf, m = n;
        for (int p : {2, 3, 5, 7, 11, 13}) while (m % p == 0) m /= p;
        if (m == 1 && factorize(n, f, &nf)) return n;
    }
}

// square plane with a split that has a kernel of its own (static splits: no calls, one table of roots); everything else takes the run-time kernel
inline bool planeSquare(const PmePlanDims& d, const Switches& sw) {
    if (sw.planeDynamic || d.nx != d.ny || d.px1 != d.py1 || d.px2 != d.py2) return false;
#define X(A, B) if (d.px1 == A && d.px2 == B) return true;
    SNB_PLANE_PAIRS(X)
#undef X
    return false;
}
inline bool planeIsStatic(const PmePlanDims& d) { return planeSquare(d, switches()); }

// Sizes, radix factors and splits of a mesh of g[0] x g[1] x g[2] points; false: a size is not FFT-legal
inline bool planDims(const int g[3], size_t realBytes, const Switches& sw, PmePlanDims& d) {
    d.nx = g[0]; d.ny = g[1]; d.nz = g[2]; d.nzc = g[2] / 2 + 1;
    if (!factorize(d.nx, d.fx, &d.nfx) || !factorize(d.ny, d.fy, &d.nfy) || !factorize(d.nz, d.fz, &d.nfz)) return false;
    splitTwoPass(d.nx, &d.rx1, &d.rx2); splitTwoPass(d.ny, &d.ry1, &d.ry2); splitTwoPass(d.nz, &d.rz1, &d.rz2);
    splitPlane(d.nx, &d.px1, &d.px2); splitPlane(d.ny, &d.py1, &d.py2);
    // measured on MI355X (120^3 = 8 x 15, 4 grids, single precision, Winograd radix-3/5 butterflies): two-pass register FFT vs
    // staged Stockham: inverse z 18.2 vs 23.5 us, y 30.6 vs 32.4, fused x/convolution 68.6 vs 71.0.  SNB_FFT_TWOPASS=0/1 overrides.
    // Round 3, double precision (c5, 180^3 = 12 x 15 and 90^3 = 9 x 10): the register passes win on the y and z axes (y 183 -> 150 us,
    // inverse z 185 -> 134, 90^3: 32 -> 22 and 21 -> 14) and in the fused x kernel of the 90^3 mesh (63 -> 42), but the x kernel of the
    // 180^3 mesh, which also holds the spectra of all subsets, spills with 15-point transforms in double (351 -> 488): staged there.
    if (!sw.fftTwoPass) d.rx1 = d.ry1 = d.rz1 = d.rx2 = d.ry2 = d.rz2 = 0;
    // (round 4: the fused x kernel runs 15- / 16-point transforms in double with 256 threads and 256 registers; SNB_CONVX_STAGED_F64=1 restores the staged form)
    if (realBytes == 8 && std::max(d.rx1, d.rx2) > 12 && sw.convxStagedF64) d.rx1 = d.rx2 = 0;
    return true;
}

// ---- the box ------------------------------------------------------------------------------------------------------------------------------
// rows of the reciprocal box (fractional = r * position) of a lower-triangular box
inline void recipBoxRows(const double box[9], double r[9]) {
    const double sc = 1.0 / (box[0] * box[4] * box[8]);
    const double rows[9] = {box[4] * box[8] * sc, 0, 0, -box[3] * box[8] * sc, box[0] * box[8] * sc, 0,
                            (box[3] * box[7] - box[4] * box[6]) * sc, -box[0] * box[7] * sc, box[0] * box[4] * sc};
    std::copy(rows, rows + 9, r);
}

// ---- bricks -------------------------------------------------------------------------------------------------------------------------------
// brick kernels: the sort columns were cut for the Coulomb mesh; any mesh whose cells tile those columns can use them, with bricks of
// `group` columns when one column is narrower than 5 cells (stencil 4 + 1 cell of drift).
struct BrickGeometry {
    bool ok = false;
    int ncx = 0, ncy = 0;      // sort columns
    int gx = 0, gy = 0;        // columns per brick side
    int cx = 0, cy = 0;        // mesh cells per brick side
    int count() const { return (ncx / gx) * (ncy / gy); }      // bricks per subset
};
inline BrickGeometry bricksOf(const PmePlanDims& d, int ncx, int ncy, int gx, int gy) {
    BrickGeometry b;
    b.ok = true; b.ncx = ncx; b.ncy = ncy; b.gx = gx; b.gy = gy; b.cx = gx * (d.nx / ncx); b.cy = gy * (d.ny / ncy);
    return b;
}
// do this mesh's cells tile the sort columns (cut for the Coulomb mesh, colCells cells wide)?
inline BrickGeometry brickGeometry(const PmePlanDims& d, const PmePlanDims& coulomb, const int colCells[2], int brickGroup) {
    if (colCells[0] <= 0) return BrickGeometry();
    const int ncx = coulomb.nx / colCells[0], ncy = coulomb.ny / colCells[1];
    auto group = [brickGroup](int n, int ncols) { if (n % ncols) return 0; const int cpc = n / ncols; for (int g = brickGroup; g <= 4; g++) if (g * cpc >= 5 && ncols % g == 0) return g; return 0; };
    const int gx = group(d.nx, ncx), gy = group(d.ny, ncy);
    const bool packable = d.nx < 1024 && d.ny < 1024 && d.nz < 1024;   // k_pmeCells packs 10 bits per axis
    if (!packable || gx <= 0 || gy <= 0) return BrickGeometry();
    BrickGeometry b = bricksOf(d, ncx, ncy, gx, gy);
    b.ok = sizeof(double) * (size_t)b.cx * b.cy * d.nz <= 100 * 1024;
    return b;
}

// ---- plane path ---------------------------------------------------------------------------------------------------------------------------
// y lines per work-group of the inverse z kernel = tile of the convolved planes' layout (c4, 8 subsets: plane + z kernel 45.5 + 55.0 us with 8, 61.2 + 42.4 with 4: 32-byte runs in the plane kernel's store)
inline int planeTileY(const Switches& sw) { return (sw.zmixNby == 2 || sw.zmixNby == 4 || sw.zmixNby == 8) ? sw.zmixNby : 8; }
struct PlanePath {
    size_t lds;          // k_planeXY: the plane with its row padding, a table of nx roots, and ny more for the run-time splits
    bool buffers;        // PmePlan::init keeps a second complex mesh and the kernel-value table: single precision, a bare plane within LDS
    bool ok;             // what sizes and switches decide of planePathOK (pme.hip adds: the buffers exist)
    int threads;         // of a forces step: 1024, or SNB_PLANE_NT = 768 on a static split (energy-only steps: always 1024)
};
inline PlanePath planePath(const PmePlanDims& d, int nsub, size_t realBytes, const Switches& sw) {
    PlanePath q;
    const bool square = planeSquare(d, sw);
    q.lds = 2 * realBytes * ((size_t)d.nx * (d.ny | 1) + d.nx + (square ? 0 : d.ny));
    q.buffers = realBytes == 4 && (size_t)d.nx * (d.ny | 1) * 8 <= 156 * 1024;      // (planes that fit LDS; y padded to whole tiles of the inverse z kernel)
    q.ok = !sw.noPlaneFft && realBytes == 4 && !(d.ny & 1) && d.px1 > 0 && d.py1 > 0 && d.px1 * d.px2 == d.nx && d.py1 * d.py2 == d.ny
           && nsub <= 8 && q.lds <= 156 * 1024 && (square || !sw.noRectPlanes);
    q.threads = (square && sw.planeNt == 768) ? 768 : 1024;
    return q;
}

// inverse z pass of the plane path (k_fftZInvMix): NBY y lines of every subset pair per work-group
struct ZMix { int NBY; size_t lds; int threads; };
inline ZMix zMix(const PmePlanDims& d, int nsub, const Switches& sw) {
    ZMix z;
    const int NP = (nsub + 1) / 2;
    z.NBY = planeTileY(sw);
    const bool twoPass = isFftPair(d.rz1, d.rz2);
    z.lds = 8 * ((size_t)(twoPass ? 1 : 2) * d.nz * (z.NBY * NP + 1) + d.nz);      // (in place with a two-pass split)
    const bool wide = sw.zmixNt ? sw.zmixNt == 512 : z.NBY * NP >= 24;      // 24+ complex transforms per work-group (5-8 subsets): 512 threads
    z.threads = (wide && twoPass) ? 512 : 256;      // (the staged form exists at 256 threads only)
    return z;
}

// ---- own-atoms spreader: k_spreadOwn over (brick, slab) work-groups, then k_spreadMerge per brick --------------------------------------------
// LDS stride of a z line in k_spreadOwn's region: a stride that is a multiple of 64 dwords puts every line on the same banks (RZ = 64 for
// sz = 60: lanes = z-neighbours of one column then collide ~13-way: 47.7 us on c3 against 27.8); a few extra values per line spread them
template <bool FIXED> SNB_PLAN_HD inline int ownLineStride(int RZ) {
    const int per = FIXED ? 4 : 2;                                  // values per 16 bytes: lines stay 16-byte aligned for the vector copy
    int st = (RZ + per - 1) / per * per;
    while (((st * (FIXED ? 1 : 2)) & 7) != 4) st += per;            // stride = 4 (mod 8) dwords: consecutive lines walk over all 64 banks
    return st;
}
// Margin: the cells an atom can drift across its column's border during a list's life (skin / 2), at least one.  r: recipBoxRows
inline int ownSpreadMargin(const PmePlanDims& d, const double r[9], double padding, const Switches& sw) {
    const double perNmX = d.nx * std::sqrt(r[0] * r[0] + r[3] * r[3] + r[6] * r[6]), perNmY = d.ny * std::sqrt(r[1] * r[1] + r[4] * r[4] + r[7] * r[7]);      // mesh cells per nm of displacement
    const int M = std::max(1, (int)std::ceil(0.5 * std::max(padding, 0.0) * std::max(perNmX, perNmY) + 0.01));
    return sw.spreadMargin >= 0 ? sw.spreadMargin : M;
}
struct OwnSpread {
    int slabs = 0;             // z slabs per brick the engine plans and sizes ownPartial for (0: none; the SNB_VERBOSE mesh line prints this)
    bool runs = false;         // ... and the launch runs it: its region fits LDS with the line stride, the merge kernel reaches every brick
    bool fixed = false; size_t accBytes = 8;      // 32-bit fixed-point accumulation (single precision), else doubles
    int RX = 0, RY = 0, RZ = 0;                   // a work-group's region: the brick slab, the stencil's reach and the margin
    size_t regions = 0, partialBytes = 0;         // of ownPartial: [regions][RX * RY * RZ] accumulators
    size_t ldsOwn = 0;
    int chunk = 1;             // values per load of the merge kernel (16, 8 or 4 bytes)
    int mergeThreads = 256;
    size_t ldsFft = 0; bool fuse = false;         // the merge kernel also does the forward z FFT
    bool plane = false;        // ... and writes the spectrum plane-major for k_planeXY (sizes and switches: planePath().ok)
};
// Slabs: the fewest that bring a work-group's LDS region under 40 KB (four work-groups per CU), at least two.
inline OwnSpread ownSpread(const PmePlanDims& d, const BrickGeometry& b, int nsub, size_t realBytes, int M, const Switches& sw) {
    OwnSpread o;
    o.fixed = realBytes == 4 && !sw.noFixedSpread;
    o.accBytes = o.fixed ? 4 : 8;
    const int cx = b.cx, cy = b.cy, nz = d.nz;
    const int RX = o.RX = cx + 4 + 2 * M, RY = o.RY = cy + 4 + 2 * M;
    if (RX > d.nx || RY > d.ny || b.gx * b.gy > 16 || nz > 256) return o;      // (nz > 256: one slab's region of nz + 4 planes would wrap onto itself)
    int best = 0;
    const int forced = sw.ownSlabs;
    for (int pass = 0; pass < 2 && !best; pass++)
        for (int k = 2; k <= 32; k++) {      // (at least two: a single slab's region, nz + 4 planes, would wrap onto itself)
            if (forced > 0 && k != forced) continue;
            if (nz % k) continue;
            const int sz = nz / k;
            if (sz < 4 || (sz & 1)) continue;      // (8- or 16-byte copies of the regions)
            if (o.accBytes * (size_t)RX * RY * (sz + 4) <= (size_t)(pass == 0 ? 40 : 64) * 1024) { best = k; break; }
        }
    if (!best) return o;
    // few, wide bricks (coarse mesh, 2 x 2 columns per brick): more slabs until a grid has ~400 work-groups (c3l's 60^3 dispersion mesh: 100 bricks)
    if (forced <= 0) for (int k = best + 1; k <= 16 && b.count() * best < 400; k++) if (nz % k == 0 && (nz / k) >= 8 && !((nz / k) & 1)) best = k;
    o.slabs = best;
    const int sz = nz / best, RZ = o.RZ = sz + 4;
    o.regions = (size_t)nsub * b.count() * best;
    o.partialBytes = o.regions * RX * RY * RZ * o.accBytes;
    // what can still decline it at the launch
    o.ldsOwn = o.accBytes * (size_t)RX * RY * (o.fixed ? ownLineStride<true>(RZ) : ownLineStride<false>(RZ));
    const int reachX = (4 + M + cx - 1) / cx + (M + cx - 1) / cx + 1, reachY = (4 + M + cy - 1) / cy + (M + cy - 1) / cy + 1;      // bricks whose regions cover a line
    o.runs = !sw.noOwnSpread && o.ldsOwn <= 64 * 1024 && reachX <= 3 && reachY <= 3
             && o.regions * RX * RY * RZ < ((size_t)1 << 31);      // (the merge kernel keeps 32-bit element offsets into ownPartial)
    const int cmax = o.fixed ? 4 : 2;
    o.chunk = (sz % cmax == 0) ? cmax : ((o.fixed && sz % 2 == 0) ? 2 : 1);
    // a long mesh in double precision gives a 256-thread work-group a dozen 16-byte chunks per thread, each three rounds of dependent loads
    // (c5, 180^3: 309 us): 512 threads there
    o.mergeThreads = (sw.mergeNt ? sw.mergeNt == 512 : (size_t)cx * cy * (nz / o.chunk) > 6 * 256) ? 512 : 256;
    const int nb = (cx * cy + 1) / 2;
    o.ldsFft = 2 * realBytes * ((size_t)2 * nz * (nb + 1) + nz);
    o.fuse = !sw.noFusedZ && o.ldsFft <= 120 * 1024;
    o.plane = o.fuse && planePath(d, nsub, realBytes, sw).ok;
    return o;
}

// ---- scanning brick spreader (k_spreadBrick) ----------------------------------------------------------------------------------------------
struct BrickSpread { bool fixed; size_t lds; bool fuse; int blocks; };
inline BrickSpread brickSpread(const PmePlanDims& d, const BrickGeometry& b, int nsub, size_t realBytes, int zSlabs, const Switches& sw) {
    BrickSpread q;
    q.fixed = realBytes == 4 && !sw.noFixedSpread && d.nz % 2 == 0 && (d.nz / zSlabs) % 2 == 0;
    const size_t accBytes = q.fixed ? sizeof(int) : sizeof(double);
    const size_t brickBytes = (accBytes * (size_t)b.cx * b.cy * (d.nz / zSlabs) + 15) & ~(size_t)15;
    const size_t listBytes = sizeof(int) * (q.fixed ? 8192 : 4096);
    const int nbz = (b.cx * b.cy + 1) / 2;
    const size_t fftBytes = 2 * realBytes * ((size_t)2 * d.nz * (nbz + 1) + d.nz);
    q.fuse = !sw.noFusedZ && zSlabs == 1 && brickBytes + std::max(listBytes, fftBytes) <= 64 * 1024;
    q.lds = brickBytes + (q.fuse ? std::max(listBytes, fftBytes) : listBytes);
    q.blocks = nsub * b.count() * zSlabs;
    return q;
}

// ---- three-pass FFT -------------------------------------------------------------------------------------------------------------------------
inline int pickBatch(size_t bytesPerBatchElem, int maxB, int minB = 1) {
    int b = (int)((size_t)96 * 1024 / bytesPerBatchElem);      // the LDS budget of a line batch
    if (b > maxB) b = maxB;
    if (b < minB) b = minB;
    return b;
}
// z axis (k_fftZ), forward and inverse: one work-group transforms NL contiguous real lines, two per complex FFT
struct ZPass { int NL; size_t lds; };
inline ZPass zPass(int nz, size_t realBytes) {
    const size_t cx = 2 * realBytes;
    int NC = pickBatch((size_t)2 * nz * cx, 17) - 1;   // complex lines per work-group (two real lines each)
    NC &= ~1;
    if (NC < 2) NC = 2;
    return {2 * NC, (size_t)2 * nz * (NC + 1) * cx + (size_t)nz * cx};
}
// a strided axis (k_fftStrided): tiles of NB adjacent lines out of `lines`
struct StridedPass { int NB; size_t lds; int tilesPerA; };
inline StridedPass stridedPass(int n, int lines, size_t realBytes, int NB) { return {NB, ((size_t)2 * n * NB + n) * 2 * realBytes, (lines + NB - 1) / NB}; }
// Columns per work-group of the y pass.  Single precision: as many as fit the LDS budget, at most 32 (c3: 32 + 29 columns 27.8 us, three
// tiles of 21 28.4).  Double precision (round 3): at least three tiles of even width -- 90^3 (46 columns) 16 + 16 + 14: 16.5 / 14.9 us per
// pass against 21.5 / 20.6 for 32 + 14; 180^3 six tiles of 16: 139 / 128 against 145 / 133 for 17 x 5 + 6; 120^3 keeps three tiles
// (four tiles of 16: 48.6 against 40.8)
inline int fftyBatch(int ny, int nzc, size_t realBytes, int forced) {
    const int cap = pickBatch((size_t)2 * ny * 2 * realBytes, forced > 0 ? forced : 32);
    if (forced > 0 || realBytes == 4) return cap;
    const int tiles = (nzc + cap - 1) / cap;
    if (tiles < 3 && nzc >= 24) return (nzc + 2) / 3;
    return cap > 2 ? (cap & ~1) : cap;      // (balanced tiles of 21 on the 120^3 mesh: 42.6 us against 40.8 for 25 + 25 + 11)
}
inline StridedPass yPass(const PmePlanDims& d, size_t realBytes, const Switches& sw) { return stridedPass(d.ny, d.nzc, realBytes, fftyBatch(d.ny, d.nzc, realBytes, sw.fftyNb)); }
// threads of the fused x kernel: k_convolveX<double, A, B> with a 15- or 16-point pass is instantiated at 256 threads (and 256 registers) only
constexpr int convxThreads(int r1, int r2, size_t realBytes) { return (realBytes == 8 && (r1 > 12 || r2 > 12)) ? 256 : 512; }

// ---- interpolation (k_interpolateBricks) ------------------------------------------------------------------------------------------------------
// The kernel needs ~100 VGPRs, so one 1024-thread work-group occupies a CU: with more bricks than CUs the launch runs in rounds.
// Wider bricks (2 x 1, 2 x 2 columns) cut the count below the CU count and the halo overhead with it, as long as LDS allows.
inline BrickGeometry interpWiden(const PmePlanDims& d, BrickGeometry q, int nsubTotal, size_t realBytes, const Switches& sw) {
    const int gEnv = sw.interpGroup;
    // (measured on c3, 400 single-column bricks: 1024 threads on 2 x 1-column bricks 35.2 us, 1024 threads on single columns 39.3,
    // 512 threads on single columns -- two work-groups per CU -- 29.1: when the single-column brick fits LDS twice, do not widen)
    auto need = [&](const BrickGeometry& b) { return realBytes * (size_t)(b.cx + 6) * (b.cy + 6) * (d.nz + 4) + 1024; };
    const size_t single = need(q);
    for (int step = 0; step < 2; step++) {
        if (gEnv >= 0 ? step >= gEnv : (q.count() <= 256 || single <= 76 * 1024)) break;
        int gx = q.gx, gy = q.gy;
        if (step == 0 && q.ncx % (2 * gx) == 0) gx *= 2; else if (q.ncy % (2 * gy) == 0) gy *= 2; else break;
        const BrickGeometry t = bricksOf(d, q.ncx, q.ncy, gx, gy);
        if (need(t) > 150 * 1024 || nsubTotal * gx * gy > 256) break;
        q = t;
    }
    return q;
}
struct InterpBricks {
    bool bricks;         // false: the 32-lanes-per-atom kernel k_interpolate
    int zSlabs; size_t lds; int blocks, threads;
};
inline InterpBricks interpBricks(const PmePlanDims& d, const BrickGeometry& b, int nsubTotal, size_t realBytes, const Switches& sw) {
    InterpBricks q;
    const int zsEnv = sw.interpZSlabs;
    int zSlabs = 1;      // measured on c3: 1 slab 52 us, 2 slabs 70, 4 slabs 72 (every slab rescans the columns' atoms)
    if (zsEnv > 0 && d.nz % zsEnv == 0 && d.nz / zsEnv >= 8) zSlabs = zsEnv;
    auto ldsFor = [&](int slabs) { return ((realBytes * (size_t)(b.cx + 6) * (b.cy + 6) * (d.nz / slabs + 4) + 15) & ~(size_t)15) + sizeof(double) * nsubTotal * (nsubTotal + 1); };
    // a brick that does not fit LDS in one piece (double precision on a large mesh: 12 x 12 x 184 doubles = 212 KB for the 180^3 mesh of
    // c5) is cut into the fewest z slabs that do, rather than falling back to the 32-lanes-per-atom gather kernel (424 us there)
    if (zsEnv <= 0) for (int k = 2; k <= 8 && ldsFor(zSlabs) > 150 * 1024; k++) if (d.nz % k == 0 && d.nz / k >= 8) zSlabs = k;
    // few, wide bricks (a coarse mesh whose bricks span 2 x 2 sort columns: the 60^3 dispersion mesh of c3l has 100 of them, 3000 atoms
    // each, on 256 CUs: 58.8 us against 26.6 for the 120^3 Coulomb mesh): slabs buy work-groups; every slab rescans the bricks' atoms,
    // which is why the fine mesh (400 bricks) does not take them
    if (zsEnv <= 0 && zSlabs == 1) for (int k = 2; k <= 6 && b.count() * zSlabs < 192; k++) if (d.nz % k == 0 && d.nz / k >= 10) zSlabs = k;
    q.zSlabs = zSlabs;
    q.lds = ldsFor(zSlabs);
    q.bricks = q.lds <= 150 * 1024 && !sw.noInterpBricks && nsubTotal * b.gx * b.gy <= 256;
    q.blocks = b.count() * zSlabs;
    // 512-thread work-groups go two to a CU when the brick fits LDS twice (the kernel's ~100 VGPRs allow 16 waves per CU either way):
    // with more bricks than CUs the second round of 1024-thread groups runs half empty
    q.threads = (sw.interpThreads ? sw.interpThreads == 512 : (q.blocks > 256 && q.lds <= 76 * 1024)) ? 512 : 1024;
    return q;
}

}  // namespace snb
