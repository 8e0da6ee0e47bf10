// engine.hip -- host side of the MI355X SlicedNonbondedForce engine and its C ABI (include/snb.h).
//
// Functionally it stands where the reference has CommonCalcSlicedNonbondedForceKernel
// (platforms/common/src/CommonNonbondedSlicingKernels.cpp: commonInitialize :256-844, execute :846-1402,
// copyParametersToContext :1404-1568) plus the OpenMM utilities that class leans on (NonbondedUtilities'
// neighbour list and tile driver, BondedUtilities, ComputeSort) -- but none of its structure: there is no JIT, no
// ComputeContext; a handle owns plain HIP buffers and enqueues precompiled gfx950 kernels on one stream.
#include "../../include/snb.h"
#include "snb_internal.h"
#include "switches.h"
#include "host_lists.h"
#include "ewald_fit.h"
#include "pme_sizes.h"
#include "pair_addressing.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <numeric>
#include <set>
#include <thread>
#include <tuple>
#include <type_traits>

namespace snb {

static thread_local std::string g_createError;

// inside a spin wait
static inline void cpuRelax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#else
    std::this_thread::yield();
#endif
}

struct HipError { std::string msg; };
#define HIPCHECK(expr)                                                                                         \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) throw HipError{std::string(#expr) + ": " + hipGetErrorString(e_)};               \
    } while (0)

// runs f when the scope is left, by return or by exception: host state that a call borrows and must put back (f makes no HIP call)
template <typename F> struct ScopeExit {
    F f;
    explicit ScopeExit(F g) : f(std::move(g)) {}
    ScopeExit(const ScopeExit&) = delete;
    ~ScopeExit() { f(); }
};

template <typename T> struct DevBuf {
    T* p = nullptr; size_t n = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    void resize(size_t m) {
        if (m <= n && p) return;
        if (p) { (void)hipFree(p); p = nullptr; }
        n = m > 0 ? m : 1;
        HIPCHECK(hipMalloc((void**)&p, sizeof(T) * n));
    }
    void upload(const T* h, size_t count, hipStream_t s) { resize(count); if (count > 0) HIPCHECK(hipMemcpyAsync(p, h, sizeof(T) * count, hipMemcpyHostToDevice, s)); }
    void upload(const std::vector<T>& h, hipStream_t s) { upload(h.data(), h.size(), s); }
};
static_assert(sizeof(Int4) == sizeof(int4) && sizeof(Int2) == sizeof(int2), "host_lists.h names int4 / int2 without HIP; its records are uploaded as such");
inline void upload(DevBuf<int4>& d, const std::vector<Int4>& h, hipStream_t s) { d.upload(reinterpret_cast<const int4*>(h.data()), h.size(), s); }
inline void upload(DevBuf<int2>& d, const std::vector<Int2>& h, hipStream_t s) { d.upload(reinterpret_cast<const int2*>(h.data()), h.size(), s); }

// Small asynchronous host-to-device updates (lambdas, energy-slice mask, dispersion coefficients, global parameter values) go through a ring
// of pinned slots, one per in-flight update, each guarded by an event: the setter's own vector may be overwritten by the next call while an
// earlier copy is still queued, and a copy from pageable memory is either staged synchronously by the runtime or reads the source late
// (ADVICE r02).  A slot is reused only after its copy has completed; with 8 slots that wait never happens in practice.
struct PinnedRing {
    static constexpr int SLOTS = 8;
    struct Slot { void* p = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool pending = false; };
    Slot slots[SLOTS]; int next = 0;
    ~PinnedRing() { for (auto& s : slots) { if (s.ev) (void)hipEventDestroy(s.ev); if (s.p) (void)hipHostFree(s.p); } }
    void copy(void* dst, const void* src, size_t bytes, hipStream_t st) {
        if (bytes == 0) return;
        if (switches().noPinnedRing) { HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st)); HIPCHECK(hipStreamSynchronize(st)); return; }
        Slot& s = slots[next]; next = (next + 1) % SLOTS;
        if (s.pending) { HIPCHECK(hipEventSynchronize(s.ev)); s.pending = false; }
        if (s.cap < bytes) { if (s.p) (void)hipHostFree(s.p); s.p = nullptr; s.cap = std::max<size_t>(bytes, 4096); HIPCHECK(hipHostMalloc(&s.p, s.cap, hipHostMallocDefault)); }
        if (!s.ev) HIPCHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
        std::memcpy(s.p, src, bytes);
        HIPCHECK(hipMemcpyAsync(dst, s.p, bytes, hipMemcpyHostToDevice, st));
        HIPCHECK(hipEventRecord(s.ev, st)); s.pending = true;
    }
    template <typename T> void upload(DevBuf<T>& d, const std::vector<T>& h, hipStream_t st) { d.resize(h.size()); copy(d.p, h.data(), sizeof(T) * h.size(), st); }
};

struct EngineBase {
    snb_config cfg;
    std::string err;
    virtual ~EngineBase() {}
    virtual void setParticles(const double*, const double*, const double*, const int32_t*) = 0;
    virtual void setExceptions(int32_t, const int32_t*, const double*, const double*, const double*, const int32_t*) = 0;
    virtual void setLambdas(const double*) = 0;
    virtual void setParameterOffsets(int, int, const int32_t*, const int32_t*, const double*, int, const int32_t*, const int32_t*, const double*) = 0;
    virtual void setGlobalParameters(int, const double*) = 0;
    virtual void setEnergySlices(const int32_t*) = 0;
    virtual void setDispersion(const double*) = 0;
    virtual void setBox(const double*) = 0;
    virtual void setPositions(const void*, int, int, int) = 0;
    virtual void requestRebuild() = 0;
    virtual void execute(int, int, int, int, double*) = 0;
    virtual void getForces(void*, int, int, int) = 0;
    virtual void setForceOutput(void*, int, int) = 0;
    virtual void bindContext(const snb_context_binding*) = 0;
    virtual void contextOrderChanged() = 0;
    virtual void setShardBlocks(int, int, int) = 0;
    virtual void getSliceEnergies(double*) = 0;
    virtual const double* sliceEnergiesDevice() = 0;
    virtual void sync() = 0;
    virtual void getStats(snb_stats*) = 0;
    virtual void resetTimers() = 0;
    virtual void setTimingInterval(int) = 0;
    virtual void getPme(double*, int32_t*, bool dispersion) = 0;
    virtual void evaluateFrames(const snb_frame_batch*) = 0;
    virtual void evaluateAtomTable(bool forces, int, int, double*, int) = 0;
    virtual void evaluateGroupEnergies(const snb_group_batch*) = 0;
    virtual void evaluateGroupForces(const snb_group_force_batch*) = 0;
    virtual void evaluateGroupPairEnergies(const snb_group_pair_batch*) = 0;
    virtual void evaluateSliceVirials(const snb_virial_batch*) = 0;
    virtual void getFrameStats(snb_frame_stats*) = 0;
};

// ---- dispersion coefficients (SlicedNonbondedForceImpl.cpp:150-185, 263-354), doubles throughout ----
static double evalIntegral(double r, double rs, double rc, double sigma) {
    double A = 1 / (rc - rs), A2 = A * A, A3 = A2 * A;
    double sig2 = sigma * sigma, sig6 = sig2 * sig2 * sig2;
    double rs2 = rs * rs, rs3 = rs * rs2;
    double r2 = r * r, r3 = r * r2, r4 = r * r3, r5 = r * r4, r6 = r * r5, r9 = r3 * r6;
    return sig6 * A3 *
           ((sig6 * (+rs3 * 28 * (6 * rs2 * A2 + 15 * rs * A + 10) - r * rs2 * 945 * (rs2 * A2 + 2 * rs * A + 1) +
                     r2 * rs * 1080 * (2 * rs2 * A2 + 3 * rs * A + 1) - r3 * 420 * (6 * rs2 * A2 + 6 * rs * A + 1) + r4 * 756 * (2 * rs * A2 + A) -
                     r5 * 378 * A2) -
             r6 * (+rs3 * 84 * (6 * rs2 * A2 + 15 * rs * A + 10) - r * rs2 * 3780 * (rs2 * A2 + 2 * rs * A + 1) +
                   r2 * rs * 7560 * (2 * rs2 * A2 + 3 * rs * A + 1))) /
                (252 * r9) -
            std::log(r) * 10 * (6 * rs2 * A2 + 6 * rs * A + 1) + r * 15 * (2 * rs * A2 + A) - r2 * 3 * A2);
}

static void dispersionCoefficients(int n, int nsub, const double* sigma, const double* epsilon, const int32_t* subset, double cutoff,
                                   int useSwitch, double switchDist, double* out) {
    const int S = nsub * (nsub + 1) / 2;
    std::map<std::tuple<double, double, int>, double> classes;
    for (int i = 0; i < n; i++) classes[std::make_tuple(sigma[i], epsilon[i], (int)subset[i])] += 1.0;
    std::vector<double> s1(S, 0.0), s2(S, 0.0), s3(S, 0.0);
    auto sl = [](int a, int b) { return a > b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; };
    for (auto& c : classes) {
        double sg = std::get<0>(c.first), ep = std::get<1>(c.first); int s = std::get<2>(c.first);
        double count = c.second * (c.second + 1) / 2;
        double q = sg * sg, s6 = q * q * q;
        int slice = s * (s + 3) / 2;
        s1[slice] += count * ep * s6 * s6; s2[slice] += count * ep * s6;
        if (useSwitch) s3[slice] += count * ep * (evalIntegral(cutoff, switchDist, cutoff, sg) - evalIntegral(switchDist, switchDist, cutoff, sg));
    }
    for (auto a = classes.begin(); a != classes.end(); ++a)
        for (auto b = classes.begin(); b != a; ++b) {
            double sg = 0.5 * (std::get<0>(a->first) + std::get<0>(b->first));
            double ep = std::sqrt(std::get<1>(a->first) * std::get<1>(b->first));
            int slice = sl(std::get<2>(a->first), std::get<2>(b->first));
            double count = a->second * b->second;
            double q = sg * sg, s6 = q * q * q;
            s1[slice] += count * ep * s6 * s6; s2[slice] += count * ep * s6;
            if (useSwitch) s3[slice] += count * ep * (evalIntegral(cutoff, switchDist, cutoff, sg) - evalIntegral(switchDist, switchDist, cutoff, sg));
        }
    double N = n, numInteractions = (N * (N + 1)) / 2;
    for (int s = 0; s < S; s++)
        out[s] = 8 * N * N * SNB_PI * ((s1[s] / numInteractions) / (9 * std::pow(cutoff, 9)) - (s2[s] / numInteractions) / (3 * std::pow(cutoff, 3)) + s3[s] / numInteractions);
}

// ---- B-spline moduli (ReferencePME.cpp:88-183) ----
static void bsplineModuli(int n, int order, std::vector<double>& out) {
    std::vector<double> data(order, 0.0), bsp(std::max(n, order + 1), 0.0);
    data[order - 1] = 0; data[1] = 0; data[0] = 1;
    for (int k = 3; k < order; k++) {
        double div = 1.0 / (k - 1.0);
        data[k - 1] = 0;
        for (int l = 1; l < (k - 1); l++) data[k - l - 1] = div * (l * data[k - l - 2] + (k - l) * data[k - l - 1]);
        data[0] = div * data[0];
    }
    double div = 1.0 / (order - 1);
    data[order - 1] = 0;
    for (int l = 1; l < (order - 1); l++) data[order - l - 1] = div * (l * data[order - l - 2] + (order - l) * data[order - l - 1]);
    data[0] = div * data[0];
    for (int i = 1; i <= order; i++) bsp[i] = data[i - 1];
    out.assign(n, 0.0);
    for (int i = 0; i < n; i++) {
        double sc = 0, ss = 0;
        for (int j = 0; j < n && j <= order; j++) { double arg = (2.0 * SNB_PI * i * j) / n; sc += bsp[j] * std::cos(arg); ss += bsp[j] * std::sin(arg); }
        out[i] = sc * sc + ss * ss;
    }
    for (int i = 0; i < n; i++)
        if (out[i] < 1.0e-7) out[i] = (out[(i - 1 + n) % n] + out[(i + 1) % n]) / 2;
}

template <typename Real> struct PmePlan {
    PmePlanDims d;
    double alpha = 0;
    bool dispersion = false;
    DevBuf<Real> gridReal;
    DevBuf<typename Vec<Real>::T2> gridCplx, gridCplxB, twx, twy, twz;      // (gridCplxB: second complex mesh of the plane path, single precision)
    DevBuf<Real> modx, mody, modz;
    DevBuf<Real> planeEterm; bool planeEtermReady = false, planeEtermFilled = false; double planeEtermKey[10] = {0};      // plane path: kernel-value table, refilled at a rebuild when the box or alpha changed
    // own-atoms spreader (pme.hip k_spreadOwn / k_spreadMerge): geometry and buffers, sized at rebuild time
    int ownSlabs = 0, ownMargin = 1; DevBuf<unsigned char> ownPartial; DevBuf<int> ownBusy; DevBuf<int2> strays;
    void init(const int g[3], int nGrids, hipStream_t s) {
        if (!planDims(g, sizeof(Real), switches(), d)) throw HipError{"PME mesh size is not FFT-legal"};      // sizes and splits: pme_plan.h
        // pme.hip divides index values by reciprocal multiplication (FastDiv: exact for dividends below 2^22).  Its dividends are LDS element
        // indices of one work-group (< 40 960), line / chunk counts of one brick, and indices into one mesh plane or one (y, kz) slab:
        // at most 1024 x 1024 = 2^20 under this cap.
        if (d.nx > 1024 || d.ny > 1024 || d.nz > 1024) throw HipError{"PME mesh dimensions above 1024 are not supported"};
        gridReal.resize((size_t)nGrids * d.nx * d.ny * d.nz);
        gridCplx.resize((size_t)nGrids * d.nx * d.ny * d.nzc);
        if (planePath(d, nGrids, sizeof(Real), switches()).buffers) { gridCplxB.resize((size_t)nGrids * d.nx * (d.ny + 8) * d.nzc);      // (plane path, planes that fit LDS; y padded to whole tiles of the inverse z kernel)
             planeEterm.resize((size_t)d.nx * d.ny * d.nzc); planeEtermReady = false; }
        auto tw = [&](int n, DevBuf<typename Vec<Real>::T2>& buf) {
            std::vector<typename Vec<Real>::T2> h(n);
            for (int k = 0; k < n; k++) { double a = -2.0 * SNB_PI * k / n; h[k].x = (Real)std::cos(a); h[k].y = (Real)std::sin(a); }
            buf.upload(h, s);
        };
        tw(d.nx, twx); tw(d.ny, twy); tw(d.nz, twz);
        auto md = [&](int n, DevBuf<Real>& buf) {
            std::vector<double> m; bsplineModuli(n, SNB_PME_ORDER, m);
            std::vector<Real> h(m.begin(), m.end());
            buf.upload(h, s);
        };
        md(d.nx, modx); md(d.ny, mody); md(d.nz, modz);
        HIPCHECK(hipStreamSynchronize(s));
    }
};

template <typename Real> class Engine : public EngineBase {
    using T4 = typename Vec<Real>::T4;
    using T2 = typename Vec<Real>::T2;
public:
    int N, nsub, S;
    hipStream_t stream = nullptr; bool ownStream = false;
    // ring of per-execute event sets, harvested lazily into cumulative kernel times (no per-step host sync)
    static constexpr int RING = 32;
    hipEvent_t evRebuild[3] = {nullptr, nullptr, nullptr};
    hipEvent_t evStepDone[2] = {nullptr, nullptr}; long long stepCounter = 0;      // displacement-triggered rebuilds: end-of-execute events
    hipStream_t stream2 = nullptr; hipEvent_t evFork = nullptr, evJoin = nullptr, evPairA = nullptr;
    const Switches& sw = switches();
    // (sw.concurrentPme, the fork of forces-only graph steps, is opt-in: the graph's cross-stream dependencies cost more than the overlap returns)
    // Overlapped steps (sw.overlap, round 4; the reference runs its reciprocal pipeline on a queue of its own beside the pair kernel,
    // CommonNonbondedSlicingKernels.cpp:520-530, 1176-1179, 1377-1380).  Graph steps run the PME chain on stream2 while a first launch of
    // the tile kernel, held to sw.overlapCuLimit work-groups per CU (its work-groups count themselves per physical CU and leave when the
    // CU is full), runs beside it; a second launch behind the chain fills the chip.  Both launches claim their work items from one
    // device counter, so the split follows the chain's actual duration.  Eager (stamped) steps stay serial: the per-kernel timers keep
    // measuring every kernel alone.  dOverlap: [0] the counter, [16 ...] the SNB_CU_SLOTS residency counts; zeroed by the gather pass.
    int numCUs = 256; DevBuf<int> dOverlap, dOverlapTrace; int overlapDumps = 3;
    int pairVgprUnits[2][3];      // [per-pair wrapping][StepEnergy]: register allocation of the tile kernel a CU-limited launch runs (direct.hip directVgprUnits), resolved by the constructor
    struct EvSet { hipEvent_t e[5]; bool pending = false; KernelStamps ks; };   // start, direct0, direct1(=recip0 after pair lists), recip1, end; per-kernel stamps (snb_stats.sum_kernel_ms)
    std::vector<EvSet> ring; int ringPos = 0;
    // host-side definition
    std::vector<double> charge, sigma, epsilon; std::vector<int32_t> subset;
    std::vector<int32_t> excPairs; std::vector<double> excQQ, excSigma, excEps; std::vector<int32_t> excForce14;
    std::vector<double> lambdas, dispCoef; std::vector<Real> hLambdas; PinnedRing pinned;
    double box[9] = {0}; bool haveBox = false, haveParticles = false;
    // positions
    const void* devUserPos = nullptr; int posIsDouble = 1, posStride4 = 0; bool havePositions = false;
    DevBuf<unsigned char> ownedPos;
    // sorted state
    int* hNbPub = nullptr; int* dNbPub = nullptr; int nbPubSeq = 0;      // the rebuild's totals in mapped host memory + sequence number (gpuRebuild)
    // Rebuild BESIDE the steps (fixed rebuild interval; startSideBuild / finishSideBuild): `sw.sideLead` steps before a rebuild falls due the
    // positions are copied aside and the whole GPU build runs on a stream of its own into the second set of list buffers (`shadow`), while the
    // steps go on with the list in use; when the rebuild falls due the two sets change places.  The build's small latency-bound kernels fill
    // gaps of the steps instead of standing between them (measured with a second engine as the builder, tools/async_rebuild_probe.py: 24 us
    // per step for a rebuild every 20 steps, against 38-40 in line).
    struct ListShadow {
        DevBuf<int> dUserToSorted, dSortedToUser, atomSubset, atomGrid, blockSubset, tileJ; DevBuf<int2> colRange; DevBuf<T4> posq, posRef; DevBuf<T2> sigeps;
        DevBuf<Real> imageOffset; DevBuf<int4> tileInfo, workItems; DevBuf<unsigned> masks;
    } shadow;
    hipStream_t streamBuild = nullptr; hipEvent_t evSnap = nullptr, evBuilt = nullptr, evFlagsReset = nullptr; bool flagsResetPending = false; DevBuf<unsigned char> posSnap;
    bool sortGraphSuspect = false;      // see gpuRebuild
    // Frame batches (snb_evaluate_frames, evaluateFrames below): the list of frame f + 1 is built on streamBuild into the shadow set, straight
    // from that frame's positions, while the energy-only step of frame f runs on the step stream.  Host frames arrive through two pinned
    // staging buffers on a copy stream, ahead of their build.  evFrameStep[f & 1] follows the step of frame f: whatever rewrites something
    // that step read (the shadow set, a staging slot) waits for it on its own stream -- the host never drains the step stream between frames.
    snb_frame_stats fstats;
    bool plainSort = false;      // frame builds issue phase A as plain launches: every frame is another position pointer, i.e. another graph key
    hipStream_t streamCopy = nullptr; hipEvent_t evFrameStep[2] = {nullptr, nullptr}, evFrameUp[2] = {nullptr, nullptr}, evBatchStart = nullptr; bool frameUpPending[2] = {false, false};
    void* framePinned[2] = {nullptr, nullptr}; size_t framePinnedCap[2] = {0, 0}; DevBuf<unsigned char> frameDev[2];
    DevBuf<double> frameTab, frameStates, dStateLambdas;
    bool sideBuilding = false, sidePending = false; int sideSeq = 0; long long sideBuilds = 0, sideDiscarded = 0;
    int lastPadCount = 0;      // the exact padded count of the last accepted build (what a frame batch sizes its own prediction from)
    int npadPredict = 0; long long padMispredictions = 0;      // > 0: size of the padded arrays the next GPU rebuild assumes (gpuRebuild); how often that was too small
    int Npad = 0, numBlocks = 0; int64_t numTiles = 0, numMaskTiles = 0, shardTiles = 0; bool wrapMode = false;
    DevBuf<T4> posq; DevBuf<T2> sigeps; DevBuf<Real> forceBuf, imageOffset, dLambdas;
    struct FView { Real* p = nullptr; } fx, fy, fz, fpx, fpy, fpz;   // views of forceBuf (7 Npad values, cleared by the position-gather pass)
    int fstride = 1;      // index stride of an atom in the direct-space accumulators (three arrays fx | fy | fz: 1)
    // SNB_MIXED: single-precision arithmetic, direct-space forces accumulated in 64-bit fixed point (direct.hip, fAdd) -- three arrays of
    // Npad 64-bit words (6 Npad floats, one spare), then the three reciprocal arrays: 10 Npad floats, all cleared by the gather pass
    bool fixedForces() const { return sizeof(Real) == 4 && cfg.precision == SNB_MIXED; }
    bool useSwitch() const { return cfg.use_switch && cfg.method != SNB_NoCutoff && cfg.method != SNB_LJPME; }
    int methodClass() const {
        if (cfg.method == SNB_CutoffNonPeriodic || cfg.method == SNB_CutoffPeriodic) return MC_RF;
        if (cfg.method == SNB_Ewald || cfg.method == SNB_PME) return MC_EWALD;
        return cfg.method == SNB_LJPME ? MC_LJPME : MC_NOCUTOFF;
    }
    int forceArrays() const { return fixedForces() ? 10 : 7; }
    void layoutForces() {
        forceBuf.resize((size_t)forceArrays() * Npad);
        pointForceViews(forceBuf.p);
    }
    // the views over a force set: forceBuf, or (energy-only steps of sharded PME engines, whose energies come from the force interpolation)
    // forceScratch, so that such a step leaves the engine's forces alone
    Real* forceBase = nullptr;
    DevBuf<Real> forceScratch;
    struct ForceSet { Real *x, *y, *z, *px, *py, *pz; };
    ForceSet forceSet(Real* base, int npad) const {      // component bases of a force set laid out for npad padded atoms
        if (fixedForces())      // (three arrays of 64-bit words, then the three reciprocal arrays)
            return {base, base + 2 * (size_t)npad, base + 4 * (size_t)npad, base + 7 * (size_t)npad, base + 8 * (size_t)npad, base + 9 * (size_t)npad};
        return {base, base + (size_t)npad, base + 2 * (size_t)npad, base + 4 * (size_t)npad, base + 5 * (size_t)npad, base + 6 * (size_t)npad};
    }
    void pointForceViews(Real* base) {
        forceBase = base;
        fstride = 1;
        const ForceSet v = forceSet(base, Npad);
        fx.p = v.x; fy.p = v.y; fz.p = v.z; fpx.p = v.px; fpy.p = v.py; fpz.p = v.pz;
    }
    // The forces of the last forces step across the rebuilds of energy-only steps.  The force arrays are in SORTED order: a rebuild re-sorts the
    // atoms (new permutation, possibly a new padded count and a reallocated forceBuf) and a side-build exchange swaps the permutations, so
    // before an energy-only step rebuilds, the force set and the user-to-sorted map it was accumulated under are copied aside (stream-ordered)
    // and snb_get_forces reads that copy until the next forces step.
    bool haveForceStep = false, keptValid = false, keptRecip = false;
    int keptNpad = 0;
    DevBuf<Real> keptForces;
    DevBuf<int> keptUserToSorted;
    void keepLastForces() {
        if (!haveForceStep || keptValid) return;
        const size_t n = (size_t)forceArrays() * Npad;
        keptForces.resize(n); keptUserToSorted.resize(std::max(N, 1));
        HIPCHECK(hipMemcpyAsync(keptForces.p, forceBuf.p, sizeof(Real) * n, hipMemcpyDeviceToDevice, stream));
        if (N > 0) HIPCHECK(hipMemcpyAsync(keptUserToSorted.p, dUserToSorted.p, sizeof(int) * N, hipMemcpyDeviceToDevice, stream));
        keptNpad = Npad; keptRecip = lastRecip; keptValid = true;
    }
    DevBuf<int> pmeCells, dZIndex, dScanA, dScanB, dScanC, dAtomCell, dExtent;
    double tileCell[9] = {0};      // the cell the tile image codes refer to (the box; an enclosing cell for CutoffNonPeriodic)
    DevBuf<long long> dNbTrace, dPmeTrace, dStepTrace;      // dStepTrace: SNB_STEP_TRACE, device wall-clock stamps of the last replayed step
    // Parameter offsets on the device (the reference: platforms/common/src/kernels/nonbondedParameters.cc:4-179).  charge/sigma/epsilon
    // and the exception arrays above hold the BASE values; effective = base + sum_k global[k] * delta is formed by k_particleParams /
    // k_exceptionParams whenever a base value, an offset or a global parameter changes -- no re-sort, no tile rebuild, no graph re-capture,
    // no host synchronisation.  The same pass reduces what the closed-form energy terms and the spreader's fixed-point scale need.
    struct Offset { int target, global; double d[3]; };
    std::vector<Offset> offP, offE; std::vector<double> gValues; int nGlobals = 0;
    bool basePDirty = true, baseEDirty = true, offsetsDirty = true, globalsDirty = true;
    DevBuf<double> dBaseP, dOffPDelta, dBase14, dOff14Delta, dGlobals, dParamSums;      // dParamSums: [3 nsub] (sum q, sum q^2, sum c6^2) + 2 ordered-int maxima
    DevBuf<int> dOffPStart, dOffPGlobal, dOff14Start, dOff14Global, dSlice14;
    DevBuf<Real> dFixScale;      // [4]: fixed-point scale and its inverse of the charge mesh, then of the dispersion mesh
    DevBuf<int> dSortedToUser, dUserToSorted, blockSubset, tileJ, atomSubset, atomGrid, gridSubset, exclStart, exclList;
    // GPU neighbour build: static user-order data and scratch
    DevBuf<int> dUSubset, dSlotOfSubset, dValsIn, dValsOut, dCounters; DevBuf<Real> dUCharge, dWrapped, dOffsetU; DevBuf<T2> dUSigEps;
    DevBuf<unsigned char> dSortTemp; DevBuf<unsigned long long> dKeysIn, dKeysOut; DevBuf<float> dBlockCenter, dBlockHalf;
    std::vector<int> hExclStart, hExclList, hSlotOfSubset;      // uploadStatic's host copies of exclStart / exclList / dSlotOfSubset, for the host builder
    size_t tileCap = 0; bool staticDirty = true, gpuBuilt = false;
    DevBuf<int2> pairs14, pairsExcl, colRange; DevBuf<int4> tileInfo, workItems, workItemsStage, workItemsPartial; int numWorkItems = 0; int colCells[2] = {0, 0}; DevBuf<unsigned> masks;
    DevBuf<T4> params14, paramsExcl; int n14 = 0, nExcl = 0;
    DevBuf<int> dSliceNeedAll, dSliceNeedSel; std::vector<int> sliceNeedSel;      // energy steps: every slice / the slices a derivative-only step (include_energy == 2) must produce
    DevBuf<double> dDispCoef, sliceE, sliceTotal;      // 64 partitioned copies of the raw [S][2] energies, and their sum (last kernel of an energy step)
    bool energyPending = false;      // the last energy step's sums are still on the device
    std::vector<double> hostSliceE;   // raw energies of the last energy evaluation (device part + host terms)
    PmePlan<Real> pme, dpme; int nGrids = 0; std::vector<int> ownedSubsets; DevBuf<int> dStrayCount;      // [2] stray atoms of the own-atoms spreader (Coulomb mesh, dispersion mesh)
    bool needRebuild = true, paramsDirty = true; int stepsSinceRebuild = 0;
    // direct-space ownership: i-block I belongs to this engine when I % shardPeriod lies in [shardBegin, shardEnd); the default is
    // (shard_rank, shard_rank + 1, shard_count); snb_set_shard_blocks lets the host rebalance direct-space work between ranks
    int shardBegin = 0, shardEnd = 1, shardPeriod = 1;
    void setShardBlocks(int begin, int end, int period) override {
        if (period < 1 || begin < 0 || end < begin || end > period) throw std::runtime_error("snb_set_shard_blocks: need 0 <= begin <= end <= period");
        if (begin == shardBegin && end == shardEnd && period == shardPeriod) return;
        shardBegin = begin; shardEnd = end; shardPeriod = period; needRebuild = true;
    }
    bool valuesDirty = false, excValuesDirty = false, haveExceptions = false;   // parameter values changed, structure did not
    // displacement watch: reference positions of the last rebuild and two flags in mapped host memory (read without synchronising)
    DevBuf<T4> posRef; int* hDispFlags = nullptr; int* dDispFlags = nullptr; int64_t listOverruns = 0;
    std::vector<int3> hKvec; DevBuf<int3> dKvec; DevBuf<Real> dCosSin;
    struct GraphKey {
        const void* pos; int isDouble, stride4; bool direct, recip; int energy; void* out; int outDouble, outAcc;      // energy: 0 forces only, 1 all slice energies, 2 selected slices
        const void* ctxPosq = nullptr; void* ctxForce = nullptr; void* ctxEnergy = nullptr; void* ctxDeriv = nullptr; int ctxPadded = 0, ctxFlags = 0;      // the bound context's buffers (ctxFlags: 1 bound, 2 double posq, 4 double accumulators, 8 this step adds its total energy)
        bool operator==(const GraphKey& o) const { return pos == o.pos && isDouble == o.isDouble && stride4 == o.stride4 && direct == o.direct && recip == o.recip && energy == o.energy && out == o.out && outDouble == o.outDouble && outAcc == o.outAcc
                                                          && ctxPosq == o.ctxPosq && ctxForce == o.ctxForce && ctxEnergy == o.ctxEnergy && ctxDeriv == o.ctxDeriv && ctxPadded == o.ctxPadded && ctxFlags == o.ctxFlags; }
    };
    void* outPtr = nullptr; int outIsDouble = 0, outAccumulate = 0; bool outputWritten = false;   // snb_set_force_output
    // Context binding (snb_bind_context): the caller's context-order buffers.  The per-step path goes straight to them -- the gather pass reads
    // posq[userToCtx[u]], the step's last kernel adds into force / energy / deriv -- through ONE engine-owned map, user -> context slot, which
    // depends on the context's order alone: rebuilds, re-sorts and list exchanges leave it alone, and snb_context_order_changed refreshes it with
    // one kernel.  Rebuild-time code (extent, sort keys, the host builder's read-back, the side build's snapshot) works from a user-order copy
    // of the positions staged when a rebuild starts (stageCtxPositions), so a list being built beside the steps does not depend on the order
    // the context has moved on to.
    struct CtxBinding { bool on = false; const void* posq = nullptr; const int* atomIndex = nullptr; int isDouble = 0, paddedN = 0; long long* force = nullptr; void* energy = nullptr; void* deriv = nullptr; int energyIsDouble = 0; } ctx;
    DevBuf<int> dUserToCtx, dCtxScratch, dDerivSlot; DevBuf<unsigned char> ctxStage; DevBuf<double> dLambdas64;
    // What a step does with forces: Full -- a forces step (accumulate, deliver to the force output); None -- an energy-only step (the
    // energy-only kernels: no force arithmetic, nothing cleared, nothing stored); Scratch -- the forces kernels into whatever set the views
    // point at, no delivery (energy-only steps of sharded PME engines).
    enum class StepForces { Full, None, Scratch };
    enum class StepEnergy { None = 0, All = 1, Selected = 2 };      // (Selected: the slices of snb_set_energy_slices, a derivative-only step; the values are GraphKey::energy)
    // What one step does.  Whoever asks for a step says all of it here: enqueueStep and what it calls read nothing else about the request,
    // and the key of a captured step (graphKey) is computed from the same value.
    struct StepRequest {
        StepEnergy energy = StepEnergy::None;
        bool direct = true, recip = true;
        StepForces forces = StepForces::Full;
        bool addCtxTotal = false;      // the bound context's total energy is added on the device
        double* rowOut = nullptr;      // the row of a frame batch's table the step's finish kernel also writes
        EvSet* ev = nullptr;      // a timed (eager) step's events
    };
    const int* sliceNeed(StepEnergy e) const { return e == StepEnergy::Selected ? dSliceNeedSel.p : dSliceNeedAll.p; }
    GraphKey graphKey(const StepRequest& r) const {      // whatever changes what a captured step launches: the request, and the position, output and binding state
        GraphKey k{devUserPos, posIsDouble, posStride4, r.direct, r.recip, (int)r.energy, outPtr, outIsDouble, outAccumulate};
        if (ctx.on) { k.ctxPosq = ctx.posq; k.ctxForce = ctx.force; k.ctxEnergy = ctx.energy; k.ctxDeriv = ctx.deriv; k.ctxPadded = ctx.paddedN;
                      k.ctxFlags = 1 | (ctx.isDouble ? 2 : 0) | (ctx.energyIsDouble ? 4 : 0) | (r.addCtxTotal ? 8 : 0); }
        return k;
    }
    void stageCtxPositions(void* dst) { launchCtxStagePositions(ctx.posq, ctx.isDouble, dUserToCtx.p, N, dst, stream); }
    void bindContext(const snb_context_binding* b) override {
        if (!b) {
            if (!ctx.on) return;
            if (sidePending) cancelSideBuild();
            ctx = CtxBinding(); devUserPos = nullptr; havePositions = false;      // (the positions must be set again)
            return;
        }
        if (cfg.shard_count > 1) { err = "snb_bind_context: not available with shard_count > 1"; throw (int)SNB_ERR_UNSUPPORTED; }
        if (!b->posq || !b->atom_index) throw HipError{"snb_bind_context: posq and atom_index must be given"};
        if (b->padded_n < N) throw HipError{"snb_bind_context: padded_n is smaller than n_atoms"};
        // atom_index must be a permutation: inverted into a scratch map with every out-of-range or repeated entry counted; nothing is read through
        // the indices, and the engine's own map is replaced only when the count is zero
        dCtxScratch.resize((size_t)N + 1);
        launchCtxFill(dCtxScratch.p, N, -1, stream); launchCtxFill(dCtxScratch.p + N, 1, 0, stream);
        launchCtxInvert(b->atom_index, N, dCtxScratch.p, dCtxScratch.p + N, stream);
        int bad = 0;
        HIPCHECK(hipMemcpyAsync(&bad, dCtxScratch.p + N, sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        if (bad != 0) throw HipError{"snb_bind_context: atom_index is not a permutation of 0 .. n_atoms-1"};
        if (sidePending) cancelSideBuild();
        dUserToCtx.resize(std::max(N, 1));
        if (N > 0) HIPCHECK(hipMemcpyAsync(dUserToCtx.p, dCtxScratch.p, sizeof(int) * N, hipMemcpyDeviceToDevice, stream));
        ctx.on = true; ctx.posq = b->posq; ctx.atomIndex = b->atom_index; ctx.isDouble = b->is_double ? 1 : 0; ctx.paddedN = b->padded_n;
        ctx.force = reinterpret_cast<long long*>(b->force_buffer); ctx.energy = b->energy_buffer; ctx.energyIsDouble = b->energy_is_double ? 1 : 0;
        ctx.deriv = (b->deriv_buffer && b->deriv_slot) ? b->deriv_buffer : nullptr;
        std::vector<int> slots((size_t)S * 2, -1);
        if (ctx.deriv) for (int i = 0; i < 2 * S; i++) slots[i] = b->deriv_slot[i] < 0 ? -1 : b->deriv_slot[i];
        dDerivSlot.upload(slots, stream);
        dLambdas64.upload(lambdas, stream);
        HIPCHECK(hipStreamSynchronize(stream));      // (the host vectors above may go)
        if (ctx.force) { outPtr = nullptr; outputWritten = false; }      // a bound force buffer takes the place of snb_set_force_output
        ctxStage.resize((size_t)std::max(N, 1) * 4 * (ctx.isDouble ? 8 : 4));
        devUserPos = ctxStage.p; posIsDouble = ctx.isDouble; posStride4 = 1; havePositions = true;      // what rebuild-time code reads
    }
    void contextOrderChanged() override {
        if (!ctx.on) { err = "snb_context_order_changed: no context is bound"; throw (int)SNB_ERR_STATE; }
        launchCtxInvert(ctx.atomIndex, N, dUserToCtx.p, nullptr, stream);      // (every entry it writes is a slot below N, whatever atom_index holds)
    }
    // captured step graphs, a few at a time: a caller that alternates between position (or output) buffers keeps one graph per buffer
    struct CachedGraph { GraphKey key; hipGraphExec_t exec; bool stale; };      // stale: the arguments changed (rebuild, parameters): re-captured and UPDATED in place at the next use
    std::vector<CachedGraph> graphs; size_t graphVictim = 0; long long execCount = 0;
    static constexpr size_t MAX_GRAPHS = 4;
    int timingInterval = 32; long long stampCounter = 0;
    void setTimingInterval(int n) override { timingInterval = n; execCount = 0; }
    struct SortGraph { std::vector<unsigned char> key; hipGraphExec_t exec; };
    std::vector<SortGraph> sortGraphs; size_t sortGraphVictim = 0; bool sortGraphBroken = false;      // phase A of the neighbour rebuild (one per buffer set / position source: up to 4)
    // A rebuild (or a changed 1-4 list, box, dispersion table) changes kernel arguments, not the step's kernels: the executable graphs are kept
    // and refreshed with hipGraphExecUpdate from a new capture.  Instantiating the forked graph of an overlapped step anew costs the host
    // ~0.7 ms (a linear one 10 us), i.e. 0.3 ms of idle GPU after every rebuild; an update that fails falls back to a new instantiation.
    void dropGraph() { for (auto& g : graphs) g.stale = true; }
    void destroyGraphs() { for (auto& g : graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec); graphs.clear(); graphVictim = 0; }
    bool lastRecip = false;
    std::vector<int> hostGridSubset;      // subset of each held mesh
    unsigned long long emptyGrids = 0;    // PmeParams::emptyGrids, from the subsets of snb_set_particles (a change of subsets rebuilds)
    snb_stats stats;

    Engine(const snb_config& c) {
        cfg = c; N = c.n_atoms; nsub = c.n_subsets; S = nsub * (nsub + 1) / 2;
        std::memset(&stats, 0, sizeof(stats)); std::memset(&fstats, 0, sizeof(fstats));
        HIPCHECK(hipSetDevice(c.device));
        if (c.stream) stream = (hipStream_t)c.stream; else { HIPCHECK(hipStreamCreate(&stream)); ownStream = true; }
        ring.resize(RING);
        { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, c.device) == hipSuccess && prop.multiProcessorCount > 0) numCUs = prop.multiProcessorCount; }
        if (cfg.method >= SNB_Ewald) buildEwaldPoly();      // (before the kernels are chosen: polyMask decides their instantiation)
        stats.ewald_poly_mask = polyMask;
        {      // the tile kernels a CU-limited launch can run: their allocations are asked for here, outside any capture
            DirectParams<Real> p;
            std::memset(&p, 0, sizeof(p));
            p.useSwitch = useSwitch() ? 1 : 0; p.ewUsePoly = polyMask; p.fixed = fixedForces();
            for (int w = 0; w < 2; w++) for (int e = 0; e < 3; e++) pairVgprUnits[w][e] = directVgprUnits<Real>(p, methodClass(), w != 0, e);
        }
        if (sw.overlap) { dOverlap.resize(SNB_OVERLAP_INTS); HIPCHECK(hipMemsetAsync(dOverlap.p, 0, sizeof(int) * SNB_OVERLAP_INTS, stream)); }
        if (sw.stepTrace) { dStepTrace.resize(16); HIPCHECK(hipMemsetAsync(dStepTrace.p, 0, sizeof(long long) * 16, stream)); }
        if (sw.overlap && sw.overlapDebug) { dOverlapTrace.resize(SNB_CU_SLOTS * 8); HIPCHECK(hipMemsetAsync(dOverlapTrace.p, 0xff, sizeof(int) * SNB_CU_SLOTS * 8, stream)); }
        for (auto& r : ring) { for (int k = 0; k < 5; k++) HIPCHECK(hipEventCreate(&r.e[k])); for (int k = 0; k < 16; k++) { HIPCHECK(hipEventCreate(&r.ks.start[k])); HIPCHECK(hipEventCreate(&r.ks.stop[k])); } }
        charge.assign(N, 0.0); sigma.assign(N, 1.0); epsilon.assign(N, 0.0); subset.assign(N, 0);
        lambdas.assign((size_t)S * 2, 1.0); dispCoef.assign(S, 0.0); hostSliceE.assign((size_t)S * 2, 0.0);
        sliceE.resize((size_t)S * 2 * SNB_SLICE_E_PARTS); sliceTotal.resize((size_t)S * 2);
        dDispCoef.upload(dispCoef, stream);
        sliceNeedSel.assign(S, 1); dSliceNeedAll.upload(sliceNeedSel, stream); dSliceNeedSel.upload(sliceNeedSel, stream);
        HIPCHECK(hipStreamSynchronize(stream));
        if (cfg.shard_count < 1) cfg.shard_count = 1;
        shardBegin = cfg.shard_count > 1 ? cfg.shard_rank : 0; shardEnd = shardBegin + 1; shardPeriod = cfg.shard_count;
        // tabulated Ewald force factor: opt-in.  Measured on MI355X it only trades 4 % of the VALU instructions for LDS gathers (the packed
        // analytic erfc is already cheap) and leaves the kernel time unchanged, so the analytic form stays the default.
        HIPCHECK(hipHostMalloc((void**)&hDispFlags, 64, hipHostMallocMapped));
        std::memset(hDispFlags, 0, 64);      // [0] warn, [1] overrun, [4] overruns counted on the device (k_dispFlagsReset)
        HIPCHECK(hipHostGetDevicePointer((void**)&dDispFlags, hDispFlags, 0));
        HIPCHECK(hipHostMalloc((void**)&hNbPub, 64, hipHostMallocMapped));
        std::memset(hNbPub, 0, 64);
        HIPCHECK(hipHostGetDevicePointer((void**)&dNbPub, hNbPub, 0));
        for (int s = 0; s < nsub; s++) if (s % cfg.shard_count == cfg.shard_rank) ownedSubsets.push_back(s);
        nGrids = cfg.shard_count == 1 ? nsub : (int)ownedSubsets.size();
        if (isPme()) {
            for (int d = 0; d < 3; d++) cfg.grid[d] = legalGridSize(cfg.grid[d]);
            pme.alpha = cfg.alpha; pme.dispersion = false;
            if (nGrids > 0) pme.init(cfg.grid, nGrids, stream); else { pme.d.nx = cfg.grid[0]; pme.d.ny = cfg.grid[1]; pme.d.nz = cfg.grid[2]; }
            if (cfg.method == SNB_LJPME) {
                for (int d = 0; d < 3; d++) cfg.dgrid[d] = legalGridSize(cfg.dgrid[d]);
                dpme.alpha = cfg.alpha_d; dpme.dispersion = true;
                if (nGrids > 0) dpme.init(cfg.dgrid, nGrids, stream); else { dpme.d.nx = cfg.dgrid[0]; dpme.d.ny = cfg.dgrid[1]; dpme.d.nz = cfg.dgrid[2]; }
            }
            std::vector<int> gs = cfg.shard_count == 1 ? std::vector<int>() : ownedSubsets;
            if (cfg.shard_count == 1) { gs.resize(nsub); std::iota(gs.begin(), gs.end(), 0); }
            gridSubset.upload(gs, stream);
            hostGridSubset = gs;
        }
    }
    ~Engine() override {
        (void)hipStreamSynchronize(stream);
        if (sw.verbose && stats.n_rebuilds > 0) fprintf(stderr, "[snb] rebuilds: %lld, of them %lld built beside the steps; %lld side builds discarded\n", (long long)stats.n_rebuilds, sideBuilds, sideDiscarded);
        if (dStepTrace.p) {      // device wall clock (100 MHz) of the last replayed step, relative to the start of its gather pass
            long long t[16] = {0}; (void)hipMemcpy(t, dStepTrace.p, sizeof(t), hipMemcpyDeviceToHost);
            auto us = [&](int k) { return t[k] ? (t[k] - t[0]) / 100.0 : -1.0; };
            fprintf(stderr, "[snb] step trace (us after the gather pass started; -1: not run): pair A %.1f .. %.1f | pair B %.1f .. %.1f | own %.1f | merge %.1f | plane %.1f | mix+z %.1f .. %.1f | interpolation %.1f .. %.1f\n",
                    us(2), us(3), us(4), us(5), us(6), us(7), us(8), us(9), us(10), us(11), us(12));
        }
        if (dPmeTrace.p) {
            long long g[8] = {0}; (void)hipMemcpy(g, dPmeTrace.p, 64, hipMemcpyDeviceToHost);
            if (g[7] > 0 && g[3] > 0) fprintf(stderr, "[snb] merge kernel prologue (busy flags, roots of unity, barrier): %.2f us per busy work-group\n", g[3] / 100.0 / g[7]);
            if (g[7] > 0) fprintf(stderr, "[snb] spreading (busy work-groups; scanning spreader: scan / entries / z FFT + store; merge kernel: sums / strays + z FFT / store): %.2f us, %.2f us, %.2f us per work-group (%lld work-groups)\n", g[4] / 100.0 / g[7], g[5] / 100.0 / g[7], g[6] / 100.0 / g[7], g[7]);
        }
        if (dPmeTrace.p) { long long h[4] = {0, 0, 0, 0}; (void)hipMemcpy(h, dPmeTrace.p, 32, hipMemcpyDeviceToHost); if (h[2] > 0) fprintf(stderr, "[snb] interpolation bricks: mean load %.2f us, mean compute %.2f us per work-group (%lld work-groups)\n", h[0] / 100.0 / h[2], h[1] / 100.0 / h[2], h[2]); }
        destroyGraphs();
        if (streamBuild) { (void)hipStreamSynchronize(streamBuild); (void)hipStreamDestroy(streamBuild); if (evSnap) (void)hipEventDestroy(evSnap); if (evBuilt) (void)hipEventDestroy(evBuilt); if (evFlagsReset) (void)hipEventDestroy(evFlagsReset); }
        if (streamCopy) { (void)hipStreamSynchronize(streamCopy); (void)hipStreamDestroy(streamCopy); }
        for (int k = 0; k < 2; k++) { if (evFrameStep[k]) (void)hipEventDestroy(evFrameStep[k]); if (evFrameUp[k]) (void)hipEventDestroy(evFrameUp[k]); if (framePinned[k]) (void)hipHostFree(framePinned[k]); }
        if (evBatchStart) (void)hipEventDestroy(evBatchStart);
        for (auto& g : sortGraphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
        sortGraphs.clear();
        for (auto& r : ring) { for (int k = 0; k < 5; k++) (void)hipEventDestroy(r.e[k]); for (int k = 0; k < 16; k++) { (void)hipEventDestroy(r.ks.start[k]); (void)hipEventDestroy(r.ks.stop[k]); } }
        for (int k = 0; k < 3; k++) if (evRebuild[k]) (void)hipEventDestroy(evRebuild[k]);
        for (int k = 0; k < 2; k++) if (evStepDone[k]) (void)hipEventDestroy(evStepDone[k]);
        if (hDispFlags) (void)hipHostFree(hDispFlags);
        if (hNbPub) (void)hipHostFree(hNbPub);
        if (stream2) { (void)hipEventDestroy(evFork); (void)hipEventDestroy(evJoin); (void)hipEventDestroy(evPairA); (void)hipStreamDestroy(stream2); }
        if (ownStream) (void)hipStreamDestroy(stream);
    }
    // Real-space Ewald force factor of the forces-only pair kernels:
    //   [erfc(ar)/r + 2a/sqrt(pi) exp(-(ar)^2)] / r^2 = 1/r^3 - Bt(r^2),   Bt(r^2) = [erf(ar) - 2ar/sqrt(pi) exp(-(ar)^2)] / r^3,
    // Bt is an entire function of r^2 (Bt(0) = 4a^3/(3 sqrt(pi))), so a polynomial in t = 2 r^2/r2max - 1 (Chebyshev fit over
    // [0, (cutoff+skin+0.02)^2], converted to monomials in t, |t| <= 1) reproduces it: degree 11 in single precision (12 packed FMAs replace
    // v_exp + v_rcp + the A&S erfc polynomial), degree 16 in double (replaces libm erfc + exp).  At the benchmark's z = a (cutoff+skin+0.02)
    // = 2.94 they are good to 1e-7 resp. ~6e-12 of Bt(0); the residual grows fast with z (degree 11: 2e-5 of Bt(0) at z = 4), so the fit
    // (ewald_fit.h) measures it for this engine's alpha, cutoff and padding, and polyMask keeps a polynomial only where it passes the guard
    // stated there.  The energy polynomial Et and the LJPME dispersion polynomial Gd of double precision go the same way.
    static constexpr int EW_DEG = sizeof(Real) == 4 ? 11 : SNB_EW_DEG_F64;
    static_assert(kEwaldFitLJPME == SNB_LJPME && kEwDegF32 == 11 && kEwDegF64 == SNB_EW_DEG_F64 && kDispDegF64 == SNB_DISP_DEG_F64, "ewald_fit.h and the kernels disagree");
    static_assert(kPolyForce == SNB_POLY_FORCE && kPolyEnergy == SNB_POLY_ENERGY && kPolyDispersion == SNB_POLY_DISPERSION, "ewald_fit.h and the kernels disagree");
    double ewPoly[EW_DEG + 1] = {0}; double ewPolyE[14] = {0}; double dispPoly[21] = {0}; double ewR2Max = 1;
    int polyMask = 0;      // SNB_POLY_* bits: the polynomials this engine's kernels use (DirectParams::ewUsePoly, snb_stats.ewald_poly_mask)
    void buildEwaldPoly() {
        const double rmax = cfg.cutoff + std::max(cfg.neighbor_padding, 0.0) + 0.02;
        const EwaldFit fit = fitEwaldPolys<Real>(cfg.alpha, cfg.alpha_d, cfg.cutoff, rmax, cfg.method);
        ewR2Max = fit.r2max;
        for (int i = 0; i <= EW_DEG; i++) ewPoly[i] = fit.ewPoly[i];
        for (int i = 0; i < 14; i++) ewPolyE[i] = fit.ewPolyE[i];
        for (int i = 0; i < 21; i++) dispPoly[i] = fit.dispPoly[i];
        // the polynomials the kernels of this precision have a branch for: single and mixed precision Bt and Et, double Bt and (LJPME) Gd
        const int have = sizeof(Real) == 4 ? (SNB_POLY_FORCE | SNB_POLY_ENERGY) : (SNB_POLY_FORCE | (cfg.method == SNB_LJPME ? SNB_POLY_DISPERSION : 0));
        polyMask = sw.ewaldErfc ? 0 : (sw.ewaldPolyAlways ? have : (fit.use & have));
        if (sw.verbose) fprintf(stderr, "[snb] Ewald polynomials: force max r|dBt| %.3g (limit %.3g), energy |dEt| %.3g (%.3g), dispersion max r|dGd| %.3g (%.3g): mask %d in use\n", fit.pairF, fit.limF, fit.sysE, fit.limE, fit.pairD, fit.limD, polyMask);
    }
    bool isPme() const { return cfg.method == SNB_PME || cfg.method == SNB_LJPME; }
    bool isPeriodic() const { return cfg.method >= SNB_CutoffPeriodic; }

    void setParticles(const double* q, const double* sg, const double* ep, const int32_t* sub) override {
        bool subsetsChanged = !haveParticles;
        for (int i = 0; i < N; i++) {
            if (sub[i] < 0 || sub[i] >= nsub) throw HipError{"subset out of range"};
            if (subset[i] != sub[i]) subsetsChanged = true;      // subsets decide the sorted order and the block layout
        }
        charge.assign(q, q + N); sigma.assign(sg, sg + N); epsilon.assign(ep, ep + N); subset.assign(sub, sub + N);
        {      // meshes of subsets without atoms: exactly zero in exact arithmetic, but the plane path's inverse z pass transforms two meshes as one
               // complex line and leaves the partner's rounding in them -- a sharded rank, which reads every mesh it holds, skips them
            std::vector<int> count(nsub, 0);
            for (int i = 0; i < N; i++) count[sub[i]]++;
            emptyGrids = 0;
            for (size_t g = 0; g < hostGridSubset.size() && g < 64; g++) if (count[hostGridSubset[g]] == 0) emptyGrids |= 1ull << g;
        }
        basePDirty = true;
        haveParticles = true;
        // new charges / sigmas / epsilons alone (parameter offsets, updateParametersInContext) do not touch the neighbour structure:
        // they are refreshed in place (refreshValues) instead of going through a rebuild
        if (subsetsChanged) { needRebuild = true; paramsDirty = true; staticDirty = true; } else valuesDirty = true;
    }
    void setExceptions(int32_t m, const int32_t* pairs, const double* qq, const double* sg, const double* ep, const int32_t* f14) override {
        for (int k = 0; k < m; k++)
            if (pairs[2 * k] < 0 || pairs[2 * k] >= N || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= N || pairs[2 * k] == pairs[2 * k + 1]) throw HipError{"exception particle index out of range"};
        for (auto& o : offE) if (o.target >= m) throw HipError{"snb_set_exceptions: a parameter offset refers to an exception past the new count (clear or re-send the offsets first)"};
        std::vector<int32_t> np(pairs, pairs + 2 * (size_t)m);
        const bool pairsChanged = !haveExceptions || np != excPairs;      // the exclusion masks live in the tiles
        excPairs.swap(np); excQQ.assign(qq, qq + m); excSigma.assign(sg, sg + m); excEps.assign(ep, ep + m);
        if (f14) excForce14.assign(f14, f14 + m); else excForce14.assign(m, 0);
        haveExceptions = true;
        baseEDirty = true;
        if (pairsChanged) { needRebuild = true; paramsDirty = true; staticDirty = true; } else excValuesDirty = true;
    }
    void setParameterOffsets(int nGlob, int nP, const int32_t* pIdx, const int32_t* pGlob, const double* pDelta, int nE, const int32_t* eIdx, const int32_t* eGlob, const double* eDelta) override {
        if (nGlob < 0 || nP < 0 || nE < 0) throw HipError{"snb_set_parameter_offsets: negative count"};
        const int m = (int)(excPairs.size() / 2);
        for (int k = 0; k < nP; k++) if (pIdx[k] < 0 || pIdx[k] >= N || pGlob[k] < 0 || pGlob[k] >= nGlob) throw HipError{"snb_set_parameter_offsets: particle offset out of range"};
        for (int k = 0; k < nE; k++) if (eIdx[k] < 0 || eIdx[k] >= m || eGlob[k] < 0 || eGlob[k] >= nGlob) throw HipError{"snb_set_parameter_offsets: exception offset out of range (set the exceptions first)"};
        std::vector<Offset> nP_(nP), nE_(nE);
        for (int k = 0; k < nP; k++) nP_[k] = Offset{pIdx[k], pGlob[k], {pDelta[3 * k], pDelta[3 * k + 1], pDelta[3 * k + 2]}};
        for (int k = 0; k < nE; k++) nE_[k] = Offset{eIdx[k], eGlob[k], {eDelta[3 * k], eDelta[3 * k + 1], eDelta[3 * k + 2]}};
        auto same = [](const std::vector<Offset>& a, const std::vector<Offset>& b, bool structureOnly) {
            if (a.size() != b.size()) return false;
            for (size_t k = 0; k < a.size(); k++) {
                if (a[k].target != b[k].target || a[k].global != b[k].global) return false;
                if (!structureOnly && (a[k].d[0] != b[k].d[0] || a[k].d[1] != b[k].d[1] || a[k].d[2] != b[k].d[2])) return false;
            }
            return true;
        };
        if (nGlob == nGlobals && same(offP, nP_, false) && same(offE, nE_, false)) return;      // unchanged (copyParametersToContext re-sends everything)
        // an exception that carries an offset is a 1-4 interaction whatever its base values (Q6): a different set of them changes the 1-4 list
        const bool structure = nGlob != nGlobals || !same(offE, nE_, true) || !same(offP, nP_, true);
        offP.swap(nP_); offE.swap(nE_);
        if (nGlob != nGlobals) { nGlobals = nGlob; gValues.assign(nGlob, 0.0); globalsDirty = true; }
        offsetsDirty = true;
        if (structure) { needRebuild = true; paramsDirty = true; staticDirty = true; } else { valuesDirty = true; excValuesDirty = true; }
    }
    void setGlobalParameters(int n, const double* v) override {
        if (n != nGlobals) throw HipError{"snb_set_global_parameters: count differs from snb_set_parameter_offsets"};
        bool changed = false;
        for (int k = 0; k < n; k++) if (gValues[k] != v[k]) { gValues[k] = v[k]; changed = true; }
        if (!changed) return;
        globalsDirty = true;
        if (!offP.empty()) valuesDirty = true;
        if (!offE.empty()) excValuesDirty = true;
    }
    void setLambdas(const double* l) override {
        lambdas.assign(l, l + (size_t)S * 2);
        hLambdas.assign(lambdas.begin(), lambdas.end());
        pinned.upload(dLambdas, hLambdas, stream);      // (pinned slot per in-flight update: no synchronisation per lambda change, and the next call may overwrite hLambdas)
        if (ctx.on) pinned.upload(dLambdas64, lambdas, stream);      // (bound context: the total energy is weighted on the device, in double)
    }
    void setEnergySlices(const int32_t* m) override {
        for (int i = 0; i < S; i++) sliceNeedSel[i] = m[i] != 0;
        pinned.upload(dSliceNeedSel, sliceNeedSel, stream);      // (same device buffer, so captured graphs stay valid)
    }
    void setDispersion(const double* c) override {
        if (c) dispCoef.assign(c, c + S); else dispCoef.assign(S, 0.0);
        pinned.upload(dDispCoef, dispCoef, stream);      // read by the last kernel of an energy step
        dropGraph();
    }
    void setBox(const double* b) override {
        if (b[1] != 0 || b[2] != 0 || b[5] != 0) throw HipError{"box vectors must be in reduced (lower triangular) form"};
        bool changed = !haveBox;
        for (int i = 0; i < 9; i++) { if (box[i] != b[i]) changed = true; box[i] = b[i]; }
        haveBox = true;
        if (changed) needRebuild = true;
    }
    void setPositions(const void* pos, int isDevice, int isDouble, int stride4) override {
        if (ctx.on) { err = "snb_set_positions: a context is bound (snb_bind_context): the positions come from its posq"; throw (int)SNB_ERR_STATE; }
        posIsDouble = isDouble; posStride4 = stride4;
        const size_t bytes = (size_t)N * (stride4 ? 4 : 3) * (isDouble ? 8 : 4);
        if (isDevice) devUserPos = pos;
        else {
            ownedPos.resize(bytes);
            HIPCHECK(hipMemcpyAsync(ownedPos.p, pos, bytes, hipMemcpyHostToDevice, stream));
            HIPCHECK(hipStreamSynchronize(stream));   // the caller's array may be freed on return
            devUserPos = ownedPos.p;
        }
        havePositions = true;
    }
    void requestRebuild() override { needRebuild = true; }
    void sync() override { HIPCHECK(hipStreamSynchronize(stream)); }

    // ------------------------------------------------------------------------------------------
    // Neighbour structure: sort, blocks, per-atom gathered j-tiles, exclusion masks.  The host builder itself is host_lists.h
    // (buildHostLists): hostRebuild brings the positions and effective parameters back from the device and sends the lists up.
    // ------------------------------------------------------------------------------------------
    void rebuild() {
        const bool verbose = sw.verbose;
        const auto tr0 = std::chrono::steady_clock::now();
        if (verbose) { HIPCHECK(hipStreamSynchronize(stream)); }      // (diagnostic only: separates the wait for the queued steps from the rebuild's own time)
        const auto tr1 = std::chrono::steady_clock::now();
        dropGraph();   // buffers may move and every kernel argument block changes
        if (staticDirty) uploadStatic();
        gpuBuilt = false;
        if (cfg.host_neighbor_build || !gpuRebuild()) hostRebuild();
        if (verbose) fprintf(stderr, "[snb] rebuild: waited %.0f us for the queued steps, then %.0f us (host) for the build itself; device time %.0f us\n",
                             std::chrono::duration<double, std::micro>(tr1 - tr0).count(), std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tr1).count(), stats.last_rebuild_ms * 1e3);
        pmeCells.resize(Npad);   // per-slot scratch is sized here: nothing may allocate while a step is being captured into a graph
        if (isPme()) { if (!dStrayCount.p) { dStrayCount.resize(2); HIPCHECK(hipMemsetAsync(dStrayCount.p, 0, 2 * sizeof(int), stream)); } planOwnSpread(pme); if (cfg.method == SNB_LJPME) planOwnSpread(dpme); planPlaneTable(pme); if (cfg.method == SNB_LJPME) planPlaneTable(dpme);
            if (verbose) { describeMesh("coulomb", pme); if (cfg.method == SNB_LJPME) describeMesh("dispersion", dpme); } }
        posRef.resize(Npad);
        HIPCHECK(hipMemcpyAsync(posRef.p, posq.p, sizeof(T4) * (size_t)Npad, hipMemcpyDeviceToDevice, stream));
        if (hDispFlags[1]) listOverruns++;      // an atom had moved more than skin/2 before this rebuild came
        hDispFlags[0] = hDispFlags[1] = 0;
        flagsResetPending = false;      // (the queue has been drained: a reset enqueued at an earlier exchange has run)
    }

    void hostRebuild() {
        auto t0 = std::chrono::steady_clock::now();
        if (ctx.on) HIPCHECK(hipStreamSynchronize(stream));      // (the user-order copy of the bound positions was staged on the engine's stream)
        std::vector<double> hp((size_t)N * 3);
        auto fetch = [&](auto type) {
            const int st = posStride4 ? 4 : 3;
            std::vector<decltype(type)> tmp((size_t)N * st);
            HIPCHECK(hipMemcpy(tmp.data(), devUserPos, sizeof(type) * tmp.size(), hipMemcpyDeviceToHost));
            for (int i = 0; i < N; i++) for (int d = 0; d < 3; d++) hp[3 * (size_t)i + d] = tmp[(size_t)i * st + d];
        };
        if (posIsDouble) fetch(double()); else fetch(float());
        HostListInput in;
        in.n = N; in.nsub = nsub; in.subset = subset.data(); in.pos = hp.data();
        for (int i = 0; i < 9; i++) in.box[i] = box[i];
        in.periodic = isPeriodic(); in.noCutoff = cfg.method == SNB_NoCutoff; in.listRadius = cfg.cutoff + cfg.neighbor_padding;
        if (isPme() && nGrids > 0) { in.mesh[0] = pme.d.nx; in.mesh[1] = pme.d.ny; in.mesh[2] = pme.d.nz; }
        in.exclStart = hExclStart.data(); in.exclList = hExclList.data(); in.slotOfSubset = hSlotOfSubset.data();
        in.shardBegin = shardBegin; in.shardEnd = shardEnd; in.shardPeriod = shardPeriod;
        const HostLists L = buildHostLists(in);
        Npad = L.npad; numBlocks = L.numBlocks; wrapMode = L.wrapMode; colCells[0] = L.colCells[0]; colCells[1] = L.colCells[1];
        numTiles = L.numTiles; numMaskTiles = L.numMaskTiles; shardTiles = L.shardTiles; numWorkItems = (int)L.workItems.size();
        if (Npad >= (1 << SNB_JSHIFT_BITS) - 1) throw HipError{"too many atoms for the 25-bit tile index"};      // (L's tile entries are then garbage; nothing of L has been uploaded)
        // sorted parameter arrays (effective parameter values: formed on the device, fetched for this host-side path)
        std::vector<Real> effQ(N); std::vector<T2> effSE(N);
        if (N > 0) { HIPCHECK(hipMemcpy(effQ.data(), dUCharge.p, sizeof(Real) * N, hipMemcpyDeviceToHost)); HIPCHECK(hipMemcpy(effSE.data(), dUSigEps.p, sizeof(T2) * N, hipMemcpyDeviceToHost)); }
        std::vector<T4> hPosq(Npad); std::vector<T2> hSigeps(Npad); std::vector<Real> hOff((size_t)Npad * 3, Real(0));
        for (int s = 0; s < Npad; s++) {
            const int u = L.sortedToUser[s];
            if (u >= 0) {
                hPosq[s].x = (Real)L.wrapped[3 * (size_t)u]; hPosq[s].y = (Real)L.wrapped[3 * (size_t)u + 1]; hPosq[s].z = (Real)L.wrapped[3 * (size_t)u + 2]; hPosq[s].w = effQ[u];
                hSigeps[s] = effSE[u];
                for (int d = 0; d < 3; d++) hOff[3 * (size_t)s + d] = (Real)L.imageOffset[3 * (size_t)u + d];
            } else {   // parked padding atom: zero parameters, far away, distinct
                hPosq[s].x = (Real)(1e9 + 1e6 * (s & 4095)); hPosq[s].y = (Real)2e9; hPosq[s].z = (Real)-3e9; hPosq[s].w = 0;
                hSigeps[s].x = 0; hSigeps[s].y = 0;
            }
        }
        static_assert(kJShiftBits == SNB_JSHIFT_BITS && kJCodeCenter == SNB_JCODE_CENTER, "host_lists.h packs the tile entries the kernels unpack");
        posq.upload(hPosq, stream); sigeps.upload(hSigeps, stream); imageOffset.upload(hOff, stream);
        dSortedToUser.upload(L.sortedToUser, stream); dUserToSorted.upload(L.userToSorted, stream);
        blockSubset.upload(L.blockSubset, stream); upload(workItems, L.workItems, stream);
        tileJ.upload(L.tileJ, stream); upload(tileInfo, L.tileInfo, stream); masks.upload(L.masks, stream);
        atomSubset.upload(L.atomSubset, stream); atomGrid.upload(L.atomGrid, stream);
        if (colCells[0] > 0) upload(colRange, L.colRange, stream);
        layoutForces();
        HIPCHECK(hipStreamSynchronize(stream));
        needRebuild = false; paramsDirty = false; stepsSinceRebuild = 0;
        stats.n_rebuilds++; stats.n_host_rebuilds++;
        stats.last_rebuild_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }

    // Static (sort-independent) device data: 1-4 list and exclusion CSR in USER indices (Q6:
    // ReferenceNonbondedSlicingKernels.cpp:99-112, 129-131), per-atom parameters in user order, the grid slot of every subset.
    // 1-4 list in user order: the exceptions with non-zero base parameters, or flagged by the caller, or carrying a parameter offset (Q6).
    // Structure only (pairs, slices, base values, offsets in CSR per 1-4 entry); the values are formed on the device (syncParameters).
    void upload14() {
        const size_t m = excPairs.size() / 2;
        // captured step graphs bake in the 1-4 count, the list pointers and the grid of the list blocks: same pairs with a different set of
        // non-zero / flagged exceptions changes all three, so the graphs go whenever any of them moved
        const int oldN14 = n14; const void* const oldPairs = pairs14.p; const void* const oldParams = params14.p;
        std::vector<char> hasOffset(m, 0);
        for (auto& o : offE) hasOffset[o.target] = 1;
        std::vector<int2> p14; std::vector<double> b14; std::vector<int> sl14, where(m, -1);
        auto sl = [](int a, int b) { return a > b ? a * (a + 1) / 2 + b : b * (b + 1) / 2 + a; };
        for (size_t k = 0; k < m; k++) {
            const int a = excPairs[2 * k], b = excPairs[2 * k + 1];
            if (excQQ[k] != 0.0 || excEps[k] != 0.0 || excForce14[k] || hasOffset[k]) {
                where[k] = (int)p14.size();
                p14.push_back(make_int2(a, b));
                b14.push_back(excQQ[k]); b14.push_back(excSigma[k]); b14.push_back(excEps[k]);
                sl14.push_back(sl(subset[a], subset[b]));
            }
        }
        n14 = (int)p14.size(); nExcl = (int)m;
        std::vector<int> start(n14 + 1, 0), glob(offE.size()); std::vector<double> delta(3 * offE.size());
        for (auto& o : offE) start[where[o.target] + 1]++;
        for (int k = 0; k < n14; k++) start[k + 1] += start[k];
        { std::vector<int> fill(n14, 0); for (auto& o : offE) { const int e = where[o.target], at = start[e] + fill[e]++; glob[at] = o.global; for (int d = 0; d < 3; d++) delta[3 * (size_t)at + d] = o.d[d]; } }
        pairs14.upload(p14, stream); dBase14.upload(b14, stream); dSlice14.upload(sl14, stream);
        dOff14Start.upload(start, stream); dOff14Global.upload(glob, stream); dOff14Delta.upload(delta, stream);
        params14.resize(n14);
        stats.n_14 = n14; stats.n_exclusions = nExcl;
        HIPCHECK(hipStreamSynchronize(stream));      // (host staging vectors go out of scope)
        baseEDirty = false;
        if (n14 != oldN14 || pairs14.p != oldPairs || params14.p != oldParams) dropGraph();
    }
    void uploadParticleBase() {
        std::vector<double> hb(3 * (size_t)N);
        for (int i = 0; i < N; i++) { hb[3 * (size_t)i] = charge[i]; hb[3 * (size_t)i + 1] = sigma[i]; hb[3 * (size_t)i + 2] = epsilon[i]; }
        std::vector<int> start((size_t)N + 1, 0), glob(offP.size()); std::vector<double> delta(3 * offP.size());
        for (auto& o : offP) start[o.target + 1]++;
        for (int i = 0; i < N; i++) start[i + 1] += start[i];
        { std::vector<int> fill(N, 0); for (auto& o : offP) { const int at = start[o.target] + fill[o.target]++; glob[at] = o.global; for (int d = 0; d < 3; d++) delta[3 * (size_t)at + d] = o.d[d]; } }
        dBaseP.upload(hb, stream); dOffPStart.upload(start, stream); dOffPGlobal.upload(glob, stream); dOffPDelta.upload(delta, stream);
        dUCharge.resize(N); dUSigEps.resize(N); dParamSums.resize((3 * (size_t)nsub + 1) * (1 + SNB_PARAM_SUM_ROWS)); dFixScale.resize(4);
        HIPCHECK(hipStreamSynchronize(stream));
        basePDirty = false;
    }
    // Effective parameters on the device, from whatever changed: base values / offsets (re-uploaded), global parameter values (a few
    // doubles).  Enqueued on the engine's stream ahead of the step; nothing here waits for the GPU unless a base array was re-uploaded.
    void syncParameters(bool particles, bool exceptions) {
        if (offsetsDirty) { basePDirty = true; baseEDirty = true; offsetsDirty = false; }
        if (basePDirty) { uploadParticleBase(); particles = true; }
        if (baseEDirty) { upload14(); exceptions = true; }
        if (globalsDirty) {
            dGlobals.resize(std::max(nGlobals, 1));
            if (nGlobals > 0) pinned.copy(dGlobals.p, gValues.data(), sizeof(double) * nGlobals, stream);
            globalsDirty = false;
        }
        if (particles) {
            // headroom of the spreader's 32-bit fixed point, per mesh: max(16, 8 x atoms per mesh cell) (misc.hip, k_fixScale)
            const double forced = sw.fixHeadroom;
            auto headroom = [&](const PmePlanDims& d) { const double cells = (double)std::max(d.nx, 1) * std::max(d.ny, 1) * std::max(d.nz, 1); return forced > 0 ? forced : std::max(16.0, 8.0 * (double)N / cells); };
            launchParticleParams<Real>(N, nsub, dBaseP.p, offP.empty() ? nullptr : dOffPStart.p, dOffPGlobal.p, dOffPDelta.p, dGlobals.p, dUSubset.p, dUCharge.p, dUSigEps.p,
                                       dParamSums.p, dFixScale.p, headroom(pme.d), headroom(dpme.d), stream);
        }
        if (exceptions) launchExceptionParams<Real>(n14, dBase14.p, offE.empty() ? nullptr : dOff14Start.p, dOff14Global.p, dOff14Delta.p, dGlobals.p, dSlice14.p, params14.p, stream);
    }
    // New parameter VALUES with the same subsets / exception pairs (copyParametersToContext, parameter offsets: the reference recomputes
    // them on the device per changed global parameter, nonbondedParameters.cc:4-179): effective values on the device, then the sorted
    // per-atom arrays are rewritten in place -- no re-sort, no tile rebuild, no host synchronisation, and the captured step graphs stay
    // valid (nothing derived from the values is baked into them: the spreader reads its fixed-point scale from device memory).
    void refreshValues() {
        const bool particles = valuesDirty;
        syncParameters(valuesDirty, excValuesDirty);
        if (particles) launchRefreshParams<Real>(dSortedToUser.p, dUCharge.p, dUSigEps.p, posq.p, sigeps.p, Npad, stream);
        valuesDirty = excValuesDirty = false;
    }

    void uploadStatic() {
        const size_t m = excPairs.size() / 2;
        hExclStart.assign((size_t)N + 1, 0); hExclList.resize(2 * m);
        for (size_t k = 0; k < m; k++) {
            const int a = excPairs[2 * k], b = excPairs[2 * k + 1];
            hExclStart[a + 1]++; hExclStart[b + 1]++;
        }
        for (int i = 0; i < N; i++) hExclStart[i + 1] += hExclStart[i];
        { std::vector<int> fill(N, 0); for (size_t k = 0; k < m; k++) { const int a = excPairs[2 * k], b = excPairs[2 * k + 1]; hExclList[hExclStart[a] + fill[a]++] = b; hExclList[hExclStart[b] + fill[b]++] = a; } }
        exclStart.upload(hExclStart, stream); exclList.upload(hExclList, stream);
        // user-order parameters: formed on the device from base values, offsets and global parameters
        dUSubset.upload(std::vector<int>(subset.begin(), subset.end()), stream);
        HIPCHECK(hipStreamSynchronize(stream));
        basePDirty = baseEDirty = true;
        syncParameters(true, true);
        hSlotOfSubset.assign(nsub, -1);
        if (cfg.shard_count == 1) std::iota(hSlotOfSubset.begin(), hSlotOfSubset.end(), 0); else for (size_t g = 0; g < ownedSubsets.size(); g++) hSlotOfSubset[ownedSubsets[g]] = (int)g;
        dSlotOfSubset.upload(hSlotOfSubset, stream);
        HIPCHECK(hipStreamSynchronize(stream));
        staticDirty = false;
        npadPredict = 0;      // (subsets or exclusions may have changed: the next rebuild waits for its padded count again)
    }

    // ------------------------------------------------------------------------------------------
    // GPU neighbour build (neighbor.hip): rectangular periodic boxes with cutoff.  Returns false when the
    // host builder must take over (per-pair-wrap regime, gather-capacity overflow).
    // ------------------------------------------------------------------------------------------
    // the totals of a build through mapped host memory: spins on the sequence number k_nbPublish writes last (falls back to a copy after
    // SNB_NB_PUBLISH_WAIT_MS, default 2000).  The copy goes on `buildStream`, the stream the build was enqueued on, and waits for it: only
    // there is it ordered after the build's counters (a side build writes them on streamBuild, not on the live step stream)
    void waitForTotals(int seq, int* h, hipStream_t buildStream) {
        const int waitMs = sw.nbPublishWaitMs;
        volatile int* pub = hNbPub;
        if (waitMs > 0) {
            const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(waitMs);
            while (pub[8] != seq && std::chrono::steady_clock::now() < deadline) cpuRelax();
            if (pub[8] == seq) { for (int k = 0; k < 8; k++) h[k] = pub[k]; return; }
        }
        HIPCHECK(hipMemcpyAsync(h, dCounters.p, sizeof(int) * 8, hipMemcpyDeviceToHost, buildStream));
        HIPCHECK(hipStreamSynchronize(buildStream));
        if (sw.verbose) fprintf(stderr, "[snb] totals of build %d not published within %d ms: copied on the %s stream (tiles %d, work items %d + %d, overflow %d, padded %d)\n",
                             seq, waitMs, buildStream == streamBuild ? "side-build" : "build", h[0], h[1], h[4], h[3], h[7]);
    }
    // a build whose totals are in: host-side counts, the next prediction, statistics
    void acceptBuild(const int* h, float sortMs) {
        numTiles = h[0]; numWorkItems = h[1] + h[4]; numMaskTiles = h[2]; wrapMode = false;
        if (sw.debugWork) {      // consistency of the work list: the items must cover every tile exactly once
            std::vector<int4> hw(numWorkItems);
            HIPCHECK(hipMemcpy(hw.data(), workItems.p, sizeof(int4) * numWorkItems, hipMemcpyDeviceToHost));
            long long sumZ = 0; int hist[9] = {0};
            for (auto& w : hw) { sumZ += w.z; hist[std::min(std::max(w.z, 0), 8)]++; }
            fprintf(stderr, "[snb] work list: %d items (%d full + %d partial), tiles %d, sum of item sizes %lld, sizes 1..8:", numWorkItems, h[1], h[4], (int)numTiles, sumZ);
            for (int k = 1; k <= 8; k++) fprintf(stderr, " %d", hist[k]);
            fprintf(stderr, "\n");
        }
        shardTiles = numTiles;      // the builder only emitted the blocks this engine owns
        // next rebuild's array size: this count + 0.4 % + 8 blocks (c3: 300 k atoms move its count by a few blocks between rebuilds); never shrinking,
        // so that the buffers -- and the step graph's arguments -- stay where they are
        lastPadCount = h[7];
        npadPredict = std::max(npadPredict, ((int)(h[7] * 1.004) + 256 + 31) / 32 * 32);
        if (sw.nbPredictShort > 0) npadPredict = std::max(32, h[7] - 32 * sw.nbPredictShort);
        stats.n_rebuilds++;
        float gpuMs = 0;   // device time of the build (the host clock would also count the queued steps this call waited for)
        HIPCHECK(hipEventElapsedTime(&gpuMs, evRebuild[0], evRebuild[1]));
        stats.last_rebuild_ms = gpuMs + sortMs;
    }

    // ---- the rebuild beside the steps ----
    void swapListSets() {
        auto exch = [](auto& a, auto& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); };
        exch(dUserToSorted, shadow.dUserToSorted); exch(dSortedToUser, shadow.dSortedToUser); exch(atomSubset, shadow.atomSubset); exch(atomGrid, shadow.atomGrid);
        exch(blockSubset, shadow.blockSubset); exch(tileJ, shadow.tileJ); exch(colRange, shadow.colRange); exch(posq, shadow.posq); exch(posRef, shadow.posRef);
        exch(sigeps, shadow.sigeps); exch(imageOffset, shadow.imageOffset); exch(tileInfo, shadow.tileInfo); exch(workItems, shadow.workItems); exch(masks, shadow.masks);
    }
    // whether the rebuild that falls due `sw.sideLead` executes from now may be built beside the steps: a list built on the GPU with a predicted
    // padded count is in use, nothing but the positions has changed since, fixed interval.  (Displacement-triggered rebuilds were given side
    // builds too, timed by a guess of the watch's next interval -- built, parity green, and slower than rebuilding in line at the watch's own
    // pace: 0.3634 against 0.3539 ms per step on c3, the guess brings rebuilds forward and a third of them still came in line.  Removed.)
    bool sideBuildPossible() const {
        return sw.sideRebuild && !sidePending && gpuBuilt && cfg.rebuild_interval > sw.sideLead + 1 && cfg.neighbor_padding > 0 && isPeriodic() && !cfg.host_neighbor_build && !cfg.disable_graph
               && !needRebuild && !paramsDirty && !staticDirty && !valuesDirty && !excValuesDirty && npadPredict > 0 && npadPredict == Npad && hNbPub && dNbPub && devUserPos;
    }
    void ensureBuildStream() {
        if (streamBuild) return;
        int lo = 0, hi = 0;
        HIPCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
        // (normal priority: at the lowest the build crawls and the steps end up waiting for it, at the highest its kernels push the tile kernel aside)
        HIPCHECK(hipStreamCreateWithPriority(&streamBuild, hipStreamNonBlocking, sw.sidePrioHigh ? hi : (sw.sidePrioLow ? lo : (lo + hi) / 2)));
        HIPCHECK(hipEventCreateWithFlags(&evSnap, hipEventDisableTiming)); HIPCHECK(hipEventCreateWithFlags(&evBuilt, hipEventDisableTiming)); HIPCHECK(hipEventCreateWithFlags(&evFlagsReset, hipEventDisableTiming));
    }
    // Enqueues the whole build on streamBuild, into the shadow buffers.  Nothing the steps use is touched; the host does not wait.
    // src == null (MD, fixed interval): the positions are copied aside first, in stream order -- the positions of the step just enqueued -- and
    // the build follows that copy.  src != null (frame batches): the build reads src, positions in the current format that the caller keeps
    // valid, and the caller has already ordered streamBuild behind the last step that used the shadow set and behind the arrival of src.
    // When the list comes into use is the caller's decision as well: it calls finishSideBuild.
    void startSideBuild(const void* src = nullptr) {
        ensureBuildStream();
        if (!src) {
            const size_t bytes = (size_t)N * (posStride4 ? 4 : 3) * (posIsDouble ? 8 : 4);
            posSnap.resize(bytes);
            if (ctx.on) stageCtxPositions(posSnap.p);      // (bound context: the snapshot is taken in USER order, so the build does not depend on the context's order)
            else HIPCHECK(hipMemcpyAsync(posSnap.p, devUserPos, bytes, hipMemcpyDeviceToDevice, stream));
            HIPCHECK(hipEventRecord(evSnap, stream));
            HIPCHECK(hipStreamWaitEvent(streamBuild, evSnap, 0));
            src = posSnap.p;
        }
        const hipStream_t liveStream = stream; const void* livePos = devUserPos;
        const int liveCells[2] = {colCells[0], colCells[1]};
        swapListSets(); stream = streamBuild; devUserPos = src; sideBuilding = true;
        bool ok = false, built = false;
        {
            ScopeExit live([&] { sideBuilding = false; stream = liveStream; devUserPos = livePos; swapListSets(); if (!built) { colCells[0] = liveCells[0]; colCells[1] = liveCells[1]; } });
            ok = gpuRebuild();
            if (ok) { posRef.resize(Npad); HIPCHECK(hipMemcpyAsync(posRef.p, posq.p, sizeof(T4) * (size_t)Npad, hipMemcpyDeviceToDevice, stream)); }
            HIPCHECK(hipEventRecord(evBuilt, stream));
            built = ok;
        }
        if (!ok) HIPCHECK(hipEventSynchronize(evBuilt));      // (whatever was enqueued has finished with the scratch arrays)
        sidePending = ok;
        if (sw.verbose && ok) fprintf(stderr, "[snb] side build started after execute %lld\n", stepCounter - 1);
    }
    // drops a pending side build (its result will not be used): waits until it has finished with the scratch arrays
    void cancelSideBuild() {
        if (!sidePending) return;
        HIPCHECK(hipEventSynchronize(evBuilt));
        sidePending = false; sideDiscarded++;
    }
    // The rebuild has fallen due and a side build is pending: true = its list is now the one in use (nothing else to do); false = it failed
    // (padded count or a partition over its capacity) and the caller rebuilds in line.
    bool finishSideBuild() {
        sidePending = false;
        int h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        waitForTotals(sideSeq, h, streamBuild);      // (a fallback copy must wait for the side build, not for the live steps)
        HIPCHECK(hipEventSynchronize(evBuilt));      // (returns at once: the totals are the build's last kernel but one)
        const bool verbose = sw.verbose;
        if (h[7] < N || (h[7] & 31) || h[7] > Npad || h[3] != 0 || sw.sideReject) {
            if (verbose) fprintf(stderr, "[snb] side rebuild discarded (padded count %d of %d, overflow flag %d): rebuilding in line\n", h[7], Npad, h[3]);
            if (h[7] > Npad) { npadPredict = 0; padMispredictions++; }
            sideDiscarded++;
            return false;
        }
        HIPCHECK(hipStreamWaitEvent(stream, evBuilt, 0));      // stream order for the steps that follow
        dropGraph();      // every kernel argument block changes
        swapListSets();
        acceptBuild(h, 0.f);
        wrapMode = false; gpuBuilt = true; needRebuild = false; stepsSinceRebuild = 0;
        launchDispFlagsReset(dDispFlags, stream);      // (in stream order: steps on the old list may still be queued, and their flags belong to it)
        HIPCHECK(hipEventRecord(evFlagsReset, stream)); flagsResetPending = true;      // (until then the host copy still shows the old list's flags)
        sideBuilds++;
        if (verbose) fprintf(stderr, "[snb] side-built list in use from execute %lld\n", stepCounter);
        return true;
    }

    bool gpuRebuild() {
        if (cfg.method == SNB_NoCutoff || N < 64) return false;
        if (sideBuilding && !(npadPredict > 0 && npadPredict == Npad && !sw.nbSyncPadded)) return false;
        if (sw.hostTriclinic && (!isPeriodic() || !(box[3] == 0 && box[6] == 0 && box[7] == 0))) return false;
        const double R = cfg.cutoff + cfg.neighbor_padding;
        // The cell the builder works in: the periodic box, or -- CutoffNonPeriodic -- a rectangular cell around the atoms' bounding box with
        // more than a list radius of empty margin on every side, so that no periodic image of anything is ever in reach
        double cell[9], origin[3] = {0, 0, 0};
        for (int i = 0; i < 9; i++) cell[i] = box[i];
        if (!isPeriodic()) {
            dExtent.resize(6);
            launchExtent(devUserPos, posIsDouble, posStride4, N, dExtent.p, stream);
            int h[6];
            HIPCHECK(hipMemcpyAsync(h, dExtent.p, sizeof(h), hipMemcpyDeviceToHost, stream));
            HIPCHECK(hipStreamSynchronize(stream));
            auto dec = [](int i) { i = i >= 0 ? i : i ^ 0x7FFFFFFF; float f; std::memcpy(&f, &i, 4); return (double)f; };
            const double margin = R + 0.5 * cfg.neighbor_padding + 0.05;
            for (int d = 0; d < 3; d++) {
                const double lo = dec(h[d]), hi = dec(h[3 + d]);
                if (!(hi >= lo) || !std::isfinite(lo) || !std::isfinite(hi)) return false;
                origin[d] = lo - margin;
                cell[4 * d] = (hi - lo) + 2.0 * margin;
            }
            cell[1] = cell[2] = cell[3] = cell[5] = cell[6] = cell[7] = 0;
        }
        const double* box = cell;      // (shadows the member for the rest of the build)
        const double diag[3] = {box[0], box[4], box[8]}; const int mesh[3] = {pme.d.nx, pme.d.ny, pme.d.nz}, noMesh[3] = {0, 0, 0};
        const SortColumns sc = sortColumns(N, diag, (isPme() && nGrids > 0) ? mesh : noMesh);
        for (int d = 0; d < 3; d++) if (!(4.0 * sc.aTarget + 2 * R < box[4 * d])) return false;   // tile-image scheme needs extent + 2R < L (checked exactly on the GPU too)
        auto t0 = std::chrono::steady_clock::now();
        const int ncx = sc.ncx, ncy = sc.ncy;
        colCells[0] = sc.colCells[0]; colCells[1] = sc.colCells[1];
        // phase A: sort and block segmentation (the padded atom count depends on where the sorted order jumps)
        dUserToSorted.resize(N);
        colRange.resize((size_t)nsub * ncx * ncy); dZIndex.resize((size_t)nsub * ncx * ncy * 65);
        dWrapped.resize((size_t)3 * N); dOffsetU.resize((size_t)3 * N); dKeysIn.resize(N); dKeysOut.resize(N); dValsIn.resize(N); dValsOut.resize(N);
        dScanA.resize(N); dScanB.resize(N); dCounters.resize(32 * 65);
        const size_t tempBytes = nbSortTempBytes<Real>(N);
        dSortTemp.resize(tempBytes);
        NbParams<Real> p;
        std::memset(&p, 0, sizeof(p));
        p.nAtoms = N; p.nSubsets = nsub; p.ncx = ncx; p.ncy = ncy;
        p.subsetBits = 1; while ((1 << p.subsetBits) < nsub) p.subsetBits++;
        p.colBits = 1; while ((1ll << p.colBits) < (long long)ncx * ncy) p.colBits++;
        for (int i = 0; i < 9; i++) p.boxm[i] = box[i];
        for (int d = 0; d < 3; d++) p.origin[d] = origin[d];
        for (int i = 0; i < 9; i++) tileCell[i] = box[i];
        // The builder measures in float whatever the engine's precision, on coordinates held relative to the cell and shifted by up to two
        // lattice vectors; the pair kernel then decides r < cutoff in the engine's own precision.  A pair within that float rounding of the
        // list radius (a double engine without a skin: a pair at cutoff (1 - 1e-9)) must still be in the list, so the radius is widened by a
        // bound on the rounding: coordinates reach 3 * span (span: the longest coordinate range of the cell), a float there is spaced
        // 3 * span * 2^-23, and a component of a difference carries about three such roundings (stored i and j, the image shift), the block
        // boxes two more; times sqrt(3) for the distance, plus the rounding of the squares and their sum.  1.5e-4 nm in a 40 nm cell.
        double span = 0;
        for (int d = 0; d < 3; d++) span = std::max(span, std::fabs(box[d]) + std::fabs(box[3 + d]) + std::fabs(box[6 + d]));
        const double listSlack = (32.0 * span + 4.0 * R) * std::ldexp(1.0, -23);
        p.listCutoff = (float)(R + listSlack);
        p.boxWalk = sw.nbBoxWalk ? 1 : 0;
        p.jumpDist = (float)(2.0 * std::sqrt(2.0) * std::max(box[0] / ncx, box[4] / ncy));   // neighbours along the sort path of a dense region are closer than this
        p.uSubset = dUSubset.p; p.uCharge = dUCharge.p; p.uSigEps = dUSigEps.p; p.uExclStart = exclStart.p; p.uExclList = exclList.p;
        p.slotOfSubset = dSlotOfSubset.p;
        p.wrapped = dWrapped.p; p.offsetU = dOffsetU.p; p.keysIn = dKeysIn.p; p.keysOut = dKeysOut.p; p.valsIn = dValsIn.p; p.valsOut = dValsOut.p;
        p.segKey = dValsIn.p; p.segStart = dScanA.p; p.padExtra = dScanB.p; p.padBefore = dScanA.p;   // valsIn is dead once the sort has run
        dScanC.resize(N); p.blockWide = dScanC.p; p.blockWideOut = dScanC.p;
        for (int d = 0; d < 3; d++) p.maxHalfExtent[d] = (float)(0.45 * (box[4 * d] - 2.0 * R));   // extent <= 0.9 (L - 2R)
        p.userToSorted = dUserToSorted.p; p.colRange = colRange.p; p.zIndex = dZIndex.p; p.counters = dCounters.p;
        if (!evRebuild[0]) { HIPCHECK(hipEventCreate(&evRebuild[0])); HIPCHECK(hipEventCreate(&evRebuild[1])); HIPCHECK(hipEventCreate(&evRebuild[2])); }
        HIPCHECK(hipEventRecord(evRebuild[0], stream));
        {
            // Phase A is ~30 small launches (key pass, radix sort, segmentation scans) with nothing but launch latency between them:
            // captured once per (parameters, buffers, position pointer) and replayed, the way the step itself is.  Any failure to
            // capture (a library call that is not capturable) falls back to plain launches for good.
            struct SortKey { NbParams<Real> p; const void* pos; int isDouble, stride4; void* temp; size_t tempBytes; };
            static_assert(std::is_trivially_copyable<SortKey>::value, "SortKey is compared bytewise");
            SortKey key; std::memset(&key, 0, sizeof(key));
            key.p = p; key.pos = devUserPos; key.isDouble = posIsDouble; key.stride4 = posStride4; key.temp = dSortTemp.p; key.tempBytes = tempBytes;
            const bool noSortGraph = sw.noSortGraph;
            bool replayed = false;
            // (round 4: a replayed phase-A graph once left 32 N padded slots -- its memset node for blockWideOut had stopped zeroing after other
            // graphs with memset nodes had been instantiated; phase A now zero-fills with a kernel, misc.hip launchZeroFill.  `sortGraphSuspect`
            // is the insurance that caught nothing since: a padded count that doubles out of a replayed graph is built once more without it.)
            // (above 2^20 keys rocprim's radix sort takes its onesweep path, which clears its histogram with hipMemsetAsync -- a memset node if
            // captured: such systems issue phase A as plain launches)
            if (!noSortGraph && !sortGraphBroken && !cfg.disable_graph && !sortGraphSuspect && !plainSort && N <= (1 << 20)) {
                hipGraphExec_t sortGraphExec = nullptr;
                for (auto& g : sortGraphs) if (g.key.size() == sizeof(key) && std::memcmp(g.key.data(), &key, sizeof(key)) == 0) sortGraphExec = g.exec;
                if (!sortGraphExec) {
                    hipGraph_t graph = nullptr;
                    if (hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                        bool threw = false;
                        try { launchNeighborSort<Real>(p, devUserPos, posIsDouble, posStride4, dSortTemp.p, tempBytes, stream); }
                        catch (...) { threw = true; }      // never leave the caller's stream in capture mode
                        hipError_t endErr = hipStreamEndCapture(stream, &graph);
                        if (threw) { endErr = hipErrorUnknown; (void)hipGetLastError(); }
                        if (endErr == hipSuccess && graph && hipGraphInstantiate(&sortGraphExec, graph, nullptr, nullptr, 0) == hipSuccess) {
                            SortGraph g; g.key.assign(reinterpret_cast<const unsigned char*>(&key), reinterpret_cast<const unsigned char*>(&key) + sizeof(key)); g.exec = sortGraphExec;
                            if (sortGraphs.size() < 4) sortGraphs.push_back(g);
                            else { (void)hipGraphExecDestroy(sortGraphs[sortGraphVictim].exec); sortGraphs[sortGraphVictim] = g; sortGraphVictim = (sortGraphVictim + 1) % 4; }
                        } else { sortGraphExec = nullptr; sortGraphBroken = true; (void)hipGetLastError(); }
                        if (graph) (void)hipGraphDestroy(graph);
                    } else { sortGraphBroken = true; (void)hipGetLastError(); }
                }
                if (sortGraphExec) { HIPCHECK(hipGraphLaunch(sortGraphExec, stream)); replayed = true; }
            }
            if (!replayed) launchNeighborSort<Real>(p, devUserPos, posIsDouble, posStride4, dSortTemp.p, tempBytes, stream);
        }
        HIPCHECK(hipEventRecord(evRebuild[2], stream));
        // The padded atom count depends on where the sorted order jumps, i.e. it is known on the device only.  Round 4: from the second
        // rebuild on the arrays are sized by the previous count plus a margin (a few spare all-padding blocks at the end) and the build
        // goes on without waiting; the exact count comes back with the tile counters below, and an overflow (k_nbScatter counts the
        // atoms that did not fit) repeats the rebuild with the exact count.  Saves one host round trip (~75 us) per rebuild.
        const bool predicted = npadPredict > 0 && !sw.nbSyncPadded;
        if (predicted) Npad = npadPredict;
        else {
            int npadDev = 0;
            HIPCHECK(hipMemcpyAsync(&npadDev, dCounters.p + 7, sizeof(int), hipMemcpyDeviceToHost, stream));
            HIPCHECK(hipStreamSynchronize(stream));
            if (npadDev < N || (npadDev & 31)) throw HipError{"neighbour build: inconsistent padded atom count"};
            Npad = npadDev;
        }
        numBlocks = Npad / 32;
        if (Npad >= (1 << SNB_JSHIFT_BITS) - 1) throw HipError{"too many atoms for the 25-bit tile index"};
        // outputs / scratch sized by the padded count
        posq.resize(Npad); sigeps.resize(Npad); imageOffset.resize((size_t)3 * Npad);
        dSortedToUser.resize(Npad); atomSubset.resize(Npad); atomGrid.resize(Npad); blockSubset.resize(numBlocks);
        layoutForces();
        dBlockCenter.resize((size_t)3 * numBlocks); dBlockHalf.resize((size_t)3 * numBlocks);
        if (tileCap < (size_t)numBlocks * 40) tileCap = (size_t)numBlocks * 40;
        if (tileCap < 64 * 128) tileCap = 64 * 128;      // 64 allocation partitions, each with room for a few blocks' worth of tiles
        float sortMs = 0;
        if (!predicted) HIPCHECK(hipEventElapsedTime(&sortMs, evRebuild[0], evRebuild[2]));      // (predicted: the sort is part of the span measured below)
        for (int attempt = 0; attempt < 3; attempt++) {
            tileJ.resize(tileCap * 32); tileInfo.resize(tileCap); masks.resize(tileCap * 32); workItems.resize(2 * (tileCap / 4 + 2 * numBlocks + 64)); workItemsStage.resize(tileCap / 4 + 2 * numBlocks + 64); workItemsPartial.resize(tileCap / 4 + 2 * numBlocks + 64);
            p.nPadded = Npad; p.nBlocks = numBlocks; p.blockSubset = blockSubset.p;
            p.shardBegin = shardBegin; p.shardWidth = shardEnd - shardBegin; p.shardPeriod = shardPeriod;
            p.exactPrune = sw.boxPrune ? 0 : 1; p.itemTiles = sw.itemTiles;
            p.blockCenter = dBlockCenter.p; p.blockHalf = dBlockHalf.p;
            p.sortedToUser = dSortedToUser.p; p.userToSorted = dUserToSorted.p; p.posq = posq.p; p.sigeps = sigeps.p; p.imageOffset = imageOffset.p;
            p.atomSubset = atomSubset.p; p.atomGrid = atomGrid.p; p.colRange = colRange.p; p.zIndex = dZIndex.p;
            dAtomCell.resize(Npad); p.atomCell = dAtomCell.p;
            const bool nbTrace = sw.nbTrace;
            if (nbTrace) { dNbTrace.resize((size_t)4 * numBlocks); p.dbgOut = dNbTrace.p; }
            p.tileJ = tileJ.p; p.tileInfo = tileInfo.p; p.masks = masks.p; p.workItems = workItems.p; p.workItemsStage = workItemsStage.p; p.workItemsPartial = workItemsPartial.p; p.counters = dCounters.p;
            p.tileCapacity = (int)tileCap; p.workCapacity = (int)(tileCap / 4 + 2 * numBlocks + 64); p.maskCapacity = (int)tileCap;
            if (!predicted || attempt > 0) HIPCHECK(hipEventRecord(evRebuild[0], stream));
            launchNeighborBuild<Real>(p, stream);
            HIPCHECK(hipEventRecord(evRebuild[1], stream));
            if (sideBuilding) {      // build beside the steps: publish the totals and leave; finishSideBuild reads them when the rebuild falls due
                sideSeq = ++nbPubSeq;
                launchNeighborPublish(dCounters.p, dNbPub, sideSeq, stream);
                return true;
            }
            int h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            // the totals come back through mapped host memory and a sequence number the host spins on (a sleeping hipStreamSynchronize wakes
            // up 30-45 us after the kernel has ended, with the GPU idle); the synchronisation behind it then returns at once
            if (hNbPub && dNbPub && !sw.nbNoSpin) {
                const int seq = ++nbPubSeq;
                launchNeighborPublish(dCounters.p, dNbPub, seq, stream);
                waitForTotals(seq, h, stream);
                HIPCHECK(hipStreamSynchronize(stream));      // (the events below are read next; nothing is running any more)
            } else {
                HIPCHECK(hipMemcpyAsync(h, dCounters.p, sizeof(h), hipMemcpyDeviceToHost, stream));
                HIPCHECK(hipStreamSynchronize(stream));
            }
            // (insurance for the above: a padded count that has doubled since the last accepted build, out of a replayed graph, is built once more
            // from plain launches before anything is sized by it)
            if (!sortGraphSuspect && stats.n_rebuilds > 0 && h[7] > 2 * std::max(Npad, N) && !sideBuilding) {
                sortGraphSuspect = true;
                if (sw.verbose) fprintf(stderr, "[snb] rebuild: padded count %d after %d: phase A once more without its graph\n", h[7], Npad);
                return gpuRebuild();
            }
            if (predicted && (h[7] > Npad || h[7] < N || (h[7] & 31))) {      // the prediction was too small (or the count is inconsistent): once more, waiting for the exact count
                if (h[7] < N || (h[7] & 31)) throw HipError{"neighbour build: inconsistent padded atom count"};
                npadPredict = 0; padMispredictions++;
                if (sw.verbose) fprintf(stderr, "[snb] rebuild: padded count %d exceeded the predicted %d, repeating with the exact count (%lld so far)\n", h[7], Npad, (long long)padMispredictions);
                return gpuRebuild();
            }
            if (nbTrace && h[3] == 0) {
                std::vector<long long> tr((size_t)4 * numBlocks);
                HIPCHECK(hipMemcpy(tr.data(), dNbTrace.p, sizeof(long long) * tr.size(), hipMemcpyDeviceToHost));
                long long t0min = tr[0], t1max = tr[1]; std::vector<long long> dur(numBlocks);
                tr.resize((size_t)4 * numBlocks);
                for (int b = 0; b < numBlocks; b++) { t0min = std::min(t0min, tr[2 * b]); t1max = std::max(t1max, tr[2 * b + 1]); dur[b] = tr[2 * b + 1] - tr[2 * b]; }
                std::vector<long long> sorted = dur; std::sort(sorted.begin(), sorted.end());
                fprintf(stderr, "[snb] nb trace: span %.1f us; per-block duration median %.1f us, p90 %.1f, p99 %.1f, max %.1f us; last start at %.1f us\n", (t1max - t0min) / 100.0, sorted[numBlocks / 2] / 100.0,
                        sorted[numBlocks * 9 / 10] / 100.0, sorted[numBlocks * 99 / 100] / 100.0, sorted.back() / 100.0, (t1max - t0min) / 100.0);
                { std::vector<long long> a(numBlocks), b(numBlocks), c(numBlocks);
                  for (int k = 0; k < numBlocks; k++) { a[k] = tr[2 * numBlocks + 2 * k] - tr[2 * k]; b[k] = tr[2 * numBlocks + 2 * k + 1] - tr[2 * numBlocks + 2 * k]; c[k] = tr[2 * k + 1] - tr[2 * numBlocks + 2 * k + 1]; }
                  std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end()); std::sort(c.begin(), c.end());
                  fprintf(stderr, "[snb] nb trace: median prologue %.1f us, gather %.1f us, final flush %.1f us\n", a[numBlocks / 2] / 100.0, b[numBlocks / 2] / 100.0, c[numBlocks / 2] / 100.0); }
                long long lastStart = 0; for (int b = 0; b < numBlocks; b++) lastStart = std::max(lastStart, tr[2 * b] - t0min);
                fprintf(stderr, "[snb] nb trace: last block start %.1f us after the first\n", lastStart / 100.0);
            }
            if (h[3] == 0) { acceptBuild(h, sortMs); gpuBuilt = true; needRebuild = false; paramsDirty = false; stepsSinceRebuild = 0; (void)t0; return true; }
            if (sw.verbose) fprintf(stderr, "[snb] gpu neighbour build attempt %d: tiles %d work %d masks %d overflow %d partial %d maxPartTiles %d maxPartWork %d (cap %zu, region %zu / %zu)\n", attempt, h[0], h[1], h[2], h[3], h[4], h[5], h[6], tileCap, tileCap / 64, (tileCap / 4 + 2 * numBlocks + 64) / 64);
            // capacity: a partition (1/64 of the arrays) ran out of tiles, masks or work items -> grow and retry
            if ((size_t)h[5] > tileCap / 64 || (size_t)h[6] > (tileCap / 4 + 2 * numBlocks + 64) / 64) { tileCap = std::max((size_t)h[5] * 64 * 5 / 4, tileCap * 3 / 2) + 4096; continue; }
            return false;   // a block gathered more than its LDS list holds, or a block is too extended for tile images: host path
        }
        return false;
    }

    // ------------------------------------------------------------------------------------------
    // need: the slices an energy step must produce (sliceNeed); cellsReady: this step's gather pass already wrote the Coulomb-mesh cells;
    // trace: SNB_STEP_TRACE stamps of a replayed step
    void fillPme(PmeParams<Real>& p, PmePlan<Real>& plan, bool wantEnergy, const int* need, bool cellsReady = false, bool trace = false) {
        p.d = plan.d; p.nsub = nGrids; p.natoms = Npad; p.posq = posq.p; p.sigeps = sigeps.p; p.atomSubset = atomSubset.p; p.atomGrid = atomGrid.p;
        p.cells = pmeCells.p;
        if (sw.pmeTrace) { if (!dPmeTrace.p) { dPmeTrace.resize(8); HIPCHECK(hipMemset(dPmeTrace.p, 0, 64)); } p.trace = dPmeTrace.p; }
        p.stepTrace = (trace && plan.dispersion == (cfg.method == SNB_LJPME)) ? dStepTrace.p : nullptr;      // (the step's LAST mesh: its inverse z transform is what the second launch follows)
        p.cellsReady = (!plan.dispersion && cellsReady) ? 1 : 0;
        p.fixDev = dFixScale.p ? dFixScale.p + (plan.dispersion ? 2 : 0) : nullptr;      // (k_fixScale keeps it in step with the parameters)
        p.gridReal = plan.gridReal.p; p.gridCplx = plan.gridCplx.p; p.planeB = plan.gridCplxB.p; p.planeEterm = plan.planeEtermReady ? plan.planeEterm.p : nullptr; p.twx = plan.twx.p; p.twy = plan.twy.p; p.twz = plan.twz.p;
        p.modx = plan.modx.p; p.mody = plan.mody.p; p.modz = plan.modz.p;
        const double det = box[0] * box[4] * box[8];
        double r[9]; recipBoxRows(box, r);
        for (int i = 0; i < 9; i++) { p.recip[i] = (Real)r[i]; p.recipLo[i] = (Real)(r[i] - (double)p.recip[i]); }
        p.alpha = (Real)plan.alpha; p.volume = (Real)det; p.dispersion = plan.dispersion ? 1 : 0;
        p.lambdas = dLambdas.p; p.sliceNeed = need; p.gridSubset = gridSubset.p; p.emptyGrids = emptyGrids; p.nsubTotal = nsub; p.mix = cfg.shard_count == 1 ? 1 : 0;
        p.mix16 = sw.mix16 ? 1 : 0;
        p.sliceE = sliceE.p; p.fpx = fpx.p; p.fpy = fpy.p; p.fpz = fpz.p; p.wantEnergy = wantEnergy ? 1 : 0;
        // brick kernels: the sort columns were cut for the Coulomb mesh; any mesh whose cells tile those columns can use them,
        // with bricks of `group` columns when one column is narrower than 5 cells (stencil 4 + 1 cell of drift)
        p.sortNcx = p.sortNcy = 0; p.groupX = p.groupY = 1; p.colRange = nullptr;
        p.zSlabs = 1;
        // measured on c3: f64 accumulation 1 slab 110 us, 2 slabs 105 us, 4 slabs 145 us; fixed-point (single precision, even nz) 1 slab 61 us, 2 slabs 67 us
        if (plan.d.nz % 2 == 0 && plan.d.nz >= 32 && !(sizeof(Real) == 4)) p.zSlabs = 2;
        if (sw.zSlabs >= 1 && plan.d.nz % sw.zSlabs == 0) p.zSlabs = sw.zSlabs;
        const BrickGeometry b = bricksFor(plan);
        if (b.ok) {
            p.sortNcx = b.ncx; p.sortNcy = b.ncy; p.groupX = b.gx; p.groupY = b.gy; p.colRange = colRange.p;
            p.ownSlabs = plan.ownSlabs; p.ownMargin = plan.ownMargin; p.ownPartial = plan.ownPartial.p; p.ownBusy = plan.ownBusy.p;
            p.strays = plan.strays.p; p.strayCount = dStrayCount.p ? dStrayCount.p + (plan.dispersion ? 1 : 0) : nullptr;
            if (!p.ownPartial || !p.ownBusy || !p.strays || !p.strayCount) p.ownSlabs = 0;
        }
    }
    // brick kernels: do this mesh's cells tile the sort columns (cut for the Coulomb mesh, `pme`)?  pme_plan.h
    BrickGeometry bricksFor(const PmePlan<Real>& plan) const { return brickGeometry(plan.d, pme.d, colCells, sw.brickGroup); }
    // Plane path (pme.hip k_planeXY): its table of reciprocal-space kernel values follows the box and alpha, both fixed between rebuilds.
    void planPlaneTable(PmePlan<Real>& plan) {
        if (!plan.planeEterm.p || !plan.gridCplxB.p || nGrids <= 0) { plan.planeEtermReady = false; return; }
        // (the table depends on the box, alpha and the mesh only: a rebuild with the same box keeps it -- 11 us of kernel + a launch per rebuild)
        double key[10]; for (int i = 0; i < 9; i++) key[i] = box[i]; key[9] = plan.alpha;
        if (plan.planeEtermReady && plan.planeEtermFilled && std::memcmp(key, plan.planeEtermKey, sizeof(key)) == 0) return;
        std::memcpy(plan.planeEtermKey, key, sizeof(key));
        plan.planeEtermReady = false;
        PmeParams<Real> pp; std::memset(&pp, 0, sizeof(pp));
        fillPme(pp, plan, false, dSliceNeedAll.p);
        plan.planeEtermFilled = launchPlaneEterm<Real>(pp, plan.planeEterm.p, stream);
        plan.planeEtermReady = true;
    }
    // SNB_VERBOSE: the spreader planned for a mesh at this rebuild.  Sort columns and bricks decide between the atomic spreader and the brick
    // kernels for good; of the own-atoms spreader the line states the planned slabs (pme_plan.h OwnSpread::slabs) -- the launch can still
    // decline them (OwnSpread::runs), and that it ran shows only where the plane path follows it (no y-pass stamps in slots 3 / 5).
    void describeMesh(const char* name, const PmePlan<Real>& plan) const {
        const BrickGeometry b = bricksFor(plan);
        const bool bricks = nGrids > 0 && b.ok;
        // (the sort columns are cut on the Coulomb mesh, `pme`, for every mesh; the mesh size and the bricks are this plan's)
        fprintf(stderr, "[snb] %s mesh %d x %d x %d: sort columns %d x %d of %d x %d cells, %s", name, plan.d.nx, plan.d.ny, plan.d.nz,
                colCells[0] > 0 ? pme.d.nx / colCells[0] : 0, colCells[0] > 0 ? pme.d.ny / colCells[1] : 0, colCells[0], colCells[1],
                !bricks ? "atomic spreader" : "");
        if (bricks) fprintf(stderr, "bricks of %d x %d columns, %s (slabs %d, margin %d)", b.gx, b.gy, plan.ownSlabs > 0 ? "own-atoms spreader planned" : "scanning brick spreader", plan.ownSlabs, plan.ownMargin);
        // the (R1, R2) instantiations the mesh size selects (0 * 0: the staged transforms; plane splits 0 * 0: no plane kernel for this size)
        const PmePlanDims& d = plan.d;
        fprintf(stderr, "; fft splits x %d*%d y %d*%d z %d*%d, plane splits x %d*%d y %d*%d (%s)\n", d.rx1, d.rx2, d.ry1, d.ry2, d.rz1, d.rz2, d.px1, d.px2, d.py1, d.py2,
                (d.px1 <= 0 || d.py1 <= 0) ? "none" : planeIsStatic(d) ? "static" : "run-time");
    }
    // Geometry and buffers of the own-atoms spreader for one mesh (called from rebuild(): nothing may allocate inside a graph capture).
    // Margin and slabs: pme_plan.h ownSpreadMargin / ownSpread; launchSpreadOwn (pme.hip) calls the same function with the same inputs.
    void planOwnSpread(PmePlan<Real>& plan) {
        plan.ownSlabs = 0;
        const BrickGeometry b = bricksFor(plan);
        if (nGrids <= 0 || !b.ok) return;
        double r[9]; recipBoxRows(box, r);
        const int M = ownSpreadMargin(plan.d, r, cfg.neighbor_padding, sw);
        const OwnSpread o = ownSpread(plan.d, b, nGrids, sizeof(Real), M, sw);
        if (!o.slabs) return;
        plan.ownPartial.resize(o.partialBytes);
        plan.ownBusy.resize(o.regions); plan.strays.resize(std::max(Npad, 1));
        plan.ownSlabs = o.slabs; plan.ownMargin = M;
    }

    // What every evaluation starts with: the state checks, then the neighbour-list rules -- a due rebuild happens (in line, or as the exchange of a
    // list built beside the steps), a side build nothing can use any more is cancelled, changed parameter values are refreshed.  forces: a forces
    // step; anything else keeps the forces of the last forces step across a re-sort.  Returns whether the lists were rebuilt in line.
    // The refusals about a periodic box x that every evaluation shares (prefix: what the caller puts before the messages about x): too small
    // for the cutoff, not rectangular under classic Ewald.  The refusal of an Ewald engine without kmax is raised between the two
    // (kmax: snb_execute's order), or alone (x == null: a batch raises it once, behind its frames).
    void checkBox(const double* x, bool recip, const std::string& prefix, bool kmax) {
        const double minAllowed = 1.999999 * cfg.cutoff;
        if (x && !(x[0] >= minAllowed && x[4] >= minAllowed && x[8] >= minAllowed)) { err = prefix + "The periodic box size has decreased to less than twice the nonbonded cutoff."; throw (int)SNB_ERR_BOX_TOO_SMALL; }
        if (cfg.method != SNB_Ewald || !recip) return;
        if (kmax && (cfg.kmax[0] < 1 || cfg.kmax[1] < 1 || cfg.kmax[2] < 1)) { err = "Ewald: kmax must be given explicitly (snb_config.kmax)"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (x && (x[3] != 0 || x[6] != 0 || x[7] != 0)) { err = prefix + "SlicedNonbondedForce: Ewald is not supported with non-rectangular boxes.  Use PME instead."; throw (int)SNB_ERR_UNSUPPORTED; }
    }
    bool beginExecute(bool forces, int includeRecip) {
        if (!haveParticles) throw HipError{"snb_execute: particles were not set"};
        if (!havePositions) throw HipError{"snb_execute: positions were not set"};
        if (isPeriodic()) {
            if (!haveBox) throw HipError{"snb_execute: box was not set"};
            checkBox(box, includeRecip != 0, "", true);
        }
        if (dLambdas.p == nullptr) setLambdas(lambdas.data());
        // rebuild_interval < 0: automatic -- rebuild when the displacement watch of the position-gather pass has seen an atom move
        // 0.8 * skin/2 since the last rebuild (the flag lives in mapped host memory: no synchronisation; it is read one execute late,
        // hence the margin), and after -rebuild_interval executes at the latest
        const bool autoMode = cfg.rebuild_interval < 0;
        // ... stream-ordered: the flag is read only after the execute before the previous one has COMPLETED on the GPU (an event recorded at
        // the end of every execute, two slots), so the host can never run far ahead of the watch -- a forces-only step is an asynchronous
        // graph launch.  The decision therefore sees every displacement up to two executes ago; the 0.8 factor leaves 0.2 * skin/2 for
        // those two steps.
        if (autoMode && cfg.neighbor_padding > 0) {
            hipEvent_t& ev = evStepDone[stepCounter & 1];
            if (ev) HIPCHECK(hipEventSynchronize(ev));
        }
        if (flagsResetPending && hipEventQuery(evFlagsReset) == hipSuccess) flagsResetPending = false;
        const bool due = autoMode ? ((hDispFlags[0] != 0 && !flagsResetPending) || stepsSinceRebuild >= -cfg.rebuild_interval) : (cfg.rebuild_interval <= 1 || stepsSinceRebuild >= cfg.rebuild_interval);
        bool rebuilding = needRebuild || paramsDirty || due || cfg.neighbor_padding <= 0;
        if (!forces && rebuilding) keepLastForces();      // (an in-line rebuild re-sorts the atoms, a side-build exchange swaps the permutations)
        if (sidePending) {
            // anything but the positions changed since the side build started: its list is of no use
            if (needRebuild || paramsDirty || staticDirty || valuesDirty || excValuesDirty || cfg.neighbor_padding <= 0) cancelSideBuild();
            else if (rebuilding && finishSideBuild()) rebuilding = false;
        }
        if ((valuesDirty || excValuesDirty) && !staticDirty && !rebuilding) refreshValues();
        if (rebuilding) { if (valuesDirty || excValuesDirty) { staticDirty = true; valuesDirty = excValuesDirty = false; } if (ctx.on) stageCtxPositions(ctxStage.p); rebuild(); }
        stepsSinceRebuild++;
        return rebuilding;
    }
    // ... and ends with: the end-of-execute event of the displacement watch, the step count, the side build that falls due sw.sideLead executes from now
    void endExecute() {
        const bool autoMode = cfg.rebuild_interval < 0;
        if (autoMode && cfg.neighbor_padding > 0) {
            hipEvent_t& ev = evStepDone[stepCounter & 1];
            if (!ev) HIPCHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            HIPCHECK(hipEventRecord(ev, stream));
        }
        stepCounter++;
        // the rebuild that falls due sw.sideLead executes from now starts here, beside the steps, from the positions of the step just enqueued
        if (!autoMode && stepsSinceRebuild == cfg.rebuild_interval - sw.sideLead && sideBuildPossible()) startSideBuild();
    }

    void execute(int includeForces, int includeEnergy, int includeDirect, int includeRecip, double* energyOut) override {
        if (includeEnergy == 2 && energyOut) { err = "snb_execute: include_energy == 2 (derivative-only step) delivers no total energy; pass energy = NULL"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        const bool forces = includeForces != 0;
        if (!forces && includeEnergy == 0) { if (energyOut) *energyOut = 0.0; return; }      // nothing asked for: nothing enqueued
        if (forces) keptValid = false;      // (this step's forces replace the kept ones)
        const bool rebuilding = beginExecute(forces, includeRecip);
        if (forces) outputWritten = outPtr != nullptr;      // (an energy-only step leaves the forces of the last forces step where they are)
        const bool energy = includeEnergy != 0;
        StepRequest req;
        req.energy = !energy ? StepEnergy::None : includeEnergy == 2 ? StepEnergy::Selected : StepEnergy::All;      // (2: derivative-only step)
        req.direct = includeDirect != 0; req.recip = includeRecip != 0;
        req.addCtxTotal = ctx.on && ctx.energy && includeEnergy == 1 && !energyOut;      // (with energy != NULL the caller takes the total on the host)
        if (forces) lastRecip = includeRecip && (isPme() || cfg.method == SNB_Ewald);
        // Forces-only steps replay a captured hipGraph (the ~14 small launches of a step are host-launch-bound otherwise:
        // 7-8 us of idle GPU between kernels).  Every 32nd step -- and every energy step -- is enqueued eagerly with HIP events
        // around the pair kernel and the reciprocal pipeline; those samples feed snb_stats' kernel timers.
        // (the step right after a rebuild goes out as plain launches: the GPU is idle at that point -- the rebuild ended with a host
        // read-back -- and capturing + instantiating the step graph first would keep it idle for another ~50 us; the capture then happens
        // at the next step, while this one is executing)
        // Energy steps (per-slice energies, the step of every force with energy-parameter derivatives, Q4) are graph steps like any other:
        // they end with the device-side sum of the slice-energy partitions and leave the result there until it is asked for.
        // (round 4: a rebuild step replays its graph too when one exists for these buffers -- refreshing it costs the host ~20 us of capture +
        // hipGraphExecUpdate, against ~40 us of launch gaps of an eager step, and an overlapped step is 37 us shorter than a serial one)
        if (!forces) {
            // Energy-only step (include_forces == 0): plain launches, timed on the eager steps' cadence; the step itself never captures or
            // updates a step graph (a rebuild it performs marks the graphs stale, as any rebuild does).  No force arithmetic, no force stores,
            // no force output -- except on sharded PME engines, whose energies come from the force interpolation: they run the forces kernels
            // into a scratch set.
            if (timingInterval > 0 && !sidePending && execCount++ % timingInterval == 0) {
                req.ev = &ring[ringPos]; ringPos = (ringPos + 1) % RING;
                if (req.ev->pending) harvest(*req.ev);
            }
            const bool scratch = includeRecip && isPme() && nGrids > 0 && cfg.shard_count > 1;
            req.forces = scratch ? StepForces::Scratch : StepForces::None;
            if (scratch) { forceScratch.resize((size_t)forceArrays() * Npad); pointForceViews(forceScratch.p); }
            {
                ScopeExit views([&] { if (scratch) pointForceViews(forceBuf.p); });
                enqueueStep(req);
            }
            if (req.ev) req.ev->pending = true;
        } else {
            haveForceStep = true;
            const GraphKey stepKey = graphKey(req);
            bool haveGraph = false;
            for (auto& g : graphs) if (g.key == stepKey && g.exec) haveGraph = true;
            const bool eager = cfg.disable_graph || sw.noStepGraph || (rebuilding && (!haveGraph || sw.eagerRebuildStep)) || (timingInterval > 0 && !sidePending && execCount++ % timingInterval == 0);      // (no timed step while a list is being built beside it: the kernel timers are for kernels running alone)
            if (eager) {
                req.ev = &ring[ringPos]; ringPos = (ringPos + 1) % RING;
                if (req.ev->pending) harvest(*req.ev);
                enqueueStep(req);
                req.ev->pending = true;
            } else replayStep(stepKey, req, rebuilding);
        }
        endExecute();
        if (energy) {
            energyPending = true;
            if (energyOut) { fetchSliceEnergies(); double e = 0; for (int i = 0; i < 2 * S; i++) e += lambdas[i] * hostSliceE[i]; *energyOut = e; }      // (synchronises)
        } else if (energyOut) *energyOut = 0.0;
    }
    // A replayed step: the captured graph of this key is found, or captured (and updated in place or instantiated anew, evicting the oldest
    // of MAX_GRAPHS), then launched
    void replayStep(const GraphKey& key, const StepRequest& req, bool rebuilding) {
        hipGraphExec_t graphExec = nullptr;
        CachedGraph* cached = nullptr;
        for (auto& g : graphs) if (g.key == key) { cached = &g; if (!g.stale) graphExec = g.exec; break; }
        if (!graphExec) {
            if (!stream2 && (sw.concurrentPme || sw.overlap)) {   // created outside the capture
                int lo = 0, hi = 0;
                HIPCHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
                HIPCHECK(hipStreamCreateWithPriority(&stream2, hipStreamNonBlocking, sw.pmePrioLow ? lo : (sw.pmePrioHigh ? hi : (lo + hi) / 2)));
                HIPCHECK(hipEventCreateWithFlags(&evFork, hipEventDisableTiming)); HIPCHECK(hipEventCreateWithFlags(&evJoin, hipEventDisableTiming)); HIPCHECK(hipEventCreateWithFlags(&evPairA, hipEventDisableTiming));
            }
            hipGraph_t graph = nullptr;
            const auto tc0 = std::chrono::steady_clock::now();
            HIPCHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
            try { enqueueStep(req); }
            catch (...) { (void)hipStreamEndCapture(stream, &graph); if (graph) (void)hipGraphDestroy(graph); throw; }
            HIPCHECK(hipStreamEndCapture(stream, &graph));
            const auto tc1 = std::chrono::steady_clock::now();
            bool updated = false;
            if (cached && cached->exec && !sw.noGraphUpdate) {
                hipGraphNode_t errNode = nullptr; hipGraphExecUpdateResult res;
                if (hipGraphExecUpdate(cached->exec, graph, &errNode, &res) == hipSuccess) { graphExec = cached->exec; cached->stale = false; updated = true; }
                else (void)hipGetLastError();
            }
            if (!updated) {
                HIPCHECK(hipGraphInstantiate(&graphExec, graph, nullptr, nullptr, 0));
                if (cached) { if (cached->exec) (void)hipGraphExecDestroy(cached->exec); cached->exec = graphExec; cached->stale = false; }
                else if (graphs.size() < MAX_GRAPHS) graphs.push_back({key, graphExec, false});
                else { (void)hipGraphExecDestroy(graphs[graphVictim].exec); graphs[graphVictim] = {key, graphExec, false}; graphVictim = (graphVictim + 1) % MAX_GRAPHS; }
            }
            HIPCHECK(hipGraphDestroy(graph));
            if (sw.verbose) fprintf(stderr, "[snb] step graph: capture %.0f us, %s %.0f us (host)\n", std::chrono::duration<double, std::micro>(tc1 - tc0).count(), updated ? "update" : "instantiate",
                                 std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tc1).count());
        }
        if (sw.verbose && rebuilding) {
            const auto tl0 = std::chrono::steady_clock::now();
            HIPCHECK(hipGraphLaunch(graphExec, stream));
            const auto tl1 = std::chrono::steady_clock::now();
            HIPCHECK(hipStreamSynchronize(stream));
            fprintf(stderr, "[snb] rebuild step: graph launch %.0f us (host), step done after %.0f us\n", std::chrono::duration<double, std::micro>(tl1 - tl0).count(),
                    std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tl0).count());
        } else HIPCHECK(hipGraphLaunch(graphExec, stream));
        if (sw.overlapDebug && sw.overlap && dOverlap.p && overlapDumps > 0) { overlapDumps--; dumpOverlapTable(); }
    }


    // ------------------------------------------------------------------------------------------
    // Frame batches (snb_evaluate_frames): F stored frames, one energy-only step each, rows of raw slice energies out.
    // ------------------------------------------------------------------------------------------
    // may the list of the NEXT frame be built beside the step of this one?  What sideBuildPossible asks of an MD rebuild, without the interval
    bool frameSideBuildPossible() const {
        return sw.sideRebuild && !sw.framesInLine && !sidePending && gpuBuilt && isPeriodic() && !cfg.host_neighbor_build
               && !needRebuild && !paramsDirty && !staticDirty && !valuesDirty && !excValuesDirty && npadPredict > 0 && npadPredict == Npad && hNbPub && dNbPub;
    }
    void ensureFrameResources(bool hostFrames, size_t frameBytes) {
        for (int k = 0; k < 2; k++) if (!evFrameStep[k]) HIPCHECK(hipEventCreateWithFlags(&evFrameStep[k], hipEventDisableTiming));
        if (!evBatchStart) HIPCHECK(hipEventCreateWithFlags(&evBatchStart, hipEventDisableTiming));
        ensureBuildStream();
        if (!hostFrames) return;
        if (!streamCopy) HIPCHECK(hipStreamCreateWithFlags(&streamCopy, hipStreamNonBlocking));
        for (int k = 0; k < 2; k++) {
            if (!evFrameUp[k]) HIPCHECK(hipEventCreateWithFlags(&evFrameUp[k], hipEventDisableTiming));
            if (frameUpPending[k]) { HIPCHECK(hipEventSynchronize(evFrameUp[k])); frameUpPending[k] = false; }
            if (framePinnedCap[k] < frameBytes) {
                if (framePinned[k]) { (void)hipHostFree(framePinned[k]); framePinned[k] = nullptr; framePinnedCap[k] = 0; }
                HIPCHECK(hipHostMalloc(&framePinned[k], std::max<size_t>(frameBytes, 4096), hipHostMallocDefault)); framePinnedCap[k] = std::max<size_t>(frameBytes, 4096);
            }
            frameDev[k].resize(frameBytes);
        }
    }
    // The frames of a batch: what snb_frame_batch and snb_group_batch say about them (who: the entry point, for the messages)
    struct FrameInput { const char* who; int F; const void* positions; bool hostFrames, isDouble, stride4; const double* boxes; };
    // ---- everything about the frames is checked before anything is enqueued or changed
    void checkFrames(const FrameInput& in, bool recip) {
        const std::string who = in.who; const int F = in.F;
        if (!haveParticles) throw HipError{who + ": particles were not set"};
        const bool frameBoxes = isPeriodic() && in.boxes != nullptr;
        if (isPeriodic()) {
            if (!frameBoxes && !haveBox) throw HipError{who + ": box was not set"};
            for (int f = 0; f < (frameBoxes ? F : 1); f++) {
                const double* x = frameBoxes ? in.boxes + 9 * (size_t)f : box;
                const std::string prefix = who + ": frame " + std::to_string(f) + ": ";
                if (x[1] != 0 || x[2] != 0 || x[5] != 0) throw HipError{prefix + "box vectors must be in reduced (lower triangular) form"};
                checkBox(x, recip, prefix, false);
            }
        }
        checkBox(nullptr, recip, "", true);
    }
    // The frame loop of a batch, for any kind of step: step(f) enqueues, on `stream`, what is evaluated at frame f -- the lists in use are
    // that frame's, box and devUserPos are set -- and everything it enqueues precedes evFrameStep[f & 1]: the build of frame f + 2 overwrites
    // the list set it reads.  finish() enqueues what follows the last frame and returns whether it synchronised (host output).  The engine's
    // own state is put back when the batch is through, or has failed.
    template <typename Step, typename Finish>
    void runFrames(const FrameInput& in, const std::chrono::steady_clock::time_point t0, Step&& step, Finish&& finish) {
        const int F = in.F;
        const bool frameBoxes = isPeriodic() && in.boxes != nullptr;
        // ---- the engine's own state, put back when the batch is through
        const void* const savedPos = devUserPos; const int savedIsDouble = posIsDouble, savedStride4 = posStride4; const bool savedHavePos = havePositions, savedHaveBox = haveBox;
        double savedBox[9]; for (int i = 0; i < 9; i++) savedBox[i] = box[i];
        const long long discardedBefore = sideDiscarded; const int savedPredict = npadPredict;
        const bool hostFrames = in.hostFrames;
        const size_t frameBytes = (size_t)N * (in.stride4 ? 4 : 3) * (in.isDouble ? 8 : 4);
        ScopeExit restore([&] {
            devUserPos = savedPos; posIsDouble = savedIsDouble; posStride4 = savedStride4; havePositions = savedHavePos; haveBox = savedHaveBox;
            for (int i = 0; i < 9; i++) box[i] = savedBox[i];
            plainSort = false;
            if (savedPredict > 0) npadPredict = savedPredict;      // (MD rebuilds size their arrays as they did before the batch; an engine that had no prediction yet keeps the batch's, so that the next batch pipelines from its second frame)
            needRebuild = true;      // the lists in memory belong to the last frame
        });
        try {
            if (dLambdas.p == nullptr) setLambdas(lambdas.data());
            if (sidePending) cancelSideBuild();      // (an MD side build in flight: its list would come into use after frames it knows nothing of)
            keepLastForces();      // before the first frame's rebuild re-sorts the atoms
            ensureFrameResources(hostFrames, frameBytes);
            posIsDouble = in.isDouble ? 1 : 0; posStride4 = in.stride4 ? 1 : 0; havePositions = true; plainSort = true;
            // The batch's own padded-count prediction: unrelated frames move the count further than consecutive MD rebuilds do (MD: last count
            // + 0.4 % + 8 blocks), so a batch sizes the arrays by the last exact count + 3 % + 32 blocks, from its first frame's build on, and
            // keeps that size while a frame's count leaves it 8 spare blocks -- a prediction that moved with every new maximum would no longer
            // equal the arrays' size, which costs the next frame its side build.
            int batchPredict = 0;
            auto widePrediction = [](int count) { return ((int)(count * 1.03) + 1024 + 31) / 32 * 32; };
            auto predictForFrames = [&]() {      // after a build was accepted (gpuBuilt), or before the first frame
                if (lastPadCount <= 0 || npadPredict <= 0) return;
                if (batchPredict == 0 || lastPadCount + 256 > batchPredict) batchPredict = std::max(std::max(batchPredict, npadPredict), widePrediction(lastPadCount));
                npadPredict = batchPredict;
            };
            predictForFrames();
            long long nBeside = 0, nInLine = 0;
            HIPCHECK(hipEventRecord(evBatchStart, stream));      // (staging slots and the shadow set may still be read by what was enqueued before the batch)
            auto frameBox = [&](int f) { return frameBoxes ? in.boxes + 9 * (size_t)f : savedBox; };
            auto sameBox = [&](int f, int g) { return std::memcmp(frameBox(f), frameBox(g), 9 * sizeof(double)) == 0; };
            // the event behind the last step that read what frame g is about to overwrite (its staging slot, the shadow set): the step of frame g - 2
            auto freeEvent = [&](int g) { return g >= 2 ? evFrameStep[g & 1] : evBatchStart; };
            // frame g on the device: the caller's own buffer, or its staging slot, filled by the copy stream
            auto stage = [&](int g) -> const void* {
                const unsigned char* src = static_cast<const unsigned char*>(in.positions) + (size_t)g * frameBytes;
                if (!hostFrames) return src;
                const int slot = g & 1;
                if (frameUpPending[slot]) { HIPCHECK(hipEventSynchronize(evFrameUp[slot])); frameUpPending[slot] = false; }      // (the copy of frame g - 2 out of this pinned slot: long done)
                std::memcpy(framePinned[slot], src, frameBytes);
                HIPCHECK(hipStreamWaitEvent(streamCopy, freeEvent(g), 0));
                HIPCHECK(hipMemcpyAsync(frameDev[slot].p, framePinned[slot], frameBytes, hipMemcpyHostToDevice, streamCopy));
                HIPCHECK(hipEventRecord(evFrameUp[slot], streamCopy)); frameUpPending[slot] = true;
                return frameDev[slot].p;
            };
            const void* cur = stage(0);
            if (hostFrames) HIPCHECK(hipStreamWaitEvent(stream, evFrameUp[0], 0));
            for (int f = 0; f < F; f++) {
                if (frameBoxes) { for (int i = 0; i < 9; i++) box[i] = frameBox(f)[i]; haveBox = true; }
                devUserPos = cur;
                bool beside = false;
                if (sidePending) beside = finishSideBuild();      // (started behind the previous frame's step, from this frame's positions; spins on the build's totals only)
                if (beside) nBeside++;
                else {
                    if (valuesDirty || excValuesDirty) { staticDirty = true; valuesDirty = excValuesDirty = false; }
                    if (hostFrames) HIPCHECK(hipEventSynchronize(evFrameUp[f & 1]));      // (an in-line build may read the positions back to the host)
                    rebuild();
                    nInLine++;
                }
                if (gpuBuilt) predictForFrames();
                stepsSinceRebuild++;
                step(f);      // plain launches, never stamped: no step graph is captured or updated
                HIPCHECK(hipEventRecord(evFrameStep[f & 1], stream));
                if (f + 1 < F) {
                    cur = stage(f + 1);
                    if (sameBox(f, f + 1) && frameSideBuildPossible()) {      // (column geometry, PME brick plans and the plane table follow the box: a changed box builds in line)
                        HIPCHECK(hipStreamWaitEvent(streamBuild, freeEvent(f + 1), 0));
                        if (hostFrames) HIPCHECK(hipStreamWaitEvent(streamBuild, evFrameUp[(f + 1) & 1], 0));
                        startSideBuild(cur);
                    }
                    if (hostFrames) HIPCHECK(hipStreamWaitEvent(stream, evFrameUp[(f + 1) & 1], 0));
                }
            }
            fstats.n_batches++; fstats.n_frames += F; fstats.n_built_beside += nBeside; fstats.n_built_in_line += nInLine; fstats.n_side_discarded += sideDiscarded - discardedBefore; fstats.last_batch_ms = 0;
            if (finish()) fstats.last_batch_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        } catch (...) {
            if (sidePending) { try { cancelSideBuild(); } catch (...) {} }      // (before the restore)
            throw;
        }
    }
    void evaluateFrames(const snb_frame_batch* b) override {
        const auto t0 = std::chrono::steady_clock::now();
        if (b->n_frames < 0) { err = "snb_evaluate_frames: negative frame count"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (ctx.on) { err = "snb_evaluate_frames: a context is bound (snb_bind_context): the positions come from its posq"; throw (int)SNB_ERR_STATE; }
        if (cfg.shard_count > 1) { err = "snb_evaluate_frames: not available with shard_count > 1"; throw (int)SNB_ERR_UNSUPPORTED; }
        const int F = b->n_frames;
        if (F == 0) return;
        if (!b->positions || !b->slice_energies) { err = "snb_evaluate_frames: positions and slice_energies must be given"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (b->mode != 1 && b->mode != 2) { err = "snb_evaluate_frames: mode must be 1 (every slice) or 2 (the slices of snb_set_energy_slices)"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        const int K = b->n_states;
        if (K < 0 || (K > 0 && (b->mode != 1 || !b->state_lambdas || !b->state_energies))) { err = "snb_evaluate_frames: lambda states need mode 1, state_lambdas and state_energies"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        const bool direct = b->include_direct != 0, recip = b->include_reciprocal != 0;
        const FrameInput in{"snb_evaluate_frames", F, b->positions, b->is_device == 0, b->is_double != 0, b->stride4 != 0, b->boxes};
        checkFrames(in, recip);
        const size_t rowLen = (size_t)S * 2;
        const bool hostOut = b->out_is_device == 0;
        double* rows = b->slice_energies;
        if (hostOut) { frameTab.resize((size_t)F * rowLen); rows = frameTab.p; }
        StepRequest req;      // one energy-only step per frame, its finish kernel writing the frame's row as well
        req.energy = b->mode == 2 ? StepEnergy::Selected : StepEnergy::All; req.direct = direct; req.recip = recip; req.forces = StepForces::None;
        runFrames(in, t0,
            [&](int f) { req.rowOut = rows + (size_t)f * rowLen; enqueueStep(req); },
            [&]() {
                double* states = b->state_energies;
                if (K > 0) {
                    pinned.upload(dStateLambdas, std::vector<double>(b->state_lambdas, b->state_lambdas + (size_t)K * rowLen), stream);
                    if (hostOut) { frameStates.resize((size_t)F * K); states = frameStates.p; }
                    launchFrameStateEnergies(rows, dStateLambdas.p, states, F, K, (int)rowLen, stream);
                }
                energyPending = true;      // (the engine's own buffer holds the last frame's sums)
                if (!hostOut) return false;
                // the one synchronisation of a batch with host output
                HIPCHECK(hipMemcpyAsync(b->slice_energies, rows, sizeof(double) * (size_t)F * rowLen, hipMemcpyDeviceToHost, stream));
                if (K > 0) HIPCHECK(hipMemcpyAsync(b->state_energies, states, sizeof(double) * (size_t)F * K, hipMemcpyDeviceToHost, stream));
                HIPCHECK(hipStreamSynchronize(stream));
                return true;
            });
    }
    void getFrameStats(snb_frame_stats* o) override { *o = fstats; }

    // SNB_OVERLAP_DEBUG: how the limited launch of the last overlapped step spread over the physical CUs (synchronises)
    void dumpOverlapTable() {
        std::vector<int> h(SNB_OVERLAP_INTS);
        HIPCHECK(hipStreamSynchronize(stream));
        HIPCHECK(hipMemcpy(h.data(), dOverlap.p, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
        int keys = 0, stayed = 0, arrived = 0, hist[8] = {0}; unsigned orKey = 0;
        const int* cu = h.data() + SNB_WORK_SHARDS * 32; int claims = 0; for (int k = 0; k < SNB_WORK_SHARDS; k++) claims += h[k * 32];
        int stayHist[8] = {0};
        for (int k = 0; k < SNB_CU_SLOTS; k++) if (cu[k] > 0) { const int arr = cu[k] & 0xFFFF, st = cu[k] >> 16; keys++; arrived += arr; stayed += st; hist[std::min(arr, 7)]++; stayHist[std::min(st, 7)]++; orKey |= (unsigned)k; }
        fprintf(stderr, "[snb] overlap: items claimed %d of %d; %d CU keys seen (or of keys 0x%x), %d work-groups arrived, %d stayed; arrivals per key 1..7+:", claims, numWorkItems, keys, orKey, arrived, stayed);
        for (int k = 1; k < 8; k++) fprintf(stderr, " %d", hist[k]);
        fprintf(stderr, "; CUs with 0..4 resident:");
        for (int k = 0; k < 5; k++) fprintf(stderr, " %d", stayHist[k]);
        fprintf(stderr, "\n");
        if (dOverlapTrace.p) {
            std::vector<int> t(SNB_CU_SLOTS * 8);
            HIPCHECK(hipMemcpy(t.data(), dOverlapTrace.p, sizeof(int) * t.size(), hipMemcpyDeviceToHost));
            int shown = 0;
            for (int k = 0; k < SNB_CU_SLOTS && shown < 12; k++) if (cu[k] > 0) {
                fprintf(stderr, "[snb] overlap: CU key 0x%03x arrivals %d, stayed %d: (GPR_ALLOC, LDS_ALLOC) of the first four:", k, cu[k] & 0xFFFF, cu[k] >> 16);
                for (int a = 0; a < 4; a++) fprintf(stderr, " (%08x, %08x)", (unsigned)t[(k * 4 + a) * 2], (unsigned)t[(k * 4 + a) * 2 + 1]);
                fprintf(stderr, "\n"); shown++;
            }
        }
    }

    // The raw slice energies of the last energy step, read back on demand (the only synchronisation of an energy / derivative step)
    void fetchSliceEnergies() {
        if (!energyPending) return;
        std::vector<double> dev((size_t)S * 2);
        HIPCHECK(hipMemcpyAsync(dev.data(), sliceTotal.p, sizeof(double) * dev.size(), hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
        hostSliceE = dev;
        energyPending = false;
    }

    // the pair kernels' view of the lists in use and of the method (p zeroed by the caller; need: the slices an energy step must produce);
    // the launch-specific fields stay with the caller
    void fillDirect(DirectParams<Real>& p, const int* need) {
        p.posq = posq.p; p.sigeps = sigeps.p; p.blockSubset = blockSubset.p; p.workItems = workItems.p;
        p.tileJ = tileJ.p; p.tileInfo = tileInfo.p; p.masks = masks.p; p.fx = fx.p; p.fy = fy.p; p.fz = fz.p; p.fs = fstride; p.fixed = fixedForces(); p.sliceE = sliceE.p; p.lambdas = dLambdas.p; p.sliceNeed = need;
        // the packed kernels' addressing (pair_addressing.h): 32-bit byte offsets while every array they index that way allows it
        const PairArrayExtents ext = {(int64_t)Npad, fstride, fixedForces(), (int64_t)std::min(tileJ.n / 32, tileInfo.n), (int64_t)(masks.n / 32)};
        p.fBytes = (unsigned)forceSlotBytes(fstride, fixedForces()); p.wideOffsets = pairOffsetsFit32(ext) ? 0 : 1;
        const int r = cfg.shard_rank, c = cfg.shard_count;
        (void)r; (void)c;
        p.workStart = 0; p.workStride = 1; p.numWork = numWorkItems;      // the lists hold only the i-blocks this engine owns (block % shard_count == shard_rank)
        p.nsub = nsub;
        p.cutoff2 = (Real)(cfg.cutoff * cfg.cutoff);
        p.krf = (Real)(std::pow(cfg.cutoff, -3.0) * (cfg.rf_dielectric - 1.0) / (2.0 * cfg.rf_dielectric + 1.0));
        p.crf = (Real)((1.0 / cfg.cutoff) * (3.0 * cfg.rf_dielectric) / (2.0 * cfg.rf_dielectric + 1.0));
        p.alpha = (Real)cfg.alpha; p.alphaD = (Real)cfg.alpha_d; p.k4pe = (Real)SNB_ONE_4PI_EPS0;
        p.alpha2l2e = (Real)(cfg.alpha * cfg.alpha * 1.4426950408889634);
        for (int i = 0; i <= EW_DEG; i++) p.ewPoly[i] = (Real)ewPoly[i];
        for (int i = 0; i < 14; i++) p.ewPolyE[i] = (Real)ewPolyE[i];
        for (int i = 0; i < 21; i++) p.dispPoly[i] = (Real)dispPoly[i];
        p.ewScale = (Real)(2.0 / ewR2Max);
        p.ewUsePoly = polyMask;
        const double ic2 = 1.0 / (cfg.cutoff * cfg.cutoff), ic6 = ic2 * ic2 * ic2;
        const double dar2 = cfg.alpha_d * cfg.alpha_d * cfg.cutoff * cfg.cutoff;
        p.invCut6 = (Real)ic6; p.multShift6 = (Real)(ic6 * (1.0 - std::exp(-dar2) * (1.0 + dar2 + 0.5 * dar2 * dar2)));
        p.useSwitch = useSwitch() ? 1 : 0; p.switchDist = (Real)cfg.switch_distance;
        p.invSwitchWidth = (Real)(useSwitch() ? 1.0 / (cfg.cutoff - cfg.switch_distance) : 0.0);
        for (int i = 0; i < 9; i++) p.box[i] = (Real)(gpuBuilt ? tileCell[i] : box[i]);
        if (isPeriodic()) { p.invBoxDiag[0] = (Real)(1.0 / box[0]); p.invBoxDiag[1] = (Real)(1.0 / box[4]); p.invBoxDiag[2] = (Real)(1.0 / box[8]); }
        p.boxDiag[0] = (Real)box[0]; p.boxDiag[1] = (Real)box[4]; p.boxDiag[2] = (Real)box[8];
    }
    // ... and of the O(N) pair lists: 1-4 exceptions and Ewald exclusion corrections
    void fillPairLists(PairListParams<Real>& q, const int* need) {
        q.posq = posq.p; q.fx = fx.p; q.fy = fy.p; q.fz = fz.p; q.fs = fstride; q.fixed = fixedForces(); q.sliceE = sliceE.p; q.lambdas = dLambdas.p; q.sliceNeed = need;
        const bool exPeriodic = (cfg.method == SNB_NoCutoff || cfg.method == SNB_CutoffNonPeriodic) ? false : cfg.exceptions_periodic != 0;
        q.periodic = exPeriodic ? 1 : 0; q.imageOffset = imageOffset.p;
        q.sigeps = sigeps.p; q.blockSubset = blockSubset.p; q.exclStart = exclStart.p; q.exclList = exclList.p; q.nSlices = S; q.sortedToUser = dSortedToUser.p; q.userToSorted = dUserToSorted.p;
        for (int i = 0; i < 9; i++) q.box[i] = (Real)box[i];
        q.alpha = (Real)cfg.alpha; q.alpha64 = cfg.alpha; q.alphaD = (Real)cfg.alpha_d; q.ljpme = cfg.method == SNB_LJPME;
        q.pairs = pairs14.p; q.params = params14.p; q.n = n14;
        q.nExclAtoms = (cfg.method >= SNB_Ewald && nExcl > 0) ? Npad : 0;
    }

    // The position-gather pass that opens a step or an atom pass: sorted positions, the displacement watch, `clearArrays` cleared force
    // arrays, and what gc is filled with here -- (recip, PME on the brick path) the packed Coulomb-mesh cell of every atom and the zeroed
    // stray counters, (clearEnergy) the cleared slice-energy partitions, (graphStep: a replayed forces step) the zeroed overlap counters
    // and the trace.  Returns whether the pass writes the mesh cells.
    bool enqueueGather(bool recip, bool clearEnergy, bool graphStep, int clearArrays) {
        GatherCells<Real> gc;
        std::memset(&gc, 0, sizeof(gc));
        bool cells = false;
        if (recip && isPme() && nGrids > 0) {
            PmeParams<Real> pp;
            std::memset(&pp, 0, sizeof(pp));
            fillPme(pp, pme, false, dSliceNeedAll.p);
            if (pp.sortNcx > 0 && pp.colRange != nullptr) {
                for (int i = 0; i < 9; i++) { gc.recip[i] = pp.recip[i]; gc.recipLo[i] = pp.recipLo[i]; }
                gc.nx = pp.d.nx; gc.ny = pp.d.ny; gc.nz = pp.d.nz; gc.cells = pp.cells; gc.atomGrid = pp.atomGrid;
                cells = true;
            }
        }
        if (cfg.neighbor_padding > 0 && posRef.p) {
            gc.posRef = posRef.p; gc.flags = dDispFlags;
            const double half = 0.5 * cfg.neighbor_padding;
            gc.fail2 = (Real)(half * half); gc.warn2 = (Real)(0.64 * half * half);      // rebuild request at 80 % of skin/2: the flag is read one step late
        }
        if (clearEnergy) { gc.clearE = sliceE.p; gc.nClearE = S * 2 * SNB_SLICE_E_PARTS; }
        if (recip && isPme() && dStrayCount.p) { gc.zeroInts = dStrayCount.p; gc.nZeroInts = 2; }
        if (graphStep && sw.overlap && dOverlap.p) { gc.zeroInts2 = dOverlap.p; gc.nZeroInts2 = SNB_OVERLAP_INTS; }
        gc.stepTrace = graphStep ? dStepTrace.p : nullptr;      // (SNB_STEP_TRACE; replayed steps only: the stamps of the last one are printed when the engine is destroyed)
        if (ctx.on) { gc.userToCtx = dUserToCtx.p; launchGatherPositions<Real>(ctx.posq, ctx.isDouble, 1, dSortedToUser.p, imageOffset.p, posq.p, Npad, forceBase, clearArrays, gc, stream); }
        else launchGatherPositions<Real>(devUserPos, posIsDouble, posStride4, dSortedToUser.p, imageOffset.p, posq.p, Npad, forceBase, clearArrays, gc, stream);
        return cells;
    }
    void enqueueStep(const StepRequest& r) {
        struct StampScope { StampScope(KernelStamps* k) { g_stamps = k; } ~StampScope() { g_stamps = nullptr; } };
        const bool energy = r.energy != StepEnergy::None, includeDirect = r.direct, includeRecip = r.recip;
        EvSet* const ev = r.ev; const StepForces fmode = r.forces; const int* const need = sliceNeed(r.energy);
        const bool forces = fmode != StepForces::None;
        const bool graphStep = !ev && fmode == StepForces::Full;      // (replayed forces steps: the only ones that overlap, fork or trace)
        const bool ctxForces = ctx.on && ctx.force && fmode == StepForces::Full;      // bound context: the step's last kernel adds into its fixed-point buffer
        void* const out = fmode == StepForces::Full ? (ctxForces ? (void*)ctx.force : outPtr) : nullptr;
        EnergyOut eo;
        std::memset(&eo, 0, sizeof(eo));
        if (ctx.on && energy) {
            eo.lambdas = dLambdas64.p; eo.energy = r.addCtxTotal ? ctx.energy : nullptr; eo.deriv = ctx.deriv; eo.derivSlot = dDerivSlot.p;
            eo.need = r.energy == StepEnergy::Selected ? need : nullptr; eo.isDouble = ctx.energyIsDouble;
        }
        if (ev) for (int k = 0; k < 16; k++) ev->ks.used[k] = false;
        const bool noStamps = sw.noKernelStamps;
        // (a stamped launch completes a signal of its own: ~8 us per kernel, 70 us per step with every PME kernel stamped -- measured: 20-step
        // region 0.484 ms per step against 0.467 without them.  Every third eager step carries the per-kernel stamps, starting with the
        // first one after snb_reset_timers; the pair-kernel and pipeline timers keep every eager step.)
        const bool fullStamps = ev && !noStamps && (stampCounter++ % 3 == 0);
        StampScope stampScope(fullStamps ? &ev->ks : nullptr);
        if (ev) HIPCHECK(hipEventRecord(ev->e[0], stream));
        const bool trace = graphStep && dStepTrace.p != nullptr;
        const bool cellsReady = enqueueGather(includeRecip, energy && Npad > 0, graphStep, forces ? forceArrays() : 0);
        if (energy && Npad <= 0) launchZeroFill(sliceE.p, sizeof(double) * S * 2 * SNB_SLICE_E_PARTS, stream);      // (inside the step graph: a kernel, not a memset node)
        // Opt-in (SNB_CONCURRENT_PME=1): forces-only graph steps run the reciprocal pipeline on a second stream beside the pair
        // kernel (disjoint force arrays fx.. / fpx..).  Timed (eager) steps stay serial so the per-kernel event timers stay clean.
        // overlapped step (see sw.overlap above): any graph step with both halves; needs the GPU-built work list (static item order is irrelevant)
        const bool overlap = graphStep && sw.overlap && includeDirect && includeRecip && isPme() && nGrids > 0 && stream2 && dOverlap.p && numWorkItems > 0 && shardTiles >= sw.overlapMinTiles;
        const bool fork = overlap || (graphStep && !energy && includeDirect && includeRecip && isPme() && nGrids > 0 && sw.concurrentPme && stream2);
        hipStream_t pmeStream = stream;
        if (fork) {
            HIPCHECK(hipEventRecord(evFork, stream));
            HIPCHECK(hipStreamWaitEvent(stream2, evFork, 0));
            pmeStream = stream2;
        }
        PairListParams<Real> q;
        std::memset(&q, 0, sizeof(q));
        // O(N) pair lists: one rank only when sharded -- the LAST one, which carries no PME grid once there are more ranks than grids
        const bool haveLists = includeDirect && cfg.shard_rank == cfg.shard_count - 1;
        if (haveLists) fillPairLists(q, need);
        bool listsDone = !haveLists, kernelTimed = false, finished = false, energyFinished = false;
        DirectParams<Real> directB; int directMc = 0;      // overlapped step: the second launch of the tile kernel
        std::memset(&directB, 0, sizeof(directB));
        if (includeDirect) {
            DirectParams<Real> p;
            std::memset(&p, 0, sizeof(p));
            fillDirect(p, need);
            const int mc = methodClass();
            const bool noFuse = sw.noFusedLists;
            p.stepTrace = trace ? dStepTrace.p : nullptr; p.traceSlot = 2;
            if (overlap) {      // first launch: resident beside the reciprocal pipeline, at most sw.overlapCuLimit work-groups per CU
                p.workCounter = dOverlap.p; p.cuSlots = dOverlap.p + SNB_WORK_SHARDS * 32; p.cuLimit = sw.overlapCuLimit;
                p.cuBaseMax = sw.overlapByCount ? -1 : 0x7fffffff;
                p.gridCap = sw.overlapGridA > 0 ? sw.overlapGridA : 6 * numCUs; p.listsLast = 1;
                p.cuTrace = dOverlapTrace.p;      // (SNB_OVERLAP_DEBUG; null otherwise)
                directB = p; directMc = mc;
                if (!sw.overlapByCount && p.cuLimit > 0) p.cuBaseMax = (p.cuLimit - 1) * pairVgprUnits[wrapMode][(int)r.energy];      // its resident work-groups sit below (cuLimit - 1) allocations of this kernel
            }
            if (!forces) { if (launchDirectEnergy<Real>(p, mc, wrapMode, (haveLists && !noFuse) ? &q : nullptr, stream, ev ? ev->e[1] : nullptr, ev ? ev->e[2] : nullptr, &kernelTimed)) listsDone = true; }
            else if (launchDirect<Real>(p, mc, wrapMode, (int)r.energy, (haveLists && !noFuse) ? &q : nullptr, stream, ev ? ev->e[1] : nullptr, ev ? ev->e[2] : nullptr, &kernelTimed)) listsDone = true;
        }
        if (ev && !kernelTimed) { HIPCHECK(hipEventRecord(ev->e[1], stream)); HIPCHECK(hipEventRecord(ev->e[2], stream)); }   // no tile kernel this step
        if (!listsDone) { if (forces) launchPairLists<Real>(q, energy, stream); else launchPairListsEnergy<Real>(q, stream); }
        if (overlap) HIPCHECK(hipEventRecord(evPairA, stream));      // the first launch of the tile kernel (and the pair lists) are done
        if (ev) HIPCHECK(hipEventRecord(ev->e[3], stream));
        if (includeRecip && isPme()) {
            if (nGrids > 0) {
                PmeParams<Real> pp;
                std::memset(&pp, 0, sizeof(pp));
                // the interpolation of the step's last mesh also writes the user-order force (no k_finishForces launch): unsharded, brick path,
                // reciprocal work on the step's own stream (the pair kernel's accumulators are complete by then)
                const bool noFuse = sw.noFusedFinish;
                // (an overlapped step keeps the fused finish: its last interpolation waits for both launches of the tile kernel)
                const bool canFinish = out && (!fork || overlap) && !noFuse && cfg.shard_count == 1;
                const bool noFusedE = sw.noFusedEnergyFinish;
                auto withOutput = [&](PmeParams<Real>& q, bool last) {
                    q.outForces = (canFinish && last) ? out : nullptr; q.outIsDouble = outIsDouble; q.outAccumulate = outAccumulate;
                    q.userToCtx = ctxForces ? dUserToCtx.p : nullptr; q.ctxStride = ctx.paddedN; q.ctxAtomic = sw.ctxAtomicAdd ? 1 : 0; q.finE = eo;
                    q.finOut = nullptr;
                    if (canFinish && last && energy && q.mix && !noFusedE) { q.finParts = sliceE.p; q.finOut = sliceTotal.p; q.finN = 2 * S; q.fin = makeSliceFinish(includeDirect, includeRecip); }
                    q.dfx = fx.p; q.dfy = fy.p; q.dfz = fz.p; q.dfs = fstride; q.dfixed = fixedForces(); q.sortedToUser = dSortedToUser.p;
                };
                // Overlapped step: everything up to the last mesh's inverse transform runs beside the resident first launch of the tile kernel;
                // then the second launch (unlimited: it takes what the first has not claimed, and the first keeps claiming) fills the chip,
                // and the last interpolation -- which also delivers the step's forces -- follows both.
                auto beforeLastInterpolation = [&]() {
                    if (!overlap) return;
                    directB.cuSlots = nullptr; directB.cuLimit = 0; directB.listsLast = 0; directB.traceSlot = 4; directB.gridCap = sw.overlapGridB > 0 ? sw.overlapGridB : 4 * numCUs;
                    bool t = false;
                    launchDirect<Real>(directB, directMc, wrapMode, (int)r.energy, nullptr, stream2, nullptr, nullptr, &t);
                    HIPCHECK(hipStreamWaitEvent(stream2, evPairA, 0));
                };
                // (energy-only steps: each mesh ends with its slice-energy Gram sums -- no mix, no inverse transforms, no interpolation)
                fillPme(pp, pme, energy, need, cellsReady, trace); withOutput(pp, cfg.method != SNB_LJPME); pp.energyOnly = forces ? 0 : 1;
                runPmeFront(pp, pmeStream);
                if (cfg.method != SNB_LJPME) beforeLastInterpolation();
                if (forces) { finished = launchPmeInterpolate<Real>(pp, pmeStream); energyFinished = finished && pp.finOut != nullptr; }
                if (cfg.method == SNB_LJPME) {
                    fillPme(pp, dpme, energy, need, cellsReady, trace); withOutput(pp, true); pp.energyOnly = forces ? 0 : 1;
                    runPmeFront(pp, pmeStream);
                    beforeLastInterpolation();
                    if (forces) { finished = launchPmeInterpolate<Real>(pp, pmeStream); energyFinished = finished && pp.finOut != nullptr; }
                }
            }
        }
        if (fork) { HIPCHECK(hipEventRecord(evJoin, stream2)); HIPCHECK(hipStreamWaitEvent(stream, evJoin, 0)); }
        if (includeRecip && cfg.method == SNB_Ewald && cfg.shard_rank == 0) runEwald(energy, forces);
        if (out && !finished) {   // the step's last kernel: user-order forces into the caller's buffer (part of the graph)
            const bool recipDone = includeRecip && (isPme() || cfg.method == SNB_Ewald);
            if (ctxForces) launchFinishForcesCtx<Real>(fx.p, fy.p, fz.p, fstride, fixedForces(), recipDone ? fpx.p : nullptr, fpy.p, fpz.p, dUserToSorted.p, N, ctx.force, dUserToCtx.p, ctx.paddedN, sw.ctxAtomicAdd ? 1 : 0, stream);
            else launchFinishForces<Real>(fx.p, fy.p, fz.p, fstride, fixedForces(), recipDone ? fpx.p : nullptr, fpy.p, fpz.p, dUserToSorted.p, N, out, outIsDouble, outAccumulate, stream);
        }
        if (energy) {
            const SliceFinish f = makeSliceFinish(includeDirect, includeRecip);
            if (!(finished && energyFinished))
            launchFinishSliceEnergies(sliceE.p, sliceTotal.p, 2 * S, f, eo, stream, r.rowOut);
        }
        if (ev) HIPCHECK(hipEventRecord(ev->e[4], stream));
    }

    // closed-form terms of the slice energies, added on the device (rank 0 only when sharded), as the reference GPU path keeps them next to its
    // kernels (CommonNonbondedSlicingKernels.cpp:618-638, 1129-1139)
    SliceFinish makeSliceFinish(bool includeDirect, bool includeRecip) const {
        SliceFinish f; std::memset(&f, 0, sizeof(f));
        if (cfg.shard_rank == 0) {
            const double volume = box[0] * box[4] * box[8];
            if (includeRecip && cfg.method >= SNB_Ewald) {
                f.sums = dParamSums.p;
                f.selfCoulomb = -SNB_ONE_4PI_EPS0 * cfg.alpha / std::sqrt(SNB_PI);
                f.selfDispersion = cfg.method == SNB_LJPME ? std::pow(cfg.alpha_d, 6.0) / 12.0 : 0.0;
                f.background = (-1.0 / (4 * cfg.alpha * cfg.alpha)) / (2 * SNB_EPSILON0 * volume);
            }
            if (includeDirect && (cfg.method == SNB_CutoffPeriodic || cfg.method == SNB_Ewald || cfg.method == SNB_PME)) { f.dispCoef = dDispCoef.p; f.invVolume = 1.0 / volume; }
        }
        return f;
    }

    // ------------------------------------------------------------------------------------------
    // Per-atom interaction energies (snb_evaluate_atom_energies): the table A[i][J][t] of every atom with every subset.
    // Behaves as an energy-only step behaves -- current box and positions (a binding's posq through the same gather), the neighbour-list
    // rules of any execute, plain launches, no step graph, no timer -- and writes only the table: no force array, no force output, no bound
    // buffer, neither the slice-energy partitions nor their sums.  Kernels: atomenergy.hip, atom_table.h.  Reciprocal part: the UNMIXED pipeline with every
    // mesh held (what a rank that owns all meshes runs), then the value part of the interpolation per (atom, mesh).
    // ------------------------------------------------------------------------------------------
    DevBuf<double> atomTab, atomOut;      // sorted-order working table [Npad][nsub][2]; user-order staging of a host result (both allocated at the first call)
    // The pass that fills a per-atom table (tab, sized by the caller, at least [Npad][nsub][rowDoubles]) for the lists, box and positions in
    // use: what snb_evaluate_atom_energies and snb_evaluate_atom_forces run between the neighbour-list rules and their finish kernels, and the
    // step of a group batch's frame.  forces chooses the kernels only: the pair and stencil launchers of atomforce.hip, else of atomenergy.hip.
    void enqueueAtomPass(bool includeDirect, bool includeRecip, double* tab, int rowDoubles, bool forces) {
        launchZeroFill(tab, sizeof(double) * (size_t)Npad * nsub * rowDoubles, stream);
        // what the pass asks of the shared step code is fixed: every slice, no trace, no row of a batch -- nothing of an earlier snb_execute
        const int* const need = sliceNeed(StepEnergy::All);
        // the position-gather pass of a step that clears nothing: sorted positions, the Coulomb-mesh cells, the displacement watch
        const bool recip = includeRecip && isPme() && nGrids > 0;
        const bool cellsReady = enqueueGather(recip, false, false, 0);
        if (includeDirect) {
            DirectParams<Real> p; PairListParams<Real> q;
            std::memset(&p, 0, sizeof(p)); std::memset(&q, 0, sizeof(q));
            fillDirect(p, need); fillPairLists(q, need);
            if (forces) launchAtomForcePairs<Real>(p, methodClass(), wrapMode, &q, tab, stream);
            else launchAtomPairs<Real>(p, methodClass(), wrapMode, &q, tab, stream);
        }
        if (recip) {
            PmeParams<Real> pp;
            std::memset(&pp, 0, sizeof(pp));
            auto mesh = [&](PmePlan<Real>& m) {      // the unmixed front of one mesh, then its part of every atom's row
                fillPme(pp, m, false, need, cellsReady); pp.mix = 0;
                runPmeFront(pp, stream);
                if (forces) launchAtomField<Real>(pp, tab, stream);
                else launchAtomPotential<Real>(pp, tab, stream);
            };
            mesh(pme);
            if (cfg.method == SNB_LJPME) mesh(dpme);
        }
    }
    // closed-form terms of a completed table row (the long-range dispersion correction is a per-slice constant: not attributed)
    SliceFinish makeAtomFinish(bool includeDirect, bool includeRecip) const { SliceFinish f = makeSliceFinish(includeDirect, includeRecip); f.dispCoef = nullptr; return f; }
    // The refusals the three analysis entry points share, in the order they are raised.  args: the argument checks (outName == nullptr: the
    // caller has checked its own outputs); state: what this engine cannot attribute to atoms.  The group calls (checkGroupCall) check their frame
    // count between the two.
    void refuseAtomCall(const std::string& who, const char* outName, const void* out, bool includeDirect, bool includeRecip, bool args, bool state) {
        if (args) {
            if (outName && !out) { err = who + ": " + outName + " is NULL"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
            if (!includeDirect && !includeRecip) { err = who + ": neither the direct nor the reciprocal part was asked for"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        }
        if (state) {
            if (cfg.shard_count > 1) { err = who + ": not available on sharded engines (a rank holds a part of the lists and of the meshes)"; throw (int)SNB_ERR_UNSUPPORTED; }
            if (cfg.method == SNB_Ewald && includeRecip) { err = who + ": the reciprocal sum of classic Ewald is not attributed to atoms (use PME, or include_reciprocal = 0)"; throw (int)SNB_ERR_UNSUPPORTED; }
        }
    }
    // snb_evaluate_atom_energies, or (forces) snb_evaluate_atom_forces: the kind of table sets the row (2 or 6 doubles), the working and
    // staging buffers (each call's own) and the finish kernel
    static constexpr int atomRow(bool forces) { return forces ? 6 : 2; }
    DevBuf<double>& atomTable(bool forces) { return forces ? atomFTab : atomTab; }
    void evaluateAtomTable(bool forces, int includeDirect, int includeRecip, double* out, int outIsDevice) override {
        const bool direct = includeDirect != 0, recip = includeRecip != 0;
        refuseAtomCall(forces ? "snb_evaluate_atom_forces" : "snb_evaluate_atom_energies", forces ? "atom_forces" : "atom_energies", out, direct, recip, true, true);
        beginExecute(false, includeRecip);
        DevBuf<double>& tab = atomTable(forces); DevBuf<double>& staged = forces ? atomFOut : atomOut;
        const size_t tabN = (size_t)Npad * nsub * atomRow(forces), outN = (size_t)N * nsub * atomRow(forces);
        tab.resize(tabN);
        if (!outIsDevice) staged.resize(outN);
        double* const dst = outIsDevice ? out : staged.p;
        enqueueAtomPass(direct, recip, tab.p, atomRow(forces), forces);
        if (forces) launchAtomForceFinish(tab.p, dUserToSorted.p, N, nsub, dst, stream);
        else launchAtomFinish<Real>(tab.p, dUserToSorted.p, blockSubset.p, posq.p, sigeps.p, N, nsub, makeAtomFinish(direct, recip), dst, stream);
        endExecute();
        if (!outIsDevice) {
            HIPCHECK(hipMemcpyAsync(out, staged.p, sizeof(double) * outN, hipMemcpyDeviceToHost, stream));
            HIPCHECK(hipStreamSynchronize(stream));
        }
    }

    // ------------------------------------------------------------------------------------------
    // Per-group interaction energies over stored frames (snb_evaluate_group_energies): the table above summed over
    // lists of atoms, on the device, per frame.  With frames: the frame loop of snb_evaluate_frames (runFrames) with the atom pass and the
    // group finish as the step.  Without: one evaluation under the rules of snb_evaluate_atom_energies.  Writes only its output: the working table,
    // the chunk sums and the staging of a host result are its own (atomTab is shared with snb_evaluate_atom_energies, which refills it).
    // ------------------------------------------------------------------------------------------
    DevBuf<int> dGroupPlan; DevBuf<double> groupPartial, groupOut;
    // What snb_evaluate_group_energies and snb_evaluate_group_forces check, in the order it is raised -- everything before anything is
    // enqueued or changed.  outputs: whether the caller's outputs are as they must be (else the message names outputNames).  Returns
    // whether there is work (false: n_frames == 0).
    bool checkGroupCall(const FrameInput& in, bool outputs, const char* outputNames, int G, const int32_t* start, const int32_t* atoms, bool direct, bool recip) {
        const std::string who = in.who;
        if (!outputs || !start || !atoms) { err = who + ": " + outputNames + ", group_start and group_atoms must be given"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (G < 1) { err = who + ": n_groups must be at least 1"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (start[0] != 0) { err = who + ": group_start[0] must be 0"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        for (int g = 0; g < G; g++) if (start[g + 1] < start[g]) { err = who + ": group_start decreases at group " + std::to_string(g); throw (int)SNB_ERR_INVALID_ARGUMENT; }
        for (int g = 0; g < G; g++) for (int e = start[g]; e < start[g + 1]; e++) {
            const int a = atoms[e];
            if (a < 0 || a >= N) { err = who + ": group " + std::to_string(g) + ": atom index " + std::to_string(a) + " is outside [0, " + std::to_string(N) + ")"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        }
        refuseAtomCall(who, nullptr, nullptr, direct, recip, true, false);
        if (in.F < 0) { err = who + ": negative frame count"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        refuseAtomCall(who, nullptr, nullptr, direct, recip, false, true);
        if (in.F == 0) return false;
        if (!in.positions && in.F != 1) { err = who + ": positions == NULL evaluates the engine's current state: n_frames must be 1"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (in.positions && ctx.on) { err = who + ": frames were given while a context is bound (snb_bind_context): the positions come from its posq"; throw (int)SNB_ERR_STATE; }
        if (in.positions) checkFrames(in, recip);
        return true;
    }
    // The two group calls: the checks; the lists packed with the work lists of the two mappings, one upload per call through the pinned ring;
    // then the engine's current state as the atom calls take it, or the frame loop with the atom pass and the group finish as the step; a host
    // result is copied back behind one synchronisation.  The table is the kind's own (atomTable).  Each call brings what is its own: sizes(plan)
    // sizes its chunk sums and staging (and uploads its states), finish(plan, f) launches its finish kernel for frame f -- before
    // evFrameStep[f & 1]: it reads the frame's list set -- and copyBack() enqueues the copies of a host result.
    struct GroupInput { int G; const int32_t* start; const int32_t* atoms; bool direct, recip, hostOut; };
    template <typename Sizes, typename Finish, typename CopyBack>
    void evaluateGroups(bool forces, const FrameInput& in, const GroupInput& g, bool outputs, const char* outputNames, Sizes&& sizes, Finish&& finish, CopyBack&& copyBack) {
        const auto t0 = std::chrono::steady_clock::now();
        if (!checkGroupCall(in, outputs, outputNames, g.G, g.start, g.atoms, g.direct, g.recip)) return;
        GroupPlan plan;
        planGroups(g.G, g.start, plan);
        std::copy(g.atoms, g.atoms + g.start[g.G], plan.packed.begin() + plan.offAtoms);
        DevBuf<double>& tab = atomTable(forces);
        auto prepare = [&]() { pinned.upload(dGroupPlan, plan.packed, stream); sizes(plan); };
        auto pass = [&](int f, int npad) {
            tab.resize((size_t)npad * nsub * atomRow(forces));
            enqueueAtomPass(g.direct, g.recip, tab.p, atomRow(forces), forces);
            finish(plan, f);
        };
        auto deliver = [&]() {
            if (!g.hostOut) return false;
            copyBack();
            HIPCHECK(hipStreamSynchronize(stream));
            return true;
        };
        if (!in.positions) {      // the engine's current state, as the atom calls take it
            beginExecute(false, g.recip);
            prepare();
            pass(0, Npad);
            endExecute();
            deliver();
            return;
        }
        prepare();
        // (the table is sized by the batch's padded-count prediction, in force from the first frame's build on: no allocation while a side build is in flight)
        runFrames(in, t0, [&](int f) { pass(f, std::max(Npad, npadPredict)); }, deliver);
    }
    void evaluateGroupEnergies(const snb_group_batch* b) override {
        const int G = b->n_groups, F = b->n_frames;
        const bool direct = b->include_direct != 0, recip = b->include_reciprocal != 0, hostOut = b->out_is_device == 0;
        const FrameInput in{"snb_evaluate_group_energies", F, b->positions, b->is_device == 0, b->is_double != 0, b->stride4 != 0, b->boxes};
        const size_t rowLen = (size_t)G * nsub * 2;
        double* rows = b->group_energies;
        evaluateGroups(false, in, {G, b->group_start, b->group_atoms, direct, recip, hostOut}, b->group_energies != nullptr, "group_energies",
            [&](const GroupPlan& plan) {
                groupPartial.resize((size_t)std::max(plan.nChunks, 1) * nsub * 2);
                if (hostOut) { groupOut.resize((size_t)F * rowLen); rows = groupOut.p; }
            },
            [&](const GroupPlan& plan, int f) {      // (reads userToSorted, blockSubset, posq and sigeps of this frame's list set)
                launchGroupFinish<Real>(atomTab.p, dUserToSorted.p, blockSubset.p, posq.p, sigeps.p, nsub, makeAtomFinish(direct, recip), plan, dGroupPlan.p, groupPartial.p, rows + (size_t)f * rowLen, stream);
            },
            [&]() { HIPCHECK(hipMemcpyAsync(b->group_energies, rows, sizeof(double) * (size_t)F * rowLen, hipMemcpyDeviceToHost, stream)); });
    }

    // ------------------------------------------------------------------------------------------
    // Per-atom forces by partner subset and term (snb_evaluate_atom_forces): G[i][J][t] = -dE_raw[slice(s_i, J)][t]/dr_i.
    // The frame, the refusals and the pass of snb_evaluate_atom_energies above (evaluateAtomTable), with the kernels of atomforce.hip: pair forces with every lambda 1
    // into both ends' columns, the derivative part of the interpolation per (atom, held mesh) of the unmixed pipeline, no closed-form term
    // (none carries a force).  Writes only its table; working and staging tables are its own.
    // ------------------------------------------------------------------------------------------
    DevBuf<double> atomFTab, atomFOut;      // sorted-order working table [Npad][nsub][2][3]; user-order staging of a host result (both allocated at the first call)

    // ------------------------------------------------------------------------------------------
    // Per-group forces over stored frames, by subset and at lambda states (snb_evaluate_group_forces): the force
    // table summed over lists of atoms on the device, per frame, and contracted per atom with K lambda states.  evaluateGroupEnergies with
    // the force pass as the step and the group-force finish of atomforce.hip.  Writes only its outputs: the chunk sums, the device copy of
    // the states and the staging of a host result are its own (atomFTab is shared with snb_evaluate_atom_forces, which refills it; the plan's
    // buffer with evaluateGroupEnergies, which uploads its own).
    // ------------------------------------------------------------------------------------------
    DevBuf<double> groupFPartial, groupFOut, groupFStates, dGroupLambdas;
    void evaluateGroupForces(const snb_group_force_batch* b) override {
        const int G = b->n_groups, F = b->n_frames, K = b->n_states;
        const FrameInput in{"snb_evaluate_group_forces", F, b->positions, b->is_device == 0, b->is_double != 0, b->stride4 != 0, b->boxes};
        if (K < 0) { err = std::string(in.who) + ": negative state count"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        const bool outputs = K > 0 ? (b->state_lambdas && b->state_forces) : b->group_forces != nullptr;
        const bool wantRows = b->group_forces != nullptr, hostOut = b->out_is_device == 0;
        const size_t rowLen = (size_t)G * nsub * 6, stateLen = (size_t)K * G * 3;
        double* rows = b->group_forces; double* states = b->state_forces;
        evaluateGroups(true, in, {G, b->group_start, b->group_atoms, b->include_direct != 0, b->include_reciprocal != 0, hostOut}, outputs, K > 0 ? "state_lambdas and state_forces" : "group_forces",
            [&](const GroupPlan& plan) {      // the states: one upload per call, through the pinned ring
                if (K > 0) pinned.upload(dGroupLambdas, std::vector<double>(b->state_lambdas, b->state_lambdas + (size_t)K * S * 2), stream);
                groupFPartial.resize((size_t)std::max(plan.nChunks, 1) * ((wantRows ? (size_t)nsub * 6 : 0) + (size_t)K * 3));
                if (hostOut && wantRows) { groupFOut.resize((size_t)F * rowLen); rows = groupFOut.p; }
                if (hostOut && K > 0) { groupFStates.resize((size_t)F * stateLen); states = groupFStates.p; }
            },
            [&](const GroupPlan& plan, int f) {      // (reads userToSorted and blockSubset of this frame's list set)
                launchGroupForceFinish(atomFTab.p, dUserToSorted.p, blockSubset.p, nsub, plan, dGroupPlan.p, dGroupLambdas.p, K, groupFPartial.p, wantRows ? rows + (size_t)f * rowLen : nullptr,
                                       K > 0 ? states + (size_t)f * stateLen : nullptr, stream);
            },
            [&]() {
                if (wantRows) HIPCHECK(hipMemcpyAsync(b->group_forces, rows, sizeof(double) * (size_t)F * rowLen, hipMemcpyDeviceToHost, stream));
                if (K > 0) HIPCHECK(hipMemcpyAsync(b->state_forces, states, sizeof(double) * (size_t)F * stateLen, hipMemcpyDeviceToHost, stream));
            });
    }

    // ------------------------------------------------------------------------------------------
    // Group-pair interaction energy matrix, direct space (snb_evaluate_group_pair_energies): the raw energies of the
    // tiles and of the two pair lists under slice(label_i, label_j) of the caller's G labels, per frame.  The frame, the refusals and the
    // neighbour-list rules of evaluateGroups above, with a step of its own: gather, zero fill, label gather, the tile launch of grouppairs.hip
    // with the direct parameters of the atom pass, the copy to the frame's row.  No PME call at all; any method, classic Ewald included.
    // Writes only its output: the labels (user and sorted order), the working matrix and the staging of a host result are its own.
    // ------------------------------------------------------------------------------------------
    DevBuf<int> dPairLabels, dPairLabelsSorted; DevBuf<double> groupPairTab, groupPairOut;
    void evaluateGroupPairEnergies(const snb_group_pair_batch* b) override {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string who = "snb_evaluate_group_pair_energies";
        const int G = b->n_groups, F = b->n_frames;
        const FrameInput in{"snb_evaluate_group_pair_energies", F, b->positions, b->is_device == 0, b->is_double != 0, b->stride4 != 0, b->boxes};
        // ---- everything is checked before anything is enqueued or changed
        if (!b->group_of_atom || !b->pair_energies) { err = who + ": group_of_atom and pair_energies must be given"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (G < 1 || G > 4096) { err = who + ": n_groups must lie in 1 .. 4096"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        for (int i = 0; i < N; i++) {
            const int l = b->group_of_atom[i];
            if (l < -1 || l >= G) { err = who + ": atom " + std::to_string(i) + ": label " + std::to_string(l) + " is outside [-1, " + std::to_string(G) + ")"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        }
        if (F < 0) { err = who + ": negative frame count"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (cfg.shard_count > 1) { err = who + ": not available on sharded engines (a rank holds a part of the lists)"; throw (int)SNB_ERR_UNSUPPORTED; }
        if (F == 0) return;
        if (!in.positions && F != 1) { err = who + ": positions == NULL evaluates the engine's current state: n_frames must be 1"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (in.positions && ctx.on) { err = who + ": frames were given while a context is bound (snb_bind_context): the positions come from its posq"; throw (int)SNB_ERR_STATE; }
        if (in.positions) checkFrames(in, false);
        const size_t rowLen = (size_t)G * (G + 1) / 2 * 2;
        // a small matrix is kept in copies (up to 64, 512 KB in all), a work-group adding into its own: few rows are hot rows
        int parts = 64;
        while (parts > 1 && parts * rowLen > 65536) parts >>= 1;
        const bool hostOut = b->out_is_device == 0;
        double* rows = b->pair_energies;
        auto prepare = [&]() {      // the labels: one upload per call, through the pinned ring
            pinned.upload(dPairLabels, std::vector<int>(b->group_of_atom, b->group_of_atom + N), stream);
            groupPairTab.resize(parts * rowLen);
            if (hostOut) { groupPairOut.resize((size_t)F * rowLen); rows = groupPairOut.p; }
        };
        auto pass = [&](int f, int npad) {
            dPairLabelsSorted.resize((size_t)npad);
            (void)enqueueGather(false, false, false, 0);      // sorted positions, the displacement watch; nothing cleared
            launchZeroFill(groupPairTab.p, sizeof(double) * parts * rowLen, stream);
            launchGroupPairLabels(dPairLabels.p, dSortedToUser.p, Npad, dPairLabelsSorted.p, stream);      // (reads this frame's list set: before evFrameStep[f & 1])
            const int* const need = sliceNeed(StepEnergy::All);
            DirectParams<Real> p; PairListParams<Real> q;
            std::memset(&p, 0, sizeof(p)); std::memset(&q, 0, sizeof(q));
            fillDirect(p, need); fillPairLists(q, need);
            launchGroupPairTiles<Real>(p, methodClass(), wrapMode, &q, dPairLabelsSorted.p, groupPairTab.p, parts, rowLen, stream);
            launchGroupPairFinish(groupPairTab.p, rowLen, parts, rows + (size_t)f * rowLen, stream);
        };
        auto deliver = [&]() {
            if (!hostOut) return false;
            HIPCHECK(hipMemcpyAsync(b->pair_energies, rows, sizeof(double) * (size_t)F * rowLen, hipMemcpyDeviceToHost, stream));
            HIPCHECK(hipStreamSynchronize(stream));
            return true;
        };
        if (!in.positions) {      // the engine's current state, as the atom calls take it
            beginExecute(false, 0);
            prepare();
            pass(0, Npad);
            endExecute();
            deliver();
            return;
        }
        prepare();
        // (the sorted labels are sized by the batch's padded-count prediction, in force from the first frame's build on: no allocation while a side build is in flight)
        runFrames(in, t0, [&](int f) { pass(f, std::max(Npad, npadPredict)); }, deliver);
    }

    // ------------------------------------------------------------------------------------------
    // Per-slice virial tensors, at the current state and over stored frames (snb_evaluate_slice_virials):
    // W[s][t][c] = -dE_raw[s][t]/d eps_c under a homogeneous deformation of box and atoms.  The frame, the refusals and the neighbour-list
    // rules of evaluateGroups above, with a step of its own: gather, zero fill, the tile launch of virial.hip with the direct parameters of
    // the atom pass, per mesh the three-pass front with the plane path off (the spectrum must reach memory) and the Gram kernel, the finish
    // into the frame's row.  Writes only its outputs: the working matrix, the device copy of the states, a row of its own when only the
    // states are asked for and the staging of a host result are its own.
    // ------------------------------------------------------------------------------------------
    DevBuf<double> virialTab, virialRow, virialOut, virialStates, dVirialLambdas;
    void evaluateSliceVirials(const snb_virial_batch* b) override {
        const auto t0 = std::chrono::steady_clock::now();
        const std::string who = "snb_evaluate_slice_virials";
        const int F = b->n_frames, K = b->n_states;
        const FrameInput in{"snb_evaluate_slice_virials", F, b->positions, b->is_device == 0, b->is_double != 0, b->stride4 != 0, b->boxes};
        // ---- everything is checked before anything is enqueued or changed
        if (K < 0) { err = who + ": negative state count"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (K > 0 ? !(b->state_lambdas && b->state_virials) : !b->slice_virials) { err = who + ": " + (K > 0 ? "state_lambdas and state_virials" : "slice_virials") + " must be given"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        const bool direct = b->include_direct != 0, recip = b->include_reciprocal != 0;
        refuseAtomCall(who, nullptr, nullptr, direct, recip, true, false);
        if (F < 0) { err = who + ": negative frame count"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        refuseAtomCall(who, nullptr, nullptr, direct, recip, false, true);
        if (F == 0) return;
        if (!in.positions && F != 1) { err = who + ": positions == NULL evaluates the engine's current state: n_frames must be 1"; throw (int)SNB_ERR_INVALID_ARGUMENT; }
        if (in.positions && ctx.on) { err = who + ": frames were given while a context is bound (snb_bind_context): the positions come from its posq"; throw (int)SNB_ERR_STATE; }
        if (in.positions) checkFrames(in, recip);
        const size_t rowLen = (size_t)S * 12, stateLen = (size_t)K * 6;
        const bool wantRows = b->slice_virials != nullptr, hostOut = b->out_is_device == 0;
        double* rows = b->slice_virials; double* states = b->state_virials;
        auto prepare = [&]() {      // the states: one upload per call, through the pinned ring
            if (K > 0) pinned.upload(dVirialLambdas, std::vector<double>(b->state_lambdas, b->state_lambdas + (size_t)K * S * 2), stream);
            virialTab.resize((size_t)SNB_SLICE_E_PARTS * rowLen);
            if (!wantRows) virialRow.resize(rowLen);
            else if (hostOut) { virialOut.resize((size_t)F * rowLen); rows = virialOut.p; }
            if (hostOut && K > 0) { virialStates.resize((size_t)F * stateLen); states = virialStates.p; }
        };
        auto pass = [&](int f) {
            const bool mesh = recip && isPme() && nGrids > 0;
            const bool cellsReady = enqueueGather(mesh, false, false, 0);      // sorted positions, the Coulomb-mesh cells, the displacement watch; nothing cleared
            launchZeroFill(virialTab.p, sizeof(double) * SNB_SLICE_E_PARTS * rowLen, stream);
            const int* const need = sliceNeed(StepEnergy::All);
            if (direct) {
                DirectParams<Real> p; PairListParams<Real> q;
                std::memset(&p, 0, sizeof(p)); std::memset(&q, 0, sizeof(q));
                fillDirect(p, need); fillPairLists(q, need);
                launchVirialTiles<Real>(p, methodClass(), wrapMode, &q, virialTab.p, stream);
            }
            if (mesh) {
                double r[9]; recipBoxRows(box, r);
                auto one = [&](PmePlan<Real>& m) {      // the unmixed forward spectrum of one mesh, then its Gram sums
                    PmeParams<Real> pp;
                    std::memset(&pp, 0, sizeof(pp));
                    fillPme(pp, m, false, need, cellsReady); pp.mix = 0; pp.planeB = nullptr; pp.planeEterm = nullptr;
                    const int zDone = launchPmeSpread<Real>(pp, stream);
                    if (zDone == 2) throw HipError{who + ": the spreader took the plane path with its buffers withheld"};
                    launchPmeForwardFFT<Real>(pp, stream, zDone == 1);
                    launchPmeFFTX<Real>(pp, -1, stream);
                    VirialMesh<Real> v;
                    std::memset(&v, 0, sizeof(v));
                    v.spectrum = pp.gridCplx; v.modx = pp.modx; v.mody = pp.mody; v.modz = pp.modz; v.gridSubset = pp.gridSubset;
                    v.nx = pp.d.nx; v.ny = pp.d.ny; v.nz = pp.d.nz; v.nzc = pp.d.nzc; v.nsub = pp.nsub; v.nsubTotal = nsub; v.dispersion = pp.dispersion;
                    for (int i = 0; i < 9; i++) v.recip[i] = r[i];
                    v.alpha = m.alpha; v.volume = box[0] * box[4] * box[8];
                    launchVirialGram<Real>(v, virialTab.p, stream);
                };
                one(pme);
                if (cfg.method == SNB_LJPME) one(dpme);
            }
            SliceFinish fin; std::memset(&fin, 0, sizeof(fin));
            if (isPeriodic()) fin = makeSliceFinish(direct, recip);
            launchVirialFinish(virialTab.p, S, fin, wantRows ? rows + (size_t)f * rowLen : virialRow.p, dVirialLambdas.p, K, K > 0 ? states + (size_t)f * stateLen : nullptr, stream);
        };
        auto deliver = [&]() {
            if (!hostOut) return false;
            if (wantRows) HIPCHECK(hipMemcpyAsync(b->slice_virials, rows, sizeof(double) * (size_t)F * rowLen, hipMemcpyDeviceToHost, stream));
            if (K > 0) HIPCHECK(hipMemcpyAsync(b->state_virials, states, sizeof(double) * (size_t)F * stateLen, hipMemcpyDeviceToHost, stream));
            HIPCHECK(hipStreamSynchronize(stream));
            return true;
        };
        if (!in.positions) {      // the engine's current state, as the atom calls take it
            beginExecute(false, recip);
            prepare();
            pass(0);
            endExecute();
            deliver();
            return;
        }
        prepare();
        runFrames(in, t0, pass, deliver);
    }

    // classic Ewald: half-space k-vectors in the reference's enumeration order (ReferenceSlicedLJCoulombIxn.cpp:288-355)
    void runEwald(bool energy, bool forces) {
        if (hKvec.empty()) {
            int lowry = 0, lowrz = 1;
            for (int rx = 0; rx < cfg.kmax[0]; rx++) {
                for (int ry = lowry; ry < cfg.kmax[1]; ry++) {
                    for (int rz = lowrz; rz < cfg.kmax[2]; rz++) { hKvec.push_back(make_int3(rx, ry, rz)); lowrz = 1 - cfg.kmax[2]; }
                    lowry = 1 - cfg.kmax[1];
                }
            }
            dKvec.upload(hKvec, stream);
            dCosSin.resize(hKvec.size() * 2 * nsub);
        }
        EwaldParams<Real> q;
        std::memset(&q, 0, sizeof(q));
        q.natoms = Npad; q.nsub = nsub; q.nk = (int)hKvec.size(); q.posq = posq.p; q.atomSubset = atomSubset.p; q.kvec = dKvec.p; q.cosSin = dCosSin.p;
        q.recipBox[0] = (Real)(2 * SNB_PI / box[0]); q.recipBox[1] = (Real)(2 * SNB_PI / box[4]); q.recipBox[2] = (Real)(2 * SNB_PI / box[8]);
        q.factorEwald = -1 / (4 * cfg.alpha * cfg.alpha); q.recipCoeff = SNB_ONE_4PI_EPS0 * 4 * SNB_PI / (box[0] * box[4] * box[8]);
        q.lambdas = dLambdas.p; q.sliceE = sliceE.p; q.wantEnergy = energy ? 1 : 0; q.fpx = fpx.p; q.fpy = fpy.p; q.fpz = fpz.p;
        launchEwald<Real>(q, stream, forces);      // (forces == false: structure factors and energies only)
    }

    void harvest(EvSet& ev) {
        HIPCHECK(hipEventSynchronize(ev.e[4]));
        float a = 0, b = 0, c = 0;
        HIPCHECK(hipEventElapsedTime(&a, ev.e[1], ev.e[2]));
        HIPCHECK(hipEventElapsedTime(&b, ev.e[3], ev.e[4]));
        HIPCHECK(hipEventElapsedTime(&c, ev.e[0], ev.e[4]));
        stats.last_direct_ms = a; stats.last_recip_ms = b; stats.last_total_ms = c;
        stats.sum_direct_ms += a; stats.sum_recip_ms += b; stats.sum_total_ms += c; stats.n_timed++;
        for (int k = 0; k < 16; k++) if (ev.ks.used[k]) {
            float t = 0;
            if (hipEventElapsedTime(&t, ev.ks.start[k], ev.ks.stop[k]) == hipSuccess) { stats.sum_kernel_ms[k] += t; stats.n_kernel_timed[k]++; }
            ev.ks.used[k] = false;
        }
        ev.pending = false;
    }
    // (also restarts the eager-step cadence: the first step after a reset is a timed one, so even a short measured region has a sample)
    void resetTimers() override { for (auto& r : ring) if (r.pending) harvest(r); stats.sum_direct_ms = stats.sum_recip_ms = stats.sum_total_ms = 0; stats.n_timed = 0; for (int k = 0; k < 16; k++) { stats.sum_kernel_ms[k] = 0; stats.n_kernel_timed[k] = 0; } execCount = 0; stampCounter = 0; }

    void runPmeFront(PmeParams<Real>& pp, hipStream_t st) {      // one mesh up to its potentials in real space; launchPmeInterpolate follows
        const int zDone = launchPmeSpread<Real>(pp, st);
        if (zDone == 2) launchPmePlanePath<Real>(pp, st);      // per-plane x / y transforms + convolution in LDS, then mix + inverse z
        else {
            launchPmeForwardFFT<Real>(pp, st, zDone == 1);
            launchPmeConvolution<Real>(pp, st);
            if (!pp.energyOnly) launchPmeInverseFFT<Real>(pp, st);
        }
    }

    void setForceOutput(void* out, int isDouble, int accumulate) override { if (out) ctx.force = nullptr;      // (takes the place of a bound force buffer)
        outPtr = out; outIsDouble = isDouble; outAccumulate = accumulate; outputWritten = false; }
    void getForces(void* out, int isDevice, int isDouble, int accumulate) override {
        if (isDevice && out == outPtr && isDouble == outIsDouble && outputWritten) return;   // the last execute already delivered them there
        const size_t bytes = (size_t)N * 3 * (isDouble ? 8 : 4);
        // the live force set, or the copy kept before an energy-only step re-sorted the atoms (keepLastForces)
        const ForceSet f = keptValid ? forceSet(keptForces.p, keptNpad) : ForceSet{fx.p, fy.p, fz.p, fpx.p, fpy.p, fpz.p};
        const int* u2s = keptValid ? keptUserToSorted.p : dUserToSorted.p;
        const Real* px = (keptValid ? keptRecip : lastRecip) ? f.px : nullptr;
        if (isDevice) { launchFinishForces<Real>(f.x, f.y, f.z, fstride, fixedForces(), px, f.py, f.pz, u2s, N, out, isDouble, accumulate, stream); return; }
        DevBuf<unsigned char> tmp; tmp.resize(bytes);
        if (accumulate) HIPCHECK(hipMemcpyAsync(tmp.p, out, bytes, hipMemcpyHostToDevice, stream));
        launchFinishForces<Real>(f.x, f.y, f.z, fstride, fixedForces(), px, f.py, f.pz, u2s, N, tmp.p, isDouble, accumulate, stream);
        HIPCHECK(hipMemcpyAsync(out, tmp.p, bytes, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipStreamSynchronize(stream));
    }
    const double* sliceEnergiesDevice() override { return sliceTotal.p; }
    void getSliceEnergies(double* out) override { fetchSliceEnergies(); std::memcpy(out, hostSliceE.data(), sizeof(double) * S * 2); }
    void getStats(snb_stats* o) override {
        HIPCHECK(hipStreamSynchronize(stream));
        stats.n_tiles = 0;
        // tiles processed by this shard
        stats.n_list_overruns = listOverruns + (hDispFlags ? hDispFlags[4] + (hDispFlags[1] ? 1 : 0) : 0);
        stats.n_tiles = shardTiles; stats.n_blocks = numBlocks; stats.n_padded_atoms = Npad; stats.n_exclusion_tiles = numMaskTiles;
        for (int d = 0; d < 3; d++) { stats.grid[d] = isPme() ? pme.d.nx * (d == 0) + pme.d.ny * (d == 1) + pme.d.nz * (d == 2) : 0; stats.dgrid[d] = cfg.method == SNB_LJPME ? dpme.d.nx * (d == 0) + dpme.d.ny * (d == 1) + dpme.d.nz * (d == 2) : 0; }
        for (int k = 0; k < RING; k++) { EvSet& r = ring[(ringPos + k) % RING]; if (r.pending) harvest(r); }
        stats.n_spread_strays = 0;
        if (dStrayCount.p) { int h[2] = {0, 0}; HIPCHECK(hipMemcpy(h, dStrayCount.p, sizeof(h), hipMemcpyDeviceToHost)); stats.n_spread_strays = (int64_t)h[0] + h[1]; }
        *o = stats;
    }
    void getPme(double* alpha, int32_t* g, bool dispersion) override {
        if (dispersion) { *alpha = cfg.alpha_d; g[0] = dpme.d.nx; g[1] = dpme.d.ny; g[2] = dpme.d.nz; }
        else { *alpha = cfg.alpha; g[0] = pme.d.nx; g[1] = pme.d.ny; g[2] = pme.d.nz; }
    }
};

template <typename Real> static void testFFT(int device, int batch, int nx, int ny, int nz, const double* in, double* spectrum, double* roundtrip) {
    HIPCHECK(hipSetDevice(device));
    hipStream_t s; HIPCHECK(hipStreamCreate(&s));
    {
        PmePlan<Real> plan; int g[3] = {nx, ny, nz};
        plan.init(g, batch, s);
        PmeParams<Real> p; std::memset(&p, 0, sizeof(p));
        p.d = plan.d; p.nsub = batch; p.gridReal = plan.gridReal.p; p.gridCplx = plan.gridCplx.p; p.twx = plan.twx.p; p.twy = plan.twy.p; p.twz = plan.twz.p;
        const size_t nr = (size_t)batch * nx * ny * nz, ncx = (size_t)batch * nx * ny * (nz / 2 + 1);
        std::vector<Real> h(nr);
        for (size_t i = 0; i < nr; i++) h[i] = (Real)in[i];
        HIPCHECK(hipMemcpyAsync(plan.gridReal.p, h.data(), sizeof(Real) * nr, hipMemcpyHostToDevice, s));
        launchPmeForwardFFT<Real>(p, s, false);
        launchPmeFFTX<Real>(p, -1, s);
        std::vector<typename Vec<Real>::T2> hc(ncx);
        HIPCHECK(hipMemcpyAsync(hc.data(), plan.gridCplx.p, sizeof(typename Vec<Real>::T2) * ncx, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        for (size_t i = 0; i < ncx; i++) { spectrum[2 * i] = hc[i].x; spectrum[2 * i + 1] = hc[i].y; }
        launchPmeFFTX<Real>(p, +1, s);
        launchPmeInverseFFT<Real>(p, s);
        HIPCHECK(hipMemcpyAsync(h.data(), plan.gridReal.p, sizeof(Real) * nr, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        for (size_t i = 0; i < nr; i++) roundtrip[i] = h[i];
    }
    HIPCHECK(hipStreamDestroy(s));
}

}  // namespace snb

// =====================================================================================================
// C ABI
// =====================================================================================================
using namespace snb;

struct snb_engine { EngineBase* impl; };

// Every entry point runs on the engine's own device and leaves the caller's current device as it found it (a process that drives
// several GPUs -- torch, OpenMM with several contexts -- switches the current device between calls).
struct DeviceScope {
    int prev = -1; bool switched = false;
    explicit DeviceScope(int dev) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess; }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};

template <typename F> static snb_status guard(snb_handle h, F&& f) {
    if (!h || !h->impl) return SNB_ERR_INVALID_ARGUMENT;
    DeviceScope scope(h->impl->cfg.device);
    try { f(); return SNB_OK; }
    catch (HipError& e) { h->impl->err = e.msg; return e.msg.find("hip") == 0 ? SNB_ERR_HIP : SNB_ERR_INVALID_ARGUMENT; }
    catch (int code) { return (snb_status)code; }
    catch (std::exception& e) { h->impl->err = e.what(); return SNB_ERR_INVALID_ARGUMENT; }
}

extern "C" {

int32_t snb_abi_version(void) { return SNB_ABI_VERSION; }
int32_t snb_legal_grid_size(int32_t n) { return legalGridSize(n); }

snb_status snb_create(const snb_config* cfg, snb_handle* out) {
    if (!cfg || !out) { g_createError = "null argument"; return SNB_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (cfg->abi_version != SNB_ABI_VERSION) { g_createError = "snb_config.abi_version mismatch"; return SNB_ERR_INVALID_ARGUMENT; }
    if (cfg->n_atoms < 0 || cfg->n_subsets < 1 || cfg->method < 0 || cfg->method > 5 || (cfg->precision != SNB_SINGLE && cfg->precision != SNB_DOUBLE && cfg->precision != SNB_MIXED)) {
        g_createError = "invalid n_atoms / n_subsets / method / precision"; return SNB_ERR_INVALID_ARGUMENT;
    }
    if (cfg->method != SNB_NoCutoff && !(cfg->cutoff > 0)) { g_createError = "cutoff must be positive"; return SNB_ERR_INVALID_ARGUMENT; }
    if (cfg->method >= SNB_Ewald && !(cfg->alpha > 0)) { g_createError = "alpha must be given explicitly for Ewald/PME/LJPME"; return SNB_ERR_INVALID_ARGUMENT; }
    if ((cfg->method == SNB_PME || cfg->method == SNB_LJPME) && (cfg->grid[0] < 1 || cfg->grid[1] < 1 || cfg->grid[2] < 1)) { g_createError = "PME grid must be given explicitly"; return SNB_ERR_INVALID_ARGUMENT; }
    if (cfg->method == SNB_LJPME && (!(cfg->alpha_d > 0) || cfg->dgrid[0] < 1 || cfg->dgrid[1] < 1 || cfg->dgrid[2] < 1)) { g_createError = "LJPME dispersion alpha/grid must be given explicitly"; return SNB_ERR_INVALID_ARGUMENT; }
    if (cfg->shard_count > 1 && (cfg->shard_rank < 0 || cfg->shard_rank >= cfg->shard_count)) { g_createError = "invalid shard_rank"; return SNB_ERR_INVALID_ARGUMENT; }
    // every shard must re-sort and rebuild on the SAME execute (sorted order, padded count and block ownership are per-rebuild facts all ranks share);
    // the displacement-triggered mode decides from a flag each rank sees at its own time, so sharded engines take a fixed interval (or
    // the caller agrees on the step itself and calls snb_rebuild_neighbors on every rank)
    if (cfg->shard_count > 1 && cfg->rebuild_interval < 0) { g_createError = "rebuild_interval < 0 (displacement-triggered rebuilds) is not available with shard_count > 1"; return SNB_ERR_UNSUPPORTED; }
    try {
        (void)switches();      // the environment is read here, once per process, before anything touches the GPU
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_createError = "hip: no HIP device available (the engine has no CPU fallback)"; return SNB_ERR_HIP; }
        if (cfg->device < 0 || cfg->device >= ndev) { g_createError = "invalid device ordinal"; return SNB_ERR_INVALID_ARGUMENT; }
        DeviceScope scope(cfg->device);
        {      // LDS requests that grow with the subset count (pme_sizes.h): what cannot run is refused here, not skipped at the launch
            char msg[320];
            const long long nSlices = (long long)cfg->n_subsets * (cfg->n_subsets + 1) / 2;
            if (!pairListLdsFits(nSlices)) {
                snprintf(msg, sizeof(msg), "n_subsets = %d: the pair-list energy kernels reduce %lld slices in %zu bytes of LDS, more than the %zu they may request",
                         (int)cfg->n_subsets, nSlices, pairListLds(nSlices), kPairListLdsMax);
                g_createError = msg; return SNB_ERR_UNSUPPORTED;
            }
            if (cfg->method == SNB_PME || cfg->method == SNB_LJPME) {
                hipDeviceProp_t prop;
                if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) { g_createError = "hip: hipGetDeviceProperties failed"; return SNB_ERR_HIP; }
                // (a work-group may raise its limit to all the LDS of a compute unit: hipFuncAttributeMaxDynamicSharedMemorySize)
                const size_t limit = std::max((size_t)prop.sharedMemPerBlock, (size_t)prop.maxSharedMemoryPerMultiProcessor);
                const int shards = cfg->shard_count > 1 ? cfg->shard_count : 1;
                const int nGrids = (cfg->n_subsets - (shards > 1 ? cfg->shard_rank : 0) + shards - 1) / shards;      // the meshes this engine holds
                const size_t realBytes = cfg->precision == SNB_DOUBLE ? 8 : 4;
                for (int mesh = 0; mesh < (cfg->method == SNB_LJPME ? 2 : 1); mesh++) {
                    const int nx = legalGridSize(mesh ? cfg->dgrid[0] : cfg->grid[0]);
                    if (nGrids > 0 && !convLdsFits(nx, nGrids, realBytes, limit)) {
                        snprintf(msg, sizeof(msg), "%s mesh with nx = %d and %d subsets in %s precision: the x kernel of the reciprocal sum needs %zu bytes of LDS at one column per work-group, the device has %zu",
                                 mesh ? "dispersion" : "PME", nx, nGrids, realBytes == 8 ? "double" : "single", convLdsNeed(nx, nGrids, realBytes), limit);
                        g_createError = msg; return SNB_ERR_UNSUPPORTED;
                    }
                }
            }
        }
        EngineBase* e = cfg->precision == SNB_DOUBLE ? (EngineBase*)new Engine<double>(*cfg) : (EngineBase*)new Engine<float>(*cfg);
        *out = new snb_engine{e};
        return SNB_OK;
    } catch (HipError& e) { g_createError = e.msg; return SNB_ERR_HIP; }
    catch (std::exception& e) { g_createError = e.what(); return SNB_ERR_INVALID_ARGUMENT; }
}

void snb_destroy(snb_handle h) { if (h) { if (h->impl) { DeviceScope scope(h->impl->cfg.device); delete h->impl; } delete h; } }
const char* snb_last_error(snb_handle h) { return h && h->impl ? h->impl->err.c_str() : g_createError.c_str(); }

snb_status snb_set_particles(snb_handle h, const double* q, const double* s, const double* e, const int32_t* sub) {
    if (!q || !s || !e || !sub) return SNB_ERR_INVALID_ARGUMENT;
    return guard(h, [&] { h->impl->setParticles(q, s, e, sub); });
}
snb_status snb_set_exceptions(snb_handle h, int32_t m, const int32_t* pairs, const double* qq, const double* s, const double* e, const int32_t* f14) {
    if (m < 0 || (m > 0 && (!pairs || !qq || !s || !e))) return SNB_ERR_INVALID_ARGUMENT;
    return guard(h, [&] { h->impl->setExceptions(m, pairs, qq, s, e, f14); });
}
snb_status snb_set_parameter_offsets(snb_handle h, int32_t nGlobals, int32_t nP, const int32_t* particle, const int32_t* pGlobal, const double* pDelta,
                                     int32_t nE, const int32_t* exception, const int32_t* eGlobal, const double* eDelta) {
    if ((nP > 0 && (!particle || !pGlobal || !pDelta)) || (nE > 0 && (!exception || !eGlobal || !eDelta))) return SNB_ERR_INVALID_ARGUMENT;
    return guard(h, [&] { h->impl->setParameterOffsets(nGlobals, nP, particle, pGlobal, pDelta, nE, exception, eGlobal, eDelta); });
}
snb_status snb_set_global_parameters(snb_handle h, int32_t n, const double* values) {
    if (n < 0 || (n > 0 && !values)) return SNB_ERR_INVALID_ARGUMENT;
    return guard(h, [&] { h->impl->setGlobalParameters(n, values); });
}
snb_status snb_set_energy_slices(snb_handle h, const int32_t* mask) { if (!mask) return SNB_ERR_INVALID_ARGUMENT; return guard(h, [&] { h->impl->setEnergySlices(mask); }); }
snb_status snb_set_lambdas(snb_handle h, const double* l) { if (!l) return SNB_ERR_INVALID_ARGUMENT; return guard(h, [&] { h->impl->setLambdas(l); }); }
snb_status snb_set_dispersion_coefficients(snb_handle h, const double* c) { return guard(h, [&] { h->impl->setDispersion(c); }); }
snb_status snb_compute_dispersion_coefficients(int32_t n, int32_t nsub, const double* sigma, const double* epsilon, const int32_t* subset, double cutoff,
                                               int32_t useSwitch, double switchDist, double* out) {
    if (n < 0 || nsub < 1 || !out || (n > 0 && (!sigma || !epsilon || !subset))) return SNB_ERR_INVALID_ARGUMENT;
    dispersionCoefficients(n, nsub, sigma, epsilon, subset, cutoff, useSwitch, switchDist, out);
    return SNB_OK;
}
snb_status snb_set_box(snb_handle h, const double* b) { if (!b) return SNB_ERR_INVALID_ARGUMENT; return guard(h, [&] { h->impl->setBox(b); }); }
snb_status snb_set_positions(snb_handle h, const void* pos, int32_t isDevice, int32_t isDouble, int32_t stride4) {
    if (!pos) return SNB_ERR_INVALID_ARGUMENT;
    return guard(h, [&] { h->impl->setPositions(pos, isDevice, isDouble, stride4); });
}
snb_status snb_rebuild_neighbors(snb_handle h) { return guard(h, [&] { h->impl->requestRebuild(); }); }
snb_status snb_execute(snb_handle h, int32_t f, int32_t e, int32_t d, int32_t r, double* energy) { return guard(h, [&] { h->impl->execute(f, e, d, r, energy); }); }
snb_status snb_get_forces(snb_handle h, void* out, int32_t isDevice, int32_t isDouble, int32_t acc) {
    if (!out) return SNB_ERR_INVALID_ARGUMENT;
    return guard(h, [&] { h->impl->getForces(out, isDevice, isDouble, acc); });
}
snb_status snb_set_shard_blocks(snb_handle h, int32_t begin, int32_t end, int32_t period) { return guard(h, [&] { h->impl->setShardBlocks(begin, end, period); }); }
snb_status snb_set_force_output(snb_handle h, void* out, int32_t isDouble, int32_t acc) { return guard(h, [&] { h->impl->setForceOutput(out, isDouble, acc); }); }
snb_status snb_bind_context(snb_handle h, const snb_context_binding* b) { return guard(h, [&] { h->impl->bindContext(b); }); }
snb_status snb_context_order_changed(snb_handle h) { return guard(h, [&] { h->impl->contextOrderChanged(); }); }
snb_status snb_get_slice_energies(snb_handle h, double* out) { if (!out) return SNB_ERR_INVALID_ARGUMENT; return guard(h, [&] { h->impl->getSliceEnergies(out); }); }
snb_status snb_slice_energies_device(snb_handle h, const double** out) { if (!out) return SNB_ERR_INVALID_ARGUMENT; return guard(h, [&] { *out = h->impl->sliceEnergiesDevice(); }); }
snb_status snb_synchronize(snb_handle h) { return guard(h, [&] { h->impl->sync(); }); }
snb_status snb_get_pme_parameters(snb_handle h, double* alpha, int32_t grid[3]) {
    if (!h || !h->impl || !alpha || !grid) return SNB_ERR_INVALID_ARGUMENT;
    if (h->impl->cfg.method != SNB_PME && h->impl->cfg.method != SNB_LJPME) { h->impl->err = "getPMEParametersInContext: This Context is not using PME or LJPME"; return SNB_ERR_NOT_PME; }
    return guard(h, [&] { h->impl->getPme(alpha, grid, false); });
}
snb_status snb_get_ljpme_parameters(snb_handle h, double* alpha, int32_t grid[3]) {
    if (!h || !h->impl || !alpha || !grid) return SNB_ERR_INVALID_ARGUMENT;
    if (h->impl->cfg.method != SNB_LJPME) { h->impl->err = "getPMEParametersInContext: This Context is not using LJPME"; return SNB_ERR_NOT_PME; }
    return guard(h, [&] { h->impl->getPme(alpha, grid, true); });
}
snb_status snb_reset_timers(snb_handle h) { return guard(h, [&] { h->impl->resetTimers(); }); }
snb_status snb_set_timing_interval(snb_handle h, int32_t n) { return guard(h, [&] { h->impl->setTimingInterval(n); }); }
snb_status snb_get_stats(snb_handle h, snb_stats* out) { if (!out) return SNB_ERR_INVALID_ARGUMENT; return guard(h, [&] { h->impl->getStats(out); }); }
snb_status snb_evaluate_frames(snb_handle h, const snb_frame_batch* b) {
    if (!b) { if (h && h->impl) h->impl->err = "snb_evaluate_frames: null batch"; return SNB_ERR_INVALID_ARGUMENT; }
    return guard(h, [&] { h->impl->evaluateFrames(b); });
}
snb_status snb_evaluate_atom_energies(snb_handle h, int32_t includeDirect, int32_t includeRecip, double* atomEnergies, int32_t outIsDevice) {
    return guard(h, [&] { h->impl->evaluateAtomTable(false, includeDirect, includeRecip, atomEnergies, outIsDevice); });
}
snb_status snb_evaluate_atom_forces(snb_handle h, int32_t includeDirect, int32_t includeRecip, double* atomForces, int32_t outIsDevice) {
    return guard(h, [&] { h->impl->evaluateAtomTable(true, includeDirect, includeRecip, atomForces, outIsDevice); });
}
snb_status snb_evaluate_group_energies(snb_handle h, const snb_group_batch* b) {
    if (!b) { if (h && h->impl) h->impl->err = "snb_evaluate_group_energies: null batch"; return SNB_ERR_INVALID_ARGUMENT; }
    return guard(h, [&] { h->impl->evaluateGroupEnergies(b); });
}
snb_status snb_evaluate_group_forces(snb_handle h, const snb_group_force_batch* b) {
    if (!b) { if (h && h->impl) h->impl->err = "snb_evaluate_group_forces: null batch"; return SNB_ERR_INVALID_ARGUMENT; }
    return guard(h, [&] { h->impl->evaluateGroupForces(b); });
}
snb_status snb_evaluate_group_pair_energies(snb_handle h, const snb_group_pair_batch* b) {
    if (!b) { if (h && h->impl) h->impl->err = "snb_evaluate_group_pair_energies: null batch"; return SNB_ERR_INVALID_ARGUMENT; }
    return guard(h, [&] { h->impl->evaluateGroupPairEnergies(b); });
}
snb_status snb_evaluate_slice_virials(snb_handle h, const snb_virial_batch* b) {
    if (!b) { if (h && h->impl) h->impl->err = "snb_evaluate_slice_virials: null batch"; return SNB_ERR_INVALID_ARGUMENT; }
    return guard(h, [&] { h->impl->evaluateSliceVirials(b); });
}
snb_status snb_get_frame_stats(snb_handle h, snb_frame_stats* out) { if (!out) return SNB_ERR_INVALID_ARGUMENT; return guard(h, [&] { h->impl->getFrameStats(out); }); }

snb_status snb_test_fft3d(int32_t precision, int32_t device, int32_t batch, int32_t nx, int32_t ny, int32_t nz, const double* in, double* spectrum, double* roundtrip) {
    if (!in || !spectrum || !roundtrip || batch < 1) return SNB_ERR_INVALID_ARGUMENT;
    if (legalGridSize(nx) != nx || legalGridSize(ny) != ny || legalGridSize(nz) != nz) return SNB_ERR_UNSUPPORTED;
    try {
        if (precision == SNB_DOUBLE) testFFT<double>(device, batch, nx, ny, nz, in, spectrum, roundtrip);
        else testFFT<float>(device, batch, nx, ny, nz, in, spectrum, roundtrip);
        return SNB_OK;
    } catch (HipError& e) { g_createError = e.msg; return SNB_ERR_HIP; }
}

}  // extern "C"
