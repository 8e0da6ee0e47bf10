// switches.h -- every SNB_* environment variable of the engine (host only; DESIGN.md section 4.5 is written from this table and
// tests/test_switches.py keeps the two in step).  The table is filled once per process, at the first snb_create and before that engine
// touches the GPU: no environment read and no first-use initialisation falls into a timed step or a stream capture, and every engine of
// the process sees the same values.  A `flag` is set by the variable's presence alone (SNB_NO_FUSED_Z=0 still sets it); the other
// variables go through atoi / atoll / atof, with the clamp written on their line.  Defaults are the measured best on c3.
#pragma once
#include <algorithm>
#include <cstdlib>

namespace snb {

struct Switches {
    static bool flag(const char* name) { return getenv(name) != nullptr; }
    static int intOr(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
    static long long longOr(const char* name, long long unset) { const char* e = getenv(name); return e ? atoll(e) : unset; }
    static double realOr(const char* name, double unset) { const char* e = getenv(name); return e ? atof(e) : unset; }

    // ---- spreaders
    bool noOwnSpread = flag("SNB_NO_OWN_SPREAD");      // test switch: the scanning brick spreader
    int ownSlabs = intOr("SNB_OWN_SLABS", 0);      // test switch: this many z slabs per brick of the own-atoms spreader (0: the planner's choice)
    int spreadMargin = flag("SNB_SPREAD_MARGIN") ? std::max(0, intOr("SNB_SPREAD_MARGIN", 0)) : -1;      // test switch (0: every border crossing becomes a stray; -1 = unset: from the list padding)
    bool noFusedZ = flag("SNB_NO_FUSED_Z");      // test switch: the forward z FFT as a kernel of its own behind the spreader
    bool noFixedSpread = flag("SNB_NO_FIXED_SPREAD");      // test switch: f64 LDS accumulation in single precision too
    int zSlabs = intOr("SNB_ZSLABS", 0);      // z slabs of the brick spreader when >= 1 and a divisor of nz; measured on c3: f64 accumulation 1 slab 110 us, 2 slabs 105 us, 4 slabs 145 us; fixed-point 1 slab 61 us, 2 slabs 67 us
    int brickGroup = intOr("SNB_BRICK_GROUP", 1);      // minimum sort columns per brick side (up to 4; 2 on c3 falls back to the atomic spreader, 1.84 ms)
    int mergeNt = intOr("SNB_MERGE_NT", 0);      // test switch: 256 / 512 threads per brick of the merge kernel (0: by brick size)
    double fixHeadroom = realOr("SNB_FIX_HEADROOM", 0.0);      // test switch: a fixed headroom of the 32-bit fixed point (16 = the rule before the mesh-dependent one; <= 0: that rule)
    // ---- FFT
    bool fftTwoPass = intOr("SNB_FFT_TWOPASS", 1) != 0;      // 0: staged Stockham transforms instead of the two-pass register FFT (measured on c3: inverse z 18.2 vs 23.5 us, y 30.6 vs 32.4, fused x/convolution 68.6 vs 71.0)
    int fftyNb = intOr("SNB_FFTY_NB", 0);      // lines per work-group of the y pass (0: chosen from the mesh); measured on c3: 8: 40 us, 16: 31, 21: 28.4, 32: 27.8
    int fftThreads = intOr("SNB_FFT_THREADS", 512) == 256 ? 256 : 512;      // threads per work-group of the y pass: 256, anything else 512 (24.4 -> 22.4 us per pass on c3)
    int convLdsKB = intOr("SNB_CONV_LDS_KB", 72);      // LDS budget of the fused x / convolution kernel; measured on c3 (4 subsets): NB = 4: 68 us, 5: 64, 7: 69, 8: 48.5, 16: 60.5
    bool planeDynamic = flag("SNB_PLANE_DYNAMIC");      // measurement aid: the run-time-split kernel on square planes too
    bool noRectPlanes = flag("SNB_NO_RECT_PLANES");      // test switch: rectangular planes on the three-pass pipeline, as before round 4
    bool convxStagedF64 = flag("SNB_CONVX_STAGED_F64");      // double precision: the staged form of the fused x kernel for 15- / 16-point transforms (c5 180^3: 351 vs 488 us before round 4)
    bool mix16 = flag("SNB_MIX_16X16");      // test switch: the 16 x 16 x 4 matrix-core form of the mix also for <= 4 subsets (x kernel 44.0 -> 51.2 us on derivative steps)
    // ---- plane path
    bool noPlaneFft = flag("SNB_NO_PLANE_FFT");      // test switch: the three-kernel y / x / y pipeline
    int planeNt = intOr("SNB_PLANE_NT", 1024);      // threads per plane: 1024 or 768
    int zmixNby = intOr("SNB_ZMIX_NBY", 0);      // y lines per work-group of the inverse z kernel: 2, 4 or 8, anything else 8 (c4, 8 subsets: plane + z kernel 45.5 + 55.0 us with 8, 61.2 + 42.4 with 4)
    int zmixNt = intOr("SNB_ZMIX_NT", 0);      // threads of the inverse z + mix kernel: 512, any other non-zero value 256 (0: 512 from 24 transforms per work-group)
    // ---- interpolation
    bool noInterpBricks = flag("SNB_NO_INTERP_BRICKS");      // testing aid: force the 32-lanes-per-atom kernel
    int interpGroup = intOr("SNB_INTERP_GROUP", -1);      // widening steps of the interpolation bricks: 0 none, 1: 2 x 1 columns, 2: 2 x 2 (-1: by brick count and LDS fit; measured on c3: 512 threads on single columns 29.1 us, 1024 on 2 x 1 35.2)
    int interpThreads = intOr("SNB_INTERP_THREADS", 0);      // 512, any other non-zero value 1024 threads per brick (0: 512 when there are more bricks than CUs and the brick fits LDS twice)
    int interpZSlabs = intOr("SNB_INTERP_ZSLABS", 0);      // z slabs per interpolation brick; measured on c3: 1 slab 52 us, 2 slabs 70, 4 slabs 72
    // ---- pair kernel
    bool ewaldErfc = flag("SNB_EWALD_ERFC");      // test switch: erfc / exp in the Ewald pair term instead of the polynomials
    bool ewaldPolyAlways = flag("SNB_EWALD_POLY_ALWAYS");      // test control: the polynomials whatever their residuals, as before the guard of ewald_fit.h (SNB_EWALD_ERFC wins)
    bool scalarEnergyKernel = flag("SNB_SCALAR_ENERGY_KERNEL");      // test switch: energy steps of single precision on the scalar tile kernel
    bool noFusedLists = flag("SNB_NO_FUSED_LISTS");      // test switch: the O(N) pair lists as a launch of their own
    int directWgs = intOr("SNB_DIRECT_WGS", 0);      // cap on the tile kernel's work-groups (0: one per four work items)
    int itemTiles = std::max(1, std::min(32, intOr("SNB_ITEM_TILES", 8)));      // tiles per work item, 1..32
    // ---- submission
    bool noStepGraph = flag("SNB_NO_STEP_GRAPH");      // measurement aid: every step as plain launches
    bool noSortGraph = flag("SNB_NO_SORT_GRAPH");      // test switch: phase A of the rebuild as plain launches instead of a replayed graph (0.98 vs 0.68 ms per rebuild on c3)
    bool noFusedFinish = flag("SNB_NO_FUSED_FINISH");      // test switch: k_finishForces as a kernel of its own
    bool noFusedEnergyFinish = flag("SNB_NO_FUSED_ENERGY_FINISH");      // test switch: k_finishSliceEnergies as a kernel of its own
    bool ctxAtomicAdd = flag("SNB_CTX_ATOMIC_ADD");      // measurement aid: a bound context's force buffer (snb_bind_context) is added to with 64-bit atomics instead of plain read-modify-write
    bool concurrentPme = intOr("SNB_CONCURRENT_PME", 0) != 0;      // forces-only graph steps fork the PME chain; measured on c3: serial 0.80 ms/step, forked 0.87 (default priority) / 1.32 (high or low priority)
    bool noKernelStamps = flag("SNB_NO_KERNEL_STAMPS");      // measurement aid: only the pair-kernel / pipeline timers
    bool noPinnedRing = flag("SNB_NO_PINNED_RING");      // test switch: the copy straight from the caller's array (synchronised)
    int overlap = intOr("SNB_OVERLAP", 1);      // 0: replayed steps stay serial (round 4: c3 0.414 -> 0.377 ms per step with derivatives)
    long long overlapMinTiles = longOr("SNB_OVERLAP_MIN_TILES", 100000);      // below this the pair kernel is shorter than the PME chain and the fork only costs (c2, 65k tiles: +2 %)
    int overlapCuLimit = intOr("SNB_OVERLAP_CU_LIMIT", 2);      // work-groups per CU of the first, resident launch of the tile kernel
    int overlapGridA = intOr("SNB_OVERLAP_GRID_A", 0);      // work-groups of the first launch (0: six per CU)
    int overlapGridB = intOr("SNB_OVERLAP_GRID_B", 0);      // work-groups of the second launch (0: four per CU)
    bool overlapByCount = flag("SNB_OVERLAP_BY_COUNT");      // test switch: resident work-groups chosen by order of arrival, not by register position
    bool overlapDebug = flag("SNB_OVERLAP_DEBUG");      // diagnostics: the residency table of the first three overlapped steps
    bool stepTrace = flag("SNB_STEP_TRACE");      // diagnostics: device-clock stamps of the last replayed step, printed when the engine goes
    bool noGraphUpdate = flag("SNB_NO_GRAPH_UPDATE");      // test switch: a new instantiation after every rebuild, as before round 4
    bool eagerRebuildStep = flag("SNB_EAGER_REBUILD_STEP");      // test switch: the rebuild step as plain launches (rounds 1-3)
    bool pmePrioLow = flag("SNB_PME_PRIO_LOW");      // the PME stream at the lowest priority (wins over _HIGH; default: the middle of the range)
    bool pmePrioHigh = flag("SNB_PME_PRIO_HIGH");      // the PME stream at the highest priority
    // ---- builder
    bool hostTriclinic = flag("SNB_HOST_TRICLINIC");      // testing aid: old behaviour, triclinic and non-periodic boxes on the host builder
    bool boxPrune = flag("SNB_BOX_PRUNE");      // test switch: tiles pruned by bounding boxes only
    bool nbBoxWalk = flag("SNB_NB_BOX_WALK");      // test switch: the round-2 candidate walk
    bool nbSyncPadded = flag("SNB_NB_SYNC_PADDED");      // test switch: wait for the padded count, as before round 4 (saves ~75 us per rebuild when off)
    int nbPredictShort = intOr("SNB_NB_PREDICT_SHORT", 0);      // test switch: predict this many blocks too FEW (exercises the repeat path)
    bool nbNoSpin = flag("SNB_NB_NO_SPIN");      // test switch: the build's totals by a synchronised copy (wakes up 30-45 us late)
    int nbPublishWaitMs = std::max(0, intOr("SNB_NB_PUBLISH_WAIT_MS", 2000));      // test switch: how long the host spins for published totals before it copies (0: always the copy)
    bool sideRebuild = intOr("SNB_SIDE_REBUILD", 1) != 0;      // 0: every rebuild in line, none beside the steps
    int sideLead = std::max(1, intOr("SNB_SIDE_LEAD", 3));      // executes before a rebuild falls due at which its side build starts, >= 1
    bool sideReject = flag("SNB_SIDE_REJECT");      // test switch: every side build is discarded and the rebuild repeated in line
    bool sidePrioHigh = flag("SNB_SIDE_PRIO_HIGH");      // the side-build stream at the highest priority: its kernels push the tile kernel aside (wins over _LOW; default: the middle)
    bool sidePrioLow = flag("SNB_SIDE_PRIO_LOW");      // the side-build stream at the lowest priority: the build crawls and the steps end up waiting for it
    bool framesInLine = flag("SNB_FRAMES_IN_LINE");      // measurement aid: snb_evaluate_frames builds the list of every frame in line, none beside the previous frame's step
    // ---- diagnostics
    bool nbTrace = flag("SNB_NB_TRACE");      // per-block trace array of the tile builder
    bool pmeTrace = flag("SNB_PME_TRACE");      // trace words of the PME kernels
    bool verbose = flag("SNB_VERBOSE");      // "[snb] ..." lines on stderr: rebuilds, side builds, graph captures and updates
    bool debugWork = flag("SNB_DEBUG_WORK");      // consistency of the work list after every build: the items must cover every tile exactly once
};

inline const Switches& switches() { static const Switches s; return s; }

}  // namespace snb
