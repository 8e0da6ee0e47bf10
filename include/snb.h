/*
 * snb.h -- C ABI of the MI355X-native SlicedNonbondedForce engine (libsnb_hip.so).
 *
 * This is the drop-in boundary.  It replaces, for the force/energy hot path, what the reference puts
 * behind  NonbondedSlicing::CalcSlicedNonbondedForceKernel
 *   (openmmapi/include/NonbondedSlicingKernels.h:27-85):
 *     initialize(system, force)                      :48   -> snb_create + snb_set_particles/_exceptions/_lambdas/...
 *     execute(context, forces, energy, direct, recip):59   -> snb_set_box/_positions + snb_execute + snb_get_forces,
 *                                                             or, with the context's own buffers bound (snb_bind_context): snb_set_box + snb_execute
 *     copyParametersToContext(context, force)        :66   -> snb_set_particles/_exceptions/_dispersion_coefficients
 *     getPMEParameters(alpha,nx,ny,nz)               :75   -> snb_get_pme_parameters
 *     getLJPMEParameters(alpha,nx,ny,nz)             :84   -> snb_get_ljpme_parameters
 * and the device work the reference enqueues from CommonCalcSlicedNonbondedForceKernel::execute
 *   (platforms/common/src/CommonNonbondedSlicingKernels.cpp:846-1402).
 *
 * Plain pointers and sizes only: no C++ types, no torch types.  Caller owns every host array;
 * the engine owns all device memory.  One handle = one device = one HIP stream as far as the caller can see: all work is ordered on
 * snb_config.stream (replayed steps fork a part of it onto an internal second stream and join it before they end); a handle is not
 * thread-safe.  Errors are status codes; snb_last_error() gives the message an adapter rethrows as
 * OpenMM::OpenMMException (INTEGRATION.md shows the adapter).
 */
#ifndef SNB_H_
#define SNB_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNB_ABI_VERSION 8

typedef struct snb_engine* snb_handle;

typedef enum {
    SNB_OK = 0,
    SNB_ERR_INVALID_ARGUMENT = 1,
    SNB_ERR_HIP = 2,              /* a HIP runtime call failed (no GPU, out of memory, ...)          */
    SNB_ERR_BOX_TOO_SMALL = 3,    /* "The periodic box size has decreased to less than twice the nonbonded cutoff."
                                     (ReferenceNonbondedSlicingKernels.cpp:202-204)                     */
    SNB_ERR_NOT_PME = 4,          /* getPMEParametersInContext on a non-PME engine (CommonNonbondedSlicingKernels.cpp:1571-1581) */
    SNB_ERR_STATE = 5,            /* call order violated (e.g. execute before positions were set)     */
    SNB_ERR_UNSUPPORTED = 6
} snb_status;

/* Values of CalcSlicedNonbondedForceKernel::NonbondedMethod (NonbondedSlicingKernels.h:29-36). */
typedef enum {
    SNB_NoCutoff = 0, SNB_CutoffNonPeriodic = 1, SNB_CutoffPeriodic = 2, SNB_Ewald = 3, SNB_PME = 4, SNB_LJPME = 5
} snb_method;

/* The precision modes of the reference's GPU platforms (CudaPlatform "Precision" property: single / mixed / double).
 * SNB_MIXED: single-precision pair and mesh arithmetic as SNB_SINGLE, but the direct-space forces are accumulated in 64-bit fixed
 * point (2^32 per kJ/mol/nm) the way the reference's GPU platforms accumulate every force (platforms/common/src/kernels/pme.cc:381-389,
 * realToFixedPoint; CommonNonbondedSlicingKernels.cpp getLongForceBuffer): integer sums are independent of the order in which waves
 * finish, so with the charge mesh already spread in fixed point the force of a step is reproducible bit for bit; the accumulators and
 * the reciprocal part are summed in double on delivery.  Range: |force component| < 2^31 kJ/mol/nm (saturating), as in the reference. */
typedef enum { SNB_SINGLE = 0, SNB_DOUBLE = 1, SNB_MIXED = 2 } snb_precision;

typedef struct {
    int32_t abi_version;        /* SNB_ABI_VERSION                                                      */
    int32_t n_atoms;
    int32_t n_subsets;          /* >= 1.  snb_create returns SNB_ERR_UNSUPPORTED (snb_last_error names the numbers) for counts whose kernels cannot
                                 * get their LDS: more than 77 subsets with any method (the pair-list energy kernels reduce n(n+1)/2 slices in 16 bytes
                                 * each, at most 48 KB), and with PME / LJPME when one x line of a mesh for every subset this engine holds
                                 * (n_subsets, or its share when sharded) exceeds the device's LDS: 2 nx n sizeof(complex) + nx sizeof(real) +
                                 * nx sizeof(complex) bytes, complex = 2 reals of 4 (single, mixed) or 8 (double) bytes -- on 160 KB in double
                                 * precision that is 42 subsets on a 120 mesh, 28 on a 180 mesh.  Tested up to 20 subsets. */
    int32_t method;             /* snb_method                                                           */
    int32_t precision;          /* snb_precision: arithmetic type of every kernel                       */
    int32_t use_switch;         /* LJ switching function (ignored for NoCutoff and LJPME, Quirk Q2)     */
    int32_t exceptions_periodic;
    int32_t device;             /* HIP device ordinal                                                   */
    double  cutoff;
    double  switch_distance;
    double  rf_dielectric;
    double  alpha;              /* Ewald/PME separation parameter (explicit; > 0 for Ewald/PME/LJPME)   */
    int32_t grid[3];            /* requested PME mesh; rounded up to the next size the FFT supports     */
    int32_t kmax[3];            /* Ewald: numRx, numRy, numRz (ReferenceSlicedLJCoulombIxn.cpp:115-121) */
    double  alpha_d;            /* LJPME dispersion separation parameter                                */
    int32_t dgrid[3];           /* LJPME dispersion mesh                                                */
    double  neighbor_padding;   /* nm added to the cutoff when building tiles (0 = rebuild every call)  */
    int32_t rebuild_interval;   /* rebuild tiles every this many executes (0, 1: every execute); < 0: automatic -- when an atom has
                                 * moved 0.8 * neighbor_padding / 2 since the last rebuild, and after -rebuild_interval executes at the latest.
                                 * (With a fixed interval > 4 the next list is built three executes ahead on an internal stream, from a
                                 * copy of the positions, and comes into use when the rebuild falls due: it is then three executes
                                 * older than one built in line.) */
    int32_t shard_rank;         /* multi-GPU: this engine owns PME subsets J with J % shard_count == shard_rank */
    int32_t shard_count;        /*            and direct-space work items w with w % shard_count == shard_rank; 1 = unsharded */
    int32_t disable_graph;      /* 1 = enqueue every step eagerly (default 0: forces-only steps replay a captured hipGraph)  */
    int32_t host_neighbor_build; /* 1 = always build the tile lists on the host (default 0: on the GPU when the box allows it)            */
    void*   stream;             /* hipStream_t to enqueue on, or NULL for an engine-owned stream        */
} snb_config;

/* Aggregate counters for measurement (bench.py / DESIGN.md byte model). */
typedef struct {
    int64_t n_tiles;            /* 32x32 tiles processed per evaluation by this engine (T)             */
    int64_t n_blocks;           /* 32-atom blocks (padded atoms / 32)                                   */
    int64_t n_padded_atoms;
    int64_t n_exclusion_tiles;  /* tiles that carry an exclusion mask                                   */
    int64_t n_exclusions;       /* excluded pairs (exceptions)                                          */
    int64_t n_14;               /* exceptions with non-zero parameters (Q6)                             */
    int64_t n_rebuilds;
    int32_t grid[3];            /* PME mesh actually used                                               */
    int32_t dgrid[3];
    double  last_direct_ms;     /* HIP-event time of the last direct-space pair kernel launch           */
    double  last_recip_ms;      /* HIP-event time of the last reciprocal pipeline (all its kernels)     */
    double  last_total_ms;      /* HIP-event time of the last snb_execute (all kernels)                 */
    double  last_rebuild_ms;    /* wall time of the last neighbour rebuild                              */
    double  sum_direct_ms;      /* cumulative HIP-event times since snb_reset_timers (harvested lazily,   */
    double  sum_recip_ms;       /*   no per-step host synchronisation)                                  */
    double  sum_total_ms;
    int64_t n_timed;            /* executes included in the sums                                        */
    int64_t n_host_rebuilds;    /* rebuilds that fell back to the host builder (triclinic / non-periodic / tiny boxes) */
    int64_t n_list_overruns;    /* list lifetimes in which an atom moved more than neighbor_padding / 2 (pairs may have been missed:
                                 * shorten rebuild_interval, widen the padding, or use the automatic mode)                */
    /* (ABI 6) per-kernel begin/end stamps of the timed (eager) steps, cumulative since snb_reset_timers.  Slots (SNB_K_*): 0 position
     * gather, 1 charge spreading (+ fused forward z FFT), 2 forward z FFT when separate, 3 forward y FFT, 4 x FFT + slice energies +
     * lambda mix + inverse x FFT, 5 inverse y FFT, 6 inverse z FFT, 7 force interpolation (+ user-order force write); 8..15 the same
     * for the LJPME dispersion mesh (8 unused). */
    double  sum_kernel_ms[16];
    int64_t n_kernel_timed[16];
    int64_t n_spread_strays;    /* atoms of the LAST execute whose spreading footprint had left their work-group's LDS region (drift beyond the
                                 * margin since the last re-sort): handled one by one, exactly, by the merge kernel -- normally 0 */
    /* (ABI 8) the polynomials the pair kernels of this engine use for the direct-space Ewald terms: bit 0 the Coulomb force factor, bit 1
     * the Coulomb pair energy (single and mixed precision), bit 2 the LJPME dispersion force factor (double precision).  A polynomial
     * whose residual at this engine's alpha, cutoff and neighbor_padding is too large is replaced by the erfc / exp form. */
    int64_t ewald_poly_mask;
} snb_stats;
#define SNB_POLY_MASK_FORCE 1
#define SNB_POLY_MASK_ENERGY 2
#define SNB_POLY_MASK_DISPERSION 4
#define SNB_K_GATHER 0
#define SNB_K_SPREAD 1
#define SNB_K_FFT_Z_FWD 2
#define SNB_K_FFT_Y_FWD 3
#define SNB_K_CONVOLVE_X 4
#define SNB_K_FFT_Y_INV 5
#define SNB_K_FFT_Z_INV 6
#define SNB_K_INTERPOLATE 7
#define SNB_K_DISPERSION_MESH 8

/* -- lifetime ---------------------------------------------------------------------------------- */
snb_status snb_create(const snb_config* cfg, snb_handle* out);
void       snb_destroy(snb_handle h);
const char* snb_last_error(snb_handle h);        /* h may be NULL: error of the last failed snb_create */

/* -- parameters (host arrays; effective values, i.e. after parameter offsets) ------------------ */
/* charge[N], sigma[N], epsilon[N] as NonbondedForce::getParticleParameters; subset[N] in [0,n_subsets). */
snb_status snb_set_particles(snb_handle h, const double* charge, const double* sigma, const double* epsilon, const int32_t* subset);
/* All exceptions: pairs[m][2], chargeProd[m], sigma[m], epsilon[m].  Every exception is an exclusion; those with
 * chargeProd != 0 or epsilon != 0 or force14[k] != 0 are also 1-4 interactions (Quirk Q6,
 * ReferenceNonbondedSlicingKernels.cpp:99-112).  force14 may be NULL. */
snb_status snb_set_exceptions(snb_handle h, int32_t m, const int32_t* pairs, const double* charge_prod, const double* sigma,
                              const double* epsilon, const int32_t* force14);
/* Parameter offsets (SlicedNonbondedForce::addParticleParameterOffset / addExceptionParameterOffset), applied ON THE DEVICE as the
 * reference does (platforms/common/src/kernels/nonbondedParameters.cc:4-179): snb_set_particles / snb_set_exceptions give the BASE
 * values and   effective = base + sum_k global[k] * delta_k .   particle_delta[n][3] = (charge, sigma, epsilon) per unit of the global
 * parameter particle_global[n]; exception_delta[n][3] = (chargeProd, sigma, epsilon); an exception that carries an offset counts as
 * a 1-4 interaction whatever its base values (Q6).  Call after snb_set_exceptions; globals start at 0. */
snb_status snb_set_parameter_offsets(snb_handle h, int32_t n_globals,
                                     int32_t n_particle_offsets, const int32_t* particle, const int32_t* particle_global, const double* particle_delta,
                                     int32_t n_exception_offsets, const int32_t* exception, const int32_t* exception_global, const double* exception_delta);
/* New values of the global parameters the offsets refer to (Context::setParameter): the next snb_execute recomputes the effective
 * parameters with two small kernels -- no re-sort, no tile rebuild, no graph re-capture, no host synchronisation. */
snb_status snb_set_global_parameters(snb_handle h, int32_t n_globals, const double* values);
/* mask[S]: the slices whose raw energies a DERIVATIVE-ONLY step (snb_execute with include_energy == 2) must produce -- the slices bound
 * to a global parameter whose derivative was requested.  The reference adds dE/dlambda on every execute
 * (CommonNonbondedSlicingKernels.cpp:712-718) but needs the energy of those slices only; here the pair kernel runs its forces-only
 * arithmetic on the tiles of every other slice (on the 300k-atom box 95 % of the tiles are solvent-solvent), the reciprocal kernel
 * skips their Gram sums.  Default: every slice.  The energies of slices outside the mask are unspecified after such a step. */
snb_status snb_set_energy_slices(snb_handle h, const int32_t* mask);
/* lambdas[S][2] = (Coulomb, vdW) per slice, S = n(n+1)/2, slice(i,j) = max(max+1)/2+min (SlicedNonbondedForce.h:22). */
snb_status snb_set_lambdas(snb_handle h, const double* lambdas);
/* Per-slice dispersion-correction coefficients (SlicedNonbondedForceImpl.cpp:263-354); NULL = none. */
snb_status snb_set_dispersion_coefficients(snb_handle h, const double* coef);
/* Host helper (no GPU work): the coefficients themselves, restating calcDispersionCorrections. out[S]. */
snb_status snb_compute_dispersion_coefficients(int32_t n_atoms, int32_t n_subsets, const double* sigma, const double* epsilon,
                                               const int32_t* subset, double cutoff, int32_t use_switch, double switch_distance,
                                               double* out);

/* -- per-step state ---------------------------------------------------------------------------- */
snb_status snb_set_box(snb_handle h, const double* box9);   /* rows a, b, c (reduced, lower triangular) */
/* pos: [N][3] (is_double=1: double, else float) or, when stride4 != 0, [N][4] (OpenMM posq layout).  is_device != 0:
 * a device pointer valid on the engine's device. */
snb_status snb_set_positions(snb_handle h, const void* pos, int32_t is_device, int32_t is_double, int32_t stride4);
snb_status snb_rebuild_neighbors(snb_handle h);             /* force a tile rebuild at the next execute */

/* -- the hot path ------------------------------------------------------------------------------ */
/* Enqueues one evaluation; forces stay on the device until snb_get_forces.  include_energy != 0: the raw per-slice energies are
 * accumulated as well (the step of every force with energy-parameter derivatives: the reference adds dE/dlambda on every execute,
 * CommonNonbondedSlicingKernels.cpp:712-718) and summed ON THE DEVICE as the step's last kernel.  With energy == NULL nothing is read
 * back and nothing synchronises -- such a step replays a captured graph like a forces-only one; snb_get_slice_energies fetches the
 * sums when the caller needs them.  With energy != NULL it receives sum_slices lambda*E (this synchronises the stream).
 * include_energy == 2: a derivative-only step -- as 1, restricted to the slices of snb_set_energy_slices (energy must be NULL).
 * include_forces == 0 with include_energy 1 or 2: an ENERGY-ONLY step (OpenMM getState(getEnergy=True) without forces, a barostat trial,
 * re-evaluating a stored frame for MBAR: E(lambda) = sum_s lambda_s E_s).  Mode 1 produces the total and every raw slice energy, mode 2 the
 * slices of snb_set_energy_slices (energy must be NULL).  It evaluates no forces: snb_get_forces still returns the forces of the last forces
 * step (when the step rebuilds the lists -- which re-sorts the atoms -- the engine first keeps a copy of those forces and serves it until the
 * next forces step), and the buffer of snb_set_force_output is not touched, whatever its accumulate flag.  It follows the neighbour-list
 * rules of any execute (box-change and displacement rebuilds, the fixed-interval count, side builds) and runs as plain launches: it never
 * captures or updates a step graph itself, while a rebuild it performs marks the graphs stale as any rebuild does (the next forces step
 * refreshes its graph).  include_forces == 0 with include_energy == 0: nothing is enqueued (SNB_OK). */
snb_status snb_execute(snb_handle h, int32_t include_forces, int32_t include_energy, int32_t include_direct,
                       int32_t include_reciprocal, double* energy);
/* out: [N][3] in the type selected by is_double; accumulate != 0 adds to what is there (the reference
 * accumulates into the platform's force buffer). */
snb_status snb_get_forces(snb_handle h, void* out, int32_t is_device, int32_t is_double, int32_t accumulate);
/* Optional: name the device buffer ([N][3], type by is_double) that every following snb_execute writes (accumulate == 0) or adds
 * (accumulate != 0) the forces to as the last kernel of the step -- it then belongs to the replayed step graph and a later
 * snb_get_forces on the same pointer is a no-op.  out == NULL switches this off.  (The reference's execute() adds into the
 * platform's force buffer itself, NonbondedSlicingKernels.h:59; this is that behaviour without an extra launch per step.) */
snb_status snb_set_force_output(snb_handle h, void* out, int32_t is_double, int32_t accumulate);
/* Optional, sharded engines: direct-space ownership of the 32-atom i-blocks.  The engine evaluates the tiles of block I when
 * I % period lies in [begin, end); the default is (shard_rank, shard_rank + 1, shard_count).  The ranges of all ranks must partition
 * [0, period).  Lets the host shift direct-space work away from ranks that carry PME grids (the role of the load balancing between
 * devices in OpenMM's parallel kernels, which the reference inherits from its platform); takes effect with a neighbour rebuild at
 * the next snb_execute.  An empty range (begin == end) is allowed. */
snb_status snb_set_shard_blocks(snb_handle h, int32_t begin, int32_t end, int32_t period);
/* Raw (unscaled) energies of the last execute with include_energy: out[S][2] = (Coulomb, vdW). */
snb_status snb_get_slice_energies(snb_handle h, double* out);
/* Device address of those energies: double[S][2], complete (pair sums, reciprocal sums, self, background and dispersion-correction
 * terms) once the last kernel of an energy step has run on the engine's stream.  For a caller that accumulates dE/dlambda on the
 * device itself (OpenMM's energy-parameter-derivative buffer): no read-back, no synchronisation.  The address is fixed for the
 * engine's lifetime. */
snb_status snb_slice_energies_device(snb_handle h, const double** out);
snb_status snb_synchronize(snb_handle h);

/* -- context binding (ABI 7) ------------------------------------------------------------------- */
/* The buffers of a GPU platform's context, named once: positions in the context's own (reordered) atom order, the 64-bit fixed-point
 * force buffer every kernel of the platform adds into, the energy and energy-parameter-derivative accumulators (the reference reads
 * cc.getPosq() and adds into cc.getLongForceBuffer(), platforms/common/src/kernels/pme.cc:381-389).  While a binding is in place a step is
 * snb_set_box + snb_execute: the step's first kernel reads posq through the permutation, its last kernel adds the forces, the energy
 * and the derivatives into the bound buffers -- no staging buffer, no kernel outside the replayed step graph, no host synchronisation.
 * The pointers are fixed for the binding's life (they belong to the step graph's key); the contents change every step.  Other writers
 * of the buffers must be ordered on snb_config.stream. */
typedef struct {
    const void*    posq;            /* device, [>= n_atoms][4], float or double by is_double, CONTEXT order; .w is ignored; never written */
    const int32_t* atom_index;      /* device, [n_atoms]: atom_index[slot] = user index; a permutation of 0 .. n_atoms-1               */
    int32_t        is_double;
    int32_t        padded_n;        /* >= n_atoms: component stride of force_buffer                                                    */
    int64_t*       force_buffer;    /* device, [3][padded_n], 2^32 per kJ/mol/nm, context order; ADDED to; NULL = no delivery.  A forces step
                                     * adds (int64)(F * 2^32) (truncated, saturating) of the step's total force on the atom in slot s to
                                     * force_buffer[d * padded_n + s], once per entry, in its last kernel; entries s >= n_atoms are never touched */
    void*          energy_buffer;   /* device scalar (type by energy_is_double) or NULL: a step with include_energy == 1 and energy == NULL
                                     * adds sum_s lambda_s E_s (summed in double, then converted)                                      */
    void*          deriv_buffer;    /* device array (same type) or NULL: steps with include_energy 1 or 2 add the raw E[slice][term] to
                                     * deriv_buffer[deriv_slot[slice][term]] (mode 2: for the slices of snb_set_energy_slices)         */
    const int32_t* deriv_slot;      /* HOST, [n_slices][2]: slot in deriv_buffer of (slice, term), -1 = none; several entries may share a
                                     * slot (their energies sum); copied at bind; NULL = no derivative delivery                        */
    int32_t        energy_is_double;
} snb_context_binding;
/* Binds (b != NULL) or unbinds (b == NULL).  Checks padded_n >= n_atoms, posq and atom_index non-NULL, and that atom_index is a
 * permutation (a device scan, read back: this call synchronises).  While bound the coordinates come from posq on every execute and
 * snb_set_positions returns SNB_ERR_STATE; after an unbind the positions must be set again.  A bound force buffer takes the place of
 * snb_set_force_output (setting one clears the other); snb_get_forces keeps working.  Sharded engines: SNB_ERR_UNSUPPORTED. */
snb_status snb_bind_context(snb_handle h, const snb_context_binding* b);
/* The caller has rewritten atom_index (and moved the contents of posq / force_buffer accordingly): call this before the next
 * snb_execute.  The engine refreshes its user -> context map with one small kernel on its stream: no neighbour rebuild, no re-sort, no
 * graph capture or update, no synchronisation; safe while a list is being built beside the steps (the build works from a user-order
 * snapshot of the positions). */
snb_status snb_context_order_changed(snb_handle h);

/* -- frame batches ----------------------------------------------------------------------------- */
/* The slice energies of F stored frames in one call: the loop of MBAR / reweighting over a trajectory (E(lambda) = sum_s lambda_s E_s, so one
 * evaluation of a frame gives its energy at every lambda state).  Row f of slice_energies is what snb_set_box (boxes[f]), snb_set_positions
 * (frame f), an energy-only snb_execute (include_forces = 0, include_energy = mode, energy = NULL) and snb_get_slice_energies give, to the
 * accuracy of the precision mode (the list built for a frame orders the sums differently) -- without a host synchronisation per frame: while
 * the energy-only step of frame f runs, the list of frame f + 1 is built beside it on an internal stream, straight from that frame's
 * positions; host frames are uploaded through pinned staging buffers on a copy stream ahead of their build.  A frame is built in line instead
 * when its box differs from its predecessor's, when it is the first of the batch, during the first two rebuilds of an engine, after a
 * discarded side build, and wherever lists are built on the host (NoCutoff, fewer than 64 atoms, tiny cells) or the system is not periodic.
 * Host output (out_is_device == 0): returns with the results written, after exactly one synchronisation, at the end.  Device output: returns
 * once the last frame is enqueued; the results are complete in stream order on snb_config.stream.
 * Everything is checked before anything is enqueued: a failed call leaves no work behind and no state changed.  n_frames == 0: SNB_OK, no
 * work.  Negative count, NULL positions / slice_energies, another mode, states with mode 2: SNB_ERR_INVALID_ARGUMENT.  A box that is not in
 * reduced form: SNB_ERR_INVALID_ARGUMENT; one smaller than twice the cutoff: SNB_ERR_BOX_TOO_SMALL; Ewald with a non-rectangular box:
 * SNB_ERR_UNSUPPORTED -- each with the frame index in snb_last_error.
 * Afterwards the engine is what it was: the caller's positions, the box, the lambdas and the energy-slice mask are in place, snb_get_forces
 * returns the forces of the last forces step, the buffer of snb_set_force_output is untouched, no step graph was captured or updated; the
 * next snb_execute rebuilds its list (the lists in memory belong to the last frame) and refreshes its graph in place, as after any rebuild.
 * The engine's own slice-energy buffer (snb_get_slice_energies, snb_slice_energies_device) holds the last frame.  Frame steps count in
 * snb_stats.n_rebuilds and are never timed steps.
 * Out of scope: while a context is bound (snb_bind_context) the call returns SNB_ERR_STATE -- a binding takes its positions from posq -- and
 * on sharded engines (shard_count > 1) SNB_ERR_UNSUPPORTED -- their energy-only steps run the forces kernels. */
typedef struct {
    int32_t        n_frames;
    const void*    positions;        /* [F][N][3], or [F][N][4] when stride4 != 0; USER atom order; float or double by is_double */
    int32_t        is_device;        /* != 0: device pointer on the engine's device, valid until the engine's stream has passed the batch */
    int32_t        is_double;
    int32_t        stride4;
    const double*  boxes;            /* HOST [F][9], reduced form, or NULL: the engine's current box for every frame */
    int32_t        mode;             /* 1: every slice; 2: the slices of snb_set_energy_slices (other entries unspecified) */
    int32_t        include_direct, include_reciprocal;
    double*        slice_energies;   /* [F][S][2] raw (Coulomb, vdW), complete as after an energy-only snb_execute: pair, reciprocal, self, background, dispersion correction */
    int32_t        out_is_device;
    int32_t        n_states;         /* optional: K lambda states, 0 = none */
    const double*  state_lambdas;    /* HOST [K][S][2] */
    double*        state_energies;   /* [F][K] = sum_s sum_t lambda_k[s][t] E[f][s][t], summed in double on the device; same residence as slice_energies; mode 1 only */
} snb_frame_batch;
snb_status snb_evaluate_frames(snb_handle h, const snb_frame_batch* b);

typedef struct { int64_t n_batches, n_frames, n_built_beside, n_built_in_line, n_side_discarded; double last_batch_ms; } snb_frame_stats;
snb_status snb_get_frame_stats(snb_handle h, snb_frame_stats* out);   /* cumulative; last_batch_ms = host wall time of the last call that ended in a synchronise, else 0 */

/* -- per-atom interaction energies ------------------------------------------------------------- */
/* Where a slice's energy sits: atom_energies[i][J][t] = the raw energy (t = 0 Coulomb, 1 vdW; not scaled by the lambdas, independent of them) of
 * atom i with ALL atoms of subset J, for every atom and every subset in one evaluation -- what one subset (and one PME mesh) per residue
 * would cost a mesh each.  It is the energy the slice (n, J) would have with atom i alone in a new subset n; in its own subset's column the
 * atom's self-interaction (its images, the Ewald self term) counts twice, so that
 *     sum_{i in I} A[i][J] = E[slice(I, J)]  (I != J),        1/2 sum_{i in I} A[i][I] = E[slice(I, I)]
 * with E the raw slice energies of an energy-only step without dispersion-correction coefficients.  Pairs inside the cutoff, the Ewald
 * exclusion corrections and the 1-4 exceptions credit both ends; the reciprocal part is q_i psi_J(r_i) from the unmixed potentials of the
 * subsets' meshes (LJPME: c6_i psi_J of the dispersion mesh into t = 1); the neutralising background is -2 c q_i Q_J.  The long-range
 * dispersion correction is a per-slice constant, coef / V (snb_compute_dispersion_coefficients), and is NOT attributed.  Parameters are the
 * effective ones (base values + offsets at the current global parameters).  USER atom order; host or device by out_is_device.
 * The call behaves as an energy-only step behaves: it takes the current box and positions (with a bound context, posq through the same
 * gather), follows the neighbour-list rules of any execute (a due rebuild happens, a pending side build is finished or cancelled as for an
 * energy-only step), runs as plain launches -- it never captures or updates a step graph -- and counts in no timer sum and not in n_timed.
 * It writes ONLY the table: the forces (snb_get_forces), the buffer of snb_set_force_output, a binding's force_buffer / energy_buffer /
 * deriv_buffer and the engine's slice-energy buffer (snb_get_slice_energies, snb_slice_energies_device) stay bit for bit what they were.
 * Host output returns after one synchronisation; device output is complete in stream order on snb_config.stream.
 * Everything is checked before anything is enqueued: atom_energies NULL or both include flags 0: SNB_ERR_INVALID_ARGUMENT; shard_count > 1:
 * SNB_ERR_UNSUPPORTED; SNB_Ewald with include_reciprocal (the k-sum of classic Ewald is not attributed; direct-only works):
 * SNB_ERR_UNSUPPORTED; particles, box or positions missing: what snb_execute returns in that state.  The working memory (a table over the
 * sorted atoms) is allocated at the first call: an engine that never calls pays nothing. */
snb_status snb_evaluate_atom_energies(snb_handle h, int32_t include_direct, int32_t include_reciprocal,
                                      double* atom_energies /* [n_atoms][n_subsets][2], USER order */, int32_t out_is_device);

/* -- per-atom forces by subset and term -------------------------------------------------------- */
/* The force split by partner subset: atom_forces[i][J][t][d] = G[i][J][t] = - d E_raw[slice(s_i, J)][t] / d r_i, component d, in kJ/mol/nm
 * (t = 0 Coulomb, 1 vdW; s_i the subset of atom i): the force ALL atoms of subset J put on atom i, for every atom and every subset in one
 * evaluation.  It is raw: not scaled by the lambdas and independent of them.  E_raw is linear in the lambdas, so the force on atom i at
 * ANY lambda state is  sum_J sum_t lambda[slice(s_i, J)][t] G[i][J][t]  -- the forces of another state without another evaluation, the
 * lambda-derivative of the forces as the sum of the bound columns, the mean force the solvent puts on a ligand atom as one column.
 * Attributed: pairs inside the cutoff (both ends, diagonal tiles included), the Ewald exclusion corrections (into t = 0; the LJPME
 * dispersion part into t = 1), the 1-4 exceptions (both ends), the reciprocal part from the UNMIXED potentials of the subsets' meshes,
 * -q_i grad psi_J(r_i) into t = 0 (LJPME: -c6_i grad psi_J of the dispersion mesh into t = 1).  The Ewald self term, the neutralising
 * background and the long-range dispersion correction carry no force: nothing is added for them.  Parameters are the effective ones (base
 * values + offsets at the current global parameters).  USER atom order; host or device by out_is_device.
 * The call behaves as an energy-only step behaves: it takes the current box and positions (with a bound context, posq through the same
 * gather), follows the neighbour-list rules of any execute (a due rebuild happens, a pending side build is finished or cancelled as for an
 * energy-only step; the forces of the last forces step are kept across a rebuild it performs), runs as plain launches -- it never captures
 * or updates a step graph -- and counts in no timer sum and not in n_timed.
 * It writes ONLY the table: the forces (snb_get_forces), the buffer of snb_set_force_output, a binding's force_buffer / energy_buffer /
 * deriv_buffer and the engine's slice-energy buffer (snb_get_slice_energies, snb_slice_energies_device) stay bit for bit what they were.
 * Host output returns after one synchronisation; device output is complete in stream order on snb_config.stream.
 * Everything is checked before anything is enqueued: atom_forces NULL or both include flags 0: SNB_ERR_INVALID_ARGUMENT; shard_count > 1:
 * SNB_ERR_UNSUPPORTED; SNB_Ewald with include_reciprocal (the k-sum of classic Ewald is not attributed; direct-only works):
 * SNB_ERR_UNSUPPORTED; particles, box or positions missing: what snb_execute returns in that state.  The working memory (a table over the
 * sorted atoms) is allocated at the first call: an engine that never calls pays nothing.  The table's double sums are accumulated with
 * atomics: equal from call to call up to the rounding of the sums, not bit for bit, in every precision mode. */
snb_status snb_evaluate_atom_forces(snb_handle h, int32_t include_direct, int32_t include_reciprocal,
                                    double* atom_forces /* [n_atoms][n_subsets][2][3], USER order */, int32_t out_is_device);

/* -- per-group interaction energies over stored frames ----------------------------------------- */
/* The product of the two calls above: the atom-energy table summed over lists of atoms (residues, a ligand, first-shell waters), for every
 * frame of a stored trajectory, reduced on the device --
 *     group_energies[f][g][J][t] = sum_{i in atoms(g)} A_f[i][J][t]
 * with A_f the table of snb_evaluate_atom_energies at frame f: the same attribution, raw (lambda-independent) values, effective parameters,
 * and the long-range dispersion correction left out.  Groups are lists (CSR: group_start[G + 1], group_atoms, USER indices): they may
 * overlap, leave atoms out, be empty (a row of zeros), and an index listed twice counts twice.  Every entry of the output is written.  The
 * sums use no atomics: a row is a function of the frame's table alone (the table itself is accumulated with double atomics).
 * With frames given the call follows the contract of snb_evaluate_frames: everything is checked before anything is enqueued; the list of
 * frame f + 1 is built beside the pass of frame f, or in line, by the same rules; host frames go through the pinned staging; host output
 * costs one synchronisation, at the end; device output is complete in stream order; afterwards positions, box, lambdas and mask are the
 * caller's and the next snb_execute rebuilds; no step graph is captured or updated; frame steps count in snb_stats.n_rebuilds and in no
 * timer; snb_get_frame_stats counts the batch and its frames.  With positions == NULL (n_frames must be 1) it is ONE evaluation of the
 * engine's current box and positions and behaves as snb_evaluate_atom_energies behaves, a bound context included.
 * In both forms it writes ONLY its output: the forces (snb_get_forces), the buffer of snb_set_force_output, a binding's buffers and the
 * engine's slice-energy buffer (snb_get_slice_energies, snb_slice_energies_device) stay bit for bit what they were.
 * NULL batch, handle, group_energies, group_start or group_atoms, n_groups < 1, a group_start that does not begin at 0 or decreases, an
 * atom index outside [0, n_atoms) (snb_last_error names the group), both include flags 0, a negative n_frames, positions == NULL with
 * n_frames != 1: SNB_ERR_INVALID_ARGUMENT.  shard_count > 1, SNB_Ewald with include_reciprocal: SNB_ERR_UNSUPPORTED.  n_frames == 0 (after
 * these checks): SNB_OK, no work.  Frames given while a context is bound: SNB_ERR_STATE.  Box errors: as snb_evaluate_frames, with the
 * frame index.  The working memory (the table over the sorted atoms, the chunk sums) is allocated at the first call. */
typedef struct {
    int32_t        n_frames;
    const void*    positions;        /* [F][N][3], or [F][N][4] when stride4 != 0; USER atom order; float or double by is_double;
                                        NULL: one evaluation of the engine's CURRENT box and positions (n_frames must be 1) */
    int32_t        is_device;        /* != 0: device pointer on the engine's device, valid until the engine's stream has passed the batch */
    int32_t        is_double;
    int32_t        stride4;
    const double*  boxes;            /* HOST [F][9], reduced form, or NULL: the engine's current box for every frame */
    int32_t        include_direct, include_reciprocal;
    int32_t        n_groups;         /* G >= 1 */
    const int32_t* group_start;      /* HOST [G + 1], group_start[0] == 0, non-decreasing */
    const int32_t* group_atoms;      /* HOST [group_start[G]], USER atom indices */
    double*        group_energies;   /* [F][G][n_subsets][2] raw (Coulomb, vdW) */
    int32_t        out_is_device;
} snb_group_batch;
snb_status snb_evaluate_group_energies(snb_handle h, const snb_group_batch* b);

/* -- per-group forces over stored frames, by subset and at lambda states ----------------------- */
/* The same product for the force table: the table of snb_evaluate_atom_forces summed over lists of atoms (coarse-grained sites, a ligand,
 * residues), for every frame of a stored trajectory, reduced on the device --
 *     group_forces[f][g][J][t][d] = sum_{i in atoms(g)} G_f[i][J][t][d]
 *     state_forces[f][k][g][d]    = sum_{i in atoms(g)} sum_J sum_t state_lambdas[k][slice(s_i, J)][t] G_f[i][J][t][d]
 * with G_f the table of snb_evaluate_atom_forces at frame f: the same attribution, raw (lambda-independent) values, effective parameters,
 * nothing added for the self term, the background or the dispersion correction.  state_forces is the net force on the group at lambda state
 * k -- the force-matching target of a centre-of-mass site, the force on a ligand at every alchemical state from one evaluation per frame.
 * The contraction is done per atom, before the group sum: s_i is the atom's own subset, and a group may span subsets.  n_states == 0: the
 * raw rows alone.  n_states > 0: state_forces, and the raw rows as well unless group_forces is NULL; there is no cap on n_states.  Groups
 * are lists as for snb_evaluate_group_energies: they may overlap, leave atoms out, be empty (zeros), and an index listed twice counts
 * twice.  Every entry of every requested output is written.  The sums use no atomics: an output row is a function of the frame's table
 * alone (the table itself is accumulated with double atomics).
 * With frames given the call follows the contract of snb_evaluate_frames: everything is checked before anything is enqueued; the list of
 * frame f + 1 is built beside the pass of frame f, or in line, by the same rules; host frames go through the pinned staging; host output
 * costs one synchronisation, at the end; device output is complete in stream order; afterwards positions, box, lambdas and mask are the
 * caller's and the next snb_execute rebuilds; no step graph is captured or updated; frame steps count in snb_stats.n_rebuilds and in no
 * timer; snb_get_frame_stats counts the batch and its frames.  With positions == NULL (n_frames must be 1) it is ONE evaluation of the
 * engine's current box and positions and behaves as snb_evaluate_atom_forces behaves, a bound context included.
 * In both forms it writes ONLY its outputs: the forces (snb_get_forces), the buffer of snb_set_force_output, a binding's buffers and the
 * engine's slice-energy buffer (snb_get_slice_energies, snb_slice_energies_device) stay bit for bit what they were.
 * NULL batch, handle, group_start or group_atoms, group_forces NULL with n_states == 0, a negative n_states, n_states > 0 with NULL
 * state_lambdas or state_forces, n_groups < 1, a group_start that does not begin at 0 or decreases, an atom index outside [0, n_atoms)
 * (snb_last_error names the group), both include flags 0, a negative n_frames, positions == NULL with n_frames != 1:
 * SNB_ERR_INVALID_ARGUMENT.  shard_count > 1, SNB_Ewald with include_reciprocal: SNB_ERR_UNSUPPORTED.  n_frames == 0 (after these checks):
 * SNB_OK, no work.  Frames given while a context is bound: SNB_ERR_STATE.  Box errors: as snb_evaluate_frames, with the frame index.  The
 * working memory (the table over the sorted atoms, shared with snb_evaluate_atom_forces; the chunk sums) is allocated at the first call. */
typedef struct {
    int32_t        n_frames;
    const void*    positions;        /* as snb_group_batch: [F][N][3] or [F][N][4]; NULL: the engine's CURRENT box and positions (n_frames must be 1) */
    int32_t        is_device;
    int32_t        is_double;
    int32_t        stride4;
    const double*  boxes;            /* HOST [F][9], reduced form, or NULL: the engine's current box for every frame */
    int32_t        include_direct, include_reciprocal;
    int32_t        n_groups;         /* G >= 1 */
    const int32_t* group_start;      /* HOST [G + 1], group_start[0] == 0, non-decreasing */
    const int32_t* group_atoms;      /* HOST [group_start[G]], USER atom indices */
    double*        group_forces;     /* [F][G][n_subsets][2][3] raw (Coulomb, vdW) x (x, y, z), kJ/mol/nm; may be NULL when n_states > 0 */
    int32_t        out_is_device;
    int32_t        n_states;         /* K >= 0 lambda states */
    const double*  state_lambdas;    /* HOST [K][S][2] */
    double*        state_forces;     /* [F][K][G][3]; same residence as group_forces */
} snb_group_force_batch;
snb_status snb_evaluate_group_forces(snb_handle h, const snb_group_force_batch* b);

/* -- group-pair interaction energy matrix over stored frames, direct space ---------------------- */
/* How much group g interacts with group h, frame by frame -- contact-energy maps, interaction networks, a per-residue-pair decomposition
 * -- without a subset (and a PME mesh) per residue: the call takes its own labelling group_of_atom[n_atoms] (USER order, values -1 or
 * 0 .. G - 1; -1: in no group), independent of the engine's subsets, and fills
 *     pair_energies[f][slice(g, h)][t],     slice(g, h) = max (max + 1) / 2 + min,     t = 0 Coulomb, 1 vdW
 * -- the engine's own slice indexing with G in place of n_subsets, P = G (G + 1) / 2 rows per frame.  An entry is the RAW DIRECT-SPACE
 * energy summed over the unordered atom pairs {i, j} with labels {g, h}, each pair once (g == h included): not scaled by the lambdas and
 * independent of them, with the effective parameters (base values + offsets at the current global parameters).  Attributed: pairs inside
 * the cutoff (diagonal tiles included), the Ewald exclusion corrections (the LJPME dispersion part into t = 1) and the 1-4 exceptions --
 * exactly what an energy-only step with include_direct = 1, include_reciprocal = 0 puts into its slice energies when no
 * dispersion-correction coefficients are set, had every atom's subset been its label.  A pair with an unlabelled end adds nothing.
 * DIRECT SPACE ONLY: the Ewald self term, the neutralising background and the mesh (or k-vector) sum belong to the reciprocal part and are
 * NOT in the matrix, and neither is the long-range dispersion correction; for PME and LJPME the matrix is the short-range part, as the
 * energy groups of other MD codes.  (The reciprocal part of a group-pair matrix needs per-group structure factors and a Gram sum over the
 * mesh: out of scope.  The full energy of a group with a SUBSET is snb_evaluate_group_energies.)  Because nothing reciprocal is
 * attributed the call works with every method, SNB_Ewald included.
 * With frames given the call follows the contract of snb_evaluate_frames: everything is checked before anything is enqueued; the list of
 * frame f + 1 is built beside the pass of frame f, or in line, by the same rules; host frames go through the pinned staging; host output
 * costs one synchronisation, at the end; device output is complete in stream order; afterwards positions, box, lambdas and mask are the
 * caller's and the next snb_execute rebuilds; no step graph is captured or updated; frame steps count in snb_stats.n_rebuilds and in no
 * timer; snb_get_frame_stats counts the batch and its frames.  With positions == NULL (n_frames must be 1) it is ONE evaluation of the
 * engine's current box and positions and behaves as snb_evaluate_atom_energies behaves, a bound context included.
 * In both forms it writes ONLY its output: the forces (snb_get_forces), the buffer of snb_set_force_output, a binding's buffers and the
 * engine's slice-energy buffer (snb_get_slice_energies, snb_slice_energies_device) stay bit for bit what they were.  Every entry of the
 * output is written; rows of empty groups are zeros.  The sums are accumulated per wave and added to the matrix with double atomics:
 * equal from call to call up to the rounding of the sums, not bit for bit, in every precision mode.
 * NULL batch, handle, group_of_atom or pair_energies, n_groups outside 1 .. 4096, a label outside [-1, G) (snb_last_error names the
 * atom), a negative n_frames, positions == NULL with n_frames != 1: SNB_ERR_INVALID_ARGUMENT.  shard_count > 1: SNB_ERR_UNSUPPORTED.
 * n_frames == 0 (after these checks): SNB_OK, no work.  Frames given while a context is bound: SNB_ERR_STATE.  Box errors: as
 * snb_evaluate_frames, with the frame index.  The cap of 4096 groups keeps a frame's row at 134 MB and the key arithmetic in 32 bits: a
 * design limit.  The working memory (the labels in sorted order, one double [P][2] matrix -- held in up to 64 copies while that stays below
 * 512 KB) is allocated at the first call.  Host output is staged on the device in one piece, n_frames * P * 16 bytes, before the one
 * transfer at the end: at G = 4096 a frame is 134 MB, so size n_frames to the device's memory (an allocation that fails is SNB_ERR_HIP),
 * or take device output. */
typedef struct {
    int32_t        n_frames;
    const void*    positions;        /* as snb_group_batch: [F][N][3] or [F][N][4]; NULL: the engine's CURRENT box and positions (n_frames must be 1) */
    int32_t        is_device;
    int32_t        is_double;
    int32_t        stride4;
    const double*  boxes;            /* HOST [F][9], reduced form, or NULL: the engine's current box for every frame */
    int32_t        n_groups;         /* G, 1 .. 4096 */
    const int32_t* group_of_atom;    /* HOST [n_atoms], USER order, -1 or 0 .. G - 1 */
    double*        pair_energies;    /* [F][G (G + 1) / 2][2] raw direct-space (Coulomb, vdW) */
    int32_t        out_is_device;
} snb_group_pair_batch;
snb_status snb_evaluate_group_pair_energies(snb_handle h, const snb_group_pair_batch* b);

/* -- per-slice virial tensors, at the current state and over stored frames --------------------- */
/* The pressure tensor of a frame at every lambda state, split by slice and by Coulomb / van der Waals, from one evaluation:
 *     slice_virials[f][s][t][c] = W_f[s][t][c] = - d E_raw[s][t] / d eps_c,     c over xx, yy, zz, xy, xz, yz,     kJ/mol
 *     state_virials[f][k][c]    = sum_s sum_t state_lambdas[k][s][t] W_f[s][t][c]
 * the derivative of the raw slice energy under the homogeneous deformation r -> (1 + eps) r of the box vectors and of every atom, at fixed
 * pair set: the internal virial in  P_ab V = sum m v_a v_b + sum_s sum_t lambda[s][t] W[s][t][ab]  (the kinetic part is the caller's).
 * E_raw is what an energy-only step with the same include flags leaves in snb_get_slice_energies: pairs inside the cutoff, Ewald
 * exclusion corrections (the LJPME dispersion part into t = 1), 1-4 exceptions, the mesh sums, the neutralising background (with
 * include_reciprocal) and the long-range dispersion correction (with include_direct, where coefficients are set); the Ewald self terms
 * do not depend on the box.  W is raw -- not scaled by the lambdas and independent of them -- with the effective parameters, and
 * symmetric: six components.  A pair adds d_a d_b f once, d as the kernels wrap it; the mesh part is the exact strain derivative of the
 * mesh energy (at fixed fractional coordinates the mesh charges do not change), taken from the forward spectrum of every held mesh; the
 * two closed forms go as 1 / V and add their energy to xx, yy and zz.  A non-periodic system has no box terms.  n_states == 0: the raw
 * rows alone.  n_states > 0: state_virials, and the raw rows as well unless slice_virials is NULL; there is no cap on n_states.  Every
 * entry of every requested output is written; rows of slices of an empty subset are zeros.  The sums are accumulated per wave and added
 * to the working matrix with double atomics: equal from call to call up to the rounding of the sums, not bit for bit.
 * With frames given the call follows the contract of snb_evaluate_frames: everything is checked before anything is enqueued; the list of
 * frame f + 1 is built beside the pass of frame f, or in line, by the same rules; host frames go through the pinned staging; host output
 * costs one synchronisation, at the end; device output is complete in stream order; afterwards positions, box, lambdas and mask are the
 * caller's and the next snb_execute rebuilds; no step graph is captured or updated; frame steps count in snb_stats.n_rebuilds and in no
 * timer; snb_get_frame_stats counts the batch and its frames.  With positions == NULL (n_frames must be 1) it is ONE evaluation of the
 * engine's current box and positions and behaves as snb_evaluate_atom_forces behaves, a bound context included.
 * In both forms it writes ONLY its outputs: the forces (snb_get_forces), the buffer of snb_set_force_output, a binding's buffers and the
 * engine's slice-energy buffer (snb_get_slice_energies, snb_slice_energies_device) stay bit for bit what they were.
 * NULL batch or handle, slice_virials NULL with n_states == 0, a negative n_states, n_states > 0 with NULL state_lambdas or
 * state_virials, both include flags 0, a negative n_frames, positions == NULL with n_frames != 1: SNB_ERR_INVALID_ARGUMENT.
 * shard_count > 1, SNB_Ewald with include_reciprocal (direct-only works): SNB_ERR_UNSUPPORTED.  n_frames == 0 (after these checks):
 * SNB_OK, no work.  Frames given while a context is bound: SNB_ERR_STATE.  Box errors: as snb_evaluate_frames, with the frame index.
 * The mesh part always takes the three-pass transforms (the plane path keeps its spectrum in LDS).  The working memory (the matrix
 * double [64][S][2][6], the states) is allocated at the first call. */
typedef struct {
    int32_t        n_frames;
    const void*    positions;        /* as snb_group_batch: [F][N][3] or [F][N][4]; NULL: the engine's CURRENT box and positions (n_frames must be 1) */
    int32_t        is_device;
    int32_t        is_double;
    int32_t        stride4;
    const double*  boxes;            /* HOST [F][9], reduced form, or NULL: the engine's current box for every frame */
    int32_t        include_direct, include_reciprocal;
    double*        slice_virials;    /* [F][S][2][6] raw (Coulomb, vdW) x (xx, yy, zz, xy, xz, yz), kJ/mol; may be NULL when n_states > 0 */
    int32_t        out_is_device;
    int32_t        n_states;         /* K >= 0 lambda states */
    const double*  state_lambdas;    /* HOST [K][S][2] */
    double*        state_virials;    /* [F][K][6]; same residence as slice_virials */
} snb_virial_batch;
snb_status snb_evaluate_slice_virials(snb_handle h, const snb_virial_batch* b);

/* -- queries ----------------------------------------------------------------------------------- */
snb_status snb_get_pme_parameters(snb_handle h, double* alpha, int32_t grid[3]);
snb_status snb_get_ljpme_parameters(snb_handle h, double* alpha, int32_t grid[3]);
snb_status snb_get_stats(snb_handle h, snb_stats* out);
snb_status snb_reset_timers(snb_handle h);
/* Every n-th execute is enqueued as plain launches with HIP-event stamps around the pair kernel and the reciprocal pipeline (the
 * samples behind snb_stats' kernel timers); the others replay the captured step graph.  Default 32; a short measured region asks
 * for more samples.  n <= 0: never (no timers). */
snb_status snb_set_timing_interval(snb_handle h, int32_t n);
/* Smallest FFT-legal mesh size >= n: no prime factor above 13, the rule of the reference's GPU platforms
 * (platforms/common/include/FFT3DFactory.h:31-47); at least 6. */
int32_t    snb_legal_grid_size(int32_t n);
int32_t    snb_abi_version(void);

/* -- unit-test hooks for the reciprocal building blocks (used by tests/ only; they run the same
 *    kernels the pipeline uses) --------------------------------------------------------------- */
/* Batched 3D real-to-complex forward FFT followed by the inverse, through the engine's own FFT kernels:
 * in[batch][nx][ny][nz] (host, double) -> spectrum[batch][nx][ny][nz/2+1][2] and roundtrip[batch][nx][ny][nz]
 * (unnormalised, like the reference's FFT3D: roundtrip = nx*ny*nz * in).  precision selects the kernel type. */
snb_status snb_test_fft3d(int32_t precision, int32_t device, int32_t batch, int32_t nx, int32_t ny, int32_t nz,
                          const double* in, double* spectrum, double* roundtrip);

#ifdef __cplusplus
}
#endif
#endif /* SNB_H_ */
