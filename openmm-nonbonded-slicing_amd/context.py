"""Host-side mirror of the reference's kernel boundary for the hot path, over the C ABI (``include/snb.h``).

``HipCalcSlicedNonbondedForceKernel`` has the interface of ``NonbondedSlicing::CalcSlicedNonbondedForceKernel``
(openmmapi/include/NonbondedSlicingKernels.h:27-85): ``initialize / execute / copyParametersToContext /
getPMEParameters / getLJPMEParameters``.  ``SlicedNonbondedForceImpl`` restates the validation and the force-group ->
(includeDirect, includeReciprocal) mapping of openmmapi/src/SlicedNonbondedForceImpl.cpp:33-142.
``System`` / ``Context`` / ``State`` are the minimum of OpenMM's driver needed so that tests read like the
reference's own (tests/TestSlicedNonbondedForce.h): they hold positions, box vectors and global parameters, nothing else.

All arithmetic happens in ``libsnb_hip.so``; this module only moves parameters (scaling parameters -> lambdas,
parameter offsets -> effective (q, sigma, epsilon), raw slice energies -> energy and dE/dlambda).
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from . import _capi
from .force import OpenMMException, SlicedNonbondedForce, sliceIndex


def _dp(a): return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
def _ip(a): return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def calcPMEParameters(force, boxVectors, lj=False):
    """OpenMM ``NonbondedForceImpl::calcPMEParameters`` (third-party; formula restated from OpenMM 8.x and
    NOT pinned by any fixture of the reference -- parity runs always pass explicit PME parameters)."""
    alpha, nx, ny, nz = force.getLJPMEParameters() if lj else force.getPMEParameters()
    if alpha == 0.0:
        tol = force.getEwaldErrorTolerance()
        alpha = math.sqrt(-math.log(2 * tol)) / force.getCutoffDistance()
        dims = []
        for d in range(3):
            L = boxVectors[d][d]
            n = (alpha * L / (3 * tol ** 0.2)) if lj else (2 * alpha * L / (3 * tol ** 0.2))
            dims.append(max(int(math.ceil(n)), 6))
        nx, ny, nz = dims
    return alpha, nx, ny, nz


def calcEwaldParameters(force, boxVectors):
    """OpenMM ``NonbondedForceImpl::calcEwaldParameters`` (third-party; restated from OpenMM 8.x, NOT pinned by a
    reference fixture).  A mesh-less explicit override for parity runs: ``force.ewaldKmax = (kx, ky, kz)`` with the alpha of
    ``setPMEParameters``."""
    alpha = force.getPMEParameters()[0]
    tol = force.getEwaldErrorTolerance()
    if alpha == 0.0:
        alpha = math.sqrt(-math.log(2 * tol)) / force.getCutoffDistance()
    explicit = getattr(force, "ewaldKmax", None)
    if explicit is not None:
        return (alpha,) + tuple(int(k) for k in explicit)

    def find(width):
        f = lambda k: tol - 0.05 * math.sqrt(width * alpha) * k * math.exp(-(k * math.pi / (width * alpha)) ** 2)
        k = 10
        v = f(k)
        if v > 0.0:
            while v > 0.0 and k > 0:
                k -= 1; v = f(k)
            k += 1
        else:
            while v < 0.0:
                k += 1; v = f(k)
        return k if k % 2 == 1 else k + 1
    return alpha, find(boxVectors[0][0]), find(boxVectors[1][1]), find(boxVectors[2][2])


VIRIAL_COMPONENTS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))      # the six entries of a virial row: xx, yy, zz, xy, xz, yz
KJ_PER_MOL_NM3_IN_BAR = 16.6053906717      # 1 kJ/mol/nm^3 = 1e3 J / N_A / 1e-27 m^3 = 1.66053906717e6 Pa


def virialMatrix(rows):
    """Virial rows [..., 6] (xx, yy, zz, xy, xz, yz) as symmetric matrices [..., 3, 3]."""
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros(rows.shape[:-1] + (3, 3))
    for c, (a, b) in enumerate(VIRIAL_COMPONENTS):
        out[..., a, b] = rows[..., c]
        out[..., b, a] = rows[..., c]
    return out


def virialsAtStates(rows, lambdaStates):
    """The virial [..., K, 6] that per-slice rows [..., S, 2, 6] imply at the lambda states [K][S][2]:
    ``sum_s sum_t lambdaStates[k][s][t] rows[..., s, t, :]`` -- the NumPy statement of state_virials."""
    rows = np.asarray(rows, dtype=np.float64); lam = np.asarray(lambdaStates, dtype=np.float64)
    return np.einsum("kst,...stc->...kc", lam.reshape(-1, rows.shape[-3], 2), rows)


def pressureFromVirial(virial, volume, kinetic=None):
    """The pressure tensor ``P = (kinetic + virial) / volume`` in kJ/mol/nm^3, from the internal virial (rows [..., 6] or matrices
    [..., 3, 3], kJ/mol, e.g. a row of virialsAtStates), the volume in nm^3 and, when given, the kinetic part ``sum_i m_i v_ia v_ib`` in
    the same shape and unit (None: the virial pressure alone).  Multiply by KJ_PER_MOL_NM3_IN_BAR = 16.6053906717 for bar."""
    p = np.asarray(virial, dtype=np.float64)
    if kinetic is not None:
        p = p + np.asarray(kinetic, dtype=np.float64)
    return p / float(volume)


class HipCalcSlicedNonbondedForceKernel:
    """MI355X kernel object behind the reference's ``CalcSlicedNonbondedForceKernel`` interface."""

    @staticmethod
    def Name():
        return "CalcSlicedNonbondedForce"

    def __init__(self, precision="single", device=0, neighbor_padding=0.0, rebuild_interval=1, shard_rank=0, shard_count=1, stream=None):
        self._lib = _capi.lib()
        self._h = ctypes.c_void_p()
        self.precision = precision
        self.device = device
        self.neighbor_padding = neighbor_padding
        self.rebuild_interval = rebuild_interval
        self.shard_rank, self.shard_count = shard_rank, shard_count
        self.stream = stream
        self.force = None
        self._bound = None

    def __del__(self):
        try:
            if self._h:
                self._lib.snb_destroy(self._h); self._h = ctypes.c_void_p()
        except Exception:
            pass

    # -- error plumbing: status codes -> the exceptions the reference throws -----------------------
    def _check(self, status):
        if status != _capi.SNB_OK:
            msg = self._lib.snb_last_error(self._h)
            raise OpenMMException((msg or b"").decode() or "snb error %d" % status)

    # -- CalcSlicedNonbondedForceKernel::initialize (NonbondedSlicingKernels.h:48) ------------------
    def initialize(self, system, force):
        self.force = force
        self.numParticles = force.getNumParticles()
        self.numSubsets = force.getNumSubsets()
        self.numSlices = force.getNumSlices()
        cfg = _capi.SnbConfig()
        cfg.abi_version = _capi.SNB_ABI_VERSION
        cfg.n_atoms = self.numParticles; cfg.n_subsets = self.numSubsets
        method = force.getNonbondedMethod()
        cfg.method = method
        cfg.precision = {"single": 0, "double": 1, "mixed": 2}[self.precision]
        cfg.use_switch = int(force.getUseSwitchingFunction() and method != SlicedNonbondedForce.NoCutoff)
        cfg.exceptions_periodic = int(force.getExceptionsUsePeriodicBoundaryConditions())
        cfg.device = self.device
        cfg.cutoff = force.getCutoffDistance(); cfg.switch_distance = force.getSwitchingDistance()
        cfg.rf_dielectric = force.getReactionFieldDielectric()
        box = system.getDefaultPeriodicBoxVectors()
        if method in (SlicedNonbondedForce.PME, SlicedNonbondedForce.LJPME):
            a, nx, ny, nz = calcPMEParameters(force, box, False)
            cfg.alpha = a; cfg.grid[0], cfg.grid[1], cfg.grid[2] = nx, ny, nz
        if method == SlicedNonbondedForce.LJPME:
            a, nx, ny, nz = calcPMEParameters(force, box, True)
            cfg.alpha_d = a; cfg.dgrid[0], cfg.dgrid[1], cfg.dgrid[2] = nx, ny, nz
        if method == SlicedNonbondedForce.Ewald:
            a, kx, ky, kz = calcEwaldParameters(force, box)
            cfg.alpha = a; cfg.kmax[0], cfg.kmax[1], cfg.kmax[2] = kx, ky, kz
        cfg.neighbor_padding = self.neighbor_padding; cfg.rebuild_interval = self.rebuild_interval
        cfg.shard_rank = self.shard_rank; cfg.shard_count = self.shard_count
        cfg.stream = self.stream
        status = self._lib.snb_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if status != _capi.SNB_OK:
            raise OpenMMException((self._lib.snb_last_error(None) or b"").decode() or "snb_create failed (%d)" % status)
        self._upload_definition(force)

    def _upload_definition(self, force):
        n = self.numParticles
        self._base = np.array([force.getParticleParameters(i) for i in range(n)], dtype=np.float64).reshape(n, 3)
        self._subset = np.array([force.getParticleSubset(i) for i in range(n)], dtype=np.int32)
        m = force.getNumExceptions()
        exc = [force.getExceptionParameters(k) for k in range(m)]
        self._excPairs = np.array([[e[0], e[1]] for e in exc], dtype=np.int32).reshape(m, 2)
        self._excBase = np.array([[e[2], e[3], e[4]] for e in exc], dtype=np.float64).reshape(m, 3)
        self._particleOffsets = [force.getParticleParameterOffset(k) for k in range(force.getNumParticleParameterOffsets())]
        self._exceptionOffsets = [force.getExceptionParameterOffset(k) for k in range(force.getNumExceptionParameterOffsets())]
        self._force14 = np.zeros(max(m, 1), dtype=np.int32)
        for (_, idx, _, _, _) in self._exceptionOffsets:
            self._force14[idx] = 1   # Q6: an exception with an offset is a 1-4 even when its base values are zero
        # scaling parameters -> (slice, term) bindings (ReferenceNonbondedSlicingKernels.cpp:58-87)
        self._binding = {}
        derivs = set(force.getEnergyParameterDerivativeName(i) for i in range(force.getNumEnergyParameterDerivatives()))
        for k in range(force.getNumScalingParameters()):
            name, s1, s2, incC, incLJ = force.getScalingParameter(k)
            s = sliceIndex(s1, s2)
            if incC: self._binding[(s, 0)] = (name, name in derivs)
            if incLJ: self._binding[(s, 1)] = (name, name in derivs)
        self._derivNames = derivs
        self._lastLambdas = None
        # dispersion-correction coefficients at DEFAULT parameter values (SlicedNonbondedForceImpl.cpp:281-291)
        defaults = {force.getGlobalParameterName(i): force.getGlobalParameterDefaultValue(i) for i in range(force.getNumGlobalParameters())}
        self._set_dispersion(force, defaults)
        self._push_definition()
        # slices whose raw energy a derivative-only step must produce: those bound to a parameter with a requested derivative
        mask = np.zeros(self.numSlices, dtype=np.int32)
        for (sl, _t), (_name, hasDeriv) in self._binding.items():
            if hasDeriv:
                mask[sl] = 1
        self._derivMask = mask
        self._check(self._lib.snb_set_energy_slices(self._h, _ip(mask)))

    def _effective(self, params):
        p = self._base.copy()
        for (name, idx, dq, ds, de) in self._particleOffsets:
            v = params[name]
            p[idx, 0] += v * dq; p[idx, 1] += v * ds; p[idx, 2] += v * de
        e = self._excBase.copy()
        for (name, idx, da, db, dc) in self._exceptionOffsets:
            v = params[name]
            e[idx, 0] += v * da; e[idx, 1] += v * db; e[idx, 2] += v * dc
        return p, e

    def _set_dispersion(self, force, params):
        method = force.getNonbondedMethod()
        coef = np.zeros(self.numSlices)
        if force.getUseDispersionCorrection() and method in (SlicedNonbondedForce.CutoffPeriodic, SlicedNonbondedForce.Ewald, SlicedNonbondedForce.PME, SlicedNonbondedForce.LJPME):
            p, _ = self._effective(params)
            sig = np.ascontiguousarray(p[:, 1]); eps = np.ascontiguousarray(p[:, 2])
            useSwitch = int(force.getUseSwitchingFunction())
            self._check(self._lib.snb_compute_dispersion_coefficients(self.numParticles, self.numSubsets, _dp(sig), _dp(eps), _ip(self._subset),
                                                                      force.getCutoffDistance(), useSwitch, force.getSwitchingDistance(), _dp(coef)))
        self._dispCoef = coef
        self._check(self._lib.snb_set_dispersion_coefficients(self._h, _dp(coef)))

    def _push_definition(self):
        """Base parameters, exceptions and parameter offsets to the engine (once per initialize / copyParametersToContext): the
        effective values base + sum global * offset are formed ON THE DEVICE (include/snb.h, snb_set_parameter_offsets), as the
        reference does in platforms/common/src/kernels/nonbondedParameters.cc:4-179."""
        p = self._base
        q = np.ascontiguousarray(p[:, 0]); sg = np.ascontiguousarray(p[:, 1]); ep = np.ascontiguousarray(p[:, 2])
        self._check(self._lib.snb_set_particles(self._h, _dp(q), _dp(sg), _dp(ep), _ip(self._subset)))
        m = self._excPairs.shape[0]
        if m > 0:
            e = self._excBase
            qq = np.ascontiguousarray(e[:, 0]); es = np.ascontiguousarray(e[:, 1]); ee = np.ascontiguousarray(e[:, 2])
            self._check(self._lib.snb_set_exceptions(self._h, m, _ip(self._excPairs), _dp(qq), _dp(es), _dp(ee), _ip(self._force14)))
        else:
            self._check(self._lib.snb_set_exceptions(self._h, 0, None, None, None, None, None))
        names = sorted(set(o[0] for o in self._particleOffsets) | set(o[0] for o in self._exceptionOffsets))
        self._offsetGlobals = names
        index = {n: k for k, n in enumerate(names)}
        pi = np.array([o[1] for o in self._particleOffsets], dtype=np.int32); pg = np.array([index[o[0]] for o in self._particleOffsets], dtype=np.int32)
        pd = np.ascontiguousarray(np.array([[o[2], o[3], o[4]] for o in self._particleOffsets], dtype=np.float64).reshape(-1, 3))
        ei = np.array([o[1] for o in self._exceptionOffsets], dtype=np.int32); eg = np.array([index[o[0]] for o in self._exceptionOffsets], dtype=np.int32)
        ed = np.ascontiguousarray(np.array([[o[2], o[3], o[4]] for o in self._exceptionOffsets], dtype=np.float64).reshape(-1, 3))
        self._check(self._lib.snb_set_parameter_offsets(self._h, len(names), len(pi), _ip(pi) if len(pi) else None, _ip(pg) if len(pi) else None, _dp(pd) if len(pi) else None,
                                                        len(ei), _ip(ei) if len(ei) else None, _ip(eg) if len(ei) else None, _dp(ed) if len(ei) else None))
        self._lastGlobals = None

    def _push_parameters(self, params):
        if self._offsetGlobals:
            vals = np.array([params[n] for n in self._offsetGlobals], dtype=np.float64)
            if self._lastGlobals is None or not np.array_equal(vals, self._lastGlobals):
                self._check(self._lib.snb_set_global_parameters(self._h, len(vals), _dp(vals)))
                self._lastGlobals = vals
        lam = np.ones((self.numSlices, 2))
        for (s, t), (name, _) in self._binding.items():
            lam[s, t] = params[name]
        if self._lastLambdas is None or not np.array_equal(lam, self._lastLambdas):
            self._check(self._lib.snb_set_lambdas(self._h, _dp(np.ascontiguousarray(lam))))
            self._lastLambdas = lam

    # -- context binding (include/snb.h, snb_bind_context) -----------------------------------------
    def bindContextBuffers(self, posq, atomIndex, paddedNumAtoms, forceBuffer=None, energyBuffer=None, derivBuffer=None, derivNames=None,
                           posqIsDouble=False, energyIsDouble=True):
        """Name the device buffers of a GPU platform's context, once: ``posq`` ([>= N][4], context order), ``atomIndex`` ([N] int32,
        atomIndex[slot] = user index), the 64-bit fixed-point force buffer ([3][paddedNumAtoms], added to), the energy accumulator
        (scalar) and the energy-parameter-derivative accumulator, whose entry k belongs to ``derivNames[k]``.  All are device addresses
        (integers) valid on the engine's device; None = not delivered.  From then on ``execute`` pushes parameters and box only, adds
        forces, energy and derivatives into those buffers on the engine's stream, reads nothing back and returns 0.0, as the reference's
        GPU kernels do."""
        slots = np.full((self.numSlices, 2), -1, dtype=np.int32)
        if derivBuffer is not None:
            index = {name: k for k, name in enumerate(derivNames or [])}
            for (s, t), (name, hasDeriv) in self._binding.items():
                if hasDeriv and name in index:
                    slots[s, t] = index[name]
        b = _capi.SnbContextBinding()
        b.posq = posq; b.atom_index = atomIndex; b.is_double = int(bool(posqIsDouble)); b.padded_n = int(paddedNumAtoms)
        b.force_buffer = forceBuffer; b.energy_buffer = energyBuffer; b.deriv_buffer = derivBuffer
        b.deriv_slot = _ip(slots) if derivBuffer is not None else None
        b.energy_is_double = int(bool(energyIsDouble))
        self._check(self._lib.snb_bind_context(self._h, ctypes.byref(b)))
        self._bound = b

    def unbindContextBuffers(self):
        self._check(self._lib.snb_bind_context(self._h, None))
        self._bound = None

    def contextOrderChanged(self):
        """The context has reordered its atoms (rewritten atomIndex): call before the next execute.  One small kernel, no rebuild."""
        self._check(self._lib.snb_context_order_changed(self._h))

    def _push_state(self, context):
        self._push_parameters(context.getParameters())
        box = np.ascontiguousarray(context.getPeriodicBoxVectors(), dtype=np.float64).reshape(9)
        self._check(self._lib.snb_set_box(self._h, _dp(box)))
        if self._bound is not None:      # the coordinates come from the bound posq
            return
        pos = context._positions
        self._check(self._lib.snb_set_positions(self._h, pos.ctypes.data_as(ctypes.c_void_p), 0, 1, 0))

    # -- CalcSlicedNonbondedForceKernel::execute (NonbondedSlicingKernels.h:59) ---------------------
    # (includeForces false: an energy-only step -- the engine evaluates no forces and keeps those of the last forces step; nothing is read back)
    def execute(self, context, includeForces, includeEnergy, includeDirect, includeReciprocal):
        self._push_state(context)
        if self._bound is not None:
            # bound context: everything is added into its device buffers on the engine's stream; nothing is read back, nothing synchronises
            mode = 1 if includeEnergy else (2 if self._derivNames else 0)
            self._check(self._lib.snb_execute(self._h, int(includeForces), mode, int(includeDirect), int(includeReciprocal), None))
            return 0.0
        energy = ctypes.c_double(0.0)
        wantE = bool(includeEnergy) or bool(self._derivNames)
        # Q4: derivatives accumulate whether or not the energy is requested -- then only the slices they are bound to are evaluated (mode 2)
        mode = 1 if includeEnergy else (2 if self._derivNames else 0)
        self._check(self._lib.snb_execute(self._h, int(includeForces), mode, int(includeDirect), int(includeReciprocal), ctypes.byref(energy) if mode == 1 else None))
        if includeForces:
            self._check(self._lib.snb_get_forces(self._h, context._forces.ctypes.data_as(ctypes.c_void_p), 0, 1, 1))
        if wantE:
            sl = np.zeros((self.numSlices, 2))
            self._check(self._lib.snb_get_slice_energies(self._h, _dp(sl)))
            self.lastSliceEnergies = sl
            # Q4: derivatives accumulate whether or not the energy was requested (ReferenceNonbondedSlicingKernels.cpp:259-265)
            for (s, t), (name, hasDeriv) in self._binding.items():
                if hasDeriv:
                    context._energyParamDerivs[name] = context._energyParamDerivs.get(name, 0.0) + sl[s, t]
        return energy.value if includeEnergy else 0.0

    def computeSliceEnergies(self, context, slices=None):
        """Raw per-slice energies [S][2] (Coulomb, vdW) at the context's positions and box, from one energy-only step (include_forces = 0).
        The energy of any lambda state is their linear combination, E(lambda) = sum_s lambda_s . E_s: the per-frame call of an MBAR or
        reweighting pass.  slices: indices of the slices wanted -- only those are evaluated (include_energy = 2), the other rows are NaN;
        None: every slice.  The forces of the last forces step stay where they are."""
        self._push_state(context)
        if slices is None:
            self._check(self._lib.snb_execute(self._h, 0, 1, 1, 1, None))
        else:
            mask = np.zeros(self.numSlices, dtype=np.int32)
            mask[np.asarray(list(slices), dtype=np.int64)] = 1
            self._check(self._lib.snb_set_energy_slices(self._h, _ip(mask)))
            try:
                self._check(self._lib.snb_execute(self._h, 0, 2, 1, 1, None))
            finally:      # (the derivative-only steps of execute() keep their own mask)
                self._check(self._lib.snb_set_energy_slices(self._h, _ip(self._derivMask)))
        sl = np.zeros((self.numSlices, 2))
        self._check(self._lib.snb_get_slice_energies(self._h, _dp(sl)))
        if slices is not None:
            sl[mask == 0] = np.nan
        return sl

    def computeAtomEnergies(self, context, includeDirect=True, includeReciprocal=True, devicePointer=None):
        """Per-atom interaction energies with every subset (include/snb.h, snb_evaluate_atom_energies): ``A[i][J] = (Coulomb, vdW)`` raw
        energy of atom i with all atoms of subset J at the context's positions, box and parameters, in one evaluation -- where a slice's
        energy sits (which residues carry the ligand-protein Coulomb energy), without one subset and one PME mesh per residue.  Returns an
        ndarray (N, n_subsets, 2) in user atom order, or None when ``devicePointer`` (address of a double [N][n_subsets][2] array on the
        engine's device, complete in stream order) takes the table.  Not scaled by the lambdas; the long-range dispersion correction is a
        per-slice constant and is not attributed.  Forces, force outputs and the slice energies of the last steps stay as they are."""
        self._push_state(context)
        if devicePointer is not None:
            self._check(self._lib.snb_evaluate_atom_energies(self._h, int(bool(includeDirect)), int(bool(includeReciprocal)), ctypes.c_void_p(int(devicePointer)), 1))
            return None
        out = np.zeros((self.numParticles, self.numSubsets, 2))
        self._check(self._lib.snb_evaluate_atom_energies(self._h, int(bool(includeDirect)), int(bool(includeReciprocal)), out.ctypes.data_as(ctypes.c_void_p), 0))
        return out

    @staticmethod
    def sliceEnergiesFromAtomEnergies(table, subsets):
        """The raw slice energies (S, 2) a per-atom table implies: E[slice(I, J)] = sum_{i in I} A[i][J] for I != J, and half that sum on
        the diagonal, where every pair is counted from both ends.  The off-diagonal entry is taken from the larger subset index's atoms
        (the other half of the table gives the same number)."""
        table = np.asarray(table, dtype=np.float64); subsets = np.asarray(subsets)
        n = table.shape[1]
        out = np.zeros((n * (n + 1) // 2, 2))
        for i in range(n):
            rows = table[subsets == i].sum(axis=0)      # (n, 2): subset i's atoms with every subset
            for j in range(i + 1):
                out[sliceIndex(i, j)] = rows[j] * (0.5 if i == j else 1.0)
        return out

    @staticmethod
    def groupAtomEnergies(table, groups):
        """Sums of a per-atom table over lists of atom indices, one list per group (residue): (G, n_subsets, 2)."""
        table = np.asarray(table, dtype=np.float64)
        out = np.zeros((len(groups),) + table.shape[1:])
        for g, atoms in enumerate(groups):
            out[g] = table[np.asarray(list(atoms), dtype=np.int64)].sum(axis=0)
        return out

    def computeAtomForces(self, context, includeDirect=True, includeReciprocal=True, devicePointer=None):
        """Per-atom forces by partner subset and term (include/snb.h, snb_evaluate_atom_forces): ``G[i][J][t] = -dE_raw[slice(s_i, J)][t]/dr_i``,
        the (Coulomb, vdW) force all atoms of subset J put on atom i at the context's positions, box and parameters, in one evaluation --
        the mean force of the solvent on a ligand atom, force-matching targets, the forces at any lambda state (forcesFromAtomForces).
        Returns an ndarray (N, n_subsets, 2, 3) in user atom order, kJ/mol/nm, or None when ``devicePointer`` (address of a double
        [N][n_subsets][2][3] array on the engine's device, complete in stream order) takes the table.  Not scaled by the lambdas.  Forces,
        force outputs and the slice energies of the last steps stay as they are."""
        self._push_state(context)
        if devicePointer is not None:
            self._check(self._lib.snb_evaluate_atom_forces(self._h, int(bool(includeDirect)), int(bool(includeReciprocal)), ctypes.c_void_p(int(devicePointer)), 1))
            return None
        out = np.zeros((self.numParticles, self.numSubsets, 2, 3))
        self._check(self._lib.snb_evaluate_atom_forces(self._h, int(bool(includeDirect)), int(bool(includeReciprocal)), out.ctypes.data_as(ctypes.c_void_p), 0))
        return out

    @staticmethod
    def forcesFromAtomForces(table, subsets, lambdas):
        """The forces (N, 3) a per-atom force table implies at a lambda state: F_i = sum_J sum_t lambdas[slice(s_i, J)][t] G[i][J][t], with
        ``lambdas`` the (S, 2) table of (Coulomb, vdW) scaling factors per slice."""
        table = np.asarray(table, dtype=np.float64); subsets = np.asarray(subsets); lambdas = np.asarray(lambdas, dtype=np.float64)
        n = table.shape[1]
        out = np.zeros((table.shape[0], 3))
        for i in range(n):
            rows = subsets == i
            for j in range(n):
                out[rows] += np.einsum("t,ntd->nd", lambdas[sliceIndex(i, j)], table[rows, j])
        return out

    @staticmethod
    def groupAtomForces(table, groups):
        """Sums of a per-atom force table over lists of atom indices, one list per group (residue, molecule): (G, n_subsets, 2, 3)."""
        return HipCalcSlicedNonbondedForceKernel.groupAtomEnergies(table, groups)      # (the reduction does not depend on the entry's shape)

    def _push_frame_state(self, context):
        """What a ...ForFrames call pushes from the context first: parameters, lambdas and the box (the frames bring the positions)."""
        self._push_parameters(context.getParameters())
        box = np.ascontiguousarray(context.getPeriodicBoxVectors(), dtype=np.float64).reshape(9)
        self._check(self._lib.snb_set_box(self._h, _dp(box)))

    def _frames_into(self, b, who, positions, boxes, positionsDevicePointer, numFrames):
        """The frames arguments the ...ForFrames methods share, written into the batch b (n_frames, positions, is_device, is_double,
        stride4, boxes).  Returns (F, the arrays b points into: the caller keeps them until the call has returned)."""
        keep = []
        if positionsDevicePointer is not None:
            if positions is not None or numFrames is None:
                raise OpenMMException("%s: positionsDevicePointer goes with numFrames and without positions" % who)
            ptr, isDouble = positionsDevicePointer
            F = int(numFrames)
            b.positions = ctypes.c_void_p(int(ptr)); b.is_device = 1; b.is_double = int(bool(isDouble))
        else:
            pos = np.asarray(positions)
            if pos.dtype != np.float32:
                pos = pos.astype(np.float64, copy=False)
            pos = np.ascontiguousarray(pos)
            if pos.ndim != 3 or pos.shape[1:] != (self.numParticles, 3):
                raise OpenMMException("%s: positions must be [F][%d][3]" % (who, self.numParticles))
            F = pos.shape[0]
            keep.append(pos)
            b.positions = pos.ctypes.data_as(ctypes.c_void_p); b.is_device = 0; b.is_double = int(pos.dtype == np.float64)
        b.n_frames = F; b.stride4 = 0
        if boxes is not None:
            bx = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 9))
            if bx.shape[0] != F:
                raise OpenMMException("%s: one box per frame" % who)
            keep.append(bx)
            b.boxes = _dp(bx)
        return F, keep

    def computeSliceEnergiesForFrames(self, context, positions=None, boxes=None, slices=None, lambdaStates=None, positionsDevicePointer=None, numFrames=None):
        """Raw per-slice energies [F][S][2] of F stored frames in one call (include/snb.h, snb_evaluate_frames): the loop of an MBAR or
        reweighting pass over a trajectory, pipelined inside the engine -- the list of the next frame is built beside the step of this one.
        positions: NumPy [F][N][3], float32 or float64 (host).  Frames already on the device: positionsDevicePointer=(address, isDouble) of
        a contiguous [F][N][3] array on the engine's device, with numFrames.  boxes: [F][3][3] (or [F][9]) reduced box vectors per frame;
        None: the context's box for every frame.  slices: as in computeSliceEnergies -- only those are evaluated, the other rows are NaN.
        lambdaStates: [K][S][2]; then the result is (sliceEnergies, stateEnergies[F][K]), stateEnergies[f][k] = sum lambdaStates[k] *
        sliceEnergies[f], summed on the device (every slice must be evaluated: not with slices).  Parameters and lambdas are pushed from the
        context first; the context's own positions, the forces of the last forces step and the derivative mask stay as they are."""
        self._push_frame_state(context)
        S = self.numSlices
        b = _capi.SnbFrameBatch()
        F, keep = self._frames_into(b, "computeSliceEnergiesForFrames", positions, boxes, positionsDevicePointer, numFrames)
        b.mode = 1 if slices is None else 2
        b.include_direct = 1; b.include_reciprocal = 1
        out = np.zeros((F, S, 2))
        b.slice_energies = out.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        states = None
        if lambdaStates is not None:
            lam = np.ascontiguousarray(np.asarray(lambdaStates, dtype=np.float64).reshape(-1, S, 2))
            states = np.zeros((F, lam.shape[0]))
            b.n_states = lam.shape[0]; b.state_lambdas = _dp(lam); b.state_energies = states.ctypes.data_as(ctypes.c_void_p)
        if slices is None:
            self._check(self._lib.snb_evaluate_frames(self._h, ctypes.byref(b)))
        else:
            mask = np.zeros(S, dtype=np.int32)
            mask[np.asarray(list(slices), dtype=np.int64)] = 1
            self._check(self._lib.snb_set_energy_slices(self._h, _ip(mask)))
            try:
                self._check(self._lib.snb_evaluate_frames(self._h, ctypes.byref(b)))
            finally:      # (the derivative-only steps of execute() keep their own mask)
                self._check(self._lib.snb_set_energy_slices(self._h, _ip(self._derivMask)))
            out[:, mask == 0] = np.nan
        return out if states is None else (out, states)

    @staticmethod
    def groupsToCSR(groups):
        """Lists of atom indices, one per group, as the CSR pair of snb_group_batch: (group_start int32 [G + 1], group_atoms int32
        [group_start[G]]).  The lists are kept as given: overlapping, empty, with repeated indices."""
        lists = [np.asarray(list(g), dtype=np.int64).reshape(-1) for g in groups]
        start = np.zeros(len(lists) + 1, dtype=np.int32)
        if lists:
            start[1:] = np.cumsum([len(a) for a in lists])
        atoms = np.concatenate(lists).astype(np.int32) if start[-1] > 0 else np.zeros(0, dtype=np.int32)
        return start, np.ascontiguousarray(atoms)

    def _groupBatch(self, groups, includeDirect, includeReciprocal, batch=_capi.SnbGroupBatch):
        start, atoms = self.groupsToCSR(groups)
        if len(start) < 2:
            raise OpenMMException("group energies and forces: at least one group")
        b = batch()
        if len(atoms) == 0:
            atoms = np.zeros(1, dtype=np.int32)      # (only empty groups: group_atoms must still be an address)
        b.n_groups = len(start) - 1; b.group_start = _ip(start); b.group_atoms = _ip(atoms)
        b.include_direct = int(bool(includeDirect)); b.include_reciprocal = int(bool(includeReciprocal))
        return b, (start, atoms)      # (the arrays the batch points into: the caller keeps them until the call has returned)

    def computeGroupEnergies(self, context, groups, includeDirect=True, includeReciprocal=True, devicePointer=None):
        """Per-group interaction energies with every subset at the context's positions, box and parameters (include/snb.h,
        snb_evaluate_group_energies with positions == NULL): the table of computeAtomEnergies summed over each list of atom indices in
        ``groups`` on the device, (G, n_subsets, 2) -- what groupAtomEnergies(computeAtomEnergies(...), groups) gives, without the per-atom
        table crossing to the host.  devicePointer: address of a double [G][n_subsets][2] array on the engine's device that takes the
        result (complete in stream order); then None is returned."""
        self._push_state(context)
        b, keep = self._groupBatch(groups, includeDirect, includeReciprocal)
        b.n_frames = 1
        out = None
        if devicePointer is not None:
            b.group_energies = ctypes.c_void_p(int(devicePointer)); b.out_is_device = 1
        else:
            out = np.zeros((b.n_groups, self.numSubsets, 2))
            b.group_energies = out.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        self._check(self._lib.snb_evaluate_group_energies(self._h, ctypes.byref(b)))
        return out

    def computeGroupEnergiesForFrames(self, context, groups, positions=None, boxes=None, includeDirect=True, includeReciprocal=True, positionsDevicePointer=None,
                                      numFrames=None, devicePointer=None):
        """Per-group interaction energies [F][G][n_subsets][2] of F stored frames in one call (include/snb.h, snb_evaluate_group_energies):
        the Coulomb and vdW energy of every residue with the ligand subset frame by frame, a per-residue decomposition over a trajectory --
        the frame pipeline of computeSliceEnergiesForFrames with the atom-energy pass as its step and the sum over each group's atoms on the
        device.  groups: a list of lists of atom indices, as in groupAtomEnergies.  positions, boxes, positionsDevicePointer, numFrames: as
        in computeSliceEnergiesForFrames.  devicePointer: address of a double [F][G][n_subsets][2] array on the engine's device that takes
        the result (complete in stream order); then None is returned.  Parameters are pushed from the context first; the context's own
        positions, the forces and the slice energies of the last steps stay as they are."""
        self._push_frame_state(context)
        b, keep = self._groupBatch(groups, includeDirect, includeReciprocal)
        if positions is None and positionsDevicePointer is None:
            raise OpenMMException("computeGroupEnergiesForFrames: positions or positionsDevicePointer must be given (computeGroupEnergies evaluates the context's own state)")
        F, frames = self._frames_into(b, "computeGroupEnergiesForFrames", positions, boxes, positionsDevicePointer, numFrames)
        out = None
        if devicePointer is not None:
            b.group_energies = ctypes.c_void_p(int(devicePointer)); b.out_is_device = 1
        else:
            out = np.zeros((F, b.n_groups, self.numSubsets, 2))
            b.group_energies = out.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        self._check(self._lib.snb_evaluate_group_energies(self._h, ctypes.byref(b)))
        return out

    @staticmethod
    def groupPairIndex(g, h):
        """Row of the group pair (g, h) in a group-pair matrix: max (max + 1) / 2 + min, the slice indexing with the labels as subsets."""
        g, h = int(g), int(h)
        if g < 0 or h < 0:
            raise OpenMMException("groupPairIndex: labels must not be negative")
        return g * (g + 1) // 2 + h if g > h else h * (h + 1) // 2 + g

    @staticmethod
    def groupPairMatrix(rows, numGroups):
        """Rows [..., P, 2] of computeGroupPairEnergies (P = G (G + 1) / 2) as the symmetric [..., G, G, 2]: entry [g][h] = [h][g] = the
        energy of the pairs with labels {g, h}; the diagonal holds the energy inside a group, once."""
        rows = np.asarray(rows); G = int(numGroups)
        if rows.ndim < 2 or rows.shape[-2:] != (G * (G + 1) // 2, 2):
            raise OpenMMException("groupPairMatrix: rows must be [..., %d, 2] for %d groups" % (G * (G + 1) // 2, G))
        g, h = np.tril_indices(G)      # (row-major lower triangle: g (g + 1) / 2 + h, the order of the rows)
        out = np.zeros(rows.shape[:-2] + (G, G, 2), dtype=rows.dtype)
        out[..., g, h, :] = rows
        out[..., h, g, :] = rows
        return out

    @staticmethod
    def labelsFromGroups(groups, numAtoms):
        """Disjoint lists of atom indices, one per group, as the label array of computeGroupPairEnergies: int32 [numAtoms], label g on the
        atoms of list g, -1 on atoms in no list.  An atom in two lists (or twice in one) is refused: a label array cannot say it."""
        labels = np.full(int(numAtoms), -1, dtype=np.int32)
        for g, lst in enumerate(groups):
            for a in np.asarray(list(lst), dtype=np.int64).reshape(-1):
                if a < 0 or a >= numAtoms:
                    raise OpenMMException("labelsFromGroups: group %d: atom index %d is outside [0, %d)" % (g, a, numAtoms))
                if labels[a] != -1:
                    raise OpenMMException("labelsFromGroups: atom %d is listed twice (groups %d and %d): the groups must be disjoint" % (a, labels[a], g))
                labels[a] = g
        return labels

    def _groupPairBatch(self, labels, numGroups):
        lab = np.ascontiguousarray(np.asarray(labels).reshape(-1), dtype=np.int32)
        if lab.shape[0] != self.numParticles:
            raise OpenMMException("group-pair energies: one label per atom (%d), -1 for atoms in no group" % self.numParticles)
        G = int(numGroups) if numGroups is not None else int(lab.max()) + 1 if lab.size else 0
        if G < 1:
            raise OpenMMException("group-pair energies: at least one group")
        b = _capi.SnbGroupPairBatch()
        b.n_groups = G; b.group_of_atom = _ip(lab)
        return b, lab      # (the array the batch points into: the caller keeps it until the call has returned)

    def computeGroupPairEnergies(self, context, labels, numGroups=None, devicePointer=None):
        """Group-pair interaction energy matrix at the context's positions, box and parameters (include/snb.h,
        snb_evaluate_group_pair_energies with positions == NULL): labels[i] in -1, 0 .. G - 1 is the group of atom i (-1: none; the
        labelling is the call's own, independent of the force's subsets), the result (G (G + 1) / 2, 2) holds the raw Coulomb and vdW
        energy of the atom pairs with labels {g, h} in row groupPairIndex(g, h) -- groupPairMatrix gives the symmetric (G, G, 2).  DIRECT
        SPACE ONLY: pairs inside the cutoff, Ewald exclusion corrections and 1-4 exceptions; with PME / LJPME / Ewald that is the
        short-range part (the reciprocal sum, the self term, the background and the dispersion correction are not attributed to group
        pairs), which is why every method is served.  numGroups: G (default: the largest label + 1; at most 4096).  devicePointer: address
        of a double [G (G + 1) / 2][2] array on the engine's device that takes the result (complete in stream order); then None is returned."""
        self._push_state(context)
        b, keep = self._groupPairBatch(labels, numGroups)
        b.n_frames = 1
        out = None
        if devicePointer is not None:
            b.pair_energies = ctypes.c_void_p(int(devicePointer)); b.out_is_device = 1
        else:
            out = np.zeros((b.n_groups * (b.n_groups + 1) // 2, 2))
            b.pair_energies = out.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        self._check(self._lib.snb_evaluate_group_pair_energies(self._h, ctypes.byref(b)))
        return out

    def computeGroupPairEnergiesForFrames(self, context, labels, positions=None, boxes=None, numGroups=None, positionsDevicePointer=None, numFrames=None,
                                          devicePointer=None):
        """The group-pair matrix [F][G (G + 1) / 2][2] of F stored frames in one call (include/snb.h, snb_evaluate_group_pair_energies): a
        contact-energy map or residue-residue interaction network over a trajectory -- the frame pipeline of computeSliceEnergiesForFrames
        with the group-pair pass as its step.  Direct space only, as computeGroupPairEnergies.  labels, numGroups: as there.  positions,
        boxes, positionsDevicePointer, numFrames: as in computeSliceEnergiesForFrames.  devicePointer: address of a double
        [F][G (G + 1) / 2][2] array on the engine's device that takes the result (complete in stream order); then None is returned.
        Parameters are pushed from the context first; the context's own positions, the forces and the slice energies of the last steps
        stay as they are."""
        self._push_frame_state(context)
        b, keep = self._groupPairBatch(labels, numGroups)
        if positions is None and positionsDevicePointer is None:
            raise OpenMMException("computeGroupPairEnergiesForFrames: positions or positionsDevicePointer must be given (computeGroupPairEnergies evaluates the context's own state)")
        F, frames = self._frames_into(b, "computeGroupPairEnergiesForFrames", positions, boxes, positionsDevicePointer, numFrames)
        out = None
        if devicePointer is not None:
            b.pair_energies = ctypes.c_void_p(int(devicePointer)); b.out_is_device = 1
        else:
            out = np.zeros((F, b.n_groups * (b.n_groups + 1) // 2, 2))
            b.pair_energies = out.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        self._check(self._lib.snb_evaluate_group_pair_energies(self._h, ctypes.byref(b)))
        return out

    def _groupForceOutputs(self, b, F, lambdaStates, keep):
        """Host outputs of a group-force batch: rows (F, G, n_subsets, 2, 3) and, with lambdaStates [K][S][2], stateForces (F, K, G, 3)."""
        rows = np.zeros((F, b.n_groups, self.numSubsets, 2, 3))
        b.group_forces = rows.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        states = None
        if lambdaStates is not None:
            lam = np.ascontiguousarray(np.asarray(lambdaStates, dtype=np.float64).reshape(-1, self.numSlices, 2))
            keep.append(lam)
            states = np.zeros((F, lam.shape[0], b.n_groups, 3))
            b.n_states = lam.shape[0]; b.state_lambdas = _dp(lam); b.state_forces = states.ctypes.data_as(ctypes.c_void_p)
        return rows, states

    def computeGroupForces(self, context, groups, includeDirect=True, includeReciprocal=True, lambdaStates=None, devicePointer=None):
        """Per-group forces by partner subset and term at the context's positions, box and parameters (include/snb.h,
        snb_evaluate_group_forces with positions == NULL): the table of computeAtomForces summed over each list of atom indices in
        ``groups`` on the device, (G, n_subsets, 2, 3) -- what groupAtomForces(computeAtomForces(...), groups) gives, without the per-atom
        table crossing to the host.  lambdaStates [K][S][2]: then the result is (rows, stateForces (K, G, 3)), the net force on every group
        at every lambda state (groupForcesAtStates of the table).  devicePointer: address of a double [G][n_subsets][2][3] array on the
        engine's device that takes the rows -- with lambdaStates a pair (rows address or None, address of a double [K][G][3] array) --
        complete in stream order; then None is returned."""
        self._push_state(context)
        b, keep = self._groupBatch(groups, includeDirect, includeReciprocal, _capi.SnbGroupForceBatch)
        keep = list(keep)
        b.n_frames = 1
        if devicePointer is None:
            rows, states = self._groupForceOutputs(b, 1, lambdaStates, keep)
            self._check(self._lib.snb_evaluate_group_forces(self._h, ctypes.byref(b)))
            return rows[0] if states is None else (rows[0], states[0])
        b.out_is_device = 1
        if lambdaStates is None:
            b.group_forces = ctypes.c_void_p(int(devicePointer))
        else:
            rowsPtr, statesPtr = devicePointer
            lam = np.ascontiguousarray(np.asarray(lambdaStates, dtype=np.float64).reshape(-1, self.numSlices, 2))
            b.group_forces = ctypes.c_void_p(int(rowsPtr)) if rowsPtr is not None else None
            b.n_states = lam.shape[0]; b.state_lambdas = _dp(lam); b.state_forces = ctypes.c_void_p(int(statesPtr))
        self._check(self._lib.snb_evaluate_group_forces(self._h, ctypes.byref(b)))
        return None

    def computeGroupForcesForFrames(self, context, groups, positions=None, boxes=None, includeDirect=True, includeReciprocal=True, lambdaStates=None,
                                    positionsDevicePointer=None, numFrames=None):
        """Per-group forces [F][G][n_subsets][2][3] of F stored frames in one call (include/snb.h, snb_evaluate_group_forces): the force
        every subset puts on every coarse-grained site or ligand frame by frame -- mean-force decomposition and force matching over a
        trajectory -- through the frame pipeline of computeSliceEnergiesForFrames with the atom-force pass as its step and the sum over
        each group's atoms on the device.  groups: a list of lists of atom indices, as in groupAtomForces.  positions, boxes,
        positionsDevicePointer, numFrames: as in computeSliceEnergiesForFrames.  lambdaStates [K][S][2]: then the result is (rows,
        stateForces (F, K, G, 3)), the net force on every group at every lambda state, contracted per atom on the device.  Parameters
        are pushed from the context first; the context's own positions, the forces and the slice energies of the last steps stay as they
        are."""
        self._push_frame_state(context)
        b, keep = self._groupBatch(groups, includeDirect, includeReciprocal, _capi.SnbGroupForceBatch)
        if positions is None and positionsDevicePointer is None:
            raise OpenMMException("computeGroupForcesForFrames: positions or positionsDevicePointer must be given (computeGroupForces evaluates the context's own state)")
        F, frames = self._frames_into(b, "computeGroupForcesForFrames", positions, boxes, positionsDevicePointer, numFrames)
        rows, states = self._groupForceOutputs(b, F, lambdaStates, frames)
        self._check(self._lib.snb_evaluate_group_forces(self._h, ctypes.byref(b)))
        return rows if states is None else (rows, states)

    @staticmethod
    def groupForcesAtStates(table, subsets, groups, lambdaStates):
        """The net force (K, G, 3) on every group at every lambda state a per-atom force table implies -- the NumPy statement of
        state_forces: forcesFromAtomForces per state, then the sum over each group's atoms."""
        K = HipCalcSlicedNonbondedForceKernel
        lam = np.asarray(lambdaStates, dtype=np.float64)
        out = np.zeros((lam.shape[0], len(groups), 3))
        for k in range(lam.shape[0]):
            out[k] = K.groupAtomEnergies(K.forcesFromAtomForces(table, subsets, lam[k]), groups)
        return out

    # -- per-slice virial tensors (include/snb.h, snb_evaluate_slice_virials) ------------------------
    def _virialOutputs(self, b, F, lambdaStates, keep):
        """Host outputs of a virial batch: rows (F, S, 2, 6) and, with lambdaStates [K][S][2], stateVirials (F, K, 6)."""
        rows = np.zeros((F, self.numSlices, 2, 6))
        b.slice_virials = rows.ctypes.data_as(ctypes.c_void_p); b.out_is_device = 0
        states = None
        if lambdaStates is not None:
            lam = np.ascontiguousarray(np.asarray(lambdaStates, dtype=np.float64).reshape(-1, self.numSlices, 2))
            keep.append(lam)
            states = np.zeros((F, lam.shape[0], 6))
            b.n_states = lam.shape[0]; b.state_lambdas = _dp(lam); b.state_virials = states.ctypes.data_as(ctypes.c_void_p)
        return rows, states

    def computeSliceVirials(self, context, includeDirect=True, includeReciprocal=True, lambdaStates=None, devicePointer=None):
        """Per-slice virial tensors at the context's positions, box and parameters (include/snb.h, snb_evaluate_slice_virials with
        positions == NULL): ``W[s][t][c] = -dE_raw[s][t]/d eps_c`` under a homogeneous deformation of the box and of every atom, (S, 2, 6)
        with t = (Coulomb, vdW) and c over xx, yy, zz, xy, xz, yz, in kJ/mol -- the internal virial of the pressure tensor, by slice and
        term, from one evaluation.  Not scaled by the lambdas.  lambdaStates [K][S][2]: then the result is (rows, stateVirials (K, 6)),
        the virial at every lambda state (virialsAtStates of the rows).  devicePointer: address of a double [S][2][6] array on the
        engine's device that takes the rows -- with lambdaStates a pair (rows address or None, address of a double [K][6] array) --
        complete in stream order; then None is returned.  Forces, force outputs and the slice energies of the last steps stay as they
        are.  See virialMatrix and pressureFromVirial."""
        self._push_state(context)
        b = _capi.SnbVirialBatch()
        b.n_frames = 1; b.include_direct = int(bool(includeDirect)); b.include_reciprocal = int(bool(includeReciprocal))
        keep = []
        if devicePointer is None:
            rows, states = self._virialOutputs(b, 1, lambdaStates, keep)
            self._check(self._lib.snb_evaluate_slice_virials(self._h, ctypes.byref(b)))
            return rows[0] if states is None else (rows[0], states[0])
        b.out_is_device = 1
        if lambdaStates is None:
            b.slice_virials = ctypes.c_void_p(int(devicePointer))
        else:
            rowsPtr, statesPtr = devicePointer
            lam = np.ascontiguousarray(np.asarray(lambdaStates, dtype=np.float64).reshape(-1, self.numSlices, 2))
            b.slice_virials = ctypes.c_void_p(int(rowsPtr)) if rowsPtr is not None else None
            b.n_states = lam.shape[0]; b.state_lambdas = _dp(lam); b.state_virials = ctypes.c_void_p(int(statesPtr))
        self._check(self._lib.snb_evaluate_slice_virials(self._h, ctypes.byref(b)))
        return None

    def computeSliceVirialsForFrames(self, context, positions=None, boxes=None, includeDirect=True, includeReciprocal=True, lambdaStates=None,
                                     positionsDevicePointer=None, numFrames=None):
        """Per-slice virial tensors [F][S][2][6] of F stored frames in one call (include/snb.h, snb_evaluate_slice_virials): the pressure
        tensor of a trajectory by slice and term -- surface tensions, osmotic pressures, stress autocorrelations, the pressure at every
        alchemical state -- through the frame pipeline of computeSliceEnergiesForFrames.  positions, boxes, positionsDevicePointer,
        numFrames: as in computeSliceEnergiesForFrames.  lambdaStates [K][S][2]: then the result is (rows, stateVirials (F, K, 6)),
        contracted on the device.  Parameters are pushed from the context first; the context's own positions, the forces and the slice
        energies of the last steps stay as they are."""
        self._push_frame_state(context)
        b = _capi.SnbVirialBatch()
        b.include_direct = int(bool(includeDirect)); b.include_reciprocal = int(bool(includeReciprocal))
        if positions is None and positionsDevicePointer is None:
            raise OpenMMException("computeSliceVirialsForFrames: positions or positionsDevicePointer must be given (computeSliceVirials evaluates the context's own state)")
        F, keep = self._frames_into(b, "computeSliceVirialsForFrames", positions, boxes, positionsDevicePointer, numFrames)
        rows, states = self._virialOutputs(b, F, lambdaStates, keep)
        self._check(self._lib.snb_evaluate_slice_virials(self._h, ctypes.byref(b)))
        return rows if states is None else (rows, states)

    @staticmethod
    def virialMatrix(rows):
        """Virial rows [..., 6] (xx, yy, zz, xy, xz, yz) as symmetric matrices [..., 3, 3]."""
        return virialMatrix(rows)

    @staticmethod
    def virialsAtStates(rows, lambdaStates):
        """The virial [..., K, 6] the rows [..., S, 2, 6] imply at the lambda states [K][S][2] -- the NumPy statement of state_virials."""
        return virialsAtStates(rows, lambdaStates)

    @staticmethod
    def pressureFromVirial(virial, volume, kinetic=None):
        """See the module-level pressureFromVirial."""
        return pressureFromVirial(virial, volume, kinetic)

    def getFrameStats(self):
        st = _capi.SnbFrameStats()
        self._check(self._lib.snb_get_frame_stats(self._h, ctypes.byref(st)))
        return st

    # -- CalcSlicedNonbondedForceKernel::copyParametersToContext (NonbondedSlicingKernels.h:66) ------
    def copyParametersToContext(self, context, force):
        if force.getNumParticles() != self.numParticles:
            raise OpenMMException("updateParametersInContext: The number of particles has changed")
        old14 = int(((self._excBase[:, 0] != 0) | (self._excBase[:, 2] != 0) | (self._force14[:len(self._excBase)] != 0)).sum()) if len(self._excBase) else 0
        m = force.getNumExceptions()
        if m != self._excPairs.shape[0]:
            raise OpenMMException("updateParametersInContext: The number of non-excluded exceptions has changed")
        self._upload_definition(force)
        new14 = int(((self._excBase[:, 0] != 0) | (self._excBase[:, 2] != 0) | (self._force14[:len(self._excBase)] != 0)).sum()) if len(self._excBase) else 0
        if new14 != old14:
            raise OpenMMException("updateParametersInContext: The number of non-excluded exceptions has changed")

    def getPMEParameters(self):
        a = ctypes.c_double(); g = (ctypes.c_int32 * 3)()
        self._check(self._lib.snb_get_pme_parameters(self._h, ctypes.byref(a), g))
        return a.value, g[0], g[1], g[2]

    def getLJPMEParameters(self):
        a = ctypes.c_double(); g = (ctypes.c_int32 * 3)()
        self._check(self._lib.snb_get_ljpme_parameters(self._h, ctypes.byref(a), g))
        return a.value, g[0], g[1], g[2]

    def getStats(self):
        st = _capi.SnbStats()
        self._check(self._lib.snb_get_stats(self._h, ctypes.byref(st)))
        return st


class SlicedNonbondedForceImpl:
    """openmmapi/src/SlicedNonbondedForceImpl.cpp:33-142."""

    def __init__(self, owner, kernelFactory):
        self.owner = owner
        self.kernel = kernelFactory()

    def initialize(self, context):
        owner = self.owner; system = context.getSystem()
        if owner.getNumParticles() != system.getNumParticles():
            raise OpenMMException("SlicedNonbondedForce must have exactly as many particles as the System it belongs to.")
        if owner.getUseSwitchingFunction():
            if owner.getSwitchingDistance() < 0 or owner.getSwitchingDistance() >= owner.getCutoffDistance():
                raise OpenMMException("SlicedNonbondedForce: Switching distance must satisfy 0 <= r_switch < r_cutoff")
        for i in range(owner.getNumParticles()):
            _, sigma, epsilon = owner.getParticleParameters(i)
            if sigma < 0: raise OpenMMException("SlicedNonbondedForce: sigma for a particle cannot be negative")
            if epsilon < 0: raise OpenMMException("SlicedNonbondedForce: epsilon for a particle cannot be negative")
        seen = set()
        for i in range(owner.getNumExceptions()):
            p1, p2, _, sigma, epsilon = owner.getExceptionParameters(i)
            for p in (p1, p2):
                if p < 0 or p >= owner.getNumParticles():
                    raise OpenMMException("SlicedNonbondedForce: Illegal particle index for an exception: %d" % p)
            if (min(p1, p2), max(p1, p2)) in seen:
                raise OpenMMException("SlicedNonbondedForce: Multiple exceptions are specified for particles %d and %d" % (p1, p2))
            seen.add((min(p1, p2), max(p1, p2)))
            if sigma < 0: raise OpenMMException("SlicedNonbondedForce: sigma for an exception cannot be negative")
            if epsilon < 0: raise OpenMMException("SlicedNonbondedForce: epsilon for an exception cannot be negative")
        for i in range(owner.getNumParticleParameterOffsets()):
            idx = owner.getParticleParameterOffset(i)[1]
            if idx < 0 or idx >= owner.getNumParticles():
                raise OpenMMException("SlicedNonbondedForce: Illegal particle index for a particle parameter offset: %d" % idx)
        for i in range(owner.getNumExceptionParameterOffsets()):
            idx = owner.getExceptionParameterOffset(i)[1]
            if idx < 0 or idx >= owner.getNumExceptions():
                raise OpenMMException("SlicedNonbondedForce: Illegal exception index for an exception parameter offset: %d" % idx)
        method = owner.getNonbondedMethod()
        if method not in (SlicedNonbondedForce.NoCutoff, SlicedNonbondedForce.CutoffNonPeriodic):
            box = system.getDefaultPeriodicBoxVectors()
            cutoff = owner.getCutoffDistance()
            if cutoff > 0.5 * box[0][0] or cutoff > 0.5 * box[1][1] or cutoff > 0.5 * box[2][2]:
                raise OpenMMException("SlicedNonbondedForce: The cutoff distance cannot be greater than half the periodic box size.")
            if method == SlicedNonbondedForce.Ewald and (box[1][0] != 0.0 or box[2][0] != 0.0 or box[2][1] != 0):
                raise OpenMMException("SlicedNonbondedForce: Ewald is not supported with non-rectangular boxes.  Use PME instead.")
        offsetParams = set(owner.getParticleParameterOffset(i)[0] for i in range(owner.getNumParticleParameterOffsets()))
        offsetParams |= set(owner.getExceptionParameterOffset(i)[0] for i in range(owner.getNumExceptionParameterOffsets()))
        for i in range(owner.getNumScalingParameters()):
            if owner.getScalingParameter(i)[0] in offsetParams:
                raise OpenMMException("SlicedNonbondedForce: Cannot use a global parameter for both slice energy scaling and parameter offset.")
        self.kernel.initialize(system, owner)

    def calcForcesAndEnergy(self, context, includeForces, includeEnergy, groups):
        owner = self.owner
        includeDirect = owner.getIncludeDirectSpace() and (groups & (1 << owner.getForceGroup())) != 0
        reciprocalGroup = owner.getReciprocalSpaceForceGroup()
        if reciprocalGroup < 0:
            reciprocalGroup = owner.getForceGroup()
        includeReciprocal = (groups & (1 << reciprocalGroup)) != 0
        return self.kernel.execute(context, includeForces, includeEnergy, includeDirect, includeReciprocal)

    def getDefaultParameters(self):
        return {self.owner.getGlobalParameterName(i): self.owner.getGlobalParameterDefaultValue(i) for i in range(self.owner.getNumGlobalParameters())}

    def updateParametersInContext(self, context):
        self.kernel.copyParametersToContext(context, self.owner)

    def getAtomEnergies(self, context, **options):
        return self.kernel.computeAtomEnergies(context, **options)

    def getAtomForces(self, context, **options):
        return self.kernel.computeAtomForces(context, **options)

    def getGroupEnergies(self, context, groups, **options):
        return self.kernel.computeGroupEnergies(context, groups, **options)

    def getGroupForces(self, context, groups, **options):
        return self.kernel.computeGroupForces(context, groups, **options)

    def getGroupPairEnergies(self, context, labels, **options):
        return self.kernel.computeGroupPairEnergies(context, labels, **options)

    def getSliceVirials(self, context, **options):
        return self.kernel.computeSliceVirials(context, **options)


class System:
    def __init__(self):
        self._masses = []
        self._box = np.diag([2.0, 2.0, 2.0]).astype(float)
        self._forces = []

    def addParticle(self, mass): self._masses.append(float(mass)); return len(self._masses) - 1
    def getNumParticles(self): return len(self._masses)
    def setDefaultPeriodicBoxVectors(self, a, b, c): self._box = np.array([a, b, c], dtype=float)
    def getDefaultPeriodicBoxVectors(self): return self._box.copy()
    def addForce(self, force): self._forces.append(force); return len(self._forces) - 1
    def getNumForces(self): return len(self._forces)
    def getForce(self, i): return self._forces[i]
    def usesPeriodicBoundaryConditions(self): return any(f.usesPeriodicBoundaryConditions() for f in self._forces)


class State:
    def __init__(self, energy, forces, derivs, params):
        self._e, self._f, self._d, self._p = energy, forces, derivs, params

    def getPotentialEnergy(self): return self._e
    def getForces(self): return self._f
    def getEnergyParameterDerivatives(self): return dict(self._d)
    def getParameters(self): return dict(self._p)


class Context:
    """The slice of OpenMM's Context/ContextImpl the kernel boundary talks to."""

    def __init__(self, system, precision="single", device=0, **kernelOptions):
        self._system = system
        self._kernelFactory = lambda: HipCalcSlicedNonbondedForceKernel(precision=precision, device=device, **kernelOptions)
        self._box = system.getDefaultPeriodicBoxVectors()
        self._positions = None
        self._parameters = {}
        self._energyParamDerivs = {}
        self._build()

    def _build(self):
        self._impls = []
        for f in self._system._forces:
            impl = SlicedNonbondedForceImpl(f, self._kernelFactory)
            for k, v in impl.getDefaultParameters().items():
                self._parameters.setdefault(k, v)
            self._impls.append(impl)
        for impl in self._impls:
            impl.initialize(self)

    def getSystem(self): return self._system
    def getParameters(self): return dict(self._parameters)
    def getParameter(self, name): return self._parameters[name]
    def setParameter(self, name, value):
        if name not in self._parameters:
            raise OpenMMException("Called setParameter() with invalid parameter name: " + name)
        self._parameters[name] = float(value)
    def setPositions(self, positions):
        p = np.ascontiguousarray(positions, dtype=np.float64).reshape(-1, 3)
        if p.shape[0] != self._system.getNumParticles():
            raise OpenMMException("Called setPositions() on a Context with the wrong number of positions")
        self._positions = p
    def setPeriodicBoxVectors(self, a, b, c): self._box = np.array([a, b, c], dtype=float)
    def getPeriodicBoxVectors(self): return self._box.copy()

    def reinitialize(self, preserveState=False):
        pos, params = self._positions, dict(self._parameters)
        self._parameters = {}
        self._box = self._system.getDefaultPeriodicBoxVectors() if not preserveState else self._box
        self._build()
        if preserveState:
            self._positions = pos
            for k, v in params.items():
                if k in self._parameters:
                    self._parameters[k] = v
        else:
            self._positions = None

    def getState(self, getEnergy=False, getForces=False, getParameterDerivatives=False, groups=0xFFFFFFFF):
        if self._positions is None:
            raise OpenMMException("Particle positions have not been set")
        n = self._system.getNumParticles()
        self._forces = np.zeros((n, 3))
        self._energyParamDerivs = {}
        energy = 0.0
        for impl in self._impls:
            energy += impl.calcForcesAndEnergy(self, getForces, getEnergy or getParameterDerivatives, groups)
        return State(energy, self._forces.copy(), self._energyParamDerivs, self._parameters)

    def getAtomEnergies(self, force, **options):
        """Per-atom interaction energies of ``force`` with every subset, (N, n_subsets, 2): HipCalcSlicedNonbondedForceKernel.computeAtomEnergies."""
        if self._positions is None:
            raise OpenMMException("Particle positions have not been set")
        for impl in self._impls:
            if impl.owner is force:
                return impl.getAtomEnergies(self, **options)
        raise OpenMMException("force not in this context")

    def getGroupEnergies(self, force, groups, **options):
        """Per-group interaction energies of ``force`` with every subset, (G, n_subsets, 2): HipCalcSlicedNonbondedForceKernel.computeGroupEnergies."""
        if self._positions is None:
            raise OpenMMException("Particle positions have not been set")
        for impl in self._impls:
            if impl.owner is force:
                return impl.getGroupEnergies(self, groups, **options)
        raise OpenMMException("force not in this context")

    def getGroupForces(self, force, groups, **options):
        """Per-group forces of ``force`` by partner subset and term, (G, n_subsets, 2, 3), with lambdaStates also (K, G, 3):
        HipCalcSlicedNonbondedForceKernel.computeGroupForces."""
        if self._positions is None:
            raise OpenMMException("Particle positions have not been set")
        for impl in self._impls:
            if impl.owner is force:
                return impl.getGroupForces(self, groups, **options)
        raise OpenMMException("force not in this context")

    def getGroupPairEnergies(self, force, labels, **options):
        """Group-pair interaction energy matrix of ``force`` (direct space), (G (G + 1) / 2, 2) for the labelling ``labels``:
        HipCalcSlicedNonbondedForceKernel.computeGroupPairEnergies."""
        if self._positions is None:
            raise OpenMMException("Particle positions have not been set")
        for impl in self._impls:
            if impl.owner is force:
                return impl.getGroupPairEnergies(self, labels, **options)
        raise OpenMMException("force not in this context")

    def getSliceVirials(self, force, **options):
        """Per-slice virial tensors of ``force``, (S, 2, 6) over xx, yy, zz, xy, xz, yz, with lambdaStates also (K, 6):
        HipCalcSlicedNonbondedForceKernel.computeSliceVirials."""
        if self._positions is None:
            raise OpenMMException("Particle positions have not been set")
        for impl in self._impls:
            if impl.owner is force:
                return impl.getSliceVirials(self, **options)
        raise OpenMMException("force not in this context")

    def getAtomForces(self, force, **options):
        """Per-atom forces of ``force`` by partner subset and term, (N, n_subsets, 2, 3): HipCalcSlicedNonbondedForceKernel.computeAtomForces."""
        if self._positions is None:
            raise OpenMMException("Particle positions have not been set")
        for impl in self._impls:
            if impl.owner is force:
                return impl.getAtomForces(self, **options)
        raise OpenMMException("force not in this context")

    def _updateParametersInContext(self, force):
        for impl in self._impls:
            if impl.owner is force:
                impl.updateParametersInContext(self)

    def _kernelFor(self, force):
        for impl in self._impls:
            if impl.owner is force:
                return impl.kernel
        raise OpenMMException("force not in this context")
