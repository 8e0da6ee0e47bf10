"""The packed pair kernels with 32-bit byte offsets (direct.hip: fAddAt / loadAt, chosen by csrc/pair_addressing.h) against the oracle.

The system is the small droplet of tests/test_gpu_derivative_tiles.py (3000 atoms, four subsets by lattice site): masked and unmasked
tiles, a padded last block, work items of one tile and of eight, and free j-slots all occur.  Single and mixed precision (32-bit float and
64-bit fixed-point accumulators: 4 and 8 bytes per atom slot), once with the engine's own force arrays read back in user order and once
with a bound context-order buffer.  A forces-only step runs k_directPacked, a derivative step k_directPackedSelected; forces and
wanted-slice energies are held to the tolerances of tests/test_gpu_derivative_tiles.py.  One oracle evaluation serves every case."""
import numpy as np
import pytest

import test_gpu_context_binding as CB
import test_gpu_derivative_tiles as DT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def F(snb):
    return snb.SlicedNonbondedForce


@pytest.mark.parametrize("bound", [False, True], ids=["own_arrays", "bound_buffer"])
@pytest.mark.parametrize("prec", ["single", "mixed"])
def test_forces_and_wanted_slices_with_32_bit_offsets(prec, bound, snb, F, oracle):
    import torch
    force, pos, box = DT.droplet(F, 4)
    st = DT.Stepper(snb, force, pos, box, prec)
    o = DT.truth(lambda f, p, b, params=None: oracle.evaluate(f, np.asarray(p, dtype=float), b, params, True, True), "pme", force, pos, box, dict(st.ctx.getParameters()))
    view = None
    if bound:
        view = CB.View(pos, False, 23)
        torch.cuda.synchronize()
        st.kern.bindContextBuffers(view.posq.data_ptr(), view.atom_index.data_ptr(), view.padded, forceBuffer=view.buf.data_ptr(), posqIsDouble=False)
        st.ctx.setPositions(np.zeros((st.n, 3)))      # (the host positions are not used while bound)
    tol = DT.TOLS[prec]
    f, _ = st.step(include_energy=0)
    DT.check_forces(o["forces"], f, tol, "%s forces-only step" % prec)
    for first in (0, 1):
        mask = np.zeros(st.S, dtype=np.int32); mask[first::2] = 1
        st.wanted(mask)
        f, e = st.step()
        DT.check_forces(o["forces"], f, tol, "%s derivative step, wanted %d::2" % (prec, first))
        DT.check_slices(o["slice_energies"], e, mask, tol, "%s wanted %d::2" % (prec, first))
    if bound:
        assert st.kern._lib.snb_synchronize(st.kern._h) == 0
        DT.check_forces(3.0 * o["forces"], view.delivered(), tol, "%s bound buffer, three steps added" % prec)
        assert view.padding_untouched()
    s = st.stats()
    assert s.n_tiles > 0 and s.n_host_rebuilds == 0
