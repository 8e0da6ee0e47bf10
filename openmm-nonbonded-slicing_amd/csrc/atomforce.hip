// atomforce.hip -- per-atom forces by partner subset and term (snb_evaluate_atom_forces).
//
// G[i][J][t] = - d E_raw[slice(s_i, J)][t] / d r_i  (t = 0 Coulomb, 1 vdW; a 3-vector): the force all atoms of subset J put on atom i, every
// lambda 1.  The kernels here fill a table double [Npad][nsub][2][3] over the SORTED atom index; the finish kernel writes the caller's table
// in user order.  The same lists, tiles and parameter structs as the energy table (atomenergy.hip), through the same walkers (atom_table.h),
// 3-vectors where that carries scalars; nothing a step reads is written.
//
//   PairForce (pair_force.h)        what a tile pair, a 1-4 exception and an Ewald exclusion correction add to the table: the force on the
//                                   i-end; the shared walkers credit the partner's end with the sign turned (J_SIGN = -1);
//   k_atomTiles<.., PairForce>      the tiles of the pair kernel and, in its first work-groups, the two pair lists; the j-side LDS region is [32][6];
//   k_atomStencil<.., GRAD = true>  -q_i grad psi_J(r_i) for every held mesh J from the UNMIXED potentials: the derivative part of the interpolation.
//   k_atomForceFinish sorted -> user order.  (Self term, neutralising background and dispersion correction carry no force.)
//   k_groupForceSums      the table summed over lists of user atoms, by subset column and contracted per atom with lambda states
//   k_groupForceCombine   (snb_evaluate_group_forces): the mapping of k_groupSums / k_groupCombine (atomenergy.hip)
#include "atom_table.h"
#include "pair_force.h"
#include <type_traits>

namespace snb {

template <typename Real> void launchAtomForcePairs(const DirectParams<Real>& p, int mc, bool wrap, const PairListParams<Real>* lists, double* tab, hipStream_t s) { launchAtomTiles<Real, PairForce>(p, mc, wrap, lists, tab, s); }
template void launchAtomForcePairs<float>(const DirectParams<float>&, int, bool, const PairListParams<float>*, double*, hipStream_t);
template void launchAtomForcePairs<double>(const DirectParams<double>&, int, bool, const PairListParams<double>*, double*, hipStream_t);

template <typename Real> void launchAtomField(const PmeParams<Real>& p, double* tab, hipStream_t s) { launchAtomStencil<Real, true>(p, tab, s); }
template void launchAtomField<float>(const PmeParams<float>&, double*, hipStream_t);
template void launchAtomField<double>(const PmeParams<double>&, double*, hipStream_t);

// ---- finish ------------------------------------------------------------------------------------------------------------------------
// One thread per table value: sorted -> user order.  row = nsub * 6 values per atom.
__global__ __launch_bounds__(256) void k_atomForceFinish(const double* __restrict__ tab, const int* __restrict__ userToSorted, const int nAtoms, const int row, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nAtoms * row) return;
    const int u = (int)(t / row), c = (int)(t - (long long)u * row);
    out[t] = tab[(size_t)userToSorted[u] * row + c];
}
void launchAtomForceFinish(const double* tab, const int* userToSorted, int nAtoms, int nsub, double* out, hipStream_t s) {
    const long long n = (long long)nAtoms * nsub * 6;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_atomForceFinish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tab, userToSorted, nAtoms, nsub * 6, out);
}

// ---- groups ------------------------------------------------------------------------------------------------------------------------
// The table summed over lists of USER atom indices (snb_evaluate_group_forces), with the lists, the plan and the
// mapping of k_groupSums (atomenergy.hip): up to SNB_GROUP_SERIAL atoms one THREAD per (group, column), longer lists one WAVE per chunk and
// column, the fixed 64-lane butterfly, then k_groupForceCombine over a group's chunks in list order.  A column c is
//   c < nRows (nRows = nsub when the raw rows are asked for, else 0)   subset J = c: six sums, sum_i G[i][J][t][d];
//   c >= nRows                                                        lambda state k = c - nRows: three sums of the atom's row contracted
//                                                                     with lambda_k[slice(s_i, J)][t] -- per ATOM, before the group sum: s_i
//                                                                     is the atom's own subset, and a group may span subsets.
// Both kinds of column run in one launch.  A row of the table is 48-byte vectors at userToSorted addresses, 16-byte aligned: three double2 loads.
// the force on sorted atom a at lambda state lam[S][2]: its columns in order, as forcesFromAtomForces adds them
__device__ __forceinline__ void atomStateForce(const double* __restrict__ tab, const int a, const int nsub, const int* __restrict__ blockSubset, const double* __restrict__ lam,
                                               double& fx, double& fy, double& fz) {
    const int si = blockSubset[a >> 5];
    const double2* v = reinterpret_cast<const double2*>(tab + (size_t)a * nsub * 6);
    fx = 0; fy = 0; fz = 0;
    for (int J = 0; J < nsub; J++, v += 3) {
        const double2 l = *reinterpret_cast<const double2*>(lam + 2 * sliceOf(si, J));
        const double2 p = v[0], q = v[1], r = v[2];
        fx += l.x * p.x + l.y * q.y; fy += l.x * p.y + l.y * r.x; fz += l.x * q.x + l.y * r.y;
    }
}
#define SNB_BUTTERFLY(x) _Pragma("unroll") for (int o_ = 32; o_ > 0; o_ >>= 1) x += __shfl_xor(x, o_, 64)
__global__ __launch_bounds__(256) void k_groupForceSums(const double* __restrict__ tab, const int* __restrict__ userToSorted, const int* __restrict__ blockSubset, const int nsub,
                                                        const int nRows, const int nStates, const double* __restrict__ lam, const int nGroups,
                                                        const int* __restrict__ start, const int* __restrict__ atoms, const int* __restrict__ small, const int nSmall, const int nSmallBlocks,
                                                        const int4* __restrict__ chunks, const int nChunks, double* __restrict__ partial, double* __restrict__ rows, double* __restrict__ states) {
    const int nCols = nRows + nStates, nSlices = nsub * (nsub + 1) / 2;
    if ((int)blockIdx.x < nSmallBlocks) {
        const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
        if (t >= (long long)nSmall * nCols) return;
        const int k = (int)(t / nCols), c = (int)(t - (long long)k * nCols);
        const int g = small[k];
        const int eBegin = start[g], eEnd = start[g + 1];
        if (c < nRows) {
            double x0 = 0, y0 = 0, z0 = 0, x1 = 0, y1 = 0, z1 = 0;
            for (int e = eBegin; e < eEnd; e++) {
                const double2* const v = reinterpret_cast<const double2*>(tab + ((size_t)userToSorted[atoms[e]] * nsub + c) * 6);
                const double2 p = v[0], q = v[1], r = v[2];
                x0 += p.x; y0 += p.y; z0 += q.x; x1 += q.y; y1 += r.x; z1 += r.y;
            }
            double* const o = rows + ((size_t)g * nsub + c) * 6;      // rows[g][J][2][3]
            o[0] = x0; o[1] = y0; o[2] = z0; o[3] = x1; o[4] = y1; o[5] = z1;
        } else {
            const double* const l = lam + (size_t)(c - nRows) * nSlices * 2;
            double x = 0, y = 0, z = 0;
            for (int e = eBegin; e < eEnd; e++) {
                double fx, fy, fz;
                atomStateForce(tab, userToSorted[atoms[e]], nsub, blockSubset, l, fx, fy, fz);
                x += fx; y += fy; z += fz;
            }
            double* const o = states + ((size_t)(c - nRows) * nGroups + g) * 3;      // states[k][g][3]
            o[0] = x; o[1] = y; o[2] = z;
        }
        return;
    }
    const int ch = ((int)blockIdx.x - nSmallBlocks) * 4 + (int)(threadIdx.x >> 6);      // (uniform over the wave)
    if (ch >= nChunks) return;
    const int lane = threadIdx.x & 63;
    const int4 range = chunks[ch];
    double* const prow = partial + (size_t)ch * (nRows * 6 + nStates * 3);      // a chunk's partial row: [rows | states]
    for (int J = 0; J < nRows; J++) {
        double x0 = 0, y0 = 0, z0 = 0, x1 = 0, y1 = 0, z1 = 0;
        for (int e = range.y + lane; e < range.z; e += 64) {
            const double2* const v = reinterpret_cast<const double2*>(tab + ((size_t)userToSorted[atoms[e]] * nsub + J) * 6);
            const double2 p = v[0], q = v[1], r = v[2];
            x0 += p.x; y0 += p.y; z0 += q.x; x1 += q.y; y1 += r.x; z1 += r.y;
        }
        SNB_BUTTERFLY(x0); SNB_BUTTERFLY(y0); SNB_BUTTERFLY(z0); SNB_BUTTERFLY(x1); SNB_BUTTERFLY(y1); SNB_BUTTERFLY(z1);
        if (lane == 0) { double* const o = prow + J * 6; o[0] = x0; o[1] = y0; o[2] = z0; o[3] = x1; o[4] = y1; o[5] = z1; }
    }
    for (int k = 0; k < nStates; k++) {
        const double* const l = lam + (size_t)k * nSlices * 2;
        double x = 0, y = 0, z = 0;
        for (int e = range.y + lane; e < range.z; e += 64) {
            double fx, fy, fz;
            atomStateForce(tab, userToSorted[atoms[e]], nsub, blockSubset, l, fx, fy, fz);
            x += fx; y += fy; z += fz;
        }
        SNB_BUTTERFLY(x); SNB_BUTTERFLY(y); SNB_BUTTERFLY(z);
        if (lane == 0) { double* const o = prow + nRows * 6 + k * 3; o[0] = x; o[1] = y; o[2] = z; }
    }
}
#undef SNB_BUTTERFLY
// one thread per (long group, value of the partial row): its chunks' rows in list order
__global__ __launch_bounds__(256) void k_groupForceCombine(const int4* __restrict__ large, const int nLarge, const int nsub, const int nRows, const int nStates, const int nGroups,
                                                           const double* __restrict__ partial, double* __restrict__ rows, double* __restrict__ states) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int row = nRows * 6 + nStates * 3;
    if (t >= (long long)nLarge * row) return;
    const int k = (int)(t / row), i = (int)(t - (long long)k * row);
    const int4 lg = large[k];
    double s = 0;
    for (int c = lg.y; c < lg.y + lg.z; c++) s += partial[(size_t)c * row + i];
    if (i < nRows * 6) rows[(size_t)lg.x * nsub * 6 + i] = s;
    else { const int j = i - nRows * 6; states[((size_t)(j / 3) * nGroups + lg.x) * 3 + j % 3] = s; }
}
void launchGroupForceFinish(const double* tab, const int* userToSorted, const int* blockSubset, int nsub, const GroupPlan& plan, const int* packed, const double* stateLambdas, int nStates,
                            double* partial, double* rows, double* states, hipStream_t s) {
    const int nRows = rows ? nsub : 0, nCols = nRows + nStates;
    const int nSmallBlocks = (int)(((long long)plan.nSmall * nCols + 255) / 256), nChunkBlocks = (plan.nChunks + 3) / 4;
    if (nCols <= 0 || nSmallBlocks + nChunkBlocks <= 0) return;
    const int4* const chunks = reinterpret_cast<const int4*>(packed + plan.offChunks);
    const int4* const large = reinterpret_cast<const int4*>(packed + plan.offLarge);
    hipLaunchKernelGGL(k_groupForceSums, dim3(nSmallBlocks + nChunkBlocks), dim3(256), 0, s, tab, userToSorted, blockSubset, nsub, nRows, nStates, stateLambdas, plan.nGroups,
                       packed + plan.offStart, packed + plan.offAtoms, packed + plan.offSmall, plan.nSmall, nSmallBlocks, chunks, plan.nChunks, partial, rows, states);
    if (plan.nLarge > 0) {
        const long long n = (long long)plan.nLarge * (nRows * 6 + nStates * 3);
        hipLaunchKernelGGL(k_groupForceCombine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, large, plan.nLarge, nsub, nRows, nStates, plan.nGroups, partial, rows, states);
    }
}

}  // namespace snb
