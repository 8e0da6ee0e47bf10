// atomenergy.hip -- per-atom interaction energies with every subset (snb_evaluate_atom_energies).
//
// A[i][J][t] = raw energy (t = 0 Coulomb, 1 vdW) of atom i with all atoms of subset J.  The kernels here fill a table
// double [Npad][nsub][2] over the SORTED atom index; the finish kernel adds the closed-form terms and writes the caller's
// table in user order.  Analysis kernels beside the step kernels: they share the lists, the tiles and the parameter structs of
// direct.hip / pme.hip and the energy expressions of the energy-only kernels, and write nothing a step reads.
//
//   PairEnergy                      what a tile pair, a 1-4 exception and an Ewald exclusion correction add to the table (pair_energy.h: shared
//                                   with the group-pair matrix).  The walkers that call it are shared with the force table and live in atom_table.h:
//   k_atomTiles<.., PairEnergy>     the tiles of the pair kernel and, in its first work-groups, the two pair lists; the j-side LDS region is [32][2];
//   k_atomStencil<.., GRAD = false> q_i psi_J(r_i) for every held mesh J from the UNMIXED potentials: the value part of the interpolation.
//   k_atomFinish     twice the Ewald self terms into column s_i, the neutralising background -2 c q_i Q_J, sorted -> user order.
//   k_groupSums      the same completed rows summed over lists of user atoms (snb_evaluate_group_energies): short
//   k_groupCombine   lists one thread per (group, subset), long lists one wave per chunk and a second launch that adds a group's chunks
//                    in list order -- no atomics, so a group's row is a function of the working table alone.
#include "atom_table.h"
#include "pair_energy.h"
#include <algorithm>
#include <vector>

namespace snb {

template <typename Real> void launchAtomPairs(const DirectParams<Real>& p, int mc, bool wrap, const PairListParams<Real>* lists, double* tab, hipStream_t s) { launchAtomTiles<Real, PairEnergy>(p, mc, wrap, lists, tab, s); }
template void launchAtomPairs<float>(const DirectParams<float>&, int, bool, const PairListParams<float>*, double*, hipStream_t);
template void launchAtomPairs<double>(const DirectParams<double>&, int, bool, const PairListParams<double>*, double*, hipStream_t);

template <typename Real> void launchAtomPotential(const PmeParams<Real>& p, double* tab, hipStream_t s) { launchAtomStencil<Real, false>(p, tab, s); }
template void launchAtomPotential<float>(const PmeParams<float>&, double*, hipStream_t);
template void launchAtomPotential<double>(const PmeParams<double>&, double*, hipStream_t);

// ---- finish ------------------------------------------------------------------------------------------------------------------------
// Entry (a, J) of the sorted-order working table, completed: the sum rule halves the diagonal column, so the self terms enter twice; the
// background -2 c q_i Q_J sums to the slice's c Q_I Q_J (x 2 off the diagonal) of sliceFinishClosedForm.
template <typename Real>
__device__ __forceinline__ void atomRowEntry(const double* __restrict__ tab, const int a, const int J, const int nsub, const int* __restrict__ blockSubset,
                                             const typename Vec<Real>::T4* __restrict__ posq, const typename Vec<Real>::T2* __restrict__ sigeps, const SliceFinish& f,
                                             double& e0, double& e1) {
    const double* e = tab + ((size_t)a * nsub + J) * 2;
    e0 = e[0]; e1 = e[1];
    if (f.sums) {
        const double q = (double)posq[a].w;
        e0 += 2.0 * f.background * q * f.sums[3 * J];
        if (blockSubset[a >> 5] == J) {
            const auto se = sigeps[a];
            const double hs = (double)se.x, c6 = 8.0 * hs * hs * hs * (double)se.y;
            e0 += 2.0 * f.selfCoulomb * q * q;
            e1 += 2.0 * f.selfDispersion * c6 * c6;
        }
    }
}
// One thread per (user atom, subset): closed-form terms, sorted -> user order.
template <typename Real>
__global__ __launch_bounds__(256) void k_atomFinish(const double* __restrict__ tab, const int* __restrict__ userToSorted, const int* __restrict__ blockSubset,
                                                    const typename Vec<Real>::T4* __restrict__ posq, const typename Vec<Real>::T2* __restrict__ sigeps,
                                                    const int nAtoms, const int nsub, const SliceFinish f, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)nAtoms * nsub) return;
    const int u = (int)(t / nsub), J = (int)(t - (long long)u * nsub);
    double e0, e1;
    atomRowEntry<Real>(tab, userToSorted[u], J, nsub, blockSubset, posq, sigeps, f, e0, e1);
    out[2 * t] = e0; out[2 * t + 1] = e1;
}
template <typename Real>
void launchAtomFinish(const double* tab, const int* userToSorted, const int* blockSubset, const typename Vec<Real>::T4* posq, const typename Vec<Real>::T2* sigeps,
                      int nAtoms, int nsub, const SliceFinish& f, double* out, hipStream_t s) {
    const long long n = (long long)nAtoms * nsub;
    if (n <= 0) return;
    hipLaunchKernelGGL((k_atomFinish<Real>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tab, userToSorted, blockSubset, posq, sigeps, nAtoms, nsub, f, out);
}
template void launchAtomFinish<float>(const double*, const int*, const int*, const Vec<float>::T4*, const Vec<float>::T2*, int, int, const SliceFinish&, double*, hipStream_t);
template void launchAtomFinish<double>(const double*, const int*, const int*, const Vec<double>::T4*, const Vec<double>::T2*, int, int, const SliceFinish&, double*, hipStream_t);

// ---- groups ------------------------------------------------------------------------------------------------------------------------
// Rows of the completed table summed over lists of USER atom indices (CSR: start[G + 1], atoms[start[G]]; lists may overlap, repeat an index,
// be empty).  The mapping follows the list's length (planGroups):
//   up to SNB_GROUP_SERIAL atoms   one THREAD per (group, subset) walks the list -- a three-atom water costs nsub lanes, not a wave;
//   longer                         chunks of max(256, length / 256 rounded up to 64) atoms, one WAVE per chunk: lanes stride the chunk, a fixed
//                                  butterfly adds the 64 partial sums, lane 0 stores the chunk's row; k_groupCombine then adds a group's
//                                  chunks (256 at the most) in list order.  "The protein" spreads over as many waves as it has chunks.
// Both kinds run in one launch (the first nSmallBlocks work-groups take the short lists).  Every entry of out[G][nsub][2] is written once.
void planGroups(int nGroups, const int32_t* start, GroupPlan& plan) {
    plan.nGroups = nGroups; plan.nSmall = plan.nChunks = plan.nLarge = 0;
    const int nIdx = start[nGroups];
    std::vector<int> small, chunks, large;
    for (int g = 0; g < nGroups; g++) {
        const int b = start[g], len = start[g + 1] - b;
        if (len <= SNB_GROUP_SERIAL) { small.push_back(g); continue; }
        const int clen = std::max(256, ((len + 255) / 256 + 63) / 64 * 64);
        const int first = (int)chunks.size() / 4;
        for (int c = b; c < b + len; c += clen) { chunks.push_back(g); chunks.push_back(c); chunks.push_back(std::min(c + clen, b + len)); chunks.push_back(0); }
        large.push_back(g); large.push_back(first); large.push_back((int)chunks.size() / 4 - first); large.push_back(0);
    }
    plan.nSmall = (int)small.size(); plan.nChunks = (int)chunks.size() / 4; plan.nLarge = (int)large.size() / 4;
    auto align4 = [](size_t n) { return (n + 3) / 4 * 4; };
    plan.offStart = 0; plan.offAtoms = (int)align4(nGroups + 1); plan.offSmall = (int)align4(plan.offAtoms + (size_t)nIdx);
    plan.offChunks = (int)align4(plan.offSmall + small.size()); plan.offLarge = plan.offChunks + (int)chunks.size();
    plan.packed.assign(plan.offLarge + large.size(), 0);
    std::copy(start, start + nGroups + 1, plan.packed.begin());
    std::copy(small.begin(), small.end(), plan.packed.begin() + plan.offSmall);
    std::copy(chunks.begin(), chunks.end(), plan.packed.begin() + plan.offChunks);
    std::copy(large.begin(), large.end(), plan.packed.begin() + plan.offLarge);
}

template <typename Real>
__global__ __launch_bounds__(256) void k_groupSums(const double* __restrict__ tab, const int* __restrict__ userToSorted, const int* __restrict__ blockSubset,
                                                   const typename Vec<Real>::T4* __restrict__ posq, const typename Vec<Real>::T2* __restrict__ sigeps, const int nsub, const SliceFinish f,
                                                   const int* __restrict__ start, const int* __restrict__ atoms, const int* __restrict__ small, const int nSmall, const int nSmallBlocks,
                                                   const int4* __restrict__ chunks, const int nChunks, double* __restrict__ partial, double* __restrict__ out) {
    if ((int)blockIdx.x < nSmallBlocks) {
        const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
        if (t >= (long long)nSmall * nsub) return;
        const int k = (int)(t / nsub), J = (int)(t - (long long)k * nsub);
        const int g = small[k];
        double s0 = 0, s1 = 0;
        for (int e = start[g], eEnd = start[g + 1]; e < eEnd; e++) {
            double e0, e1;
            atomRowEntry<Real>(tab, userToSorted[atoms[e]], J, nsub, blockSubset, posq, sigeps, f, e0, e1);
            s0 += e0; s1 += e1;
        }
        double* const o = out + ((size_t)g * nsub + J) * 2;
        o[0] = s0; o[1] = s1;
        return;
    }
    const int c = ((int)blockIdx.x - nSmallBlocks) * 4 + (int)(threadIdx.x >> 6);      // (uniform over the wave)
    if (c >= nChunks) return;
    const int lane = threadIdx.x & 63;
    const int4 ch = chunks[c];
    for (int J = 0; J < nsub; J++) {
        double s0 = 0, s1 = 0;
        for (int e = ch.y + lane; e < ch.z; e += 64) {
            double e0, e1;
            atomRowEntry<Real>(tab, userToSorted[atoms[e]], J, nsub, blockSubset, posq, sigeps, f, e0, e1);
            s0 += e0; s1 += e1;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { s0 += __shfl_xor(s0, o, 64); s1 += __shfl_xor(s1, o, 64); }
        if (lane == 0) { double* const o = partial + ((size_t)c * nsub + J) * 2; o[0] = s0; o[1] = s1; }
    }
}
// one thread per (long group, subset, term): its chunks' rows in list order
__global__ __launch_bounds__(256) void k_groupCombine(const int4* __restrict__ large, const int nLarge, const int nsub, const double* __restrict__ partial, double* __restrict__ out) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int row = 2 * nsub;
    if (t >= (long long)nLarge * row) return;
    const int k = (int)(t / row), i = (int)(t - (long long)k * row);
    const int4 lg = large[k];
    double s = 0;
    for (int c = lg.y; c < lg.y + lg.z; c++) s += partial[(size_t)c * row + i];
    out[(size_t)lg.x * row + i] = s;
}
template <typename Real>
void launchGroupFinish(const double* tab, const int* userToSorted, const int* blockSubset, const typename Vec<Real>::T4* posq, const typename Vec<Real>::T2* sigeps, int nsub,
                       const SliceFinish& f, const GroupPlan& plan, const int* packed, double* partial, double* out, hipStream_t s) {
    const int nSmallBlocks = (int)(((long long)plan.nSmall * nsub + 255) / 256), nChunkBlocks = (plan.nChunks + 3) / 4;
    if (nSmallBlocks + nChunkBlocks <= 0) return;
    const int4* const chunks = reinterpret_cast<const int4*>(packed + plan.offChunks);
    const int4* const large = reinterpret_cast<const int4*>(packed + plan.offLarge);
    hipLaunchKernelGGL((k_groupSums<Real>), dim3(nSmallBlocks + nChunkBlocks), dim3(256), 0, s, tab, userToSorted, blockSubset, posq, sigeps, nsub, f, packed + plan.offStart,
                       packed + plan.offAtoms, packed + plan.offSmall, plan.nSmall, nSmallBlocks, chunks, plan.nChunks, partial, out);
    if (plan.nLarge > 0) hipLaunchKernelGGL(k_groupCombine, dim3((unsigned)(((long long)plan.nLarge * 2 * nsub + 255) / 256)), dim3(256), 0, s, large, plan.nLarge, nsub, partial, out);
}
template void launchGroupFinish<float>(const double*, const int*, const int*, const Vec<float>::T4*, const Vec<float>::T2*, int, const SliceFinish&, const GroupPlan&, const int*, double*, double*, hipStream_t);
template void launchGroupFinish<double>(const double*, const int*, const int*, const Vec<double>::T4*, const Vec<double>::T2*, int, const SliceFinish&, const GroupPlan&, const int*, double*, double*, hipStream_t);

}  // namespace snb
