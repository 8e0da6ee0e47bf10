// grouppairs.hip -- group-pair interaction energy matrix, direct space (snb_evaluate_group_pair_energies).
//
// M[slice(g, h)][t] = raw direct-space energy (t = 0 Coulomb, 1 vdW) summed over the unordered atom pairs {i, j} whose labels are {g, h}:
// pairs inside the cutoff, Ewald exclusion corrections, 1-4 exceptions; slice(g, h) = max (max + 1) / 2 + min over the G labels of the
// call.  A pair whose either end carries label -1 adds nothing.  The pair values are PairEnergy's (pair_energy.h), the walk is that of
// k_atomTiles (atom_table.h): the same work items, tile heads, shift codes, parked padding slots, exclusion masks and rotated slot order.
// What is new is the key: a pair is added under BOTH ends' labels.
//
//   k_groupPairLabels   labelSorted[slot] = group_of_atom[sortedToUser[slot]], -1 on padding slots; per frame, after that frame's list exists.
//   k_groupPairTiles    one wave per work item, runs of 8 items per wave.  The <= 32 distinct labels of the item's i-atoms and of a tile's j-atoms are numbered by a
//                       ballot loop (waveLocalIds; -1 takes no number); a pair (i, j) belongs to cell (id_i, id_j) of a block of nI x nJ cells.
//     uniform case      nI = nJ = 1 (solvent, one big group): the lane's own registers, drained into double per item, kept across tiles
//                       AND items while the two labels stay, folded by a butterfly: one pair of global atomics per change of labels.
//     general case      per-wave LDS block of 1024 entries per term: cell c owns R = 2^k entries, the largest power of two with nI nJ R <=
//                       1024, and a lane adds into entry c R + (lane mod R): with nI nJ <= 16 every lane has an entry of its own (no
//                       collision at all); at 32 x 32 labels R = 1 and two lanes meet only when they share both labels.  The block is
//                       flushed when the tile's j-label set changes (kept across the tiles of an item while they all carry one and the
//                       same j-label): replicas folded in double by a segmented butterfly, one double atomic per non-zero cell and term.
//   list work-groups    the first work-groups of the same launch: Ewald exclusion corrections (one thread per atom; the end with the
//                       smaller sorted index adds, so a pair counts once) and 1-4 exceptions (one thread per pair).  A thread sums runs of
//                       equal key; a wave whose live lanes all hold the same key folds them first (waveKeyedAdd).
//   k_groupPairFinish   the working matrix to row f of the output.  A small matrix (G = 8: 36 rows) is kept in up to 64 copies, a work-group
//                       adding into copy blockIdx mod copies, as the slice energies of a step are (SNB_SLICE_E_PARTS): tens of thousands of
//                       waves adding into a few dozen doubles serialise in L2.  The finish adds the copies in index order.
// No kernel here adds a pair with a global atomic of its own, and none serialises when every atom carries one label.
#include "pair_energy.h"
#include <algorithm>
#include <cstring>

namespace snb {

#define SNB_GROUP_PAIR_RUN 8      // consecutive work items a wave takes at a time

__device__ __forceinline__ int groupPairSlice(const int a, const int b) { const int hi = a > b ? a : b, lo = a > b ? b : a; return hi * (hi + 1) / 2 + lo; }

__device__ __forceinline__ void waveSync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void k_groupPairLabels(const int* __restrict__ labelsUser, const int* __restrict__ sortedToUser, const int nPad, int* __restrict__ labelSorted) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nPad) return;
    const int u = sortedToUser[s];
    labelSorted[s] = u >= 0 ? labelsUser[u] : -1;
}

// Numbers the distinct non-negative values of `lab` over the 64 lanes of the wave in order of first appearance: returns the lane's own id,
// n = how many there are (0: none), first = the first of them (-1: none), leader = whether this lane is the first to hold its value.  A
// lane with lab < 0 (a padding slot, an atom in no group) takes no number: its id is -1, and it does not end a run of one label.  Every
// lane must call.
__device__ __forceinline__ int waveLocalIds(const int lab, const int lane, int& n, int& first, bool& leader) {
    unsigned long long todo = __ballot(lab >= 0);
    int id = 0, mine = -1;
    leader = false;
    first = todo ? __builtin_amdgcn_readlane(lab, __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1)) : -1;
    while (todo) {
        const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
        const int v = __builtin_amdgcn_readlane(lab, src);
        const unsigned long long same = __ballot(lab == v);
        if (lab == v) { mine = id; leader = lane == src; }
        todo &= ~same;
        id++;
    }
    n = id;
    return mine;
}

// M[key][0 .. 2) += (v0, v1) from every lane with key >= 0.  Live lanes that all hold one key are folded first: one pair of atomics per
// wave.  Every lane of the wave must call.
__device__ __forceinline__ void waveKeyedAdd(double* const M, const int key, double v0, double v1, const int lane) {
    const unsigned long long live = __ballot(key >= 0);
    if (live == 0) return;
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
    const int k0 = __builtin_amdgcn_readlane(key, src);
    if (__ballot(key >= 0 && key != k0) == 0) {
        if (key < 0) { v0 = 0; v1 = 0; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { v0 += __shfl_xor(v0, o, 64); v1 += __shfl_xor(v1, o, 64); }
        if (lane == 0) { if (v0 != 0.0) gAdd(M + 2 * (size_t)k0, v0); if (v1 != 0.0) gAdd(M + 2 * (size_t)k0 + 1, v1); }
    } else if (key >= 0) {
        if (v0 != 0.0) gAdd(M + 2 * (size_t)key, v0);
        if (v1 != 0.0) gAdd(M + 2 * (size_t)key + 1, v1);
    }
}

// 1-4 exceptions: the geometry of atomExceptionsBody (atom_table.h), one thread per pair, the pair's value once under both ends' labels
template <typename Real> __device__ __forceinline__ void groupPairExceptionsBody(const PairListParams<Real>& p, const int k, const int* __restrict__ labels, double* const M, const int lane) {
    int key = -1; double v[2] = {0.0, 0.0};
    if (k < p.n) {
        int2 ij = p.pairs[k];
        ij.x = p.userToSorted[ij.x]; ij.y = p.userToSorted[ij.y];
        const int la = labels[ij.x], lb = labels[ij.y];
        if (la >= 0 && lb >= 0) {
            const auto par = p.params[k];
            const auto xi = p.posq[ij.x]; const auto xj = p.posq[ij.y];
            Real dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
            if (p.periodic) { Real inv[3] = {Real(1) / p.box[0], Real(1) / p.box[4], Real(1) / p.box[8]}; wrapDelta<Real>(dx, dy, dz, p.box, inv); }
            else unwrapDelta<Real>(dx, dy, dz, p.imageOffset, ij.x, ij.y);
            const Real invR = rsq(dx * dx + dy * dy + dz * dz);
            Real s2 = invR * par.x; s2 *= s2;
            const Real s6 = s2 * s2 * s2;
            PairEnergy::template exception<Real>(par, dx, dy, dz, invR, s6, v);
            key = groupPairSlice(la, lb);
        }
    }
    waveKeyedAdd(M, key, v[0], v[1], lane);
}

// Ewald exclusion corrections: the geometry of atomExclusionsBody (atom_table.h).  The atom's thread walks its own exclusion list and takes
// the partners with a LARGER sorted index: each excluded pair counts once.
template <typename Real> __device__ __forceinline__ void groupPairExclusionsBody(const PairListParams<Real>& p, const int a, const int* __restrict__ labels, double* const M, const int lane) {
    int key = -1; double s0 = 0.0, s1 = 0.0;
    const int ua = a < p.nExclAtoms ? p.sortedToUser[a] : -1;
    const int la = ua >= 0 ? labels[a] : -1;
    if (la >= 0) {
        const int e0 = p.exclStart[ua], e1 = p.exclStart[ua + 1];
        const auto xi = p.posq[a];
        const auto sei = p.sigeps[a];
        Real inv[3] = {Real(1) / p.box[0], Real(1) / p.box[4], Real(1) / p.box[8]};
        for (int e = e0; e < e1; e++) {
            const int b = p.userToSorted[p.exclList[e]];
            if (b <= a) continue;
            const int lb = labels[b];
            if (lb < 0) continue;
            const auto xj = p.posq[b];
            Real dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
            if (p.periodic) wrapDelta<Real>(dx, dy, dz, p.box, inv); else unwrapDelta<Real>(dx, dy, dz, p.imageOffset, a, b);
            double v[2];
            PairEnergy::template exclusion<Real>(p, xi.w, xj.w, sei, b, dx, dy, dz, v);
            const int k = groupPairSlice(la, lb);
            if (k != key) {      // a run of one key ends: the thread's own add (label borders only)
                if (key >= 0) { if (s0 != 0.0) gAdd(M + 2 * (size_t)key, s0); if (s1 != 0.0) gAdd(M + 2 * (size_t)key + 1, s1); }
                key = k; s0 = 0.0; s1 = 0.0;
            }
            s0 += v[0]; s1 += v[1];
        }
    }
    waveKeyedAdd(M, key, s0, s1, lane);
}

// Tile kernel: W waves per work-group (4 in single precision, 2 in double: the LDS block is 8 KB resp. 16 KB per wave), one wave per work
// item.  Lane l holds i-atom l & 31 and meets the j-slots of half l >> 5 in the rotated order of k_atomTiles.
template <typename Real, int MC, bool WRAP, int W>
__global__ __launch_bounds__(64 * W) void k_groupPairTiles(const DirectParams<Real> p, const PairListParams<Real> q, const int nExclBlocks, const int nListBlocks,
                                                           const int* __restrict__ labels, double* const Mall, const int mParts, const size_t mStride) {
    constexpr int CELLS = 1024;
    double* const M = Mall + (size_t)(blockIdx.x & (mParts - 1)) * mStride;      // this work-group's copy of the matrix
    const int lane = threadIdx.x & 63;
    if ((int)blockIdx.x < nListBlocks) {
        if ((int)blockIdx.x < nExclBlocks) groupPairExclusionsBody<Real>(q, blockIdx.x * (64 * W) + threadIdx.x, labels, M, lane);
        else groupPairExceptionsBody<Real>(q, ((int)blockIdx.x - nExclBlocks) * (64 * W) + threadIdx.x, labels, M, lane);
        return;
    }
    const int tileBlock = (int)blockIdx.x - nListBlocks, nTileBlocks = gridDim.x - nListBlocks;
    using T4 = typename Vec<Real>::T4;
    using T2 = typename Vec<Real>::T2;
    __shared__ T4 s_pos[W][32];
    __shared__ T2 s_se[W][32];
    __shared__ Real s_acc[W][2][CELLS];
    __shared__ int s_gI[W][32], s_gJ[W][32], s_jid[W][32];
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int il = lane & 31, jh = lane >> 5;
    T4* const myPos = s_pos[wid];
    T2* const mySe = s_se[wid];
    Real* const acc0 = s_acc[wid][0];
    Real* const acc1 = s_acc[wid][1];
    int* const myGI = s_gI[wid];
    int* const myGJ = s_gJ[wid];
    int* const myJid = s_jid[wid];
    for (int k = lane; k < CELLS; k += 64) { acc0[k] = 0; acc1[k] = 0; }
    waveSync();
    // what is accumulated and not yet in M: the labels it belongs to (wave-uniform), the lane's registers of the uniform case
    int curNI = 0, curNJ = 0, curGI0 = -1, curGJ0 = -1, log2R = 6;
    bool pending = false;
    double d0 = 0.0, d1 = 0.0;
    Real r0 = 0, r1 = 0;
    auto flush = [&]() {
        if (curNI == 1 && curNJ == 1) {
            d0 += (double)r0; d1 += (double)r1; r0 = 0; r1 = 0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { d0 += __shfl_xor(d0, o, 64); d1 += __shfl_xor(d1, o, 64); }
            if (lane == 0 && curGI0 >= 0 && curGJ0 >= 0) {
                const size_t k = groupPairSlice(curGI0, curGJ0);
                if (d0 != 0.0) gAdd(M + 2 * k, d0);
                if (d1 != 0.0) gAdd(M + 2 * k + 1, d1);
            }
            d0 = 0.0; d1 = 0.0;
        } else {
            waveSync();
            const int total = (curNI * curNJ) << log2R, R = 1 << log2R;
            for (int base = 0; base < total; base += 64) {
                const int idx = base + lane;
                double b0 = 0.0, b1 = 0.0;
                if (idx < total) { b0 = (double)acc0[idx]; b1 = (double)acc1[idx]; acc0[idx] = 0; acc1[idx] = 0; }
                for (int o = 1; o < R; o <<= 1) { b0 += __shfl_xor(b0, o, 64); b1 += __shfl_xor(b1, o, 64); }
                if (idx < total && (lane & (R - 1)) == 0) {
                    const int cell = idx >> log2R, ii = cell / curNJ, jj = cell - ii * curNJ;
                    const int ga = myGI[ii], gb = myGJ[jj];
                    if (ga >= 0 && gb >= 0) {
                        const size_t k = groupPairSlice(ga, gb);
                        if (b0 != 0.0) gAdd(M + 2 * k, b0);
                        if (b1 != 0.0) gAdd(M + 2 * k + 1, b1);
                    }
                }
            }
            waveSync();
        }
        pending = false;
    };
    // a wave takes runs of SNB_GROUP_PAIR_RUN consecutive items, the runs dealt round to the waves: neighbouring items are neighbouring
    // blocks, whose labels repeat (few flushes), while a region of many labels (a solute) is still spread over all waves
    const int nWaves = nTileBlocks * W;
    for (int run = (tileBlock * W + wid) * SNB_GROUP_PAIR_RUN; run < p.numWork; run += nWaves * SNB_GROUP_PAIR_RUN)
    for (int item = run; item < run + SNB_GROUP_PAIR_RUN && item < p.numWork; item++) {
        const int4 wi = p.workItems[p.workStart + item * p.workStride];
        const int I = __builtin_amdgcn_readfirstlane(wi.x);
        const int tBegin = __builtin_amdgcn_readfirstlane(wi.y), tEnd = tBegin + __builtin_amdgcn_readfirstlane(wi.z);
        const T4 pi = p.posq[I * 32 + il];
        const T2 sei = p.sigeps[I * 32 + il];
        const Real qi = pi.w * p.k4pe;
        Real c6i = 0;
        if (MC == MC_LJPME) c6i = Real(8) * sei.x * sei.x * sei.x * sei.y;
        // the item's i-labels (lanes l and l + 32 hold the same atom)
        const int li = labels[I * 32 + il];
        int nI, gI0; bool leaderI;
        const int myI = waveLocalIds(li, lane, nI, gI0, leaderI);
        if (nI == 0) continue;      // no i-atom of the block is in a group (wave-uniform; the lane registers are empty between items)
        // registers carry over from the last item only while both labels stay
        if (pending && !(curNI == 1 && curNJ == 1 && nI == 1 && gI0 == curGI0)) flush();
        curNI = nI; curGI0 = gI0;
        if (leaderI) myGI[myI] = li;
        for (int t = tBegin; t < tEnd; t++) {
            const int4 head = p.tileInfo[t];
            const int maskIdx = __builtin_amdgcn_readfirstlane(head.y);
            const int code = p.tileJ[t * 32 + il];      // (both halves load it: lanes l and l + 32 hold the same j-slot here)
            T4 pj; T2 sej; int lj = -1;
            if (code != -1) {
                const int idx = code & SNB_JIDX_MASK;
                pj = p.posq[idx]; sej = p.sigeps[idx]; lj = labels[idx];
                if (!WRAP) {
                    const int sc = (code >> SNB_JSHIFT_BITS) & 127;
                    const int kx = sc / 25, ky = (sc - 25 * kx) / 5, kz = sc - 25 * kx - 5 * ky;
                    const Real ka = Real(kx - 2), kb = Real(ky - 2), kc = Real(kz - 2);
                    pj.x += ka * p.box[0] + kb * p.box[3] + kc * p.box[6]; pj.y += kb * p.box[4] + kc * p.box[7]; pj.z += kc * p.box[8];
                }
            } else { pj.x = Real(3e9) + Real(1e6) * il; pj.y = Real(-5e9); pj.z = Real(7e9); pj.w = 0; sej.x = 0; sej.y = 0; }      // padding slot: parked far away
            const unsigned maskWord = maskIdx >= 0 ? p.masks[maskIdx * 32 + il] : 0u;
            int nJ, gJ0; bool leaderJ;
            const int myJ = waveLocalIds(lj, lane, nJ, gJ0, leaderJ);
            if (nJ == 0) continue;      // no j-atom of the tile is in a group (wave-uniform): the tile adds nothing and ends no run
            // pairs left out: the excluded ones and those with an end in no group (bit jj: j-slot jj; the lane's own i-atom: all of them)
            const unsigned deadJ = (unsigned)__ballot(lj < 0);      // (taken by every lane, outside the choice below: a ballot counts active lanes only)
            const unsigned skip = li >= 0 ? (maskWord | deadJ) : 0xFFFFFFFFu;
            // the block is kept across tiles while they carry one and the same j-label; any other tile starts a block of its own
            const bool carry = pending && nJ == 1 && curNJ == 1 && gJ0 == curGJ0;
            if (pending && !carry) flush();
            if (!carry) {
                curNJ = nJ; curGJ0 = gJ0;
                log2R = 6;
                while (((curNI * curNJ) << log2R) > CELLS) log2R--;
            }
            __builtin_amdgcn_wave_barrier();
            if (jh == 0) { myPos[il] = pj; mySe[il] = sej; myJid[il] = myJ; }
            if (leaderJ) myGJ[myJ] = lj;
            waveSync();
            const bool uniform = curNI == 1 && curNJ == 1;
            const int rowBase = myI * curNJ, rep = lane & ((1 << log2R) - 1);
#pragma unroll PairEnergy::UNROLL
            for (int s = 0; s < 16; s++) {
                const int jj = 16 * jh + ((il + s) & 15);
                Real v[2];
                bool include = PairEnergy::template eval<Real, MC, WRAP>(p, pi, sei, qi, c6i, myPos[jj], mySe[jj], v);
                include = include && !((skip >> jj) & 1u);
                if (include) {
                    if (uniform) { r0 += v[0]; r1 += v[1]; }
                    else {
                        const int a = ((rowBase + myJid[jj]) << log2R) + rep;
                        ldsAdd(acc0 + a, v[0]); ldsAdd(acc1 + a, v[1]);
                    }
                }
            }
            pending = true;
            waveSync();
        }
        d0 += (double)r0; d1 += (double)r1; r0 = 0; r1 = 0;      // (the uniform case: single-precision sums span one item)
    }
    if (pending) flush();
}

template <typename Real, int MC> void launchGroupPairTilesMC(const DirectParams<Real>& p, bool wrap, const PairListParams<Real>& q, int nExclBlocks, int nListBlocks, dim3 grid,
                                                            const int* labels, double* M, int parts, size_t stride, hipStream_t s) {
    constexpr int W = sizeof(Real) == 4 ? 4 : 2;
    if (wrap) hipLaunchKernelGGL((k_groupPairTiles<Real, MC, true, W>), grid, dim3(64 * W), 0, s, p, q, nExclBlocks, nListBlocks, labels, M, parts, stride);
    else hipLaunchKernelGGL((k_groupPairTiles<Real, MC, false, W>), grid, dim3(64 * W), 0, s, p, q, nExclBlocks, nListBlocks, labels, M, parts, stride);
}
// At most SNB_GROUP_PAIR_BLOCKS tile work-groups, however long the work list: each wave walks runs of items, so that what the uniform
// case holds in registers is flushed once per change of labels, not once per item.
#define SNB_GROUP_PAIR_BLOCKS 2048
template <typename Real> void launchGroupPairTiles(const DirectParams<Real>& p, int mc, bool wrap, const PairListParams<Real>* lists, const int* labels, double* M, int parts, size_t stride, hipStream_t s) {
    constexpr int W = sizeof(Real) == 4 ? 4 : 2;
    PairListParams<Real> q;
    std::memset(&q, 0, sizeof(q));
    int nExclBlocks = 0, nListBlocks = 0;
    if (lists) { q = *lists; nExclBlocks = (q.nExclAtoms + 64 * W - 1) / (64 * W); nListBlocks = nExclBlocks + (q.n + 64 * W - 1) / (64 * W); }
    const int perBlock = W * SNB_GROUP_PAIR_RUN;      // every wave launched has a run of items to take
    const int nTileBlocks = p.numWork > 0 ? std::min((p.numWork + perBlock - 1) / perBlock, SNB_GROUP_PAIR_BLOCKS) : 0;
    if (nTileBlocks + nListBlocks <= 0) return;
    const dim3 grid(nTileBlocks + nListBlocks);
    switch (mc) {
        case MC_NOCUTOFF: launchGroupPairTilesMC<Real, MC_NOCUTOFF>(p, wrap, q, nExclBlocks, nListBlocks, grid, labels, M, parts, stride, s); break;
        case MC_RF: launchGroupPairTilesMC<Real, MC_RF>(p, wrap, q, nExclBlocks, nListBlocks, grid, labels, M, parts, stride, s); break;
        case MC_EWALD: launchGroupPairTilesMC<Real, MC_EWALD>(p, wrap, q, nExclBlocks, nListBlocks, grid, labels, M, parts, stride, s); break;
        default: launchGroupPairTilesMC<Real, MC_LJPME>(p, wrap, q, nExclBlocks, nListBlocks, grid, labels, M, parts, stride, s); break;
    }
}
template void launchGroupPairTiles<float>(const DirectParams<float>&, int, bool, const PairListParams<float>*, const int*, double*, int, size_t, hipStream_t);
template void launchGroupPairTiles<double>(const DirectParams<double>&, int, bool, const PairListParams<double>*, const int*, double*, int, size_t, hipStream_t);

void launchGroupPairLabels(const int* labelsUser, const int* sortedToUser, int nPad, int* labelSorted, hipStream_t s) {
    if (nPad <= 0) return;
    hipLaunchKernelGGL(k_groupPairLabels, dim3((nPad + 255) / 256), dim3(256), 0, s, labelsUser, sortedToUser, nPad, labelSorted);
}

__global__ __launch_bounds__(256) void k_groupPairFinish(const double* __restrict__ M, const size_t n, const int parts, double* __restrict__ row) {
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) {
        double v = M[k];
        for (int c = 1; c < parts; c++) v += M[(size_t)c * n + k];      // (the copies in index order: the row is a function of the copies alone)
        row[k] = v;
    }
}
void launchGroupPairFinish(const double* M, size_t n, int parts, double* row, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_groupPairFinish, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, M, n, parts, row);
}

}  // namespace snb
