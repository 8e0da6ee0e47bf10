// atom_table.h -- the device code the per-atom table kernels share (atomenergy.hip, atomforce.hip; DESIGN.md sections 4.8 and 4.9).
//
// A per-atom table is double [Npad][nsub][NV] over the SORTED atom index: NV = 2 raw energies (Coulomb, vdW) or 6 force components (Coulomb
// x y z, vdW x y z) of atom i with all atoms of subset J.  What walks the tiles, the two pair lists and the mesh stencil is the same for
// both and lives here once; what a pair or a list entry contributes is the table's own and comes in as a struct Pair:
//
//   NV, UNROLL, J_SIGN        values per pair, the unroll count of the 16-step tile loop, the sign the partner's end takes (+1 energy, -1 force)
//   eval<Real, MC, WRAP>      the NV values of a tile pair (i, j) for the i-end; returns whether the pair is inside the cutoff
//   exception<Real>           the NV values of a 1-4 exception for the i-end, from the walker's delta, 1/r and (sigma/r)^6
//   exclusion<Real>           the NV values of an Ewald exclusion correction for the atom's own end, from the walker's delta
//
//   k_atomTiles      the tiles of the pair kernel.  A tile lies in one slice (32 i-atoms of one block x 32 j-atoms of one subset), so
//                    inside a tile every i-atom's values belong to column s_J and every j-atom's to column s_I: the i-side is the lane's own
//                    NV running sums (flushed per run of tiles of one j subset), the j-side a per-wave LDS region [32][NV] the steps add
//                    into, flushed per tile with J_SIGN.  Every pair is visited once (diagonal tiles included) and credits both ends.
//   list blocks      Ewald exclusion corrections (one thread per atom, the whole pair value into its own row -- the partner's thread
//                    credits the other end) and 1-4 exceptions (one thread per pair, both ends), in the same launch.
//   k_atomStencil    q_i psi_J(r_i) (GRAD = false) or -q_i grad psi_J(r_i) (GRAD = true) for every held mesh J from the UNMIXED potentials
//                    (the pipeline of a rank that owns every mesh).
#pragma once
#include "snb_internal.h"
#include "pair_math.h"
#include <cstring>

namespace snb {

// one column entry of a table: tab[atom][col][0 .. NV) += v; adds of exactly zero are skipped
template <int NV> __device__ inline void tabAddN(double* tab, int nsub, int atom, int col, const double* v) {
    double* const e = tab + ((size_t)atom * nsub + col) * NV;
#pragma unroll
    for (int c = 0; c < NV; c++) if (v[c] != 0.0) gAdd(e + c, v[c]);
}

// 1-4 exceptions: the geometry of exceptionsBody (direct.hip); Pair::exception forms the i-end's values, the j-end takes them with J_SIGN
template <typename Real, typename Pair> __device__ __forceinline__ void atomExceptionsBody(const PairListParams<Real>& p, const int blk, double* tab, const int nsub) {
    const int k = blk * 256 + threadIdx.x;
    if (k >= p.n) return;
    int2 ij = p.pairs[k];
    ij.x = p.userToSorted[ij.x]; ij.y = p.userToSorted[ij.y];
    const auto par = p.params[k];
    const auto xi = p.posq[ij.x]; const auto xj = p.posq[ij.y];
    Real dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
    if (p.periodic) { Real inv[3] = {Real(1) / p.box[0], Real(1) / p.box[4], Real(1) / p.box[8]}; wrapDelta<Real>(dx, dy, dz, p.box, inv); }
    else unwrapDelta<Real>(dx, dy, dz, p.imageOffset, ij.x, ij.y);
    const Real invR = rsq(dx * dx + dy * dy + dz * dz);
    Real s2 = invR * par.x; s2 *= s2;
    const Real s6 = s2 * s2 * s2;
    double vi[Pair::NV], vj[Pair::NV];
    Pair::template exception<Real>(par, dx, dy, dz, invR, s6, vi);
#pragma unroll
    for (int c = 0; c < Pair::NV; c++) vj[c] = Pair::J_SIGN * vi[c];
    tabAddN<Pair::NV>(tab, nsub, ij.x, p.blockSubset[ij.y >> 5], vi);
    tabAddN<Pair::NV>(tab, nsub, ij.y, p.blockSubset[ij.x >> 5], vj);
}

// Ewald exclusion corrections: the pairs of exclusionAtomsBody (direct.hip).  The atom's thread walks its own exclusion list and takes the
// WHOLE pair value (Pair::exclusion) into its own row, column of the partner's subset; the partner's thread does the same for its end.
template <typename Real, typename Pair> __device__ __forceinline__ void atomExclusionsBody(const PairListParams<Real>& p, const int blk, double* tab, const int nsub) {
    const int a = blk * 256 + threadIdx.x;
    const int ua = a < p.nExclAtoms ? p.sortedToUser[a] : -1;
    if (ua < 0) return;
    const int e0 = p.exclStart[ua], e1 = p.exclStart[ua + 1];
    if (e1 <= e0) return;
    const auto xi = p.posq[a];
    const auto sei = p.sigeps[a];
    Real inv[3] = {Real(1) / p.box[0], Real(1) / p.box[4], Real(1) / p.box[8]};
    for (int e = e0; e < e1; e++) {
        const int b = p.userToSorted[p.exclList[e]];
        const auto xj = p.posq[b];
        Real dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
        if (p.periodic) wrapDelta<Real>(dx, dy, dz, p.box, inv); else unwrapDelta<Real>(dx, dy, dz, p.imageOffset, a, b);
        double v[Pair::NV];
        Pair::template exclusion<Real>(p, xi.w, xj.w, sei, b, dx, dy, dz, v);
        tabAddN<Pair::NV>(tab, nsub, a, p.blockSubset[b >> 5], v);
    }
}

// Tile kernel.  One wave per work item (an i-block and a run of its tiles), as the pair kernels; lane l holds i-atom l & 31 and meets the
// j-slots of half l >> 5, 16 steps per tile: at step s slot 16 (l >> 5) + ((l + s) & 15), so the 32 lanes of a half read 16 LDS entries
// (each by two lanes) and the j-side LDS adds of a step collide at most two ways.  The first nListBlocks work-groups run the pair lists.
// sliceNeed is not consulted: the table covers every slice.
template <typename Real, int MC, bool WRAP, typename Pair>
__global__ __launch_bounds__(256) void k_atomTiles(const DirectParams<Real> p, const PairListParams<Real> q, const int nExclBlocks, const int nListBlocks, double* const tab) {
    constexpr int NV = Pair::NV;
    if ((int)blockIdx.x < nListBlocks) {
        if ((int)blockIdx.x < nExclBlocks) atomExclusionsBody<Real, Pair>(q, blockIdx.x, tab, p.nsub);
        else atomExceptionsBody<Real, Pair>(q, blockIdx.x - nExclBlocks, tab, p.nsub);
        return;
    }
    const int tileBlock = (int)blockIdx.x - nListBlocks, nTileBlocks = gridDim.x - nListBlocks;
    using T4 = typename Vec<Real>::T4;
    using T2 = typename Vec<Real>::T2;
    __shared__ T4 s_pos[4][32];
    __shared__ T2 s_se[4][32];
    __shared__ Real s_vj[4][32][NV];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int il = lane & 31, jh = lane >> 5;
    T4* const myPos = s_pos[wid];
    T2* const mySe = s_se[wid];
    Real (*const myVj)[NV] = s_vj[wid];
    const int nsub = p.nsub;
    for (int item = tileBlock * 4 + wid; item < p.numWork; item += nTileBlocks * 4) {
        const int4 wi = p.workItems[p.workStart + item * p.workStride];
        const int I = __builtin_amdgcn_readfirstlane(wi.x);
        const int tBegin = __builtin_amdgcn_readfirstlane(wi.y), tEnd = tBegin + __builtin_amdgcn_readfirstlane(wi.z);
        const int sI = __builtin_amdgcn_readfirstlane(p.blockSubset[I]);
        const T4 pi = p.posq[I * 32 + il];
        const T2 sei = p.sigeps[I * 32 + il];
        const Real qi = pi.w * p.k4pe;
        Real c6i = 0;
        if (MC == MC_LJPME) c6i = Real(8) * sei.x * sei.x * sei.x * sei.y;
        Real vi[NV];
#pragma unroll
        for (int c = 0; c < NV; c++) vi[c] = 0;
        int curJ = -1;
        // i-side: the two lanes of an i-atom (one per j-half) merged, then one add per value into column curJ
        auto flushI = [&]() {
            double m[NV];
#pragma unroll
            for (int c = 0; c < NV; c++) { m[c] = (double)vi[c] + (double)__shfl_xor(vi[c], 32, 64); vi[c] = 0; }
            if (curJ >= 0 && jh == 0) tabAddN<NV>(tab, nsub, I * 32 + il, curJ, m);
        };
        for (int t = tBegin; t < tEnd; t++) {
            const int4 head = p.tileInfo[t];
            const int maskIdx = __builtin_amdgcn_readfirstlane(head.y), sJ = __builtin_amdgcn_readfirstlane(head.z);
            if (sJ != curJ) { flushI(); curJ = sJ; }
            const int code = p.tileJ[t * 32 + il];      // (both halves load it: lanes l and l + 32 hold the same j-slot here)
            T4 pj; T2 sej;
            if (code != -1) {
                const int idx = code & SNB_JIDX_MASK;
                pj = p.posq[idx]; sej = p.sigeps[idx];
                if (!WRAP) {
                    const int sc = (code >> SNB_JSHIFT_BITS) & 127;
                    const int kx = sc / 25, ky = (sc - 25 * kx) / 5, kz = sc - 25 * kx - 5 * ky;
                    const Real ka = Real(kx - 2), kb = Real(ky - 2), kc = Real(kz - 2);
                    pj.x += ka * p.box[0] + kb * p.box[3] + kc * p.box[6]; pj.y += kb * p.box[4] + kc * p.box[7]; pj.z += kc * p.box[8];
                }
            } else { pj.x = Real(3e9) + Real(1e6) * il; pj.y = Real(-5e9); pj.z = Real(7e9); pj.w = 0; sej.x = 0; sej.y = 0; }      // padding slot: parked far away
            const unsigned maskWord = maskIdx >= 0 ? p.masks[maskIdx * 32 + il] : 0u;
            __builtin_amdgcn_wave_barrier();
            if (jh == 0) {
                myPos[il] = pj; mySe[il] = sej;
#pragma unroll
                for (int c = 0; c < NV; c++) myVj[il][c] = 0;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
#pragma unroll Pair::UNROLL
            for (int s = 0; s < 16; s++) {
                const int jj = 16 * jh + ((il + s) & 15);
                Real v[NV];
                bool include = Pair::template eval<Real, MC, WRAP>(p, pi, sei, qi, c6i, myPos[jj], mySe[jj], v);
                include = include && !((maskWord >> jj) & 1u);
                if (include) {
#pragma unroll
                    for (int c = 0; c < NV; c++) { vi[c] += v[c]; ldsAdd(&myVj[jj][c], v[c]); }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // j-side: lanes 0-31 flush slot l into column s_I of their j-atom, with the partner's sign
            if (jh == 0 && code != -1) {
                double m[NV];
#pragma unroll
                for (int c = 0; c < NV; c++) m[c] = Pair::J_SIGN * (double)myVj[il][c];
                tabAddN<NV>(tab, nsub, code & SNB_JIDX_MASK, sI, m);
            }
        }
        flushI();
        __builtin_amdgcn_wave_barrier();
    }
}

// the tile kernel of one table for (method class, wrap), the pair lists in its first work-groups
template <typename Real, int MC, typename Pair>
void launchAtomTilesMC(const DirectParams<Real>& p, bool wrap, const PairListParams<Real>& q, int nExclBlocks, int nListBlocks, dim3 grid, double* tab, hipStream_t s) {
    if (wrap) hipLaunchKernelGGL((k_atomTiles<Real, MC, true, Pair>), grid, dim3(256), 0, s, p, q, nExclBlocks, nListBlocks, tab);
    else hipLaunchKernelGGL((k_atomTiles<Real, MC, false, Pair>), grid, dim3(256), 0, s, p, q, nExclBlocks, nListBlocks, tab);
}
template <typename Real, typename Pair> void launchAtomTiles(const DirectParams<Real>& p, int mc, bool wrap, const PairListParams<Real>* lists, double* tab, hipStream_t s) {
    PairListParams<Real> q;
    std::memset(&q, 0, sizeof(q));
    int nExclBlocks = 0, nListBlocks = 0;
    if (lists) { q = *lists; nExclBlocks = (q.nExclAtoms + 255) / 256; nListBlocks = nExclBlocks + (q.n + 255) / 256; }
    const int nTileBlocks = p.numWork > 0 ? (p.numWork + 3) / 4 : 0;
    if (nTileBlocks + nListBlocks <= 0) return;
    const dim3 grid(nTileBlocks + nListBlocks);
    switch (mc) {
        case MC_NOCUTOFF: launchAtomTilesMC<Real, MC_NOCUTOFF, Pair>(p, wrap, q, nExclBlocks, nListBlocks, grid, tab, s); break;
        case MC_RF: launchAtomTilesMC<Real, MC_RF, Pair>(p, wrap, q, nExclBlocks, nListBlocks, grid, tab, s); break;
        case MC_EWALD: launchAtomTilesMC<Real, MC_EWALD, Pair>(p, wrap, q, nExclBlocks, nListBlocks, grid, tab, s); break;
        default: launchAtomTilesMC<Real, MC_LJPME, Pair>(p, wrap, q, nExclBlocks, nListBlocks, grid, tab, s); break;
    }
}

// ---- reciprocal part per atom ------------------------------------------------------------------------------------------------------
// B-spline weights of order 5 without the derivatives.  Kept beside bspline5 (snb_internal.h): the same expressions, but the compiler fuses
// their multiply-adds differently, and the single-precision energy table moves by 7e-6 of an entry when the value path takes bspline5.
template <typename Real> __device__ inline void bsplineWeights5(Real dr, Real* d) {
    d[4] = 0; d[1] = dr; d[0] = 1 - dr; d[2] = 0; d[3] = 0;
    d[2] = Real(0.5) * dr * d[1];
    d[1] = Real(0.5) * ((dr + 1) * d[0] + (2 - dr) * d[1]);
    d[0] = Real(0.5) * (1 - dr) * d[0];
    d[3] = Real(1.0 / 3.0) * dr * d[2];
    d[2] = Real(1.0 / 3.0) * ((dr + 1) * d[1] + (3 - dr) * d[2]);
    d[1] = Real(1.0 / 3.0) * ((dr + 2) * d[0] + (2 - dr) * d[1]);
    d[0] = Real(1.0 / 3.0) * (1 - dr) * d[0];
    d[4] = Real(0.25) * dr * d[3];
    d[3] = Real(0.25) * ((dr + 1) * d[2] + (4 - dr) * d[3]);
    d[2] = Real(0.25) * ((dr + 2) * d[1] + (3 - dr) * d[2]);
    d[1] = Real(0.25) * ((dr + 3) * d[0] + (2 - dr) * d[1]);
    d[0] = Real(0.25) * (1 - dr) * d[0];
}
// 32 lanes per atom, lane = one (x, y) row of the 5 x 5 x 5 stencil, as the gather interpolation k_interpolate (pme.hip), unmixed and without
// lambdas; the atom loops over the held meshes (mesh g is the potential of subset gridSubset[g]) and adds into its row of the table
//   GRAD = false   q_i psi_J(r_i): the value part of the interpolation, no force arithmetic (tab [..][nsub][2]);
//   GRAD = true    -q_i grad psi_J(r_i): the derivative part, through the same triclinic back-transformation (tab [..][nsub][2][3])
// -- c6_i for q_i on the dispersion mesh.  Plain read-modify-write: the launch is ordered behind the pair kernel and an entry has one writer here.
template <typename Real, bool GRAD> __global__ __launch_bounds__(256) void k_atomStencil(const PmeParams<Real> p, double* const tab) {
    constexpr int NS = GRAD ? 3 : 1;      // sums per (atom, mesh) = table values per term
    const int gid = blockIdx.x * 8 + (threadIdx.x >> 5);
    const int r = threadIdx.x & 31;
    if (gid >= p.natoms) return;
    const int si = p.atomSubset[gid];
    if (si < 0) return;      // padding slot (uniform over the atom's 32 lanes)
    const auto pos = p.posq[gid];
    Real q = pos.w;
    if (p.dispersion) { const auto se = p.sigeps[gid]; q = Real(8) * se.x * se.x * se.x * se.y; }
    if (q == Real(0)) return;
    int idx[3]; Real fr[3];
    gridCoord<Real>(p.recip, p.recipLo, pos.x, pos.y, pos.z, p.d.nx, p.d.ny, p.d.nz, idx, fr);
    Real tx[5], ty[5], tz[5], dx[5], dy[5], dz[5];      // (GRAD = false: no derivative weight is formed or read)
    if constexpr (GRAD) { bspline5<Real>(fr[0], tx, dx); bspline5<Real>(fr[1], ty, dy); bspline5<Real>(fr[2], tz, dz); }
    else { bsplineWeights5<Real>(fr[0], tx); bsplineWeights5<Real>(fr[1], ty); bsplineWeights5<Real>(fr[2], tz); }
    const int ix = r < 25 ? r / 5 : 0, iy = r < 25 ? r - ix * 5 : 0;
    int xi = idx[0] + ix; if (xi >= p.d.nx) xi -= p.d.nx;
    int yi = idx[1] + iy; if (yi >= p.d.ny) yi -= p.d.ny;
    Real txv = 0, dxv = 0, tyv = 0, dyv = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) {
        if (k == ix) { txv = tx[k]; if constexpr (GRAD) dxv = dx[k]; }
        if (k == iy) { tyv = ty[k]; if constexpr (GRAD) dyv = dy[k]; }
    }
    if (r >= 25) { txv = 0; dxv = 0; }
    const int term = p.dispersion ? 1 : 0;
    const double nx = p.d.nx, ny = p.d.ny, nz = p.d.nz;
    for (int g = 0; g < p.nsub; g++) {
        const Real* row = p.gridReal + (((size_t)g * p.d.nx + xi) * p.d.ny + yi) * p.d.nz;
        Real sz = 0, sdz = 0;
#pragma unroll
        for (int iz = 0; iz < 5; iz++) {
            int zi = idx[2] + iz; if (zi >= p.d.nz) zi -= p.d.nz;
            const Real gv = row[zi];
            sz += tz[iz] * gv;
            if constexpr (GRAD) sdz += dz[iz] * gv;
        }
        double f[NS];
        if constexpr (GRAD) { f[0] = (double)(dxv * tyv * sz); f[1] = (double)(txv * dyv * sz); f[2] = (double)(txv * tyv * sdz); }
        else f[0] = (double)(txv * tyv * sz);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
#pragma unroll
            for (int c = 0; c < NS; c++) f[c] += __shfl_xor(f[c], o, 64);
        }
        if (r == 0) {
            double* const e = tab + (((size_t)gid * p.nsubTotal + p.gridSubset[g]) * 2 + term) * NS;
            if constexpr (GRAD) {
                const double mq = -(double)q;
                e[0] += mq * (f[0] * nx * (double)p.recip[0]);
                e[1] += mq * (f[0] * nx * (double)p.recip[3] + f[1] * ny * (double)p.recip[4]);
                e[2] += mq * (f[0] * nx * (double)p.recip[6] + f[1] * ny * (double)p.recip[7] + f[2] * nz * (double)p.recip[8]);
            } else e[0] += (double)q * f[0];
        }
    }
}
template <typename Real, bool GRAD> void launchAtomStencil(const PmeParams<Real>& p, double* tab, hipStream_t s) {
    if (p.natoms <= 0 || p.nsub <= 0) return;
    hipLaunchKernelGGL((k_atomStencil<Real, GRAD>), dim3((p.natoms + 7) / 8), dim3(256), 0, s, p, tab);
}

}  // namespace snb
