// virial.hip -- per-slice virial tensors (snb_evaluate_slice_virials).
//
// W[s][t][c] = - d E_raw[s][t] / d eps_c  under the homogeneous deformation r -> (1 + eps) r of the box vectors and of every atom, at fixed
// pair set: s = slice, t = 0 Coulomb / 1 vdW, c over xx, yy, zz, xy, xz, yz; raw (every lambda 1), kJ/mol.  The kernels here add into a
// working matrix double [SNB_SLICE_E_PARTS][S][2][6], a work-group into copy blockIdx mod SNB_SLICE_E_PARTS, as the slice energies of a
// step are kept: no kernel adds a pair with a global atomic of its own.
//
//   k_virialTiles    the walk of k_atomTiles (atom_table.h): the same work items, tile heads, shift codes, parked padding slots, masks and
//                    rotated slot order, and the two pair lists in the launch's first work-groups.  A pair adds d_a d_b f, once, with
//                    (d, fC, fLJ) of pairForces (pair_force.h); a tile lies in one slice (its head names it), so a lane keeps 12 running
//                    sums, drains them into double per tile and the wave folds them by a butterfly when the slice of the run changes.
//   k_virialGram     one thread per point of the forward spectrum gridCplx[sub][kx][ky][kzc] of the held meshes: the strain derivative of
//                    the reciprocal-space kernel value, a symmetric tensor per k, times the Gram product of every pair of meshes; reduced
//                    per wave and per work-group.  At fixed fractional coordinates the mesh charges do not change under strain, so this
//                    is the exact derivative of the mesh energy.
//   k_virialFinish   the copies in index order, the closed forms that go as 1 / V, row f of the output and its contraction with the lambda states.
#include "pair_force.h"
#include <cstring>

namespace snb {

#define SNB_VIRIAL_ROW 12      // doubles per slice: [2][6]

__device__ __forceinline__ void virialButterfly(double* w) {
#pragma unroll
    for (int c = 0; c < SNB_VIRIAL_ROW; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) w[c] += __shfl_xor(w[c], o, 64);
    }
}
__device__ __forceinline__ void virialRowAdd(double* const W, const int slice, const double* w) {
    double* const e = W + (size_t)slice * SNB_VIRIAL_ROW;
#pragma unroll
    for (int c = 0; c < SNB_VIRIAL_ROW; c++) if (w[c] != 0.0) gAdd(e + c, w[c]);
}
// the 12 values of a pair from the force on its i-end (v: Coulomb x y z, vdW x y z) and its delta
__device__ __forceinline__ void virialOfForce(const double dx, const double dy, const double dz, const double* v, double* w) {
#pragma unroll
    for (int t = 0; t < 2; t++) {
        w[6 * t] = dx * v[3 * t]; w[6 * t + 1] = dy * v[3 * t + 1]; w[6 * t + 2] = dz * v[3 * t + 2];
        w[6 * t + 3] = dx * v[3 * t + 1]; w[6 * t + 4] = dx * v[3 * t + 2]; w[6 * t + 5] = dy * v[3 * t + 2];
    }
}
// W[key] += w from every lane with key >= 0.  Live lanes that all hold one key are folded first: 12 atomics per wave.  Every lane of the
// wave must call.
__device__ __forceinline__ void virialKeyedAdd(double* const W, const int key, double* w, const int lane) {
    const unsigned long long live = __ballot(key >= 0);
    if (live == 0) return;
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
    const int k0 = __builtin_amdgcn_readlane(key, src);
    if (__ballot(key >= 0 && key != k0) == 0) {
        if (key < 0) {
#pragma unroll
            for (int c = 0; c < SNB_VIRIAL_ROW; c++) w[c] = 0;
        }
        virialButterfly(w);
        if (lane == 0) virialRowAdd(W, k0, w);
    } else if (key >= 0) virialRowAdd(W, key, w);
}

// 1-4 exceptions: the geometry of atomExceptionsBody (atom_table.h), one thread per pair, the pair once under the slice of its ends' subsets
template <typename Real> __device__ __forceinline__ void virialExceptionsBody(const PairListParams<Real>& p, const int k, double* const W, const int lane) {
    int key = -1; double w[SNB_VIRIAL_ROW];
#pragma unroll
    for (int c = 0; c < SNB_VIRIAL_ROW; c++) w[c] = 0;
    if (k < p.n) {
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
        double v[6];
        PairForce::template exception<Real>(par, dx, dy, dz, invR, s6, v);
        virialOfForce(dx, dy, dz, v, w);
        key = sliceOf(p.blockSubset[ij.x >> 5], p.blockSubset[ij.y >> 5]);
    }
    virialKeyedAdd(W, key, w, lane);
}

// Ewald exclusion corrections: the geometry of atomExclusionsBody (atom_table.h).  The atom's thread walks its own exclusion list and takes
// the partners with a LARGER sorted index: each excluded pair counts once.
template <typename Real> __device__ __forceinline__ void virialExclusionsBody(const PairListParams<Real>& p, const int a, double* const W, const int lane) {
    int key = -1; double w[SNB_VIRIAL_ROW];
#pragma unroll
    for (int c = 0; c < SNB_VIRIAL_ROW; c++) w[c] = 0;
    const int ua = a < p.nExclAtoms ? p.sortedToUser[a] : -1;
    if (ua >= 0) {
        const int e0 = p.exclStart[ua], e1 = p.exclStart[ua + 1];
        const int sa = p.blockSubset[a >> 5];
        const auto xi = p.posq[a];
        const auto sei = p.sigeps[a];
        Real inv[3] = {Real(1) / p.box[0], Real(1) / p.box[4], Real(1) / p.box[8]};
        for (int e = e0; e < e1; e++) {
            const int b = p.userToSorted[p.exclList[e]];
            if (b <= a) continue;
            const auto xj = p.posq[b];
            Real dx = xi.x - xj.x, dy = xi.y - xj.y, dz = xi.z - xj.z;
            if (p.periodic) wrapDelta<Real>(dx, dy, dz, p.box, inv); else unwrapDelta<Real>(dx, dy, dz, p.imageOffset, a, b);
            double v[6], u[SNB_VIRIAL_ROW];
            PairForce::template exclusion<Real>(p, xi.w, xj.w, sei, b, dx, dy, dz, v);
            virialOfForce(dx, dy, dz, v, u);
            const int k = sliceOf(sa, p.blockSubset[b >> 5]);
            if (k != key) {      // a run of one slice ends: the thread's own add (partners in another subset only)
                if (key >= 0) virialRowAdd(W, key, w);
                key = k;
#pragma unroll
                for (int c = 0; c < SNB_VIRIAL_ROW; c++) w[c] = 0;
            }
#pragma unroll
            for (int c = 0; c < SNB_VIRIAL_ROW; c++) w[c] += u[c];
        }
    }
    virialKeyedAdd(W, key, w, lane);
}

// Tile kernel.  One wave per work item, lane l holds i-atom l & 31 and meets the j-slots of half l >> 5 in the rotated order of k_atomTiles.
// The first nListBlocks work-groups run the pair lists.  sliceNeed is not consulted: every slice has a row.
template <typename Real, int MC, bool WRAP>
__global__ __launch_bounds__(256) void k_virialTiles(const DirectParams<Real> p, const PairListParams<Real> q, const int nExclBlocks, const int nListBlocks, double* const Wall) {
    const int nSlices = p.nsub * (p.nsub + 1) / 2;
    double* const W = SNB_SLICE_E_PARTITION(Wall, nSlices * SNB_VIRIAL_ROW);      // this work-group's copy of the matrix
    const int lane = threadIdx.x & 63;
    if ((int)blockIdx.x < nListBlocks) {
        if ((int)blockIdx.x < nExclBlocks) virialExclusionsBody<Real>(q, blockIdx.x * 256 + threadIdx.x, W, lane);
        else virialExceptionsBody<Real>(q, ((int)blockIdx.x - nExclBlocks) * 256 + threadIdx.x, W, lane);
        return;
    }
    const int tileBlock = (int)blockIdx.x - nListBlocks, nTileBlocks = gridDim.x - nListBlocks;
    using T4 = typename Vec<Real>::T4;
    using T2 = typename Vec<Real>::T2;
    __shared__ T4 s_pos[4][32];
    __shared__ T2 s_se[4][32];
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int il = lane & 31, jh = lane >> 5;
    T4* const myPos = s_pos[wid];
    T2* const mySe = s_se[wid];
    for (int item = tileBlock * 4 + wid; item < p.numWork; item += nTileBlocks * 4) {
        const int4 wi = p.workItems[p.workStart + item * p.workStride];
        const int I = __builtin_amdgcn_readfirstlane(wi.x);
        const int tBegin = __builtin_amdgcn_readfirstlane(wi.y), tEnd = tBegin + __builtin_amdgcn_readfirstlane(wi.z);
        const T4 pi = p.posq[I * 32 + il];
        const T2 sei = p.sigeps[I * 32 + il];
        const Real qi = pi.w * p.k4pe;
        Real c6i = 0;
        if (MC == MC_LJPME) c6i = Real(8) * sei.x * sei.x * sei.x * sei.y;
        double d[SNB_VIRIAL_ROW];
#pragma unroll
        for (int c = 0; c < SNB_VIRIAL_ROW; c++) d[c] = 0;
        int curSlice = -1;
        // the wave's sums of the run that ends, into row curSlice
        auto flush = [&]() {
            if (curSlice >= 0) {
                virialButterfly(d);
                if (lane == 0) virialRowAdd(W, curSlice, d);
            }
#pragma unroll
            for (int c = 0; c < SNB_VIRIAL_ROW; c++) d[c] = 0;
        };
        for (int t = tBegin; t < tEnd; t++) {
            const int4 head = p.tileInfo[t];
            const int slice = __builtin_amdgcn_readfirstlane(head.x), maskIdx = __builtin_amdgcn_readfirstlane(head.y);
            if (slice != curSlice) { flush(); curSlice = slice; }
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
            if (jh == 0) { myPos[il] = pj; mySe[il] = sej; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            Real a[SNB_VIRIAL_ROW];
#pragma unroll
            for (int c = 0; c < SNB_VIRIAL_ROW; c++) a[c] = 0;
#pragma unroll 2
            for (int s = 0; s < 16; s++) {
                const int jj = 16 * jh + ((il + s) & 15);
                Real dx, dy, dz, fC, fLJ;
                bool include = pairForces<Real, MC, WRAP>(p, pi, sei, qi, c6i, myPos[jj], mySe[jj], dx, dy, dz, fC, fLJ);
                include = include && !((maskWord >> jj) & 1u);
                if (include) {
                    const Real xx = dx * dx, yy = dy * dy, zz = dz * dz, xy = dx * dy, xz = dx * dz, yz = dy * dz;
                    a[0] += xx * fC; a[1] += yy * fC; a[2] += zz * fC; a[3] += xy * fC; a[4] += xz * fC; a[5] += yz * fC;
                    a[6] += xx * fLJ; a[7] += yy * fLJ; a[8] += zz * fLJ; a[9] += xy * fLJ; a[10] += xz * fLJ; a[11] += yz * fLJ;
                }
            }
#pragma unroll
            for (int c = 0; c < SNB_VIRIAL_ROW; c++) d[c] += (double)a[c];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        flush();
    }
}

template <typename Real, int MC> static void launchVirialTilesMC(const DirectParams<Real>& p, bool wrap, const PairListParams<Real>& q, int nExclBlocks, int nListBlocks, dim3 grid, double* W, hipStream_t s) {
    if (wrap) hipLaunchKernelGGL((k_virialTiles<Real, MC, true>), grid, dim3(256), 0, s, p, q, nExclBlocks, nListBlocks, W);
    else hipLaunchKernelGGL((k_virialTiles<Real, MC, false>), grid, dim3(256), 0, s, p, q, nExclBlocks, nListBlocks, W);
}
template <typename Real> void launchVirialTiles(const DirectParams<Real>& p, int mc, bool wrap, const PairListParams<Real>* lists, double* W, hipStream_t s) {
    PairListParams<Real> q;
    std::memset(&q, 0, sizeof(q));
    int nExclBlocks = 0, nListBlocks = 0;
    if (lists) { q = *lists; nExclBlocks = (q.nExclAtoms + 255) / 256; nListBlocks = nExclBlocks + (q.n + 255) / 256; }
    const int nTileBlocks = p.numWork > 0 ? (p.numWork + 3) / 4 : 0;
    if (nTileBlocks + nListBlocks <= 0) return;
    const dim3 grid(nTileBlocks + nListBlocks);
    switch (mc) {
        case MC_NOCUTOFF: launchVirialTilesMC<Real, MC_NOCUTOFF>(p, wrap, q, nExclBlocks, nListBlocks, grid, W, s); break;
        case MC_RF: launchVirialTilesMC<Real, MC_RF>(p, wrap, q, nExclBlocks, nListBlocks, grid, W, s); break;
        case MC_EWALD: launchVirialTilesMC<Real, MC_EWALD>(p, wrap, q, nExclBlocks, nListBlocks, grid, W, s); break;
        default: launchVirialTilesMC<Real, MC_LJPME>(p, wrap, q, nExclBlocks, nListBlocks, grid, W, s); break;
    }
}
template void launchVirialTiles<float>(const DirectParams<float>&, int, bool, const PairListParams<float>*, double*, hipStream_t);
template void launchVirialTiles<double>(const DirectParams<double>&, int, bool, const PairListParams<double>*, double*, hipStream_t);

// ---- mesh part -----------------------------------------------------------------------------------------------------------------------
// The strain derivative of the reciprocal-space kernel value at mesh point (kx, ky, kz), t[c] = - d eterm / d eps_c, with eterm as
// recipTermRaw (pme.hip) forms it, in double from the unrounded reciprocal box:
//   Coulomb      eterm [delta_ab - 2 mh_a mh_b (1 / m^2 + pi^2 / alpha^2)],                                       0 at k = 0;
//   dispersion   (boxfactor / bprod) [g(m) delta_ab + 3 mh_a mh_b (fac1 erfc(b) m + fac3 exp(-b^2))],   b = pi m / alpha_d, k = 0 included.
// (d m^2 / d eps_ab = -2 mh_a mh_b and d V / d eps_ab = V delta_ab; the B-spline moduli depend on the indices alone.)
template <typename Real> __device__ inline void virialKernelTerm(const VirialMesh<Real>& p, const int kx, const int ky, const int kz, double* t) {
    const int nx = p.nx, ny = p.ny, nz = p.nz;
    const double mx = (double)((kx < (nx + 1) / 2) ? kx : kx - nx);
    const double my = (double)((ky < (ny + 1) / 2) ? ky : ky - ny);
    const double mz = (double)((kz < (nz + 1) / 2) ? kz : kz - nz);
    const double hx = mx * p.recip[0];
    const double hy = mx * p.recip[3] + my * p.recip[4];
    const double hz = mx * p.recip[6] + my * p.recip[7] + mz * p.recip[8];
    const double m2 = hx * hx + hy * hy + hz * hz;
    const double bprod = (double)p.modx[kx] * (double)p.mody[ky] * (double)p.modz[kz];
    double iso, aniso;      // t_ab = iso delta_ab + aniso mh_a mh_b
    if (!p.dispersion) {
        if (kx == 0 && ky == 0 && kz == 0) { iso = 0; aniso = 0; }
        else {
            const double factor = SNB_PI * SNB_PI / (p.alpha * p.alpha);
            iso = SNB_ONE_4PI_EPS0 * exp(-factor * m2) / (m2 * SNB_PI * p.volume * bprod);
            aniso = -2.0 * iso * (1.0 / m2 + factor);
        }
    } else {
        const double denom = (-2 * SNB_PI * 1.7724538509055159) / (6.0 * p.volume) / bprod;
        const double fac1 = 2 * SNB_PI * SNB_PI * SNB_PI * 1.7724538509055159;
        const double fac2 = p.alpha * p.alpha * p.alpha;
        const double fac3 = -2.0 * p.alpha * SNB_PI * SNB_PI;
        const double m = sqrt(m2), b = SNB_PI / p.alpha * m;
        const double eb = exp(-b * b), ec = erfc(b);
        iso = denom * (fac1 * ec * m * m2 + eb * (fac2 + fac3 * m2));
        aniso = 3.0 * denom * (fac1 * ec * m + fac3 * eb);
    }
    t[0] = iso + aniso * hx * hx; t[1] = iso + aniso * hy * hy; t[2] = iso + aniso * hz * hz;
    t[3] = aniso * hx * hy; t[4] = aniso * hx * hz; t[5] = aniso * hy * hz;
}

// One thread per point of the half-complex spectrum.  W[slice(I, J)][term][c] += sum_k weight t_c(k) Re(S_I conj S_J) (x 1/2 for I = J)
// over the FULL mesh: weight 2 off the kz = 0 and Nyquist planes, as the Gram loop of k_convolveX; on Nyquist planes the average over k and
// -k that recipTerm (pme.hip) applies to the energy.  A pair of meshes at a time: the wave's butterfly, the work-group's four waves
// through LDS (two buffers in turn: one barrier per pair), six atomics per work-group and pair into its copy of the matrix.
template <typename Real> __global__ __launch_bounds__(256) void k_virialGram(const VirialMesh<Real> p, double* const Wall) {
    const int nSlices = p.nsubTotal * (p.nsubTotal + 1) / 2;
    double* const W = SNB_SLICE_E_PARTITION(Wall, nSlices * SNB_VIRIAL_ROW);
    __shared__ double s_red[2][4][6];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long nPts = (long long)p.nx * p.ny * p.nzc;
    const long long idx = (long long)blockIdx.x * 256 + tid;
    const bool valid = idx < nPts;
    double t[6] = {0, 0, 0, 0, 0, 0};
    if (valid) {
        const int kz = (int)(idx % p.nzc);
        const long long r = idx / p.nzc;
        const int ky = (int)(r % p.ny), kx = (int)(r / p.ny);
        virialKernelTerm<Real>(p, kx, ky, kz, t);
        if (2 * kx == p.nx || 2 * ky == p.ny || 2 * kz == p.nz) {
            double u[6];
            virialKernelTerm<Real>(p, kx == 0 ? 0 : p.nx - kx, ky == 0 ? 0 : p.ny - ky, kz == 0 ? 0 : p.nz - kz, u);
#pragma unroll
            for (int c = 0; c < 6; c++) t[c] = 0.5 * (t[c] + u[c]);
        }
        const double w = (kz == 0 || 2 * kz == p.nz) ? 1.0 : 2.0;
#pragma unroll
        for (int c = 0; c < 6; c++) t[c] *= w;
    }
    const int term = p.dispersion ? 1 : 0;
    int turn = 0;
    for (int I = 0; I < p.nsub; I++) {
        const int gi = p.gridSubset[I];
        typename Vec<Real>::T2 a; a.x = 0; a.y = 0;
        if (valid) a = p.spectrum[(size_t)I * nPts + idx];
        for (int J = 0; J <= I; J++, turn ^= 1) {
            typename Vec<Real>::T2 b; b.x = 0; b.y = 0;
            if (valid) b = p.spectrum[(size_t)J * nPts + idx];
            double g = (double)a.x * (double)b.x + (double)a.y * (double)b.y;
            if (I == J) g *= 0.5;
            double v[6];
#pragma unroll
            for (int c = 0; c < 6; c++) {
                v[c] = g * t[c];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o, 64);
            }
            if (lane == 0) {
#pragma unroll
                for (int c = 0; c < 6; c++) s_red[turn][wave][c] = v[c];
            }
            __syncthreads();
            if (tid < 6) {
                const double tot = s_red[turn][0][tid] + s_red[turn][1][tid] + s_red[turn][2][tid] + s_red[turn][3][tid];
                if (tot != 0.0) gAdd(W + (size_t)sliceOf(gi, p.gridSubset[J]) * SNB_VIRIAL_ROW + term * 6 + tid, tot);
            }
        }
    }
}
template <typename Real> void launchVirialGram(const VirialMesh<Real>& p, double* W, hipStream_t s) {
    const long long nPts = (long long)p.nx * p.ny * p.nzc;
    if (nPts <= 0 || p.nsub <= 0) return;
    hipLaunchKernelGGL((k_virialGram<Real>), dim3((unsigned)((nPts + 255) / 256)), dim3(256), 0, s, p, W);
}
template void launchVirialGram<float>(const VirialMesh<float>&, double*, hipStream_t);
template void launchVirialGram<double>(const VirialMesh<double>&, double*, hipStream_t);

// ---- finish --------------------------------------------------------------------------------------------------------------------------
// The closed forms of raw slice energy (slice, term) that go as 1 / V -- the neutralising background (Coulomb) and the long-range
// dispersion correction (vdW), switched as makeSliceFinish switches their energies: - dE/d eps_ab = E delta_ab.  The self terms do not
// depend on the box.
__device__ inline double virialClosedForm(const SliceFinish& f, const int slice, const int term) {
    if (term == 1) return f.dispCoef ? f.dispCoef[slice] * f.invVolume : 0.0;
    if (!f.sums) return 0.0;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= slice) a++;      // slice = a (a + 1) / 2 + b, b <= a
    const int b = slice - a * (a + 1) / 2;
    return (a == b ? 1.0 : 2.0) * f.sums[3 * a] * f.sums[3 * b] * f.background;
}
// One work-group: every entry of row[S][2][6] from the copies in index order (the row is a function of the copies alone), then
// states[k][c] = sum_s sum_t lam[k][s][t] row[s][t][c].
__global__ __launch_bounds__(256) void k_virialFinish(const double* __restrict__ W, const int nSlices, const SliceFinish f, double* __restrict__ row,
                                                      const double* __restrict__ lam, const int nStates, double* __restrict__ states) {
    const int n = nSlices * SNB_VIRIAL_ROW;
    for (int i = threadIdx.x; i < n; i += 256) {
        double v = W[i];
        for (int c = 1; c < SNB_SLICE_E_PARTS; c++) v += W[(size_t)c * n + i];
        const int slice = i / SNB_VIRIAL_ROW, r = i - slice * SNB_VIRIAL_ROW, term = r / 6, c = r - term * 6;
        if (c < 3) v += virialClosedForm(f, slice, term);
        row[i] = v;
    }
    __syncthreads();
    for (int o = threadIdx.x; o < nStates * 6; o += 256) {
        const int k = o / 6, c = o - k * 6;
        const double* const l = lam + (size_t)k * nSlices * 2;
        double acc = 0;
        for (int e = 0; e < nSlices * 2; e++) acc += l[e] * row[e * 6 + c];
        states[o] = acc;
    }
}
void launchVirialFinish(const double* W, int nSlices, const SliceFinish& f, double* row, const double* stateLambdas, int nStates, double* states, hipStream_t s) {
    hipLaunchKernelGGL(k_virialFinish, dim3(1), dim3(256), 0, s, W, nSlices, f, row, stateLambdas, nStates, states);
}

}  // namespace snb
