// The host neighbour-list builder as a pure function: plain data in, plain data out, no HIP.  It is the only builder for NoCutoff, for
// systems of fewer than 64 atoms, for cells that are not rectangular and for boxes too small for tile images (the per-pair-wrap regime),
// and the second opinion on the GPU builder (host_neighbor_build = 1).  Engine::hostRebuild reads the positions back, calls
// buildHostLists and uploads the result; tests/host_lists_check.cpp calls it without a GPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <numeric>
#include <utility>
#include <vector>

namespace snb {

// a tile j entry: sorted index | image code << kJShiftBits, or -1 for a free slot; code = (ix + 2) * 25 + (iy + 2) * 5 + (iz + 2)
constexpr int kJShiftBits = 25, kJCodeCenter = 62;
struct Int2 { int32_t x, y; };
struct Int4 { int32_t x, y, z, w; };

// Sort-column geometry, shared by both builders.  ext: the rectangular domain the atoms are sorted in.  mesh: the Coulomb mesh when the
// columns should be whole mesh cells (>= 5 wide), so that the same sorted order feeds the brick-spreading kernel (pme.hip k_spreadBrick);
// mesh[0] == 0 asks for plain columns of about one block edge.
struct SortColumns { double aTarget; int ncx, ncy, colCells[2]; };
inline SortColumns sortColumns(int n, const double ext[3], const int mesh[3]) {
    SortColumns c;
    const double volume = ext[0] * ext[1] * ext[2];
    c.aTarget = std::cbrt(32.0 * volume / std::max(n, 1));
    c.ncx = std::max(1, std::min(2048, (int)std::lround(ext[0] / c.aTarget)));
    c.ncy = std::max(1, std::min(2048, (int)std::lround(ext[1] / c.aTarget)));
    c.colCells[0] = c.colCells[1] = 0;
    if (mesh[0] <= 0) return c;
    auto pick = [&](int m, double L) {
        int best = 0; double bestErr = 1e300;
        for (int d = 5; d <= 16 && d <= m; d++) if (m % d == 0) { double e = std::fabs(d * L / m - c.aTarget); if (e < bestErr) { bestErr = e; best = d; } }
        return best;
    };
    const int px = pick(mesh[0], ext[0]), py = pick(mesh[1], ext[1]);
    const size_t brickBytes = sizeof(double) * (size_t)px * py * mesh[2];
    if (px > 0 && py > 0 && brickBytes <= 60 * 1024 && std::max(mesh[0], std::max(mesh[1], mesh[2])) < 1024) {      // (the packed mesh cell of an atom holds 10 bits per axis)
        c.colCells[0] = px; c.colCells[1] = py; c.ncx = mesh[0] / px; c.ncy = mesh[1] / py; }
    return c;
}

struct HostListInput {
    int n = 0, nsub = 1; const int32_t* subset = nullptr;      // user order
    const double* pos = nullptr;                               // [n][3], user order, as read back
    double box[9] = {0}; bool periodic = false, noCutoff = false; double listRadius = 0;      // lower-triangular box; cutoff + padding
    int mesh[3] = {0, 0, 0};                                   // Coulomb mesh when sort columns are wanted (PME with a mesh of its own), else 0
    const int* exclStart = nullptr; const int* exclList = nullptr;      // exclusion CSR over user indices
    const int* slotOfSubset = nullptr;                         // grid slot per subset or -1
    int shardBegin = 0, shardEnd = 1, shardPeriod = 1;         // work items are kept for the i-blocks b with b % shardPeriod in [shardBegin, shardEnd)
};
struct HostLists {
    int npad = 0, numBlocks = 0, ncx = 1, ncy = 1, colCells[2] = {0, 0}; bool wrapMode = false;
    int64_t numTiles = 0, numMaskTiles = 0, shardTiles = 0;
    std::vector<int> sortedToUser, userToSorted, blockSubset, atomSubset, atomGrid, tileJ;      // sortedToUser: -1 for a padding slot
    std::vector<double> wrapped, imageOffset;      // [n][3] per USER atom: position in the primary cell, and wrapped - given
    std::vector<Int4> tileInfo;      // per tile: (slice, mask index or -1, j subset, 0)
    std::vector<Int2> blockTiles;    // per block: (first tile, tile count); the first tile is the diagonal one
    std::vector<Int4> workItems;     // (block, first tile, 1..8 tiles, block subset), longest first
    std::vector<Int2> colRange;      // with sort columns: sorted range [x, y) of every (subset, column)
    std::vector<uint32_t> masks;     // 32 rows per mask tile; a set bit removes the pair
};

inline bool ownsTile(int I, int J) { return ((I + J) & 1) ? (I > J) : (I < J); }      // which of two blocks lists the other

inline HostLists buildHostLists(const HostListInput& in) {
    HostLists L;
    const int N = in.n, nsub = in.nsub; const int32_t* subset = in.subset; const double* box = in.box; const double* hp = in.pos;
    const bool periodic = in.periodic, rect = box[3] == 0 && box[6] == 0 && box[7] == 0;
    const double R = in.noCutoff ? 1e300 : in.listRadius;
    // 1. wrap into the primary cell (fractional coordinates; lower-triangular box)
    std::vector<double> wp(hp, hp + (size_t)N * 3), off((size_t)N * 3, 0.0);      // (the lists grow in locals and are handed to L at the end)
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    if (periodic) {
        for (int i = 0; i < N; i++) {
            double* x = &wp[3 * (size_t)i];
            double s2 = std::floor(x[2] / box[8]); x[0] -= s2 * box[6]; x[1] -= s2 * box[7]; x[2] -= s2 * box[8];
            double s1 = std::floor(x[1] / box[4]); x[0] -= s1 * box[3]; x[1] -= s1 * box[4];
            double s0 = std::floor(x[0] / box[0]); x[0] -= s0 * box[0];
            for (int d = 0; d < 3; d++) off[3 * (size_t)i + d] = x[d] - hp[3 * (size_t)i + d];
        }
        lo[0] = lo[1] = lo[2] = 0; hi[0] = box[0]; hi[1] = box[4]; hi[2] = box[8];
        if (!rect) { lo[0] = std::min(0.0, box[3]) + std::min(0.0, box[6]); hi[0] = box[0] + std::max(0.0, box[3]) + std::max(0.0, box[6]); lo[1] = std::min(0.0, box[7]); hi[1] = box[4] + std::max(0.0, box[7]); }
    } else {
        for (int i = 0; i < N; i++) for (int d = 0; d < 3; d++) { lo[d] = std::min(lo[d], wp[3 * (size_t)i + d]); hi[d] = std::max(hi[d], wp[3 * (size_t)i + d]); }
        if (N == 0) { lo[0] = lo[1] = lo[2] = 0; hi[0] = hi[1] = hi[2] = 1; }
        for (int d = 0; d < 3; d++) { hi[d] += 1e-6 + 1e-9 * std::fabs(hi[d]); }
    }
    double ext[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    for (int d = 0; d < 3; d++) if (!(ext[d] > 1e-9)) ext[d] = 1e-9;
    // 2. sort: (subset, serpentine xy column, z up/down); mesh-commensurate columns on rectangular periodic cells only
    const int noMesh[3] = {0, 0, 0};
    const SortColumns sc = sortColumns(N, ext, (periodic && rect) ? in.mesh : noMesh);
    const double aTarget = sc.aTarget; const int ncx = L.ncx = sc.ncx, ncy = L.ncy = sc.ncy; L.colCells[0] = sc.colCells[0]; L.colCells[1] = sc.colCells[1];
    std::vector<uint64_t> key(N); std::vector<int> colOfAtom(N);
    for (int i = 0; i < N; i++) {
        const double* x = &wp[3 * (size_t)i];
        int cx = std::min(ncx - 1, std::max(0, (int)((x[0] - lo[0]) / ext[0] * ncx)));
        int cy = std::min(ncy - 1, std::max(0, (int)((x[1] - lo[1]) / ext[1] * ncy)));
        colOfAtom[i] = cx * ncy + cy;
        int col = cx * ncy + ((cx & 1) ? (ncy - 1 - cy) : cy);
        double zf = std::min(1.0, std::max(0.0, (x[2] - lo[2]) / ext[2]));
        if (col & 1) zf = 1.0 - zf;
        uint64_t zq = (uint64_t)(zf * 1048575.0);
        key[i] = ((uint64_t)subset[i] << 44) | ((uint64_t)col << 20) | zq;
    }
    std::vector<int> order(N); std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return key[a] != key[b] ? key[a] < key[b] : a < b; });
    // blocks of 32 sorted atoms of one subset; a subset's last block is filled up with padding slots (-1), so every block has real atoms
    std::vector<int> sortedToUser, userToSorted(N, -1), blkSubset;
    for (int s = 0, k = 0; s < nsub; s++) {
        size_t start = sortedToUser.size();
        while (k < N && subset[order[k]] == s) { userToSorted[order[k]] = (int)sortedToUser.size(); sortedToUser.push_back(order[k]); k++; }
        while ((sortedToUser.size() - start) % 32) sortedToUser.push_back(-1);
        for (size_t b = start / 32; b < sortedToUser.size() / 32; b++) blkSubset.push_back(s);
    }
    const int Npad = L.npad = (int)sortedToUser.size(), numBlocks = L.numBlocks = Npad / 32;
    if (L.colCells[0] > 0) {   // sorted range of every (subset, column): atoms of one column are contiguous in the sorted order
        const int ncol = ncx * ncy;
        L.colRange.assign((size_t)nsub * ncol, Int2{0, 0});
        for (int s = 0; s < Npad; s++) {
            const int u = sortedToUser[s]; if (u < 0) continue;
            Int2& rg = L.colRange[(size_t)subset[u] * ncol + colOfAtom[u]];
            if (rg.y == 0) rg.x = s;
            rg.y = s + 1;
        }
    }
    // 3. subset and grid slot of every sorted atom
    L.atomSubset.assign(Npad, -1); L.atomGrid.assign(Npad, -1);
    for (int s = 0; s < Npad; s++) { const int u = sortedToUser[s]; if (u >= 0) { L.atomSubset[s] = subset[u]; L.atomGrid[s] = in.slotOfSubset[subset[u]]; } }
    // 4. block bounding boxes (real atoms only)
    std::vector<double> bc((size_t)numBlocks * 3, 0.0), bh((size_t)numBlocks * 3, 0.0);
    double maxFullExt[3] = {0, 0, 0};
    for (int b = 0; b < numBlocks; b++) {
        double mn[3] = {1e300, 1e300, 1e300}, mx[3] = {-1e300, -1e300, -1e300};
        for (int k = 0; k < 32; k++) {
            int u = sortedToUser[b * 32 + k]; if (u < 0) continue;
            for (int d = 0; d < 3; d++) { mn[d] = std::min(mn[d], wp[3 * (size_t)u + d]); mx[d] = std::max(mx[d], wp[3 * (size_t)u + d]); }
        }
        for (int d = 0; d < 3; d++) { bc[3 * (size_t)b + d] = 0.5 * (mn[d] + mx[d]); bh[3 * (size_t)b + d] = 0.5 * (mx[d] - mn[d]); maxFullExt[d] = std::max(maxFullExt[d], mx[d] - mn[d]); }
    }
    // 5. tiles
    bool allPairs = in.noCutoff;
    if (periodic) {
        if (!rect) { L.wrapMode = true; allPairs = true; }
        else for (int d = 0; d < 3; d++) if (!(maxFullExt[d] + 2 * R < box[4 * d])) { L.wrapMode = true; allPairs = true; }
    }
    std::vector<int> hTileJ; std::vector<Int4> hTileInfo; std::vector<uint32_t> hMasks;
    L.blockTiles.resize(numBlocks);
    // cell grid over sorted real atoms (rectangular domains only; allPairs mode does not need it)
    int nc[3] = {1, 1, 1}; double csz[3] = {ext[0], ext[1], ext[2]}; std::vector<int> cellStart, cellAtoms;
    if (!allPairs) {
        const double target = std::max(aTarget, R / 3.0);
        for (int d = 0; d < 3; d++) { nc[d] = std::max(1, std::min(512, (int)(ext[d] / target))); csz[d] = ext[d] / nc[d]; }
        const size_t ncell = (size_t)nc[0] * nc[1] * nc[2];
        cellStart.assign(ncell + 1, 0);
        std::vector<int> cellOf(Npad, -1);
        for (int s = 0; s < Npad; s++) {
            int u = sortedToUser[s]; if (u < 0) continue;
            int c[3];
            for (int d = 0; d < 3; d++) c[d] = std::min(nc[d] - 1, std::max(0, (int)((wp[3 * (size_t)u + d] - lo[d]) / csz[d])));
            cellOf[s] = (c[0] * nc[1] + c[1]) * nc[2] + c[2];
            cellStart[cellOf[s] + 1]++;
        }
        for (size_t c = 0; c < ncell; c++) cellStart[c + 1] += cellStart[c];
        cellAtoms.resize(cellStart[ncell]);
        std::vector<int> fill(ncell, 0);
        for (int s = 0; s < Npad; s++) if (cellOf[s] >= 0) cellAtoms[cellStart[cellOf[s]] + fill[cellOf[s]]++] = s;
    }
    std::vector<int> slotOf(Npad, -1);            // sorted j index -> position in this block's candidate list
    std::vector<std::pair<int, int>> cand;        // (sorted j index, image code)
    // the mask rows of a tile, allotted when the tile gets its first masked entry (tileInfo.y: mask index or -1)
    auto maskRows = [&](int tile) { Int4& ti = hTileInfo[tile]; if (ti.y < 0) { ti.y = (int)(hMasks.size() / 32); hMasks.resize(hMasks.size() + 32, 0u); } return &hMasks[(size_t)ti.y * 32]; };
    for (int I = 0; I < numBlocks; I++) {
        cand.clear();
        const double* c = &bc[3 * (size_t)I]; const double* h = &bh[3 * (size_t)I];
        if (allPairs) {
            for (int J = 0; J < numBlocks; J++) {
                if (J == I || !ownsTile(I, J)) continue;
                for (int k = 0; k < 32; k++) if (sortedToUser[J * 32 + k] >= 0) cand.push_back({J * 32 + k, kJCodeCenter});
            }
        } else {
            int cmin[3], cmax[3];
            for (int d = 0; d < 3; d++) {
                cmin[d] = (int)std::floor((c[d] - h[d] - R - lo[d]) / csz[d]);
                cmax[d] = (int)std::floor((c[d] + h[d] + R - lo[d]) / csz[d]);
                if (!periodic) { cmin[d] = std::max(cmin[d], 0); cmax[d] = std::min(cmax[d], nc[d] - 1); }
            }
            for (int ix = cmin[0]; ix <= cmax[0]; ix++) for (int iy = cmin[1]; iy <= cmax[1]; iy++) for (int iz = cmin[2]; iz <= cmax[2]; iz++) {
                int cc[3] = {ix, iy, iz}, img[3] = {0, 0, 0};
                for (int d = 0; d < 3; d++) { img[d] = (int)std::floor((double)cc[d] / nc[d]); cc[d] -= img[d] * nc[d]; }
                if (std::abs(img[0]) > 1 || std::abs(img[1]) > 1 || std::abs(img[2]) > 1) continue;
                const double sh[3] = {img[0] * box[0], img[1] * box[4], img[2] * box[8]};
                const int code = (img[0] + 2) * 25 + (img[1] + 2) * 5 + (img[2] + 2);
                const int cell = (cc[0] * nc[1] + cc[1]) * nc[2] + cc[2];
                for (int a = cellStart[cell]; a < cellStart[cell + 1]; a++) {
                    const int sj = cellAtoms[a]; const int J = sj >> 5;
                    if (J == I || !ownsTile(I, J)) continue;
                    const int u = sortedToUser[sj];
                    double d2 = 0;
                    for (int d = 0; d < 3; d++) { double dd = std::fabs(wp[3 * (size_t)u + d] + sh[d] - c[d]) - h[d]; if (dd > 0) d2 += dd * dd; }
                    if (d2 < R * R) cand.push_back({sj, code});
                }
            }
        }
        // group by j subset, ascending index inside a group
        std::sort(cand.begin(), cand.end(), [&](const std::pair<int, int>& a, const std::pair<int, int>& b) {
            int sa = blkSubset[a.first >> 5], sb = blkSubset[b.first >> 5];
            return sa != sb ? sa < sb : a.first < b.first;
        });
        const int firstTile = (int)hTileInfo.size();
        // diagonal tile first: slots 0..31, keeps j > i only
        for (int k = 0; k < 32; k++) hTileJ.push_back((sortedToUser[I * 32 + k] >= 0) ? ((I * 32 + k) | (kJCodeCenter << kJShiftBits)) : -1);
        hTileInfo.push_back(Int4{blkSubset[I] * (blkSubset[I] + 3) / 2, -1, blkSubset[I], 0});      // (slice, mask, j subset)
        for (int i = 0; i < 32; i++) { uint32_t m = 0; for (int j = 0; j <= i; j++) m |= 1u << j; maskRows(firstTile)[i] = m; }
        for (int k = 0; k < 32; k++) slotOf[I * 32 + k] = k;
        size_t pos = 0;
        while (pos < cand.size()) {
            const int sjSub = blkSubset[cand[pos].first >> 5];
            int cnt = 0; const int tIndex = (int)hTileInfo.size() - firstTile;
            while (pos < cand.size() && cnt < 32 && blkSubset[cand[pos].first >> 5] == sjSub) {
                hTileJ.push_back(cand[pos].first | (cand[pos].second << kJShiftBits));
                slotOf[cand[pos].first] = tIndex * 32 + cnt;
                cnt++; pos++;
            }
            for (; cnt < 32; cnt++) hTileJ.push_back(-1);
            const int a = std::max(blkSubset[I], sjSub), b = std::min(blkSubset[I], sjSub);
            hTileInfo.push_back(Int4{a * (a + 1) / 2 + b, -1, sjSub, 0});
        }
        const int nTiles = (int)hTileInfo.size() - firstTile;
        // exclusion masks
        uint32_t iPadRows = 0;
        for (int k = 0; k < 32; k++) {
            int u = sortedToUser[I * 32 + k]; if (u < 0) { iPadRows |= 1u << k; continue; }
            for (int e = in.exclStart[u]; e < in.exclStart[u + 1]; e++) {
                const int sl = slotOf[userToSorted[in.exclList[e]]];
                if (sl >= 0) maskRows(firstTile + (sl >> 5))[k] |= 1u << (sl & 31);
            }
        }
        // padding slots (partially filled tiles, padded i rows) are masked out as well, so that parked padding
        // coordinates can never contribute (in the per-pair-wrap variant they would be folded back into the box)
        for (int t = 0; t < nTiles; t++) {
            uint32_t jPad = 0;
            for (int k = 0; k < 32; k++) if (hTileJ[(size_t)(firstTile + t) * 32 + k] == -1) jPad |= 1u << k;
            if (!jPad && !iPadRows) continue;
            uint32_t* rows = maskRows(firstTile + t);
            for (int k = 0; k < 32; k++) rows[k] |= ((iPadRows >> k) & 1u) ? 0xFFFFFFFFu : jPad;
        }
        // reset the scratch map
        for (int k = 0; k < 32; k++) slotOf[I * 32 + k] = -1;
        for (auto& cd : cand) slotOf[cd.first] = -1;
        L.blockTiles[I] = Int2{firstTile, nTiles};
    }
    L.numTiles = (int64_t)hTileInfo.size(); L.numMaskTiles = (int64_t)(hMasks.size() / 32);      // (every mask belongs to one tile)
    // work items: runs of <= 8 tiles of one i-block (fine grain => several rounds of waves per CU, small tail).  Sharded engines keep the
    // items of the i-blocks they own: a rule every rank evaluates identically, whatever order its own builder emitted the items in
    const int CH = 8;
    for (int b = 0; b < numBlocks; b++) {
        if (b % in.shardPeriod < in.shardBegin || b % in.shardPeriod >= in.shardEnd) continue;
        L.shardTiles += L.blockTiles[b].y;
        for (int o = 0; o < L.blockTiles[b].y; o += CH) L.workItems.push_back(Int4{b, L.blockTiles[b].x + o, std::min(CH, L.blockTiles[b].y - o), blkSubset[b]});
    }
    std::stable_sort(L.workItems.begin(), L.workItems.end(), [&](const Int4& a, const Int4& b) { return a.z > b.z; });
    L.wrapped = std::move(wp); L.imageOffset = std::move(off); L.sortedToUser = std::move(sortedToUser); L.userToSorted = std::move(userToSorted);
    L.blockSubset = std::move(blkSubset); L.tileJ = std::move(hTileJ); L.tileInfo = std::move(hTileInfo); L.masks = std::move(hMasks);
    return L;
}

}  // namespace snb
