// Stand-alone driver of the host neighbour-list builder (csrc/host_lists.h) for tests/test_host_lists_cpu.py: reads one system from a
// raw binary file, calls snb::buildHostLists and writes every list back as raw arrays.  No GPU, no HIP; built with ASan + UBSan.
//
//   in : int32[12] = n, nsub, periodic, noCutoff, mesh[3], shardBegin, shardEnd, shardPeriod, nExcl, 0
//        double[10] = box[9], listRadius;  int32 subset[n];  double pos[3n];  int32 exclStart[n+1], exclList[nExcl], slotOfSubset[nsub]
//   out: int64[16] = npad, numBlocks, ncx, ncy, colCells[2], wrapMode, numTiles, numMaskTiles, shardTiles, numWorkItems, nColRange, nMaskWords, 0...
//        double wrapped[3n], imageOffset[3n];  int32 sortedToUser[npad], userToSorted[n], blockSubset[numBlocks], atomSubset[npad],
//        atomGrid[npad], tileJ[32 numTiles], tileInfo[4 numTiles], blockTiles[2 numBlocks], workItems[4 numWorkItems], colRange[2 nColRange];
//        uint32 masks[nMaskWords]
#include "host_lists.h"

#include <cstdio>
#include <stdexcept>

template <typename T> static std::vector<T> readArray(FILE* f, size_t count) {
    std::vector<T> v(count);
    if (count > 0 && fread(v.data(), sizeof(T), count, f) != count) throw std::runtime_error("input file is too short");
    return v;
}
template <typename T> static void writeArray(FILE* f, const T* p, size_t count) {
    if (count > 0 && fwrite(p, sizeof(T), count, f) != count) throw std::runtime_error("cannot write the output file");
}
template <typename T> static void writeArray(FILE* f, const std::vector<T>& v) { writeArray(f, v.data(), v.size()); }

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s input.bin output.bin\n", argv[0]); return 2; }
    try {
        FILE* f = fopen(argv[1], "rb");
        if (!f) throw std::runtime_error("cannot open the input file");
        const std::vector<int32_t> head = readArray<int32_t>(f, 12);
        const std::vector<double> real = readArray<double>(f, 10);
        const int n = head[0], nsub = head[1], nExcl = head[10];
        if (n < 0 || nsub < 1 || nExcl < 0) throw std::runtime_error("bad header");
        const std::vector<int32_t> subset = readArray<int32_t>(f, n);
        const std::vector<double> pos = readArray<double>(f, (size_t)3 * n);
        const std::vector<int32_t> exclStart = readArray<int32_t>(f, (size_t)n + 1), exclList = readArray<int32_t>(f, nExcl), slot = readArray<int32_t>(f, nsub);
        fclose(f);
        if (exclStart[n] != nExcl) throw std::runtime_error("exclusion CSR does not end at nExcl");

        snb::HostListInput in;
        in.n = n; in.nsub = nsub; in.subset = subset.data(); in.pos = pos.data();
        for (int i = 0; i < 9; i++) in.box[i] = real[i];
        in.periodic = head[2] != 0; in.noCutoff = head[3] != 0; in.listRadius = real[9];
        for (int d = 0; d < 3; d++) in.mesh[d] = head[4 + d];
        in.exclStart = exclStart.data(); in.exclList = exclList.data(); in.slotOfSubset = slot.data();
        in.shardBegin = head[7]; in.shardEnd = head[8]; in.shardPeriod = head[9];
        const snb::HostLists L = snb::buildHostLists(in);

        FILE* o = fopen(argv[2], "wb");
        if (!o) throw std::runtime_error("cannot open the output file");
        const int64_t oh[16] = {L.npad, L.numBlocks, L.ncx, L.ncy, L.colCells[0], L.colCells[1], L.wrapMode ? 1 : 0, L.numTiles, L.numMaskTiles, L.shardTiles,
                                (int64_t)L.workItems.size(), (int64_t)L.colRange.size(), (int64_t)L.masks.size(), 0, 0, 0};
        writeArray(o, oh, 16);
        writeArray(o, L.wrapped); writeArray(o, L.imageOffset);
        writeArray(o, L.sortedToUser); writeArray(o, L.userToSorted); writeArray(o, L.blockSubset); writeArray(o, L.atomSubset); writeArray(o, L.atomGrid); writeArray(o, L.tileJ);
        static_assert(sizeof(snb::Int4) == 16 && sizeof(snb::Int2) == 8, "written as raw int32");
        writeArray(o, L.tileInfo); writeArray(o, L.blockTiles); writeArray(o, L.workItems); writeArray(o, L.colRange); writeArray(o, L.masks);
        if (fclose(o) != 0) throw std::runtime_error("cannot write the output file");
    } catch (const std::exception& e) { fprintf(stderr, "host_lists_check: %s\n", e.what()); return 1; }
    return 0;
}
