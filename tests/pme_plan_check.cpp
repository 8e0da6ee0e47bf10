// CPU driver of csrc/pme_plan.h (tests/test_mesh_census.py builds it with g++ under ASan + UBSan and runs it once per census row and
// precision; no GPU, nothing loaded into python).  It plans one mesh the way the engine does -- planDims, sortColumns (host_lists.h),
// brickGeometry, ownSpreadMargin, ownSpread, planePath, zMix -- under the SNB_* switches of its own environment, and prints what the plan
// decides, one "<key> <value>" per line, the splits (fft, plane) in the words of the engine's SNB_VERBOSE mesh line.
//   pme_plan_check nx ny nz subsets realBytes Lx Ly Lz atoms padding
#include <cstdio>
#include <cstdlib>

#include "host_lists.h"
#include "pme_plan.h"

using namespace snb;

int main(int argc, char** argv) {
    if (argc != 11) { fprintf(stderr, "usage: %s nx ny nz subsets realBytes Lx Ly Lz atoms padding\n", argv[0]); return 2; }
    const int g[3] = {atoi(argv[1]), atoi(argv[2]), atoi(argv[3])};
    const int nsub = atoi(argv[4]);
    const size_t realBytes = (size_t)atoi(argv[5]);
    const double ext[3] = {atof(argv[6]), atof(argv[7]), atof(argv[8])};
    const int natoms = atoi(argv[9]);
    const double padding = atof(argv[10]);
    const Switches& sw = switches();
    for (int a = 0; a < 3; a++) if (legalGridSize(g[a]) != g[a]) { fprintf(stderr, "mesh size %d is not legal\n", g[a]); return 1; }
    PmePlanDims d;
    if (!planDims(g, realBytes, sw, d)) { fprintf(stderr, "mesh is not FFT-legal\n"); return 1; }
    printf("fft x %d*%d y %d*%d z %d*%d\n", d.rx1, d.rx2, d.ry1, d.ry2, d.rz1, d.rz2);
    printf("plane x %d*%d y %d*%d (%s)\n", d.px1, d.px2, d.py1, d.py2, (d.px1 <= 0 || d.py1 <= 0) ? "none" : planeIsStatic(d) ? "static" : "run-time");
    const SortColumns sc = sortColumns(natoms, ext, g);
    const BrickGeometry b = brickGeometry(d, d, sc.colCells, sw.brickGroup);      // (the Coulomb mesh: the sort columns are cut on this mesh)
    printf("cells %d %d\nbricks %d\ngroup %d %d\n", sc.colCells[0], sc.colCells[1], b.ok ? 1 : 0, b.gx, b.gy);
    const double box[9] = {ext[0], 0, 0, 0, ext[1], 0, 0, 0, ext[2]};
    double r[9];
    recipBoxRows(box, r);
    const int M = ownSpreadMargin(d, r, padding, sw);
    const OwnSpread o = b.ok ? ownSpread(d, b, nsub, realBytes, M, sw) : OwnSpread();
    printf("own %d\nslabs %d\nmargin %d\n", o.runs ? 1 : 0, o.slabs, M);
    printf("fuse %d\npath %s\n", (o.runs && o.fuse) ? 1 : 0, (o.runs && o.plane) ? "plane" : "three-pass");
    printf("merge_nt %d\nzmix_nt %d\nconvx_nt %d\nplane_nt %d\n", o.mergeThreads, zMix(d, nsub, sw).threads, convxThreads(d.rx1, d.rx2, realBytes), planePath(d, nsub, realBytes, sw).threads);
    return 0;
}
