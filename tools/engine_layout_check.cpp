// Stand-alone checks of the engine's host-side arithmetic (skirt_amd/csrc/host/engine_layout.cpp), no GPU and no
// HIP: tools/engine_layout_cpu.py builds this with the address and undefined-behaviour sanitizers from
// engine_layout.cpp and host/voronoi.cpp, tests/test_engine_layout.py runs it group by group.
//   engine_layout_check [pool|instruments|trees|leafmap|voronoi|labs|lds]...   (no argument: every group)
// Prints one line per group; exit status 1 with the failed condition's line if a check fails.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../skirt_amd/csrc/device/vor_terms.hpp"
#include "../skirt_amd/csrc/host/engine_layout.hpp"
#include "../skirt_amd/csrc/host/voronoi.hpp"

using namespace skirt_dev;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

namespace {

// ------------------------------------------------------------------ pool layout
struct Piece {
    uintptr_t at;
    size_t bytes, align;
};

void poolCase(size_t nslots, size_t ninstr, bool continuous, bool detPair, bool pol, int gridKind) {
    const size_t rayCap = poolRayCap(nslots, ninstr, continuous);
    CHECK(rayCap == nslots * (1 + ninstr) + (continuous ? nslots * kPathCap * ninstr : 0));
    const bool refs = poolRefs(continuous, gridKind);
    CHECK(refs == (!continuous && gridKind != SKIRT_GRID_VORONOI));
    const bool path = continuous && nslots > 0;
    Args counted{}, a{};
    const size_t bytes = poolLayout(nullptr, nslots, rayCap, refs, detPair, path, pol, counted);
    char* const base = reinterpret_cast<char*>(uintptr_t(1) << 20);  // an address as hipMalloc aligns it; never read
    CHECK(poolLayout(base, nslots, rayCap, refs, detPair, path, pol, a) == bytes);  // counted = carved
    const size_t ndet = (detPair ? 2 : 1) * (rayCap - nslots);
    std::vector<Piece> v;
    auto add = [&](const void* p, size_t n, size_t size, size_t align) { v.push_back({(uintptr_t)p, n * size, align}); };
    add(a.rays, rayCap, refs ? sizeof(RayRef) : sizeof(RayRec), 16);
    add(a.det, ndet, sizeof(DetRec), 16);
    for (double* d : {a.srx, a.sry, a.srz, a.skx, a.sky, a.skz, a.sL, a.sLth, a.resA, a.resB, a.resS, a.fuseU, a.fuseThr})
        add(d, nslots, 8, 8);
    if (pol) {
        add(a.detPol, ndet, sizeof(DetPol), 8);
        for (double* d : {a.sQ, a.sU, a.sV, a.snx, a.sny, a.snz}) add(d, nslots, 8, 8);
        add(a.spol, nslots, 4, 4);
    } else {
        CHECK(!a.detPol && !a.sQ && !a.sU && !a.sV && !a.snx && !a.sny && !a.snz && !a.spol);
    }
    for (int* d : {a.sell, a.snscatt, a.sstellar, a.sstate, a.svcell}) add(d, nslots, 4, 4);
    for (uint32_t* d : {a.splo, a.sphi, a.sblock, a.sw2, a.sw3, a.shave}) add(d, nslots, 4, 4);
    add(a.act[0], nslots, 4, 4);
    add(a.act[1], nslots, 4, 4);
    if (path) {
        add(a.pathBuf, nslots * kPathCap, sizeof(PathRec), 16);  // aligned again, within the spare
        add(a.pathCnt, nslots, 4, 4);
    } else {
        CHECK(!a.pathBuf && !a.pathCnt);
    }
    // in order, disjoint, aligned, inside the allocation of bytes + kPoolSpare
    uintptr_t end = (uintptr_t)base;
    size_t sum = 0;
    for (const Piece& p : v) {
        CHECK(p.at >= end);
        CHECK(p.at % p.align == 0);
        end = p.at + p.bytes;
        sum += p.bytes;
    }
    CHECK(sum == bytes);
    CHECK(end - (uintptr_t)base <= bytes + kPoolSpare);
    CHECK(end - (uintptr_t)base - bytes < 16);  // the one padding: the path records' alignment
}

void pool() {
    int n = 0;
    for (size_t nslots : {1, 3, 64, 1023, 32768})
        for (size_t ninstr : {0, 1, 3, 7})
            for (int continuous = 0; continuous < 2; continuous++)
                for (int detPair = 0; detPair < 2; detPair++)
                    for (int pol = 0; pol < 2; pol++)
                        for (int kind : {SKIRT_GRID_CARTESIAN, SKIRT_GRID_VORONOI}) {
                            poolCase(nslots, ninstr, continuous != 0, detPair != 0, pol != 0, kind);
                            n++;
                        }
    printf("pool: %d cases\n", n);
}

// ------------------------------------------------------------------ instrument layout
SkirtInstrDesc instrument(int kind, int levels) {
    SkirtInstrDesc d{};
    d.kind = kind;
    d.nx = 3;
    d.ny = 2;
    d.scattering_levels = levels;
    d.kobs[2] = 1.0;
    return d;
}

void instrumentsCase(const std::vector<SkirtInstrDesc>& in, int nlambda, bool pol) {
    InstrLayout lay;
    std::string err;
    CHECK(instrLayout(in.data(), (int)in.size(), nlambda, pol, lay, err) == SKIRT_OK);
    CHECK(lay.instr.size() == in.size());
    long long end = 0, used = 0;
    int sed = 0;
    for (size_t i = 0; i < in.size(); i++) {
        const DevInstr& d = lay.instr[i];
        const bool full = in[i].kind == SKIRT_INSTR_FULL;
        const int slots = full ? 5 + in[i].scattering_levels + (pol ? 3 : 0) : 1;
        CHECK(d.nslots == slots);
        CHECK(d.levels == (full ? in[i].scattering_levels : 0));
        CHECK(d.stokes == (full && pol ? 5 + in[i].scattering_levels : 0));
        CHECK(d.slotStride == (slots == 1 ? 1 : (slots + 7) / 8 * 8));
        CHECK(d.slotStride >= slots && (slots == 1 || d.slotStride % 8 == 0));
        CHECK(d.frameBase % 8 == 0);
        CHECK(d.frameBase >= end && d.frameBase - end < 8);
        const long long frames = in[i].kind == SKIRT_INSTR_SED ? 0 : (long long)d.slotStride * nlambda * 3 * 2;
        const long long seds = in[i].kind == SKIRT_INSTR_FRAME ? 0 : (long long)slots * nlambda;
        if (in[i].kind == SKIRT_INSTR_SED) CHECK(d.nx == 0 && d.ny == 0);
        CHECK(d.sedBase == d.frameBase + frames);  // disjoint: frames, then SEDs, then the next instrument
        end = d.sedBase + seds;
        used += frames + seds;
        CHECK(d.sedOff == sed);  // a running sum
        sed += (int)seds;
    }
    CHECK(lay.nInstrTally == (size_t)end);
    CHECK(end - used < 8 * (long long)in.size());  // the regions and the frames' alignment gaps make up the tally
    CHECK(lay.nsed == sed);
}

void instruments() {
    const std::vector<SkirtInstrDesc> a = {instrument(SKIRT_INSTR_FULL, 0), instrument(SKIRT_INSTR_FULL, 3),
                                           instrument(SKIRT_INSTR_SED, 0), instrument(SKIRT_INSTR_FRAME, 0)};
    const std::vector<SkirtInstrDesc> b = {a[2], a[1], a[3], a[0]};
    for (int pol = 0; pol < 2; pol++)
        for (const auto* order : {&a, &b}) instrumentsCase(*order, 5, pol != 0);
    InstrLayout lay;
    std::string err;
    SkirtInstrDesc bad = instrument(7, 0);
    CHECK(instrLayout(&bad, 1, 5, false, lay, err) == SKIRT_ERR_ARG && err == "bad instrument kind");
    bad = instrument(SKIRT_INSTR_FULL, 251);
    CHECK(instrLayout(&bad, 1, 5, false, lay, err) == SKIRT_ERR_ARG && err == "scattering levels out of range");
    CHECK(instrLayout(nullptr, 0, 5, false, lay, err) == SKIRT_OK && lay.instr.empty() && lay.nInstrTally == 0 && lay.nsed == 0);
    printf("instruments: 4 layouts, 2 refusals\n");
}

// ------------------------------------------------------------------ trees
struct Tree {
    std::vector<double> box;
    std::vector<int> fc, cn, nbrOffset;
    std::vector<signed char> dir;
    bool bin = false;
    int ncells = 0;
    SkirtGridDesc desc() {
        nbrOffset.assign(6 * fc.size() + 1, 0);
        SkirtGridDesc g{};
        g.kind = SKIRT_GRID_OCTREE;
        g.ncells = ncells;
        g.nnodes = (int)fc.size();
        g.box = box.data();
        g.first_child = fc.data();
        g.cellnumber = cn.data();
        g.nbr_offset = nbrOffset.data();
        g.search = SKIRT_TREE_TOPDOWN;
        g.split_dir = bin ? dir.data() : nullptr;
        return g;
    }
    void root() {
        box = {0, 0, 0, 1, 1, 1};
        fc = {-1};
        dir = {0};
    }
    // the children of `node`, split at the box's centre (Box::center); octree children in octant order (x, y, z bits)
    void subdivide(int node, int axis = -1) {
        fc[node] = (int)fc.size();
        if (axis >= 0) dir[node] = (signed char)axis;
        const double* b = &box[6 * (size_t)node];
        const double lo[3] = {b[0], b[1], b[2]}, hi[3] = {b[3], b[4], b[5]};
        for (int k = 0; k < (axis < 0 ? 8 : 2); k++) {
            double c[6] = {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]};
            for (int ax = 0; ax < 3; ax++) {
                if (axis >= 0 && ax != axis) continue;
                const int bit = axis < 0 ? (k >> ax) & 1 : k;
                const double mid = 0.5 * (lo[ax] + hi[ax]);
                if (bit) c[ax] = mid;
                else c[3 + ax] = mid;
            }
            box.insert(box.end(), c, c + 6);
            fc.push_back(-1);
            dir.push_back(0);
        }
    }
    void numberCells() {
        cn.assign(fc.size(), -1);
        ncells = 0;
        for (size_t l = 0; l < fc.size(); l++)
            if (fc[l] < 0) cn[l] = ncells++;
    }
};

Tree octree17() {  // the root and its child 3 subdivided: 17 nodes, 15 leaves, breadth-first
    Tree t;
    t.root();
    t.subdivide(0);
    t.subdivide(3);
    t.numberCells();
    return t;
}

void trees() {
    std::string err;
    std::vector<int> father;
    Tree t = octree17();
    SkirtGridDesc g = t.desc();
    CHECK(g.nnodes == 17 && g.ncells == 15);
    CHECK(checkTree(&g, father, err) == SKIRT_OK && father.empty());
    unsetenv("SKIRT_AMD_CELL_ALIGN");
    CellNumbering num;
    CHECK(numberTreeLeaves(&g, num, err) == SKIRT_OK);
    CHECK((int)num.devCell.size() == g.ncells && num.ndev >= g.ncells);
    std::set<int> seen(num.devCell.begin(), num.devCell.end());
    CHECK((int)seen.size() == g.ncells && *seen.begin() >= 0 && *seen.rbegin() < num.ndev);  // injective, in range
    for (int l = 0; l < g.nnodes; l++) {  // 8 sibling leaves: consecutive numbers from a multiple of 8
        const int fc = t.fc[l];
        if (fc < 0) continue;
        bool leaves = true;
        for (int k = 0; k < 8; k++) leaves = leaves && t.fc[fc + k] < 0;
        if (!leaves) continue;
        CHECK(num.devCell[t.cn[fc]] % 8 == 0);
        for (int k = 0; k < 8; k++) CHECK(num.devCell[t.cn[fc + k]] == num.devCell[t.cn[fc]] + k);
    }
    CHECK(num.devCell[t.cn[9]] % 8 == 0);  // (node 3's children are nodes 9 .. 16)
    CHECK(num.ndev > g.ncells);            // the alignment left a gap: three leaves precede node 3's group
    setenv("SKIRT_AMD_CELL_ALIGN", "0", 1);
    CHECK(numberTreeLeaves(&g, num, err) == SKIRT_OK && num.ndev == g.ncells);
    seen = std::set<int>(num.devCell.begin(), num.devCell.end());
    CHECK((int)seen.size() == g.ncells && *seen.begin() == 0 && *seen.rbegin() == g.ncells - 1);
    unsetenv("SKIRT_AMD_CELL_ALIGN");
    // the Bookkeeping search takes this tree (breadth-first) and gets the fathers
    g.search = SKIRT_TREE_BOOKKEEPING;
    CHECK(checkTree(&g, father, err) == SKIRT_OK && (int)father.size() == 17 && father[0] == -1 && father[8] == 0 && father[9] == 3);
    g.search = SKIRT_TREE_TOPDOWN;

    // a three-level k-d tree (x, then y, then z): 15 nodes, 8 leaves, no gaps
    Tree b;
    b.bin = true;
    b.root();
    b.subdivide(0, 0);
    for (int l = 1; l <= 2; l++) b.subdivide(l, 1);
    for (int l = 3; l <= 6; l++) b.subdivide(l, 2);
    b.numberCells();
    SkirtGridDesc gb = b.desc();
    CHECK(gb.nnodes == 15 && gb.ncells == 8);
    CHECK(checkTree(&gb, father, err) == SKIRT_OK);
    CHECK(numberTreeLeaves(&gb, num, err) == SKIRT_OK && num.ndev == 8);
    seen = std::set<int>(num.devCell.begin(), num.devCell.end());
    CHECK(seen.size() == 8 && *seen.begin() == 0 && *seen.rbegin() == 7);
    gb.search = SKIRT_TREE_BOOKKEEPING;
    CHECK(checkTree(&gb, father, err) == SKIRT_ERR_ARG && err == "Bookkeeping method is not compatible with binary tree");

    // the engine's refusals
    Tree twice = octree17();
    twice.cn[2] = twice.cn[1];
    SkirtGridDesc g2 = twice.desc();
    CHECK(checkTree(&g2, father, err) == SKIRT_OK);
    CHECK(numberTreeLeaves(&g2, num, err) == SKIRT_ERR_ARG && err == "octree cell number used twice");
    Tree range = octree17();
    range.fc[3] = 12;  // 12 + 8 > 17 nodes
    SkirtGridDesc g3 = range.desc();
    CHECK(checkTree(&g3, father, err) == SKIRT_ERR_ARG && err == "octree child index out of range");
    Tree order;  // ten nodes, the root's children from node 2: not the breadth-first numbering
    order.box.assign(60, 0.0);
    order.fc = {2, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    order.dir.assign(10, 0);
    order.numberCells();
    SkirtGridDesc g4 = order.desc();
    CHECK(checkTree(&g4, father, err) == SKIRT_OK);
    g4.search = SKIRT_TREE_BOOKKEEPING;
    CHECK(checkTree(&g4, father, err) == SKIRT_ERR_ARG && err == "octree not numbered breadth-first for the Bookkeeping search");
    printf("trees: octree of 17 nodes, k-d tree of 15, 4 refusals\n");
}

// ------------------------------------------------------------------ leaf-map plan
void leafmap() {
    unsetenv("SKIRT_AMD_LEAFMAP");
    Tree t = octree17();
    SkirtGridDesc g = t.desc();
    LeafMapPlan p = planLeafMapTables(&g, 16);
    CHECK(p.L == 2 && p.N == 4 && p.T.size() == 15);
    for (int ax = 0; ax < 3; ax++) {
        for (int j = 0; j <= 4; j++) CHECK(p.T[ax * 5 + j] == 0.25 * j);  // the boxes' edges
        CHECK(p.inv[ax] == 4.0 && p.origin[ax] == 0.0);
    }
    for (int l = 0; l < g.nnodes; l++)  // every box edge is a table entry
        for (int q = 0; q < 6; q++) {
            bool found = false;
            for (int j = 0; j <= 4; j++) found = found || t.box[6 * l + q] == p.T[(q % 3) * 5 + j];
            CHECK(found);
        }
    setenv("SKIRT_AMD_LEAFMAP", "0", 1);
    CHECK(planLeafMapTables(&g, 16).L < 0);
    unsetenv("SKIRT_AMD_LEAFMAP");
    CHECK(planLeafMapTables(&g, 1 << kLeafLevelShift).L < 0);  // the cell numbers would not fit the entries
    // one edge of one box 1 ulp off: no map
    for (int q : {6 * 10 + 0, 6 * 16 + 4, 6 * 5 + 3}) {
        Tree u = octree17();
        u.box[q] = std::nextafter(u.box[q], 2.0);
        SkirtGridDesc gu = u.desc();
        CHECK(planLeafMapTables(&gu, 16).L < 0);
    }
    // a chain of kMaxMapLevel subdivisions has a map, one more has none
    for (int depth : {kMaxMapLevel, kMaxMapLevel + 1}) {
        Tree c;
        c.root();
        int node = 0;
        for (int d = 0; d < depth; d++) {
            c.subdivide(node);
            node = c.fc[node];
        }
        c.numberCells();
        SkirtGridDesc gc = c.desc();
        const LeafMapPlan pc = planLeafMapTables(&gc, gc.ncells);
        if (depth <= kMaxMapLevel) CHECK(pc.L == depth && pc.N == 1 << depth);
        else CHECK(pc.L < 0);
    }
    printf("leafmap: L = 2 and N = 4 for the octree of 17 nodes, 3 moved edges, chains of %d and %d levels\n", kMaxMapLevel,
           kMaxMapLevel + 1);
}

// ------------------------------------------------------------------ Voronoi packing
bool sameBits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }

void voronoi() {
    // 27 sites jittered about a 3 x 3 x 3 lattice in the unit cube, and one exactly on the xmin wall
    std::vector<double> sites;
    uint64_t s = 88172645463325252ull;
    auto u01 = [&]() {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        return (double)(s >> 11) / 9007199254740992.0;
    };
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            for (int k = 0; k < 3; k++)
                for (int ax = 0; ax < 3; ax++) sites.push_back(((ax == 0 ? i : ax == 1 ? j : k) + 0.3 + 0.4 * u01()) / 3.0);
    sites.insert(sites.end(), {0.0, 0.52, 0.47});
    const int N = (int)sites.size() / 3, onWall = N - 1;
    skirt::VoronoiGrid vg;
    skirt::buildVoronoi(vg, sites, 0, 1, 0, 1, 0, 1);
    SkirtGridDesc g{};
    g.kind = SKIRT_GRID_VORONOI;
    g.ncells = N;
    g.site = vg.site.data();
    g.cell_nbr_offset = vg.nbrOffset.data();
    g.cell_nbr_list = vg.nbrList.data();
    g.cell_bbox = vg.bbox.data();
    const double ext[6] = {0, 0, 0, 1, 1, 1};
    std::memcpy(g.extent, ext, sizeof ext);
    g.eps = vg.eps;
    g.nblocks = vg.nb;
    g.block_offset = vg.blockOffset.data();
    g.block_list = vg.blockList.data();
    VoronoiPack P;
    std::string err;
    CHECK(packVoronoi(&g, P, err) == SKIRT_OK);
    CHECK(P.vorScale == 2.0);
    // the device numbering: a permutation, and sites and boxes in its order
    std::set<int> seen(P.devCell.begin(), P.devCell.end());
    CHECK((int)seen.size() == N && *seen.begin() == 0 && *seen.rbegin() == N - 1);
    CHECK((int)P.start.size() == N + 1 && P.start[0] == 0);
    CHECK(P.slots.size() == (size_t)P.start[N] + kVorPad);
    bool sawWall = false;
    for (int m = 0; m < N; m++) {
        const int d = P.devCell[m];
        const int cnt = g.cell_nbr_offset[m + 1] - g.cell_nbr_offset[m];
        const int padded = (cnt + kVorUnroll - 1) / kVorUnroll * kVorUnroll;
        CHECK(P.start[d + 1] - P.start[d] == kVorHead + padded);  // the header plus whole groups
        for (int q = 0; q < 3; q++) CHECK(P.site[3 * d + q] == g.site[3 * m + q]);
        for (int q = 0; q < 6; q++) CHECK(P.bbox[6 * d + q] == g.cell_bbox[6 * m + q]);
        const VorEntry* blk = P.slots.data() + P.start[d];
        double head[4];
        int ids[4];
        std::memcpy(head, blk, sizeof head);
        std::memcpy(ids, blk + 2, sizeof ids);
        CHECK(head[0] == g.site[3 * m] && head[1] == g.site[3 * m + 1] && head[2] == g.site[3 * m + 2] && head[3] == 0.0);
        CHECK(ids[0] == d && ids[1] == cnt);
        std::vector<float> off;
        for (int o = 0; o < padded; o++) {
            const float* F = reinterpret_cast<const float*>(blk + kVorHead + (o & ~1));
            const int h = o & 1;
            const float e[3] = {F[h], F[2 + h], F[4 + h]};
            int next;
            std::memcpy(&next, F + 6 + h, 4);
            if (o >= cnt) {  // the list's padding: NaN, no exit
                CHECK(std::isnan(e[0]) && std::isnan(e[1]) && std::isnan(e[2]) && next == -1);
                continue;
            }
            const int id = g.cell_nbr_list[g.cell_nbr_offset[m] + o];
            double n[3] = {0.0, 0.0, 0.0};
            if (id < 0) {
                const int axis = (-id - 1) / 2;
                const double w = ext[(-id - 1) % 2 ? 3 + axis : axis] - g.site[3 * m + axis];
                n[axis] = w != 0.0 ? 2.0 * w * P.vorScale : NAN;
                if (m == onWall && id == -1) {  // the site on its wall: a NaN offset, stored as the degenerate entry
                    CHECK(std::isnan(n[0]));
                    CHECK(e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f);
                    sawWall = true;
                }
                CHECK(next == id);
            } else {
                for (int q = 0; q < 3; q++) n[q] = (g.site[3 * id + q] - g.site[3 * m + q]) * P.vorScale;
                CHECK(next == P.start[P.devCell[id]]);
            }
            float want[3];
            vorRecipOffset(n[0], n[1], n[2], want);
            CHECK(sameBits(e[0], want[0]) && sameBits(e[1], want[1]) && sameBits(e[2], want[2]));
            off.insert(off.end(), e, e + 3);
        }
        float eA, eB, hA, hB;
        vorRecipErrorTerms(off.data(), cnt, 3, &eA, &eB);
        std::memcpy(&hA, &ids[2], 4);
        std::memcpy(&hB, &ids[3], 4);
        CHECK(sameBits(eA, hA) && sameBits(eB, hB));
    }
    CHECK(sawWall);
    for (int q = 0; q < kVorPad; q++) {  // the slots after the last block, as allocated: no neighbour
        const VorEntry& e = P.slots[(size_t)P.start[N] + q];
        CHECK(e.ox == 0.0f && e.oy == 0.0f && e.oz == 0.0f && e.next == -1);
    }
    const size_t nb3 = (size_t)vg.nb * vg.nb * vg.nb;
    const int nbl = vg.blockOffset[nb3];
    CHECK(nbl > 0 && (int)P.blocks.size() == nbl);
    for (int q = 0; q < nbl; q++) {
        const int m = vg.blockList[q];
        CHECK(P.blocks[q].id == P.devCell[m] && P.blocks[q].x == g.site[3 * m] && P.blocks[q].y == g.site[3 * m + 1] &&
              P.blocks[q].z == g.site[3 * m + 2]);
    }
    std::vector<int> none(N + 1, 0);  // a cell without neighbours is refused
    g.cell_nbr_offset = none.data();
    CHECK(packVoronoi(&g, P, err) == SKIRT_ERR_ARG && err == "Voronoi cell without neighbours");
    printf("voronoi: %d sites, %d slots, %d block entries\n", N, (int)P.slots.size(), nbl);
}

// ------------------------------------------------------------------ Labs addressing
LabsPlan labsOf(uint64_t elems, bool store, bool selfAbs, int want = SKIRT_OK) {
    LabsPlan p;
    std::string err;
    CHECK(planLabsMode(elems, store, selfAbs, p, err) == want);
    if (want) CHECK(err == "Labs table of 2^40 elements or more");
    return p;
}

void labs() {
    for (const char* v : {"SKIRT_AMD_LABS_HI", "SKIRT_AMD_LABS_GLOBAL", "SKIRT_AMD_LABS_COPIES"}) unsetenv(v);
    const uint64_t MiB = (1ull << 20) / 8;  // elements
    // a table of exactly 0xfffffff8 bytes: the buffer path; 8 bytes more: global atomics
    LabsPlan p = labsOf(0xfffffff8ull / 8, true, false);
    CHECK(!p.global && !p.hi && p.bytes == 0xfffffff8u && p.copies == 1);
    p = labsOf(0xfffffff8ull / 8 + 1, true, false);
    CHECK(p.global && !p.hi && p.bytes == 0 && p.copies == 1 && p.stride == 0);
    // 2^32 - 1 elements: 32-bit element indices; 2^32 + 1: the high-index path
    p = labsOf((1ull << 32) - 1, true, false);
    CHECK(p.global && !p.hi);
    p = labsOf((1ull << 32) + 1, true, false);
    CHECK(p.global && p.hi);
    CHECK(!labsOf((1ull << 32) + 1, false, false).hi);  // nothing stored: no mode to choose
    p = labsOf((1ull << 40) - 1, true, false);
    CHECK(p.global && p.hi);
    labsOf(1ull << 40, true, false, SKIRT_ERR_UNSUPPORTED);
    labsOf(1ull << 40, false, false);  // refused only where it is added to
    // replicas: 400 MiB (self-absorption 800 MiB) over the table's size, 1 .. 8
    struct { uint64_t mib; bool self; int copies; } rows[] = {{10, false, 8}, {50, false, 8}, {100, false, 4}, {129, false, 3},
                                                              {200, false, 2}, {201, false, 1}, {300, false, 1}, {100, true, 8},
                                                              {129, true, 6}, {400, true, 2}, {401, true, 1}, {900, true, 1}};
    for (const auto& r : rows) {
        p = labsOf(r.mib * MiB, true, r.self);
        CHECK(p.copies == r.copies);
        CHECK(p.stride == (r.copies > 1 ? (unsigned)(r.mib << 20) : 0u));
        CHECK(labsOf(r.mib * MiB, false, r.self).copies == 1);  // nothing stored: no replicas
    }
    p = labsOf(MiB + 1, true, false);  // the stride: the table rounded up to 256 bytes
    CHECK(p.copies == 8 && p.stride == (1u << 20) + 256 && p.bytes == (1u << 20) + 8);
    setenv("SKIRT_AMD_LABS_COPIES", "3", 1);
    CHECK(labsOf(300 * MiB, true, false).copies == 3);
    CHECK(labsOf(10 * MiB, true, true).copies == 3);
    CHECK(labsOf(1365 * MiB, true, false).copies == 3);   // 3 x 1365 MiB = 0xfff00000 <= 0xfffffff0
    CHECK(labsOf(1366 * MiB, true, false).copies == 1);   // past it: no replicas
    CHECK(labsOf(0xfffffff8ull / 8 + 1, true, false).copies == 1);  // a global table has none
    CHECK(labsOf(10 * MiB, false, false).copies == 1);
    setenv("SKIRT_AMD_LABS_COPIES", "1", 1);
    CHECK(labsOf(10 * MiB, true, false).copies == 1);
    setenv("SKIRT_AMD_LABS_COPIES", "65", 1);
    CHECK(labsOf(MiB, true, false).copies == 1);  // at most 64
    unsetenv("SKIRT_AMD_LABS_COPIES");
    setenv("SKIRT_AMD_LABS_GLOBAL", "1", 1);
    p = labsOf(10 * MiB, true, false);
    CHECK(p.global && !p.hi && p.bytes == 0 && p.copies == 1);
    unsetenv("SKIRT_AMD_LABS_GLOBAL");
    setenv("SKIRT_AMD_LABS_HI", "1", 1);
    p = labsOf(10 * MiB, true, false);
    CHECK(p.global && p.hi && p.copies == 1);
    unsetenv("SKIRT_AMD_LABS_HI");
    printf("labs: thresholds at 0xfffffff8 bytes, 2^32 and 2^40 elements; %d replica rows\n", (int)(sizeof rows / sizeof rows[0]));
}

// ------------------------------------------------------------------ LDS
LdsPlan ldsOf(const LdsInputs& in, int want = SKIRT_OK, std::string* msg = nullptr) {
    LdsPlan p;
    std::string err;
    CHECK(planLdsLayout(in, p, err) == want);
    if (msg) *msg = err;
    return p;
}

void lds() {
    unsetenv("SKIRT_AMD_DET_COPIES");
    unsetenv("SKIRT_AMD_NO_NOSTORE");
    const size_t labsBufs = (size_t)kLabsBuf * kBlock * 12;
    LdsInputs in;
    in.meshWords = 7; in.ncomp = 3; in.nlambda = 5; in.ninstr = 2; in.nsed = 40; in.store = true; in.budget = 160 * 1024;
    LdsPlan p = ldsOf(in);
    const int instrWords = (int)(sizeof(DevInstr) / 8);
    CHECK(p.meshOff == 0 && p.optOff == 8 && p.instrOff == 8 + 60 && p.sedOff == 68 + 2 * instrWords);  // 7 rounded to 8
    CHECK(p.optOff % 2 == 0 && p.instrOff % 2 == 0);
    CHECK(!p.noStore);
    CHECK(p.trace == 68 * 8 + (size_t)kSegWords * 8 + labsBufs);
    CHECK(p.event == (size_t)p.sedOff * 8 && p.detCopies == 8 && p.detect == p.event + 8 * 40 * 8);
    in.labsHi = true;
    CHECK(ldsOf(in).trace == p.trace + (size_t)kLabsBuf * kBlock);
    in.labsHi = false;
    in.meshWords = 0; in.treeWords = 3 * 5; in.ncomp = 1;  // a leaf map's tables: 15 rounded to 16; 4 x 1 x 5 = 20 words
    p = ldsOf(in);
    CHECK(p.optOff == 16 && p.instrOff == 36);
    // noStore: nothing stored, one component, no continuous scattering, no Voronoi grid, not switched off
    in.store = false;
    p = ldsOf(in);
    CHECK(p.noStore && p.trace == 36 * 8 + (size_t)kSegWords * 8);
    in.store = true;      CHECK(!ldsOf(in).noStore); in.store = false;
    in.ncomp = 2;         CHECK(!ldsOf(in).noStore); in.ncomp = 1;
    in.continuous = true; CHECK(!ldsOf(in).noStore); in.continuous = false;
    in.voronoi = true;    CHECK(!ldsOf(in).noStore); in.voronoi = false;
    setenv("SKIRT_AMD_NO_NOSTORE", "1", 1);
    p = ldsOf(in);
    CHECK(!p.noStore && p.trace == 36 * 8 + (size_t)kSegWords * 8 + labsBufs);
    unsetenv("SKIRT_AMD_NO_NOSTORE");
    CHECK(ldsOf(in).noStore);
    // the budget: tables that fill it exactly fit, one double more is refused with both numbers
    in.store = true; in.ninstr = 0; in.nsed = 0; in.treeWords = 0; in.meshWords = 1000;
    p = ldsOf(in);
    in.budget = p.trace;
    CHECK(ldsOf(in).trace == in.budget);
    in.budget = p.trace - 8;
    std::string msg;
    ldsOf(in, SKIRT_ERR_UNSUPPORTED, &msg);
    CHECK(msg == "grid and optical tables do not fit in LDS (" + std::to_string(p.trace) + " of " + std::to_string(p.trace - 8) +
                     " bytes)");
    in.store = false;  // the event kernel's tables alone can be what does not fit
    in.ninstr = 63; in.budget = 4096 + 8 * 1000;
    p = ldsOf(in, SKIRT_ERR_UNSUPPORTED, &msg);
    CHECK(msg.find(" of 12096 bytes)") != std::string::npos);
    // the detect kernel's SED copies: as many of 8, 4, 2, 1 as fit beside the event tables, else none
    in = LdsInputs{};
    in.ncomp = 1; in.nlambda = 5; in.ninstr = 1; in.store = true; in.budget = 160 * 1024;
    struct { int nsed, copies; } rows[] = {{0, 8}, {2000, 8}, {2500, 8}, {2600, 4}, {5000, 4}, {5200, 2}, {10000, 2}, {10400, 1},
                                           {20000, 1}, {20500, 0}, {40000, 0}};
    for (const auto& r : rows) {
        in.nsed = r.nsed;
        p = ldsOf(in);
        CHECK(p.detCopies == r.copies);
        CHECK(p.detect == p.event + (size_t)r.copies * r.nsed * 8 && p.detect <= in.budget);
        if (r.copies < 8) CHECK(p.event + (size_t)(r.copies ? 2 * r.copies : 1) * r.nsed * 8 > in.budget);  // the next step up does not fit
    }
    setenv("SKIRT_AMD_DET_COPIES", "2", 1);
    in.nsed = 100;    CHECK(ldsOf(in).detCopies == 2);
    in.nsed = 10400;  CHECK(ldsOf(in).detCopies == 1);
    setenv("SKIRT_AMD_DET_COPIES", "0", 1);
    in.nsed = 100;
    p = ldsOf(in);
    CHECK(p.detCopies == 0 && p.detect == p.event);
    setenv("SKIRT_AMD_DET_COPIES", "5", 1);  // between two steps: the step below
    CHECK(ldsOf(in).detCopies == 4);
    unsetenv("SKIRT_AMD_DET_COPIES");
    printf("lds: offsets, the no-store choice, the budget's refusal, %d rows of SED copies\n", (int)(sizeof rows / sizeof rows[0]));
}

}  // namespace

int main(int argc, char** argv) {
    const struct { const char* name; void (*run)(); } groups[] = {{"pool", pool},       {"instruments", instruments}, {"trees", trees},
                                                                  {"leafmap", leafmap}, {"voronoi", voronoi},         {"labs", labs},
                                                                  {"lds", lds}};
    for (int i = 1; i < argc; i++) {
        bool known = false;
        for (const auto& g : groups) known = known || std::string(argv[i]) == g.name;
        if (!known) {
            printf("unknown group %s\n", argv[i]);
            return 2;
        }
    }
    for (const auto& g : groups) {
        bool wanted = argc < 2;
        for (int i = 1; i < argc; i++) wanted = wanted || std::string(argv[i]) == g.name;
        if (wanted) g.run();
    }
    return 0;
}
