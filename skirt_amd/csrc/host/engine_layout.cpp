// The engine's host-side arithmetic (engine_layout.hpp): plain C++ on plain arrays, no HIP.
#include "engine_layout.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "../device/vor_terms.hpp"

namespace skirt_dev {

int envInt(const char* name, int dflt) {
    const char* s = getenv(name);
    return s ? atoi(s) : dflt;
}

bool cellAlign() {
    const char* env = getenv("SKIRT_AMD_CELL_ALIGN");
    return !(env && env[0] == '0');
}

size_t poolRayCap(size_t nslots, size_t ninstr, bool continuous) {
    return nslots * (1 + ninstr) + (continuous ? nslots * kPathCap * ninstr : 0);
}

// slot pool: the ray queue, SoA packet state, per-slot results and two active lists of nslots slots
// With continuous scattering every slot may also queue one peel-off per instrument and recorded path
// segment in one iteration, and keeps the dust segments of its last path (kPathCap each).
//
// The pool's layout, written once: poolLayout hands out the arrays from `base` in this order and returns the
// bytes they take; with a null base it only counts them (ensurePool). The records of 16-byte alignment come
// first, from the allocation's start, each a whole number of 16-byte chunks; then the arrays of doubles, then
// the 4-byte ones. The path records are aligned again: that padding comes out of the kPoolSpare bytes.
// The ray queue holds rayCap records of the phase's format: references (refs, kRayRefs) or whole records.
static_assert(sizeof(RayRec) % 16 == 0 && alignof(RayRec) == 16 && sizeof(RayRef) % 16 == 0 && alignof(RayRef) == 16 &&
                  sizeof(DetRec) % 16 == 0 && alignof(DetRec) == 16 && alignof(PathRec) <= 16,
              "pool order: ray records, detection records, 8-byte arrays, 4-byte arrays, aligned path records");
size_t poolLayout(char* base, size_t nslots, size_t rayCap, bool refs, bool detPair, bool path, bool pol, Args& a) {
    char* p = base;
    size_t bytes = 0;
    auto take = [&](auto*& d, size_t count) {
        using T = std::remove_reference_t<decltype(*d)>;
        d = reinterpret_cast<T*>(p);
        if (base) p += count * sizeof(T);
        bytes += count * sizeof(T);
    };
    if (refs) {
        RayRef* queue = nullptr;
        take(queue, rayCap);
        a.rays = reinterpret_cast<RayRec*>(queue);
    } else {
        take(a.rays, rayCap);
    }
    // at most one peel-off per instrument and slot per iteration, in one region or one per iteration parity
    take(a.det, (detPair ? 2 : 1) * (rayCap - nslots));
    for (double** d : {&a.srx, &a.sry, &a.srz, &a.skx, &a.sky, &a.skz, &a.sL, &a.sLth, &a.resA, &a.resB, &a.resS, &a.fuseU,
                       &a.fuseThr})
        take(*d, nslots);
    // a polarised simulation: the detection records' Stokes parameters and, per slot, the packet's Stokes vector,
    // normal and flag (52 bytes per slot); nothing otherwise, so that the other arrays lie where they did
    a.detPol = nullptr;
    a.sQ = a.sU = a.sV = a.snx = a.sny = a.snz = nullptr;
    a.spol = nullptr;
    if (pol) {
        take(a.detPol, (detPair ? 2 : 1) * (rayCap - nslots));
        for (double** d : {&a.sQ, &a.sU, &a.sV, &a.snx, &a.sny, &a.snz}) take(*d, nslots);
        take(a.spol, nslots);
    }
    for (int** d : {&a.sell, &a.snscatt, &a.sstellar, &a.sstate, &a.svcell}) take(*d, nslots);
    for (uint32_t** d : {&a.splo, &a.sphi, &a.sblock, &a.sw2, &a.sw3, &a.shave}) take(*d, nslots);
    take(a.act[0], nslots);
    take(a.act[1], nslots);
    a.pathBuf = nullptr;
    a.pathCnt = nullptr;
    if (path) {
        p = reinterpret_cast<char*>(((uintptr_t)p + 15) & ~(uintptr_t)15);
        take(a.pathBuf, nslots * kPathCap);
        take(a.pathCnt, nslots);
    }
    return bytes;
}

static int failed(std::string& err, int code, const std::string& msg) {
    err = msg;
    return code;
}

// The instruments' device descriptors and where their frames and SEDs lie in the global tally and in the LDS sums
int instrLayout(const SkirtInstrDesc* in, int n, int nlambda, bool pol, InstrLayout& out, std::string& err) {
    out.instr.clear();
    long long off = 0;
    int sedOff = 0;
    for (int i = 0; i < n; i++) {
        DevInstr d{};
        d.kind = in[i].kind;
        if (d.kind < SKIRT_INSTR_FULL || d.kind > SKIRT_INSTR_FRAME) return failed(err, SKIRT_ERR_ARG, "bad instrument kind");
        d.nx = in[i].nx;
        d.ny = in[i].ny;
        if (d.kind != SKIRT_INSTR_SED && (d.nx < 1 || d.ny < 1)) return failed(err, SKIRT_ERR_ARG, "bad instrument frame size");
        if (d.kind == SKIRT_INSTR_SED) { d.nx = 0; d.ny = 0; }
        d.levels = d.kind == SKIRT_INSTR_FULL ? in[i].scattering_levels : 0;
        if (d.levels < 0 || d.levels > 250) return failed(err, SKIRT_ERR_ARG, "scattering levels out of range");
        d.nslots = d.kind == SKIRT_INSTR_FULL ? 5 + d.levels : 1;
        // a polarised simulation's FullInstrument: Stokes Q, U, V after the scattering levels
        if (d.kind == SKIRT_INSTR_FULL && pol) {
            d.stokes = d.nslots;
            d.nslots += 3;
        }
        for (int q = 0; q < 3; q++) d.kobs[q] = in[i].kobs[q];
        d.sinphi = in[i].sinphi; d.cosphi = in[i].cosphi; d.sintheta = in[i].sintheta; d.costheta = in[i].costheta;
        d.sinpa = in[i].sinpa; d.cospa = in[i].cospa;
        d.xpmin = in[i].xpmin; d.xpsiz = in[i].xpsiz; d.ypmin = in[i].ypmin; d.ypsiz = in[i].ypsiz;
        d.slotStride = d.nslots == 1 ? 1 : (d.nslots + 7) / 8 * 8;
        // every frame starts on a 64-byte line (the tally itself is at least 256-byte aligned), so that a
        // detection's slots (slotStride 8) share one line and one atomic request also after another
        // instrument's SEDs
        off = (off + 7) & ~7LL;
        d.frameBase = off;
        const long long nframes = (d.kind == SKIRT_INSTR_SED) ? 0 : (long long)d.slotStride * nlambda * d.nx * d.ny;
        off += nframes;
        d.sedBase = off;
        const long long nseds = (d.kind == SKIRT_INSTR_FRAME) ? 0 : (long long)d.nslots * nlambda;
        off += nseds;
        d.sedOff = sedOff;
        sedOff += (int)nseds;
        out.instr.push_back(d);
    }
    out.nInstrTally = (size_t)off;
    out.nsed = sedOff;
    return SKIRT_OK;
}

int checkTree(const SkirtGridDesc* g, std::vector<int>& father, std::string& err) {
    if (g->nnodes < 1 || !g->box || !g->first_child || !g->cellnumber || !g->nbr_offset)
        return failed(err, SKIRT_ERR_ARG, "bad octree grid");
    // validate the index arrays so that the kernels never read out of bounds
    const bool bin = g->split_dir != nullptr;
    const int arity = bin ? 2 : 8;
    int nleaf = 0;
    for (int l = 0; l < g->nnodes; l++) {
        const int fc = g->first_child[l];
        if (fc >= 0 && (fc + arity > g->nnodes || fc <= l)) return failed(err, SKIRT_ERR_ARG, "octree child index out of range");
        if (fc >= 0 && bin && (g->split_dir[l] < 0 || g->split_dir[l] > 2)) return failed(err, SKIRT_ERR_ARG, "bad k-d tree split axis");
        if (fc < 0) {
            if (g->cellnumber[l] < 0 || g->cellnumber[l] >= g->ncells) return failed(err, SKIRT_ERR_ARG, "octree cell number out of range");
            nleaf++;
        }
    }
    if (nleaf != g->ncells) return failed(err, SKIRT_ERR_ARG, "octree leaf count != ncells");
    const int nnbr = g->nbr_offset[6 * (size_t)g->nnodes];
    for (size_t q = 0; q < 6 * (size_t)g->nnodes; q++)
        if (g->nbr_offset[q] < 0 || g->nbr_offset[q] > g->nbr_offset[q + 1]) return failed(err, SKIRT_ERR_ARG, "bad neighbor offsets");
    for (int q = 0; q < nnbr; q++)
        if (g->nbr_list[q] < 0 || g->nbr_list[q] >= g->nnodes) return failed(err, SKIRT_ERR_ARG, "neighbor index out of range");
    if (g->search < SKIRT_TREE_TOPDOWN || g->search > SKIRT_TREE_BOOKKEEPING) return failed(err, SKIRT_ERR_ARG, "bad tree search method");
    father.clear();
    if (g->search == SKIRT_TREE_BOOKKEEPING) {
        // the Bookkeeping search reads octants off the breadth-first numbering: every group of
        // children must start at an id = 1 (mod 8) (TreeDustGrid.cpp:525)
        if (bin) return failed(err, SKIRT_ERR_ARG, "Bookkeeping method is not compatible with binary tree");
        father.assign(g->nnodes, -1);
        for (int l = 0; l < g->nnodes; l++) {
            const int fc = g->first_child[l];
            if (fc < 0) continue;
            if ((fc - 1) % 8 != 0) return failed(err, SKIRT_ERR_ARG, "octree not numbered breadth-first for the Bookkeeping search");
            for (int k = 0; k < 8; k++) father[fc + k] = l;
        }
    }
    return SKIRT_OK;
}

// Morton order of the leaves: depth-first, children in octant order (x, y, z bits). A ray crosses
// about 2.5 of the 8 children of a node it enters, so 8 sibling leaves are numbered from a
// multiple of 8 (one 64-byte line of every Labs row), leaving unused device cells before them:
// the ray's Labs adds into them then share one atomic request (SKIRT_AMD_CELL_ALIGN=0: no gaps).
int numberTreeLeaves(const SkirtGridDesc* g, CellNumbering& out, std::string& err) {
    out.devCell.assign(g->ncells, -1);
    const int arity = g->split_dir ? 2 : 8;
    const bool align = arity == 8 && cellAlign();
    std::vector<int> stack{0};
    int next = 0, used = 0;
    auto number = [&](int l) -> bool {
        if (out.devCell[g->cellnumber[l]] >= 0) return false;
        out.devCell[g->cellnumber[l]] = next++;
        used++;
        return true;
    };
    while (!stack.empty()) {
        const int l = stack.back();
        stack.pop_back();
        const int fc = g->first_child[l];
        if (fc < 0) {
            if (!number(l)) return failed(err, SKIRT_ERR_ARG, "octree cell number used twice");
            continue;
        }
        bool leaves = align;
        for (int k = 0; k < arity && leaves; k++) leaves = g->first_child[fc + k] < 0;
        if (leaves) {  // the sibling leaves, aligned: the same depth-first order
            next = (next + 7) & ~7;
            for (int k = 0; k < arity; k++)
                if (!number(fc + k)) return failed(err, SKIRT_ERR_ARG, "octree cell number used twice");
        } else {
            for (int k = arity - 1; k >= 0; k--) stack.push_back(fc + k);
        }
    }
    if (used != g->ncells) return failed(err, SKIRT_ERR_ARG, "octree leaves do not cover the cells");
    out.ndev = next;
    return SKIRT_OK;
}

// Decides whether the octree can be walked through a leaf map (Grid<SKIRT_GRID_OCTREE>): every node
// box must equal the box its level and integer coordinates give in the per-axis split tables, and the
// tree must be at most kMaxMapLevel deep. Returns the tables, or no map (L < 0); the map itself is built at the
// first phase (it caches the densities). SKIRT_AMD_LEAFMAP=0 forces the node-array walk.
LeafMapPlan planLeafMapTables(const SkirtGridDesc* g, int ndev) {
    LeafMapPlan none, plan;
    const char* env = getenv("SKIRT_AMD_LEAFMAP");
    if (env && env[0] == '0') return none;
    const bool bin = g->split_dir != nullptr;
    if (ndev >= (int)(1u << (bin ? kBinCellBits : kLeafLevelShift))) return none;
    const int maxL = bin ? kMaxBinMapLevel : kMaxMapLevel;
    struct Item { int node, lv[3], idx[3]; };  // per-axis depth and integer coordinate
    std::vector<Item> stack{{0, {0, 0, 0}, {0, 0, 0}}};
    std::vector<Item> nodes;
    nodes.reserve(g->nnodes);
    int L = 0;
    while (!stack.empty()) {
        const Item it = stack.back();
        stack.pop_back();
        nodes.push_back(it);
        L = std::max(L, std::max(it.lv[0], std::max(it.lv[1], it.lv[2])));
        if (L > maxL) return none;
        const int fc = g->first_child[it.node];
        if (fc < 0) continue;
        if (bin) {
            const int d = g->split_dir[it.node];
            for (int k = 0; k < 2; k++) {
                Item ch = it;
                ch.node = fc + k;
                ch.lv[d]++;
                ch.idx[d] = 2 * it.idx[d] + k;
                stack.push_back(ch);
            }
        } else {
            for (int k = 0; k < 8; k++) {
                Item ch;
                ch.node = fc + k;
                for (int ax = 0; ax < 3; ax++) {
                    ch.lv[ax] = it.lv[ax] + 1;
                    ch.idx[ax] = 2 * it.idx[ax] + ((k >> ax) & 1);
                }
                stack.push_back(ch);
            }
        }
    }
    if ((int)nodes.size() != g->nnodes) return none;  // not a tree reachable from node 0
    const int N = 1 << L;
    std::vector<double> T(3 * (size_t)(N + 1));
    for (int ax = 0; ax < 3; ax++) {
        double* t = T.data() + ax * (N + 1);
        t[0] = g->box[ax];
        t[N] = g->box[3 + ax];
        for (int w = N; w > 1; w >>= 1)  // Box::center of every node, coarse to fine
            for (int lo = 0; lo < N; lo += w) t[lo + w / 2] = 0.5 * (t[lo] + t[lo + w]);
        for (int j = 0; j < N; j++)
            if (!(t[j] < t[j + 1])) return none;
    }
    for (const Item& it : nodes) {
        const double* b = g->box + 6 * (size_t)it.node;
        for (int ax = 0; ax < 3; ax++) {
            const int sh = L - it.lv[ax];
            const double* t = T.data() + ax * (N + 1);
            if (b[ax] != t[it.idx[ax] << sh] || b[3 + ax] != t[(it.idx[ax] + 1) << sh]) return none;
        }
    }
    plan.L = L;
    plan.N = N;
    for (int ax = 0; ax < 3; ax++) plan.inv[ax] = N / (g->box[3 + ax] - g->box[ax]);
    for (int ax = 0; ax < 3; ax++) plan.origin[ax] = T[ax * (N + 1)];
    plan.T = std::move(T);
    return plan;
}

// device cell numbers in Morton order of the sites (21 bits per axis, ties by reference number):
// cells adjacent in space are adjacent in memory, for the neighbour lists, the densities and the
// Labs tallies alike. Every list keeps its reference order (first-minimum choices depend on it).
static void numberVoronoiCells(const SkirtGridDesc* g, std::vector<int>& devCell) {
    const int N = g->ncells;
    devCell.assign(N, 0);
    std::vector<std::pair<uint64_t, int>> key(N);
    const double ext[3] = {g->extent[3] - g->extent[0], g->extent[4] - g->extent[1], g->extent[5] - g->extent[2]};
    const double lo[3] = {g->extent[0], g->extent[1], g->extent[2]};
    for (int m = 0; m < N; m++) {
        uint64_t code = 0;
        for (int d = 0; d < 3; d++) {
            const double f = (g->site[3 * (size_t)m + d] - lo[d]) / ext[d];
            const uint64_t u = (uint64_t)std::max(0.0, std::min(2097151.0, f * 2097152.0));
            for (int bit = 0; bit < 21; bit++) code |= ((u >> bit) & 1ull) << (3 * bit + (2 - d));
        }
        key[m] = {code, m};
    }
    std::sort(key.begin(), key.end());
    for (int q = 0; q < N; q++) devCell[key[q].second] = q;
}

// The Voronoi grid as the device holds it: the cells renumbered, their sites and boxes in device order, every cell's
// block of slots (see VorEntry) and the block lists with the cells' sites
int packVoronoi(const SkirtGridDesc* g, VoronoiPack& out, std::string& err) {
    const int N = g->ncells;
    if (N < 1 || !g->site || !g->cell_nbr_offset || !g->cell_nbr_list || !g->cell_bbox || g->nblocks < 1 ||
        !g->block_offset || !g->block_list)
        return failed(err, SKIRT_ERR_ARG, "bad Voronoi grid");
    if (N > kCellMaskOut) return failed(err, SKIRT_ERR_UNSUPPORTED, "more than 2^28 Voronoi cells");
    const int nnbr = g->cell_nbr_offset[N];
    for (int m = 0; m < N; m++)
        if (g->cell_nbr_offset[m] < 0 || g->cell_nbr_offset[m] > g->cell_nbr_offset[m + 1])
            return failed(err, SKIRT_ERR_ARG, "bad Voronoi neighbour offsets");
    for (int q = 0; q < nnbr; q++)
        if (g->cell_nbr_list[q] < -6 || g->cell_nbr_list[q] >= N) return failed(err, SKIRT_ERR_ARG, "Voronoi neighbour out of range");
    const size_t nb3 = (size_t)g->nblocks * g->nblocks * g->nblocks;
    const int nbl = g->block_offset[nb3];
    for (int q = 0; q < nbl; q++)
        if (g->block_list[q] < 0 || g->block_list[q] >= N) return failed(err, SKIRT_ERR_ARG, "Voronoi block list out of range");
    const double gx0 = g->extent[0], gy0 = g->extent[1], gz0 = g->extent[2];
    const double gx1 = g->extent[3], gy1 = g->extent[4], gz1 = g->extent[5];
    std::vector<int>& devCell = out.devCell;
    numberVoronoiCells(g, devCell);
    std::vector<int> refOf(N);
    for (int m = 0; m < N; m++) refOf[devCell[m]] = m;
    std::vector<double> site(3 * (size_t)N), bbox(6 * (size_t)N);
    // each device cell's block: kVorHead header slots + one slot per neighbour, in pairs (see VorEntry);
    // the array is padded by kVorPad slots, since a step loads whole groups of entries
    std::vector<int> start(N + 1, 0);
    for (int d = 0; d < N; d++) {
        const int m = refOf[d];
        const int cnt = g->cell_nbr_offset[m + 1] - g->cell_nbr_offset[m];
        if (cnt < 1) return failed(err, SKIRT_ERR_ARG, "Voronoi cell without neighbours");
        // whole groups of kVorUnroll entries (even)
        const int per = kVorUnroll;
        start[d + 1] = start[d] + kVorHead + (cnt + per - 1) / per * per;
    }
    if ((size_t)start[N] + kVorPad >= (size_t)INT32_MAX) return failed(err, SKIRT_ERR_UNSUPPORTED, "Voronoi mesh too large");
    std::vector<VorEntry> slots((size_t)start[N] + kVorPad, VorEntry{0.f, 0.f, 0.f, -1});
    // offsets in units of the domain's largest half-width: single-precision squares stay in range
    const double vorScale = out.vorScale = 2.0 / std::max({gx1 - gx0, gy1 - gy0, gz1 - gz0});
    for (int d = 0; d < N; d++) {
        const int m = refOf[d];
        const double* sm = g->site + 3 * (size_t)m;
        for (int q = 0; q < 3; q++) site[3 * (size_t)d + q] = sm[q];
        for (int q = 0; q < 6; q++) bbox[6 * (size_t)d + q] = g->cell_bbox[6 * (size_t)m + q];
        VorEntry* blk = slots.data() + start[d];
        const double head[4] = {sm[0], sm[1], sm[2], 0.0};  // rho of component 0: set by upload_media
        std::memcpy(blk, head, sizeof head);
        const int cnt = g->cell_nbr_offset[m + 1] - g->cell_nbr_offset[m];
        std::vector<float> off(3 * (size_t)cnt);
        int o = 0;
        for (int q = g->cell_nbr_offset[m]; q < g->cell_nbr_offset[m + 1]; q++, o++) {
            const int id = g->cell_nbr_list[q];
            VorEntry e;
            if (id < 0) {
                // a wall (-1 xmin, -2 xmax, ... -6 zmax) is the bisector plane of the site and its mirror
                // image: the offset to the mirror site along the wall's axis (NaN when the site lies on
                // the wall, which vorRecipOffset stores as the degenerate entry 0: the step then evaluates the
                // list exactly)
                const int axis = (-id - 1) / 2;
                const double lim[6] = {gx0, gx1, gy0, gy1, gz0, gz1};
                const double w = lim[-id - 1] - sm[axis];
                double n[3] = {0.0, 0.0, 0.0};
                n[axis] = w != 0.0 ? 2.0 * w * vorScale : NAN;
                float o[3];
                vorRecipOffset(n[0], n[1], n[2], o);  // m = n / |n|^2 (vor_terms.hpp)
                e = VorEntry{o[0], o[1], o[2], id};
            } else {
                const double* si = g->site + 3 * (size_t)id;
                float o[3];
                vorRecipOffset((si[0] - sm[0]) * vorScale, (si[1] - sm[1]) * vorScale,
                               (si[2] - sm[2]) * vorScale, o);
                e = VorEntry{o[0], o[1], o[2], start[devCell[id]]};
            }
            // entry o in its pair (see VorEntry): {ox0, ox1, oy0, oy1} {oz0, oz1, next0, next1}
            float* P = reinterpret_cast<float*>(blk + kVorHead + (o & ~1));
            const int h = o & 1;
            P[h] = e.ox; P[2 + h] = e.oy; P[4 + h] = e.oz;
            std::memcpy(P + 6 + h, &e.next, 4);
            off[3 * (size_t)o] = e.ox; off[3 * (size_t)o + 1] = e.oy; off[3 * (size_t)o + 2] = e.oz;
        }
        // the padding up to the next block: NaN entries, no exit for any direction (bounds())
        for (int q = cnt; q < start[d + 1] - start[d] - kVorHead; q++) {
            float* P = reinterpret_cast<float*>(blk + kVorHead + (q & ~1));
            const int h = q & 1;
            P[h] = P[2 + h] = P[4 + h] = NAN;
            const int none = -1;
            std::memcpy(P + 6 + h, &none, 4);
        }
        // the header's last words: id, count and the cell's error terms of the bounds (vor_terms.hpp)
        float eA, eB;
        vorRecipErrorTerms(off.data(), cnt, 3, &eA, &eB);
        int ids[4] = {d, cnt, 0, 0};
        std::memcpy(&ids[2], &eA, 4);
        std::memcpy(&ids[3], &eB, 4);
        std::memcpy(blk + 2, ids, sizeof ids);
    }
    std::vector<BlockSite> blocks(std::max(nbl, 1), BlockSite{0.0, 0.0, 0.0, -1, 0});
    for (int q = 0; q < nbl; q++) {
        const int m = g->block_list[q];
        blocks[q] = BlockSite{g->site[3 * (size_t)m], g->site[3 * (size_t)m + 1], g->site[3 * (size_t)m + 2], devCell[m], 0};
    }
    out.site = std::move(site);
    out.bbox = std::move(bbox);
    out.start = std::move(start);
    out.slots = std::move(slots);
    out.blocks = std::move(blocks);
    return SKIRT_OK;
}

// the Labs addressing mode and replicas of a phase whose table holds labsElems elements
int planLabsMode(uint64_t labsElems, bool store, bool selfAbsorption, LabsPlan& out, std::string& err) {
    // the trace kernel adds to Labs through a buffer descriptor (32-bit byte offsets, one byte past the end
    // for the drain's empty lanes) while the table holds at most 4 GiB - 8 (e.g. 2^21 cells x 255
    // wavelengths), with global atomics beyond (SKIRT_AMD_LABS_GLOBAL=1 forces them: tests)
    // 2^32 elements or more (32 GiB): the buffered adds carry 40-bit element indices (SKIRT_AMD_LABS_HI=1 forces
    // that path: tests); 2^40 elements at most
    if (store && labsElems >= (1ull << 40)) return failed(err, SKIRT_ERR_UNSUPPORTED, "Labs table of 2^40 elements or more");
    const bool forceHi = envInt("SKIRT_AMD_LABS_HI", 0) != 0;
    out.hi = (store && (forceHi || labsElems > 0xffffffffull)) ? 1 : 0;
    const bool forceGlobal = envInt("SKIRT_AMD_LABS_GLOBAL", 0) != 0;
    out.global = (forceGlobal || out.hi || labsElems * sizeof(double) > 0xfffffff8ull) ? 1 : 0;
    out.bytes = out.global ? 0u : (unsigned)(labsElems * sizeof(double));
    // The trace waves add into K replicas of the table (wave w into w % K), folded into it at the phase end:
    // the adds to one cell spread over K lines, which the memory-side atomic unit works on side by side.
    // In the stellar phase the replicas pay while they stay near the MALL (256 MB): C3 (a 129 MB table) 2:
    // +1.1 %, 3: +1.2 %, 4: +0.8 %, 6: -1 %, 8: -3.4 %; C2 (21 MB) 4: +2 %, 8: +3.3 %. The self-absorption
    // cycles' adds crowd onto fewer lines and gain up to 6: C5 with 3 in the stellar phase and 6 in the
    // cycles +9.0 % against none, +3.6 % against 2 everywhere; C3 +1.2 % (profiles/r05_labs_copies_ab.txt).
    // K = 400 MiB (self-absorption: 800 MiB) / the table, at most 8; SKIRT_AMD_LABS_COPIES sets it (1: none)
    out.copies = 1;
    out.stride = 0;
    const uint64_t tableBytes = (uint64_t)out.bytes > 0 ? (uint64_t)out.bytes : 1;
    const uint64_t budget = selfAbsorption ? (800ull << 20) : (400ull << 20);
    const int Kauto = (int)std::min<uint64_t>(8, std::max<uint64_t>(1, budget / tableBytes));
    const int K = envInt("SKIRT_AMD_LABS_COPIES", Kauto);
    const uint64_t stride = ((uint64_t)out.bytes + 255) & ~255ull;
    if (store && !out.global && K > 1 && K <= 64 && stride * (uint64_t)K <= 0xfffffff0ull) {
        out.copies = K;
        out.stride = (unsigned)stride;
    }
    return SKIRT_OK;
}

// the LDS layout of a phase (Args::lds*Off, Args::detCopies), the LDS sizes and the no-store choice
int planLdsLayout(const LdsInputs& in, LdsPlan& out, std::string& err) {
    // LDS layout (doubles): mesh | optics | instruments | SED sums
    int off = 0;
    out.meshOff = off;
    off += in.meshWords;
    off += in.treeWords;
    off = (off + 1) & ~1;
    out.optOff = off;
    off += 4 * in.ncomp * in.nlambda;
    off = (off + 1) & ~1;
    out.instrOff = off;
    off += in.ninstr * (int)(sizeof(DevInstr) / sizeof(double));
    out.sedOff = off;
    off += in.nsed;
    // a phase storing no absorption with one component runs traceKernelNoStore (no Labs buffers)
    const bool noStore = out.noStore = !in.store && in.ncomp == 1 && !in.continuous && !in.voronoi &&
                         !getenv("SKIRT_AMD_NO_NOSTORE");
    const size_t ldsTrace = out.trace = (size_t)out.instrOff * sizeof(double)            // grid tables + optics
                            + (size_t)kSegWords * sizeof(double)                          // + segment counts
                            + (noStore ? 0 : (size_t)kLabsBuf * kBlock * (sizeof(double) + sizeof(unsigned)))  // + Labs buffers
                            + (in.labsHi ? (size_t)kLabsBuf * kBlock : 0);  // + their high index bytes
    const size_t ldsEvent = out.event = (size_t)out.sedOff * sizeof(double);              // + instruments
    // budget: what one workgroup may allocate (160 KiB on gfx950). The trace and event kernels need their
    // tables; the detect kernel keeps as many SED copies as fit (8, 4, 2, 1), or none (SEDs to the tally)
    const size_t budget = in.budget;
    if (ldsTrace > budget || ldsEvent > budget)
        return failed(err, SKIRT_ERR_UNSUPPORTED, "grid and optical tables do not fit in LDS (" +
                                                      std::to_string(std::max(ldsTrace, ldsEvent)) + " of " +
                                                      std::to_string(budget) + " bytes)");
    // SKIRT_AMD_DET_COPIES caps the copies (tests of the fallbacks)
    const int capCopies = envInt("SKIRT_AMD_DET_COPIES", kDetectCopies);
    out.detCopies = kDetectCopies;
    while (out.detCopies > 0 && out.detCopies > capCopies) out.detCopies >>= 1;
    while (out.detCopies > 0 && ldsEvent + (size_t)out.detCopies * in.nsed * sizeof(double) > budget) out.detCopies >>= 1;
    out.detect = ldsEvent + (size_t)out.detCopies * in.nsed * sizeof(double);
    return SKIRT_OK;
}

}  // namespace skirt_dev
