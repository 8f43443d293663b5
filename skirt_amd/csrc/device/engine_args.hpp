// What the engine's two halves share: the constants, the records of the pool and the queues, the grid tables'
// formats and the kernels' argument structs. Plain types only: device/engine.hip (hipcc) and the host sources
// host/engine_*.cpp (the host compiler, no device compiler needed) include the same text, so both see one set of
// types in skirt_dev. The kernels themselves live in engine.hip's anonymous namespace; the host side reaches
// them through device/engine_launch.hpp.
#ifndef SKIRT_AMD_DEVICE_ENGINE_ARGS_HPP
#define SKIRT_AMD_DEVICE_ENGINE_ARGS_HPP

#include <stddef.h>
#include <stdint.h>

#include "../../../include/skirt_mcrt.h"
#include "particle_density.hpp"

#define SKIRT_HIDDEN __attribute__((visibility("hidden")))  // not among the library's dynamic symbols
#if defined(__HIPCC__)
#define SKIRT_ARGS_FN __host__ __device__ __forceinline__
#else
#define SKIRT_ARGS_FN SKIRT_HIDDEN inline
#endif

namespace skirt_dev {

constexpr int kBlock = 256;
constexpr int kSegWords = 3 * (kBlock / 64) * 4 / 8;  // the trace kernel's per-wave segment counts, in doubles
#ifndef SKIRT_LABS_BUF
#define SKIRT_LABS_BUF 16
#endif
constexpr int kLabsBuf = SKIRT_LABS_BUF;  // buffered Labs adds per trace lane (LDS)
// device counters of the pipeline (Args::ctr): 16, each on a 128-byte line of its own (kCtrStride words
// apart). The event kernel's block reservations add to four of them every round; packed in one line, those
// atomics serialized on it: C3 +2.1 %, C2 +6.9 %, C4 +0.5 % apart (profiles/r05_ctr_lines_ab.txt)
constexpr int kCtrStride = 32;
// which counter is which. The ones "by parity" are pairs: + Args::parity is this iteration's, + 1 - parity the
// next one's, which the kernels of this iteration already append to or reset
enum Ctr : int {
    CTR_RAYS = 0,      // by parity: rays queued from the bottom of the ray queue
    CTR_ACTIVE = 2,    // by parity: entries of the active slot list Args::act
    CTR_PULL = 4,      // the trace kernel's pull counter: queue ids handed out in this launch
    CTR_DET = 5,       // by parity: detection records
    CTR_RESERVED = 7,  // reserved
    CTR_WALK = 8,      // by parity: WALK rays, queued from the top of the ray queue (Args::walkBack)
    CTR_COUNT = 16     // 10 .. 15 reserved
};
constexpr int kCtrWords = CTR_COUNT * kCtrStride;
#define CTR(base, k) ((base)[(k) * kCtrStride])
#define CTRP(base, k) ((base) + (k) * kCtrStride)
constexpr const char* kGeomCapMessage =
    "a TorusGeometry or ConicalShellGeometry found no position in 65536 attempts";
constexpr int kSersicTable = 202;  // SersicFunction: 101 radii, then 101 cumulative masses
constexpr int kDetectCopies = 8;   // most LDS copies of the SED sums in the detect kernel (one per 8 lanes)
constexpr int kPollEvery = 1;      // iterations between two counter copies
constexpr int kPollRing = 3;       // copies in flight (the host reads each kPollRing copies late)

// ------------------------------------------------------------------ descriptors
struct DevInstr {
    int kind, nx, ny, nslots, levels, sedOff;  // sedOff: offset of this instrument's SEDs in the LDS sums
    int slotStride, stokes;                     // frames: slots per pixel, padded (see frameAt); the first of the
                                                //   Stokes Q, U, V slots of a polarised simulation (0: none)
    long long frameBase;                        // offset of the frames in the global instrument tally
    long long sedBase;                          // offset of the SEDs in the global instrument tally
    double kobs[3];
    double sinphi, cosphi, sintheta, costheta, sinpa, cospa;
    double xpmin, xpsiz, ypmin, ypsiz;
};

// One queued ray, written by the event kernel (or the continuous peel-off kernel) and pulled by the trace
// kernel, which enters the grid when it pulls the ray (the path before the grid, the first cell): that lookup
// then overlaps with the other lanes' steps instead of stalling the event kernel, whose waves are few and long.
// The reciprocal direction is computed by the trace kernel (three divisions per ray).
//
// The queue has two formats, chosen per phase (kRayRefs in engine.hip):
//
// RayRef, 16 bytes, one store: every grid the trace kernel enters itself, without continuous scattering. A ray
// starts where its slot's packet is, and the event kernel stores that state (Events::store) in the same visit,
// untouched until the slot's next visit; so the record only names the slot and the trace lane reads the rest
// there (Tracer::load): the origin from srx/sry/srz[slot]; a FILL/WALK direction from skx/sky/skz[slot], a
// peel-off's from its instrument (Args::instr, kobs); a FILL ray's luminosity from sL[slot], its fused deviate
// and threshold from fuseU/fuseThr[slot]; a queued WALK ray's optical depth from fuseU[slot] (the FILL that
// used it is over). A peel-off's luminosity lives in its detection record only. Against the 80-byte record
// this takes 2 x 64 bytes per slot visit off the event kernel's stores, written at a 160-byte lane stride.
//
// RayRec, 80 bytes = 5 x 16-byte chunks: Voronoi grids, whose rays the event kernel enters (kEnterInEvent: s0
// then holds the path length before the grid, ci/cj the first cell, per ray, peel-offs included), and
// continuous scattering, whose peel-offs start at points of the path and not where the packet is.
struct __attribute__((aligned(16))) RayRef {
    int idx;               // FILL/WALK: slot; PEEL: detection record
    unsigned flags;        // as RayRec::flags
    int slot;              // the packet's slot, for all three modes
    int spare;
};
static_assert(sizeof(RayRef) == 16, "ray reference layout");
struct __attribute__((aligned(16))) RayRec {
    double x, y, z;        // c0-c1: start point
    double dx, dy, dz;     // c1-c2: direction
    double s0;             // c3: path length before the grid (Voronoi) | a fused FILL ray's termination threshold | 0
    double param;          // c3: FILL: packet luminosity L; WALK: optical depth to reach; PEEL: peel-off L
    int idx;               // c4: FILL/WALK: slot; PEEL: detection record
    unsigned flags;        // c4: mode | cat << 2 | instrument << 4 | scattering level << 10 | ell << 18
    int ci, cj;            // c4: Voronoi: first cell and where its block starts | a fused FILL ray's deviate (Args::fuseU)
};
static_assert(sizeof(RayRec) == 80, "ray record layout");

// continuous scattering (MonteCarloSimulation::continuouspeeloffscattering): the dust segments of a FILL
// ray's path as DustGridPath holds them -- where the segment starts along the path (s, tau) and its
// lengths (ds, dtau) -- recorded by the trace kernel for the peel-off kernel, at most kPathCap per path
struct PathRec {
    double s0, ds, tau0, dtau;
    int m, pad;
};
constexpr int kPathCap = 2048;
constexpr int kContSlots = 1 << 15;  // packet slots in flight with continuous scattering (ray queue sizing)
enum ErrorBits : unsigned { ERR_TAU = 1u, ERR_PATH_CAP = 2u, ERR_QUEUE = 4u, ERR_GEOM = 8u };

// a ray entered by the event kernel carries the number of its segments before the grid in the top bits
// of its first cell (Voronoi device cells < 2^28)
constexpr int kOutsideShift = 28;
constexpr int kCellMaskOut = (1 << kOutsideShift) - 1;

// the detection of one peel-off ray, in a compact array of its own (the detect kernel reads only these,
// contiguously, instead of scanning every ray record): written by the event kernel, tau by the trace
// kernel
struct __attribute__((aligned(16))) DetRec {
    double Lp;             // peel-off luminosity
    double tau;            // optical depth to the grid edge
    int l;                 // frame pixel (-1: none)
    unsigned flags;        // as the ray's flags
};
static_assert(sizeof(DetRec) == 24 || sizeof(DetRec) == 32, "detection record layout");
// beside it in a polarised phase, in an array of its own: Q/I, U/I, V/I of the peel-off (0 for an emission peel-off)
struct DetPol {
    double Q, U, V;
};

// Voronoi cells on the device: per cell a block of 16-byte slots, contiguous, in device cell order: a
// 48-byte header {exact site x, y | z, rho of component 0 | device cell number, neighbour count, the
// bounds' error terms eA, eB (vor_terms.hpp)} followed by one 16-byte slot per neighbour, in the reference's
// list order: the neighbour's site relative to the cell's site, scaled by Args::vorScale and rounded to
// float (an approximate bisector plane), and where the neighbour's block starts (walls: -1 xmin .. -6
// zmax). The entries are stored in pairs, component-interleaved: slots {ox0, ox1, oy0, oy1} and {oz0, oz1,
// next0, next1}, so that the two 16-byte loads of a pair hand the packed (v_pk_*) arithmetic its operand
// pairs directly; a list of odd length ends in an unused half pair. A step bounds every plane distance from
// the float offsets, and evaluates the reference's exact expression only for the winner (from the winner's
// header, which is the next step's first load) or, when the bounds cannot single one out, for every
// possible winner.
// one entry of a Voronoi block list (Box::cellindices): the device cell and its exact site, so that cellIndex
// reads a candidate in one round trip (two 16-byte loads) instead of the list entry, then the site
struct alignas(16) BlockSite {
    double x, y, z;
    int id, pad;
};
static_assert(sizeof(BlockSite) == 32, "block site layout");

struct alignas(16) VorEntry {
    float ox, oy, oz;
    int next;
};
constexpr int kVorHead = 3;  // header slots

// Voronoi walk: entries per load group, even (pairs); with exp(-tau) per FILL segment 4 is best (C4 7.30e7;
// 6: 7.26e7 with 28 B/lane spilled; one group of 8: 7.25e7; profiles/r03_vor_pipe.txt, r03_exact_attenuation.txt)
constexpr int kVorUnroll = 4;
// groups of entries in flight per step: loaded with the header, each reloaded once consumed. 3: C4 trace
// launch 23.64 -> 23.19 ms, 9.64e7 -> 9.89e7 pkt/s, profiles/r04_ktrace_groups_nolicm.txt; 4 with each
// cell's list padded to whole groups with NaN entries (no per-entry count check): 1.0155e8 -> 1.0243e8
// (profiles/r04_vor_groups4.txt). Measured and removed (git history): the neighbour-parallel drain step
// (profiles/r03_vor_wide.txt), the drain split around the step's loads (profiles/r04_c4_variants.txt).
#ifndef SKIRT_VOR_GROUPS
#define SKIRT_VOR_GROUPS 4
#endif
constexpr int kVorGroups = SKIRT_VOR_GROUPS;
// slots after the last cell's block: a step loads whole groups of entries past its list
constexpr int kVorPad = (kVorGroups + 2) * kVorUnroll;

// grid kinds of the kernels: SKIRT_GRID_CARTESIAN, SKIRT_GRID_OCTREE (leaf-map walk), the k-d tree
// through its leaf map, and any tree walked through the node arrays (trees deeper than the leaf maps
// allow or not split at box centres, e.g. barycentric subdivision)
constexpr int kOctreeNodes = 16;
constexpr int kBinTreeMap = 17;
constexpr int kOctreeBookkeeping = 18;  // octree, Bookkeeping search (node arrays)

struct LeafEntry;

struct Args {
    // grid
    int nx, ny, nz, ncells;
    int brick;                   // Cartesian: device cells numbered in 2x2x2 bricks (see Grid<CARTESIAN>::dev)
    int labsStride;              // Labs row length (device cells, padded to a 64-byte line)
    const double* mesh;          // Cartesian borders x | y | z (staged in LDS)
    double gx0, gx1, gy0, gy1, gz0, gz1;
    const double* box;           // octree
    const int* firstChild;
    const signed char* splitDir;  // binary trees: split axis per node (null for octrees)
    const int* father;            // octree, Bookkeeping search: father of every node (-1 for the root)
    const int* cellnumber;
    const int* nbrOffset;
    const int* nbrList;
    double eps;
    int search;
    const double* site;          // Voronoi, device cell order: 3 per cell
    const int* vorStart;         // Voronoi: where each device cell's block of slots starts
    const VorEntry* vorSlots;    // Voronoi: headers and neighbour entries
    float vorScale;              // Voronoi: 1 / (largest half-width of the domain), the entries' offset unit
    const double* cellBbox;      // Voronoi: enclosing box per cell
    const int* devCell;          // reference cell -> device cell (Voronoi launches)
    int vnb;                     // Voronoi block grid: blocks per axis
    const int* blockOffset;
    const struct BlockSite* blockSites;  // Voronoi: the block lists, each entry with its cell's exact site
    const LeafEntry* leafMap;       // octree leaf map: Morton-ordered finest-level cells -> leaf
    const double* treeT;         // octree split coordinates per axis, 3 x (mapN + 1) (staged in LDS)
    int mapL, mapN;              // leaf map depth and 2^depth
    double mapInvX, mapInvY, mapInvZ;
    double mapX0, mapY0, mapZ0;  // T[0] of each axis (the root box's lower corner)
    // media
    int ncomp, nlambda;
    const double* rho;
    const double* optics;        // [4][ncomp][nlambda]: kext, ksca, albedo, g
    // sources
    int nstar;
    const double* geomParam;
    const double* geomTable;     // per component kSersicTable words: SersicFunction s_i, then M_i
    const double* lum;
    const double* lumtot;
    const double* cdf;
    double emissionBias;
    // dust-phase cell sources (PanMonteCarloSimulation.cpp:193-205, 273-294), reference cell order
    const double* cellLv;        // [nlambda][ncells]
    const double* cellCdf;       // [nlambda][ncells + 1]
    const int* cellGuide;        // [nlambda][ncells + 1]: the CDF index at k / ncells (cellGuideKernel)
    const double* cellLtot;      // [nlambda]
    double cellBias;             // PanDustSystem::emissionBias (dust emission phase)
    const int* cellNode;         // octree: the leaf node of every reference cell
    int phase, peel;             // SKIRT_PHASE_*; peel-off on
    // instruments
    int ninstr;
    const DevInstr* instr;
    int nsed;
    // phase
    unsigned long long npp, first, end, seed;
    // the per-wavelength slice [sliceLo, sliceLo + sliceCnt) of a sharded phase (sliceCnt == npp: the
    // whole phase); first/end index the slice's packets, wavelength-slowest (see globalPacket)
    unsigned long long sliceLo, sliceCnt;
    unsigned int tag;
    double minWeightReduction;
    int minScatt;
    double xi;
    int store, hasDust;
    // tallies
    double* labs;                // [nlambda][labsStride], device cell order
    unsigned labsBytes;          // its size (< 4 GiB: the trace kernel addresses it through a buffer descriptor)
    int labsGlobal;              // 1: a table of 4 GiB or more, added to with global atomics (no descriptor)
    int labsHi;                  // 1: a table of 2^32 elements or more (32 GiB): the buffered adds keep the
                                 //    element index's high bits in pendHi (implies labsGlobal)
    int labsCopies;              // > 1: `labs` holds that many replicas labsCopyStride bytes apart, wave w adding
    unsigned labsCopyStride;     //   into replica w % labsCopies (folded into the table at the phase end)
    double* tally;
    unsigned int* error;
    unsigned long long* stats;   // packets, seg_fill, seg_walk, seg_peel, detects, absorbs, lane slots
    // DustSystem's _crossed histogram (DustSystem.cpp:959-1000), or null: per FILL and PEEL path one count in
    // bin min(segments, crossedBins - 1), kCrossedCopies copies (by wave) against same-address contention
    unsigned long long* crossed;
    int crossedBins;
    // slot pool (structure of arrays) and queues
    int nslots;
    double *srx, *sry, *srz, *skx, *sky, *skz, *sL, *sLth;
    int *sell, *snscatt, *sstellar, *sstate;
    int* svcell;                 // Voronoi: the cell of the packet's position (cellIndex), kNoCell if not known
    uint32_t *splo, *sphi, *sblock, *sw2, *sw3, *shave;
    double *resA, *resB;         // per slot: FILL -> tau, Lsca | WALK -> distance
    // fuse != 0: every FILL ray is fused -- its lane decides the interaction depth itself (decideFill) and walks
    // on to it along its own record. Per slot: WALK -> distance, now in resS (resA keeps tau for the event
    // kernel's own draws) | a FILL ray whose lane did not walk -> -1
    double* resS;
    // the lane's deviate u (negative: X < xi was drawn before it) and termination threshold, per slot. With
    // RayRef records fuseU[slot] also holds the optical depth a queued WALK ray has to reach
    double *fuseU, *fuseThr;
    int fuse;                    // 0: FILL and WALK rays queued apart | 1: fused | 2: fused, odd slots fall back (tests)
    RayRec* rays;                // the ray queue: rayCap RayRec, or rayCap RayRef (kRayRefs) in the same place
    DetRec* det;                 // detection records of the peel-off rays
    int* act[2];                 // active slot lists (double buffered)
    unsigned long long* claim;   // next packet index (relative to first)
    unsigned int* ctr;           // the pipeline's counters (enum Ctr), through CTR / CTRP
    int parity, init, threshold;
    int walkBack;                // WALK rays queued from the top of the ray queue, so they are pulled last
    // continuous scattering: per slot the dust segments of its last FILL path and their number
    int continuous, rayCap;
    PathRec* pathBuf;            // [slot][kPathCap]
    int* pathCnt;
    int ldsMeshOff, ldsOptOff, ldsInstrOff, ldsSedOff;  // in doubles
    int detCopies;  // detect kernel: LDS copies of the SED sums (8, 4, 2, 1), 0 = SEDs straight to the tally
    // polarised scattering (skirt_mcrt_set_mueller; pol == 0: none of these is read): the mixes' tables in global
    // memory (polarization.hpp, polTableWords), per slot the packet's Stokes vector, the normal of its scattering
    // plane and its polarized flag, and the detection records' Stokes parameters
    int pol, polNtheta;
    const double* polTab;
    double *sQ, *sU, *sV, *snx, *sny, *snz;
    int* spol;
    DetPol* detPol;
};

// One finest-level cell of the octree leaf map: the leaf node that covers it, that leaf's dust cell
// number and level, and the leaf's density of dust component 0 (the one-component kernels need no
// other gather per segment). 16 bytes, one global_load_dwordx4.
struct __attribute__((aligned(16))) LeafEntry {
    int node;
    unsigned cl;  // cell | level << 27
    double rho0;
};
constexpr int kLeafLevelShift = 27;
constexpr unsigned kLeafCellMask = (1u << kLeafLevelShift) - 1u;
constexpr int kMaxMapLevel = 9;  // 512^3 x 16 B = 2 GiB of HBM at most
// k-d tree leaf map entries: cl = cell | (shift x | shift y << 3 | shift z << 6) << kBinCellBits, the
// leaf's extent along each axis being 2^shift finest cells (binary trees split one axis at a time)
constexpr int kBinCellBits = 23;
constexpr unsigned kBinCellMask = (1u << kBinCellBits) - 1u;
constexpr int kMaxBinMapLevel = 7;

// Leaf map order of the finest-level cells of an N^3 map (N = 2^L): 2x2x2 bricks of 8 consecutive
// 16-byte entries (one 128-byte line), the bricks in (x, y, z) row-major order. Per line the same
// neighbourhood as Morton order, at a few integer operations instead of three bit spreads per step.
SKIRT_ARGS_FN unsigned leafBricks(int N) { return (unsigned)((N + 1) >> 1); }
SKIRT_ARGS_FN unsigned leafIndex(int N, unsigned x, unsigned y, unsigned z) {
    const unsigned nb = leafBricks(N);
    return ((((x >> 1) * nb + (y >> 1)) * nb + (z >> 1)) << 3) | ((x & 1u) << 2) | ((y & 1u) << 1) | (z & 1u);
}
SKIRT_ARGS_FN unsigned long long leafMapSize(int N) {
    const unsigned long long nb = leafBricks(N);
    return 8ull * nb * nb * nb;
}

// The counters live in kStatCopies copies of one 64-byte line each (summed by the host): the waves of a
// launch end together, and same-line atomics from all of them would queue on one L2 channel.
constexpr int kStatCopies = 64;
constexpr int kCrossedCopies = 64;

// The grid walks the host side knows, each listed once: the Grid<> kind its kernels are instantiated for, its
// SkirtStats::grid_walk value, and whether the walk's mesh is staged in LDS (nx + ny + nz + 3 doubles). The
// node-array tree walk comes last: withWalk (engine.hip) falls back to it.
struct Walk {
    int kind, stat;
    bool meshInLds;
};
constexpr Walk kWalks[] = {
    {SKIRT_GRID_CARTESIAN, SKIRT_WALK_CARTESIAN, true},
    {SKIRT_GRID_OCTREE, SKIRT_WALK_OCTREE_MAP, false},  // octree leaf map
    {kBinTreeMap, SKIRT_WALK_KDTREE_MAP, false},
    {kOctreeBookkeeping, SKIRT_WALK_OCTREE_BOOKKEEPING, false},
    {SKIRT_GRID_CYLINDER2D, SKIRT_WALK_CYLINDER2D, true},
    {SKIRT_GRID_SPHERE1D, SKIRT_WALK_SPHERE1D, true},
    {SKIRT_GRID_SPHERE2D, SKIRT_WALK_SPHERE2D, true},
    {SKIRT_GRID_VORONOI, SKIRT_WALK_VORONOI, false},
    {kOctreeNodes, SKIRT_WALK_TREE_NODES, false},
};
constexpr int kNumWalks = (int)(sizeof kWalks / sizeof kWalks[0]);

SKIRT_HIDDEN inline const Walk& walkOf(int kind) {
    for (const Walk& w : kWalks)
        if (w.kind == kind) return w;
    return kWalks[kNumWalks - 1];
}

// the arguments of the dust emission source kernels (device/emission.hpp)
struct EmisArgs {
    int ncells, nlambda, ncomp, ntemp;
    const int* devCell;          // reference cell -> device cell (null: identity)
    const double* labs;          // [nlambda][device cell]
    const double* labsDust;      // same, or null
    const double* rho;           // [device cell][ncomp]
    const double* volume;        // [reference cell]
    const double* kabs;          // [ncomp][nlambda]
    const double* sigmaabs;      // [ncomp][nlambda]
    const double* mu;            // [ncomp]
    const double* Tv;            // [ntemp]
    const double* planckabs;     // [ncomp][ntemp]
    const double* lambda;        // [nlambda]
    const double* dlambda;       // [nlambda]
    int labsStride;              // Labs row length
    double* lv;                  // out [nlambda][ncells]
    double* cdf;                 // out [nlambda][ncells + 1]
    double* ltot;                // out [nlambda]
    double* blockSums;           // scratch [nlambda][nblocks]
    int nblocks;
};

// the arguments of densitySampleKernel (device/density_sample.hpp)
struct DensArgs {
    int ncomp, ntab, nsample, mode;
    const int* kind;
    const double* param;  // ncomp x 8
    const double* norm;   // ncomp
    const double* table;  // ncomp x 2 ntab
    const double* boxes;  // n x 6
    const uint32_t* words;
    double* out;
    size_t n;
};

// the arguments of particleSampleKernel and particleMassKernel (device/particle_kernels.hpp)
struct PartArgs {
    PartView view;
    int nsample, mode;
    const double* boxes;  // n x 6 (SKIRT_PART_POINTS: n x 3)
    const uint32_t* words;
    double* out;
    size_t n;
};

}  // namespace skirt_dev

#endif
