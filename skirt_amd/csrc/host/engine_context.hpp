// The engine's context behind the C ABI of include/skirt_mcrt.h, and what its host sources share: engine_setup.cpp
// (create, destroy, the uploads and the probes) and engine_phase.cpp (pool, plan, iterations, phase, reduction,
// downloads and statistics). Runtime API only: the kernels are reached through device/engine_launch.hpp.
#ifndef SKIRT_AMD_HOST_ENGINE_CONTEXT_HPP
#define SKIRT_AMD_HOST_ENGINE_CONTEXT_HPP

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../../include/skirt_mcrt.h"
#include "../device/engine_args.hpp"
#include "../device/engine_launch.hpp"
#include "engine_layout.hpp"

using namespace skirt_dev;

struct SkirtMcrt {
    int device = 0;
    hipStream_t own = nullptr, stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    // grid
    int gridKind = -1, ncells = 0, nx = 0, ny = 0, nz = 0, nnodes = 0, search = 1;
    // device cell space: ndev >= ncells device cell numbers (octrees leave unused numbers so that every
    // group of 8 sibling leaves starts on a 64-byte line), Labs rows of labsStride (ndev rounded up to 8)
    int ndev = 0;
    int labsStride = 0;
    bool brick = false;  // Cartesian cells numbered in 2x2x2 bricks
    double eps = 0, gx0 = 0, gx1 = 0, gy0 = 0, gy1 = 0, gz0 = 0, gz1 = 0;
    double* dMesh = nullptr;
    double* dBox = nullptr;
    int *dFirstChild = nullptr, *dCellnumber = nullptr, *dNbrOffset = nullptr, *dNbrList = nullptr;
    signed char* dSplitDir = nullptr;  // k-d tree split axes (null for octrees)
    int* dFather = nullptr;            // octree fathers (Bookkeeping search)
    bool binTree = false;
    // Voronoi grid
    double *dSite = nullptr, *dCellBbox = nullptr;
    VorEntry* dVorSlots = nullptr;
    int *dVorStart = nullptr, *dBlockOffset = nullptr;
    BlockSite* dBlockSites = nullptr;
    std::vector<VorEntry> vorSlotsHost;  // host copy: upload_media writes the densities into the headers
    std::vector<int> vorStartHost;
    double vorScale = 1.0;
    int vnb = 0;
    // octree leaf map (mapL < 0: walk the node arrays)
    int mapL = -1, mapN = 0;
    double mapInv[3] = {0, 0, 0};
    double mapOrigin[3] = {0, 0, 0};
    double* dTreeT = nullptr;
    LeafEntry* dLeafMap = nullptr;
    bool mapReady = false;
    int lastWalk = -1;  // SKIRT_WALK_* of the last run
    // device cell numbering: devCell[reference cell] (empty = identity). Octree cells are renumbered in
    // Morton (depth-first, children in octant order) order so that neighbouring cells share Labs lines;
    // rho is uploaded and Labs downloaded through it.
    std::vector<int> devCell;
    // media
    int ncomp = 0, nlambda = 0;
    double *dRho = nullptr, *dOptics = nullptr;
    // polarised scattering (skirt_mcrt_set_mueller): the mixes' tables as polarization.hpp lays them out, on the
    // device and on the host (the probe's host side), and their theta resolution; null: unpolarised
    double* dPolTab = nullptr;
    std::vector<double> polTab;
    int polNtheta = 0;
    // sources
    int nstar = 0;
    double *dGeomParam = nullptr, *dLum = nullptr, *dLumtot = nullptr, *dCdf = nullptr;
    // the first and last wavelength with stellar luminosity: a stellar phase shoots only the packet indices of
    // [lumLo, lumHi] (the others launch nothing, MonteCarloSimulation.cpp:272-273; each packet's stream is
    // keyed by its own index, so skipping them changes no other packet)
    int lumLo = 0, lumHi = -1;
    double* dGeomTable = nullptr;  // SersicGeometry tables, kSersicTable per component
    // a component of an anisotropic kind (aniso_emission.hpp): the stellar phase runs the ANISO event kernels, and
    // dGeomParam holds the Netzer table (anisoNetzerWords) behind the components' rows
    bool anyAniso = false;
    std::vector<double> geomParamHost;  // the rows of dGeomParam (the launch probe's checks)
    double emissionBias = 0.5;
    // dust-phase cell sources and the dust Labs tally
    double *dCellLv = nullptr, *dCellCdf = nullptr, *dCellLtot = nullptr;
    int* dCellGuide = nullptr;  // guide tables of the cell CDFs (cellGuideKernel)
    size_t cellGuideCount = 0;
    double cellBias = 0.5;
    int* dCellNode = nullptr;
    double* dLabsDust = nullptr;
    bool ownLabsDust = true;
    // Labs replicas (SKIRT_AMD_LABS_COPIES > 1): the absorbing phases add into them, folded at the phase end
    double* dLabsRep = nullptr;
    size_t labsRepBytes = 0;
    // trace launches have added into the replicas since their last fold: a phase that ended early (an error
    // return after its first trace launch) left partial adds there, which the next storing phase clears
    bool labsRepDirty = false;
    // grey-body emissivity tables for the device-side dust emission sources
    int emisNtemp = 0;
    double *dEmisVolume = nullptr, *dEmisKabs = nullptr, *dEmisSigma = nullptr, *dEmisMu = nullptr, *dEmisTv = nullptr,
           *dEmisPlanck = nullptr, *dEmisLambda = nullptr, *dEmisDlambda = nullptr, *dEmisScratch = nullptr;
    int* dDevCell = nullptr;
    // instruments
    std::vector<DevInstr> instr;
    DevInstr* dInstr = nullptr;
    size_t nInstrTally = 0;
    int nsed = 0;
    // tallies
    double *dLabs = nullptr, *dTally = nullptr;
    bool ownLabs = true, ownTally = true;
    unsigned long long *dClaim = nullptr, *dStats = nullptr;
    unsigned long long* dCrossed = nullptr;  // kCrossedCopies x crossedBins (skirt_mcrt_set_crossed)
    int crossedBins = 0;
    unsigned int *dError = nullptr, *dCtr = nullptr, *hCtr = nullptr;  // kCtrWords counters; hCtr: poll ring
    // The pipeline runs on the caller's stream. The detect kernel of iteration k may run on sD, beside the
    // event and trace kernels of iteration k + 1 (the detection records alternate between two regions by
    // iteration parity, Args::det); evDet[q]: the detect kernel of the last parity-q iteration is done
    hipStream_t sD = nullptr;
    hipEvent_t evDetT = nullptr, evDet[2] = {}, evDetJoin = nullptr;
    std::vector<hipEvent_t> pollEv;      // kPollRing events behind the counter copies
    // slot pool
    int nslots = 0, rayCap = 0;
    bool poolRefs = false;  // the pool's ray queue holds RayRef records (16 bytes), not RayRec (80)
    bool poolPath = false;  // the pool holds the continuous-scattering path records
    bool poolDetPair = false;  // the pool holds two detection-record regions (one per iteration parity)
    bool poolPol = false;      // the pool holds the Stokes arrays of a polarised simulation
    void* dPool = nullptr;               // nslots slots
    size_t poolBytes = 0;
    // config
    // threshold 0: 16 idle lanes before a trace wave pulls rays, 8 on Voronoi grids (C3 +0.6 %, C2 +0.5 %, C5
    // +0.5 % against 8; C4 -0.1 %; profiles/r06_pull_threshold.txt)
    int traceGrid = 0, threshold = 0, slotsWanted = 0;
    // WALK rays at the end of the pull order: SKIRT_AMD_WALK_BACK=1 / 0, default (-1) on Voronoi grids only.
    // It shortens every grid's launch tail, but on the tree and Cartesian grids the launch's main part then
    // runs without the atomic-free WALK paths between the absorbing FILL paths: C3 2.16e8 -> 2.08e8, C2
    // 2.9e8 -> 2.8e8; C4 9.30e7 -> 9.38e7 (profiles/r03_walk_back_ab.txt)
    int walkBack = getenv("SKIRT_AMD_WALK_BACK") ? atoi(getenv("SKIRT_AMD_WALK_BACK")) : -1;
    // The lane of a finished FILL ray walks on to the interaction point (Args::fuse): SKIRT_AMD_FUSE_WALK=1 / 0,
    // 2: fused with every odd slot falling back to a queued WALK ray (tests); default (-1): fused, but for
    // Voronoi grids. Never with continuous scattering, whose peel-off kernel draws between the FILL and the walk.
    // A scattering order then costs a packet one pipeline iteration instead of two: C3 38 -> 22 launches per
    // step, +3.5 %; C2 +6.6 %; C5 +3.1 %. C4 -0.6 % (lane use 0.920 -> 0.918: its WALK rays, pulled last
    // (walkBack), filled the launch tails that a lane's FILL + WALK lengthens), so Voronoi grids stay unfused
    // (medians of three alternating runs, profiles/fused_walk_ab.txt)
    int fuseWalk = getenv("SKIRT_AMD_FUSE_WALK") ? atoi(getenv("SKIRT_AMD_FUSE_WALK")) : -1;
    int traceBlocksPerCU = 0;  // the occupancy the last trace launch was sized for
    int lastDetCopies = 0;  // SED copies of the last run's detect kernel
    double lastMs = 0;
    bool phaseTimed = false;  // ev0/ev1 recorded by the last phase (an empty slice records nothing)
    std::vector<hipEvent_t> traceEv;  // pairs around the trace launches not yet timed
    int traceLaunches = 0;
    uint64_t packagesTotal = 0;       // packet indices of the phases run since the last zero_tallies (SkirtStats::packages)
    double traceMs = 0;               // all timed trace launches since the context was created
    uint64_t traceLaunchesTotal = 0;
    int numCUs = 0;
    size_t ldsMax = 64 * 1024;  // LDS one workgroup may allocate (hipDeviceProp_t::sharedMemPerBlock; 160 KiB on gfx950)
    int lastIterations = 0;
    // multi-process reduction of the tallies (skirt_mcrt_set_reducer)
    SkirtReduceTallyFn reduce = nullptr;
    void* reduceUser = nullptr;
    bool instrReduced = false;
};

#pragma GCC visibility push(hidden)  // what follows is the engine's own: not among the library's dynamic symbols

inline int fail(SkirtMcrt* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIPCHECK(ctx, call)                                                                    \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) return fail(ctx, SKIRT_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class T>
int upload(SkirtMcrt* c, T*& dst, const T* src, size_t n) {
    if (dst) { (void)hipFree(dst); dst = nullptr; }
    if (n == 0) return SKIRT_OK;
    if (!src) return fail(c, SKIRT_ERR_ARG, "null host array");
    HIPCHECK(c, hipMalloc(&dst, n * sizeof(T)));
    HIPCHECK(c, hipMemcpy(dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return SKIRT_OK;
}

// shared by the two sources (defined in engine_phase.cpp)
// the walk of the uploaded grid; trees go through their leaf map where there is one and the phase has dust
int walkKind(const SkirtMcrt* c, bool hasDust);
// the grid and density fields of the kernel arguments (every kernel that walks the grid)
void gridArgs(const SkirtMcrt* c, Args& a);
int ensureDustLabs(SkirtMcrt* c);

// a kernel taking one Args, by its address (engine_launch.hpp)
inline hipError_t launchArgs(const void* fn, int grid, size_t lds, hipStream_t st, const Args& a) {
    void* args[] = {const_cast<Args*>(&a)};
    return hipLaunchKernel(fn, dim3(grid), dim3(kBlock), args, lds, st);
}

#pragma GCC visibility pop

#endif
