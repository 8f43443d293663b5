// The engine's C ABI (include/skirt_mcrt.h), second half: the slot pool, the plan of a phase, its iterations, the
// reductions at its end, and synchronize, the downloads and the statistics. Runtime API only; the kernels are behind
// device/engine_launch.hpp, the arithmetic of the plans in engine_layout.cpp.
#include <cstring>

#include "engine_context.hpp"

int walkKind(const SkirtMcrt* c, bool hasDust) {
    if (c->gridKind < 0) return kOctreeNodes;  // no grid (a dust-free simulation): nothing is walked
    if (c->gridKind != SKIRT_GRID_OCTREE) return c->gridKind;
    if (c->search == SKIRT_TREE_BOOKKEEPING) return kOctreeBookkeeping;
    if (c->mapL >= 0 && hasDust) return c->binTree ? kBinTreeMap : SKIRT_GRID_OCTREE;
    return kOctreeNodes;
}

static int ensurePool(SkirtMcrt* c, int nslots, bool continuous, bool detPair, bool pol) {
    const int ninstr = (int)c->instr.size();
    const size_t rays = poolRayCap((size_t)nslots, (size_t)ninstr, continuous);
    if (rays >= (size_t)INT32_MAX) return fail(c, SKIRT_ERR_UNSUPPORTED, "ray queue too large");
    const int rayCap = (int)rays;
    const bool path = continuous && nslots > 0;
    const bool refs = poolRefs(continuous, c->gridKind);
    if (c->dPool && c->nslots == nslots && c->rayCap == rayCap && c->poolRefs == refs && c->poolPath == path &&
        c->poolDetPair == detPair && c->poolPol == pol)
        return SKIRT_OK;
    Args counted{};
    const size_t bytes = poolLayout(nullptr, (size_t)nslots, (size_t)rayCap, refs, detPair, path, pol, counted) + kPoolSpare;
    c->poolRefs = refs;
    c->poolPath = path;
    c->poolPol = pol;
    c->poolDetPair = detPair;
    if (c->dPool) { (void)hipFree(c->dPool); c->dPool = nullptr; }
    HIPCHECK(c, hipMalloc(&c->dPool, bytes));
    c->poolBytes = bytes;
    c->nslots = nslots;
    c->rayCap = rayCap;
    return SKIRT_OK;
}

static void carvePool(SkirtMcrt* c, Args& a) {
    poolLayout(static_cast<char*>(c->dPool), (size_t)c->nslots, (size_t)c->rayCap, c->poolRefs, c->poolDetPair, c->poolPath,
               c->poolPol, a);
    a.nslots = c->nslots;
    a.rayCap = c->rayCap;
    a.ctr = c->dCtr;
}

void gridArgs(const SkirtMcrt* c, Args& a) {
    a.ncells = c->ncells;
    a.labsStride = c->labsStride;
    a.nx = c->nx; a.ny = c->ny; a.nz = c->nz;
    a.brick = c->brick ? 1 : 0;
    a.mesh = c->dMesh;
    a.gx0 = c->gx0; a.gx1 = c->gx1; a.gy0 = c->gy0; a.gy1 = c->gy1; a.gz0 = c->gz0; a.gz1 = c->gz1;
    a.box = c->dBox; a.firstChild = c->dFirstChild; a.cellnumber = c->dCellnumber;
    a.splitDir = c->binTree ? c->dSplitDir : nullptr;
    a.father = c->dFather;
    a.nbrOffset = c->dNbrOffset; a.nbrList = c->dNbrList; a.eps = c->eps; a.search = c->search;
    a.site = c->dSite; a.vorStart = c->dVorStart; a.vorSlots = c->dVorSlots; a.vorScale = (float)c->vorScale; a.cellBbox = c->dCellBbox;
    a.devCell = c->dDevCell;
    a.vnb = c->vnb; a.blockOffset = c->dBlockOffset; a.blockSites = c->dBlockSites;
    a.ncomp = std::max(1, c->ncomp); a.nlambda = c->nlambda;
    a.rho = c->dRho;
}

static int ensureLeafMap(SkirtMcrt* c) {
    if (c->mapL < 0 || c->mapReady) return SKIRT_OK;
    const size_t n = (size_t)leafMapSize(1 << c->mapL);
    if (!c->dLeafMap) HIPCHECK(c, hipMalloc(&c->dLeafMap, n * sizeof(LeafEntry)));
    const int blocks = (int)std::min<size_t>((n + kBlock - 1) / kBlock, 65536);
    launchBuildLeafMap(dim3(blocks), c->stream, c->dLeafMap, c->dFirstChild, c->binTree ? c->dSplitDir : nullptr,
                       c->dCellnumber, c->dRho, std::max(1, c->ncomp), c->mapL);
    HIPCHECK(c, hipGetLastError());
    c->mapReady = true;
    return SKIRT_OK;
}

int ensureDustLabs(SkirtMcrt* c) {
    const size_t nl = (size_t)c->labsStride * c->nlambda;
    if (!c->dLabsDust && nl) {
        HIPCHECK(c, hipMalloc(&c->dLabsDust, nl * sizeof(double)));
        HIPCHECK(c, hipMemsetAsync(c->dLabsDust, 0, nl * sizeof(double), c->stream));
        c->ownLabsDust = true;
    }
    return SKIRT_OK;
}

extern "C" {

static int ensureTallies(SkirtMcrt* c) {
    const size_t nl = (size_t)c->labsStride * c->nlambda;
    if (!c->dLabs && nl) {
        HIPCHECK(c, hipMalloc(&c->dLabs, nl * sizeof(double)));
        HIPCHECK(c, hipMemsetAsync(c->dLabs, 0, nl * sizeof(double), c->stream));
        c->ownLabs = true;
    }
    if (!c->dTally && c->nInstrTally) {
        HIPCHECK(c, hipMalloc(&c->dTally, c->nInstrTally * sizeof(double)));
        HIPCHECK(c, hipMemsetAsync(c->dTally, 0, c->nInstrTally * sizeof(double), c->stream));
        c->ownTally = true;
    }
    return SKIRT_OK;
}

int skirt_mcrt_zero_tallies(SkirtMcrt* c) {
    if (!c) return SKIRT_ERR_ARG;
    HIPCHECK(c, hipSetDevice(c->device));
    int rc = ensureTallies(c);
    if (rc) return rc;
    const size_t nl = (size_t)c->labsStride * c->nlambda;
    if (c->dLabs && nl) HIPCHECK(c, hipMemsetAsync(c->dLabs, 0, nl * sizeof(double), c->stream));
    if (c->dTally && c->nInstrTally) HIPCHECK(c, hipMemsetAsync(c->dTally, 0, c->nInstrTally * sizeof(double), c->stream));
    HIPCHECK(c, hipMemsetAsync(c->dStats, 0, 8 * kStatCopies * sizeof(unsigned long long), c->stream));
    HIPCHECK(c, hipMemsetAsync(c->dError, 0, sizeof(unsigned int), c->stream));
    if (c->dCrossed)
        HIPCHECK(c, hipMemsetAsync(c->dCrossed, 0, (size_t)kCrossedCopies * c->crossedBins * sizeof(unsigned long long), c->stream));
    c->instrReduced = false;
    c->packagesTotal = 0;
    return SKIRT_OK;
}

int skirt_mcrt_run_stellar(SkirtMcrt* c, uint64_t npp, uint64_t first, uint64_t count, uint64_t seed,
                           const SkirtPhaseParams* p) {
    return skirt_mcrt_run_phase(c, SKIRT_PHASE_STELLAR, 0, npp, first, count, seed, p);
}

int skirt_mcrt_zero_dust_labs(SkirtMcrt* c) {
    if (!c) return SKIRT_ERR_ARG;
    HIPCHECK(c, hipSetDevice(c->device));
    int rc = ensureDustLabs(c);
    if (rc) return rc;
    const size_t nl = (size_t)c->labsStride * c->nlambda;
    if (nl) HIPCHECK(c, hipMemsetAsync(c->dLabsDust, 0, nl * sizeof(double), c->stream));
    return SKIRT_OK;
}

int skirt_mcrt_download_dust_labs(SkirtMcrt* c, double* labs) {
    if (!c || !labs) return SKIRT_ERR_ARG;
    int rc = skirt_mcrt_synchronize(c);
    if (rc) return rc;
    const size_t nl = (size_t)c->labsStride * c->nlambda;
    if (!c->dLabsDust) { std::fill(labs, labs + nl, 0.0); return SKIRT_OK; }
    std::vector<double> t(nl);
    HIPCHECK(c, hipMemcpy(t.data(), c->dLabsDust, nl * sizeof(double), hipMemcpyDeviceToHost));
    const bool perm = !c->devCell.empty();
    for (int ell = 0; ell < c->nlambda; ell++)
        for (int m = 0; m < c->ncells; m++)
            labs[(size_t)m * c->nlambda + ell] = t[(size_t)ell * c->labsStride + (perm ? c->devCell[m] : m)];
    return SKIRT_OK;
}

static const char* const kSummedTwice =
    "the instrument tallies were already summed over the processes: zero the tallies before another phase";
static int runPhase(SkirtMcrt* c, int phase, uint32_t cycle, uint64_t npp, uint64_t first, uint64_t count,
                    uint64_t sliceLo, uint64_t sliceCnt, uint64_t seed, const SkirtPhaseParams* p);
static int phaseEndReduce(SkirtMcrt* c, int phase, const SkirtPhaseParams* p);

int skirt_mcrt_run_phase(SkirtMcrt* c, int phase, uint32_t cycle, uint64_t npp, uint64_t first, uint64_t count,
                         uint64_t seed, const SkirtPhaseParams* p) {
    if (!c || !p) return SKIRT_ERR_ARG;
    if (first + count > npp * (uint64_t)c->nlambda) return fail(c, SKIRT_ERR_ARG, "packet range exceeds npp*nlambda");
    if (c->instrReduced) return fail(c, SKIRT_ERR_STATE, kSummedTwice);
    int rc = runPhase(c, phase, cycle, npp, first, count, 0, npp, seed, p);
    return rc ? rc : phaseEndReduce(c, phase, p);
}

int skirt_mcrt_run_phase_shard(SkirtMcrt* c, int phase, uint32_t cycle, uint64_t npp, int rank, int world,
                               uint64_t seed, const SkirtPhaseParams* p) {
    if (!c || !p) return SKIRT_ERR_ARG;
    if (world < 1 || rank < 0 || rank >= world) return fail(c, SKIRT_ERR_ARG, "bad shard (rank, world)");
    if (world > 1 && !c->reduce) return fail(c, SKIRT_ERR_STATE, "a sharded phase needs a reducer (skirt_mcrt_set_reducer)");
    if (c->instrReduced) return fail(c, SKIRT_ERR_STATE, kSummedTwice);
    // SequentialAssigner over the packets of one wavelength (SequentialAssigner.cpp:37-59), the same
    // block at every wavelength (IdenticalAssigner.cpp:37-58)
    uint64_t lo = 0, cnt = 0;
    skirt_mcrt_shard_slice(npp, rank, world, &lo, &cnt);
    int rc = runPhase(c, phase, cycle, npp, 0, cnt * (uint64_t)c->nlambda, lo, cnt, seed, p);
    return rc ? rc : phaseEndReduce(c, phase, p);
}

void skirt_mcrt_shard_slice(uint64_t npp, int rank, int world, uint64_t* lo, uint64_t* count) {
    const unsigned __int128 n = npp;
    const uint64_t a = (uint64_t)(n * (unsigned)rank / (unsigned)world);
    const uint64_t b = (uint64_t)(n * (unsigned)(rank + 1) / (unsigned)world);
    if (lo) *lo = a;
    if (count) *count = b - a;
}

int skirt_mcrt_set_reducer(SkirtMcrt* c, SkirtReduceTallyFn fn, void* user) {
    if (!c) return SKIRT_ERR_ARG;
    c->reduce = fn;
    c->reduceUser = user;
    return SKIRT_OK;
}

int skirt_mcrt_reduce_instruments(SkirtMcrt* c) {
    if (!c) return SKIRT_ERR_ARG;
    if (!c->reduce || c->instrReduced || !c->dTally || !c->nInstrTally) return SKIRT_OK;
    HIPCHECK(c, hipSetDevice(c->device));
    // marked summed only once the reducer succeeded: a failed reduction can be retried
    if (c->reduce(c->reduceUser, SKIRT_TALLY_INSTRUMENTS, c->dTally, c->nInstrTally, (void*)c->stream))
        return fail(c, SKIRT_ERR_STATE, "the instrument reduction failed");
    c->instrReduced = true;
    return SKIRT_OK;
}

// PanDustSystem::sumResults at the end of a phase (PanDustSystem.cpp:394-403): the stellar Labs after the
// stellar phase, the dust Labs after a self-absorption cycle, summed over the processes by the caller's
// reducer, enqueued behind the phase on the engine stream. Instrument::sumResults (Instrument.cpp:57)
// comes once, before the tallies are read (skirt_mcrt_reduce_instruments / download).
static int phaseEndReduce(SkirtMcrt* c, int phase, const SkirtPhaseParams* p) {
    if (!c->reduce) return SKIRT_OK;
    const size_t n = (size_t)c->labsStride * c->nlambda;
    int r = 0;
    if (phase == SKIRT_PHASE_STELLAR && p->store_absorption && c->dLabs && n)
        r = c->reduce(c->reduceUser, SKIRT_TALLY_LABS, c->dLabs, n, (void*)c->stream);
    else if (phase == SKIRT_PHASE_DUST_SELFABS && c->dLabsDust && n)
        r = c->reduce(c->reduceUser, SKIRT_TALLY_DUST_LABS, c->dLabsDust, n, (void*)c->stream);
    return r ? fail(c, SKIRT_ERR_STATE, "the absorption reduction failed") : SKIRT_OK;
}

// What one phase runs with: everything the iteration loop needs that does not change between iterations.
struct PhasePlan {
    Args a{};  // the kernel arguments, but for the pool (carvePool) and the per-iteration parity, init and det
    int kind = kOctreeNodes;  // the grid walk (kWalks)
    bool continuous = false, noStore = false, detAside = false;
    bool aniso = false;  // a stellar phase with an anisotropic component: the ANISO event kernels
    size_t ldsTrace = 0, ldsEvent = 0, ldsDetect = 0;  // dynamic LDS of the trace, event / continuous and detect kernels
    const void* traceFn = nullptr;
    int tgrid = 0, egrid = 0, dgrid = 0;  // workgroups of the trace, event / continuous and detect launches
    double* labsTarget = nullptr;  // the Labs replicas (a.labsCopies > 1) fold into this table of labsElems elements
    uint64_t labsElems = 0;
};

// the plan's Labs addressing mode and replicas (a.store is set; fills a.labs*): planLabsMode decides, this
// allocates and clears the replicas
static int planLabs(SkirtMcrt* c, int phase, PhasePlan& pl) {
    Args& a = pl.a;
    const uint64_t labsElems = pl.labsElems = (uint64_t)c->labsStride * (uint64_t)c->nlambda;
    std::string err;
    LabsPlan lp;
    if (int rc = planLabsMode(labsElems, a.store != 0, phase == SKIRT_PHASE_DUST_SELFABS, lp, err)) return fail(c, rc, err);
    a.labsHi = lp.hi;
    a.labsGlobal = lp.global;
    a.labs = phase == SKIRT_PHASE_DUST_SELFABS ? c->dLabsDust : c->dLabs;
    a.labsBytes = lp.bytes;
    pl.labsTarget = a.labs;
    a.labsCopies = 1;
    a.labsCopyStride = 0;
    if (lp.copies > 1) {
        const size_t need = (size_t)lp.stride * lp.copies;
        if (c->labsRepBytes < need) {
            if (c->dLabsRep) HIPCHECK(c, hipFree(c->dLabsRep));
            c->dLabsRep = nullptr;
            c->labsRepBytes = 0;
            HIPCHECK(c, hipMalloc(&c->dLabsRep, need));
            HIPCHECK(c, hipMemsetAsync(c->dLabsRep, 0, need, c->stream));
            c->labsRepBytes = need;
        }
        if (c->labsRepDirty) {  // (the failed phase's kernels may still run, on sD too)
            HIPCHECK(c, hipDeviceSynchronize());
            HIPCHECK(c, hipMemsetAsync(c->dLabsRep, 0, c->labsRepBytes, c->stream));
        }
        c->labsRepDirty = true;  // until the fold at this phase's end
        a.labs = c->dLabsRep;
        a.labsCopies = lp.copies;
        a.labsCopyStride = lp.stride;
    }
    return SKIRT_OK;
}

// the plan's LDS layout (a.lds*Off, a.detCopies), LDS sizes and the no-store choice (planLdsLayout)
static int planLds(SkirtMcrt* c, PhasePlan& pl) {
    Args& a = pl.a;
    LdsInputs in;
    in.meshWords = (walkOf(pl.kind).meshInLds && a.hasDust) ? (c->nx + c->ny + c->nz + 3) : 0;
    in.treeWords = a.leafMap ? 3 * (c->mapN + 1) : 0;
    in.ncomp = a.ncomp; in.nlambda = a.nlambda; in.ninstr = a.ninstr; in.nsed = c->nsed;
    in.store = a.store != 0; in.continuous = pl.continuous; in.voronoi = c->gridKind == SKIRT_GRID_VORONOI;
    in.labsHi = a.labsHi != 0;
    in.budget = c->ldsMax;
    std::string err;
    LdsPlan lp;
    if (int rc = planLdsLayout(in, lp, err)) return fail(c, rc, err);
    a.ldsMeshOff = lp.meshOff; a.ldsOptOff = lp.optOff; a.ldsInstrOff = lp.instrOff; a.ldsSedOff = lp.sedOff;
    pl.noStore = lp.noStore;
    pl.ldsTrace = lp.trace; pl.ldsEvent = lp.event; pl.ldsDetect = lp.detect;
    a.detCopies = lp.detCopies;
    c->lastDetCopies = a.detCopies;
    // launches above 64 KiB of dynamic LDS declare it first
    if (pl.ldsDetect > 64 * 1024)
        HIPCHECK(c, hipFuncSetAttribute(detectKernelOf(a.pol != 0), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)pl.ldsDetect));
    return SKIRT_OK;
}

// Fills the plan of a phase over the packets [first, first + count). What the plan's values depend on is made
// ready on the way, in the order the phase has always issued these calls: the pool and the detect stream are
// allocated, ensureLeafMap launches buildLeafMapKernel on the caller's stream, planLabs allocates and clears
// the Labs replicas (hipMemsetAsync, after a failed phase behind a hipDeviceSynchronize), and planLds and this
// function declare LDS above 64 KiB (hipFuncSetAttribute) and ask for the trace kernel's occupancy.
static int planPhase(SkirtMcrt* c, int phase, uint32_t cycle, uint64_t npp, uint64_t first, uint64_t count,
                     uint64_t sliceLo, uint64_t sliceCnt, uint64_t seed, const SkirtPhaseParams* p, PhasePlan& pl) {
    int rc;
    // slot pool: enough packets in flight to fill the chip many times over, bounded by the phase size.
    // 2^24 slots (7.0 GB of packet state and ray queues with one instrument) make each iteration's trace
    // launch long enough that its drain tail and the event kernel amortise (round 1, C3: 2^21 slots 1.87e8
    // pkt/s, 2^22 1.98e8, 2^23 2.04e8, 2^24 2.05e8; round 4 at the configurations' sizes, 2^24 against
    // 2^23: C3 +1.5 %, C2 +0.7 %, C4 +0.7 %, C5 +0.3 %, profiles/r04_slots_2e24.txt)
    int slots = c->slotsWanted > 0 ? c->slotsWanted : (1 << 24);
    // continuous scattering (MonteCarloSimulation::continuousScattering): peel-offs from every dust segment
    // of every path replace the ones at the interaction points; fewer slots, each with a longer queue
    const bool continuous = pl.continuous = p->continuous_scattering && phase != SKIRT_PHASE_DUST_SELFABS && p->has_dust &&
                            !c->instr.empty();
    // (the queue holds kPathCap peel-offs per instrument and slot: the slots shrink with the instruments)
    if (continuous) slots = std::min(slots, std::max(64, kContSlots / std::max(1, (int)c->instr.size())));
    if ((uint64_t)slots > count) slots = (int)count;
    // (a phase that fits the pool runs its packets in lockstep; admitting them in 2 or 4 waves instead changes
    // neither the C5 step nor its 164 trace launches: the tail iterations are the few long-lived packets either
    // way, profiles/r06_ab.txt)
    slots = std::max(slots, 64);
    // the detect kernel of an iteration beside the next iteration's event kernel (peel-offs at the
    // interaction points): C3 +1.9 %, C2 within the spread; beside the next trace kernel as well, C3 +1.6 %,
    // C2 -1.5 %. Not for Voronoi grids: C4 -2.2 %, and -2.6 % again after the counter-line and event-grid
    // changes (profiles/r05_detect_aside_ab.txt)
    pl.detAside = !continuous && !c->instr.empty() && p->has_dust && c->gridKind != SKIRT_GRID_VORONOI;
    const bool pol = c->dPolTab != nullptr && p->has_dust;  // (runPhase has refused what has no polarised kernel)
    if ((rc = ensurePool(c, slots, continuous, pl.detAside, pol))) return rc;
    if (pl.detAside && !c->sD) {
        HIPCHECK(c, hipStreamCreateWithFlags(&c->sD, hipStreamNonBlocking));
        HIPCHECK(c, hipEventCreateWithFlags(&c->evDetT, hipEventDisableTiming));
        HIPCHECK(c, hipEventCreateWithFlags(&c->evDet[0], hipEventDisableTiming));
        HIPCHECK(c, hipEventCreateWithFlags(&c->evDet[1], hipEventDisableTiming));
        HIPCHECK(c, hipEventCreateWithFlags(&c->evDetJoin, hipEventDisableTiming));
    }
    Args& a = pl.a;
    gridArgs(c, a);
    const int kind = pl.kind = walkKind(c, p->has_dust);
    if (kind == SKIRT_GRID_OCTREE || kind == kBinTreeMap) {  // the leaf-map walks
        if ((rc = ensureLeafMap(c))) return rc;
        a.leafMap = c->dLeafMap; a.treeT = c->dTreeT; a.mapL = c->mapL; a.mapN = c->mapN;
        a.mapInvX = c->mapInv[0]; a.mapInvY = c->mapInv[1]; a.mapInvZ = c->mapInv[2];
        a.mapX0 = c->mapOrigin[0]; a.mapY0 = c->mapOrigin[1]; a.mapZ0 = c->mapOrigin[2];
    }
    a.optics = c->dOptics;
    pl.aniso = c->anyAniso && phase == SKIRT_PHASE_STELLAR;
    a.pol = pol ? 1 : 0;
    a.polTab = pol ? c->dPolTab : nullptr;
    a.polNtheta = c->polNtheta;
    a.nstar = c->nstar; a.geomParam = c->dGeomParam; a.geomTable = c->dGeomTable; a.lum = c->dLum;
    a.lumtot = c->dLumtot; a.cdf = c->dCdf; a.emissionBias = c->emissionBias;
    a.ninstr = (int)c->instr.size(); a.instr = c->dInstr; a.nsed = c->nsed;
    a.npp = npp; a.first = first; a.end = first + count; a.seed = seed;
    a.sliceLo = sliceLo; a.sliceCnt = sliceCnt;
    a.tag = (unsigned)phase | (cycle << 2);  // Philox counter word 1: streams differ per phase and cycle
    a.phase = phase;
    a.peel = phase != SKIRT_PHASE_DUST_SELFABS;
    a.continuous = continuous ? 1 : 0;
    a.cellLv = c->dCellLv; a.cellCdf = c->dCellCdf; a.cellGuide = c->dCellGuide; a.cellLtot = c->dCellLtot; a.cellBias = c->cellBias;
    a.cellNode = c->dCellNode;
    a.minWeightReduction = p->min_weight_reduction; a.minScatt = p->min_scatt_events; a.xi = p->scatt_bias;
    // absorption: the stellar phase as its parameters say (into Labs), self-absorption always (into the
    // dust Labs), dust emission never (MonteCarloSimulation.cpp:287, PanMonteCarloSimulation.cpp:223, 331)
    a.store = phase == SKIRT_PHASE_STELLAR ? (p->store_absorption ? 1 : 0) : (phase == SKIRT_PHASE_DUST_SELFABS ? 1 : 0);
    a.hasDust = p->has_dust ? 1 : 0;
    if (a.store && !c->dLabs) return fail(c, SKIRT_ERR_STATE, "no Labs buffer");
    if ((rc = planLabs(c, phase, pl))) return rc;
    a.tally = c->dTally;
    a.error = c->dError; a.stats = c->dStats;
    a.crossed = c->dCrossed; a.crossedBins = c->crossedBins;
    a.claim = c->dClaim;
    a.threshold = c->threshold > 0 ? c->threshold : (c->gridKind == SKIRT_GRID_VORONOI ? 8 : 16);
    a.walkBack = c->walkBack >= 0 ? c->walkBack : (c->gridKind == SKIRT_GRID_VORONOI ? 1 : 0);
    if ((rc = planLds(c, pl))) return rc;
    // (the node-array walk's no-store kernel has no registers for the lane's decision, Tracer::kFuse)
    a.fuse = (continuous || (pl.noStore && kind == kOctreeNodes)) ? 0
             : c->fuseWalk >= 0                                    ? std::min(c->fuseWalk, 2)
                                                                   : (c->gridKind == SKIRT_GRID_VORONOI ? 0 : 1);
    c->lastWalk = walkOf(kind).stat;
    pl.traceFn = traceKernelOf(kind, a.ncomp == 1, continuous, a.labsGlobal != 0, pl.noStore);
    if (pl.ldsTrace > 64 * 1024)
        HIPCHECK(c, hipFuncSetAttribute(pl.traceFn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.ldsTrace));
    pl.tgrid = c->traceGrid;
    if (pl.tgrid <= 0) {
        int per = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, pl.traceFn, kBlock, pl.ldsTrace) != hipSuccess || per < 1) per = 2;
        pl.tgrid = std::max(1, c->numCUs) * per;
        c->traceBlocksPerCU = per;
    }
    // event kernel blocks per CU: 3 (3 waves/SIMD, the registers allow it). Voronoi: C4 +0.6 % against 2
    // (profiles/r04_event_bpc_sweep.txt); the other grids, once the block reservations no longer serialize on
    // one counter line: C3 +0.7 %, C2 +2.3 % against 2, 4 the same as 3 (profiles/r05_event_bpc_ab.txt)
#ifndef SKIRT_EVENT_BPC
#define SKIRT_EVENT_BPC 3
#endif
    const int ebpc = SKIRT_EVENT_BPC;
    pl.egrid = std::max(1, std::min((slots + kBlock - 1) / kBlock, std::max(1, c->numCUs) * ebpc));
    pl.dgrid = std::max(1, std::max(1, c->numCUs) * 4);
    return SKIRT_OK;
}

// Iteration it (parity q = it & 1): the event kernel consumes active list ctr[2+q] and queues rays
// into ctr[q] and the next active list into ctr[2+1-q]; the trace kernel walks the ctr[q] rays and
// resets ctr[1-q] and ctr[2+q] for the next iteration; the detect kernel turns the finished peel-off
// rays into detections. After every detect kernel the counters are copied to pinned memory behind an
// event; the host reads each copy kPollRing copies later (by then long complete), so it never drains
// the stream. Once an active count was 0 the phase is finished; the few iterations launched after
// that point find no work and exit at once.
static int runIterations(SkirtMcrt* c, const PhasePlan& pl) {
    const int kind = pl.kind;
    const bool one = pl.a.ncomp == 1;
    // the kernels of the plan, each launched through its generic entry (launchArgs)
    const void* const eventFn = eventKernelOf(kind, one, pl.a.pol != 0, pl.aniso);
    const void* const contFn = contKernelOf(kind, one);
    const void* const detectFn = detectKernelOf(pl.a.pol != 0);
    auto launchEvent = [&](const Args& aa, hipStream_t st) { return launchArgs(eventFn, pl.egrid, pl.ldsEvent, st, aa); };
    auto launchCont = [&](const Args& aa, hipStream_t st) { return launchArgs(contFn, pl.egrid, pl.ldsEvent, st, aa); };
    auto launchTrace = [&](const Args& aa, hipStream_t st) { return launchArgs(pl.traceFn, pl.tgrid, pl.ldsTrace, st, aa); };
    while ((int)c->pollEv.size() < kPollRing) {
        hipEvent_t e;
        HIPCHECK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->pollEv.push_back(e);
    }
    hipStream_t st = c->stream;
    Args aa = pl.a, prev;
    carvePool(c, aa);
    DetRec* const detBase = aa.det;
    DetPol* const detPolBase = aa.detPol;
    int rc, its = 0, polls = 0;
    int pollIt[kPollRing] = {};  // the iteration count each copy was taken at
    bool pendingDet = false;
    // the detect kernel of the last trace launch (after that launch), then the counter copy.
    // With detAside it runs on sD after the trace launch; the next iteration of the same parity, which
    // writes that region of detection records again, waits for it (evDet). Its record count is then
    // zeroed for that iteration's event kernel to append to.
    bool detUsed[2] = {false, false};
    auto detect = [&]() -> int {
        pendingDet = false;
        const Args& d = prev;
        hipStream_t sd = pl.detAside ? c->sD : st;
        if (pl.detAside) {
            HIPCHECK(c, hipEventRecord(c->evDetT, st));
            HIPCHECK(c, hipStreamWaitEvent(sd, c->evDetT, 0));
        }
        HIPCHECK(c, launchArgs(detectFn, pl.dgrid, pl.ldsDetect, sd, d));
        HIPCHECK(c, hipGetLastError());
        HIPCHECK(c, hipMemsetAsync(CTRP(d.ctr, CTR_DET + d.parity), 0, sizeof(unsigned int), sd));
        if (pl.detAside) {
            HIPCHECK(c, hipEventRecord(c->evDet[d.parity], sd));
            detUsed[d.parity] = true;
        }
        return SKIRT_OK;
    };
    // iterations before the phase is declared stuck; SKIRT_AMD_MAX_ITERATIONS lowers the cap (tests of the
    // error exits)
    const int maxIts = envInt("SKIRT_AMD_MAX_ITERATIONS", 10000000);
    int total = 0;
    while (true) {
        if (pendingDet && (rc = detect())) return rc;
        if (its > 0 && its % kPollEvery == 0) {
            const int slot = polls % kPollRing;
            unsigned int* hc = c->hCtr + slot * kCtrWords;
            hipEvent_t pe = c->pollEv[slot];
            if (polls >= kPollRing) {
                // the copy made kPollRing polls ago: is the phase finished?
                HIPCHECK(c, hipEventSynchronize(pe));
                if (CTR(hc, CTR_ACTIVE + (pollIt[slot] & 1)) == 0) break;
            }
            // (the counters before CTR_WALK; the poll reads CTR_ACTIVE)
            HIPCHECK(c, hipMemcpyAsync(hc, aa.ctr, CTR_WALK * kCtrStride * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
            HIPCHECK(c, hipEventRecord(pe, st));
            pollIt[slot] = its;
            polls++;
        }
        if (its > maxIts) return fail(c, SKIRT_ERR_STATE, "photon phase did not terminate");
        aa.parity = its & 1;
        aa.init = (its == 0) ? 1 : 0;
        if (pl.detAside) {
            // this iteration's detection records: the region of its parity, free once the detect kernel of
            // the last iteration of that parity is done
            aa.det = detBase + (size_t)aa.parity * (size_t)(c->rayCap - c->nslots);
            if (detPolBase) aa.detPol = detPolBase + (size_t)aa.parity * (size_t)(c->rayCap - c->nslots);
            if (detUsed[aa.parity]) HIPCHECK(c, hipStreamWaitEvent(st, c->evDet[aa.parity], 0));
        }
        if (aa.continuous && !aa.init) {  // the continuous peel-offs of the FILL rays that just returned
            HIPCHECK(c, launchCont(aa, st));
            HIPCHECK(c, hipGetLastError());
        }
        HIPCHECK(c, launchEvent(aa, st));
        HIPCHECK(c, hipGetLastError());
        if (!aa.hasDust) break;  // every packet completes in the event kernel
        if ((int)c->traceEv.size() < 2 * (c->traceLaunches + 1)) {
            hipEvent_t e0, e1;
            HIPCHECK(c, hipEventCreate(&e0));
            HIPCHECK(c, hipEventCreate(&e1));
            c->traceEv.push_back(e0);
            c->traceEv.push_back(e1);
        }
        // the detect kernel of the last iteration runs beside this iteration's event kernel only
        if (pl.detAside && detUsed[1 - aa.parity]) HIPCHECK(c, hipStreamWaitEvent(st, c->evDet[1 - aa.parity], 0));
        HIPCHECK(c, hipEventRecord(c->traceEv[2 * c->traceLaunches], st));
        HIPCHECK(c, launchTrace(aa, st));
        HIPCHECK(c, hipGetLastError());
        HIPCHECK(c, hipEventRecord(c->traceEv[2 * c->traceLaunches + 1], st));
        c->traceLaunches++;
        if (aa.ninstr > 0) { prev = aa; pendingDet = true; }
        its++;
        total++;
    }
    if (pendingDet && (rc = detect())) return rc;
    c->lastIterations = total;
    if (pl.detAside && (detUsed[0] || detUsed[1])) {  // the caller's stream continues after the last detect kernel
        HIPCHECK(c, hipEventRecord(c->evDetJoin, c->sD));
        HIPCHECK(c, hipStreamWaitEvent(c->stream, c->evDetJoin, 0));
    }
    return SKIRT_OK;
}

static int runPhase(SkirtMcrt* c, int phase, uint32_t cycle, uint64_t npp, uint64_t first, uint64_t count,
                    uint64_t sliceLo, uint64_t sliceCnt, uint64_t seed, const SkirtPhaseParams* p) {
    if (phase < SKIRT_PHASE_STELLAR || phase > SKIRT_PHASE_DUST_SELFABS) return fail(c, SKIRT_ERR_ARG, "unknown phase");
    if (cycle >= (1u << 30)) return fail(c, SKIRT_ERR_ARG, "cycle number too large");
    const bool cellPhase = phase != SKIRT_PHASE_STELLAR;
    // polarised scattering: the stellar phase's interaction-point peel-offs only (the continuous peel-off and the
    // dust phases have no polarised kernels: refused, not run unpolarised)
    if (c->dPolTab && p->has_dust && p->continuous_scattering)
        return fail(c, SKIRT_ERR_UNSUPPORTED, "continuous scattering is not supported with polarised dust mixes");
    if (c->dPolTab && cellPhase)
        return fail(c, SKIRT_ERR_UNSUPPORTED, "dust emission phases are not supported with polarised dust mixes");
    // anisotropic sources: every grid but the Voronoi grid (kAnisoGrid)
    if (c->anyAniso && !cellPhase && c->gridKind == SKIRT_GRID_VORONOI)
        return fail(c, SKIRT_ERR_UNSUPPORTED, "anisotropic sources are not supported on a Voronoi dust grid");
    if (cellPhase && (!c->dCellLtot || !p->has_dust)) return fail(c, SKIRT_ERR_STATE, "a dust phase needs a dust system and uploaded cell sources");
    if (c->gridKind < 0 && p->has_dust) return fail(c, SKIRT_ERR_STATE, "no grid uploaded");
    if (!cellPhase && !c->dLumtot) return fail(c, SKIRT_ERR_STATE, "no sources uploaded");
    if (p->has_dust && !c->dRho) return fail(c, SKIRT_ERR_STATE, "no media uploaded");
    if (first + count > npp * (uint64_t)c->nlambda) return fail(c, SKIRT_ERR_ARG, "packet range exceeds npp*nlambda");
    if (p->min_weight_reduction <= 0 || p->scatt_bias < 0 || p->scatt_bias > 1) return fail(c, SKIRT_ERR_ARG, "bad phase parameters");
    HIPCHECK(c, hipSetDevice(c->device));
    int rc = ensureTallies(c);
    if (rc) return rc;
    if (phase == SKIRT_PHASE_DUST_SELFABS && (rc = ensureDustLabs(c))) return rc;
    c->lastMs = 0;
    c->phaseTimed = false;
    c->lastIterations = 0;
    if (c->traceLaunches) {  // time the previous call's launches before their events are reused
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        float ms = 0;
        for (int k = 0; k < c->traceLaunches; k++)
            if (hipEventElapsedTime(&ms, c->traceEv[2 * k], c->traceEv[2 * k + 1]) == hipSuccess) c->traceMs += ms;
        c->traceLaunchesTotal += (uint64_t)c->traceLaunches;
        c->traceLaunches = 0;
    }
    c->packagesTotal += count;
    if (!cellPhase) {
        // the wavelengths outside [lumLo, lumHi] launch nothing: their packet indices (per wavelength sliceCnt
        // of them, wavelength-slowest) are left out of the phase instead of being claimed and skipped one by one
        const uint64_t lo = c->lumHi < 0 ? 0 : (uint64_t)c->lumLo * sliceCnt;
        const uint64_t hi = c->lumHi < 0 ? 0 : (uint64_t)(c->lumHi + 1) * sliceCnt;
        const uint64_t b = std::max(first, lo), e = std::min(first + count, hi);
        first = b;
        count = e > b ? e - b : 0;
    }
    if (count == 0) return SKIRT_OK;
    if (!c->dOptics) {  // a dust-free simulation still stages (zero) optical tables
        std::vector<double> z(4 * (size_t)c->nlambda, 0.0);
        if ((rc = upload(c, c->dOptics, z.data(), z.size()))) return rc;
    }
    PhasePlan pl;
    if ((rc = planPhase(c, phase, cycle, npp, first, count, sliceLo, sliceCnt, seed, p, pl))) return rc;
    HIPCHECK(c, hipMemsetAsync(c->dClaim, 0, sizeof(unsigned long long), c->stream));
    HIPCHECK(c, hipMemsetAsync(c->dCtr, 0, kCtrWords * sizeof(unsigned int), c->stream));
    HIPCHECK(c, hipEventRecord(c->ev0, c->stream));
    if ((rc = runIterations(c, pl))) return rc;
    if (pl.a.labsCopies > 1) {
        launchLabsFold(dim3(2048), c->stream, pl.labsTarget, c->dLabsRep, (size_t)pl.labsElems, pl.a.labsCopies,
                       (size_t)pl.a.labsCopyStride / sizeof(double));
        HIPCHECK(c, hipGetLastError());
        c->labsRepDirty = false;  // the fold zeroes the replicas
    }
    HIPCHECK(c, hipEventRecord(c->ev1, c->stream));
    c->phaseTimed = true;
    return SKIRT_OK;
}

int skirt_mcrt_synchronize(SkirtMcrt* c) {
    if (!c) return SKIRT_ERR_ARG;
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    // only events this phase recorded: an elapsed time over unrecorded ones fails, and the failure would stay
    // behind as the thread's last error for the next launch check of any engine on this thread
    if (c->phaseTimed && hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) c->lastMs = ms;
    for (int k = 0; k < c->traceLaunches; k++)
        if (hipEventElapsedTime(&ms, c->traceEv[2 * k], c->traceEv[2 * k + 1]) == hipSuccess) c->traceMs += ms;
    c->traceLaunchesTotal += (uint64_t)c->traceLaunches;
    c->traceLaunches = 0;  // timed: the event pairs can be reused
    unsigned int e = 0;
    HIPCHECK(c, hipMemcpy(&e, c->dError, sizeof e, hipMemcpyDeviceToHost));
    if (e & ERR_TAU) return fail(c, SKIRT_ERR_NUMERIC, "the optical depth along the path is not a positive number");
    if (e & ERR_GEOM) return fail(c, SKIRT_ERR_NUMERIC, kGeomCapMessage);
    if (e & ERR_PATH_CAP)
        return fail(c, SKIRT_ERR_UNSUPPORTED, "continuous scattering: a path crosses more than " +
                                                  std::to_string(kPathCap) + " dust cells");
    if (e) return fail(c, SKIRT_ERR_STATE, "ray queue overflow");
    return SKIRT_OK;
}

int skirt_mcrt_download(SkirtMcrt* c, double* labs, double* instr) {
    if (!c) return SKIRT_ERR_ARG;
    int rc = instr ? skirt_mcrt_reduce_instruments(c) : SKIRT_OK;
    if (rc) return rc;
    rc = skirt_mcrt_synchronize(c);
    if (rc) return rc;
    const size_t nl = (size_t)c->labsStride * c->nlambda;
    if (labs && nl) {
        if (!c->dLabs) return fail(c, SKIRT_ERR_STATE, "no Labs buffer");
        std::vector<double> t(nl);
        HIPCHECK(c, hipMemcpy(t.data(), c->dLabs, nl * sizeof(double), hipMemcpyDeviceToHost));
        const bool perm = !c->devCell.empty();
        for (int ell = 0; ell < c->nlambda; ell++)
            for (int m = 0; m < c->ncells; m++)
                labs[(size_t)m * c->nlambda + ell] = t[(size_t)ell * c->labsStride + (perm ? c->devCell[m] : m)];
    }
    if (instr && c->nInstrTally) {
        if (!c->dTally) return fail(c, SKIRT_ERR_STATE, "no instrument buffer");
        std::vector<double> t(c->nInstrTally);
        HIPCHECK(c, hipMemcpy(t.data(), c->dTally, c->nInstrTally * sizeof(double), hipMemcpyDeviceToHost));
        // per instrument, the reference's order: frames [slot][lambda][pixel], then SEDs [slot][lambda]
        size_t o = 0;
        const size_t nl = (size_t)c->nlambda;
        for (const DevInstr& d : c->instr) {
            const size_t npix = (size_t)d.nx * d.ny;
            if (d.kind != SKIRT_INSTR_SED)
                for (int slot = 0; slot < d.nslots; slot++)
                    for (size_t ell = 0; ell < nl; ell++)
                        for (size_t l = 0; l < npix; l++)
                            instr[o++] = t[d.frameBase + (ell * npix + l) * d.slotStride + slot];
            if (d.kind != SKIRT_INSTR_FRAME)
                for (size_t q = 0; q < (size_t)d.nslots * nl; q++) instr[o++] = t[d.sedBase + q];
        }
    }
    return SKIRT_OK;
}

int skirt_mcrt_download_crossed(SkirtMcrt* c, uint64_t* hist, int bins) {
    if (!c || !hist || bins < 0) return SKIRT_ERR_ARG;
    if (!c->dCrossed) return fail(c, SKIRT_ERR_STATE, "the cells-crossed histogram is off (skirt_mcrt_set_crossed)");
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> h((size_t)kCrossedCopies * c->crossedBins);
    HIPCHECK(c, hipMemcpy(h.data(), c->dCrossed, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int b = 0; b < bins; b++) {
        uint64_t v = 0;
        if (b < c->crossedBins)
            for (int k = 0; k < kCrossedCopies; k++) v += h[(size_t)k * c->crossedBins + b];
        hist[b] = v;
    }
    return SKIRT_OK;
}

int skirt_mcrt_stats(SkirtMcrt* c, SkirtStats* out) {
    if (!c || !out) return SKIRT_ERR_ARG;
    HIPCHECK(c, hipSetDevice(c->device));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    std::vector<unsigned long long> copies(8 * kStatCopies);
    HIPCHECK(c, hipMemcpy(copies.data(), c->dStats, copies.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < kStatCopies; k++)
        for (int q = 0; q < 8; q++) v[q] += copies[8 * k + q];
    out->packets = v[0];
    out->segments_fill = v[1];
    out->segments_walk = v[2];
    out->segments_peel = v[3];
    out->detects = v[4];
    out->absorb_adds = v[5];
    out->lane_slots = v[6];
    out->iterations = (uint64_t)c->lastIterations;
    out->kernel_ms = c->lastMs;
    out->trace_ms = c->traceMs;
    out->trace_launches = c->traceLaunchesTotal;
    out->grid_walk = c->lastWalk;
    out->map_level = c->mapL;
    out->labs_requests = v[7];
    out->device_cells = c->ndev;
    out->trace_blocks_per_cu = (uint64_t)c->traceBlocksPerCU;
    out->packages = c->packagesTotal;
    return SKIRT_OK;
}

}  // extern "C"
