// The engine's C ABI (include/skirt_mcrt.h), first half: the context's life, the uploads of grid, media, sources,
// instruments and cell sources, and the probes. Runtime API only; the kernels are behind device/engine_launch.hpp,
// the arithmetic of the uploads in engine_layout.cpp.
#include <cmath>
#include <cstring>
#include <utility>

#include "engine_context.hpp"
#include "../device/aniso_emission.hpp"
#include "../device/polarization.hpp"

extern "C" {

int skirt_mcrt_abi_version(void) { return SKIRT_MCRT_ABI_VERSION; }

int skirt_mcrt_create(int device, SkirtMcrt** out) {
    if (!out) return SKIRT_ERR_ARG;
    *out = nullptr;
    auto* c = new SkirtMcrt();
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipMalloc(&c->dClaim, sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&c->dStats, 8 * kStatCopies * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&c->dError, sizeof(unsigned int)) != hipSuccess ||
        hipMalloc(&c->dCtr, kCtrWords * sizeof(unsigned int)) != hipSuccess ||
        hipHostMalloc(&c->hCtr, kPollRing * kCtrWords * sizeof(unsigned int)) != hipSuccess) {
        skirt_mcrt_destroy(c);  // frees what the failed step left allocated
        return SKIRT_ERR_HIP;
    }
    c->stream = c->own;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        c->numCUs = prop.multiProcessorCount;
        if (prop.sharedMemPerBlock > 0) c->ldsMax = prop.sharedMemPerBlock;
    }
    (void)hipMemset(c->dStats, 0, 8 * kStatCopies * sizeof(unsigned long long));
    (void)hipMemset(c->dError, 0, sizeof(unsigned int));
    *out = c;
    return SKIRT_OK;
}

int skirt_mcrt_set_stream(SkirtMcrt* c, void* s) {
    if (!c) return SKIRT_ERR_ARG;
    c->stream = s ? (hipStream_t)s : c->own;
    return SKIRT_OK;
}

int skirt_mcrt_configure(SkirtMcrt* c, int slots, int grid, int threshold) {
    if (!c) return SKIRT_ERR_ARG;
    if (slots < 0 || grid < 0 || threshold < 0) return fail(c, SKIRT_ERR_ARG, "negative configuration value");
    c->slotsWanted = slots;
    c->traceGrid = grid;
    if (threshold) c->threshold = std::max(1, std::min(64, threshold));
    return SKIRT_OK;
}

// n cells between n + 1 strictly increasing points (none: nothing to check)
static bool increasing(const double* v, int n) {
    for (int i = 0; i < n; i++)
        if (!(v[i] < v[i + 1])) return false;
    return true;
}

// The mesh of the Cartesian, cylindrical and spherical grids: the points of each axis in turn, nx + 1 | ny + 1 |
// nz + 1 doubles; an axis without cells (n = 0) keeps one unused word.
static int uploadMesh(SkirtMcrt* c, const double* xv, int nx, const double* yv, int ny, const double* zv, int nz) {
    std::vector<double> mesh;
    auto axis = [&](const double* v, int n) {
        if (n > 0) mesh.insert(mesh.end(), v, v + n + 1);
        else mesh.push_back(0.0);
    };
    axis(xv, nx);
    axis(yv, ny);
    axis(zv, nz);
    c->nx = nx; c->ny = ny; c->nz = nz;
    return upload(c, c->dMesh, mesh.data(), mesh.size());
}

static int uploadCartesian(SkirtMcrt* c, const SkirtGridDesc* g) {
    if (g->nx < 1 || g->ny < 1 || g->nz < 1 || !g->xv || !g->yv || !g->zv) return fail(c, SKIRT_ERR_ARG, "bad Cartesian grid");
    if ((long long)g->nx * g->ny * g->nz != g->ncells) return fail(c, SKIRT_ERR_ARG, "ncells != nx*ny*nz");
    if (!increasing(g->xv, g->nx)) return fail(c, SKIRT_ERR_ARG, "x mesh not increasing");
    if (!increasing(g->yv, g->ny)) return fail(c, SKIRT_ERR_ARG, "y mesh not increasing");
    if (!increasing(g->zv, g->nz)) return fail(c, SKIRT_ERR_ARG, "z mesh not increasing");
    // device numbers in 2x2x2 bricks (Grid<SKIRT_GRID_CARTESIAN>::dev); SKIRT_AMD_CELL_ALIGN=0: the
    // reference's numbering
    c->brick = cellAlign();
    if (c->brick) {
        const long long bx = (g->nx + 1) / 2, by = (g->ny + 1) / 2, bz = (g->nz + 1) / 2;
        if (8 * bx * by * bz >= (1ll << 31)) return fail(c, SKIRT_ERR_UNSUPPORTED, "Cartesian grid too large");
        c->devCell.assign(g->ncells, 0);
        for (int i = 0; i < g->nx; i++)
            for (int j = 0; j < g->ny; j++)
                for (int k = 0; k < g->nz; k++)
                    c->devCell[k + g->nz * j + g->nz * g->ny * i] =
                        (int)((((i >> 1) * by + (j >> 1)) * bz + (k >> 1)) << 3) | ((i & 1) << 2) | ((j & 1) << 1) | (k & 1);
        c->ndev = (int)(8 * bx * by * bz);
    }
    c->gx0 = g->xv[0]; c->gx1 = g->xv[g->nx];
    c->gy0 = g->yv[0]; c->gy1 = g->yv[g->ny];
    c->gz0 = g->zv[0]; c->gz1 = g->zv[g->nz];
    return uploadMesh(c, g->xv, g->nx, g->yv, g->ny, g->zv, g->nz);
}

static int uploadTree(SkirtMcrt* c, const SkirtGridDesc* g) {
    std::string err;
    std::vector<int> father;
    int rc;
    if ((rc = checkTree(g, father, err))) return fail(c, rc, err);
    const bool bin = g->split_dir != nullptr;
    const int nnbr = g->nbr_offset[6 * (size_t)g->nnodes];
    c->nnodes = g->nnodes;
    c->eps = g->eps;
    c->search = g->search;
    c->gx0 = g->box[0]; c->gy0 = g->box[1]; c->gz0 = g->box[2];
    c->gx1 = g->box[3]; c->gy1 = g->box[4]; c->gz1 = g->box[5];
    if ((rc = upload(c, c->dBox, g->box, 6 * (size_t)g->nnodes))) return rc;
    if ((rc = upload(c, c->dFirstChild, g->first_child, (size_t)g->nnodes))) return rc;
    c->binTree = bin;
    if (!father.empty() && (rc = upload(c, c->dFather, father.data(), father.size()))) return rc;
    if (bin) {
        std::vector<signed char> dirs(g->split_dir, g->split_dir + g->nnodes);
        for (int l = 0; l < g->nnodes; l++)
            if (g->first_child[l] < 0) dirs[l] = 0;
        if ((rc = upload(c, c->dSplitDir, dirs.data(), dirs.size()))) return rc;
    }
    CellNumbering num;
    if ((rc = numberTreeLeaves(g, num, err))) return fail(c, rc, err);
    c->devCell = std::move(num.devCell);
    c->ndev = num.ndev;
    std::vector<int> cellNode(g->ncells, 0);
    for (int l = 0; l < g->nnodes; l++)
        if (g->first_child[l] < 0) cellNode[g->cellnumber[l]] = l;
    if ((rc = upload(c, c->dCellNode, cellNode.data(), cellNode.size()))) return rc;
    std::vector<int> cn(g->cellnumber, g->cellnumber + g->nnodes);
    for (int l = 0; l < g->nnodes; l++)
        if (cn[l] >= 0) cn[l] = c->devCell[cn[l]];
    if ((rc = upload(c, c->dCellnumber, cn.data(), (size_t)g->nnodes))) return rc;
    if ((rc = upload(c, c->dNbrOffset, g->nbr_offset, 6 * (size_t)g->nnodes + 1))) return rc;
    std::vector<int> dummy(1, 0);
    if ((rc = upload(c, c->dNbrList, nnbr ? g->nbr_list : dummy.data(), nnbr ? (size_t)nnbr : 1))) return rc;
    // the leaf map's split tables, where the tree can be walked through one (planLeafMapTables)
    c->mapL = -1;
    c->mapReady = false;
    if (c->dLeafMap) { (void)hipFree(c->dLeafMap); c->dLeafMap = nullptr; }
    const LeafMapPlan map = planLeafMapTables(g, c->ndev);
    if (map.L < 0) return SKIRT_OK;
    if ((rc = upload(c, c->dTreeT, map.T.data(), map.T.size()))) return rc;
    c->mapL = map.L;
    c->mapN = map.N;
    for (int ax = 0; ax < 3; ax++) c->mapInv[ax] = map.inv[ax];
    for (int ax = 0; ax < 3; ax++) c->mapOrigin[ax] = map.origin[ax];
    return SKIRT_OK;
}

static int uploadVoronoi(SkirtMcrt* c, const SkirtGridDesc* g) {
    std::string err;
    VoronoiPack v;
    int rc;
    if ((rc = packVoronoi(g, v, err))) return fail(c, rc, err);
    c->eps = g->eps;
    c->gx0 = g->extent[0]; c->gy0 = g->extent[1]; c->gz0 = g->extent[2];
    c->gx1 = g->extent[3]; c->gy1 = g->extent[4]; c->gz1 = g->extent[5];
    c->vnb = g->nblocks;
    c->devCell = std::move(v.devCell);
    c->vorScale = v.vorScale;
    c->vorSlotsHost = std::move(v.slots);
    const size_t nb3 = (size_t)g->nblocks * g->nblocks * g->nblocks;
    if ((rc = upload(c, c->dSite, v.site.data(), v.site.size()))) return rc;
    if ((rc = upload(c, c->dCellBbox, v.bbox.data(), v.bbox.size()))) return rc;
    if ((rc = upload(c, c->dVorStart, v.start.data(), v.start.size()))) return rc;
    if ((rc = upload(c, c->dVorSlots, c->vorSlotsHost.data(), c->vorSlotsHost.size()))) return rc;
    c->vorStartHost = std::move(v.start);
    if ((rc = upload(c, c->dBlockOffset, g->block_offset, nb3 + 1))) return rc;
    if ((rc = upload(c, c->dBlockSites, v.blocks.data(), v.blocks.size()))) return rc;
    return upload(c, c->dDevCell, c->devCell.data(), c->devCell.size());
}

static int uploadCylinder(SkirtMcrt* c, const SkirtGridDesc* g) {
    if (g->nx < 1 || g->nz < 1 || !g->xv || !g->zv) return fail(c, SKIRT_ERR_ARG, "bad cylindrical grid");
    if ((long long)g->nx * g->nz != g->ncells) return fail(c, SKIRT_ERR_ARG, "ncells != nx*nz");
    if (g->xv[0] != 0.0) return fail(c, SKIRT_ERR_ARG, "the radial mesh does not start at 0");
    if (!increasing(g->xv, g->nx)) return fail(c, SKIRT_ERR_ARG, "R mesh not increasing");
    if (!increasing(g->zv, g->nz)) return fail(c, SKIRT_ERR_ARG, "z mesh not increasing");
    c->gx0 = -g->xv[g->nx]; c->gx1 = g->xv[g->nx];
    c->gy0 = -g->xv[g->nx]; c->gy1 = g->xv[g->nx];
    c->gz0 = g->zv[0]; c->gz1 = g->zv[g->nz];
    // R | one unused word | z: the Cartesian mesh layout with ny = 0
    return uploadMesh(c, g->xv, g->nx, nullptr, 0, g->zv, g->nz);
}

static int uploadSphere(SkirtMcrt* c, const SkirtGridDesc* g) {
    const bool two = g->kind == SKIRT_GRID_SPHERE2D;
    const int nt = two ? g->nz : 0;
    if (g->nx < 1 || !g->xv) return fail(c, SKIRT_ERR_ARG, "bad spherical grid");
    if (two ? (nt < 1 || g->ny != nt || !g->yv || !g->zv) : (g->ny != 0 || g->nz != 0))
        return fail(c, SKIRT_ERR_ARG, "bad spherical grid");
    if ((long long)g->nx * (two ? nt : 1) != g->ncells) return fail(c, SKIRT_ERR_ARG, "ncells != nx*nz");
    const double rmax = g->extent[3];
    if (!(rmax > 0.0) || !(g->xv[g->nx - 1] < rmax)) return fail(c, SKIRT_ERR_ARG, "extent does not hold the outer radius");
    if (g->xv[0] != 0.0) return fail(c, SKIRT_ERR_ARG, "the radial mesh does not start at 0");
    if (!increasing(g->xv, g->nx)) return fail(c, SKIRT_ERR_ARG, "r mesh not increasing");
    if (!increasing(g->zv, nt)) return fail(c, SKIRT_ERR_ARG, "theta mesh not increasing");
    for (int i = 0; i < nt; i++) if (!(g->yv[i] > g->yv[i + 1])) return fail(c, SKIRT_ERR_ARG, "cosines not decreasing");
    if (two && !(g->eps > 0.0)) return fail(c, SKIRT_ERR_ARG, "eps should be positive");
    c->gx0 = -rmax; c->gx1 = rmax;
    c->gy0 = -rmax; c->gy1 = rmax;
    c->gz0 = -rmax; c->gz1 = rmax;
    c->eps = two ? g->eps : 0.0;
    // r | cos theta | theta: the Cartesian mesh layout (one unused word each where ny = nz = 0)
    return uploadMesh(c, g->xv, g->nx, g->yv, nt, g->zv, nt);
}

int skirt_mcrt_upload_grid(SkirtMcrt* c, const SkirtGridDesc* g) {
    if (!c || !g) return SKIRT_ERR_ARG;
    HIPCHECK(c, hipSetDevice(c->device));
    c->gridKind = -1;  // a rejected upload leaves no grid
    c->ncells = g->ncells;
    c->ndev = g->ncells;
    // the state only some grids set
    c->brick = false;
    c->devCell.clear();
    c->mapL = -1;
    c->mapReady = false;
    c->binTree = false;
    int rc;
    switch (g->kind) {
    case SKIRT_GRID_CARTESIAN: rc = uploadCartesian(c, g); break;
    case SKIRT_GRID_OCTREE: rc = uploadTree(c, g); break;
    case SKIRT_GRID_VORONOI: rc = uploadVoronoi(c, g); break;
    case SKIRT_GRID_CYLINDER2D: rc = uploadCylinder(c, g); break;
    case SKIRT_GRID_SPHERE1D:
    case SKIRT_GRID_SPHERE2D: rc = uploadSphere(c, g); break;
    default: return fail(c, SKIRT_ERR_UNSUPPORTED, "unsupported grid kind");
    }
    if (rc) return rc;
    c->labsStride = (c->ndev + 7) & ~7;
    c->gridKind = g->kind;
    return SKIRT_OK;
}

int skirt_mcrt_upload_media(SkirtMcrt* c, const SkirtMediaDesc* m) {
    if (!c || !m) return SKIRT_ERR_ARG;
    if (c->gridKind < 0) return fail(c, SKIRT_ERR_STATE, "upload the grid before the media");
    if (m->ncells != c->ncells || m->ncomp < 1 || m->ncomp > 8 || m->nlambda < 1)
        return fail(c, SKIRT_ERR_ARG, "media sizes do not match the grid (1 <= ncomp <= 8)");
    if (m->nlambda >= (1 << 14)) return fail(c, SKIRT_ERR_ARG, "at most 16383 wavelengths");
    HIPCHECK(c, hipSetDevice(c->device));
    c->mapReady = false;  // the leaf map caches the densities
    if (c->dPolTab && (m->ncomp != c->ncomp || m->nlambda != c->nlambda)) {  // Mueller tables of other media
        // (instruments set with them keep their Stokes slots, which no unpolarised kernel fills: as set_mueller)
        if (!c->instr.empty())
            return fail(c, SKIRT_ERR_STATE, "media of other sizes drop the Mueller tables: clear the instruments first");
        (void)hipFree(c->dPolTab);
        c->dPolTab = nullptr;
        c->polTab.clear();
        c->polNtheta = 0;
    }
    c->ncomp = m->ncomp;
    c->nlambda = m->nlambda;
    const size_t nt = (size_t)m->ncomp * m->nlambda;
    std::vector<double> opt(4 * nt);
    std::memcpy(opt.data(), m->kext, nt * sizeof(double));
    std::memcpy(opt.data() + nt, m->ksca, nt * sizeof(double));
    std::memcpy(opt.data() + 2 * nt, m->albedo, nt * sizeof(double));
    std::memcpy(opt.data() + 3 * nt, m->g, nt * sizeof(double));
    int rc;
    if (c->devCell.empty()) {
        if ((rc = upload(c, c->dRho, m->rho, (size_t)m->ncells * m->ncomp))) return rc;
    } else {
        std::vector<double> rho((size_t)c->ndev * m->ncomp, 0.0);  // unused device cells: no dust
        for (int q = 0; q < m->ncells; q++)
            for (int h = 0; h < m->ncomp; h++) rho[(size_t)c->devCell[q] * m->ncomp + h] = m->rho[(size_t)q * m->ncomp + h];
        if ((rc = upload(c, c->dRho, rho.data(), rho.size()))) return rc;
    }
    if ((rc = upload(c, c->dOptics, opt.data(), opt.size()))) return rc;
    if (c->gridKind == SKIRT_GRID_VORONOI && !c->vorSlotsHost.empty()) {
        // the density of component 0 in every cell's header, next to its site
        for (int q = 0; q < m->ncells; q++) {
            const double v = m->rho[(size_t)q * m->ncomp];
            std::memcpy(reinterpret_cast<char*>(c->vorSlotsHost.data() + c->vorStartHost[c->devCell[q]]) + 3 * sizeof(double),
                        &v, sizeof v);
        }
        if ((rc = upload(c, c->dVorSlots, c->vorSlotsHost.data(), c->vorSlotsHost.size()))) return rc;
    }
    return SKIRT_OK;
}

int skirt_mcrt_upload_sources(SkirtMcrt* c, const SkirtSourceDesc* s) {
    if (!c || !s) return SKIRT_ERR_ARG;
    if (s->ncomp < 1 || s->nlambda < 1) return fail(c, SKIRT_ERR_ARG, "bad source sizes");
    // device geometry table: the 8 parameters of each component with its kind in the last word
    std::vector<double> gp(8 * (size_t)s->ncomp);
    bool tables = false, aniso = false;
    for (int h = 0; h < s->ncomp; h++) {
        if (s->geom_kind[h] < SKIRT_GEOM_PLUMMER || s->geom_kind[h] > SKIRT_GEOM_LASER)
            return fail(c, SKIRT_ERR_UNSUPPORTED, "unsupported source geometry");
        if (anisoIsKind(s->geom_kind[h])) {
            aniso = true;
            const bool sized = s->geom_kind[h] != SKIRT_GEOM_NETZER && s->geom_kind[h] != SKIRT_GEOM_LASER;
            if (sized && !(s->geom_param[8 * h] > 0))
                return fail(c, SKIRT_ERR_ARG, "an anisotropic source's radius or extent should be positive");
        }
        if (s->geom_kind[h] == SKIRT_GEOM_SERSIC) {
            if (!s->geom_table) return fail(c, SKIRT_ERR_ARG, "SersicGeometry without its tables");
            tables = true;
        }
        if (s->geom_kind[h] == SKIRT_GEOM_TORUS || s->geom_kind[h] == SKIRT_GEOM_CONICALSHELL) {
            if (!s->geom_table) return fail(c, SKIRT_ERR_ARG, "TorusGeometry or ConicalShellGeometry without its table row");
            tables = true;
        }
        for (int q = 0; q < 7; q++) gp[8 * h + q] = s->geom_param[8 * h + q];
        gp[8 * h + 7] = (double)s->geom_kind[h];
    }
    c->geomParamHost = gp;
    if (aniso) {  // the Netzer disk's table behind the rows (one copy for every component, 6.4 KB)
        gp.resize(8 * (size_t)s->ncomp + anisoNetzerWords);
        anisoNetzerTable(gp.data() + 8 * (size_t)s->ncomp);
    }
    c->anyAniso = aniso;
    HIPCHECK(c, hipSetDevice(c->device));
    if (c->nlambda && c->nlambda != s->nlambda) return fail(c, SKIRT_ERR_ARG, "sources and media disagree on nlambda");
    if (s->nlambda >= (1 << 14)) return fail(c, SKIRT_ERR_ARG, "at most 16383 wavelengths");
    c->nstar = s->ncomp;
    c->emissionBias = s->emission_bias;
    c->nlambda = s->nlambda;
    int rc;
    if ((rc = upload(c, c->dGeomParam, gp.data(), gp.size()))) return rc;
    if (tables) {
        if ((rc = upload(c, c->dGeomTable, s->geom_table, (size_t)kSersicTable * s->ncomp))) return rc;
    } else if (c->dGeomTable) {
        (void)hipFree(c->dGeomTable);
        c->dGeomTable = nullptr;
    }
    if ((rc = upload(c, c->dLum, s->lum, (size_t)s->ncomp * s->nlambda))) return rc;
    if ((rc = upload(c, c->dLumtot, s->lumtot, (size_t)s->nlambda))) return rc;
    c->lumLo = 0;
    c->lumHi = -1;
    for (int ell = 0; ell < s->nlambda; ell++)
        if (s->lumtot[ell] > 0) {
            if (c->lumHi < 0) c->lumLo = ell;
            c->lumHi = ell;
        }
    if ((rc = upload(c, c->dCdf, s->cdf, (size_t)s->nlambda * (s->ncomp + 1)))) return rc;
    return SKIRT_OK;
}

int skirt_mcrt_set_instruments(SkirtMcrt* c, const SkirtInstrDesc* in, int n) {
    if (!c || n < 0 || (n > 0 && !in)) return SKIRT_ERR_ARG;
    if (n > 63) return fail(c, SKIRT_ERR_ARG, "at most 63 instruments");
    if (c->nlambda < 1) return fail(c, SKIRT_ERR_STATE, "upload sources or media before instruments");
    HIPCHECK(c, hipSetDevice(c->device));
    c->instr.clear();
    std::string err;
    InstrLayout lay;
    int rc = instrLayout(in, n, c->nlambda, c->dPolTab != nullptr, lay, err);
    if (rc) return fail(c, rc, err);
    c->instr = std::move(lay.instr);
    c->nInstrTally = lay.nInstrTally;
    c->nsed = lay.nsed;
    rc = upload(c, c->dInstr, c->instr.data(), c->instr.size());
    if (rc) return rc;
    if (c->ownTally && c->dTally) { (void)hipFree(c->dTally); c->dTally = nullptr; }
    if (c->dPool) { (void)hipFree(c->dPool); c->dPool = nullptr; c->nslots = 0; }
    return SKIRT_OK;
}

int skirt_mcrt_tally_sizes(SkirtMcrt* c, size_t* nl, size_t* ni) {
    if (!c) return SKIRT_ERR_ARG;
    if (nl) *nl = (size_t)c->labsStride * c->nlambda;
    if (ni) *ni = c->nInstrTally;
    return SKIRT_OK;
}

int skirt_mcrt_bind_tallies(SkirtMcrt* c, double* dl, double* di) {
    if (!c) return SKIRT_ERR_ARG;
    if (dl) {
        if (c->ownLabs && c->dLabs) (void)hipFree(c->dLabs);
        c->dLabs = dl;
        c->ownLabs = false;
    }
    if (di) {
        if (c->ownTally && c->dTally) (void)hipFree(c->dTally);
        c->dTally = di;
        c->ownTally = false;
    }
    return SKIRT_OK;
}

// the guide tables of the cell CDFs (dCellCdf must hold them), on the engine's stream
static int buildCellGuide(SkirtMcrt* c) {
    const int N = c->ncells, Nl = c->nlambda;
    const size_t n = (size_t)Nl * (N + 1);
    if (c->dCellGuide && c->cellGuideCount != n) { (void)hipFree(c->dCellGuide); c->dCellGuide = nullptr; }
    if (!c->dCellGuide) HIPCHECK(c, hipMalloc(&c->dCellGuide, n * sizeof(int)));
    c->cellGuideCount = n;
    launchCellGuide(dim3((N + 1 + kBlock - 1) / kBlock, Nl), c->stream, c->dCellCdf, c->dCellGuide, N);
    HIPCHECK(c, hipGetLastError());
    return SKIRT_OK;
}

int skirt_mcrt_upload_cell_sources(SkirtMcrt* c, const SkirtCellSourceDesc* src) {
    if (!c || !src) return SKIRT_ERR_ARG;
    if (c->gridKind < 0) return fail(c, SKIRT_ERR_STATE, "upload the grid before cell sources");
    if (src->ncells != c->ncells || src->nlambda != c->nlambda || !src->lv || !src->cdf || !src->ltot)
        return fail(c, SKIRT_ERR_ARG, "cell sources do not match the grid and wavelengths");
    if (!(src->emission_bias >= 0 && src->emission_bias < 1)) return fail(c, SKIRT_ERR_ARG, "emission bias outside [0,1)");
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t nl = (size_t)c->nlambda, nc = (size_t)c->ncells;
    int rc;
    if ((rc = upload(c, c->dCellLv, src->lv, nl * nc))) return rc;
    if ((rc = upload(c, c->dCellCdf, src->cdf, nl * (nc + 1)))) return rc;
    if ((rc = upload(c, c->dCellLtot, src->ltot, nl))) return rc;
    c->cellBias = src->emission_bias;
    return buildCellGuide(c);
}

// scratch of the cell-source scans and the dust Labs sum: block sums of every wavelength (or of the
// whole dust table) plus two result slots
static int ensureEmisScratch(SkirtMcrt* c) {
    if (c->dEmisScratch) return SKIRT_OK;
    const size_t nb = (size_t)c->nlambda * (((size_t)c->ncells + kBlock - 1) / kBlock);
    const size_t nbAll = ((size_t)c->labsStride * c->nlambda + kBlock - 1) / kBlock;
    HIPCHECK(c, hipMalloc(&c->dEmisScratch, (std::max(nb, nbAll) + 2) * sizeof(double)));
    return SKIRT_OK;
}

int skirt_mcrt_upload_emissivity(SkirtMcrt* c, const SkirtEmissivityDesc* d) {
    if (!c || !d) return SKIRT_ERR_ARG;
    if (c->gridKind < 0 || !c->dRho) return fail(c, SKIRT_ERR_STATE, "upload the grid and media before the emissivity");
    if (d->ncells != c->ncells || d->nlambda != c->nlambda || d->ncomp != c->ncomp || d->ntemp < 2)
        return fail(c, SKIRT_ERR_ARG, "emissivity tables do not match the grid, wavelengths and media");
    HIPCHECK(c, hipSetDevice(c->device));
    const size_t nl = (size_t)d->nlambda, nh = (size_t)d->ncomp;
    int rc;
    if ((rc = upload(c, c->dEmisVolume, d->volume, (size_t)d->ncells))) return rc;
    if ((rc = upload(c, c->dEmisKabs, d->kabs, nh * nl))) return rc;
    if ((rc = upload(c, c->dEmisSigma, d->sigmaabs, nh * nl))) return rc;
    if ((rc = upload(c, c->dEmisMu, d->mu, nh))) return rc;
    if ((rc = upload(c, c->dEmisTv, d->tv, (size_t)d->ntemp))) return rc;
    if ((rc = upload(c, c->dEmisPlanck, d->planckabs, nh * d->ntemp))) return rc;
    if ((rc = upload(c, c->dEmisLambda, d->lambda, nl))) return rc;
    if ((rc = upload(c, c->dEmisDlambda, d->dlambda, nl))) return rc;
    if (!c->devCell.empty() && (rc = upload(c, c->dDevCell, c->devCell.data(), c->devCell.size()))) return rc;
    c->emisNtemp = d->ntemp;
    c->cellBias = d->emission_bias;
    return SKIRT_OK;
}

int skirt_mcrt_compute_cell_sources(SkirtMcrt* c, int include_dust) {
    if (!c) return SKIRT_ERR_ARG;
    if (!c->emisNtemp) return fail(c, SKIRT_ERR_STATE, "no emissivity uploaded");
    if (!c->dLabs) return fail(c, SKIRT_ERR_STATE, "no Labs tally");
    HIPCHECK(c, hipSetDevice(c->device));
    if (include_dust) {
        int rc = ensureDustLabs(c);
        if (rc) return rc;
    }
    const int N = c->ncells, Nl = c->nlambda;
    const int nblocks = (N + kBlock - 1) / kBlock;
    auto alloc = [&](double*& p, size_t n) -> int {
        if (!p) HIPCHECK(c, hipMalloc(&p, n * sizeof(double)));
        return SKIRT_OK;
    };
    int rc;
    if ((rc = alloc(c->dCellLv, (size_t)Nl * N)) || (rc = alloc(c->dCellCdf, (size_t)Nl * (N + 1))) ||
        (rc = alloc(c->dCellLtot, (size_t)Nl)) || (rc = ensureEmisScratch(c)))
        return rc;
    EmisArgs e{};
    e.ncells = N; e.nlambda = Nl; e.ncomp = c->ncomp; e.ntemp = c->emisNtemp; e.labsStride = c->labsStride;
    e.devCell = c->devCell.empty() ? nullptr : c->dDevCell;
    e.labs = c->dLabs; e.labsDust = include_dust ? c->dLabsDust : nullptr;
    e.rho = c->dRho; e.volume = c->dEmisVolume; e.kabs = c->dEmisKabs; e.sigmaabs = c->dEmisSigma; e.mu = c->dEmisMu;
    e.Tv = c->dEmisTv; e.planckabs = c->dEmisPlanck; e.lambda = c->dEmisLambda; e.dlambda = c->dEmisDlambda;
    e.lv = c->dCellLv; e.cdf = c->dCellCdf; e.ltot = c->dCellLtot; e.blockSums = c->dEmisScratch; e.nblocks = nblocks;
    launchCellSpectra(dim3(nblocks), c->stream, e);
    launchCellBlockSum(dim3(nblocks, Nl), c->stream, e);
    launchCellScanBlocks(dim3(Nl), c->stream, e);
    launchCellCdf(dim3(nblocks, Nl), c->stream, e);
    HIPCHECK(c, hipGetLastError());
    return buildCellGuide(c);
}

int skirt_mcrt_dust_labs_total(SkirtMcrt* c, double* total) {
    if (!c || !total) return SKIRT_ERR_ARG;
    HIPCHECK(c, hipSetDevice(c->device));
    int rc = ensureDustLabs(c);
    if (rc) return rc;
    const size_t n = (size_t)c->labsStride * c->nlambda;  // unused device cells hold zeros
    if ((rc = ensureEmisScratch(c))) return rc;
    // reuse the cell-sum kernels on the dust table viewed as one "wavelength" of n cells
    EmisArgs e{};
    e.ncells = (int)n; e.nlambda = 1; e.lv = c->dLabsDust; e.blockSums = c->dEmisScratch;
    e.nblocks = (int)((n + kBlock - 1) / kBlock);
    e.ltot = c->dEmisScratch + e.nblocks;  // one slot past the block sums
    launchCellBlockSum(dim3(e.nblocks, 1), c->stream, e);
    launchCellScanBlocks(dim3(1), c->stream, e);
    HIPCHECK(c, hipGetLastError());
    HIPCHECK(c, hipMemcpyAsync(total, e.ltot, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    return SKIRT_OK;
}

int skirt_mcrt_bind_dust_labs(SkirtMcrt* c, double* d) {
    if (!c || !d) return SKIRT_ERR_ARG;
    if (c->ownLabsDust && c->dLabsDust) (void)hipFree(c->dLabsDust);
    // the Labs replicas (dLabsRep) stay: they depend on the table's size only, not on where it lives
    c->dLabsDust = d;
    c->ownLabsDust = false;
    return SKIRT_OK;
}

int skirt_mcrt_set_crossed(SkirtMcrt* c, int bins) {
    if (!c || bins < 0 || bins > (1 << 20)) return SKIRT_ERR_ARG;
    HIPCHECK(c, hipSetDevice(c->device));
    if (c->dCrossed) {
        HIPCHECK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(c->dCrossed);
        c->dCrossed = nullptr;
    }
    c->crossedBins = bins;
    if (!bins) return SKIRT_OK;
    const size_t n = (size_t)kCrossedCopies * bins;
    HIPCHECK(c, hipMalloc(&c->dCrossed, n * sizeof(unsigned long long)));
    HIPCHECK(c, hipMemsetAsync(c->dCrossed, 0, n * sizeof(unsigned long long), c->stream));
    return SKIRT_OK;
}

int skirt_mcrt_column_densities(SkirtMcrt* c, const double* rays, int n, double* out) {
    if (!c || n < 0 || (n > 0 && (!rays || !out))) return SKIRT_ERR_ARG;
    if (n == 0) return SKIRT_OK;
    if (!c->dRho) return fail(c, SKIRT_ERR_STATE, "no grid and media uploaded");
    HIPCHECK(c, hipSetDevice(c->device));
    Args a{};
    gridArgs(c, a);
    a.ldsMeshOff = a.ldsOptOff = a.ldsInstrOff = a.ldsSedOff = 0;
    double* d = nullptr;
    HIPCHECK(c, hipMalloc(&d, (size_t)n * 7 * sizeof(double)));
    int rc = SKIRT_OK;
    hipError_t e = hipMemcpyAsync(d, rays, (size_t)n * 6 * sizeof(double), hipMemcpyHostToDevice, c->stream);
    const dim3 grid((n + kBlock - 1) / kBlock);
    if (e == hipSuccess) {
        const int kind = walkKind(c, true);
        const size_t lds = walkOf(kind).meshInLds ? (size_t)(c->nx + c->ny + c->nz + 3) * sizeof(double) : 0;
        double* res = d + 6 * (size_t)n;
        void* args[] = {&a, &d, &n, &res};  // columnKernel(Args, rays, n, out)
        e = hipLaunchKernel(columnKernelOf(kind), grid, dim3(kBlock), args, lds, c->stream);
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d + 6 * (size_t)n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(c, SKIRT_ERR_HIP, hipGetErrorString(e));
    (void)hipFree(d);
    return rc;
}

const char* skirt_mcrt_last_error(SkirtMcrt* c) { return c ? c->err.c_str() : "null context"; }

void skirt_mcrt_destroy(SkirtMcrt* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void* bufs[] = {c->dMesh, c->dBox, c->dFirstChild, c->dSplitDir, c->dFather, c->dCellnumber, c->dNbrOffset, c->dNbrList, c->dTreeT,
                    c->dLeafMap, c->dCellLv, c->dCellCdf, c->dCellGuide, c->dCellLtot, c->dCellNode, c->dEmisVolume, c->dEmisKabs,
                    c->dEmisSigma, c->dEmisMu, c->dEmisTv, c->dEmisPlanck, c->dEmisLambda, c->dEmisDlambda,
                    c->dEmisScratch, c->dDevCell, c->dSite, c->dCellBbox, c->dVorStart, c->dVorSlots,
                    c->dBlockOffset, c->dBlockSites, c->dRho,
                    c->dOptics, c->dGeomParam, c->dGeomTable, c->dLum, c->dLumtot, c->dCdf, c->dInstr,
                    c->dClaim, c->dStats, c->dError, c->dCtr, c->dPool, c->dCrossed, c->dPolTab};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    if (c->hCtr) (void)hipHostFree(c->hCtr);
    if (c->ownLabs && c->dLabs) (void)hipFree(c->dLabs);
    if (c->ownTally && c->dTally) (void)hipFree(c->dTally);
    if (c->ownLabsDust && c->dLabsDust) (void)hipFree(c->dLabsDust);
    if (c->dLabsRep) (void)hipFree(c->dLabsRep);
    for (hipEvent_t e : c->traceEv) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->pollEv) (void)hipEventDestroy(e);
    if (c->sD) (void)hipStreamDestroy(c->sD);
    for (hipEvent_t e : {c->evDetT, c->evDet[0], c->evDet[1], c->evDetJoin})
        if (e) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
}

int skirt_mcrt_sample_positions(SkirtMcrt* c, int comp, uint64_t seed, uint64_t first, size_t n, double* pos,
                                int32_t* draws) {
    if (!c) return SKIRT_ERR_ARG;
    if (!c->dGeomParam || c->nstar < 1) return fail(c, SKIRT_ERR_STATE, "sample_positions before upload_sources");
    if (comp < 0 || comp >= c->nstar || (n && !pos)) return fail(c, SKIRT_ERR_ARG, "bad component or buffer");
    if (anisoIsKind((int)c->geomParamHost[8 * (size_t)comp + 7]))  // (its kernel is the isotropic launch's)
        return fail(c, SKIRT_ERR_UNSUPPORTED, "sample_positions: an anisotropic component's positions come with its launches (sample_launches)");
    if (n == 0) return SKIRT_OK;
    const size_t nblocks = (n + kBlock - 1) / kBlock;
    if (nblocks > 0x7fffffffu) return fail(c, SKIRT_ERR_ARG, "too many positions");
    HIPCHECK(c, hipSetDevice(c->device));
    double* dPos = nullptr;
    int* dDraws = nullptr;
    unsigned* dErr = nullptr;
    unsigned err = 0;
    int rc = SKIRT_OK;
    if (hipMalloc(&dPos, 3 * n * sizeof(double)) != hipSuccess || hipMalloc(&dDraws, n * sizeof(int)) != hipSuccess ||
        hipMalloc(&dErr, sizeof(unsigned)) != hipSuccess ||
        hipMemsetAsync(dErr, 0, sizeof(unsigned), c->stream) != hipSuccess) {
        rc = fail(c, SKIRT_ERR_HIP, "sample_positions: allocation failed");
    } else {
        launchSamplePositions(dim3((unsigned)nblocks), c->stream, c->dGeomParam, c->dGeomTable, comp, (unsigned long long)seed, (unsigned long long)first, n, dPos, dDraws, dErr);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(pos, dPos, 3 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            (draws && hipMemcpyAsync(draws, dDraws, n * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            hipMemcpyAsync(&err, dErr, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            rc = fail(c, SKIRT_ERR_HIP, "sample_positions: the kernel or a copy failed");
        else if (err & ERR_GEOM)
            rc = fail(c, SKIRT_ERR_NUMERIC, kGeomCapMessage);
    }
    if (dPos) (void)hipFree(dPos);
    if (dDraws) (void)hipFree(dDraws);
    if (dErr) (void)hipFree(dErr);
    return rc;
}

// the reference's message for a position where a kind's generateDirection / probabilityForDirection throws; null
// where the position is accepted
static const char* anisoPositionError(int kind, double r0, const double* p) {
    if (!anisoIsKind(kind) || anisoPositionValid(kind, r0, p[0], p[1], p[2])) return nullptr;
    switch (kind) {
    case SKIRT_GEOM_STELLARSURFACE:
        return "the directional probability function is not defined for positions not on the stellar surface";
    case SKIRT_GEOM_SPHEBACKGROUND:
        return "the directional probability function is not defined for positions not on the background sphere";
    case SKIRT_GEOM_CUBBACKGROUND:
        return "the directional probability function is not defined for positions not on the background cube";
    default: return "the angular probability function is not defined for positions besides the origin";
    }
}

int skirt_mcrt_sample_launches(SkirtMcrt* c, int comp, uint64_t seed, uint64_t first, size_t n, double* pos, double* dir,
                               int32_t* draws, size_t nprob, const double* prob_pos, const double* prob_dir,
                               double* prob) {
    if (!c) return SKIRT_ERR_ARG;
    if (!c->dGeomParam || c->nstar < 1) return fail(c, SKIRT_ERR_STATE, "sample_launches before upload_sources");
    if (comp < 0 || comp >= c->nstar || (n && (!pos || !dir)) || (nprob && (!prob_dir || !prob)) ||
        (nprob && !prob_pos && nprob > n))
        return fail(c, SKIRT_ERR_ARG, "bad component or buffer");
    const double* gph = c->geomParamHost.data() + 8 * (size_t)comp;
    if (prob_pos)  // checked on the host, before any launch
        for (size_t i = 0; i < nprob; i++)
            if (const char* msg = anisoPositionError((int)gph[7], gph[0], prob_pos + 3 * i)) return fail(c, SKIRT_ERR_ARG, msg);
    const size_t nthreads = std::max(n, nprob);
    if (nthreads == 0) return SKIRT_OK;
    const size_t nblocks = (nthreads + kBlock - 1) / kBlock;
    if (nblocks > 0x7fffffffu) return fail(c, SKIRT_ERR_ARG, "too many launches");
    HIPCHECK(c, hipSetDevice(c->device));
    // one allocation: positions, directions, probabilities' inputs and outputs, then the draws and the error word
    const size_t offPos = 0, offDir = offPos + 3 * n, offPpos = offDir + 3 * n, offPdir = offPpos + (prob_pos ? 3 * nprob : 0),
                 offProb = offPdir + 3 * nprob, nd = offProb + nprob;
    const size_t bytes = nd * sizeof(double) + (n + 1) * sizeof(int);
    double* buf = nullptr;
    unsigned err = 0;
    int rc = SKIRT_OK;
    if (hipMalloc(&buf, bytes) != hipSuccess) return fail(c, SKIRT_ERR_HIP, "sample_launches: allocation failed");
    int* dDraws = reinterpret_cast<int*>(buf + nd);
    unsigned* dErr = reinterpret_cast<unsigned*>(dDraws + n);
    if (hipMemsetAsync(dErr, 0, sizeof(unsigned), c->stream) != hipSuccess ||
        (prob_pos && hipMemcpyAsync(buf + offPpos, prob_pos, 3 * nprob * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) ||
        (nprob && hipMemcpyAsync(buf + offPdir, prob_dir, 3 * nprob * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess)) {
        rc = fail(c, SKIRT_ERR_HIP, "sample_launches: a copy failed");
    } else {
        launchSampleLaunches(dim3((unsigned)nblocks), c->stream, c->dGeomParam, c->dGeomTable, c->nstar, comp, (unsigned long long)seed, (unsigned long long)first, n, buf + offPos,
                           buf + offDir, dDraws, nprob, prob_pos ? buf + offPpos : nullptr, buf + offPdir, buf + offProb, dErr);
        if (hipGetLastError() != hipSuccess ||
            (n && hipMemcpyAsync(pos, buf + offPos, 3 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (n && hipMemcpyAsync(dir, buf + offDir, 3 * n * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (n && draws && hipMemcpyAsync(draws, dDraws, n * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            (nprob && hipMemcpyAsync(prob, buf + offProb, nprob * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
            hipMemcpyAsync(&err, dErr, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            rc = fail(c, SKIRT_ERR_HIP, "sample_launches: the kernel or a copy failed");
        else if (err & ERR_GEOM)
            rc = fail(c, SKIRT_ERR_NUMERIC, kGeomCapMessage);
    }
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(buf);
    return rc;
}

int skirt_mcrt_set_mueller(SkirtMcrt* c, const SkirtMuellerDesc* m) {
    if (!c) return SKIRT_ERR_ARG;
    if (!c->instr.empty()) return fail(c, SKIRT_ERR_STATE, "set_mueller after set_instruments (it changes their slots)");
    HIPCHECK(c, hipSetDevice(c->device));
    if (c->dPool) { (void)hipFree(c->dPool); c->dPool = nullptr; c->nslots = 0; }
    if (!m) {  // unpolarised, as without the call
        if (c->dPolTab) { (void)hipFree(c->dPolTab); c->dPolTab = nullptr; }
        c->polTab.clear();
        c->polNtheta = 0;
        return SKIRT_OK;
    }
    if (c->ncomp < 1 || c->nlambda < 1) return fail(c, SKIRT_ERR_STATE, "set_mueller before upload_media");
    if (m->ncomp != c->ncomp || m->nlambda != c->nlambda || m->ntheta < 2 || m->ntheta > 100000 || !m->S11 || !m->S12 ||
        !m->S33 || !m->S34 || !m->thetaX || !m->pfnorm)
        return fail(c, SKIRT_ERR_ARG, "Mueller tables do not match the media (ntheta >= 2, no null table)");
    const size_t plane = (size_t)m->ncomp * m->nlambda * m->ntheta, rows = (size_t)m->ncomp * m->nlambda;
    std::vector<double> tab(polTableWords(m->ncomp, m->nlambda, m->ntheta));
    const double* src[5] = {m->S11, m->S12, m->S33, m->S34, m->thetaX};
    for (int q = 0; q < 5; q++) std::memcpy(tab.data() + q * plane, src[q], plane * sizeof(double));
    std::memcpy(tab.data() + 5 * plane, m->pfnorm, rows * sizeof(double));
    double* phi = tab.data() + 5 * plane + rows;
    polPhiTables(nullptr, phi, phi + polNphi, phi + 2 * polNphi);
    const int rc = upload(c, c->dPolTab, tab.data(), tab.size());
    if (rc) return rc;
    c->polTab.swap(tab);
    c->polNtheta = m->ntheta;
    return SKIRT_OK;
}

int skirt_mcrt_scatterings(SkirtMcrt* c, int instrument, size_t n, const double* states, const double* deviates,
                           double* out) {
    if (!c) return SKIRT_ERR_ARG;
    if (!c->dPolTab) return fail(c, SKIRT_ERR_STATE, "scatterings before set_mueller");
    if (instrument < 0 || instrument >= (int)c->instr.size() || (n && (!states || !deviates || !out)))
        return fail(c, SKIRT_ERR_ARG, "bad instrument or buffer");
    for (size_t i = 0; i < n; i++) {
        const double ell = states[polStateWords * i + 10], h = states[polStateWords * i + 11];
        if (!(ell >= 0 && ell < c->nlambda && h >= 0 && h < c->ncomp && ell == (int)ell && h == (int)h))
            return fail(c, SKIRT_ERR_ARG, "a state's wavelength or component index is out of range");
    }
    if (n == 0) return SKIRT_OK;
    const size_t nblocks = (n + kBlock - 1) / kBlock;
    if (nblocks > 0x7fffffffu) return fail(c, SKIRT_ERR_ARG, "too many states");
    HIPCHECK(c, hipSetDevice(c->device));
    const DevInstr& ins = c->instr[instrument];
    // DistantInstrument::bfky, as Events::peelWeightPol
    const double kyx = -ins.cosphi * ins.costheta * ins.cospa - ins.sinphi * ins.sinpa;
    const double kyy = -ins.sinphi * ins.costheta * ins.cospa + ins.cosphi * ins.sinpa;
    const double kyz = +ins.sintheta * ins.cospa;
    const size_t nin = polStateWords * n, ndv = 2 * n, nout = polResultWords * n;
    double* buf = nullptr;
    int rc = SKIRT_OK;
    if (hipMalloc(&buf, (nin + ndv + nout) * sizeof(double)) != hipSuccess) {
        rc = fail(c, SKIRT_ERR_HIP, "scatterings: allocation failed");
    } else if (hipMemcpyAsync(buf, states, nin * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
               hipMemcpyAsync(buf + nin, deviates, ndv * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
        rc = fail(c, SKIRT_ERR_HIP, "scatterings: a copy failed");
    } else {
        launchScatterings(dim3((unsigned)nblocks), c->stream, c->dPolTab, c->ncomp,
                           c->nlambda, c->polNtheta, buf, buf + nin, ins.kobs[0], ins.kobs[1], ins.kobs[2], kyx, kyy, kyz, n,
                           buf + nin + ndv);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(out, buf + nin + ndv, nout * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            rc = fail(c, SKIRT_ERR_HIP, "scatterings: the kernel or a copy failed");
    }
    if (buf) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(buf);
    }
    return rc;
}

int skirt_mcrt_sample_density(int device, const SkirtDensityDesc* dens, const double* boxes, size_t n,
                              const uint32_t* words, int nsample, int mode, double* out) {
    if (!dens || dens->ncomp < 1 || !dens->geom_kind || !dens->geom_param || !dens->norm || nsample < 1 ||
        (mode != SKIRT_DENS_COMPONENTS && mode != SKIRT_DENS_NODE) || (n && (!boxes || !words || !out)))
        return SKIRT_ERR_ARG;
    for (int h = 0; h < dens->ncomp; h++) {
        const int k = dens->geom_kind[h];
        if (k < SKIRT_GEOM_PLUMMER || k > SKIRT_GEOM_CONICALSHELL) return SKIRT_ERR_ARG;
        if ((k == SKIRT_GEOM_SERSIC || k == SKIRT_GEOM_TORUS || k == SKIRT_GEOM_CONICALSHELL) &&
            (!dens->dens_table || dens->ntab < 2))
            return SKIRT_ERR_ARG;
    }
    if (n == 0) return SKIRT_OK;
    const size_t nout = n * (mode == SKIRT_DENS_NODE ? 6 : (size_t)dens->ncomp);
    const size_t nw = n * 3 * (size_t)nsample;
    const size_t ntable = dens->dens_table ? (size_t)2 * dens->ntab * dens->ncomp : 0;
    if (hipSetDevice(device) != hipSuccess) return SKIRT_ERR_HIP;
    hipStream_t st = nullptr;
    char* buf = nullptr;
    // one allocation: parameters, boxes, words, output
    const size_t offParam = 0, offNorm = offParam + 8 * (size_t)dens->ncomp * sizeof(double);
    const size_t offKind = offNorm + (size_t)dens->ncomp * sizeof(double);
    const size_t offTable = (offKind + (size_t)dens->ncomp * sizeof(int) + 15) & ~(size_t)15;
    const size_t offBoxes = (offTable + ntable * sizeof(double) + 15) & ~(size_t)15;
    const size_t offOut = (offBoxes + 6 * n * sizeof(double) + 15) & ~(size_t)15;
    const size_t offWords = (offOut + nout * sizeof(double) + 15) & ~(size_t)15;
    const size_t total = offWords + nw * sizeof(uint32_t);
    int rc = SKIRT_OK;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return SKIRT_ERR_HIP;
    if (hipMalloc(&buf, total) != hipSuccess) {
        (void)hipStreamDestroy(st);
        return SKIRT_ERR_HIP;
    }
    DensArgs d{};
    d.ncomp = dens->ncomp;
    d.ntab = dens->ntab;
    d.nsample = nsample;
    d.mode = mode;
    d.param = reinterpret_cast<const double*>(buf + offParam);
    d.norm = reinterpret_cast<const double*>(buf + offNorm);
    d.kind = reinterpret_cast<const int*>(buf + offKind);
    d.table = ntable ? reinterpret_cast<const double*>(buf + offTable) : nullptr;
    d.boxes = reinterpret_cast<const double*>(buf + offBoxes);
    d.out = reinterpret_cast<double*>(buf + offOut);
    d.words = reinterpret_cast<const uint32_t*>(buf + offWords);
    d.n = n;
    const size_t nblocks = (n + kBlock - 1) / kBlock;
    if (hipMemcpyAsync(buf + offParam, dens->geom_param, 8 * (size_t)dens->ncomp * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(buf + offNorm, dens->norm, (size_t)dens->ncomp * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(buf + offKind, dens->geom_kind, (size_t)dens->ncomp * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess ||
        (ntable && hipMemcpyAsync(buf + offTable, dens->dens_table, ntable * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess) ||
        hipMemcpyAsync(buf + offBoxes, boxes, 6 * n * sizeof(double), hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(buf + offWords, words, nw * sizeof(uint32_t), hipMemcpyHostToDevice, st) != hipSuccess ||
        nblocks > 0x7fffffffu) {
        rc = SKIRT_ERR_HIP;
    } else {
        launchDensitySample(dim3((unsigned)nblocks), st, d);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(out, buf + offOut, nout * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            rc = SKIRT_ERR_HIP;
    }
    (void)hipStreamSynchronize(st);
    (void)hipFree(buf);
    (void)hipStreamDestroy(st);
    return rc;
}

// ------------------------------------------------------------------ imported particle dust
struct SkirtParticles {
    int device = 0;
    hipStream_t st = nullptr;
    char* buf = nullptr;  // one allocation: records, separators, erf table, offsets, lists
    unsigned* dBack = nullptr;
    PartView view{};
};

void skirt_mcrt_particles_free(SkirtParticles* p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->st) (void)hipStreamSynchronize(p->st);
    if (p->buf) (void)hipFree(p->buf);
    if (p->dBack) (void)hipFree(p->dBack);
    if (p->st) (void)hipStreamDestroy(p->st);
    delete p;
}

int skirt_mcrt_particles_upload(int device, const SkirtParticlesDesc* d, SkirtParticles** out) {
    if (!out) return SKIRT_ERR_ARG;
    *out = nullptr;
    constexpr int ncell = partGrid * partGrid * partGrid, nsep = 3 * (partGrid + 1);
    if (!d || d->nparticles < 1 || !d->rec || !d->separators || !d->cell_offset || !d->cell_list || !d->erf_table)
        return SKIRT_ERR_ARG;
    // every offset and index the kernels will follow, checked here: offsets ascending from 0, ids inside the particle
    // array and ascending within a cell (the ordered merge relies on it)
    if (d->cell_offset[0] != 0) return SKIRT_ERR_ARG;
    for (int c = 0; c < ncell; c++) {
        if (d->cell_offset[c + 1] < d->cell_offset[c]) return SKIRT_ERR_ARG;
        for (int q = d->cell_offset[c]; q < d->cell_offset[c + 1]; q++) {
            const int id = d->cell_list[q];
            if (id < 0 || id >= d->nparticles || (q > d->cell_offset[c] && id <= d->cell_list[q - 1])) return SKIRT_ERR_ARG;
        }
    }
    const size_t nlist = (size_t)d->cell_offset[ncell];
    const size_t offRec = 0, offSep = offRec + (size_t)d->nparticles * sizeof(PartRec);
    const size_t offErf = offSep + nsep * sizeof(double);
    const size_t offOff = offErf + (partErfN + 1) * sizeof(double);
    const size_t offList = offOff + (ncell + 1) * sizeof(int);
    const size_t total = offList + (nlist ? nlist : 1) * sizeof(int);
    auto* p = new SkirtParticles();
    p->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&p->buf, total) != hipSuccess || hipMalloc(&p->dBack, sizeof(unsigned)) != hipSuccess ||
        hipMemcpyAsync(p->buf + offRec, d->rec, (size_t)d->nparticles * sizeof(PartRec), hipMemcpyHostToDevice, p->st) != hipSuccess ||
        hipMemcpyAsync(p->buf + offSep, d->separators, nsep * sizeof(double), hipMemcpyHostToDevice, p->st) != hipSuccess ||
        hipMemcpyAsync(p->buf + offErf, d->erf_table, (partErfN + 1) * sizeof(double), hipMemcpyHostToDevice, p->st) != hipSuccess ||
        hipMemcpyAsync(p->buf + offOff, d->cell_offset, (ncell + 1) * sizeof(int), hipMemcpyHostToDevice, p->st) != hipSuccess ||
        (nlist && hipMemcpyAsync(p->buf + offList, d->cell_list, nlist * sizeof(int), hipMemcpyHostToDevice, p->st) != hipSuccess) ||
        hipStreamSynchronize(p->st) != hipSuccess) {
        skirt_mcrt_particles_free(p);
        return SKIRT_ERR_HIP;
    }
    p->view.rec = reinterpret_cast<const PartRec*>(p->buf + offRec);
    p->view.sep = reinterpret_cast<const double*>(p->buf + offSep);
    p->view.erfTable = reinterpret_cast<const double*>(p->buf + offErf);
    p->view.cellOffset = reinterpret_cast<const int*>(p->buf + offOff);
    p->view.cellList = reinterpret_cast<const int*>(p->buf + offList);
    p->view.fdust = d->dust_fraction;
    p->view.nparticles = d->nparticles;
    *out = p;
    return SKIRT_OK;
}

namespace {
// one call of either particle kernel: items in (nin doubles each), words (sampling only), out (nout doubles each)
int runParticles(SkirtParticles* p, const double* in, size_t nin, size_t n, const uint32_t* words, int nsample, int mode,
                 size_t nout, bool massKernel, double* out, size_t* handedBack) {
    const size_t nw = words ? n * 3 * (size_t)nsample : 0;
    const int block = massKernel ? partMassBlock : kBlock;
    const size_t nblocks = (n + block - 1) / block;
    if (nblocks > 0x7fffffffu) return SKIRT_ERR_ARG;
    if (hipSetDevice(p->device) != hipSuccess) return SKIRT_ERR_HIP;
    const size_t offOut = (nin * n * sizeof(double) + 15) & ~(size_t)15;
    const size_t offWords = (offOut + nout * n * sizeof(double) + 15) & ~(size_t)15;
    char* buf = nullptr;
    if (hipMalloc(&buf, offWords + (nw ? nw : 1) * sizeof(uint32_t)) != hipSuccess) return SKIRT_ERR_HIP;
    PartArgs a{};
    a.view = p->view;
    a.nsample = nsample;
    a.mode = mode;
    a.boxes = reinterpret_cast<const double*>(buf);
    a.out = reinterpret_cast<double*>(buf + offOut);
    a.words = reinterpret_cast<const uint32_t*>(buf + offWords);
    a.n = n;
    int rc = SKIRT_OK;
    unsigned back = 0;
    if (hipMemcpyAsync(buf, in, nin * n * sizeof(double), hipMemcpyHostToDevice, p->st) != hipSuccess ||
        (nw && hipMemcpyAsync(buf + offWords, words, nw * sizeof(uint32_t), hipMemcpyHostToDevice, p->st) != hipSuccess) ||
        (massKernel && hipMemsetAsync(p->dBack, 0, sizeof(unsigned), p->st) != hipSuccess)) {
        rc = SKIRT_ERR_HIP;
    } else {
        if (massKernel) launchParticleMass(dim3((unsigned)nblocks), p->st, a, p->dBack);
        else launchParticleSample(dim3((unsigned)nblocks), p->st, a);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(out, buf + offOut, nout * n * sizeof(double), hipMemcpyDeviceToHost, p->st) != hipSuccess ||
            (massKernel && hipMemcpyAsync(&back, p->dBack, sizeof(unsigned), hipMemcpyDeviceToHost, p->st) != hipSuccess) ||
            hipStreamSynchronize(p->st) != hipSuccess)
            rc = SKIRT_ERR_HIP;
    }
    (void)hipStreamSynchronize(p->st);
    (void)hipFree(buf);
    if (handedBack) *handedBack = back;
    return rc;
}
}  // namespace

int skirt_mcrt_particles_sample(SkirtParticles* p, const double* boxes, size_t n, const uint32_t* words, int nsample,
                                int mode, double* out) {
    const bool points = mode == SKIRT_PART_POINTS;
    if (!p || (mode != SKIRT_DENS_COMPONENTS && mode != SKIRT_DENS_NODE && !points) || (!points && nsample < 1) ||
        (n && (!boxes || !out || (!points && !words))))
        return SKIRT_ERR_ARG;
    if (n == 0) return SKIRT_OK;
    return runParticles(p, boxes, points ? 3 : 6, n, points ? nullptr : words, points ? 0 : nsample, mode,
                        mode == SKIRT_DENS_NODE ? 6 : 1, false, out, nullptr);
}

int skirt_mcrt_particles_mass_in_box(SkirtParticles* p, const double* boxes, size_t n, double* out, size_t* handed_back) {
    if (handed_back) *handed_back = 0;
    if (!p || (n && (!boxes || !out))) return SKIRT_ERR_ARG;
    if (n == 0) return SKIRT_OK;
    return runParticles(p, boxes, 6, n, nullptr, 0, 0, 1, true, out, handed_back);
}

}  // extern "C"
