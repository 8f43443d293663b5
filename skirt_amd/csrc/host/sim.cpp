// Host driver: .ski -> Model -> device engine -> outputs (include/skirt_host.h).
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/skirt_host.h"
#include "dustemission.hpp"
#include "model.hpp"
#include "outputs.hpp"
#include "workers.hpp"
#include "../device/philox.hpp"
#include "../device/polarization.hpp"

using namespace skirt;

namespace {

constexpr int kCrossedBins = 16384;  // cells-crossed histogram bins written to ds_crossed (paths of 0 .. 16383 cells);
// the device keeps one more, which counts the longer paths
thread_local std::string g_err;
}

struct SkirtSim {
    Model m;
    double setupSeconds = 0;
    uint64_t npp = 0;
    SkirtMcrt* eng = nullptr;
    int device = -1;                          // the HIP device of eng (skirt_sim_attach)
    std::vector<double> labs;                 // Ncells x Nlambda (stellar)
    std::vector<double> labsDust;             // Ncells x Nlambda (last self-absorption cycle)
    bool dustLabsOnDevice = false;            // labsDust is still to be downloaded (skirt_sim_fetch)
    std::vector<double> dustTotals;           // Labsdusttot after every self-absorption cycle
    std::vector<double> instrAll;             // concatenated, per instrument frames [slot][lambda][pixel] + SEDs
    std::vector<size_t> instrOff;             // per instrument offset into instrAll
    std::vector<std::vector<double>> frames, seds;
    // per HIP device, the sampler that holds this simulation's uploaded particle set (the set-up's, and the probes')
    std::map<int, std::shared_ptr<DensitySampler>> samplers;
    ~SkirtSim() {
        if (eng) skirt_mcrt_destroy(eng);
    }
    size_t instrTotal() const {
        size_t n = 0;
        for (auto& ins : m.instruments) {
            if (ins.hasFrames()) n += (size_t)ins.nslots() * m.wl.n() * ins.nframe();
            if (ins.hasSeds()) n += (size_t)ins.nslots() * m.wl.n();
        }
        return n;
    }
    void splitInstr() {
        frames.assign(m.instruments.size(), {});
        seds.assign(m.instruments.size(), {});
        size_t off = 0;
        for (size_t i = 0; i < m.instruments.size(); i++) {
            const Instrument& ins = m.instruments[i];
            size_t nf = ins.hasFrames() ? (size_t)ins.nslots() * m.wl.n() * ins.nframe() : 0;
            size_t ns = ins.hasSeds() ? (size_t)ins.nslots() * m.wl.n() : 0;
            frames[i].assign(instrAll.begin() + off, instrAll.begin() + off + nf);
            off += nf;
            seds[i].assign(instrAll.begin() + off, instrAll.begin() + off + ns);
            off += ns;
        }
    }
};

namespace {
int check(SkirtSim* s, int rc) {
    if (rc != SKIRT_OK) g_err = s && s->eng ? skirt_mcrt_last_error(s->eng) : "engine error";
    return rc;
}
}  // namespace

namespace skirt {
// the calling thread's skirt_sim_error message (rccl_reducer.cpp: a device thread's failure, reported on
// the caller's thread)
void setSimError(const std::string& msg) { g_err = msg; }
}  // namespace skirt

extern "C" {

const char* skirt_sim_error(void) { return g_err.c_str(); }


namespace {
// SkirtGeometry parameters as SkirtSourceDesc::geom_param lays them out; returns the SKIRT_GEOM_* kind
int packGeometry(const Geometry& g, double* p) {
    for (int q = 0; q < 8; q++) p[q] = 0.0;
    switch (g.kind) {
    case GeometryKind::Point: return SKIRT_GEOM_POINT;
    case GeometryKind::Sersic: p[0] = g.reff; p[1] = g.n; p[2] = g.rho0; return SKIRT_GEOM_SERSIC;
    case GeometryKind::ExpDisk: {
        const double v[6] = {g.hR, g.hz, g.Rmax, g.zmax, g.Rmin, g.rho0};
        for (int q = 0; q < 6; q++) p[q] = v[q];
        return SKIRT_GEOM_EXPDISK;
    }
    case GeometryKind::Shell: {
        const double v[6] = {g.rmin, g.rmax, g.p, g.smin, g.sdiff, g.A};
        for (int q = 0; q < 6; q++) p[q] = v[q];
        return SKIRT_GEOM_SHELL;
    }
    case GeometryKind::Gamma: p[0] = g.b; p[1] = g.gamma; p[2] = g.rho0; return SKIRT_GEOM_GAMMA;
    case GeometryKind::Gaussian: p[0] = g.sigma; p[1] = g.q; p[2] = g.rho0; return SKIRT_GEOM_GAUSSIAN;
    case GeometryKind::TTauriDisk: {
        const double v[5] = {g.rmin, g.rmax, g.Rd, g.zd, g.rho0};
        for (int q = 0; q < 5; q++) p[q] = v[q];
        return SKIRT_GEOM_TTAURIDISK;
    }
    case GeometryKind::Torus:
    case GeometryKind::ConicalShell: {
        const double v[7] = {g.p, g.q, g.rmin, g.rmax, g.rani ? 1.0 : 0.0, g.rcut, g.A};
        for (int q = 0; q < 7; q++) p[q] = v[q];
        return g.kind == GeometryKind::Torus ? SKIRT_GEOM_TORUS : SKIRT_GEOM_CONICALSHELL;
    }
    case GeometryKind::Netzer:
    case GeometryKind::StellarSurface:
    case GeometryKind::SpheBackground:
    case GeometryKind::CubBackground:
    case GeometryKind::SolarPatch:
    case GeometryKind::Laser: p[0] = g.r0; return (int)g.kind;  // (SKIRT_GEOM_* are the kinds' values: asserted below)
    default: p[0] = g.c; p[1] = g.rho0; return SKIRT_GEOM_PLUMMER;
    }
}
static_assert((int)GeometryKind::Netzer == SKIRT_GEOM_NETZER && (int)GeometryKind::Laser == SKIRT_GEOM_LASER &&
                  (int)GeometryKind::CubBackground == SKIRT_GEOM_CUBBACKGROUND,
              "the anisotropic kinds of model.hpp are the C ABI's");
// the first words of a TorusGeometry's or ConicalShellGeometry's row of geom_table / dens_table
bool packGeometryTable(const Geometry& g, double* t) {
    if (g.kind != GeometryKind::Torus && g.kind != GeometryKind::ConicalShell) return false;
    t[0] = g.sinDelta; t[1] = g.sinDeltaIn; t[2] = g.smin; t[3] = g.sdiff;
    return true;
}
constexpr int kDensTab = 101;  // SersicFunction's table length: the rows of dens_table hold 2 * kDensTab doubles

static_assert((int)kDensComponents == (int)SKIRT_DENS_COMPONENTS && (int)kDensNode == (int)SKIRT_DENS_NODE,
              "density sampling modes");

static_assert(sizeof(KdNode) == sizeof(SkirtKdNode) && offsetof(KdNode, split) == offsetof(SkirtKdNode, split) &&
                  offsetof(KdNode, bmax) == offsetof(SkirtKdNode, bmax),
              "the host k-d tree node is the C ABI's SkirtKdNode");

// a Voronoi tessellation's cells on a HIP device through skirt_mcrt_voronoi_cells
VoronoiCellsFn deviceVoronoiCells(int device) {
    return [device](const std::vector<double>& sites, const double box[6], const std::vector<KdNode>& nodes,
                    const std::vector<int>& perm, int maxIds, int* ids, int* nids, double* bbox, double* volume,
                    double* centroid) {
        const int rc = skirt_mcrt_voronoi_cells(device, sites.data(), (int)(sites.size() / 3), box,
                                                reinterpret_cast<const SkirtKdNode*>(nodes.data()), (int)nodes.size(),
                                                perm.data(), maxIds, ids, nids, bbox, volume, centroid);
        if (rc)
            throw std::runtime_error("Voronoi cells on device " + std::to_string(device) + " failed (error " +
                                     std::to_string(rc) + ")");
    };
}

// the setup's density sampling (and a Voronoi grid's cells) on a HIP device through
// skirt_mcrt_sample_density (skirt_mcrt_voronoi_cells)
struct DeviceDensitySampler final : DensitySampler {
    int device;
    VoronoiCellsFn cells;
    // an imported particle set on the device: uploaded once, when first used
    const ParticleSet* uploaded = nullptr;
    SkirtParticles* parts = nullptr;
    explicit DeviceDensitySampler(int d) : device(d), cells(deviceVoronoiCells(d)) {}
    ~DeviceDensitySampler() override { skirt_mcrt_particles_free(parts); }
    const VoronoiCellsFn* voronoiCells() const override { return &cells; }
    [[noreturn]] void fail(const char* what, int rc) const {
        throw std::runtime_error(std::string(what) + " on device " + std::to_string(device) + " failed (error " +
                                 std::to_string(rc) + ")");
    }
    SkirtParticles* handle(const ParticleSet& ps) {
        if (uploaded == &ps) return parts;
        skirt_mcrt_particles_free(parts);
        parts = nullptr;
        uploaded = nullptr;
        static_assert(sizeof(PartRec) == 8 * sizeof(double), "a particle record is eight doubles");
        const SkirtParticlesDesc d{ps.size(), reinterpret_cast<const double*>(ps.rec.data()), ps.sep, ps.cellOffset.data(),
                                   ps.cellList.data(), ps.erfTable.data(), ps.fdust};
        const int rc = skirt_mcrt_particles_upload(device, &d, &parts);
        if (rc) fail("the particle upload", rc);
        uploaded = &ps;
        return parts;
    }
    void massInBox(const ParticleSet& ps, const double* boxes, size_t n, double* out, size_t* handedBack) override {
        // the boxes beyond the kernel's merge cap go to worker threads, which run beside the kernel
        std::vector<size_t> over;
        for (size_t q = 0; q < n; q++)
            if (ps.boxCells(boxes + 6 * q) > partMergeCap) over.push_back(q);
        std::vector<double> hostOut(over.size());
        SkirtParticles* h = handle(ps);
        size_t back = 0;
        int rc = SKIRT_OK;
        parallelFor(
            over.size(), 4,
            [&](size_t i0, size_t i1) {
                for (size_t i = i0; i < i1; i++) hostOut[i] = ps.massInBox(boxes + 6 * over[i]);
            },
            [&] { rc = skirt_mcrt_particles_mass_in_box(h, boxes, n, out, &back); });
        if (rc) fail("the particle mass in boxes", rc);
        if (back != over.size())
            throw std::runtime_error("the device handed back " + std::to_string(back) + " boxes, the host counted " +
                                     std::to_string(over.size()) + " beyond the merge cap");
        for (size_t i = 0; i < over.size(); i++) out[over[i]] = hostOut[i];
        if (handedBack) *handedBack = back;
    }
    void pointDensity(const ParticleSet& ps, const double* points, size_t n, double* out) override {
        const int rc = skirt_mcrt_particles_sample(handle(ps), points, n, nullptr, 0, SKIRT_PART_POINTS, out);
        if (rc) fail("the particle density", rc);
    }
    void sample(const std::vector<DustComp>& dust, const double* boxes, size_t n, const uint32_t* words, int nsample,
                int mode, double* out) override {
        if (dust.size() == 1 && dust[0].particles) {
            const int rc = skirt_mcrt_particles_sample(handle(*dust[0].particles), boxes, n, words, nsample, mode, out);
            if (rc) fail("particle density sampling", rc);
            return;
        }
        const int nc = (int)dust.size();
        std::vector<int> kind(nc);
        std::vector<double> param(8 * (size_t)nc), norm(nc), table;
        int ntab = 0;
        for (int h = 0; h < nc; h++)
            if (dust[h].geom.kind == GeometryKind::Sersic) ntab = std::max(ntab, (int)dust[h].geom.sv.size());
            else if (dust[h].geom.kind == GeometryKind::Torus || dust[h].geom.kind == GeometryKind::ConicalShell)
                ntab = std::max(ntab, kDensTab);
        if (ntab) table.assign(2 * (size_t)ntab * nc, 0.0);
        for (int h = 0; h < nc; h++) {
            const Geometry& g = dust[h].geom;
            kind[h] = packGeometry(g, &param[8 * (size_t)h]);
            norm[h] = dust[h].nf;
            if (g.kind == GeometryKind::Sersic) {
                if ((int)g.sv.size() != ntab || g.Sv.size() != g.sv.size())
                    throw std::runtime_error("Sersic density tables of unequal lengths");
                std::copy(g.sv.begin(), g.sv.end(), table.begin() + 2 * (size_t)ntab * h);
                std::copy(g.Sv.begin(), g.Sv.end(), table.begin() + 2 * (size_t)ntab * h + ntab);
            }
            packGeometryTable(g, &table[ntab ? 2 * (size_t)ntab * h : 0]);
        }
        const SkirtDensityDesc d{nc, kind.data(), param.data(), norm.data(), ntab ? table.data() : nullptr, ntab};
        const int rc = skirt_mcrt_sample_density(device, &d, boxes, n, words, nsample, mode, out);
        if (rc) throw std::runtime_error("density sampling on device " + std::to_string(device) + " failed (error " +
                                         std::to_string(rc) + ")");
    }
};
}  // namespace

SkirtSim* skirt_sim_load(const char* ski, const char* datadir, double packages, uint64_t seed) {
    return skirt_sim_load_ex(ski, datadir, packages, seed, -1);
}

SkirtSim* skirt_sim_load_ex(const char* ski, const char* datadir, double packages, uint64_t seed, int setup_device) {
    return skirt_sim_load_in(ski, datadir, packages, seed, setup_device, nullptr);
}

SkirtSim* skirt_sim_load_in(const char* ski, const char* datadir, double packages, uint64_t seed, int setup_device,
                            const char* input_path) {
    try {
        auto s = std::make_unique<SkirtSim>();
        auto t0 = std::chrono::steady_clock::now();
        unsigned long theSeed = seed ? (unsigned long)seed : readSkiSeed(ski);
        // a seed of 0 (mod 2^32) fills the generator's state with zeros: it emits only zeros, which the
        // deviates reject forever (the reference hangs in its setup); refuse it
        if ((theSeed & 0xffffffffUL) == 0) throw std::runtime_error("random seed 0 (mod 2^32) is not usable");
        MTRandom mt(theSeed);  // setup draws exactly like the reference (density / tree sampling)
        std::shared_ptr<DeviceDensitySampler> sampler;
        if (setup_device >= 0) sampler.reset(new DeviceDensitySampler(setup_device));
        s->m = loadSki(ski, mt, datadir && *datadir ? datadir : defaultDataDir(), sampler.get(),
                       input_path ? input_path : "");
        if (sampler && s->m.particles) s->samplers[setup_device] = sampler;  // keeps the uploaded particle set
        s->m.seed = theSeed;
        if (packages > 0) s->m.packages = packages;
        s->npp = (uint64_t)std::ceil(s->m.packages);
        s->setupSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        s->labs.assign(s->m.hasDust && s->m.storeAbsorption ? (size_t)s->m.ncells() * s->m.wl.n() : 0, 0.0);
        s->instrAll.assign(s->instrTotal(), 0.0);
        s->splitInstr();
        return s.release();
    } catch (std::exception& e) {
        g_err = e.what();
        return nullptr;
    }
}

int skirt_sim_info(SkirtSim* s, SkirtSimInfo* o) {
    if (!s || !o) return SKIRT_ERR_ARG;
    o->pan = s->m.pan;
    o->ncells = s->m.ncells();
    o->nlambda = s->m.wl.n();
    o->ncomp = s->m.ncomp();
    o->ninstruments = (int)s->m.instruments.size();
    o->grid_kind = s->m.grid.kind == GridKind::Octree ? SKIRT_GRID_OCTREE
                   : s->m.grid.kind == GridKind::Voronoi ? SKIRT_GRID_VORONOI
                   : s->m.grid.kind == GridKind::Cylinder2D ? SKIRT_GRID_CYLINDER2D
                   : s->m.grid.kind == GridKind::Sphere1D ? SKIRT_GRID_SPHERE1D
                   : s->m.grid.kind == GridKind::Sphere2D ? SKIRT_GRID_SPHERE2D : SKIRT_GRID_CARTESIAN;
    o->nnodes = s->m.grid.kind == GridKind::Octree ? s->m.grid.tree.nnodes() : 0;
    o->npp = s->npp;
    o->total_packets = s->npp * (uint64_t)s->m.wl.n();
    o->seed = s->m.seed;
    o->store_absorption = s->m.hasDust && s->m.storeAbsorption;
    o->has_dust = s->m.hasDust;
    o->setup_seconds = s->setupSeconds;
    return SKIRT_OK;
}

int skirt_host_particle_merge_cap(void) { return partMergeCap; }

int skirt_sim_particle_info(SkirtSim* s, int* nparticles, int* nignored, int* mass_interface, double* separators) {
    if (!s || !s->m.particles) {
        g_err = "the model has no particle dust (SPHDustDistribution)";
        return SKIRT_ERR_ARG;
    }
    const ParticleSet& ps = *s->m.particles;
    if (nparticles) *nparticles = ps.size();
    if (nignored) *nignored = ps.nignored;
    if (mass_interface) *mass_interface = ps.massInterface();
    if (separators) std::copy(ps.sep, ps.sep + 3 * (partGrid + 1), separators);
    return SKIRT_OK;
}

namespace {
// the sampler of `device` that holds this simulation's particle set
DensitySampler& particleSampler(SkirtSim* s, int device) {
    auto& sp = s->samplers[device];
    if (!sp) sp.reset(new DeviceDensitySampler(device));
    return *sp;
}
}  // namespace

int skirt_sim_particle_density(SkirtSim* s, int device, size_t n, const double* points, double* out) {
    if (!s || !s->m.particles || (n && (!points || !out))) {
        g_err = "no particle dust, or a null buffer";
        return SKIRT_ERR_ARG;
    }
    try {
        const ParticleSet& ps = *s->m.particles;
        if (n == 0) return SKIRT_OK;
        if (device >= 0) particleSampler(s, device).pointDensity(ps, points, n, out);
        else for (size_t i = 0; i < n; i++) out[i] = ps.density(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
        return SKIRT_OK;
    } catch (std::exception& e) {
        g_err = e.what();
        return SKIRT_ERR_HIP;
    }
}

int skirt_sim_particle_mass_in_box(SkirtSim* s, int device, size_t n, const double* boxes, double* out,
                                   size_t* handed_back) {
    if (handed_back) *handed_back = 0;
    if (!s || !s->m.particles || (n && (!boxes || !out))) {
        g_err = "no particle dust, or a null buffer";
        return SKIRT_ERR_ARG;
    }
    try {
        const ParticleSet& ps = *s->m.particles;
        if (n == 0) return SKIRT_OK;
        if (device >= 0) particleSampler(s, device).massInBox(ps, boxes, n, out, handed_back);
        else for (size_t i = 0; i < n; i++) out[i] = ps.massInBox(boxes + 6 * i);
        return SKIRT_OK;
    } catch (std::exception& e) {
        g_err = e.what();
        return SKIRT_ERR_HIP;
    }
}

int skirt_sim_set_photon_seed(SkirtSim* s, uint64_t seed) {
    if (!s || !seed) return SKIRT_ERR_ARG;
    s->m.seed = seed;
    return SKIRT_OK;
}

}  // extern "C"

namespace {
// The descriptors skirt_sim_attach uploads (and skirt_sim_describe writes), over the model's arrays
struct Descs {
    bool hasGrid = false;
    SkirtGridDesc g{};
    SkirtMediaDesc md{};
    SkirtSourceDesc sd{};
    std::vector<SkirtInstrDesc> ids;
    std::vector<double> kext, ksca, alb, gg, gp, lum, cdf, gt;
    std::vector<int> gk;
    // a polarising model's Mueller tables, [comp][ell][theta]
    bool hasMueller = false;
    SkirtMuellerDesc mu{};
    std::vector<double> S11, S12, S33, S34, thetaX, pfnorm;
};

void buildDescs(const Model& m, Descs& d) {
    const int Nl = m.wl.n();
    if (m.hasDust) {
        d.hasGrid = true;
        SkirtGridDesc& g = d.g;
        g.ncells = m.ncells();
        if (m.grid.kind == GridKind::Voronoi) {
            const VoronoiGrid& v = m.grid.vor;
            g.kind = SKIRT_GRID_VORONOI;
            g.site = v.site.data();
            g.cell_nbr_offset = v.nbrOffset.data();
            g.cell_nbr_list = v.nbrList.data();
            g.cell_bbox = v.bbox.data();
            g.extent[0] = v.xmin; g.extent[1] = v.ymin; g.extent[2] = v.zmin;
            g.extent[3] = v.xmax; g.extent[4] = v.ymax; g.extent[5] = v.zmax;
            g.eps = v.eps;
            g.nblocks = v.nb;
            g.block_offset = v.blockOffset.data();
            g.block_list = v.blockList.data();
        } else if (m.grid.kind == GridKind::Cartesian) {
            g.kind = SKIRT_GRID_CARTESIAN;
            g.nx = m.grid.cart.Nx; g.ny = m.grid.cart.Ny; g.nz = m.grid.cart.Nz;
            g.xv = m.grid.cart.xv.data(); g.yv = m.grid.cart.yv.data(); g.zv = m.grid.cart.zv.data();
        } else if (m.grid.kind == GridKind::Cylinder2D) {
            g.kind = SKIRT_GRID_CYLINDER2D;
            g.nx = m.grid.cyl.NR; g.ny = 0; g.nz = m.grid.cyl.Nz;
            g.xv = m.grid.cyl.Rv.data(); g.zv = m.grid.cyl.zv.data();
        } else if (m.grid.kind == GridKind::Sphere1D || m.grid.kind == GridKind::Sphere2D) {
            // r borders in xv; 2D: the fixed-up cosines in yv and the polar borders in zv; extent carries maxR
            const SphereGrid& sg = m.grid.sph;
            const bool two = m.grid.kind == GridKind::Sphere2D;
            g.kind = two ? SKIRT_GRID_SPHERE2D : SKIRT_GRID_SPHERE1D;
            g.nx = sg.Nr; g.ny = sg.Ntheta; g.nz = sg.Ntheta;
            g.xv = sg.rv.data();
            if (two) { g.yv = sg.cv.data(); g.zv = sg.thetav.data(); }
            for (int q = 0; q < 3; q++) { g.extent[q] = -sg.rmax; g.extent[3 + q] = sg.rmax; }
            if (two) g.eps = 1e-11 * sg.rmax;
        } else {
            const OctreeGrid& t = m.grid.tree;
            g.kind = SKIRT_GRID_OCTREE;
            g.nnodes = t.nnodes();
            g.box = t.box.data();
            g.first_child = t.firstChild.data();
            g.split_dir = t.binary ? t.dir.data() : nullptr;
            g.cellnumber = t.cellnumber.data();
            g.nbr_offset = t.nbrOffset.data();
            g.nbr_list = t.nbrList.data();
            g.eps = t.eps;
            g.search = t.search == 0 ? SKIRT_TREE_TOPDOWN : t.search == 2 ? SKIRT_TREE_BOOKKEEPING : SKIRT_TREE_NEIGHBOR;
        }
        const int nc = m.ncomp();
        d.kext.resize(nc * Nl); d.ksca.resize(nc * Nl); d.alb.resize(nc * Nl); d.gg.resize(nc * Nl);
        for (int h = 0; h < nc; h++)
            for (int ell = 0; ell < Nl; ell++) {
                d.kext[h * Nl + ell] = m.dust[h].mix.kext[ell];
                d.ksca[h * Nl + ell] = m.dust[h].mix.ksca[ell];
                d.alb[h * Nl + ell] = m.dust[h].mix.albedo[ell];
                d.gg[h * Nl + ell] = m.dust[h].mix.g[ell];
            }
        d.md = SkirtMediaDesc{m.ncells(), nc, Nl, m.rho.data(), d.kext.data(), d.ksca.data(), d.alb.data(), d.gg.data()};
        if (m.polarization) {
            d.hasMueller = true;
            const int nt = m.dust[0].mix.ntheta;  // (the same for every mix: loadSki checks)
            for (int h = 0; h < nc; h++) {
                const DustMix& x = m.dust[h].mix;
                d.S11.insert(d.S11.end(), x.S11.begin(), x.S11.end());
                d.S12.insert(d.S12.end(), x.S12.begin(), x.S12.end());
                d.S33.insert(d.S33.end(), x.S33.begin(), x.S33.end());
                d.S34.insert(d.S34.end(), x.S34.begin(), x.S34.end());
                d.thetaX.insert(d.thetaX.end(), x.thetaX.begin(), x.thetaX.end());
                d.pfnorm.insert(d.pfnorm.end(), x.pfnorm.begin(), x.pfnorm.end());
            }
            d.mu = SkirtMuellerDesc{nc, Nl, nt, d.S11.data(), d.S12.data(), d.S33.data(), d.S34.data(), d.thetaX.data(),
                                    d.pfnorm.data()};
        }
    }
    const int ns = (int)m.starL.size();
    d.gk.assign(ns, SKIRT_GEOM_PLUMMER);
    d.gp.assign(8 * ns, 0.0);
    d.lum.resize(ns * Nl);
    d.cdf.resize(Nl * (ns + 1));
    for (int h = 0; h < ns; h++) {
        const Geometry& g = m.starGeom[h];
        d.gk[h] = packGeometry(g, &d.gp[8 * h]);
        if (g.kind == GeometryKind::Sersic) {
            d.gt.resize(202 * (size_t)ns, 0.0);
            for (int q = 0; q < 101; q++) {
                d.gt[202 * (size_t)h + q] = g.sv[q];
                d.gt[202 * (size_t)h + 101 + q] = g.Mv[q];
            }
        }
        if (g.kind == GeometryKind::Torus || g.kind == GeometryKind::ConicalShell) {
            d.gt.resize(202 * (size_t)ns, 0.0);
            packGeometryTable(g, &d.gt[202 * (size_t)h]);
        }
        for (int ell = 0; ell < Nl; ell++) d.lum[h * Nl + ell] = m.starL[h][ell];
    }
    for (int ell = 0; ell < Nl; ell++)
        for (int q = 0; q <= ns; q++) d.cdf[ell * (ns + 1) + q] = m.starX[ell][q];
    d.sd = SkirtSourceDesc{ns, Nl, d.gk.data(), d.gp.data(), d.lum.data(), m.starLtot.data(), d.cdf.data(),
                           m.starEmissionBias, d.gt.empty() ? nullptr : d.gt.data()};
    for (const Instrument& ins : m.instruments) {
        SkirtInstrDesc x{};
        x.kind = (int)ins.kind;
        x.nx = ins.Nx; x.ny = ins.Ny;
        x.scattering_levels = ins.scatteringLevels;
        for (int q = 0; q < 3; q++) x.kobs[q] = ins.kobs[q];
        x.sinphi = ins.sinphi; x.cosphi = ins.cosphi; x.sintheta = ins.sintheta; x.costheta = ins.costheta;
        x.sinpa = ins.sinpa; x.cospa = ins.cospa;
        x.xpmin = ins.xpmin; x.xpsiz = ins.xpsiz; x.ypmin = ins.ypmin; x.ypsiz = ins.ypsiz;
        d.ids.push_back(x);
    }
}
}  // namespace

extern "C" {

int skirt_sim_attach(SkirtSim* s, int device) {
    if (!s) return SKIRT_ERR_ARG;
    if (s->eng) { skirt_mcrt_destroy(s->eng); s->eng = nullptr; }
    int rc = skirt_mcrt_create(device, &s->eng);
    if (rc) { g_err = "cannot create the engine on device " + std::to_string(device); return rc; }
    s->device = device;
    const Model& m = s->m;
    Descs d;
    buildDescs(m, d);
    if (d.hasGrid) {
        if ((rc = check(s, skirt_mcrt_upload_grid(s->eng, &d.g)))) return rc;
        if ((rc = check(s, skirt_mcrt_upload_media(s->eng, &d.md)))) return rc;
        if (d.hasMueller && (rc = check(s, skirt_mcrt_set_mueller(s->eng, &d.mu)))) return rc;
    }
    if ((rc = check(s, skirt_mcrt_upload_sources(s->eng, &d.sd)))) return rc;
    if ((rc = check(s, skirt_mcrt_set_instruments(s->eng, d.ids.data(), (int)d.ids.size())))) return rc;
    size_t nl = 0, ni = 0;
    skirt_mcrt_tally_sizes(s->eng, &nl, &ni);
    // the device tally pads each frame pixel's slots to a 64-byte line; downloads restore this layout
    if (ni < s->instrAll.size()) { g_err = "instrument tally size mismatch"; return SKIRT_ERR_STATE; }
    // DustSystem writeCellsCrossed: the engine keeps the cells-crossed histogram for ds_crossed
    if (m.hasDust && m.writeCellsCrossed && (rc = check(s, skirt_mcrt_set_crossed(s->eng, kCrossedBins + 1)))) return rc;
    return check(s, skirt_mcrt_zero_tallies(s->eng));
}

int skirt_sim_describe(SkirtSim* s, const char* path) {
    if (!s || !path) return SKIRT_ERR_ARG;
    Descs d;
    buildDescs(s->m, d);
    if (FILE* f = std::fopen(path, "wb")) std::fclose(f);  // the writer appends
    else { g_err = std::string("cannot write ") + path; return SKIRT_ERR_ARG; }
    int rc = skirt_host_write_descriptors(path, d.hasGrid ? &d.g : nullptr, d.hasGrid ? &d.md : nullptr, &d.sd,
                                          d.ids.data(), (int)d.ids.size());
    if (!rc && d.hasMueller) rc = skirt_host_write_mueller(path, &d.mu);
    if (rc) g_err = std::string("cannot write ") + path;
    return rc;
}

int skirt_sim_polarization(SkirtSim* s) { return s && s->m.hasDust && s->m.polarization ? 1 : 0; }

int skirt_sim_scatterings(SkirtSim* s, int instrument, int device, size_t n, const double* states, const double* deviates,
                          double* out) {
    if (!s || (n && (!states || !deviates || !out))) return SKIRT_ERR_ARG;
    if (!skirt_sim_polarization(s)) { g_err = "the simulation's dust mixes do not polarise"; return SKIRT_ERR_STATE; }
    if (instrument < 0 || instrument >= (int)s->m.instruments.size()) {
        g_err = "no instrument " + std::to_string(instrument);
        return SKIRT_ERR_ARG;
    }
    if (device >= 0) {
        if (!s->eng) { g_err = "no engine attached"; return SKIRT_ERR_STATE; }
        if (device != s->device) {
            g_err = "the engine is attached to device " + std::to_string(s->device) + ", not " + std::to_string(device);
            return SKIRT_ERR_ARG;
        }
        return check(s, skirt_mcrt_scatterings(s->eng, instrument, n, states, deviates, out));
    }
    // the host's compilation of the engine's routines, on the tables as the engine lays them out
    Descs d;
    buildDescs(s->m, d);
    const int nc = d.mu.ncomp, nl = d.mu.nlambda, nt = d.mu.ntheta;
    const size_t plane = (size_t)nc * nl * nt, rows = (size_t)nc * nl;
    std::vector<double> tab(polTableWords(nc, nl, nt));
    const double* src[5] = {d.mu.S11, d.mu.S12, d.mu.S33, d.mu.S34, d.mu.thetaX};
    for (int q = 0; q < 5; q++) std::copy(src[q], src[q] + plane, tab.begin() + q * plane);
    std::copy(d.mu.pfnorm, d.mu.pfnorm + rows, tab.begin() + 5 * plane);
    double* phi = tab.data() + 5 * plane + rows;
    polPhiTables(nullptr, phi, phi + polNphi, phi + 2 * polNphi);
    const Instrument& ins = s->m.instruments[instrument];
    for (size_t i = 0; i < n; i++) {
        const double ell = states[polStateWords * i + 10], h = states[polStateWords * i + 11];
        if (!(ell >= 0 && ell < nl && h >= 0 && h < nc && ell == (int)ell && h == (int)h)) {
            g_err = "a state's wavelength or component index is out of range";
            return SKIRT_ERR_ARG;
        }
        polProbeOne(tab.data(), nc, nl, nt, states + polStateWords * i, deviates + 2 * i, ins.kobs, ins.ky,
                    out + polResultWords * i);
    }
    return SKIRT_OK;
}

SkirtMcrt* skirt_sim_engine(SkirtSim* s) { return s ? s->eng : nullptr; }

int skirt_sim_sample_positions(SkirtSim* s, int comp, int device, uint64_t seed, uint64_t first, size_t n, double* pos,
                               int32_t* draws) {
    if (!s || (n && !pos)) return SKIRT_ERR_ARG;
    if (comp < 0 || comp >= (int)s->m.starGeom.size()) {
        g_err = "no stellar component " + std::to_string(comp);
        return SKIRT_ERR_ARG;
    }
    if (device >= 0) {
        if (!s->eng) { g_err = "no engine attached"; return SKIRT_ERR_STATE; }
        return check(s, skirt_mcrt_sample_positions(s->eng, comp, seed, first, n, pos, draws));
    }
    // the host's position templates (model.hpp) on the engine's per-packet streams
    const Geometry& g = s->m.starGeom[comp];
    for (size_t i = 0; i < n; i++) {
        skirt_dev::PacketRng rng;
        rng.start(seed, SKIRT_POSITIONS_TAG, first + i);
        if (!geometryPosition(g, rng, pos[3 * i], pos[3 * i + 1], pos[3 * i + 2])) {
            g_err = "a TorusGeometry or ConicalShellGeometry found no position in 65536 attempts";
            return SKIRT_ERR_NUMERIC;
        }
        if (draws) draws[i] = (int32_t)(2u * rng.block - (rng.have ? 1u : 0u));
    }
    return SKIRT_OK;
}

int skirt_sim_sample_launches(SkirtSim* s, int comp, int device, uint64_t seed, uint64_t first, size_t n, double* pos,
                              double* dir, int32_t* draws, size_t nprob, const double* prob_pos, const double* prob_dir,
                              double* prob) {
    if (!s || (n && (!pos || !dir)) || (nprob && (!prob_dir || !prob))) return SKIRT_ERR_ARG;
    if (comp < 0 || comp >= (int)s->m.starGeom.size()) {
        g_err = "no stellar component " + std::to_string(comp);
        return SKIRT_ERR_ARG;
    }
    if (nprob && !prob_pos && nprob > n) {
        g_err = "more directions than launched positions";
        return SKIRT_ERR_ARG;
    }
    if (device >= 0) {
        if (!s->eng) { g_err = "no engine attached"; return SKIRT_ERR_STATE; }
        if (device != s->device) {
            g_err = "the engine is attached to device " + std::to_string(s->device) + ", not " + std::to_string(device);
            return SKIRT_ERR_ARG;
        }
        return check(s, skirt_mcrt_sample_launches(s->eng, comp, seed, first, n, pos, dir, draws, nprob, prob_pos, prob_dir,
                                                   prob));
    }
    const Geometry& g = s->m.starGeom[comp];
    const bool aniso = isAnisotropic(g.kind);
    // a position where the reference's functions throw, in its words, before anything runs
    if (aniso && prob_pos)
        for (size_t i = 0; i < nprob; i++) {
            const double* p = prob_pos + 3 * i;
            if (anisoPositionValid((int)g.kind, g.r0, p[0], p[1], p[2])) continue;
            g_err = g.kind == GeometryKind::StellarSurface
                        ? "the directional probability function is not defined for positions not on the stellar surface"
                    : g.kind == GeometryKind::SpheBackground
                        ? "the directional probability function is not defined for positions not on the background sphere"
                    : g.kind == GeometryKind::CubBackground
                        ? "the directional probability function is not defined for positions not on the background cube"
                        : "the angular probability function is not defined for positions besides the origin";
            return SKIRT_ERR_ARG;
        }
    // the host's compilation of the engine's routines (aniso_emission.hpp; the host's position templates and
    // Random::direction for the isotropic kinds) on the engine's per-packet streams
    std::vector<double> netzer;
    if (g.kind == GeometryKind::Netzer) {
        netzer.resize(anisoNetzerWords);
        anisoNetzerTable(netzer.data());
    }
    for (size_t i = 0; i < n; i++) {
        skirt_dev::PacketRng rng;
        rng.start(seed, SKIRT_LAUNCHES_TAG, first + i);
        double* p = pos + 3 * i;
        double* k = dir + 3 * i;
        if (!geometryPosition(g, rng, p[0], p[1], p[2])) {
            g_err = "a TorusGeometry or ConicalShellGeometry found no position in 65536 attempts";
            return SKIRT_ERR_NUMERIC;
        }
        if (aniso) anisoDirectionOf((int)g.kind, g.r0, netzer.data(), rng, p[0], p[1], p[2], k[0], k[1], k[2]);
        else radialPosition(1.0, rng, k[0], k[1], k[2]);  // Random::direction()
        if (draws) draws[i] = (int32_t)(2u * rng.block - (rng.have ? 1u : 0u));
    }
    for (size_t i = 0; i < nprob; i++) {
        const double* p = prob_pos ? prob_pos + 3 * i : pos + 3 * i;
        const double* k = prob_dir + 3 * i;
        prob[i] = aniso ? anisoProbabilityOf((int)g.kind, g.r0, p[0], p[1], p[2], k[0], k[1], k[2]) : 1.0;
    }
    return SKIRT_OK;
}

int skirt_sim_run_stellar(SkirtSim* s, uint64_t first, uint64_t count) {
    if (!s || !s->eng) { g_err = "no engine attached"; return SKIRT_ERR_STATE; }
    uint64_t total = s->npp * (uint64_t)s->m.wl.n();
    if (count == 0) count = total - std::min(first, total);
    SkirtPhaseParams p{s->m.minWeightReduction, s->m.minScattEvents, s->m.scattBias,
                       s->m.hasDust && s->m.storeAbsorption ? 1 : 0, s->m.hasDust ? 1 : 0, s->m.continuousScattering ? 1 : 0};
    return check(s, skirt_mcrt_run_stellar(s->eng, s->npp, first, count, s->m.seed, &p));
}

int skirt_sim_run_stellar_shard(SkirtSim* s, int rank, int world) {
    if (!s || !s->eng) { g_err = "no engine attached"; return SKIRT_ERR_STATE; }
    SkirtPhaseParams p{s->m.minWeightReduction, s->m.minScattEvents, s->m.scattBias,
                       s->m.hasDust && s->m.storeAbsorption ? 1 : 0, s->m.hasDust ? 1 : 0, s->m.continuousScattering ? 1 : 0};
    return check(s, skirt_mcrt_run_phase_shard(s->eng, SKIRT_PHASE_STELLAR, 0, s->npp, rank, world, s->m.seed, &p));
}

int skirt_sim_run_dust(SkirtSim* s) { return skirt_sim_run_dust_shard(s, 0, 1); }

int skirt_sim_run_dust_shard(SkirtSim* s, int rank, int world) {
    if (!s || !s->eng) { g_err = "no engine attached"; return SKIRT_ERR_STATE; }
    if (world < 1 || rank < 0 || rank >= world) {
        g_err = "bad shard (rank, world)";
        return SKIRT_ERR_ARG;
    }
    const Model& m = s->m;
    if (!(m.hasDust && m.pan && m.dustEmission)) return SKIRT_OK;  // no dust emission: nothing to do
    try {
        int rc;
        const int Nl = m.wl.n();
        // SKIRT_AMD_PHASE_TIMES: wall time of the host driver's stages (a stage ending in a device
        // synchronization includes the device work queued before it)
        static const bool timing = getenv("SKIRT_AMD_PHASE_TIMES") != nullptr;
        auto t0 = std::chrono::steady_clock::now();
        auto stage = [&](const char* what) {
            if (!timing) return;
            const auto t1 = std::chrono::steady_clock::now();
            fprintf(stderr, "[dust] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
            t0 = t1;
        };
        const std::vector<PlanckTable> tables = planckTables(m);
        stage("planck tables");
        SkirtPhaseParams p{m.minWeightReduction, m.minScattEvents, m.scattBias, 0, 1, m.continuousScattering ? 1 : 0};
        // The cell sources between phases: on the device from the device tallies (default), or on the
        // host by the restatement the oracle shares (SKIRT_AMD_HOST_SOURCES=1)
        const char* env = getenv("SKIRT_AMD_HOST_SOURCES");
        const bool hostSources = env && env[0] == '1';
        std::vector<double> lum;
        CellSources src;
        if (hostSources) {
            // the stellar phase's Labs on the host (already summed over the processes at its phase end)
            if (!s->labs.empty() && (rc = check(s, skirt_mcrt_download(s->eng, s->labs.data(), nullptr)))) return rc;
        } else {
            std::vector<double> sigma, kabs, mu, planck;
            for (int h = 0; h < m.ncomp(); h++) {
                const DustMix& mx = m.dust[h].mix;
                sigma.insert(sigma.end(), mx.sigmaabs.begin(), mx.sigmaabs.end());
                kabs.insert(kabs.end(), mx.kabs.begin(), mx.kabs.end());
                mu.push_back(mx.mu);
                planck.insert(planck.end(), tables[h].planckabs.begin(), tables[h].planckabs.end());
            }
            SkirtEmissivityDesc ed{m.ncells(), Nl, m.ncomp(), (int)tables[0].Tv.size(), m.volume.data(), kabs.data(),
                                   sigma.data(), mu.data(), tables[0].Tv.data(), planck.data(), m.wl.lambda.data(),
                                   m.wl.dlambda.data(), m.dustEmissionBias};
            if ((rc = check(s, skirt_mcrt_upload_emissivity(s->eng, &ed)))) return rc;
            stage("emissivity upload");
        }
        auto prepare = [&](bool withDust) -> int {
            if (!hostSources) return check(s, skirt_mcrt_compute_cell_sources(s->eng, withDust ? 1 : 0));
            const std::vector<double>* dust = withDust ? &s->labsDust : nullptr;
            dustEmissionSpectra(m, tables, totalLabs(m, s->labs, dust), lum);
            cellSources(m, s->labs, dust, lum, src);
            SkirtCellSourceDesc d{src.ncells, src.nlambda, src.lv.data(), src.cdf.data(), src.ltot.data(),
                                  m.dustEmissionBias};
            return check(s, skirt_mcrt_upload_cell_sources(s->eng, &d));
        };
        s->dustTotals.clear();
        if (m.selfAbsorption) {
            // PanMonteCarloSimulation::rundustselfabsorption (PanMonteCarloSimulation.cpp:109-181). The
            // first cycle's spectra come from the stellar Labs alone: the dust Labs start at zero (also
            // on the device, where an earlier run may have left its last cycle's tally)
            s->labsDust.assign((size_t)m.ncells() * Nl, 0.0);
            if ((rc = check(s, skirt_mcrt_zero_dust_labs(s->eng)))) return rc;
            SelfAbsorptionSchedule sched;
            sched.fixedCycles = m.cycles;
            uint32_t cycle = 0;
            while (sched.next()) {
                if ((rc = prepare(true))) return rc;  // calculatedustemission, Labsbolv = Labs(m)
                if ((rc = check(s, skirt_mcrt_zero_dust_labs(s->eng)))) return rc;  // rebootLabsdust
                uint64_t npp = (uint64_t)std::ceil(m.packages * SelfAbsorptionSchedule::factor(sched.stage));
                // this rank's slice of every wavelength; the engine's reducer sums the dust Labs over the
                // processes at the phase end (PanDustSystem::Labsdusttot sums over processes)
                if ((rc = check(s, skirt_mcrt_run_phase_shard(s->eng, SKIRT_PHASE_DUST_SELFABS, cycle++, npp, rank,
                                                              world, m.seed, &p))))
                    return rc;
                double total = 0;
                if (hostSources) {
                    if ((rc = check(s, skirt_mcrt_download_dust_labs(s->eng, s->labsDust.data())))) return rc;
                    total = tableTotal(s->labsDust);
                } else if ((rc = check(s, skirt_mcrt_dust_labs_total(s->eng, &total)))) {
                    return rc;
                }
                s->dustTotals.push_back(total);
                sched.finishCycle(total);
                stage("self-absorption cycle");
            }
            // the final dust Labs reach the host with the other tallies (skirt_sim_fetch), not here
            s->dustLabsOnDevice = !hostSources;
        }
        // PanMonteCarloSimulation::rundustemission (PanMonteCarloSimulation.cpp:245-264)
        if ((rc = prepare(m.selfAbsorption))) return rc;
        uint64_t npp = (uint64_t)std::ceil(m.packages * m.emissionBoost);
        rc = check(s, skirt_mcrt_run_phase_shard(s->eng, SKIRT_PHASE_DUST_EMISSION, 0, npp, rank, world, m.seed, &p));
        stage("dust emission (launched)");
        return rc;
    } catch (std::exception& e) {
        g_err = e.what();
        return SKIRT_ERR_ARG;
    }
}

const double* skirt_sim_labs_dust(SkirtSim* s) {
    if (!s || s->labsDust.empty()) return nullptr;
    if (s->dustLabsOnDevice) {  // still on the device (skirt_sim_fetch not called yet): download it now
        if (!s->eng || check(s, skirt_mcrt_download_dust_labs(s->eng, s->labsDust.data()))) return nullptr;
        s->dustLabsOnDevice = false;
    }
    return s->labsDust.data();
}

int skirt_sim_selfabs_totals(SkirtSim* s, const double** totals) {
    if (!s || !totals) return -1;
    *totals = s->dustTotals.empty() ? nullptr : s->dustTotals.data();
    return (int)s->dustTotals.size();
}

int skirt_sim_fetch(SkirtSim* s) {
    if (!s || !s->eng) { g_err = "no engine attached"; return SKIRT_ERR_STATE; }
    int rc = check(s, skirt_mcrt_download(s->eng, s->labs.empty() ? nullptr : s->labs.data(),
                                          s->instrAll.empty() ? nullptr : s->instrAll.data()));
    if (rc) return rc;
    if (s->dustLabsOnDevice) {
        if ((rc = check(s, skirt_mcrt_download_dust_labs(s->eng, s->labsDust.data())))) return rc;
        s->dustLabsOnDevice = false;
    }
    s->splitInstr();
    return SKIRT_OK;
}

const double* skirt_sim_labs(SkirtSim* s) { return s && !s->labs.empty() ? s->labs.data() : nullptr; }
const double* skirt_sim_density(SkirtSim* s) { return s && !s->m.rho.empty() ? s->m.rho.data() : nullptr; }

const double* skirt_sim_instrument(SkirtSim* s, int i, int* nslots, int* nframe, int* hasFrames, int* hasSeds) {
    if (!s || i < 0 || i >= (int)s->m.instruments.size()) return nullptr;
    const Instrument& ins = s->m.instruments[i];
    if (nslots) *nslots = ins.nslots();
    if (nframe) *nframe = ins.hasFrames() ? ins.nframe() : 0;
    if (hasFrames) *hasFrames = ins.hasFrames();
    if (hasSeds) *hasSeds = ins.hasSeds();
    size_t off = 0;
    for (int q = 0; q < i; q++) {
        const Instrument& o = s->m.instruments[q];
        if (o.hasFrames()) off += (size_t)o.nslots() * s->m.wl.n() * o.nframe();
        if (o.hasSeds()) off += (size_t)o.nslots() * s->m.wl.n();
    }
    return s->instrAll.data() + off;
}

int skirt_sim_set_tallies(SkirtSim* s, const double* labs, const double* instr) {
    if (!s) return SKIRT_ERR_ARG;
    if (labs && !s->labs.empty()) std::copy(labs, labs + s->labs.size(), s->labs.begin());
    if (instr && !s->instrAll.empty()) std::copy(instr, instr + s->instrAll.size(), s->instrAll.begin());
    s->splitInstr();
    return SKIRT_OK;
}

int skirt_sim_write(SkirtSim* s, const char* prefix) {
    if (!s || !prefix) return SKIRT_ERR_ARG;
    std::string overflow;  // a limit met by ds_crossed, reported after every other output is written
    try {
        writeOutputs(s->m, prefix, s->frames, s->seds,
                     totalLabs(s->m, s->labs, s->labsDust.empty() ? nullptr : &s->labsDust));
        if (s->m.hasDust && s->m.writeCellsCrossed && s->eng) {
            std::vector<uint64_t> hist(kCrossedBins + 1);
            int rc = check(s, skirt_mcrt_download_crossed(s->eng, hist.data(), kCrossedBins + 1));
            if (rc) return rc;
            // the device's extra bin counts every longer path: the reference's _crossed grows without limit
            // (DustSystem.cpp:969), so such a path cannot be written as an exact count
            if (hist[kCrossedBins])
                overflow = "ds_crossed: " + std::to_string(hist[kCrossedBins]) + " paths crossed " +
                           std::to_string(kCrossedBins) + " or more cells, beyond the histogram's bins";
            else {
                hist.resize(kCrossedBins);
                writeCellsCrossed(s->m, prefix, hist);
            }
        }
        if (s->m.hasDust && s->m.writeConvergence && s->eng) {
            // the six half axes from the origin (DustSystem.cpp:213-242), walked by the engine
            const double rays[36] = {0, 0, 0, 1, 0, 0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 1, 0,
                                     0, 0, 0, 0, -1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, -1};
            double col[6];
            int rc = check(s, skirt_mcrt_column_densities(s->eng, rays, 6, col));
            if (rc) return rc;
            double sigma[3];
            for (int ax = 0; ax < 3; ax++) {
                sigma[ax] = 0.0;
                sigma[ax] += col[2 * ax];
                sigma[ax] += col[2 * ax + 1];
            }
            writeConvergence(s->m, prefix, sigma);
        }
    } catch (std::exception& e) {
        g_err = e.what();
        return SKIRT_ERR_ARG;
    }
    if (!overflow.empty()) {
        g_err = overflow;
        return SKIRT_ERR_UNSUPPORTED;
    }
    return SKIRT_OK;
}

void skirt_sim_free(SkirtSim* s) { delete s; }

struct SkirtVoronoi {
    VoronoiGrid g;
};

SkirtVoronoi* skirt_host_voronoi_build(const double* sites, int nsites, const double extent[6]) {
    return skirt_host_voronoi_build_ex(sites, nsites, extent, -1, nullptr);
}

SkirtVoronoi* skirt_host_voronoi_build_ex(const double* sites, int nsites, const double extent[6], int device,
                                          int* host_cells) {
    if (!sites || nsites < 1 || !extent) {
        g_err = "skirt_host_voronoi_build: no sites or no extent";
        return nullptr;
    }
    try {
        auto v = std::make_unique<SkirtVoronoi>();
        std::vector<double> sv(sites, sites + 3 * (size_t)nsites);
        const VoronoiCellsFn dev = device >= 0 ? deviceVoronoiCells(device) : VoronoiCellsFn();
        buildVoronoi(v->g, sv, extent[0], extent[3], extent[1], extent[4], extent[2], extent[5],
                     device >= 0 ? &dev : nullptr, host_cells);
        return v.release();
    } catch (std::exception& e) {
        g_err = e.what();
        return nullptr;
    }
}

int skirt_host_voronoi_cells(const SkirtVoronoi* v, double* volume, double* centroid) {
    if (!v) return SKIRT_ERR_ARG;
    if (volume) std::copy(v->g.volume.begin(), v->g.volume.end(), volume);
    if (centroid) std::copy(v->g.centroid.begin(), v->g.centroid.end(), centroid);
    return SKIRT_OK;
}

int skirt_host_voronoi_describe(const SkirtVoronoi* v, SkirtGridDesc* g) {
    if (!v || !g) return SKIRT_ERR_ARG;
    const VoronoiGrid& vg = v->g;
    g->kind = SKIRT_GRID_VORONOI;
    g->ncells = vg.ncells();
    g->site = vg.site.data();
    g->cell_nbr_offset = vg.nbrOffset.data();
    g->cell_nbr_list = vg.nbrList.data();
    g->cell_bbox = vg.bbox.data();
    g->extent[0] = vg.xmin; g->extent[1] = vg.ymin; g->extent[2] = vg.zmin;
    g->extent[3] = vg.xmax; g->extent[4] = vg.ymax; g->extent[5] = vg.zmax;
    g->eps = vg.eps;
    g->nblocks = vg.nb;
    g->block_offset = vg.blockOffset.data();
    g->block_list = vg.blockList.data();
    return SKIRT_OK;
}

void skirt_host_voronoi_free(SkirtVoronoi* v) { delete v; }

}  // extern "C"
