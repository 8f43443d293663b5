// The cell densities: DustSystem::setupSelfAfter (DustSystem.cpp:63-178), every component's density averaged over
// sampleCount random positions per cell, on the caller's random stream in the reference's order.
#include <algorithm>
#include <memory>
#include <stdexcept>

#include "ski_parse.hpp"
#include "workers.hpp"

namespace skirt {

namespace {

// a cell's density per component from the sums over its samples
void storeCellMeans(Model& m, size_t cell, const double* sumv) {
    const int Ncomp = m.ncomp();
    for (int h = 0; h < Ncomp; h++) m.rho[cell * Ncomp + h] = 1.0 * sumv[h] / m.sampleCount;
}

// sums every component's density over the cell's sampleCount positions, in sample order: position(n, p) gives
// the n-th one
template <class PositionFn>
void accumulateCell(Model& m, size_t cell, PositionFn position) {
    const int Ncomp = m.ncomp();
    std::vector<double> sumv(Ncomp, 0.0);
    for (int n = 0; n < m.sampleCount; n++) {
        double p[3];
        position(n, p);
        for (int h = 0; h < Ncomp; h++) sumv[h] += m.dust[h].density(p[0], p[1], p[2]);
    }
    storeCellMeans(m, cell, sumv.data());
}

// The grids whose random position in a cell takes three deviates: the deviates are drawn ahead in cell order
// (parallelDraws), makePosition(cell) returns the cell's position as a function of three of them.
template <class MakePosition>
void sampleCellDensities(Model& m, UniformSource& rng, MakePosition makePosition) {
    parallelDraws(rng, (size_t)m.grid.ncells, 3 * m.sampleCount, [&](size_t cell, const double* u) {
        const auto position = makePosition((int)cell);
        accumulateCell(m, cell, [&](int n, double p[3]) { position(&u[3 * n], p); });
    });
}

// The Voronoi grid: rejection sampling draws a data-dependent number of deviates, so the positions are drawn one
// cell after the other (VoronoiMesh::randomPosition, the cell's neighbour sites gathered once);
// their densities are then summed, in sample order, on worker threads, a chunk of cells at a time
void sampleVoronoiDensities(Model& m, UniformSource& rng, DensitySampler* sampler) {
    const VoronoiGrid& g = m.grid.vor;
    const int Ncells = m.grid.ncells;
    const int ns = m.sampleCount;
    MTRandom* mtr = dynamic_cast<MTRandom*>(&rng);  // a final class: its uniform() inlines
    auto uniform = [&]() { return mtr ? mtr->uniform() : rng.uniform(); };
    const int chunk = std::max(1, (1 << 22) / std::max(1, ns));
    std::vector<double> pos, nb;
    for (int c0 = 0; c0 < Ncells; c0 += chunk) {
        const int c1 = std::min(Ncells, c0 + chunk);
        pos.resize(3 * (size_t)(c1 - c0) * ns);
        std::unique_ptr<StageTimer> pst(new StageTimer("voronoi positions"));
        for (int cell = c0; cell < c1; cell++) {
            nb.clear();
            for (int q = g.nbrOffset[cell]; q < g.nbrOffset[cell + 1]; q++) {
                const int id = g.nbrList[q];
                if (id >= 0) nb.insert(nb.end(), &g.site[3 * (size_t)id], &g.site[3 * (size_t)id] + 3);
            }
            const double* b = &g.bbox[6 * (size_t)cell];
            const double* sc = &g.site[3 * (size_t)cell];
            const size_t nn = nb.size() / 3;
            for (int n = 0; n < ns; n++) {
                double p[3] = {0, 0, 0};
                bool in = false;
                for (int t = 0; t < 10000 && !in; t++) {
                    // Random::position(box) then Box::fracpos; VoronoiMesh::isPointClosestTo (any
                    // closer neighbour rejects, so the order of the checks is free: the neighbour that
                    // rejected last is checked first)
                    const double fx = uniform();
                    const double fy = uniform();
                    const double fz = uniform();
                    const double f[3] = {fx, fy, fz};
                    boxPosition(b, f, p);
                    const double x = p[0], y = p[1], z = p[2];
                    const double tx = x - sc[0], ty = y - sc[1], tz = z - sc[2];
                    const double target = tx * tx + ty * ty + tz * tz;
                    in = true;
                    for (size_t q = 0; q < nn; q++) {
                        const double dx = x - nb[3 * q], dy = y - nb[3 * q + 1], dz = z - nb[3 * q + 2];
                        if (dx * dx + dy * dy + dz * dz < target) {
                            in = false;
                            if (q) for (int d = 0; d < 3; d++) std::swap(nb[3 * q + d], nb[d]);
                            break;
                        }
                    }
                }
                if (!in) throw std::runtime_error("Can't find random position in cell");
                double* o = &pos[3 * ((size_t)(cell - c0) * ns + n)];
                o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
            }
        }
        pst.reset(new StageTimer("voronoi densities"));
        if (sampler && m.particles) {
            // particle dust on a device: the density at every position there, summed here in sample order
            std::vector<double> rhov((size_t)(c1 - c0) * ns);
            sampler->pointDensity(*m.particles, pos.data(), rhov.size(), rhov.data());
            for (int cell = c0; cell < c1; cell++) {
                double sum = 0.0;
                for (int n = 0; n < ns; n++) sum += rhov[(size_t)(cell - c0) * ns + n];
                storeCellMeans(m, cell, &sum);
            }
            continue;
        }
        parallelFor((size_t)(c1 - c0), 256, [&](size_t q0, size_t q1) {
            for (size_t q = q0; q < q1; q++)
                accumulateCell(m, c0 + q, [&](int n, double p[3]) {
                    const double* o = &pos[3 * (q * ns + n)];
                    p[0] = o[0]; p[1] = o[1]; p[2] = o[2];
                });
        });
    }
}

}  // namespace

void sampleDensities(const Ctx& c, Model& m) {
    StageTimer st("cell densities");
    UniformSource& rng = *c.rng;
    const int Ncells = m.grid.ncells, Ncomp = m.ncomp();
    m.volume.resize(Ncells);
    for (int cell = 0; cell < Ncells; cell++) m.volume[cell] = m.grid.cellVolume(cell);
    m.rho.assign((size_t)Ncells * Ncomp, 0.0);
    // the cylinder's and the spheres' positions are always the host's (the device sampler draws in boxes)
    const DustGrid& g = m.grid;
    switch (g.kind) {
    case GridKind::Voronoi: sampleVoronoiDensities(m, rng, c.sampler); return;
    case GridKind::Cylinder2D:
        sampleCellDensities(m, rng, [&](int cell) { return g.cyl.positionInCell(cell); });
        return;
    case GridKind::Sphere1D:
        sampleCellDensities(m, rng, [&](int cell) { return g.sph.positionInCell1D(cell); });
        return;
    case GridKind::Sphere2D:
        sampleCellDensities(m, rng, [&](int cell) { return g.sph.positionInCell2D(cell); });
        return;
    case GridKind::Cartesian:
    case GridKind::Octree: break;
    }
    // DustGridDensityInterface (TreeDustGrid::density, offered where the distribution has massInBox): the mass in
    // the cell's box over its volume, no draws; also for a barycentric tree
    if (g.kind == GridKind::Octree && m.particles && m.particles->massInterface()) {
        std::vector<double> boxes(6 * (size_t)Ncells), mass(Ncells);
        for (int cell = 0; cell < Ncells; cell++) g.cellBox(cell, &boxes[6 * (size_t)cell]);
        particleMasses(c, *m.particles, boxes.data(), (size_t)Ncells, mass.data());
        for (int cell = 0; cell < Ncells; cell++) {
            const double* b = &boxes[6 * (size_t)cell];
            m.rho[cell] = mass[cell] / ((b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]));  // Box::volume
        }
        return;
    }
    // Random::position(box) per sample: three deviates, drawn ahead in cell order; on the device where there is one
    const bool onDevice = deviceSampling(
        c, m.dust, (size_t)Ncells, m.sampleCount, kDensComponents,
        [&](size_t cell, double* b) { g.cellBox((int)cell, b); },
        [&](size_t cell, const double* sumv) { storeCellMeans(m, cell, sumv); });
    if (onDevice) return;
    if (g.kind == GridKind::Cartesian)
        sampleCellDensities(m, rng, [&](int cell) { return g.cart.positionInCell(cell); });
    else
        sampleCellDensities(m, rng, [&](int cell) { return g.tree.positionInCell(cell); });
}

}  // namespace skirt
