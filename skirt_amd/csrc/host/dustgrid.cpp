// Dust grids: every kind's cell geometry (box or volume and centre, whichcell, the random position in a cell), the
// DustGrid methods that dispatch on the kind, and one .ski parser per kind. The tree kinds' builder is treegrid.cpp,
// the Voronoi tessellation voronoi.cpp.
#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "nr.hpp"
#include "ski_parse.hpp"

namespace skirt {

// ------------------------------------------------------------ Cartesian
void CartesianGrid::cellBox(int m, double b[6]) const {
    const CartesianGrid& g = *this;
    int i = m / (g.Nz * g.Ny), j = (m / g.Nz) % g.Ny, k = m % g.Nz;  // CartesianDustGrid::box
    b[0] = g.xv[i]; b[1] = g.yv[j]; b[2] = g.zv[k];
    b[3] = g.xv[i + 1]; b[4] = g.yv[j + 1]; b[5] = g.zv[k + 1];
}
int CartesianGrid::whichcell(double x, double y, double z) const {
    int i = nr::locateFail(xv, x), j = nr::locateFail(yv, y), k = nr::locateFail(zv, z);
    if (i < 0 || j < 0 || k < 0) return -1;
    return k + Nz * j + Nz * Ny * i;
}
BoxPosition CartesianGrid::positionInCell(int m) const {
    BoxPosition p;
    cellBox(m, p.b);
    return p;
}

// ------------------------------------------------------------ octree and k-d tree
void OctreeGrid::cellBox(int m, double b[6]) const {
    int l = idv[m];
    for (int q = 0; q < 6; q++) b[q] = box[6 * (size_t)l + q];
}
int OctreeGrid::whichcell(double x, double y, double z) const {
    const double* b = &box[0];
    if (!(x >= b[0] && x <= b[3] && y >= b[1] && y <= b[4] && z >= b[2] && z <= b[5])) return -1;
    int l = 0;
    while (firstChild[l] >= 0) l = child(l, x, y, z);
    return cellnumber[l];
}
BoxPosition OctreeGrid::positionInCell(int m) const {
    BoxPosition p;
    cellBox(m, p.b);
    return p;
}

// ------------------------------------------------------------ cylinder
double Cylinder2DGrid::volume(int m) const {  // Cylinder2DDustGrid::volume
    const int i = m / Nz, k = m % Nz;
    return M_PI * (zv[k + 1] - zv[k]) * (Rv[i + 1] - Rv[i]) * (Rv[i + 1] + Rv[i]);
}
void Cylinder2DGrid::center(int m, double c[3]) const {  // Cylinder2DDustGrid::centralPositionInCell: (R, phi = 0, z)
    const int i = m / Nz, k = m % Nz;
    const double R = (Rv[i] + Rv[i + 1]) / 2.0, phi = 0.0;
    c[0] = R * std::cos(phi); c[1] = R * std::sin(phi); c[2] = (zv[k] + zv[k + 1]) / 2.0;
}
int Cylinder2DGrid::whichcell(double x, double y, double z) const {  // (Position::cylradius, height)
    int i = nr::locateFail(Rv, std::sqrt(x * x + y * y)), k = nr::locateFail(zv, z);
    if (i < 0 || k < 0) return -1;
    return k + Nz * i;
}
Cylinder2DGrid::Position Cylinder2DGrid::positionInCell(int m) const {
    const int i = m / Nz, k = m % Nz;
    return {Rv[i], Rv[i + 1], zv[k], zv[k + 1]};
}

// ------------------------------------------------------------ spheres
double SphereGrid::volume1D(int m) const {  // Sphere1DDustGrid::volume
    const double rL = rv[m], rR = rv[m + 1];
    return 4.0 * M_PI / 3.0 * (rR - rL) * (rR * rR + rR * rL + rL * rL);
}
double SphereGrid::volume2D(int m) const {  // Sphere2DDustGrid::volume (the cosines of theta, not the fixed-up array)
    const int i = m / Ntheta, k = m % Ntheta;
    return (2.0 / 3.0) * M_PI * (std::pow(rv[i + 1], 3) - std::pow(rv[i], 3)) *
           (std::cos(thetav[k]) - std::cos(thetav[k + 1]));
}
void SphereGrid::center1D(int m, double c[3]) const {  // Sphere1DDustGrid::centralPositionInCell: Position(r, 0, 0)
    c[0] = (rv[m] + rv[m + 1]) / 2.0; c[1] = 0; c[2] = 0;
}
void SphereGrid::center2D(int m, double c[3]) const {  // ...: Position(r, theta, 0, SPHERICAL)
    const int i = m / Ntheta, k = m % Ntheta;
    const double r = (rv[i] + rv[i + 1]) / 2.0;
    const double theta = (thetav[k] + thetav[k + 1]) / 2.0, phi = 0.0;
    const double costheta = std::cos(theta), sintheta = std::sin(theta);
    c[0] = r * sintheta * std::cos(phi); c[1] = r * sintheta * std::sin(phi); c[2] = r * costheta;
}
int SphereGrid::whichcell1D(double x, double y, double z) const {
    return nr::locateFail(rv, std::sqrt(x * x + y * y + z * z));
}
int SphereGrid::whichcell2D(double x, double y, double z) const {  // (Position::spherical: theta = 0 at r = 0)
    const double r = std::sqrt(x * x + y * y + z * z);
    const double theta = r == 0 ? 0.0 : std::acos(z / r);
    const int i = nr::locateFail(rv, r);
    if (i < 0) return -1;
    return nr::locateClip(thetav, theta) + Ntheta * i;
}
SphereGrid::Position1D SphereGrid::positionInCell1D(int m) const { return {rv[m], rv[m + 1]}; }
SphereGrid::Position2D SphereGrid::positionInCell2D(int m) const {
    const int i = m / Ntheta, k = m % Ntheta;
    return {rv[i] * rv[i], rv[i + 1] * rv[i + 1], thetav[k], thetav[k + 1]};
}

// ------------------------------------------------------------ any kind
void DustGrid::cellBox(int m, double b[6]) const {
    switch (kind) {
    case GridKind::Cartesian: cart.cellBox(m, b); return;
    case GridKind::Octree: tree.cellBox(m, b); return;
    case GridKind::Voronoi:
        for (int q = 0; q < 6; q++) b[q] = vor.bbox[6 * (size_t)m + q];
        return;
    case GridKind::Cylinder2D: throw std::runtime_error("a cylindrical dust cell has no Cartesian box");
    case GridKind::Sphere1D:
    case GridKind::Sphere2D: throw std::runtime_error("a spherical dust cell has no Cartesian box");
    }
}

void DustGrid::cellCenter(int m, double c[3]) const {
    switch (kind) {
    case GridKind::Voronoi:
        for (int q = 0; q < 3; q++) c[q] = vor.centroid[3 * (size_t)m + q];
        return;
    case GridKind::Cylinder2D: cyl.center(m, c); return;
    case GridKind::Sphere1D: sph.center1D(m, c); return;
    case GridKind::Sphere2D: sph.center2D(m, c); return;
    case GridKind::Cartesian:
    case GridKind::Octree: {
        double b[6];
        cellBox(m, b);
        for (int q = 0; q < 3; q++) c[q] = 0.5 * (b[q] + b[3 + q]);
        return;
    }
    }
}

double DustGrid::cellVolume(int m) const {
    switch (kind) {
    case GridKind::Voronoi: return vor.volume[m];
    case GridKind::Cylinder2D: return cyl.volume(m);
    case GridKind::Sphere1D: return sph.volume1D(m);
    case GridKind::Sphere2D: return sph.volume2D(m);
    case GridKind::Cartesian:
    case GridKind::Octree: {
        double b[6];
        cellBox(m, b);
        return (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
    }
    }
    return 0;
}

int DustGrid::whichcell(double x, double y, double z) const {
    switch (kind) {
    case GridKind::Cartesian: return cart.whichcell(x, y, z);
    case GridKind::Octree: return tree.whichcell(x, y, z);
    case GridKind::Voronoi: return vor.cellIndex(x, y, z);
    case GridKind::Cylinder2D: return cyl.whichcell(x, y, z);
    case GridKind::Sphere1D: return sph.whichcell1D(x, y, z);
    case GridKind::Sphere2D: return sph.whichcell2D(x, y, z);
    }
    return -1;
}

// ------------------------------------------------------------ .ski parsers
namespace {

// A Mesh on [0,1] (LinMesh.cpp, PowMesh.cpp, SymPowMesh.cpp, LogMesh.cpp; NR::lingrid, NR::powgrid,
// NR::sympowgrid, NR::zerologgrid, Fundamentals/NR.hpp:171-289): its N+1 borders. LogMesh is an AnchoredMesh,
// not a MoveableMesh, so only a property of type Mesh accepts it.
std::vector<double> unitMesh(const Ctx& c, const XmlElement* me, int& N, bool allowLog) {
    N = attrInt(me, "numBins", 100);
    if (N < 1) throw std::runtime_error("the number of mesh bins should be positive");
    std::vector<double> tv(N + 1);
    auto lingrid = [&](int n) {
        const double dx = (1.0 - 0.0) / n;
        for (int i = 0; i <= n; i++) tv[i] = 0.0 + i * dx;
    };
    if (me->name == "LinMesh") {
        lingrid(N);
    } else if (me->name == "PowMesh" || me->name == "SymPowMesh") {
        const double ratio = attr(c, me, "ratio", "", 1.0);
        if (!(ratio > 0)) throw std::runtime_error("the bin width ratio should be positive");
        const bool sym = me->name == "SymPowMesh";
        if (sym ? N <= 2 : N <= 1) lingrid(N);
        else if (std::fabs(ratio - 1.) < 1e-3) lingrid(N);
        else if (!sym) {
            const double range = 1.0 - 0.0;
            const double q = std::pow(ratio, 1. / (N - 1));
            const double qn = std::pow(q, N);
            for (int i = 0; i <= N; ++i) tv[i] = 0.0 + (1. - std::pow(q, i)) / (1. - qn) * range;
        } else {
            const double xc = 0.5 * (0.0 + 1.0);
            if (N % 2 == 0) {
                const int M = N / 2;
                const double q = std::pow(ratio, 1.0 / (M - 1.0));
                const double qM = std::pow(q, M);
                tv[M] = xc;
                for (int i = 1; i <= M; ++i) {
                    const double dxi = (1.0 - std::pow(q, i)) / (1.0 - qM) * 0.5 * (1.0 - 0.0);
                    tv[M + i] = xc + dxi;
                    tv[M - i] = xc - dxi;
                }
            } else {
                const int M = (N + 1) / 2;
                const double q = std::pow(ratio, 1.0 / (M - 1.0));
                const double qM = std::pow(q, M);
                for (int i = 1; i <= M; ++i) {
                    const double dxi = (0.5 + 0.5 * q - std::pow(q, i)) / (0.5 + 0.5 * q - qM) * 0.5 * (1.0 - 0.0);
                    tv[M - 1 + i] = xc + dxi;
                    tv[M - i] = xc - dxi;
                }
            }
        }
    } else if (me->name == "LogMesh" && allowLog) {
        // LogMesh::mesh (LogMesh.cpp): NR::zerologgrid(tv, tc, 1, N), or NR::lingrid for a single bin
        const double tc = attr(c, me, "centralBinFraction", "", 0.0);
        if (tc <= 0 || tc >= 1) throw std::runtime_error("The central bin width fraction should be within range ]0,1[");
        if (N > 1) {
            const double logxmin = std::log10(tc);
            const double dlogx = std::log10(1.0 / tc) / (N - 1);
            tv[0] = 0.0;
            for (int i = 0; i < N; i++) tv[i + 1] = std::pow(10, logxmin + i * dlogx);
        } else {
            lingrid(N);
        }
    } else {
        throw std::runtime_error("unsupported mesh " + me->name);
    }
    return tv;
}

void parseCartesianGrid(const Ctx& c, const XmlElement* ge, Model& m) {
    m.grid.kind = GridKind::Cartesian;
    CartesianGrid& g = m.grid.cart;
    g.xmin = attr(c, ge, "minX", "length", 0);
    g.xmax = attr(c, ge, "maxX", "length", 0);
    g.ymin = attr(c, ge, "minY", "length", 0);
    g.ymax = attr(c, ge, "maxY", "length", 0);
    g.zmin = attr(c, ge, "minZ", "length", 0);
    g.zmax = attr(c, ge, "maxZ", "length", 0);
    if (g.xmax <= g.xmin || g.ymax <= g.ymin || g.zmax <= g.zmin) throw std::runtime_error("invalid grid extent");
    // the MoveableMesh of each axis on [0,1] (LinMesh.cpp, PowMesh.cpp, SymPowMesh.cpp; NR::lingrid,
    // NR::powgrid, NR::sympowgrid, Fundamentals/NR.hpp:171-261), then
    // _xv = mesh*(xmax-xmin) + xmin (CartesianDustGrid.cpp:34-36)
    auto mesh = [&](const char* prop, int& N, std::vector<double>& v, double lo, double hi) {
        const std::vector<double> tv = unitMesh(c, need(ge, prop), N, false);
        v.resize(N + 1);
        for (int i = 0; i <= N; i++) v[i] = tv[i] * (hi - lo) + lo;
    };
    mesh("meshX", g.Nx, g.xv, g.xmin, g.xmax);
    mesh("meshY", g.Ny, g.yv, g.ymin, g.ymax);
    mesh("meshZ", g.Nz, g.zv, g.zmin, g.zmax);
    m.grid.ncells = g.Nx * g.Ny * g.Nz;
}

// VoronoiDustGrid::setupSelfBefore (VoronoiDustGrid.cpp:28-138): the sites for the Uniform and
// DustDensity distributions, then the tessellation
void buildVoronoiGrid(const Ctx& c, const XmlElement* ge, Model& m, UniformSource& rng) {
    const double xmin = attr(c, ge, "minX", "length", 0), xmax = attr(c, ge, "maxX", "length", 0);
    const double ymin = attr(c, ge, "minY", "length", 0), ymax = attr(c, ge, "maxY", "length", 0);
    const double zmin = attr(c, ge, "minZ", "length", 0), zmax = attr(c, ge, "maxZ", "length", 0);
    const int N = attrInt(ge, "numParticles", 0);
    const std::string dist = ge->get("distribution", "DustDensity");
    if (dist != "SPHParticles" && N < 10) throw std::runtime_error("The number of particles should be at least 10");
    auto contains = [&](double x, double y, double z) {  // Box::contains
        return x >= xmin && x <= xmax && y >= ymin && y <= ymax && z >= zmin && z <= zmax;
    };
    std::vector<double> sites(dist == "SPHParticles" ? 0 : 3 * (size_t)N);
    if (dist == "SPHParticles") {
        // VoronoiMesh(DustParticleInterface*, extent): the particle centres inside the extent, in file order
        if (!m.particles) throw std::runtime_error("Can't retrieve particle locations from this dust distribution");
        for (const PartRec& r : m.particles->rec)
            if (contains(r.x, r.y, r.z)) sites.insert(sites.end(), {r.x, r.y, r.z});
    } else if (dist == "DustDensity" && m.particles) {
        // SPHDustDistribution::generatePosition; points outside the domain are redrawn
        for (int q = 0; q < N; q++) {
            while (true) {
                double x, y, z;
                m.particles->generatePosition(rng, [](UniformSource& r) { return gaussDeviate(r); }, x, y, z);
                if (contains(x, y, z)) {
                    sites[3 * q] = x; sites[3 * q + 1] = y; sites[3 * q + 2] = z;
                    break;
                }
            }
        }
    } else if (dist == "Uniform") {
        for (int q = 0; q < N; q++) {
            double fx = rng.uniform(), fy = rng.uniform(), fz = rng.uniform();  // Random::position(extent)
            sites[3 * q] = xmin + fx * (xmax - xmin);
            sites[3 * q + 1] = ymin + fy * (ymax - ymin);
            sites[3 * q + 2] = zmin + fz * (zmax - zmin);
        }
    } else if (dist == "DustDensity") {
        // CompDustDistribution::generatePosition: a component by mass (NR::locate_clip on the normalized
        // cumulative masses), then its geometry's generatePosition; points outside the domain are redrawn
        std::vector<double> masses, cum;
        for (const DustComp& d : m.dust) masses.push_back(d.nf);
        nr::cdf(cum, masses);
        for (int q = 0; q < N; q++) {
            while (true) {
                double X = rng.uniform();
                int h;
                if (X < cum[0]) h = 0;
                else h = nr::locateBasic(cum, X, (int)cum.size() - 1);
                const Geometry& geo = m.dust[h].geom;
                // Geometry::generatePosition of the component's kind, in the reference's draw order
                double x, y, z;
                if (!geometryPosition(geo, rng, x, y, z))
                    throw std::runtime_error("a TorusGeometry or ConicalShellGeometry found no position in 65536 attempts");
                if (contains(x, y, z)) {
                    sites[3 * q] = x; sites[3 * q + 1] = y; sites[3 * q + 2] = z;
                    break;
                }
            }
        }
    } else if (dist == "DustTesselation" || dist == "File") {
        throw std::runtime_error("the Voronoi particle distribution " + dist +
                                 " is not supported (imported Voronoi meshes are out of scope)");
    } else {
        throw std::runtime_error("unsupported Voronoi particle distribution " + dist);
    }
    StageTimer st("tessellation");
    buildVoronoi(m.grid.vor, sites, xmin, xmax, ymin, ymax, zmin, zmax, c.sampler ? c.sampler->voronoiCells() : nullptr);
}

// CylinderDustGrid::setupSelfBefore, Cylinder2DDustGrid::setupSelfAfter
void parseCylinder2DGrid(const Ctx& c, const XmlElement* ge, Model& m) {
    m.grid.kind = GridKind::Cylinder2D;
    Cylinder2DGrid& g = m.grid.cyl;
    g.Rmax = attr(c, ge, "maxR", "length", 0);
    g.zmin = attr(c, ge, "minZ", "length", 0);
    g.zmax = attr(c, ge, "maxZ", "length", 0);
    if (g.Rmax <= 0) throw std::runtime_error("The outer radius of the grid should be positive");
    if (g.zmax <= g.zmin) throw std::runtime_error("The extent of the Cylinder should be positive in the Z direction");
    const std::vector<double> tR = unitMesh(c, need(ge, "meshR"), g.NR, true);
    const std::vector<double> tz = unitMesh(c, need(ge, "meshZ"), g.Nz, false);
    g.Rv.resize(g.NR + 1);
    g.zv.resize(g.Nz + 1);
    for (int i = 0; i <= g.NR; i++) g.Rv[i] = tR[i] * g.Rmax;
    for (int k = 0; k <= g.Nz; k++) g.zv[k] = tz[k] * (g.zmax - g.zmin) + g.zmin;
    m.grid.ncells = g.NR * g.Nz;
}

// SphereDustGrid::setupSelfBefore, Sphere1DDustGrid::setupSelfAfter, Sphere2DDustGrid::setupSelfAfter
void parseSphereGrid(const Ctx& c, const XmlElement* ge, Model& m) {
    const bool two = ge->name == "Sphere2DDustGrid";
    m.grid.kind = two ? GridKind::Sphere2D : GridKind::Sphere1D;
    SphereGrid& g = m.grid.sph;
    g.rmax = attr(c, ge, "maxR", "length", 0);
    if (g.rmax <= 0) throw std::runtime_error("The outer radius of the grid should be positive");
    const std::vector<double> tr = unitMesh(c, need(ge, "meshR"), g.Nr, true);
    g.rv.resize(g.Nr + 1);
    for (int i = 0; i <= g.Nr; i++) g.rv[i] = tr[i] * g.rmax;
    m.grid.ncells = g.Nr;
    if (two) {
        const std::vector<double> tt = unitMesh(c, need(ge, "meshTheta"), g.Ntheta, false);
        g.thetav.resize(g.Ntheta + 1);
        g.cv.resize(g.Ntheta + 1);
        for (int k = 0; k <= g.Ntheta; k++) g.thetav[k] = tt[k] * M_PI;
        for (int k = 0; k <= g.Ntheta; k++) g.cv[k] = std::cos(g.thetav[k]);
        g.cv[0] = 1.;
        g.cv[g.Ntheta] = -1.;
        // path() needs a border at pi/2: a cosine close to zero becomes exactly zero, else one is inserted
        int numzeroes = 0;
        for (int k = 1; k < g.Ntheta; k++)
            if (std::fabs(g.cv[k]) < 1e-9) {
                numzeroes++;
                g.cv[k] = 0.;
            }
        if (numzeroes > 1) throw std::runtime_error("There are multiple grid points very close to pi/2");
        if (numzeroes == 0) {
            const std::vector<double> orTheta = g.thetav, orC = g.cv;
            g.Ntheta++;
            g.thetav.assign(g.Ntheta + 1, M_PI_2);
            g.cv.assign(g.Ntheta + 1, 0.0);
            for (int k = 0; k < g.Ntheta; k++) {
                const int target = (orC[k] > 0) ? k : k + 1;
                g.thetav[target] = orTheta[k];
                g.cv[target] = orC[k];
            }
        }
        m.grid.ncells = g.Nr * g.Ntheta;
    }
}

// DustGrid::setupSelfBefore (DustGrid.cpp:33-38), before the grid is built, for the anisotropic sources
// only (for the other kinds models load as they did): the grid has at least the dimension of the geometry
void checkGridDimension(const XmlElement* ge, const Model& m) {
    const int dimGrid = ge->name == "Sphere1DDustGrid" ? 1
                        : (ge->name == "Sphere2DDustGrid" || ge->name == "Cylinder2DDustGrid") ? 2 : 3;
    // particle dust: SPHDustDistribution::dimension() is 3, and DustGrid::setupSelfBefore compares the grid with the
    // dust distribution
    if (m.particles && dimGrid < 3)
        throw std::runtime_error("The grid dimension " + std::to_string(dimGrid) +
                                 " is lower than the geometry dimension 3");
    int dimGeometry = 0;
    for (const Geometry& sg : m.starGeom)
        if (isAnisotropic(sg.kind)) dimGeometry = std::max(dimGeometry, anisoDimension(sg.kind));
    if (dimGeometry > dimGrid)
        throw std::runtime_error("The grid dimension " + std::to_string(dimGrid) +
                                 " is lower than the geometry dimension " + std::to_string(dimGeometry));
    // the engine's own limit: the Voronoi grid's event kernel has no anisotropic instantiation
    if (dimGeometry > 0 && ge->name == "VoronoiDustGrid")
        throw std::runtime_error("anisotropic sources are not supported on a VoronoiDustGrid");
}

void parseTreeGrid(const Ctx& c, const XmlElement* ge, Model& m) {
    m.grid.kind = GridKind::Octree;
    StageTimer st("octree");
    buildOctree(c, ge, m, m.grid.tree, ge->name == "BinTreeDustGrid");
    m.grid.ncells = (int)m.grid.tree.idv.size();
}

void parseVoronoiGrid(const Ctx& c, const XmlElement* ge, Model& m) {
    m.grid.kind = GridKind::Voronoi;
    StageTimer st("voronoi");
    buildVoronoiGrid(c, ge, m, *c.rng);
    m.grid.ncells = m.grid.vor.ncells();
}

}  // namespace

void parseDustGrid(const Ctx& c, const XmlElement* ge, Model& m) {
    checkGridDimension(ge, m);
    if (ge->name == "CartesianDustGrid") parseCartesianGrid(c, ge, m);
    else if (ge->name == "OctTreeDustGrid" || ge->name == "BinTreeDustGrid") parseTreeGrid(c, ge, m);
    else if (ge->name == "VoronoiDustGrid") parseVoronoiGrid(c, ge, m);
    else if (ge->name == "Cylinder2DDustGrid") parseCylinder2DGrid(c, ge, m);
    else if (ge->name == "Sphere1DDustGrid" || ge->name == "Sphere2DDustGrid") parseSphereGrid(c, ge, m);
    else if (ge->name == "ParticleTreeDustGrid")
        throw std::runtime_error("ParticleTreeDustGrid is not supported (use an OctTreeDustGrid or a BinTreeDustGrid)");
    else throw std::runtime_error("unsupported dust grid " + ge->name);
}

}  // namespace skirt
