// The simulation model built from a .ski file: everything the photon-shooting hot path reads.
//
// The reference spreads this state over its SimulationItem tree (MonteCarloSimulation, StellarSystem,
// DustSystem, DustGrid, DustMix, Instrument subclasses). Here it is one plain struct of flat arrays,
// built once on the host and then handed to the device engine through the C ABI (include/skirt_mcrt.h) or to
// the CPU checker in oracle/. loadSki (build.cpp) drives the set-up, one file per subject: geometry.cpp (the
// Geometry members, the special functions, the geometry parsers), sources.cpp (wavelength grids, SEDs, the stellar
// system), dustmix.cpp, dustgrid.cpp (the grids' members and parsers), treegrid.cpp (the tree builder) and
// densities.cpp (the cell densities), with nr.hpp, workers.hpp and the internal ski_parse.hpp.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "mt_random.hpp"
#include "particles.hpp"
#include "units.hpp"
#include "voronoi.hpp"
#include "../device/aniso_emission.hpp"

namespace skirt {

// ---------------------------------------------------------------- geometries
// Reference: SKIRTcore/PlummerGeometry.cpp (density 49-54, randomradius 57-63), SpheGeometry.cpp
// (generatePosition = randomradius then isotropic direction); ExpDiskGeometry.cpp (setupSelfBefore:
// rho0; density; randomR with SpecialFunctions::LambertW1; randomz) and SepAxGeometry::generatePosition
// (R, then phi = 2 pi u, then z; Position(R, phi, z, CYLINDRICAL), Position.cpp:23-31).
// The kind values are the engine's (skirt_mcrt.h SKIRT_GEOM_*).
// SersicGeometry.cpp (setupSelfBefore, density, randomradius) with SersicFunction.cpp (its 101-point
// tables of the deprojected profile S(s) and the cumulative mass M(s), log-log interpolated) and
// SpheGeometry::generatePosition (radius, then Random::direction).
// PointGeometry.cpp: every position at the origin (no random draws), an infinite density there.
// ShellGeometry.cpp, GammaGeometry.cpp (SpheGeometry: randomradius, then Random::direction), GaussianGeometry.cpp
// (SepAxGeometry: R, phi, z), TTauriDiskGeometry.cpp and TorusGeometry.cpp, ConicalShellGeometry.cpp (AxGeometry with
// a generatePosition of their own; the last two reject positions by their density), with SpecialFunctions::gln /
// gln2 / gexp and Random::gauss. A TorusGeometry's RotateGeometryDecorator look-up does not apply (no decorators).
// NetzerAccretionDiskGeometry.cpp, StellarSurfaceGeometry.cpp, SpheBackgroundGeometry.cpp, CubBackgroundGeometry.cpp,
// SolarPatchGeometry.cpp and LaserGeometry.cpp: sources only (densities 0 or infinite), emitting anisotropically
// (AngularDistribution); their positions, directions and probabilities are device/aniso_emission.hpp's, compiled here
// for the host.
enum class GeometryKind : int {
    Plummer = 0, ExpDisk = 1, Sersic = 2, Point = 3, Shell = 4, Gamma = 5, Gaussian = 6, TTauriDisk = 7, Torus = 8,
    ConicalShell = 9, Netzer = 10, StellarSurface = 11, SpheBackground = 12, CubBackground = 13, SolarPatch = 14,
    Laser = 15
};
inline bool isAnisotropic(GeometryKind k) { return (int)k >= (int)GeometryKind::Netzer; }
// Geometry::dimension() of the anisotropic kinds (the others' is not looked at: loadSki)
inline int anisoDimension(GeometryKind k) {
    return k == GeometryKind::CubBackground ? 3
           : (k == GeometryKind::StellarSurface || k == GeometryKind::SpheBackground) ? 1 : 2;
}

// geometry.cpp: SpecialFunctions::gln, gln2, gexp (SpecialFunctions.cpp:754-791) and LambertW1
// (SpecialFunctions.cpp:579-626, the W_{-1} branch), which the position templates below call
double gln(double p, double x);
double gln2(double p, double x1, double x2);
double gexp(double p, double x);
double lambertW1(double z);

struct Geometry {
    GeometryKind kind = GeometryKind::Plummer;
    double c = 0;     // Plummer scale length
    double rho0 = 0;  // Plummer: 0.75/c^3/pi (PlummerGeometry.cpp setupSelfBefore); ExpDisk, Sersic: theirs
    double hR = 0, hz = 0, Rmax = 0, zmax = 0, Rmin = 0;  // ExpDisk scales and truncations (0: none)
    double n = 0, reff = 0, b = 0;             // Sersic index, effective radius and b(n); Gamma: its scale length b
    std::vector<double> sv, Sv, Mv;            // SersicFunction tables
    // Shell, Torus, ConicalShell: radial range, exponent p, cached smin, sdiff and normalization A.
    // Torus, ConicalShell: polar index q, (outer) half opening angle Delta and inner angle DeltaIn with their sines,
    // cos of the mean angle, anisotropic inner radius (rani) and its cutoff rcut
    double rmin = 0, rmax = 0, p = 0, smin = 0, sdiff = 0, A = 0;
    double q = 0, Delta = 0, DeltaIn = 0, sinDelta = 0, sinDeltaIn = 0, cosDelta = 0, rcut = 0;
    bool rani = false;
    // Gamma: slope gamma (scale in b); Gaussian: dispersion sigma (flattening in q); TTauriDisk: radial scale Rd and
    // axial scale zd (inner and outer radius in rmin, rmax); rho0 above for the three
    double gamma = 0, sigma = 0, Rd = 0, zd = 0;
    // StellarSurface, SpheBackground, SolarPatch: the radius; CubBackground: the extent (half-size)
    double r0 = 0;

    double density(double x, double y, double z) const;
    double sersicInverseMass(double M) const;  // SersicFunction::inversemass
    // surface densities of the normalizations (AxGeometry::SigmaR / SigmaZ, SpheGeometry::Sigmar):
    // ExpDiskGeometry.cpp SigmaR/SigmaZ, PlummerGeometry.cpp:73-77, SersicGeometry.cpp Sigmar
    double SigmaR() const;
    double SigmaZ() const;
    double Sigmar() const;
};

// ExpDiskGeometry::randomR / randomz and SepAxGeometry::generatePosition, in the reference's draw order
template <class R>
void expDiskPosition(const Geometry& g, R& rng, double& x, double& y, double& z) {
    double Rc, X;
    do {
        X = rng.uniform();
        Rc = g.hR * (-1.0 - lambertW1((X - 1.0) / M_E));
    } while ((g.Rmax > 0.0 && Rc >= g.Rmax) || Rc <= g.Rmin);
    const double phi = 2.0 * M_PI * rng.uniform();
    double zc;
    do {
        X = rng.uniform();
        zc = (X <= 0.5) ? g.hz * std::log(2.0 * X) : -g.hz * std::log(2.0 * (1.0 - X));
    } while (g.zmax > 0.0 && std::fabs(zc) >= g.zmax);
    x = Rc * std::cos(phi);
    y = Rc * std::sin(phi);
    z = zc;
}

// Direction(theta, phi) (Direction.cpp): the unit vector, the poles within 1e-8 exactly on the axis
inline void direction(double theta, double phi, double& kx, double& ky, double& kz) {
    if (theta <= 1e-8) { kx = 0; ky = 0; kz = 1; }
    else if (theta >= M_PI - 1e-8) { kx = 0; ky = 0; kz = -1; }
    else {
        const double st = std::sin(theta);
        kx = st * std::cos(phi); ky = st * std::sin(phi); kz = std::cos(theta);
    }
}

// SpheGeometry::generatePosition after randomradius: Position(r, Random::direction()), Random::direction() as
// Direction(theta, phi) with theta = acos(2u-1), phi = 2 pi u' (Random.cpp:179-184)
template <class R>
void radialPosition(double r, R& rng, double& x, double& y, double& z) {
    const double theta = std::acos(2.0 * rng.uniform() - 1.0);
    const double phi = 2.0 * M_PI * rng.uniform();
    double kx, ky, kz;
    direction(theta, phi, kx, ky, kz);
    x = r * kx; y = r * ky; z = r * kz;
}

// SersicGeometry::randomradius then SpheGeometry::generatePosition
template <class R>
void sersicPosition(const Geometry& g, R& rng, double& x, double& y, double& z) {
    radialPosition(g.reff * g.sersicInverseMass(rng.uniform()), rng, x, y, z);
}

// Random::gauss (Random.cpp:140-150)
template <class R>
double gaussDeviate(R& rng) {
    double rsq, v1, v2;
    do {
        v1 = 2.0 * rng.uniform() - 1.0;
        v2 = 2.0 * rng.uniform() - 1.0;
        rsq = v1 * v1 + v2 * v2;
    } while (rsq >= 1.0 || rsq == 0.0);
    return v2 * std::sqrt(-2.0 * std::log(rsq) / rsq);
}

// ShellGeometry::randomradius
template <class R>
void shellPosition(const Geometry& g, R& rng, double& x, double& y, double& z) {
    const double X = rng.uniform();
    const double s = g.smin + X * g.sdiff;
    radialPosition(gexp(g.p - 2.0, s), rng, x, y, z);
}

// GammaGeometry::randomradius
template <class R>
void gammaPosition(const Geometry& g, R& rng, double& x, double& y, double& z) {
    const double X = rng.uniform();
    const double t = std::pow(X, 1.0 / (3.0 - g.gamma));
    radialPosition(g.b * t / (1.0 - t), rng, x, y, z);
}

// GaussianGeometry::randomR / randomz in SepAxGeometry::generatePosition's order (R, phi, z)
template <class R>
void gaussianPosition(const Geometry& g, R& rng, double& x, double& y, double& z) {
    const double X = rng.uniform();
    const double Rc = g.sigma * std::sqrt(-2.0 * std::log(X));
    const double phi = 2.0 * M_PI * rng.uniform();
    z = (g.q * g.sigma) * gaussDeviate(rng);
    x = Rc * std::cos(phi);
    y = Rc * std::sin(phi);
}

// TTauriDiskGeometry::generatePosition (TTauriDiskGeometry.cpp:107-118): phi, R, z
template <class R>
void ttauriPosition(const Geometry& g, R& rng, double& x, double& y, double& z) {
    const double phi = 2.0 * M_PI * rng.uniform();
    const double tinn = std::pow(g.rmin, 2.125);
    const double tout = std::pow(g.rmax, 2.125);
    const double Rc = std::pow(tinn + rng.uniform() * (tout - tinn), 1.0 / 2.125);
    const double h = g.zd * std::pow(Rc / g.Rd, 1.125);
    const double sigma = std::sqrt(2.0 / M_PI) * h;
    z = gaussDeviate(rng) * sigma;
    x = Rc * std::cos(phi);
    y = Rc * std::sin(phi);
}

// the rejection loops' cap (an engine choice; the reference's loops have none)
constexpr int kGeomAttemptCap = 1 << 16;

// TorusGeometry::generatePosition (:179-201) and ConicalShellGeometry::generatePosition (:190-212); false when
// kGeomAttemptCap attempts were rejected
template <class R>
bool torusPosition(const Geometry& g, R& rng, double& x, double& y, double& z) {
    for (int attempt = 0; attempt < kGeomAttemptCap; attempt++) {
        double X = rng.uniform();
        const double s = g.smin + X * g.sdiff;
        const double r = gexp(g.p - 2.0, s);
        X = rng.uniform();
        double costheta = 0.0;
        if (g.q < 1e-3) costheta = (1.0 - 2.0 * X) * g.sinDelta;
        else {
            const double B = 1.0 - std::exp(-g.q * g.sinDelta);
            costheta = (X < 0.5) ? -std::log(1.0 - B * (1.0 - 2.0 * X)) / g.q
                                 : std::log(1.0 - B * (2.0 * X - 1.0)) / g.q;
        }
        const double theta = std::acos(costheta);
        X = rng.uniform();
        const double phi = 2.0 * M_PI * X;
        // Position(r, theta, phi, SPHERICAL), Position.cpp
        const double ct = std::cos(theta), st = std::sin(theta), cp = std::cos(phi), sp = std::sin(phi);
        const double px = r * st * cp, py = r * st * sp, pz = r * ct;
        if (g.density(px, py, pz) != 0.0) {  // density(bfr.cylradius(), bfr.height())
            x = px; y = py; z = pz;
            return true;
        }
    }
    x = y = z = 0.0;
    return false;
}

// Geometry::generatePosition of every kind; false when a rejection loop reached its cap
template <class R>
bool geometryPosition(const Geometry& g, R& rng, double& x, double& y, double& z) {
    switch (g.kind) {
    case GeometryKind::ExpDisk: expDiskPosition(g, rng, x, y, z); return true;
    case GeometryKind::Sersic: sersicPosition(g, rng, x, y, z); return true;
    case GeometryKind::Point: x = y = z = 0.0; return true;
    case GeometryKind::Shell: shellPosition(g, rng, x, y, z); return true;
    case GeometryKind::Gamma: gammaPosition(g, rng, x, y, z); return true;
    case GeometryKind::Gaussian: gaussianPosition(g, rng, x, y, z); return true;
    case GeometryKind::TTauriDisk: ttauriPosition(g, rng, x, y, z); return true;
    case GeometryKind::Torus:
    case GeometryKind::ConicalShell: return torusPosition(g, rng, x, y, z);
    case GeometryKind::Netzer:
    case GeometryKind::StellarSurface:
    case GeometryKind::SpheBackground:
    case GeometryKind::CubBackground:
    case GeometryKind::SolarPatch:
    case GeometryKind::Laser: anisoPositionOf((int)g.kind, g.r0, rng, x, y, z); return true;
    case GeometryKind::Plummer: {
        // PlummerGeometry::randomradius, then SpheGeometry::generatePosition (Random::direction)
        const double t = std::pow(rng.uniform(), 1.0 / 3.0);
        radialPosition(g.c * t / std::sqrt((1.0 - t) * (1.0 + t)), rng, x, y, z);
        return true;
    }
    }
    return true;
}

// ---------------------------------------------------------------- wavelength grid
struct WavelengthGrid {
    bool pan = false;  // issampledrange()
    std::vector<double> lambda, dlambda;
    int n() const { return (int)lambda.size(); }
    double lambdamin(int ell) const;  // WavelengthGrid.cpp lambdamin/lambdamax
    double lambdamax(int ell) const;
};

// ---------------------------------------------------------------- dust
// Reference: SKIRTcore/DustMix.cpp:44-264 (per-wavelength tables), DustMix.cpp:440-443 quirks kept.
struct DustMix {
    std::string type;
    std::vector<double> kabs, ksca, kext, albedo, g;  // per ell
    // per-population cross sections (needed for dust emission equilibrium temperatures)
    double mu = 0;
    std::vector<double> sigmaabs;  // per ell, summed over populations
    // a mix that supports polarisation (DustMix::addpolarization; ElectronDustMix.cpp): the Mueller matrix elements
    // at ntheta scattering angles per wavelength, [ell][t] row-major, and what DustMix::setupSelfAfter derives from
    // them (DustMix.cpp:96-123): the cumulative distribution of theta and the phase function's normalization
    bool polarization = false;
    int ntheta = 0;
    std::vector<double> S11, S12, S33, S34, thetaX;
    std::vector<double> pfnorm;  // per ell
};

struct DustComp {
    Geometry geom;
    DustMix mix;
    double nf = 0;  // normalization factor = dust mass (DustMassDustCompNormalization); particle dust: mass()
    // imported particle dust (SPHDustDistribution, particles.hpp): the one component's density is the particle
    // set's, geom is not looked at
    std::shared_ptr<const ParticleSet> particles;
    double density(double x, double y, double z) const {
        return particles ? particles->density(x, y, z) : nf * geom.density(x, y, z);
    }
};

// The grids of every kind, each with its cells' geometry read together (dustgrid.cpp): the box or the volume and
// central position, whichcell, and positionInCell(m), which returns the random position in cell m as a function
// of three uniform deviates, (const double u[3], double p[3]), in the reference's arithmetic. These members are the
// library's own (SKIRT_LOCAL: not among its dynamic symbols); DustGrid's four methods below are what other code calls.
#define SKIRT_LOCAL __attribute__((visibility("hidden")))

// Random::position(box) then Box::fracpos: the position at the fractions u of a box's extent
inline void boxPosition(const double b[6], const double u[3], double p[3]) {
    p[0] = b[0] + u[0] * (b[3] - b[0]);
    p[1] = b[1] + u[1] * (b[4] - b[1]);
    p[2] = b[2] + u[2] * (b[5] - b[2]);
}
struct BoxPosition {
    double b[6];
    void operator()(const double u[3], double p[3]) const { boxPosition(b, u, p); }
};

// Cartesian grid: SKIRTcore/CartesianDustGrid.cpp
struct CartesianGrid {
    int Nx = 0, Ny = 0, Nz = 0;
    double xmin = 0, xmax = 0, ymin = 0, ymax = 0, zmin = 0, zmax = 0;
    std::vector<double> xv, yv, zv;  // N+1 borders each
    SKIRT_LOCAL void cellBox(int m, double b[6]) const;
    SKIRT_LOCAL int whichcell(double x, double y, double z) const;
    SKIRT_LOCAL BoxPosition positionInCell(int m) const;
};

// Tree grids: SKIRTcore/TreeDustGrid.cpp with OctTreeNode.cpp / BaryOctTreeNode.cpp (OctTreeDustGrid) or
// BinTreeNode.cpp / BaryBinTreeNode.cpp (BinTreeDustGrid, the k-d tree), flattened breadth-first exactly
// as the reference's _tree vector: node l has children firstChild[l] .. firstChild[l]+7 (octree) or
// firstChild[l] .. firstChild[l]+1 (binary tree), or -1 for a leaf.
struct OctreeGrid {
    double xmin = 0, xmax = 0, ymin = 0, ymax = 0, zmin = 0, zmax = 0;
    double eps = 0;  // 1e-12 * |extent widths| (TreeDustGrid.cpp:76)
    int minLevel = 2, maxLevel = 6;
    int search = 1;  // 0 TopDown, 1 Neighbor, 2 Bookkeeping
    std::vector<double> box;      // 6 per node: xmin ymin zmin xmax ymax zmax
    std::vector<int> firstChild;  // per node, -1 for a leaf
    std::vector<int> father;      // per node, -1 for the root
    std::vector<int> level;       // per node
    std::vector<int> cellnumber;  // per node, -1 for non-leaves
    std::vector<int> idv;         // per cell: node index
    // neighbor lists per (node, wall), walls ordered BACK FRONT LEFT RIGHT BOTTOM TOP (TreeNode.hpp)
    std::vector<int> nbrOffset;   // 6*Nnodes+1
    std::vector<int> nbrList;
    bool binary = false;              // BinTreeDustGrid: two children per node
    std::vector<signed char> dir;     // binary trees: split axis per node (0 x, 1 y, 2 z; -1 for leaves)
    int nnodes() const { return (int)firstChild.size(); }
    // the child of non-leaf node l holding (x,y,z): OctTreeNode::child(r) (OctTreeNode.cpp:184-189) or
    // BinTreeNode::child(r) (BinTreeNode.cpp:322-331); both compare with the first child's upper corner
    int child(int l, double x, double y, double z) const {
        const int c0 = firstChild[l];
        const double* cb = &box[6 * (size_t)c0];
        if (binary) {
            const int d = dir[l];
            return c0 + ((d == 0 ? x : d == 1 ? y : z) < cb[3 + d] ? 0 : 1);
        }
        return c0 + (x < cb[3] ? 0 : 1) + (y < cb[4] ? 0 : 2) + (z < cb[5] ? 0 : 4);
    }
    SKIRT_LOCAL void cellBox(int m, double b[6]) const;  // of cell m (not node m)
    SKIRT_LOCAL int whichcell(double x, double y, double z) const;
    SKIRT_LOCAL BoxPosition positionInCell(int m) const;
};

// Axisymmetric R-z grid: SKIRTcore/Cylinder2DDustGrid.cpp (CylinderDustGrid.cpp); cell m = k + Nz*i
struct Cylinder2DGrid {
    int NR = 0, Nz = 0;
    double Rmax = 0, zmin = 0, zmax = 0;
    std::vector<double> Rv, zv;  // NR+1 radial borders (Rv[0] = 0), Nz+1 z borders
    // Cylinder2DDustGrid::randomPositionInCell: three deviates (R, phi, z)
    struct Position {
        double R0, R1, z0, z1;
        void operator()(const double u[3], double p[3]) const {
            const double R = R0 + (R1 - R0) * u[0];
            const double phi = 2.0 * M_PI * u[1];
            const double z = z0 + (z1 - z0) * u[2];
            p[0] = R * std::cos(phi); p[1] = R * std::sin(phi); p[2] = z;
        }
    };
    SKIRT_LOCAL double volume(int m) const;
    SKIRT_LOCAL void center(int m, double c[3]) const;
    SKIRT_LOCAL int whichcell(double x, double y, double z) const;
    SKIRT_LOCAL Position positionInCell(int m) const;
};

// Spherical grids: SKIRTcore/Sphere1DDustGrid.cpp (shells, cell m = i) and Sphere2DDustGrid.cpp (shells x polar
// bins, cell m = k + Ntheta*i), both on SphereDustGrid.cpp. Ntheta = 0 for the 1D grid.
struct SphereGrid {
    int Nr = 0, Ntheta = 0;
    double rmax = 0;
    std::vector<double> rv;      // Nr+1 radial borders (mesh * rmax; a LogMesh's last may miss rmax by a bit)
    std::vector<double> thetav;  // 2D: Ntheta+1 polar borders, a border pi/2 inserted where the mesh has none
    std::vector<double> cv;      // 2D: their cosines, with exact 1, 0, -1 (Sphere2DDustGrid::setupSelfAfter)
    // Sphere1DDustGrid::randomPositionInCell: Random::direction() (theta, phi), then r uniform in the shell
    struct Position1D {
        double r0, r1;
        void operator()(const double u[3], double p[3]) const {
            const double theta = std::acos(2.0 * u[0] - 1.0);
            const double phi = 2.0 * M_PI * u[1];
            double kx, ky, kz;
            direction(theta, phi, kx, ky, kz);
            const double r = r0 + (r1 - r0) * u[2];
            p[0] = r * kx; p[1] = r * ky; p[2] = r * kz;
        }
    };
    // Sphere2DDustGrid::randomPositionInCell: r, theta, phi, then Position(.., SPHERICAL)
    struct Position2D {
        double ris, ri1s, theta0, theta1;  // the squares of the shell's radii, the polar bin's borders
        void operator()(const double u[3], double p[3]) const {
            const double r = std::sqrt(ris + (ri1s - ris) * u[0]);
            const double theta = theta0 + (theta1 - theta0) * u[1];
            const double phi = 2.0 * M_PI * u[2];
            const double costheta = std::cos(theta), sintheta = std::sin(theta);
            const double cosphi = std::cos(phi), sinphi = std::sin(phi);
            p[0] = r * sintheta * cosphi; p[1] = r * sintheta * sinphi; p[2] = r * costheta;
        }
    };
    SKIRT_LOCAL double volume1D(int m) const;
    SKIRT_LOCAL double volume2D(int m) const;
    SKIRT_LOCAL void center1D(int m, double c[3]) const;
    SKIRT_LOCAL void center2D(int m, double c[3]) const;
    SKIRT_LOCAL int whichcell1D(double x, double y, double z) const;
    SKIRT_LOCAL int whichcell2D(double x, double y, double z) const;
    SKIRT_LOCAL Position1D positionInCell1D(int m) const;
    SKIRT_LOCAL Position2D positionInCell2D(int m) const;
};

enum class GridKind : int { Cartesian = 0, Octree = 1, Voronoi = 2, Cylinder2D = 3, Sphere1D = 4, Sphere2D = 5 };

struct DustGrid {
    GridKind kind = GridKind::Cartesian;
    CartesianGrid cart;
    OctreeGrid tree;
    VoronoiGrid vor;
    Cylinder2DGrid cyl;
    SphereGrid sph;
    int ncells = 0;
    // xmin ymin zmin xmax ymax zmax (Voronoi: the enclosing box; not defined for a cylindrical or spherical grid)
    void cellBox(int m, double b[6]) const;
    double cellVolume(int m) const;
    // DustGrid::centralPositionInCell: the box centre, the centroid of a Voronoi cell, or (R, phi = 0, z) at the
    // middle of a cylindrical cell's borders, or (r, theta, phi = 0) at the middle of a spherical cell's
    void cellCenter(int m, double c[3]) const;
    int whichcell(double x, double y, double z) const;
};

// ---------------------------------------------------------------- instruments
// Reference: DistantInstrument.cpp:27-50 (angles, kobs, kx, ky), SingleFrameInstrument.cpp:24-38
// (frame geometry) and :130-147 (pixelondetector), FullInstrument.cpp:107-174 (detect).
enum class InstrumentKind : int { Full = 0, Simple = 1, SED = 2, Frame = 3 };

// slots of the FullInstrument accumulation arrays (FullInstrument.cpp:58-86)
enum FullSlot : int { SlotTrav = 0, SlotStrDir = 1, SlotStrSca = 2, SlotDusDir = 3, SlotDusSca = 4, SlotLevel0 = 5 };

struct Instrument {
    std::string name;
    InstrumentKind kind = InstrumentKind::Full;
    double distance = 0, inclination = 0, azimuth = 0, positionAngle = 0;
    int Nx = 250, Ny = 250;
    double fovx = 0, fovy = 0, xc = 0, yc = 0;
    int scatteringLevels = 0;
    // FullInstrument::_polarization: the dust system's mixes polarise, so the instrument has Stokes Q, U, V arrays
    bool polarization = false;
    // derived
    double costheta = 1, sintheta = 0, cosphi = 1, sinphi = 0, cospa = 1, sinpa = 0;
    double kobs[3] = {0, 0, 1}, kx[3] = {0, 0, 0}, ky[3] = {0, 0, 0};
    double xpmin = 0, xpmax = 0, xpsiz = 0, ypmin = 0, ypmax = 0, ypsiz = 0;
    int nframe() const { return Nx * Ny; }
    bool hasFrames() const { return kind != InstrumentKind::SED; }
    bool hasSeds() const { return kind != InstrumentKind::Frame; }
    // number of accumulation slots (frames and SEDs share the slot index)
    // (the Stokes Q, U, V slots of a polarised simulation follow the scattering levels)
    int nslots() const { return kind == InstrumentKind::Full ? SlotLevel0 + scatteringLevels + (polarization ? 3 : 0) : 1; }
    int stokesSlot() const { return SlotLevel0 + scatteringLevels; }
    int pixel(double x, double y, double z) const;
};

// ---------------------------------------------------------------- simulation
struct Model {
    bool pan = false;
    std::string units_system = "ExtragalacticUnits";
    unsigned long seed = 4357;

    // MonteCarloSimulation properties (MonteCarloSimulation.cpp:31-35 defaults)
    double packages = 1e6;
    double minWeightReduction = 1e4;
    int minScattEvents = 0;
    double scattBias = 0.5;
    bool continuousScattering = false;

    WavelengthGrid wl;

    // stellar system (StellarSystem.cpp)
    std::vector<Geometry> starGeom;              // per component
    std::vector<std::vector<double>> starL;      // [comp][ell] luminosity (W)
    double starEmissionBias = 0.5;
    std::vector<double> starLtot;                // per ell, sum over comps
    std::vector<std::vector<double>> starX;      // per ell: normalized cumulative luminosity over comps

    // dust system
    bool hasDust = false;
    bool polarization = false;  // DustSystem::polarization(): every dust mix supports polarisation
    std::vector<DustComp> dust;
    // SPHDustDistribution: the particle set (dust then holds its one component, which shares it); null otherwise
    std::shared_ptr<const ParticleSet> particles;
    DustGrid grid;
    std::vector<double> rho;     // Ncells x Ncomp row-major (DustSystem::_rhovv)
    std::vector<double> volume;  // per cell
    bool storeAbsorption = false;   // DustSystem::storeabsorptionrates()
    bool dustEmission = false;      // PanDustSystem::dustemission()
    bool selfAbsorption = false;
    double dustEmissionBias = 0.5;  // PanDustSystem emissionBias
    double emissionBoost = 1;
    int cycles = 0;
    bool writeISRF = false, writeCellProperties = false, writeMeanIntensity = false, writeConvergence = false;
    bool writeCellsCrossed = false;  // DustSystem writeCellsCrossed: the ds_crossed path histogram
    int sampleCount = 100;

    std::vector<Instrument> instruments;

    int ncomp() const { return (int)dust.size(); }
    int ncells() const { return grid.ncells; }
    // kappa_ext * rho summed over components (the KappaRho functor, DustSystem.cpp:465-491)
    double kapparho(int m, int ell) const;
};

// The setup's density sampling on a device (skirt_mcrt_sample_density, supplied by the product library):
// for n boxes (6 doubles each) and 3 * nsample Mersenne-twister words per box, the sums of mode
// kDensComponents (ncomp per box) or kDensNode (6 per box). Throws on failure.
enum DensityMode : int { kDensComponents = 0, kDensNode = 1 };  // SKIRT_DENS_COMPONENTS, SKIRT_DENS_NODE
struct DensitySampler {
    virtual ~DensitySampler() = default;
    // (a particle component, dust[0].particles, samples the particle density: one component)
    virtual void sample(const std::vector<DustComp>& dust, const double* boxes, size_t n, const uint32_t* words,
                        int nsample, int mode, double* out) = 0;
    // particle dust: the mass in each of n boxes (SPHDustDistribution::massInBox), and the density at each of n
    // points; handedBack (may be null) receives the number of boxes the device left to the host's worker threads
    virtual void massInBox(const ParticleSet& ps, const double* boxes, size_t n, double* out, size_t* handedBack) = 0;
    virtual void pointDensity(const ParticleSet& ps, const double* points, size_t n, double* out) = 0;
    // the Voronoi tessellation's cells on the same device (null: on the host)
    virtual const VoronoiCellsFn* voronoiCells() const { return nullptr; }
};

// Builds the model from a .ski file; `rng` supplies the setup random numbers (octree subdivision
// sampling, cell density sampling) in the reference's order. `datadir` holds SunSED.bin etc. With a
// sampler (and a Mersenne-twister rng), the density sampling of the tree subdivision and of the cell
// densities runs on its device; the host still draws every random number and takes every decision.
// `inputdir` is where a relative file name of the model (an imported particle file) is looked up; empty: the .ski
// file's own folder.
Model loadSki(const std::string& path, UniformSource& rng, const std::string& datadir,
              DensitySampler* sampler = nullptr, const std::string& inputdir = std::string());

// directory holding the packaged resource tables (skirt_amd/data), located relative to this library
std::string defaultDataDir();

}  // namespace skirt
