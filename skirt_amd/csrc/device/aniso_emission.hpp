// Anisotropic emission: the six geometries of the reference that override AngularDistribution --
// NetzerAccretionDiskGeometry, StellarSurfaceGeometry, SpheBackgroundGeometry, CubBackgroundGeometry,
// SolarPatchGeometry and LaserGeometry (SKIRTcore/*.cpp of the same names) -- as GeometricStellarComp::launch uses
// them: generatePosition, generateDirection(position) and, for an emission peel-off
// (PhotonPackage::launchEmissionPeelOff, PhotonPackage.cpp:46), probabilityForDirection(position, direction). In the
// reference's f64 operations, order and draw order, with Random::cdf (NR::locate_clip + NR::interpolate_linlin) and
// Direction(theta, phi) (Direction.cpp:12-38). The same text compiles for gfx950 (engine.hip: the ANISO event
// kernels' Events::launchPosition, launchDirection and emission peel-off; sampleLaunchesKernel) and as plain C++
// (the host driver's skirt_sim_sample_launches, the CPU logic test), so it touches nothing of the engine.
//
// Each kind has at most one parameter, the first word of its row of SkirtSourceDesc::geom_param:
//   NETZER, LASER                      none (every packet leaves the origin)
//   STELLARSURFACE, SPHEBACKGROUND     the sphere's radius
//   CUBBACKGROUND                      the cube's half-size (extent)
//   SOLARPATCH                         the patch's radius
// The Netzer disk draws its polar angle from a 401-entry table (theta_i, X_i) without parameters
// (NetzerAccretionDiskGeometry::setupSelfBefore). anisoNetzerTable builds it, on the host only: the bisection lands
// in the interval the reference's lands in when the entries are the reference's to the bit, so they come from the
// host's libm cos and the device reads them (one copy in global memory, 6.4 KB, read-mostly).
//
// Trigonometry, as DESIGN.md section 7 states it: cos and sin of acos(c) are c and sqrt((1-c)(1+c)); sin and
// cos(2 pi X) are sincospi(2 X) on the device; asin(sqrt(u)) is the angle with sine sqrt(u) and cosine sqrt(1-u),
// pi - acos(sqrt(u)) the one with cosine -sqrt(u) and sine sqrt(1-u); the rotation by a position's (theta, phi) takes
// z/r, sqrt(1-(z/r)^2), x/R and y/R, and at a pole (R = 0), where the reference's atan2(0, 0) is 0, cos phi = 1 and
// sin phi = 0. Direction(theta, phi)'s 1e-8 pole cut-offs are kept where an angle is at hand (the Netzer disk's
// table angle); the other kinds' primed angles do not reach them: asin(sqrt(u)) <= 1e-8 needs u <= 1e-16, which of
// the 2^53 deviates only the smallest, 2^-54, meets (the cut-off would then move the direction by 7e-9), and
// pi - acos(sqrt(u)) >= pi - 1e-8 needs u = 1.
#pragma once

#include <math.h>

#include "geom_sample.hpp"

// the kinds, as SKIRT_GEOM_* of include/skirt_mcrt.h (engine.hip asserts the equality)
enum {
    ANISO_NETZER = 10, ANISO_STELLARSURFACE = 11, ANISO_SPHEBACKGROUND = 12, ANISO_CUBBACKGROUND = 13,
    ANISO_SOLARPATCH = 14, ANISO_LASER = 15
};
constexpr int anisoNetzerN = 401;                    // entries of the Netzer table
constexpr int anisoNetzerWords = 2 * anisoNetzerN;   // theta_0..theta_400, then X_0..X_400
constexpr double anisoEps = 1e-8;                    // the reference's tolerance for "on the surface" and the poles

SKIRT_GEOM_FN bool anisoIsKind(int kind) { return kind >= ANISO_NETZER && kind <= ANISO_LASER; }

// NetzerAccretionDiskGeometry::setupSelfBefore: the cumulative luminosity distribution on 401 polar angles (a host
// function)
inline void anisoNetzerTable(double* tab) {
    const int N = anisoNetzerN;
    double* thetav = tab;
    double* Xv = tab + N;
    thetav[0] = 0;
    Xv[0] = 0;
    for (int i = 1; i < N - 1; i++) {
        thetav[i] = geomPi * i / (N - 1);
        // (through a volatile: the call is the C library's at run time, never a constant the compiler folded)
        volatile double arg = thetav[i];
        const double ct = cos(arg);
        const double sign = ct > 0 ? 1. : -1;
        Xv[i] = (1. / 2.) - (2. / 7.) * ct * ct * ct - sign * (3. / 14.) * ct * ct;
    }
    thetav[N - 1] = geomPi;
    Xv[N - 1] = 1.0;
}

// Direction(theta', phi') of a primed angle given by its sine and cosine, phi' = 2 pi X
SKIRT_GEOM_FN void anisoPrimed(double st, double ct, double X, double& kpx, double& kpy, double& kpz) {
    double sp, cp;
    geomSinCosTwoPi(X, sp, cp);
    kpx = st * cp; kpy = st * sp; kpz = ct;
}

// the face of the background cube a position lies on, by the reference's cascade (-x, +x, -y, +y, -z, +z: an edge or
// a corner takes the first that matches); -1 off the cube
SKIRT_GEOM_FN int anisoCubeFace(double h, double x, double y, double z) {
    const double eps = anisoEps;
    const double ax = fabs(x), ay = fabs(y), az = fabs(z);
    if (fabs(x / h + 1.0) < eps && ay <= h && az <= h) return 0;
    else if (fabs(x / h - 1.0) < eps && ay <= h && az <= h) return 1;
    else if (fabs(y / h + 1.0) < eps && ax <= h && az <= h) return 2;
    else if (fabs(y / h - 1.0) < eps && ax <= h && az <= h) return 3;
    else if (fabs(z / h + 1.0) < eps && ax <= h && ay <= h) return 4;
    else if (fabs(z / h - 1.0) < eps && ax <= h && ay <= h) return 5;
    return -1;
}

// whether the reference's generateDirection and probabilityForDirection accept the position (they throw otherwise):
// the origin for the disk and the laser, |r/r0 - 1| <= 1e-8 for the spheres, a face of the cube; any for the patch
SKIRT_GEOM_FN bool anisoPositionValid(int kind, double r0, double x, double y, double z) {
    switch (kind) {
    case ANISO_NETZER:
    case ANISO_LASER: return !(sqrt(x * x + y * y + z * z) > 0.0);
    case ANISO_STELLARSURFACE:
    case ANISO_SPHEBACKGROUND: return !(fabs(sqrt(x * x + y * y + z * z) / r0 - 1.0) > anisoEps);
    case ANISO_CUBBACKGROUND: return anisoCubeFace(r0, x, y, z) >= 0;
    default: return true;
    }
}

// ---------------------------------------------------------------- positions
// Geometry::generatePosition of the six kinds
template <class R>
SKIRT_GEOM_FN void anisoPositionOf(int kind, double r0, R& rng, double& x, double& y, double& z) {
    switch (kind) {
    case ANISO_STELLARSURFACE:
    case ANISO_SPHEBACKGROUND: geomRadial(rng, r0, x, y, z); break;  // Position(r0, Random::direction())
    case ANISO_CUBBACKGROUND: {
        const double t1 = r0 * (2.0 * rng.uniform() - 1.0);
        const double t2 = r0 * (2.0 * rng.uniform() - 1.0);
        const double X = rng.uniform();
        if (X < 1.0 / 6.0) { x = -r0; y = t1; z = t2; }
        else if (X < 1.0 / 3.0) { x = r0; y = t1; z = t2; }
        else if (X < 0.5) { x = t1; y = -r0; z = t2; }
        else if (X < 2.0 / 3.0) { x = t1; y = r0; z = t2; }
        else if (X < 5.0 / 6.0) { x = t1; y = t2; z = -r0; }
        else { x = t1; y = t2; z = r0; }
        break;
    }
    case ANISO_SOLARPATCH: {  // Position(R, phi, 0, CYLINDRICAL)
        const double Rc = r0 * sqrt(rng.uniform());
        double sp, cp;
        geomSinCosTwoPi(rng.uniform(), sp, cp);
        x = Rc * cp; y = Rc * sp; z = 0.0;
        break;
    }
    default: x = 0.0; y = 0.0; z = 0.0; break;  // the Netzer disk and the laser: the origin, no draws
    }
}

// ---------------------------------------------------------------- directions
// the rotation of a direction in the frame of a sphere's normal at (x, y, z) to the regular frame
// (StellarSurfaceGeometry::generateDirection, SpheBackgroundGeometry::generateDirection)
SKIRT_GEOM_FN void anisoRotate(double x, double y, double z, double kpx, double kpy, double kpz, double& kx, double& ky,
                               double& kz) {
    // bfr.spherical(r, theta, phi): theta = acos(z/r), phi = atan2(y, x); r = 0: theta = phi = 0
    const double r = sqrt(x * x + y * y + z * z);
    double costheta = 1.0, sintheta = 0.0, cosphi = 1.0, sinphi = 0.0;
    if (r != 0) {
        costheta = z / r;
        sintheta = sqrt((1.0 - costheta) * (1.0 + costheta));
        const double Rc = sqrt(x * x + y * y);
        if (Rc != 0) { cosphi = x / Rc; sinphi = y / Rc; }
    }
    kx = costheta * cosphi * kpx - sinphi * kpy + sintheta * cosphi * kpz;
    ky = costheta * sinphi * kpx + cosphi * kpy + sintheta * sinphi * kpz;
    kz = -sintheta * kpx + costheta * kpz;
}

// AngularDistribution::generateDirection of the six kinds at a position that anisoPositionValid accepts (a position
// off the cube leaves along +z). netzer: the table of anisoNetzerTable, looked at by the Netzer disk only.
template <class R>
SKIRT_GEOM_FN void anisoDirectionOf(int kind, double r0, const double* netzer, R& rng, double x, double y, double z,
                                    double& kx, double& ky, double& kz) {
    switch (kind) {
    case ANISO_NETZER: {
        // Random::cdf(thetav, Xv)
        const double* thetav = netzer;
        const double* Xv = netzer + anisoNetzerN;
        const double X = rng.uniform();
        int i = 0;
        if (!(X < Xv[0])) {  // NR::locate_clip
            int jl = -1, ju = anisoNetzerN - 1;
            while (ju - jl > 1) {
                const int jm = (ju + jl) >> 1;
                if (X < Xv[jm]) ju = jm;
                else jl = jm;
            }
            i = jl;
        }
        const double theta = thetav[i] + ((X - Xv[i]) / (Xv[i + 1] - Xv[i])) * (thetav[i + 1] - thetav[i]);
        const double U = rng.uniform();
        // Direction(theta, phi)
        if (theta <= anisoEps) { kx = 0; ky = 0; kz = 1; }
        else if (theta >= geomPi - anisoEps) { kx = 0; ky = 0; kz = -1; }
        else anisoPrimed(sin(theta), cos(theta), U, kx, ky, kz);
        break;
    }
    case ANISO_STELLARSURFACE: {  // theta' = asin(sqrt(u))
        const double u = rng.uniform();
        double kpx, kpy, kpz;
        anisoPrimed(sqrt(u), sqrt(1.0 - u), rng.uniform(), kpx, kpy, kpz);
        anisoRotate(x, y, z, kpx, kpy, kpz, kx, ky, kz);
        break;
    }
    case ANISO_SPHEBACKGROUND: {  // theta' = pi - acos(sqrt(u))
        const double u = rng.uniform();
        double kpx, kpy, kpz;
        anisoPrimed(sqrt(1.0 - u), -sqrt(u), rng.uniform(), kpx, kpy, kpz);
        anisoRotate(x, y, z, kpx, kpy, kpz, kx, ky, kz);
        break;
    }
    case ANISO_CUBBACKGROUND: {  // theta' = pi - acos(sqrt(u)), then the face's frame
        const double u = rng.uniform();
        double kpx, kpy, kpz;
        anisoPrimed(sqrt(1.0 - u), -sqrt(u), rng.uniform(), kpx, kpy, kpz);
        switch (anisoCubeFace(r0, x, y, z)) {
        case 0: kx = -kpz; ky = -kpy; kz = -kpx; break;
        case 1: kx = kpz; ky = kpy; kz = -kpx; break;
        case 2: kx = kpy; ky = -kpz; kz = -kpx; break;
        case 3: kx = -kpy; ky = kpz; kz = -kpx; break;
        case 4: kx = -kpx; ky = kpy; kz = -kpz; break;
        case 5: kx = kpx; ky = kpy; kz = kpz; break;
        default: kx = 0; ky = 0; kz = 1; break;
        }
        break;
    }
    case ANISO_SOLARPATCH: {  // theta = asin(sqrt(u))
        const double u = rng.uniform();
        anisoPrimed(sqrt(u), sqrt(1.0 - u), rng.uniform(), kx, ky, kz);
        break;
    }
    default: kx = 0.0; ky = 0.0; kz = 1.0; break;  // the laser: Direction(0, 0, 1), no draws
    }
}

// ---------------------------------------------------------------- probabilities
// AngularDistribution::probabilityForDirection of the six kinds, normalized to 1 over the mean of the unit sphere,
// at a position that anisoPositionValid accepts (a position off the cube has none: -1)
SKIRT_GEOM_FN double anisoProbabilityOf(int kind, double r0, double x, double y, double z, double kx, double ky,
                                        double kz) {
    switch (kind) {
    case ANISO_NETZER: {
        const double ct = kz;  // cos(theta) of bfk.spherical(theta, phi)
        const double sign = ct > 0 ? 1. : -1;
        return (6. / 7.) * ct * (2. * ct + sign);
    }
    case ANISO_STELLARSURFACE: {
        const double costhetap = (x * kx + y * ky + z * kz) / r0;
        return costhetap > 0.0 ? 4.0 * costhetap : 0.0;
    }
    case ANISO_SPHEBACKGROUND: {
        const double costhetap = (x * kx + y * ky + z * kz) / r0;
        return costhetap > 0.0 ? 0.0 : -4.0 * costhetap;
    }
    case ANISO_CUBBACKGROUND: {
        double nx = 0.0, ny = 0.0, nz = 0.0;
        switch (anisoCubeFace(r0, x, y, z)) {
        case 0: nx = -1.0; break;
        case 1: nx = 1.0; break;
        case 2: ny = -1.0; break;
        case 3: ny = 1.0; break;
        case 4: nz = -1.0; break;
        case 5: nz = 1.0; break;
        default: return -1.0;
        }
        const double costhetap = nx * kx + ny * ky + nz * kz;
        return costhetap > 0.0 ? 0.0 : -4.0 * costhetap;
    }
    case ANISO_SOLARPATCH: return kz > 0.0 ? 4.0 * kz : 0.0;
    default:  // the laser: infinite where theta = acos(kz) is 0, that is at kz = 1 alone
        return kz == 1.0 ? INFINITY : 0.0;
    }
}
