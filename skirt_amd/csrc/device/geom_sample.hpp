// Densities and random positions of the six closed-form geometries beyond Plummer, ExpDisk, Sersic and Point:
// ShellGeometry, GammaGeometry, GaussianGeometry, TTauriDiskGeometry, TorusGeometry and ConicalShellGeometry
// (SKIRTcore/*.cpp of the same names), with SpecialFunctions::gln / gln2 / gexp (SpecialFunctions.cpp:754-791) and
// Random::gauss (Random.cpp:140-150), in the reference's f64 operations, order and draw order. The same text
// compiles for gfx950 (engine.hip: Events::launchStellar; density_sample.hpp: geomDensity, samplePositionsKernel) and as plain C++
// (tools/geom_sample_cpu.py, the CPU logic test), so it touches nothing of the engine: parameters come in as the
// component's row of SkirtSourceDesc::geom_param (7 doubles) and, for the torus and the cone, the first words of
// its row of geom_table / dens_table; the random numbers come from any object with a uniform().
//
// Parameter rows (include/skirt_mcrt.h documents the same):
//   SHELL        gp = {rmin, rmax, p, smin, sdiff, A}
//   GAMMA        gp = {b, gamma, rho0}
//   GAUSSIAN     gp = {sigma, q, rho0}
//   TTAURIDISK   gp = {Rinn, Rout, Rd, zd, rho0}
//   TORUS        gp = {p, q, rmin, rmax, rani (0 or 1), rcut, A},  tab = {sinDelta, -1, smin, sdiff}
//   CONICALSHELL gp = {p, q, rmin, rmax, rani (0 or 1), rcut, A},  tab = {sinDeltaOut, sinDeltaIn, smin, sdiff}
// The torus is the cone without an inner angle: its tab[1] = -1 makes the cone's test |cos theta| <= sinDeltaIn
// never hold, so one routine serves both.
//
// The one choice of the engine's own: the rejection loops of the torus and the cone end after geomAttemptCap
// attempts (the reference's never do; parameters that admit no position make it spin). The routines then return
// false and leave the position at the origin.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define SKIRT_GEOM_FN __host__ __device__ inline
#else
#define SKIRT_GEOM_FN inline
#endif

constexpr int geomAttemptCap = 1 << 16;
constexpr double geomPi = 3.14159265358979323846;

// the kinds, as SKIRT_GEOM_* of include/skirt_mcrt.h (engine.hip asserts the equality)
enum {
    GEOMS_SHELL = 4, GEOMS_GAMMA = 5, GEOMS_GAUSSIAN = 6, GEOMS_TTAURIDISK = 7, GEOMS_TORUS = 8, GEOMS_CONICALSHELL = 9
};

// SpecialFunctions::gln: the generalized logarithm (x^(1-p) - 1) / (1-p)
SKIRT_GEOM_FN double geomGln(double p, double x) {
    const double q = 1.0 - p;
    if (q == 0.0) return log(x);
    else if (fabs(q) < 1e-3) {
        const double lnx = log(x);
        const double s = q * lnx;
        return lnx * (1.0 + 0.5 * s + 1.0 / 6.0 * s * s + 1.0 / 24.0 * s * s * s);
    } else
        return (pow(x, q) - 1.0) / q;
}

// SpecialFunctions::gln2: gln(p, x1) - gln(p, x2)
SKIRT_GEOM_FN double geomGln2(double p, double x1, double x2) { return pow(x2, 1.0 - p) * geomGln(p, x1 / x2); }

// SpecialFunctions::gexp: the inverse of gln
SKIRT_GEOM_FN double geomGexp(double p, double x) {
    const double q = 1.0 - p;
    if (q == 0.0) return exp(x);
    else if (fabs(q) < 1e-3) {
        const double x2 = x * x;
        return exp(x) * (1.0 - 0.5 * x2 * q + 1.0 / 24.0 * x * x2 * (8.0 + 3.0 * x) * q * q -
                         1.0 / 48.0 * x2 * x2 * (12.0 + 8.0 * x + x2) * q * q * q);
    } else
        return pow(1.0 + q * x, 1.0 / q);
}

// Random::gauss: the polar Box-Muller method, two deviates per attempt, the second variate dropped
template <class R>
SKIRT_GEOM_FN double geomGauss(R& rng) {
    double rsq, v1, v2;
    do {
        v1 = 2.0 * rng.uniform() - 1.0;
        v2 = 2.0 * rng.uniform() - 1.0;
        rsq = v1 * v1 + v2 * v2;
    } while (rsq >= 1.0 || rsq == 0.0);
    return v2 * sqrt(-2.0 * log(rsq) / rsq);
}

// sin and cos of phi = 2 pi X. The device takes sincospi(2 X): the same values to rounding without the
// large-argument reduction of sin and cos, whose registers the event kernel cannot spare.
SKIRT_GEOM_FN void geomSinCosTwoPi(double X, double& s, double& c) {
#if defined(__HIP_DEVICE_COMPILE__)
    sincospi(2.0 * X, &s, &c);
#else
    const double phi = 2.0 * geomPi * X;
    s = sin(phi);
    c = cos(phi);
#endif
}

// SpheGeometry::generatePosition after the radius: Position(r, Random::direction()), the direction as
// Direction(theta, phi) with theta = acos(2u-1), phi = 2 pi u' (Random.cpp:179-184, Direction.cpp), evaluated as the
// engine's other isotropic directions are: cos(theta) = 2u-1 and sin(theta) = sqrt((1-cos)(1+cos)), the same values
// to rounding without acos. The reference's 1e-8 pole cut-offs are never reached by a deviate in (0,1).
template <class R>
SKIRT_GEOM_FN void geomRadial(R& rng, double r, double& x, double& y, double& z) {
    const double ct = 2.0 * rng.uniform() - 1.0;
    const double st = sqrt((1.0 - ct) * (1.0 + ct));
    double sp, cp;
    geomSinCosTwoPi(rng.uniform(), sp, cp);
    const double kx = st * cp, ky = st * sp, kz = ct;
    x = r * kx; y = r * ky; z = r * kz;
}

// ---------------------------------------------------------------- densities
// ShellGeometry::density(r)
SKIRT_GEOM_FN double geomShellDensity(const double* gp, double r) {
    if (r < gp[0] || r > gp[1]) return 0.0;
    return gp[5] * pow(r, -gp[2]);
}
// GammaGeometry::density(r)
SKIRT_GEOM_FN double geomGammaDensity(const double* gp, double r) {
    const double b = gp[0], gamma = gp[1];
    return gp[2] * pow(r / b, -gamma) * pow(1.0 + r / b, gamma - 4.0);
}
// GaussianGeometry::density(R, z)
SKIRT_GEOM_FN double geomGaussianDensity(const double* gp, double R, double z) {
    const double sigma = gp[0], q = gp[1];
    const double m2 = R * R + z * z / (q * q);
    const double sigma2 = sigma * sigma;
    return gp[2] * exp(-0.5 * m2 / sigma2);
}
// TTauriDiskGeometry::density(R, z)
SKIRT_GEOM_FN double geomTTauriDensity(const double* gp, double R, double z) {
    const double Rinn = gp[0], Rout = gp[1], Rd = gp[2], zd = gp[3];
    if (R < Rinn || R > Rout) return 0.0;
    const double h = zd * pow(R / Rd, 1.125);
    return gp[4] / (R / Rd) * exp(-geomPi / 4.0 * pow(z / h, 2));
}
// TorusGeometry::density(R, z) and ConicalShellGeometry::density(R, z). The parameters are read through volatile
// pointers, here and in geomConePosition: each is loaded where it is used instead of being kept in registers over
// the rejection loop, which is what keeps the event kernel at its three waves per SIMD.
SKIRT_GEOM_FN double geomConeDensity(const volatile double* gp, const volatile double* tab, double R, double z) {
    const double p = gp[0], q = gp[1], rmin = gp[2], rmax = gp[3], rcut = gp[5];
    const double r = sqrt(R * R + z * z);
    const double costheta = z / r;
    if (r >= rmax) return 0.0;
    if (gp[4] != 0.0) {
        const double rminani = rmin * sqrt(6. / 7. * fabs(costheta) * (2. * fabs(costheta) + 1));
        if (r <= rminani || r < rcut) return 0.0;
    } else {
        if (r <= rmin) return 0.0;
    }
    if (fabs(costheta) >= tab[0]) return 0.0;
    if (fabs(costheta) <= tab[1]) return 0.0;
    return gp[6] * pow(r, -p) * exp(-q * fabs(costheta));
}

// Geometry::density(Position) of the six kinds: SpheGeometry takes Position::radius, AxGeometry cylradius and height
SKIRT_GEOM_FN double geomDensityOf(int kind, const double* gp, const double* tab, double x, double y, double z) {
    switch (kind) {
    case GEOMS_SHELL: return geomShellDensity(gp, sqrt(x * x + y * y + z * z));
    case GEOMS_GAMMA: return geomGammaDensity(gp, sqrt(x * x + y * y + z * z));
    case GEOMS_GAUSSIAN: return geomGaussianDensity(gp, sqrt(x * x + y * y), z);
    case GEOMS_TTAURIDISK: return geomTTauriDensity(gp, sqrt(x * x + y * y), z);
    default: return geomConeDensity(gp, tab, sqrt(x * x + y * y), z);
    }
}

// ---------------------------------------------------------------- positions
// ShellGeometry::randomradius, then SpheGeometry::generatePosition
template <class R>
SKIRT_GEOM_FN void geomShellPosition(const double* gp, R& rng, double& x, double& y, double& z) {
    const double X = rng.uniform();
    const double s = gp[3] + X * gp[4];
    geomRadial(rng, geomGexp(gp[2] - 2.0, s), x, y, z);
}
// GammaGeometry::randomradius, then SpheGeometry::generatePosition
template <class R>
SKIRT_GEOM_FN void geomGammaPosition(const double* gp, R& rng, double& x, double& y, double& z) {
    const double X = rng.uniform();
    const double t = pow(X, 1.0 / (3.0 - gp[1]));
    geomRadial(rng, gp[0] * t / (1.0 - t), x, y, z);
}
// GaussianGeometry::randomR, phi, randomz as SepAxGeometry::generatePosition orders them; Position(CYLINDRICAL)
template <class R>
SKIRT_GEOM_FN void geomGaussianPosition(const double* gp, R& rng, double& x, double& y, double& z) {
    const double sigma = gp[0], q = gp[1];
    const double X = rng.uniform();
    const double Rc = sigma * sqrt(-2.0 * log(X));
    double sp, cp;
    geomSinCosTwoPi(rng.uniform(), sp, cp);
    z = (q * sigma) * geomGauss(rng);
    x = Rc * cp;
    y = Rc * sp;
}
// TTauriDiskGeometry::generatePosition: phi first, then R, then z
template <class R>
SKIRT_GEOM_FN void geomTTauriPosition(const double* gp, R& rng, double& x, double& y, double& z) {
    const double Rinn = gp[0], Rout = gp[1], Rd = gp[2], zd = gp[3];
    double sp, cp;
    geomSinCosTwoPi(rng.uniform(), sp, cp);
    const double tinn = pow(Rinn, 2.125);
    const double tout = pow(Rout, 2.125);
    const double Rc = pow(tinn + rng.uniform() * (tout - tinn), 1.0 / 2.125);
    const double h = zd * pow(Rc / Rd, 1.125);
    const double sigma = sqrt(2.0 / geomPi) * h;
    z = geomGauss(rng) * sigma;
    x = Rc * cp;
    y = Rc * sp;
}
// TorusGeometry::generatePosition and ConicalShellGeometry::generatePosition: r by the power law, cos theta by the
// exponential (or uniform, q < 1e-3) law within the outer angle, phi; Position(r, theta, phi, SPHERICAL) and then
// the density test on its cylradius() and height(). False after geomAttemptCap rejected attempts.
template <class R>
SKIRT_GEOM_FN bool geomConePosition(const double* gp_, const double* tab_, R& rng, double& x, double& y, double& z) {
    const volatile double* gp = gp_;
    const volatile double* tab = tab_;
    for (int attempt = 0; attempt < geomAttemptCap; attempt++) {
        const double p = gp[0], q = gp[1];
        const double sinDelta = tab[0], smin = tab[2], sdiff = tab[3];
        double X = rng.uniform();
        const double s = smin + X * sdiff;
        const double r = geomGexp(p - 2.0, s);
        X = rng.uniform();
        double costheta = 0.0;
        if (q < 1e-3) costheta = (1.0 - 2.0 * X) * sinDelta;
        else {
            const double B = 1.0 - exp(-q * sinDelta);
            costheta = (X < 0.5) ? -log(1.0 - B * (1.0 - 2.0 * X)) / q : log(1.0 - B * (2.0 * X - 1.0)) / q;
        }
        // theta = acos(costheta), then Position's cos(theta) and sin(theta): costheta itself and
        // sqrt((1-cos)(1+cos)), the same values to rounding (|costheta| < sinDelta <= 1)
        const double ct = costheta, st = sqrt((1.0 - costheta) * (1.0 + costheta));
        X = rng.uniform();
        double sp, cp;
        geomSinCosTwoPi(X, sp, cp);
        const double px = r * st * cp, py = r * st * sp, pz = r * ct;
        if (geomConeDensity(gp, tab, sqrt(px * px + py * py), pz) != 0.0) {
            x = px; y = py; z = pz;
            return true;
        }
    }
    x = 0.0; y = 0.0; z = 0.0;
    return false;
}

// Geometry::generatePosition of the six kinds
template <class R>
SKIRT_GEOM_FN bool geomPositionOf(int kind, const double* gp, const double* tab, R& rng, double& x, double& y,
                                  double& z) {
    switch (kind) {
    case GEOMS_SHELL: geomShellPosition(gp, rng, x, y, z); return true;
    case GEOMS_GAMMA: geomGammaPosition(gp, rng, x, y, z); return true;
    case GEOMS_GAUSSIAN: geomGaussianPosition(gp, rng, x, y, z); return true;
    case GEOMS_TTAURIDISK: geomTTauriPosition(gp, rng, x, y, z); return true;
    default: return geomConePosition(gp, tab, rng, x, y, z);
    }
}
