// Geometries: the special functions they need (SpecialFunctions.cpp), the Geometry members (densities, surface
// densities, the Sersic tables) and the .ski parser of every geometry kind with its set-up checks. The random
// positions are model.hpp's templates.
#include <cfloat>
#include <cmath>
#include <limits>
#include <stdexcept>

#include "nr.hpp"
#include "ski_parse.hpp"

namespace skirt {

// SpecialFunctions::gln / gln2 / gexp (SpecialFunctions.cpp:754-791)
double gln(double p, double x) {
    const double q = 1.0 - p;
    if (q == 0.0) return std::log(x);
    else if (std::fabs(q) < 1e-3) {
        const double lnx = std::log(x);
        const double s = q * lnx;
        return lnx * (1.0 + 0.5 * s + 1.0 / 6.0 * s * s + 1.0 / 24.0 * s * s * s);
    } else
        return (std::pow(x, q) - 1.0) / q;
}
double gln2(double p, double x1, double x2) { return std::pow(x2, 1.0 - p) * gln(p, x1 / x2); }
double gexp(double p, double x) {
    const double q = 1.0 - p;
    if (q == 0.0) return std::exp(x);
    else if (std::fabs(q) < 1e-3) {
        const double x2 = x * x;
        return std::exp(x) * (1.0 - 0.5 * x2 * q + 1.0 / 24.0 * x * x2 * (8.0 + 3.0 * x) * q * q -
                              1.0 / 48.0 * x2 * x2 * (12.0 + 8.0 * x + x2) * q * q * q);
    } else
        return std::pow(1.0 + q * x, 1.0 / q);
}

// SpecialFunctions::lngamma / gamma (SpecialFunctions.cpp:16-40)
static double lngamma(double a) {
    static const double cof[6] = {76.18009172947146, -86.50532032941677, 24.01409824083091, -1.231739572450155,
                                  0.1208650973866179e-2, -0.5395239384953e-5};
    double y, xx, tmp, ser;
    y = xx = a;
    tmp = xx + 5.5;
    tmp -= (xx + 0.5) * std::log(tmp);
    ser = 1.000000000190015;
    for (int j = 0; j < 6; j++) ser += cof[j] / ++y;
    return -tmp + std::log(2.5066282746310005 * ser / xx);
}

double Geometry::density(double x, double y, double z) const {
    switch (kind) {
    case GeometryKind::Plummer: {
        double r = std::sqrt(x * x + y * y + z * z);  // Position::radius -> Vec::norm
        double s = r / c;
        return rho0 * std::pow(1.0 + s * s, -2.5);
    }
    case GeometryKind::Point:  // PointGeometry::density
        return (x * x + y * y + z * z) == 0 ? std::numeric_limits<double>::infinity() : 0.0;
    case GeometryKind::Sersic: {
        // SpheGeometry::density(Position) -> SersicGeometry::density(r) = rho0 S(r/reff)
        const double r = std::sqrt(x * x + y * y + z * z);
        const double s = r / reff;
        const int Ns = (int)sv.size();
        if (s <= sv[0]) return rho0 * Sv[0];
        if (s >= sv[Ns - 1]) return rho0 * Sv[Ns - 1];
        const int i = nr::locateClip(sv, s);
        return rho0 * nr::interpolateLogLog(s, sv[i], sv[i + 1], Sv[i], Sv[i + 1]);
    }
    case GeometryKind::ExpDisk: {
        // AxGeometry::density(Position) -> ExpDiskGeometry::density(R, z) (Position::cylradius)
        const double R = std::sqrt(x * x + y * y);
        const double absz = std::fabs(z);
        if (Rmax > 0.0 && R > Rmax) return 0.0;
        else if (zmax > 0.0 && absz > zmax) return 0.0;
        else if (R < Rmin) return 0.0;
        return rho0 * std::exp(-R / hR) * std::exp(-absz / hz);
    }
    case GeometryKind::Shell: {  // ShellGeometry::density(r)
        const double r = std::sqrt(x * x + y * y + z * z);
        if (r < rmin || r > rmax) return 0.0;
        return A * std::pow(r, -p);
    }
    case GeometryKind::Gamma: {  // GammaGeometry::density(r)
        const double r = std::sqrt(x * x + y * y + z * z);
        return rho0 * std::pow(r / b, -gamma) * std::pow(1.0 + r / b, gamma - 4.0);
    }
    case GeometryKind::Gaussian: {  // GaussianGeometry::density(R, z)
        const double R = std::sqrt(x * x + y * y);
        const double m2 = R * R + z * z / (q * q);
        const double sigma2 = sigma * sigma;
        return rho0 * std::exp(-0.5 * m2 / sigma2);
    }
    case GeometryKind::TTauriDisk: {  // TTauriDiskGeometry::density(R, z)
        const double R = std::sqrt(x * x + y * y);
        if (R < rmin || R > rmax) return 0.0;
        const double h = zd * std::pow(R / Rd, 1.125);
        return rho0 / (R / Rd) * std::exp(-M_PI / 4.0 * std::pow(z / h, 2));
    }
    case GeometryKind::Torus:
    case GeometryKind::ConicalShell: {  // TorusGeometry::density(R, z), ConicalShellGeometry::density(R, z)
        const double R = std::sqrt(x * x + y * y);
        const double r = std::sqrt(R * R + z * z);
        const double costheta = z / r;
        if (r >= rmax) return 0.0;
        if (rani) {
            const double rminani = rmin * std::sqrt(6. / 7. * std::fabs(costheta) * (2. * std::fabs(costheta) + 1));
            if (r <= rminani || r < rcut) return 0.0;
        } else {
            if (r <= rmin) return 0.0;
        }
        if (std::fabs(costheta) >= sinDelta) return 0.0;
        if (kind == GeometryKind::ConicalShell && std::fabs(costheta) <= sinDeltaIn) return 0.0;
        return A * std::pow(r, -p) * std::exp(-q * std::fabs(costheta));
    }
    case GeometryKind::Netzer:
    case GeometryKind::StellarSurface:
    case GeometryKind::SpheBackground:
    case GeometryKind::CubBackground:
    case GeometryKind::SolarPatch:
    case GeometryKind::Laser:
        // a point, a surface or a patch: infinite there and 0 elsewhere; never asked, these kinds are sources only
        throw std::runtime_error("an anisotropic source geometry has no density to sample");
    }
    return 0;
}

double Geometry::SigmaR() const {
    if (kind == GeometryKind::Gaussian) return 1.0 / (4.0 * M_PI * q * sigma * sigma);
    if (kind == GeometryKind::TTauriDisk) return rho0 * Rd * std::log(rmax / rmin);
    if (kind == GeometryKind::Torus) return A * gln2(p, rmax, rmin);
    if (kind == GeometryKind::ConicalShell) return A * std::exp(-q * cosDelta) * gln2(p, rmax, rmin);
    if (kind != GeometryKind::ExpDisk) throw std::runtime_error("Geometry is not axisymmetric");
    if (Rmax > 0.0) return rho0 * hR * (std::exp(-Rmin / hR) - std::exp(-Rmax / hR));
    return rho0 * hR * std::exp(-Rmin / hR);
}
double Geometry::SigmaZ() const {
    if (kind == GeometryKind::Gaussian) return 1.0 / (2.0 * M_PI * sigma * sigma);
    if (kind == GeometryKind::TTauriDisk || kind == GeometryKind::Torus || kind == GeometryKind::ConicalShell) return 0.0;
    if (kind != GeometryKind::ExpDisk) throw std::runtime_error("Geometry is not axisymmetric");
    if (Rmin > 0.0) return 0.0;
    if (zmax > 0.0) return -2.0 * rho0 * hz * std::expm1(-zmax / hz);
    return 2.0 * rho0 * hz;
}
double Geometry::Sigmar() const {
    if (kind == GeometryKind::Plummer) return 0.5 / (M_PI * c * c);
    if (kind == GeometryKind::Shell) return A * gln2(p, rmax, rmin);
    if (kind == GeometryKind::Gamma)
        return gamma < 1.0 ? 1.0 / (2.0 * M_PI * b * b * (1.0 - gamma) * (2.0 - gamma))
                           : std::numeric_limits<double>::infinity();
    if (kind == GeometryKind::Sersic)
        return 1.0 / (reff * reff) * std::pow(b, 2.0 * n) / (2.0 * M_PI * std::exp(lngamma(2.0 * n + 1.0)));
    throw std::runtime_error("Geometry is not spherically symmetric");
}

double Geometry::sersicInverseMass(double M) const {
    const int Ns = (int)sv.size();
    if (M <= Mv[0]) return sv[0];
    if (M >= Mv[Ns - 1]) return sv[Ns - 1];
    const int i = nr::locateClip(Mv, M);
    return nr::interpolateLogLog(M, Mv[i], Mv[i + 1], sv[i], sv[i + 1]);
}

// SersicFunction::SersicFunction(n) (SersicFunction.cpp): S(s) by the Abel-type integral on a
// 10001-point trapezoid, M(s) by a 33-point trapezoid per table interval, normalized
static void buildSersicTables(Geometry& g) {
    const double n = g.n;
    if (n < 0.5 || n > 10.0) throw std::runtime_error("The Sersic parameter should be between 0.5 and 10");
    const double b = 2.0 * n - 1.0 / 3.0 + 4.0 / 405.0 / n + 46.0 / 25515.0 / (n * n) + 131.0 / 1148175.0 / (n * n * n);
    g.b = b;  // SersicGeometry::setupSelfBefore computes the same expression
    const double I0 =std::pow(b, 2.0 * n) / (M_PI * std::exp(lngamma(2.0 * n + 1)));
    const int Ns = 101;
    g.sv.assign(Ns, 0.0);
    g.Sv.assign(Ns, 0.0);
    g.Mv.assign(Ns, 0.0);
    const double logsmin = -6.0, logsmax = 4.0;
    const double dlogs = (logsmax - logsmin) / (Ns - 1.0);
    for (int i = 0; i < Ns; i++) {
        const double logs = logsmin + i * dlogs;
        const double s = std::pow(10.0, logs);
        g.sv[i] = s;
        const double alpha = b * std::pow(s, 1.0 / n);
        double sum = 0.0;
        const int Nu = 10000;
        const double tmax = 100.0;
        const double umax = std::sqrt((tmax + 1.0) * (tmax - 1.0));
        const double du = umax / Nu;
        for (int j = 0; j <= Nu; j++) {
            double weight = 1.0;
            if (j == 0 || j == Nu) weight = 0.5;
            const double u = j * du;
            const double u2 = u * u;
            double w;
            if (u > 1e-3) w = (std::pow(1.0 + u2, 2.0 * n) - 1.0) / u2;
            else w = 2.0 * n + n * (2.0 * n - 1.0) * u2 + 2.0 / 3.0 * n * (2.0 * n - 1.0) * (n - 1.0) * u2 * u2;
            const double integrandum = 2.0 * std::exp(-alpha * (1.0 + u2)) / std::sqrt(w);
            sum += weight * integrandum;
        }
        g.Sv[i] = I0 * std::pow(b, n) * std::pow(alpha, 1.0 - n) / M_PI * du * sum;
    }
    auto S = [&](double s) {  // SersicFunction::operator()
        if (s <= g.sv[0]) return g.Sv[0];
        if (s >= g.sv[Ns - 1]) return g.Sv[Ns - 1];
        const int i = nr::locateClip(g.sv, s);
        return nr::interpolateLogLog(s, g.sv[i], g.sv[i + 1], g.Sv[i], g.Sv[i + 1]);
    };
    for (int i = 1; i < Ns; i++) {
        double sum = 0.0;
        for (int j = 0; j <= 32; j++) {
            double weight = 1.0;
            if (j == 0 || j == 32) weight = 0.5;
            const double ds = (g.sv[i] - g.sv[i - 1]) / 32.0;
            const double s = g.sv[i - 1] + j * ds;
            sum += weight * S(s) * s * s * ds;
        }
        const double dM = 4.0 * M_PI * sum;
        g.Mv[i] = g.Mv[i - 1] + dM;
    }
    for (int i = 0; i < Ns; i++) g.Mv[i] /= g.Mv[Ns - 1];
}

double lambertW1(double z) {
    const double eps = 1.0e-12;
    const double em1 = 0.3678794411714423215955237701614608;
    static const double c[12] = {-1.0, 2.331643981597124203363536062168, -1.812187885639363490240191647568,
                                 1.936631114492359755363277457668, -2.353551201881614516821543561516,
                                 3.066858901050631912893148922704, -4.175335600258177138854984177460,
                                 5.858023729874774148815053846119, -8.401032217523977370984161688514,
                                 12.250753501314460424, -18.100697012472442755, 27.029044799010561650};
    if (z < -em1 || z > 0.0 || std::isinf(z) || std::isnan(z)) throw std::runtime_error("LambertW1: bad argument");
    if (z == 0.0) return -DBL_MAX;
    const double q = z + em1;
    const double r = -std::sqrt(q);
    const double t8 = c[8] + r * (c[9] + r * (c[10] + r * c[11]));
    const double t5 = c[5] + r * (c[6] + r * (c[7] + r * t8));
    const double t1 = c[1] + r * (c[2] + r * (c[3] + r * (c[4] + r * t5)));
    const double w0 = c[0] + r * t1;
    if (q < 3.0e-3) return w0;
    double w;
    if (z < -1e-6) {
        w = w0;
    } else {
        const double l1 = std::log(-z);
        const double l2 = std::log(-l1);
        w = l1 - l2 + l2 / l1;
    }
    for (int i = 0; i < 10; i++) {  // Halley iteration
        const double e = std::exp(w);
        double t = w * e - z;
        const double p = w + 1.0;
        t /= e * p - 0.5 * (p + 1.0) * t / p;
        w -= t;
        if (std::fabs(t) < eps * (1.0 + std::fabs(w))) return w;
    }
    throw std::runtime_error("LambertW1: no convergence");
}

namespace {

// The rejection loops of TorusGeometry and ConicalShellGeometry::generatePosition have no bound in the reference;
// parameters that admit no position (an anisotropic inner radius with cutRadius >= maxRadius, say) make it spin.
// The engine's loops end at kGeomAttemptCap attempts; a geometry whose acceptance, estimated here over 20000
// attempts on a private stream (never the setup's generator, whose draw order is the reference's), is below 1e-3
// is refused at load, so that the cap is out of reach (e^-65) for every model that loads.
struct AcceptanceRng {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    double uniform() {  // splitmix64, 53 bits, inside (0,1)
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return ((double)(z >> 11) + 0.5) * (1.0 / 9007199254740992.0);
    }
};
struct CountingRng {
    AcceptanceRng r;
    long draws = 0;
    double uniform() { draws++; return r.uniform(); }
};
void checkAcceptance(const Geometry& geo, const std::string& name) {
    const long attempts = 20000;
    CountingRng rng;
    long accepted = 0;
    double x, y, z;
    // three deviates per attempt: positions until the attempts are spent (a position that meets the cap ends it)
    while (rng.draws < 3 * attempts && torusPosition(geo, rng, x, y, z)) accepted++;
    if ((double)accepted < 1e-3 * (double)(rng.draws / 3))
        throw std::runtime_error(name + ": fewer than 1 in 1000 candidate positions lie inside the geometry (" +
                                 std::to_string(accepted) + " of " + std::to_string(rng.draws / 3) +
                                 "); its parameters leave (almost) no volume");
}

void parseTorusGeometry(const Ctx& c, const XmlElement* g, Geometry& geo) {
    // TorusGeometry::setupSelfBefore (its RotateGeometryDecorator look-up finds none: _beta = 0) and
    // ConicalShellGeometry::setupSelfBefore
    const bool cone = g->name == "ConicalShellGeometry";
    const std::string of = cone ? " of the conical shell" : " of the torus";
    geo.kind = cone ? GeometryKind::ConicalShell : GeometryKind::Torus;
    geo.p = attr(c, g, "expon", "", 0);
    geo.q = attr(c, g, "index", "", 0);
    geo.Delta = attr(c, g, cone ? "outAngle" : "openAngle", "posangle", 0);
    geo.DeltaIn = cone ? attr(c, g, "inAngle", "posangle", 0) : 0.0;
    geo.rmin = attr(c, g, "minRadius", "length", 0);
    geo.rmax = attr(c, g, "maxRadius", "length", 0);
    geo.rani = attrBool(g, "anisoRadius", false);
    geo.rcut = attr(c, g, "cutRadius", "length", 0);
    if (geo.p < 0) throw std::runtime_error("The radial power law exponent p" + of + " should be positive");
    if (geo.q < 0) throw std::runtime_error("The polar index q" + of + " should be positive");
    if (cone) {
        if (geo.DeltaIn < 0) throw std::runtime_error("The inner angle of the conical shell should be positive");
        if (geo.Delta < 0) throw std::runtime_error("The outer angle of the conical shell should be positive");
        if (geo.Delta <= geo.DeltaIn)
            throw std::runtime_error("the outer angle of the shell should be larger than the inner angle");
    } else if (geo.Delta < 0) {
        throw std::runtime_error("The half opening angle of the torus should be positive");
    }
    if (geo.rmin <= 0) throw std::runtime_error("The minimum radius" + of + " should be positive");
    if (geo.rmax <= geo.rmin)
        throw std::runtime_error("The maximum radius" + of + " should be larger than the minimum radius");
    if (geo.rani && geo.rcut <= 0) throw std::runtime_error("The inner cutoff radius of the torus should be positive");
    geo.sinDelta = std::sin(geo.Delta);
    geo.smin = gln(geo.p - 2.0, geo.rmin);
    geo.sdiff = gln2(geo.p - 2.0, geo.rmax, geo.rmin);
    if (cone) {
        geo.sinDeltaIn = std::sin(geo.DeltaIn);
        geo.cosDelta = std::cos((geo.Delta + geo.DeltaIn) / 2.);
        if (geo.q > 1e-3)
            geo.A = geo.q * 0.25 / M_PI / geo.sdiff /
                    (std::exp(-geo.q * geo.sinDeltaIn) - std::exp(-geo.q * geo.sinDelta));
        else
            geo.A = 0.25 / M_PI / geo.sdiff / (geo.sinDelta - geo.sinDeltaIn);
    } else {
        geo.sinDeltaIn = -1.0;  // no inner angle: no |cos theta| lies at or below it
        if (geo.q > 1e-3) geo.A = geo.q * 0.25 / M_PI / geo.sdiff / (1.0 - std::exp(-geo.q * geo.sinDelta));
        else geo.A = 0.25 / M_PI / geo.sdiff / geo.sinDelta;
    }
    checkAcceptance(geo, g->name);
}

}  // namespace

Geometry parseGeometry(const Ctx& c, const XmlElement* g) {
    Geometry geo;
    if (g->name == "PlummerGeometry") {
        geo.kind = GeometryKind::Plummer;
        geo.c = attr(c, g, "scale", "length", 0);
        if (geo.c <= 0) throw std::runtime_error("the scale length c should be positive");
        geo.rho0 = 0.75 / std::pow(geo.c, 3) / M_PI;
    } else if (g->name == "PointGeometry") {
        geo.kind = GeometryKind::Point;
    } else if (g->name == "SersicGeometry") {
        // SersicGeometry::setupSelfBefore
        geo.kind = GeometryKind::Sersic;
        geo.n = attr(c, g, "index", "", 0);
        geo.reff = attr(c, g, "radius", "length", 0);
        if (geo.n <= 0.5 || geo.n > 10) throw std::runtime_error("the Sersic index n should be between 0.5 and 10");
        if (geo.reff <= 0) throw std::runtime_error("the effective radius should be positive");
        geo.rho0 = 1.0 / (geo.reff * geo.reff * geo.reff);
        buildSersicTables(geo);
    } else if (g->name == "ExpDiskGeometry") {
        // ExpDiskGeometry::setupSelfBefore (ExpDiskGeometry.cpp): checks and the normalization rho0
        geo.kind = GeometryKind::ExpDisk;
        geo.hR = attr(c, g, "radialScale", "length", 0);
        geo.hz = attr(c, g, "axialScale", "length", 0);
        geo.Rmax = attr(c, g, "radialTrunc", "length", 0);
        geo.zmax = attr(c, g, "axialTrunc", "length", 0);
        geo.Rmin = attr(c, g, "innerRadius", "length", 0);
        if (geo.hR <= 0) throw std::runtime_error("The radial scale length hR should be positive");
        if (geo.hz <= 0) throw std::runtime_error("The axial scale height hz should be positive");
        if (geo.Rmax < 0) throw std::runtime_error("The radial truncation length Rmax should be zero or positive");
        if (geo.zmax < 0) throw std::runtime_error("The axial truncation length zmax should be zero or positive");
        if (geo.Rmin < 0) throw std::runtime_error("The minimum radius Rmax should be zero or positive");
        else if (geo.Rmin > geo.Rmax && geo.Rmax > 0)
            throw std::runtime_error("The minimum radius Rmin should be larger than the truncation radius Rmax");
        const double intphi = 2.0 * M_PI;
        const double intz = (geo.zmax > 0) ? -2.0 * geo.hz * std::expm1(-geo.zmax / geo.hz) : 2.0 * geo.hz;
        const double tmin = (geo.Rmin > 0) ? std::exp(-geo.Rmin / geo.hR) * (1.0 + geo.Rmin / geo.hR) : 1.0;
        const double tmax = (geo.Rmax > 0) ? std::exp(-geo.Rmax / geo.hR) * (1.0 + geo.Rmax / geo.hR) : 0.0;
        const double intR = geo.hR * geo.hR * (tmin - tmax);
        geo.rho0 = 1.0 / (intR * intphi * intz);
    } else if (g->name == "ShellGeometry") {
        // ShellGeometry::setupSelfBefore
        geo.kind = GeometryKind::Shell;
        geo.rmin = attr(c, g, "minRadius", "length", 0);
        geo.rmax = attr(c, g, "maxRadius", "length", 0);
        geo.p = attr(c, g, "expon", "", 0);
        if (geo.rmin <= 0) throw std::runtime_error("the inner radius of the shell should be positive");
        if (geo.rmax <= geo.rmin)
            throw std::runtime_error("the outer radius of the shell should be larger than the inner radius");
        if (geo.p < 0) throw std::runtime_error("the power law exponent p should be positive");
        geo.smin = gln(geo.p - 2.0, geo.rmin);
        geo.sdiff = gln2(geo.p - 2.0, geo.rmax, geo.rmin);
        geo.A = 0.25 / M_PI / geo.sdiff;
    } else if (g->name == "GammaGeometry") {
        // GammaGeometry::setupSelfBefore
        geo.kind = GeometryKind::Gamma;
        geo.b = attr(c, g, "scale", "length", 0);
        geo.gamma = attr(c, g, "gamma", "", 1);
        if (geo.b <= 0) throw std::runtime_error("the scale length b should be positive");
        if (geo.gamma < 0 || geo.gamma >= 3.0)
            throw std::runtime_error("the central density slope gamma should be between 0 and 3");
        geo.rho0 = (3.0 - geo.gamma) / (4.0 * M_PI) / std::pow(geo.b, 3);
    } else if (g->name == "GaussianGeometry") {
        // GaussianGeometry::setupSelfBefore
        geo.kind = GeometryKind::Gaussian;
        geo.sigma = attr(c, g, "dispersion", "length", 0);
        geo.q = attr(c, g, "flattening", "", 0);
        if (geo.sigma <= 0) throw std::runtime_error("the dispersion parameter sigma should be positive");
        if (geo.q <= 0 || geo.q > 1.0) throw std::runtime_error("the flattening parameter q should be between 0 and 1");
        geo.rho0 = 1.0 / std::pow(std::sqrt(2.0 * M_PI) * geo.sigma, 3) / geo.q;
    } else if (g->name == "TTauriDiskGeometry") {
        // TTauriDiskGeometry::setupSelfBefore
        geo.kind = GeometryKind::TTauriDisk;
        geo.rmin = attr(c, g, "minRadius", "length", 0);
        geo.rmax = attr(c, g, "maxRadius", "length", 0);
        geo.Rd = attr(c, g, "radialScale", "length", 0);
        geo.zd = attr(c, g, "axialScale", "length", 0);
        if (geo.rmin <= 0) throw std::runtime_error("the inner radius of the disk should be positive");
        if (geo.rmax <= geo.rmin)
            throw std::runtime_error("the outer radius of the disk must be larger than the inner radius");
        if (geo.Rd <= 0) throw std::runtime_error("the radial scale length Rd should be positive");
        if (geo.zd <= 0) throw std::runtime_error("the axial scale height zd should be positive");
        geo.rho0 = 17.0 / 32.0 / M_PI / (geo.Rd * geo.Rd * geo.zd) /
                   (std::pow(geo.rmax / geo.Rd, 17.0 / 8.0) - std::pow(geo.rmin / geo.Rd, 17.0 / 8.0));
    } else if (g->name == "TorusGeometry" || g->name == "ConicalShellGeometry") {
        parseTorusGeometry(c, g, geo);
    } else if (g->name == "NetzerAccretionDiskGeometry") {
        geo.kind = GeometryKind::Netzer;  // (its 401-entry table has no parameters: anisoNetzerTable)
    } else if (g->name == "LaserGeometry") {
        geo.kind = GeometryKind::Laser;
    } else if (g->name == "StellarSurfaceGeometry") {
        geo.kind = GeometryKind::StellarSurface;
        geo.r0 = attr(c, g, "radius", "length", 0);
        if (geo.r0 <= 0) throw std::runtime_error("the stellar radius rstar should be positive");
    } else if (g->name == "SpheBackgroundGeometry") {
        geo.kind = GeometryKind::SpheBackground;
        geo.r0 = attr(c, g, "radius", "length", 0);
        if (geo.r0 <= 0) throw std::runtime_error("the background sphere radius rbg should be positive");
    } else if (g->name == "CubBackgroundGeometry") {
        geo.kind = GeometryKind::CubBackground;
        geo.r0 = attr(c, g, "extent", "length", 0);
        if (geo.r0 <= 0) throw std::runtime_error("the background cube extent h should be positive");
    } else if (g->name == "SolarPatchGeometry") {
        geo.kind = GeometryKind::SolarPatch;
        geo.r0 = attr(c, g, "radius", "length", 0);
        if (geo.r0 <= 0) throw std::runtime_error("the patch radius Rmax should be positive");
    } else {
        throw std::runtime_error("unsupported geometry " + g->name);
    }
    return geo;
}

}  // namespace skirt
