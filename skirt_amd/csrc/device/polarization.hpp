// Polarised scattering: the Stokes vector of a photon packet and the polarised branches of the dust mix
// (SKIRTcore/StokesVector.cpp; DustMix.cpp:541-670 indexForTheta, angleBetweenScatteringPlanes,
// angleBetweenScatteringAndInstrumentReference, scatteringDirectionAndPolarization, scatteringPeelOffPolarization,
// phaseFunctionValue; :716-731 sampleTheta, samplePhi; Random::cdf, NR::locate_clip, NR::interpolate_linlin), in the
// reference's f64 operations and order. The same text compiles for gfx950 (engine.hip: Events<.., POL = true>, the
// scatterings probe) and as plain C++ (the host's side of the probe; tools/pol_cpu.py, the CPU logic test), so it
// touches nothing of the engine: the tables come in as one block of doubles (polTableWords), the random numbers
// from any object with a uniform().
//
// Three things are the engine's own:
//   the phi CDF   samplePhi fills a 361-entry array shared by all threads (DustMix.cpp:729). Here the bisection of
//                 NR::locate_clip evaluates (phi1[f] + c phis[f]) + s phic[f] at each entry it probes, from the one
//                 shared copy of the three tables: the same values, the same interval, no array per lane;
//   acos          where the dot product of two unit vectors rounds beyond +-1 the reference's acos gives NaN and
//                 its conversion to an index is undefined; the dot product is clamped to [-1, 1];
//   draws         the deviates come through a draws object (uniform()), as decideFill takes them: the event kernel
//                 draws from the packet's stream, the probe hands in given numbers.
#pragma once

#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define SKIRT_POL_FN __host__ __device__ inline
#else
#define SKIRT_POL_FN inline
#endif

constexpr double polPi = 3.14159265358979323846;  // M_PI
constexpr int polNphi = 361;                      // DustMix::_Nphi

// StokesVector: Q, U, V normalized by I, the normal of the scattering plane they refer to, the polarized flag
struct PolStokes {
    double Q, U, V, nx, ny, nz;
    int pol;
};

SKIRT_POL_FN void polSetUnpolarized(PolStokes& s) {
    s.pol = 0;
    s.Q = 0; s.U = 0; s.V = 0;
    s.nx = 0; s.ny = 0; s.nz = 0;
}

// The tables of all mixes as one block of doubles, nt = ntheta:
//   S11, S12, S33, S34 [ncomp][nlambda][nt] each | thetaX [ncomp][nlambda][nt] | pfnorm [ncomp][nlambda] |
//   phi1, phis, phic [polNphi] each (DustMix.cpp:125-139; the same for every mix)
SKIRT_POL_FN size_t polTableWords(int ncomp, int nlambda, int nt) {
    return (size_t)ncomp * nlambda * (5 * (size_t)nt + 1) + 3 * (size_t)polNphi;
}

// the phi tables of DustMix::setupSelfAfter (DustMix.cpp:131-139); phi itself is f * df wherever it is needed
inline void polPhiTables(double* phi, double* phi1, double* phis, double* phic) {
    const double df = 2 * polPi / (polNphi - 1);
    for (int f = 0; f < polNphi; f++) {
        const double p = f * df;
        if (phi) phi[f] = p;
        phi1[f] = p / (2 * polPi);
        phis[f] = sin(2 * p);
        phic[f] = 1 - cos(2 * p);
    }
}

// one mix at one wavelength
struct PolMix {
    int nt;
    const double *S11, *S12, *S33, *S34, *thetaX;
    double pfnorm;
    const double *phi1, *phis, *phic;
};

SKIRT_POL_FN PolMix polMixAt(const double* tab, int ncomp, int nlambda, int nt, int h, int ell) {
    const size_t plane = (size_t)ncomp * nlambda * nt, row = ((size_t)h * nlambda + ell) * nt;
    PolMix m;
    m.nt = nt;
    m.S11 = tab + row;
    m.S12 = tab + plane + row;
    m.S33 = tab + 2 * plane + row;
    m.S34 = tab + 3 * plane + row;
    m.thetaX = tab + 4 * plane + row;
    m.pfnorm = tab[5 * plane + (size_t)h * nlambda + ell];
    const double* phi = tab + 5 * plane + (size_t)ncomp * nlambda;
    m.phi1 = phi;
    m.phis = phi + polNphi;
    m.phic = phi + 2 * polNphi;
    return m;
}

// StokesVector::linearPolarizationDegree, polarizationAngle
SKIRT_POL_FN double polLinearDegree(const PolStokes& s) { return sqrt(s.Q * s.Q + s.U * s.U); }
SKIRT_POL_FN double polAngle(const PolStokes& s) {
    if (s.U == 0 && s.Q == 0) return 0;
    return 0.5 * atan2(s.U, s.Q);
}

// StokesVector::rotateStokes: the first scattering makes the normal by the Bianchi formula
SKIRT_POL_FN void polRotateStokes(PolStokes& s, double phi, double kx, double ky, double kz) {
    if (!s.pol) {
        if (fabs(kz) > 0.99999) {
            s.nx = 1; s.ny = 0; s.nz = 0;
        } else {
            const double nz = sqrt((1.0 - kz) * (1.0 + kz));
            const double nx = -kx * kz / nz;
            const double ny = -ky * kz / nz;
            s.nx = nx; s.ny = ny; s.nz = nz;
        }
        s.pol = 1;
    } else {
        const double cos2phi = cos(2.0 * phi);
        const double sin2phi = sin(2.0 * phi);
        const double Q = cos2phi * s.Q + sin2phi * s.U;
        const double U = -sin2phi * s.Q + cos2phi * s.U;
        s.Q = Q;
        s.U = U;
    }
    // Rodrigues' rotation: normal cos(phi) + (k x normal) sin(phi), then normalized
    const double c = cos(phi), sn = sin(phi);
    const double cx = ky * s.nz - kz * s.ny, cy = kz * s.nx - kx * s.nz, cz = kx * s.ny - ky * s.nx;
    const double nx = s.nx * c + cx * sn, ny = s.ny * c + cy * sn, nz = s.nz * c + cz * sn;
    const double norm = sqrt(nx * nx + ny * ny + nz * nz);
    s.nx = nx / norm; s.ny = ny / norm; s.nz = nz / norm;
}

// StokesVector::applyMueller with setPolarized's I != 0 test; returns I
SKIRT_POL_FN double polApplyMueller(PolStokes& s, double S11, double S12, double S33, double S34) {
    const double I = S11 * 1. + S12 * s.Q;
    const double Q = S12 * 1. + S11 * s.Q;
    const double U = S33 * s.U + S34 * s.V;
    const double V = -S34 * s.U + S33 * s.V;
    if (I != 0.0) {
        s.Q = Q / I; s.U = U / I; s.V = V / I;
        s.pol = 1;
    } else {
        polSetUnpolarized(s);
    }
    return I;
}

SKIRT_POL_FN int polIndexForTheta(double theta, int Ntheta) {
    const double dt = polPi / (Ntheta - 1);
    int t = static_cast<int>(theta / dt + 0.5);
    if (t < 0) t = 0;
    else if (t >= Ntheta) t = Ntheta - 1;
    return t;
}

// acos of the dot product of two unit vectors, clamped (the engine's own, see above)
SKIRT_POL_FN double polAcosDot(double ax, double ay, double az, double bx, double by, double bz) {
    double d = ax * bx + ay * by + az * bz;
    if (d > 1.0) d = 1.0;
    else if (d < -1.0) d = -1.0;
    return acos(d);
}

// angle between the previous and the current scattering plane; 0 where atan2 is not finite
SKIRT_POL_FN double polAngleBetweenScatteringPlanes(double npx, double npy, double npz, double kcx, double kcy,
                                                    double kcz, double knx, double kny, double knz) {
    double ncx = kcy * knz - kcz * kny, ncy = kcz * knx - kcx * knz, ncz = kcx * kny - kcy * knx;
    const double norm = sqrt(ncx * ncx + ncy * ncy + ncz * ncz);
    ncx /= norm; ncy /= norm; ncz /= norm;
    const double cosphi = npx * ncx + npy * ncy + npz * ncz;
    const double wx = npy * ncz - npz * ncy, wy = npz * ncx - npx * ncz, wz = npx * ncy - npy * ncx;
    const double sinphi = wx * kcx + wy * kcy + wz * kcz;
    const double phi = atan2(sinphi, cosphi);
    if (isfinite(phi)) return phi;
    return 0;
}

// angle between the reference axis of the peel-off scattering plane and the instrument frame's x axis
SKIRT_POL_FN double polAngleBetweenScatteringAndInstrumentReference(double nx, double ny, double nz, double knx,
                                                                    double kny, double knz, double kyx, double kyy,
                                                                    double kyz) {
    const double cosalpha = nx * kyx + ny * kyy + nz * kyz;
    const double wx = ny * kyz - nz * kyy, wy = nz * kyx - nx * kyz, wz = nx * kyy - ny * kyx;
    const double sinalpha = wx * knx + wy * kny + wz * knz;
    return atan2(sinalpha, cosalpha);
}

// NR::locate_clip's bisection over n table entries given as a function of the index
template <class F>
SKIRT_POL_FN int polLocateClip(int n, double x, F at) {
    if (x < at(0)) return 0;
    int jl = -1;
    int ju = n - 1;
    while (ju - jl > 1) {
        const int jm = (ju + jl) >> 1;
        if (x < at(jm)) ju = jm;
        else jl = jm;
    }
    return jl;
}

// DustMix::sampleTheta: Random::cdf(thetav, thetaXv) for the deviate X
SKIRT_POL_FN double polSampleTheta(const PolMix& m, double X) {
    const double* Xv = m.thetaX;
    const int i = polLocateClip(m.nt, X, [Xv](int j) { return Xv[j]; });
    const double dt = polPi / (m.nt - 1);
    const double x1 = i * dt, x2 = (i + 1) * dt;
    return x1 + ((X - Xv[i]) / (Xv[i + 1] - Xv[i])) * (x2 - x1);
}

// DustMix::samplePhi for the deviate X
SKIRT_POL_FN double polSamplePhi(const PolMix& m, double theta, double polDegree, double polAng, double X) {
    const int t = polIndexForTheta(theta, m.nt);
    const double PF = polDegree * m.S12[t] / m.S11[t] / (4 * polPi);
    const double c = cos(2 * polAng) * PF;
    const double s = sin(2 * polAng) * PF;
    const double *p1 = m.phi1, *ps = m.phis, *pc = m.phic;
    auto at = [p1, ps, pc, c, s](int f) { return (p1[f] + c * ps[f]) + s * pc[f]; };
    const int i = polLocateClip(polNphi, X, at);
    const double df = 2 * polPi / (polNphi - 1);
    const double x1 = i * df, x2 = (i + 1) * df;
    const double X1 = at(i), X2 = at(i + 1);
    return x1 + ((X - X1) / (X2 - X1)) * (x2 - x1);
}

// DustMix::scatteringDirectionAndPolarization, polarized: the packet's direction and Stokes vector after a
// scattering by mix m; two deviates, theta's first
template <class Draws>
SKIRT_POL_FN void polScatter(const PolMix& m, double& kx, double& ky, double& kz, PolStokes& s, Draws& draws) {
    const double theta = polSampleTheta(m, draws.uniform());
    const double phi = polSamplePhi(m, theta, polLinearDegree(s), polAngle(s), draws.uniform());
    polRotateStokes(s, phi, kx, ky, kz);
    const int t = polIndexForTheta(theta, m.nt);
    polApplyMueller(s, m.S11[t], m.S12[t], m.S33[t], m.S34[t]);
    // the direction rotated in the scattering plane: k cos(theta) + (normal x k) sin(theta), normalized
    const double ct = cos(theta), st = sin(theta);
    const double cx = s.ny * kz - s.nz * ky, cy = s.nz * kx - s.nx * kz, cz = s.nx * ky - s.ny * kx;
    const double dx = kx * ct + cx * st, dy = ky * ct + cy * st, dz = kz * ct + cz * st;
    const double norm = sqrt(dx * dx + dy * dy + dz * dz);
    kx = dx / norm; ky = dy / norm; kz = dz / norm;
}

// DustMix::phaseFunctionValue, polarized, of a packet with direction k and Stokes vector s towards knew
SKIRT_POL_FN double polPhaseFunctionValue(const PolMix& m, const PolStokes& s, double kx, double ky, double kz,
                                          double knx, double kny, double knz) {
    const double phi = polAngleBetweenScatteringPlanes(s.nx, s.ny, s.nz, kx, ky, kz, knx, kny, knz);
    const double theta = polAcosDot(kx, ky, kz, knx, kny, knz);
    const int t = polIndexForTheta(theta, m.nt);
    const double polDegree = polLinearDegree(s);
    const double polAng = polAngle(s);
    return m.pfnorm * (m.S11[t] + polDegree * m.S12[t] * cos(2. * (phi - polAng)));
}

// DustMix::scatteringPeelOffPolarization, polarized: the Stokes vector a peel-off towards knew carries, in the frame
// of the instrument whose y axis is (kyx, kyy, kyz)
SKIRT_POL_FN PolStokes polPeelOff(const PolMix& m, const PolStokes& s, double kx, double ky, double kz, double knx,
                                  double kny, double knz, double kyx, double kyy, double kyz) {
    PolStokes out = s;
    polRotateStokes(out, 0, kx, ky, kz);  // makes the normal at a first scattering
    const double phi = polAngleBetweenScatteringPlanes(out.nx, out.ny, out.nz, kx, ky, kz, knx, kny, knz);
    polRotateStokes(out, phi, kx, ky, kz);
    const double theta = polAcosDot(kx, ky, kz, knx, kny, knz);
    const int t = polIndexForTheta(theta, m.nt);
    polApplyMueller(out, m.S11[t], m.S12[t], m.S33[t], m.S34[t]);
    const double alpha = polAngleBetweenScatteringAndInstrumentReference(out.nx, out.ny, out.nz, knx, kny, knz, kyx,
                                                                         kyy, kyz);
    polRotateStokes(out, alpha, kx, ky, kz);
    return out;
}

// One component's share of MonteCarloSimulation::peeloffscattering's sums (MonteCarloSimulation.cpp:347-358): adds
// w = wv phaseFunctionValue times (1, Q, U, V) of the peel-off's Stokes vector to I, Q, U, V
SKIRT_POL_FN void polPeelAdd(const PolMix& m, double wv, const PolStokes& s, double kx, double ky, double kz,
                             double knx, double kny, double knz, double kyx, double kyy, double kyz, double& I,
                             double& Q, double& U, double& V) {
    const double w = wv * polPhaseFunctionValue(m, s, kx, ky, kz, knx, kny, knz);
    const PolStokes sv = polPeelOff(m, s, kx, ky, kz, knx, kny, knz, kyx, kyy, kyz);
    I += w * 1.;
    Q += w * sv.Q;
    U += w * sv.U;
    V += w * sv.V;
}

// PhotonPackage::setPolarized(I, Q, U, V) of the peel-off package: what the detection carries beside L I
SKIRT_POL_FN void polPeelNormalize(double I, double& Q, double& U, double& V) {
    if (I != 0.0) { Q = Q / I; U = U / I; V = V / I; }
    else { Q = 0; U = 0; V = 0; }
}

// The scatterings probe (skirt_mcrt_scatterings), one state: in[12] = {kx, ky, kz, Q, U, V, nx, ny, nz, polarized,
// ell, comp}, two deviates; out[14] = direction, Q, U, V, normal and polarized flag after one scattering by mix
// `comp`, then I and the normalized Q, U, V of the peel-off from the state BEFORE that scattering towards kobs (the
// one component at weight 1), as the event kernel orders them
struct PolGivenDraws {
    double u[2];
    int n;
    SKIRT_POL_FN double uniform() { return u[n++ & 1]; }
};
constexpr int polStateWords = 12, polResultWords = 14;
SKIRT_POL_FN void polProbeOne(const double* tab, int ncomp, int nlambda, int nt, const double* in, const double* dev,
                              const double* kobs, const double* kyv, double* out) {
    double kx = in[0], ky = in[1], kz = in[2];
    PolStokes s{in[3], in[4], in[5], in[6], in[7], in[8], in[9] != 0.0 ? 1 : 0};
    const int ell = (int)in[10], h = (int)in[11];
    const PolMix m = polMixAt(tab, ncomp, nlambda, nt, h, ell);
    double I = 0, Q = 0, U = 0, V = 0;
    polPeelAdd(m, 1.0, s, kx, ky, kz, kobs[0], kobs[1], kobs[2], kyv[0], kyv[1], kyv[2], I, Q, U, V);
    polPeelNormalize(I, Q, U, V);
    PolGivenDraws draws{{dev[0], dev[1]}, 0};
    polScatter(m, kx, ky, kz, s, draws);
    out[0] = kx; out[1] = ky; out[2] = kz;
    out[3] = s.Q; out[4] = s.U; out[5] = s.V;
    out[6] = s.nx; out[7] = s.ny; out[8] = s.nz;
    out[9] = s.pol;
    out[10] = I; out[11] = Q; out[12] = U; out[13] = V;
}
