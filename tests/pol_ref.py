"""Plain-Python restatement of the reference's polarised scattering, line by line from SKIRTcore/StokesVector.cpp
(setPolarized, rotateStokes, applyMueller, linearPolarizationDegree, polarizationAngle), DustMix.cpp:96-140 (the
theta and phi tables of setupSelfAfter), :541-670 (indexForTheta, angleBetweenScatteringPlanes,
angleBetweenScatteringAndInstrumentReference, scatteringDirectionAndPolarization, scatteringPeelOffPolarization,
phaseFunctionValue), :716-731 (sampleTheta, samplePhi, the whole 361-entry phi CDF filled as there), Random::cdf,
NR::cdf / locate_clip / interpolate_linlin, ElectronDustMix.cpp and MonteCarloSimulation.cpp:347-360, with the deviates
passed in. Python floats are IEEE doubles and `math` calls the C library, so on one machine these are the host
library's values bit for bit. One departure, the engine's own: the dot product under acos is
clamped to [-1, 1], where the reference's acos would give NaN.

Not a test module: tests/test_pol_logic.py, test_pol_host.py and test_gpu_pol.py import it."""
import math

import numpy as np

NTHETA = 181
NPHI = 361
SIGMA_THOMSON = 6.652458734e-29  # Units::sigmaThomson()
MASS_ELECTRON = 9.10938215e-31   # Units::masselectron()
STATE_WORDS, RESULT_WORDS = 12, 14


def _div(a, b):
    """a / b as IEEE does it (Python raises on a zero divisor)"""
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


# ---------------------------------------------------------------- tables
def phi_tables():
    df = 2 * math.pi / (NPHI - 1)
    phi, phi1, phis, phic = [], [], [], []
    for f in range(NPHI):
        p = f * df
        phi.append(p)
        phi1.append(p / (2 * math.pi))
        phis.append(math.sin(2 * p))
        phic.append(1 - math.cos(2 * p))
    return phi, phi1, phis, phic


def derive(S11, ntheta=NTHETA):
    """(thetaX[ntheta], pfnorm) of one wavelength's S11 row (DustMix.cpp:98-123)"""
    dt = math.pi / (ntheta - 1)
    thetav = [t * dt for t in range(ntheta)]
    P = [0.0]
    for t in range(ntheta - 1):
        P.append(P[t] + S11[t + 1] * math.sin(thetav[t + 1]) * dt)
    last = P[ntheta - 1]
    P = [v / last for v in P]
    total = 0.
    for t in range(ntheta):
        total += S11[t] * math.sin(thetav[t]) * dt
    return P, 2.0 / total


def mix_from_rows(S11, S12, S33, S34, nlambda):
    """a mix whose Mueller rows are the same at every wavelength, as a dict of [nlambda][ntheta] lists"""
    X, pf = derive(S11, len(S11))
    return {"S11": [list(S11)] * nlambda, "S12": [list(S12)] * nlambda, "S33": [list(S33)] * nlambda,
            "S34": [list(S34)] * nlambda, "thetaX": [list(X)] * nlambda, "pfnorm": [pf] * nlambda,
            "ntheta": len(S11)}


def electron_mix(nlambda):
    """ElectronDustMix::setupSelfBefore"""
    dt = math.pi / (NTHETA - 1)
    S11, S12, S33 = [], [], []
    for t in range(NTHETA):
        theta = t * dt
        costheta = math.cos(theta)
        S11.append(0.5 * (costheta * costheta + 1.))
        S12.append(0.5 * (costheta * costheta - 1.))
        S33.append(costheta)
    return mix_from_rows(S11, S12, S33, [0.0] * NTHETA, nlambda)


def madeup_mix(nlambda):
    """a mix no file describes, with S34 != 0 (so that V takes part) and a forward-peaked S11"""
    dt = math.pi / (NTHETA - 1)
    S11, S12, S33, S34 = [], [], [], []
    for t in range(NTHETA):
        theta = t * dt
        c = math.cos(theta)
        a = 1.0 + 0.6 * c + 0.3 * c * c
        S11.append(a)
        S12.append(-0.4 * a * math.sin(theta) ** 2)
        S33.append(0.8 * a * c)
        S34.append(0.3 * a * math.sin(theta) ** 2)
    return mix_from_rows(S11, S12, S33, S34, nlambda)


def pack(mixes):
    """the mixes' tables as the one block of doubles of polarization.hpp (polTableWords)"""
    _, phi1, phis, phic = phi_tables()
    out = []
    for key in ("S11", "S12", "S33", "S34", "thetaX"):
        for m in mixes:
            for row in m[key]:
                out.extend(row)
    for m in mixes:
        out.extend(m["pfnorm"])
    out.extend(phi1)
    out.extend(phis)
    out.extend(phic)
    return np.array(out, dtype=np.float64)


# ---------------------------------------------------------------- StokesVector
class Stokes:
    def __init__(self, Q=0.0, U=0.0, V=0.0, n=(0.0, 0.0, 0.0), pol=False):
        self.Q, self.U, self.V, self.n, self.pol = Q, U, V, tuple(n), bool(pol)

    def copy(self):
        return Stokes(self.Q, self.U, self.V, self.n, self.pol)

    def set_unpolarized(self):
        self.pol = False
        self.Q = self.U = self.V = 0.0
        self.n = (0.0, 0.0, 0.0)

    def set_polarized(self, I, Q, U, V, n):
        if I != 0.0:
            self.Q, self.U, self.V = Q / I, U / I, V / I
            self.n = n
            self.pol = True
        else:
            self.set_unpolarized()

    def linear_degree(self):
        return math.sqrt(self.Q * self.Q + self.U * self.U)

    def angle(self):
        if self.U == 0 and self.Q == 0:
            return 0
        return 0.5 * math.atan2(self.U, self.Q)

    def rotate(self, phi, k):
        kx, ky, kz = k
        if not self.pol:
            if abs(kz) > 0.99999:
                self.n = (1.0, 0.0, 0.0)
            else:
                nz = math.sqrt((1.0 - kz) * (1.0 + kz))
                nx = -kx * kz / nz
                ny = -ky * kz / nz
                self.n = (nx, ny, nz)
            self.pol = True
        else:
            cos2phi = math.cos(2.0 * phi)
            sin2phi = math.sin(2.0 * phi)
            Q = cos2phi * self.Q + sin2phi * self.U
            U = -sin2phi * self.Q + cos2phi * self.U
            self.Q, self.U = Q, U
        c, s = math.cos(phi), math.sin(phi)
        cr = cross(k, self.n)
        v = tuple(self.n[i] * c + cr[i] * s for i in range(3))
        norm = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        self.n = tuple(_div(x, norm) for x in v)

    def apply_mueller(self, S11, S12, S33, S34):
        I = S11 * 1. + S12 * self.Q
        Q = S12 * 1. + S11 * self.Q
        U = S33 * self.U + S34 * self.V
        V = -S34 * self.U + S33 * self.V
        self.set_polarized(I, Q, U, V, self.n)


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


# ---------------------------------------------------------------- DustMix
# theta / dt + 0.5 of every index conversion since the last reset: the tests count those within 1e-9 of an integer,
# where a last-bit difference in theta would pick another table row
INDEX_ARGS = []


def index_for_theta(theta, ntheta):
    dt = math.pi / (ntheta - 1)
    x = theta / dt + 0.5
    INDEX_ARGS.append(x)
    t = int(x)
    if t < 0:
        t = 0
    elif t >= ntheta:
        t = ntheta - 1
    return t


def near_integer_count(tol=1e-9):
    return sum(1 for x in INDEX_ARGS if abs(x - round(x)) < tol)


def angle_between_scattering_planes(np_, kc, kn):
    nc = cross(kc, kn)
    norm = math.sqrt(nc[0] * nc[0] + nc[1] * nc[1] + nc[2] * nc[2])
    nc = tuple(_div(x, norm) for x in nc)
    cosphi = dot(np_, nc)
    sinphi = dot(cross(np_, nc), kc)
    phi = math.atan2(sinphi, cosphi)
    if math.isfinite(phi):
        return phi
    return 0


def angle_between_scattering_and_instrument_reference(n, knew, ky):
    cosalpha = dot(n, ky)
    sinalpha = dot(cross(n, ky), knew)
    return math.atan2(sinalpha, cosalpha)


def acos_dot(a, b):
    return math.acos(max(-1.0, min(1.0, dot(a, b))))


def locate_clip(xv, x):
    n = len(xv)
    if x < xv[0]:
        return 0
    jl, ju = -1, n - 1
    while ju - jl > 1:
        jm = (ju + jl) >> 1
        if x < xv[jm]:
            ju = jm
        else:
            jl = jm
    return jl


def random_cdf(xv, Xv, X):
    i = locate_clip(Xv, X)
    return xv[i] + ((X - Xv[i]) / (Xv[i + 1] - Xv[i])) * (xv[i + 1] - xv[i])


_PHI = phi_tables()


def sample_theta(mix, ell, X):
    nt = mix["ntheta"]
    dt = math.pi / (nt - 1)
    return random_cdf([t * dt for t in range(nt)], mix["thetaX"][ell], X)


def sample_phi(mix, ell, theta, pol_degree, pol_angle, X):
    phi, phi1, phis, phic = _PHI
    t = index_for_theta(theta, mix["ntheta"])
    PF = pol_degree * mix["S12"][ell][t] / mix["S11"][ell][t] / (4 * math.pi)
    c = math.cos(2 * pol_angle) * PF
    s = math.sin(2 * pol_angle) * PF
    phiX = [(phi1[f] + c * phis[f]) + s * phic[f] for f in range(NPHI)]
    return random_cdf(phi, phiX, X)


def scatter(mix, ell, k, sv, u_theta, u_phi):
    """scatteringDirectionAndPolarization: (new direction, new Stokes)"""
    theta = sample_theta(mix, ell, u_theta)
    phi = sample_phi(mix, ell, theta, sv.linear_degree(), sv.angle(), u_phi)
    out = sv.copy()
    out.rotate(phi, k)
    t = index_for_theta(theta, mix["ntheta"])
    out.apply_mueller(mix["S11"][ell][t], mix["S12"][ell][t], mix["S33"][ell][t], mix["S34"][ell][t])
    c, s = math.cos(theta), math.sin(theta)
    cr = cross(out.n, k)
    v = tuple(k[i] * c + cr[i] * s for i in range(3))
    norm = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return tuple(_div(x, norm) for x in v), out


def phase_function_value(mix, ell, k, sv, knew):
    phi = angle_between_scattering_planes(sv.n, k, knew)
    theta = acos_dot(k, knew)
    t = index_for_theta(theta, mix["ntheta"])
    return mix["pfnorm"][ell] * (mix["S11"][ell][t] + sv.linear_degree() * mix["S12"][ell][t] *
                                 math.cos(2. * (phi - sv.angle())))


def peel_off(mix, ell, k, sv, knew, ky):
    out = sv.copy()
    out.rotate(0, k)
    phi = angle_between_scattering_planes(out.n, k, knew)
    out.rotate(phi, k)
    theta = acos_dot(k, knew)
    t = index_for_theta(theta, mix["ntheta"])
    out.apply_mueller(mix["S11"][ell][t], mix["S12"][ell][t], mix["S33"][ell][t], mix["S34"][ell][t])
    alpha = angle_between_scattering_and_instrument_reference(out.n, knew, ky)
    out.rotate(alpha, k)
    return out


def probe(mixes, states, deviates, kobs, ky):
    """what the scatterings probe returns: per state the 14 words of polarization.hpp's polProbeOne"""
    kobs, ky = tuple(float(x) for x in kobs), tuple(float(x) for x in ky)
    res = np.zeros((len(states), RESULT_WORDS))
    for i, (st, dv) in enumerate(zip(states, deviates)):
        st = [float(x) for x in st]
        k = tuple(st[0:3])
        sv = Stokes(st[3], st[4], st[5], st[6:9], st[9] != 0.0)
        ell, mix = int(st[10]), mixes[int(st[11])]
        # MonteCarloSimulation::peeloffscattering with one component at weight 1, on the state before the scattering
        w = 1.0 * phase_function_value(mix, ell, k, sv, kobs)
        p = peel_off(mix, ell, k, sv, kobs, ky)
        I, Q, U, V = 0 + w * 1., 0 + w * p.Q, 0 + w * p.U, 0 + w * p.V
        pp = Stokes()
        pp.set_polarized(I, Q, U, V, sv.n)
        knew, out = scatter(mix, ell, k, sv, float(dv[0]), float(dv[1]))
        res[i] = [*knew, out.Q, out.U, out.V, *out.n, 1.0 if out.pol else 0.0, I, pp.Q, pp.U, pp.V]
    return res


# ---------------------------------------------------------------- the tests' states
SEED = 20240611
N_RANDOM = 4096


def instrument_axes(inclination_deg, azimuth_deg, pa_deg):
    """kobs and ky of a DistantInstrument (DistantInstrument.cpp:27-50)"""
    th, ph, pa = (math.radians(x) for x in (inclination_deg, azimuth_deg, pa_deg))
    ct, st, cp, sp, ca, sa = math.cos(th), math.sin(th), math.cos(ph), math.sin(ph), math.cos(pa), math.sin(pa)
    kobs = (st * cp, st * sp, ct)
    ky = (-sp * sa - cp * ct * ca, cp * sa - sp * ct * ca, st * ca)
    return kobs, ky


def _perp(k, rng):
    """a unit vector perpendicular to k"""
    while True:
        v = rng.standard_normal(3)
        v -= np.dot(v, k) * np.asarray(k)
        n = np.linalg.norm(v)
        if n > 1e-3:
            return v / n


def make_states(mixes, nlambda, kobs, seed=SEED, n=N_RANDOM):
    """(states [m, 12], deviates [m, 2]): n random states from `seed`, then the explicit ones"""
    rng = np.random.default_rng(seed)
    ncomp = len(mixes)
    states, devs = [], []
    for i in range(n):
        k = rng.standard_normal(3)
        k /= np.linalg.norm(k)
        ell, h = int(rng.integers(nlambda)), int(rng.integers(ncomp))
        if i % 4 == 0:
            st = [*k, 0, 0, 0, 0, 0, 0, 0, ell, h]
        else:
            q = rng.standard_normal(3)
            q *= rng.uniform() / np.linalg.norm(q)
            if i % 4 == 1:
                q[2] = 0.0
            st = [*k, *q, *_perp(k, rng), 1, ell, h]
        states.append(st)
        devs.append(rng.uniform(size=2))
    pols = [(0, 0, 0, 0), (1, 0, 0, 1), (0, -1, 0, 1), (0.3, -0.2, 0.5, 1)]
    top = 1.0 - 2.0 ** -53
    for kz in (1.0, -1.0, 0.999995, -0.999995, 0.99998, -0.99998):
        kx = math.sqrt((1.0 - kz) * (1.0 + kz))
        k = (kx, 0.0, kz)
        for q in pols:
            nrm = (0.0, 1.0, 0.0) if q[3] else (0.0, 0.0, 0.0)
            for h in range(ncomp):
                states.append([*k, q[0], q[1], q[2], *nrm, q[3], 0, h])
                devs.append((0.25 + 0.1 * h, 0.6))
    for sign in (1.0, -1.0):  # peel-off exactly forward and backward
        k = tuple(sign * x for x in kobs)
        for q in pols:
            nrm = tuple(_perp(k, rng)) if q[3] else (0.0, 0.0, 0.0)
            for h in range(ncomp):
                states.append([*k, q[0], q[1], q[2], *nrm, q[3], nlambda - 1, h])
                devs.append((0.37, 0.125))
    k = (0.6, 0.0, 0.8)
    for h in range(ncomp):
        X = mixes[h]["thetaX"][0]
        for dv in ((0.0, 0.0), (top, top), (0.0, top), (top, 0.0), (X[1], 0.41), (X[90], X[45]), (X[120], 0.75),
                   (X[178], 0.25)):  # (the last two entries are both 1: sin(pi) dt rounds away)
            for q in pols[:3]:
                nrm = (0.0, 1.0, 0.0) if q[3] else (0.0, 0.0, 0.0)
                states.append([*k, q[0], q[1], q[2], *nrm, q[3], 0, h])
                devs.append(dv)
    return np.array(states, dtype=np.float64), np.array(devs, dtype=np.float64)
