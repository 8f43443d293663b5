"""Plain-Python restatement of the reference's six anisotropically emitting geometries -- NetzerAccretionDiskGeometry,
StellarSurfaceGeometry, SpheBackgroundGeometry, CubBackgroundGeometry, SolarPatchGeometry, LaserGeometry
(SKIRTcore/*.cpp of the same names) -- as GeometricStellarComp::launch and PhotonPackage::launchEmissionPeelOff use
them: generatePosition, generateDirection(position) and probabilityForDirection(position, direction), with the
reference's own trigonometry (acos, asin, atan2, sin and cos of the angles; Direction(theta, phi) with its 1e-8 pole
cut-offs; Position::spherical; Random::cdf as NR::locate_clip + NR::interpolate_linlin). A geometry is (kind, r0):
r0 the radius (surface, sphebg, patch) or the extent (cubbg), unused for netzer and laser. u is a callable that returns
the next uniform deviate (geom_ref.PhiloxStream). The engine's header (skirt_amd/csrc/device/aniso_emission.hpp)
avoids the inverse functions; the tests compare the two on the same deviates."""
import math

KINDS = ["netzer", "surface", "sphebg", "cubbg", "patch", "laser"]
KIND_CODE = {"netzer": 10, "surface": 11, "sphebg": 12, "cubbg": 13, "patch": 14, "laser": 15}  # SKIRT_GEOM_*
ELEMENT = {
    "netzer": '<NetzerAccretionDiskGeometry/>',
    "surface": '<StellarSurfaceGeometry radius="%s pc"/>',
    "sphebg": '<SpheBackgroundGeometry radius="%s pc"/>',
    "cubbg": '<CubBackgroundGeometry extent="%s pc"/>',
    "patch": '<SolarPatchGeometry radius="%s pc"/>',
    "laser": '<LaserGeometry/>',
}
DRAWS = {"netzer": 2, "surface": 4, "sphebg": 4, "cubbg": 5, "patch": 4, "laser": 0}  # position + direction
DIMENSION = {"netzer": 2, "surface": 1, "sphebg": 1, "cubbg": 3, "patch": 2, "laser": 2}
EPS = 1e-8


class FatalError(RuntimeError):
    pass


def element(kind, r0_pc=300):
    e = ELEMENT[kind]
    return e % r0_pc if "%s" in e else e


def direction_of(theta, phi):
    """Direction(theta, phi), Direction.cpp:12-38"""
    if theta < -EPS or theta > math.pi + EPS:
        raise FatalError("Theta should be between 0 and pi.")
    if theta <= EPS:
        return (0.0, 0.0, 1.0)
    if theta >= math.pi - EPS:
        return (0.0, 0.0, -1.0)
    st = math.sin(theta)
    return (st * math.cos(phi), st * math.sin(phi), math.cos(theta))


def random_direction(u):
    """Random::direction()"""
    theta = math.acos(2.0 * u() - 1.0)
    phi = 2.0 * math.pi * u()
    return direction_of(theta, phi)


def netzer_table():
    """NetzerAccretionDiskGeometry::setupSelfBefore: (thetav, Xv), 401 entries"""
    N = 401
    thetav, Xv = [0.0] * N, [0.0] * N
    for i in range(1, N - 1):
        thetav[i] = math.pi * i / (N - 1)
        ct = math.cos(thetav[i])
        sign = 1.0 if ct > 0 else -1.0
        Xv[i] = (1. / 2.) - (2. / 7.) * ct * ct * ct - sign * (3. / 14.) * ct * ct
    thetav[N - 1] = math.pi
    Xv[N - 1] = 1.0
    return thetav, Xv


_NETZER = netzer_table()


def _cdf(xv, Xv, u):
    """Random::cdf"""
    X = u()
    n = len(Xv)
    if X < Xv[0]:
        i = 0
    else:  # NR::locate_basic_impl(Xv, X, n - 1)
        jl, ju = -1, n - 1
        while ju - jl > 1:
            jm = (ju + jl) >> 1
            if X < Xv[jm]:
                ju = jm
            else:
                jl = jm
        i = jl
    return xv[i] + ((X - Xv[i]) / (Xv[i + 1] - Xv[i])) * (xv[i + 1] - xv[i])


def position(kind, r0, u):
    """Geometry::generatePosition"""
    if kind in ("netzer", "laser"):
        return (0.0, 0.0, 0.0)
    if kind in ("surface", "sphebg"):
        k = random_direction(u)
        return (r0 * k[0], r0 * k[1], r0 * k[2])
    if kind == "cubbg":
        h = r0
        t1 = h * (2.0 * u() - 1.0)
        t2 = h * (2.0 * u() - 1.0)
        X = u()
        if X < 1.0 / 6.0:
            return (-h, t1, t2)
        elif X < 1.0 / 3.0:
            return (h, t1, t2)
        elif X < 0.5:
            return (t1, -h, t2)
        elif X < 2.0 / 3.0:
            return (t1, h, t2)
        elif X < 5.0 / 6.0:
            return (t1, t2, -h)
        return (t1, t2, h)
    if kind == "patch":
        R = r0 * math.sqrt(u())
        phi = 2.0 * math.pi * u()
        return (R * math.cos(phi), R * math.sin(phi), 0.0)  # Position(R, phi, z, CYLINDRICAL)
    raise ValueError(kind)


def _radius(p):
    return math.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2])


def _spherical(p):
    """Position::spherical"""
    r = _radius(p)
    if r == 0:
        return r, 0.0, 0.0
    return r, math.acos(p[2] / r), math.atan2(p[1], p[0])


def _rotate(p, kp):
    r, theta, phi = _spherical(p)
    ct, st, cp, sp = math.cos(theta), math.sin(theta), math.cos(phi), math.sin(phi)
    kpx, kpy, kpz = kp
    return (ct * cp * kpx - sp * kpy + st * cp * kpz, ct * sp * kpx + cp * kpy + st * sp * kpz, -st * kpx + ct * kpz)


def cube_face(h, p):
    """the face of the reference's cascade: 0 -x, 1 +x, 2 -y, 3 +y, 4 -z, 5 +z; None off the cube"""
    x, y, z = p
    ax, ay, az = abs(x), abs(y), abs(z)
    if abs(x / h + 1.0) < EPS and ay <= h and az <= h:
        return 0
    elif abs(x / h - 1.0) < EPS and ay <= h and az <= h:
        return 1
    elif abs(y / h + 1.0) < EPS and ax <= h and az <= h:
        return 2
    elif abs(y / h - 1.0) < EPS and ax <= h and az <= h:
        return 3
    elif abs(z / h + 1.0) < EPS and ax <= h and ay <= h:
        return 4
    elif abs(z / h - 1.0) < EPS and ax <= h and ay <= h:
        return 5
    return None


def direction(kind, r0, p, u):
    """AngularDistribution::generateDirection at position p"""
    if kind == "netzer":
        if _radius(p) > 0.0:
            raise FatalError("no directions should be generated at positions besides the origin")
        theta = _cdf(_NETZER[0], _NETZER[1], u)
        phi = 2.0 * math.pi * u()
        return direction_of(theta, phi)
    if kind == "laser":
        if _radius(p) > 0.0:
            raise FatalError("no directions should be generated at positions besides the origin")
        return (0.0, 0.0, 1.0)
    if kind == "surface":
        if abs(_radius(p) / r0 - 1.0) > EPS:
            raise FatalError("cannot generate directions for positions not on the stellar surface")
        thetap = math.asin(math.sqrt(u()))
        phip = 2.0 * math.pi * u()
        return _rotate(p, direction_of(thetap, phip))
    if kind == "sphebg":
        if abs(_radius(p) / r0 - 1.0) > EPS:
            raise FatalError("cannot generate directions for positions not on the SpheBackground sphere")
        thetap = math.pi - math.acos(math.sqrt(u()))
        phip = 2.0 * math.pi * u()
        return _rotate(p, direction_of(thetap, phip))
    if kind == "cubbg":
        thetap = math.pi - math.acos(math.sqrt(u()))
        phip = 2.0 * math.pi * u()
        kpx, kpy, kpz = direction_of(thetap, phip)
        face = cube_face(r0, p)
        if face is None:
            raise FatalError("cannot generate directions for positions not on the background cube")
        return [(-kpz, -kpy, -kpx), (kpz, kpy, -kpx), (kpy, -kpz, -kpx), (-kpy, kpz, -kpx), (-kpx, kpy, -kpz),
                (kpx, kpy, kpz)][face]
    if kind == "patch":
        theta = math.asin(math.sqrt(u()))
        phi = 2.0 * math.pi * u()
        return direction_of(theta, phi)
    raise ValueError(kind)


def _theta_of(k):
    """theta of Direction::spherical"""
    return math.acos(k[2])


def probability(kind, r0, p, k):
    """AngularDistribution::probabilityForDirection"""
    if kind == "netzer":
        if _radius(p) > 0.0:
            raise FatalError("the angular probability function is not defined for positions besides the origin")
        ct = math.cos(_theta_of(k))
        sign = 1.0 if ct > 0 else -1.0
        return (6. / 7.) * ct * (2. * ct + sign)
    if kind == "laser":
        if _radius(p) > 0.0:
            raise FatalError("the angular probability function is not defined for positions besides the origin")
        return math.inf if _theta_of(k) == 0.0 else 0.0
    if kind == "surface":
        if abs(_radius(p) / r0 - 1.0) > EPS:
            raise FatalError("the directional probability function is not defined for positions not on the stellar surface")
        c = (p[0] * k[0] + p[1] * k[1] + p[2] * k[2]) / r0
        return 4.0 * c if c > 0.0 else 0.0
    if kind == "sphebg":
        if abs(_radius(p) / r0 - 1.0) > EPS:
            raise FatalError("the directional probability function is not defined for positions not on the background sphere")
        c = (p[0] * k[0] + p[1] * k[1] + p[2] * k[2]) / r0
        return 0.0 if c > 0.0 else -4.0 * c
    if kind == "cubbg":
        face = cube_face(r0, p)
        if face is None:
            raise FatalError("the directional probability function is not defined for positions not on the background cube")
        n = [(-1., 0., 0.), (1., 0., 0.), (0., -1., 0.), (0., 1., 0.), (0., 0., -1.), (0., 0., 1.)][face]
        c = n[0] * k[0] + n[1] * k[1] + n[2] * k[2]
        return 0.0 if c > 0.0 else -4.0 * c
    if kind == "patch":
        return 4.0 * k[2] if k[2] > 0.0 else 0.0
    raise ValueError(kind)


def netzer_probability(cos_theta):
    """P = (6/7) c (2 c + sign c)"""
    return (6. / 7.) * cos_theta * (2. * cos_theta + (1.0 if cos_theta > 0 else -1.0))


def adversarial_positions(kind, r0):
    """positions where the rotation or the face cascade could go wrong: both poles and the x and y axes of a sphere;
    the 12 edges and 8 corners of the cube, where the first matching face decides; the origin for the disk and the laser;
    centre, rim and axes of the patch"""
    if kind in ("netzer", "laser"):
        return [(0.0, 0.0, 0.0)]
    if kind in ("surface", "sphebg"):
        return [(0.0, 0.0, r0), (0.0, 0.0, -r0), (r0, 0.0, 0.0), (-r0, 0.0, 0.0), (0.0, r0, 0.0), (0.0, -r0, 0.0)]
    if kind == "cubbg":
        pts = [(sx * r0, sy * r0, sz * r0) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]  # 8 corners
        for s1 in (-1, 1):
            for s2 in (-1, 1):  # 12 edges, at a point off their middle
                pts += [(0.3 * r0, s1 * r0, s2 * r0), (s1 * r0, -0.7 * r0, s2 * r0), (s1 * r0, s2 * r0, 0.1 * r0)]
        return pts
    return [(0.0, 0.0, 0.0), (r0, 0.0, 0.0), (0.0, -r0, 0.0), (0.5 * r0, 0.5 * r0, 0.0)]


def adversarial_directions(kind):
    """kz = +-1 and kz = 0 (the Netzer law's sign change), and a few oblique ones; the laser never along +z"""
    s = math.sqrt(0.5)
    dirs = [(0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (s, 0.0, s), (0.0, -s, -s), (0.6, 0.0, 0.8),
            (-0.48, 0.6, -0.64)]
    if kind != "laser":
        dirs.append((0.0, 0.0, 1.0))
    return dirs
