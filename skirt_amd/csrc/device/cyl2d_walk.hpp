// The path of a ray through an axisymmetric R-z dust grid: Cylinder2DDustGrid::path
// (SKIRTcore/Cylinder2DDustGrid.cpp:135-362) as an entry function and a step function, in the reference's f64
// operations and order. The same text compiles for gfx950 (grid_mesh2d.hpp, Grid<SKIRT_GRID_CYLINDER2D>) and as
// plain C++ (tools/cyl2d_walk_cpu.py, the CPU logic test), so it touches nothing of the engine: borders come in
// as plain arrays (LDS on the device), segments leave through a callable.
//
// In the plane of the ray and the z axis' parallel through it, a ray is (q, z): q the coordinate along the
// ray's horizontal projection, zero at its point of closest approach to the axis, p >= 0 that closest
// distance, so R^2 = p^2 + q^2. k_q and k_z are the direction's components; q grows along the ray. The ray
// moves inward (R falls) while q < 0, crossing the borders R_i at q = -sqrt((R_i - p)(R_i + p)), down to the
// shell that holds p, then outward, crossing R_{i+1} at the positive root. The reference writes this as two
// loops (inward, outward) per vertical direction; cyl2dStep is those four loops as one step. Behaviour of the
// reference that this reproduces on purpose ("Cylindrical walk"): a path that starts at
// R >= R_max gets its outside segment to the FAR side of the cylinder (q_max is the positive root) and so
// crosses no dust; a downward path ends when it crosses outward into the last radial shell (i >= N_R - 1,
// upward paths i >= N_R); k_z == 0 and k_q == 0 become 1e-20, and k_z == 0 counts as upward.
//
// A grid kind with other coordinates (a spherical r-theta sibling) would add its own state and its own
// enter/step pair next to these, under the same two-function shape.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define SKIRT_CYL_FN __host__ __device__ __forceinline__
#else
#define SKIRT_CYL_FN inline
#endif

// the walk's state between two steps
struct Cyl2dState {
    double q, z;    // the ray's position in its (q, z) plane
    double p;       // distance of closest approach to the axis
    double kq, kz;  // direction components (exact zeros replaced by 1e-20)
    double qN;      // q of the next radial crossing: of R_i while inward, of R_{i+1} while outward
    int i, k;       // radial and vertical bin of the current cell (cell number k + Nz i)
    int imin;       // the shell holding p: the inward part ends on reaching it
    int inward;     // 1 in the reference's inward loop (q < 0 and i > imin), else 0
};

SKIRT_CYL_FN int cyl2dLocateBasic(const double* v, double x, int n) {  // NR::locate_basic_impl
    int jl = -1, ju = n;
    while (ju - jl > 1) {
        const int jm = (ju + jl) >> 1;
        if (x < v[jm]) ju = jm;
        else jl = jm;
    }
    return jl;
}
// NR::locate_clip / NR::locate_fail over the n + 1 borders of n bins
SKIRT_CYL_FN int cyl2dLocateClip(const double* v, int n, double x) {
    if (x < v[0]) return 0;
    return cyl2dLocateBasic(v, x, n);
}
SKIRT_CYL_FN int cyl2dLocateFail(const double* v, int n, double x) {
    if (x > v[n]) return -1;
    return cyl2dLocateBasic(v, x, n);
}

// Cylinder2DDustGrid::whichcell: the cell of a position, -1 outside
SKIRT_CYL_FN int cyl2dWhichCell(const double* Rv, int NR, const double* zv, int Nz, double x, double y, double z) {
    const int i = cyl2dLocateFail(Rv, NR, sqrt(x * x + y * y));
    const int k = cyl2dLocateFail(zv, Nz, z);
    if (i < 0 || k < 0) return -1;
    return k + Nz * i;
}

// the radial crossing a state heads for, after its cell changed radially or the walk began
SKIRT_CYL_FN void cyl2dAim(const double* Rv, Cyl2dState& s) {
    s.inward = s.inward && s.i > s.imin;  // (leaving the inward loop emits no segment)
    const double RN = s.inward ? Rv[s.i] : Rv[s.i + 1];
    const double root = sqrt((RN - s.p) * (RN + s.p));
    s.qN = s.inward ? -root : root;
}

// Entry (Cylinder2DDustGrid.cpp:137-202): the segments before the grid through emit(-1, ds), then the first
// cell in s; false for an empty path. Rv: NR + 1 borders with R_max = Rv[NR]; zv: Nz + 1 borders with
// z_min = zv[0], z_max = zv[Nz]. Segments are emitted only once the path is known not to be empty (the
// reference clears them otherwise).
template <class Emit>
SKIRT_CYL_FN bool cyl2dEnter(const double* Rv, int NR, const double* zv, int Nz, double x, double y, double z,
                             double kx, double ky, double kz, Cyl2dState& s, Emit emit) {
    double kq = sqrt(kx * kx + ky * ky);
    if (kz == 0.0) kz = 1e-20;  // avoid moving exactly parallel to the equatorial plane
    if (kq == 0.0) kq = 1e-20;  // avoid moving exactly parallel to the z axis
    double R = sqrt(x * x + y * y);
    double q = (x * kx + y * ky) / kq;
    const double p2 = (R - q) * (R + q);
    const double p = sqrt(p2 > 0.0 ? p2 : 0.0);
    const double Rmax = Rv[NR], zmin = zv[0], zmax = zv[Nz];
    double d0 = 0.0, d1 = 0.0;
    if (R >= Rmax) {
        if (q > 0.0 || p > Rmax) return false;
        R = Rmax - 1e-8 * (Rv[NR] - Rv[NR - 1]);
        const double qmax = sqrt((Rmax - p) * (Rmax + p));
        d0 = (qmax - q) / kq;
        q = qmax;
        z += kz * d0;
    }
    if (z < zmin) {
        if (kz <= 0.0) return false;
        d1 = (zmin - z) / kz;
        q += kq * d1;
        R = sqrt(p * p + q * q);
        z = zmin + 1e-8 * (zv[1] - zv[0]);
    } else if (z > zmax) {
        if (kz >= 0.0) return false;
        d1 = (zmax - z) / kz;
        q += kq * d1;
        R = sqrt(p * p + q * q);
        z = zmax - 1e-8 * (zv[Nz] - zv[Nz - 1]);
    }
    // (NaN fails every comparison and an infinity one of them: the reference's isinf/isnan tests)
    if (!(R < Rmax && z > zmin && z < zmax)) return false;
    if (d0 > 0.0) emit(-1, d0);  // (DustGridPath::addSegment skips ds <= 0)
    if (d1 > 0.0) emit(-1, d1);
    s.q = q; s.z = z; s.p = p; s.kq = kq; s.kz = kz;
    s.i = cyl2dLocateClip(Rv, NR, R);
    s.k = cyl2dLocateClip(zv, Nz, z);
    s.imin = cyl2dLocateClip(Rv, NR, p);
    s.inward = q < 0.0;
    cyl2dAim(Rv, s);
    return true;
}

// One step (Cylinder2DDustGrid.cpp:206-361): the segment (m, ds) of the current cell, then the next state;
// false when the path ended with this segment.
SKIRT_CYL_FN bool cyl2dStep(const double* Rv, int NR, const double* zv, int Nz, Cyl2dState& s, int& m, double& ds) {
    const bool up = s.kz >= 0.0;
    const double zN = up ? zv[s.k + 1] : zv[s.k];
    const double dsq = (s.qN - s.q) / s.kq;
    const double dsz = (zN - s.z) / s.kz;
    const bool radial = dsq < dsz;
    m = s.k + Nz * s.i;
    ds = radial ? dsq : dsz;
    if (radial) {
        s.i += s.inward ? -1 : 1;
        // outward, the upward loop ends past the last shell, the downward loop on entering it
        if (!s.inward && s.i >= (up ? NR : NR - 1)) return false;
        s.q = s.qN;
        s.z += s.kz * ds;
        cyl2dAim(Rv, s);
    } else {
        s.k += up ? 1 : -1;
        if (s.k >= Nz || s.k < 0) return false;
        s.q += s.kq * ds;
        s.z = zN;
    }
    return true;
}
