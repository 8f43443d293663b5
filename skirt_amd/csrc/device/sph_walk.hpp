// The paths of a ray through the two spherical dust grids: Sphere1DDustGrid::path
// (SKIRTcore/Sphere1DDustGrid.cpp:111-187) and Sphere2DDustGrid::path (SKIRTcore/Sphere2DDustGrid.cpp:186-359),
// each as an entry function, a step function and a whichcell, in the reference's f64 operations and order. The
// same text compiles for gfx950 (grid_mesh2d.hpp, Grid<SKIRT_GRID_SPHERE1D>, Grid<SKIRT_GRID_SPHERE2D>) and as plain
// C++ (tools/sph_walk_cpu.py, the CPU logic test), so it touches nothing of the engine: borders come in as plain
// arrays (LDS on the device), segments leave through a callable or by reference.
//
// Sphere1D (shells r_i): a ray is (q, p), q the coordinate along the ray, zero at its point of closest approach
// to the centre, p that closest distance, r^2 = p^2 + q^2. The ray moves inward while q < 0, crossing r_i at
// q = -sqrt((r_i - p)(r_i + p)), down to the shell that holds p, then outward through the positive roots. The
// reference's two loops are one step function; a step is ds = q_N - q, the next shell, one square root.
//
// Sphere2D (shells r_i, cones theta_k): the position itself advances, by ds + eps per segment. A step takes the
// smallest positive finite distance among up to four boundaries (inner sphere if i > 0, outer sphere, upper cone
// if k > 0, lower cone if k < N_theta - 1), each the smallest positive root of a quadratic. When no boundary
// gives one, the position moves by eps and (i, k) are located anew from it; such a step emits no segment.
//
// Behaviour of the reference that this reproduces on purpose ("Spherical walks"): a Sphere1D path
// from r > r_max gets its outside segment to the FAR side of the sphere (q_max is the positive root), then one
// zero-length segment in the outermost shell, and so crosses no dust; the Sphere1D outward loop ends at
// i >= N_r - 1, so only a path that starts in the outermost shell crosses it; p = sqrt((r - q)(r + q)) is not
// clamped and may be NaN, after which every segment is NaN (dropped by ds > 0) and the walk still ends within
// N_r steps; Sphere2D discards NaN and infinite candidates by s > 0 && s < DBL_MAX, adds eps to every advance
// but not to ds, and nudges a start at the origin by eps. The one choice of the engine's own: a Sphere2D path
// ends after sph2dStepCap steps. The reference's nudge branch has no bound: with a NaN direction inside the grid
// every candidate is NaN, the nudged position is NaN, and NR::locate_fail puts a NaN radius in the last shell
// (every comparison is false), so its loop never returns. Here that path ends at the cap, without a segment.
#pragma once

#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define SKIRT_SPH_FN __host__ __device__ __forceinline__
#else
#define SKIRT_SPH_FN inline
#endif

SKIRT_SPH_FN int sphLocateBasic(const double* v, double x, int n) {  // NR::locate_basic_impl
    int jl = -1, ju = n;
    while (ju - jl > 1) {
        const int jm = (ju + jl) >> 1;
        if (x < v[jm]) ju = jm;
        else jl = jm;
    }
    return jl;
}
// NR::locate_clip / NR::locate_fail over the n + 1 borders of n bins (a NaN lands in the last bin: every
// comparison with it is false)
SKIRT_SPH_FN int sphLocateClip(const double* v, int n, double x) {
    if (x < v[0]) return 0;
    return sphLocateBasic(v, x, n);
}
SKIRT_SPH_FN int sphLocateFail(const double* v, int n, double x) {
    if (x > v[n]) return -1;
    return sphLocateBasic(v, x, n);
}

// ------------------------------------------------------------------ Sphere1D
// the walk's state between two steps
struct Sph1dState {
    double q;    // the ray's position along itself
    double p;    // distance of closest approach to the centre (NaN for a ray radial to within rounding)
    double qN;   // q of the next crossing: of r_i while inward, of r_{i+1} while outward
    int i;       // shell of the current cell (cell number i)
    int imin;    // the shell holding p: the inward part ends on reaching it
    int inward;  // 1 in the reference's inward loop (q < 0 and i > imin), else 0
};

// Sphere1DDustGrid::whichcell: the cell of a position, -1 outside (Vec::norm)
SKIRT_SPH_FN int sph1dWhichCell(const double* rv, int Nr, double x, double y, double z) {
    return sphLocateFail(rv, Nr, sqrt(x * x + y * y + z * z));
}

// the crossing a state heads for, after its shell changed or the walk began
SKIRT_SPH_FN void sph1dAim(const double* rv, Sph1dState& s) {
    s.inward = s.inward && s.i > s.imin;  // (leaving the inward loop emits no segment)
    const double rN = s.inward ? rv[s.i] : rv[s.i + 1];
    const double root = sqrt((rN - s.p) * (rN + s.p));
    s.qN = s.inward ? -root : root;
}

// Entry (Sphere1DDustGrid.cpp:113-144): the segment before the grid through emit(-1, ds), then the first shell
// in s; false for an empty path. rv: Nr + 1 borders; rmax = maxR(), which a LogMesh's rv[Nr] may miss by a bit.
template <class Emit>
SKIRT_SPH_FN bool sph1dEnter(const double* rv, int Nr, double rmax, double x, double y, double z, double kx,
                             double ky, double kz, Sph1dState& s, Emit emit) {
    double r = sqrt(x * x + y * y + z * z);
    double q = x * kx + y * ky + z * kz;
    const double p = sqrt((r - q) * (r + q));
    if (r > rmax) {
        if (q > 0.0 || p > rmax) return false;
        r = rmax - 1e-8 * (rv[Nr] - rv[Nr - 1]);
        const double qmax = sqrt((rmax - p) * (rmax + p));
        emit(-1, qmax - q);
        q = qmax;
    }
    s.q = q; s.p = p;
    s.i = sphLocateClip(rv, Nr, r);
    s.inward = q < 0.0;
    s.imin = s.inward ? sphLocateClip(rv, Nr, p) : 0;
    sph1dAim(rv, s);
    return true;
}

// One step (Sphere1DDustGrid.cpp:148-186): the segment (m, ds) of the current shell, then the next state; false
// when the path ended with this segment. i moves monotonically in each part, so a path has at most 2 N_r steps.
SKIRT_SPH_FN bool sph1dStep(const double* rv, int Nr, Sph1dState& s, int& m, double& ds) {
    m = s.i;
    ds = s.qN - s.q;
    if (s.inward) {
        s.i--;
    } else {
        s.i++;
        if (s.i >= Nr - 1) return false;
    }
    s.q = s.qN;
    sph1dAim(rv, s);
    return true;
}

// ------------------------------------------------------------------ Sphere2D
// the longest path in steps, segments and eps nudges alike: a line crosses at most 2 (N_r + 1) spheres and
// 2 (N_theta + 1) cone sheets
SKIRT_SPH_FN int sph2dStepCap(int Nr, int Nt) { return 4 * (Nr + Nt) + 16; }

// Vec::spherical's radius and polar angle (Vec.cpp: r = norm(), theta = acos(z/r), 0 at r = 0)
SKIRT_SPH_FN void sph2dLocate(const double* rv, int Nr, const double* thv, int Nt, double x, double y, double z,
                              int& i, int& k) {
    const double r = sqrt(x * x + y * y + z * z);
    const double theta = r == 0 ? 0.0 : acos(z / r);
    i = sphLocateFail(rv, Nr, r);
    k = sphLocateClip(thv, Nt, theta);
}

// Sphere2DDustGrid::whichcell: the cell of a position, -1 outside
SKIRT_SPH_FN int sph2dWhichCell(const double* rv, int Nr, const double* thv, int Nt, double x, double y, double z) {
    int i, k;
    sph2dLocate(rv, Nr, thv, Nt, x, y, z, i, k);
    if (i < 0) return -1;
    return k + Nt * i;
}

// smallest positive solution of x^2 + 2 b x + c = 0, or 0 (Sphere2DDustGrid.cpp:189-217)
SKIRT_SPH_FN double sphSmallestPositive(double b, double c) {
    if (b * b > c) {
        if (b > 0) {
            if (c < 0) {
                const double x1 = -b - sqrt(b * b - c);
                return c / x1;
            }
        } else {
            const double x2 = -b + sqrt(b * b - c);
            if (c > 0) {
                const double x1 = c / x2;
                if (x1 < x2) return x1;
            }
            return x2;
        }
    }
    return 0;
}
// of a x^2 + 2 b x + c = 0 (Sphere2DDustGrid.cpp:220-226)
SKIRT_SPH_FN double sphSmallestPositive(double a, double b, double c) {
    if (fabs(a) > 1e-9) return sphSmallestPositive(b / a, c / a);
    const double x = -0.5 * c / b;
    if (x > 0) return x;
    return 0;
}

struct Sph2dState {
    double x, y, z;  // the position, advanced by k (ds + eps) per segment
    int i, k;        // radial and polar bin of the current cell (cell number k + N_theta i)
    int left;        // steps the path may still take (sph2dStepCap at the start)
};

// Entry (Sphere2DDustGrid.cpp:250-284): the segment before the grid through emit(-1, ds), then the first cell in
// s; false for an empty path (also one whose start has no radial bin: the reference's loop does not run).
// rv, cv, thv: the N_r + 1 radial borders, the N_theta + 1 fixed-up cosines and polar borders; rmax = maxR().
template <class Emit>
SKIRT_SPH_FN bool sph2dEnter(const double* rv, int Nr, const double* thv, int Nt, double rmax, double eps, double x,
                             double y, double z, double kx, double ky, double kz, Sph2dState& s, Emit emit) {
    const double r2 = x * x + y * y + z * z;
    if (r2 > rmax * rmax) {
        const double ds = sphSmallestPositive(x * kx + y * ky + z * kz, r2 - rmax * rmax);
        if (!ds) return false;
        emit(-1, ds);
        x += kx * (ds + eps); y += ky * (ds + eps); z += kz * (ds + eps);
    } else if (r2 == 0) {
        x += kx * eps; y += ky * eps; z += kz * eps;
    }
    s.x = x; s.y = y; s.z = z;
    sph2dLocate(rv, Nr, thv, Nt, x, y, z, s.i, s.k);
    s.left = sph2dStepCap(Nr, Nt);
    return s.i >= 0;  // (locate_fail never returns N_r or more)
}

// One step (Sphere2DDustGrid.cpp:285-358): either the segment (m, ds) of the current cell and the move into the
// next one, or (m = -1, ds = 0) after an eps nudge; false when the path ended with this step (the segment, if
// any, still counts).
SKIRT_SPH_FN bool sph2dStep(const double* rv, int Nr, const double* cv, const double* thv, int Nt, double eps,
                            double kx, double ky, double kz, Sph2dState& s, int& m, double& ds) {
    const int i = s.i, k = s.k;
    // the terms the four boundaries share (Vec::dot, Vec::norm2 and the products with the z components)
    const double rk = s.x * kx + s.y * ky + s.z * kz;
    const double rr = s.x * s.x + s.y * s.y + s.z * s.z;
    const double zk = s.z * kz, kzkz = kz * kz, zz = s.z * s.z;
    auto cone = [&](double c) {
        return c ? sphSmallestPositive(c * c - kzkz, c * c * rk - zk, c * c * rr - zz) : -s.z / kz;
    };
    int inext = i, knext = k;
    ds = DBL_MAX;
    if (i > 0) {
        const double t = sphSmallestPositive(rk, rr - rv[i] * rv[i]);
        if (t > 0 && t < ds) { ds = t; inext = i - 1; knext = k; }
    }
    {
        const double t = sphSmallestPositive(rk, rr - rv[i + 1] * rv[i + 1]);
        if (t > 0 && t < ds) { ds = t; inext = i + 1; knext = k; }
    }
    if (k > 0) {
        const double t = cone(cv[k]);
        if (t > 0 && t < ds) { ds = t; inext = i; knext = k - 1; }
    }
    if (k < Nt - 1) {
        const double t = cone(cv[k + 1]);
        if (t > 0 && t < ds) { ds = t; inext = i; knext = k + 1; }
    }
    if (inext != i || knext != k) {
        m = k + Nt * i;
        s.x += kx * (ds + eps); s.y += ky * (ds + eps); s.z += kz * (ds + eps);
        s.i = inext; s.k = knext;
    } else {
        // no exit point found: move a tiny bit along the path and locate the cell again
        m = -1;
        ds = 0.0;
        s.x += kx * eps; s.y += ky * eps; s.z += kz * eps;
        sph2dLocate(rv, Nr, thv, Nt, s.x, s.y, s.z, s.i, s.k);
    }
    s.left--;
    return s.i < Nr && s.i >= 0 && s.left > 0;
}
