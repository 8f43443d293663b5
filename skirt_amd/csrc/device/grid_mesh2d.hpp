// Grid<SKIRT_GRID_CYLINDER2D>, Grid<SKIRT_GRID_SPHERE1D> and Grid<SKIRT_GRID_SPHERE2D>: the adapters of the
// axisymmetric and spherical walks of cyl2d_walk.hpp and sph_walk.hpp to the trace lane's Ray.
// Compiles only where engine.hip includes it, inside its anonymous namespace (after Args, Shared and Ray).
#ifndef SKIRT_AMD_DEVICE_GRID_MESH2D_HPP
#define SKIRT_AMD_DEVICE_GRID_MESH2D_HPP

// Axisymmetric R-z grid: Cylinder2DDustGrid.cpp:135-362 through device/cyl2d_walk.hpp (the walk's arithmetic,
// shared with the CPU logic test). The borders R | (one unused word, ny = 0) | z are staged in LDS like the
// Cartesian mesh; device cell number = reference cell number k + nz i, so the cells of one radial shell that
// are adjacent in z share Labs lines. The walk's state lives in registers the Cartesian walk leaves unused:
// q, p, k_q, k_z, q_N in bx0, by0, bz0, bx1, by1; z in r.z; i, i_min, k in ci, cj, ck; inward in jx.
template <>
struct Grid<SKIRT_GRID_CYLINDER2D> {
    __device__ static __forceinline__ const double* zBorders(const Args& a, const Shared& sh) {
        return sh.mesh + a.nx + 1 + a.ny + 1;
    }
    __device__ static __forceinline__ Cyl2dState get(const Ray& r) {
        return Cyl2dState{r.bx0, r.z, r.by0, r.bz0, r.bx1, r.by1, r.ci, r.ck, r.cj, r.jx};
    }
    __device__ static __forceinline__ void put(Ray& r, const Cyl2dState& s) {
        r.bx0 = s.q; r.z = s.z; r.by0 = s.p; r.bz0 = s.kq; r.bx1 = s.kz; r.by1 = s.qN;
        r.ci = s.i; r.ck = s.k; r.cj = s.imin; r.jx = s.inward;
    }
    __device__ static __forceinline__ int dev(const Args& a, int i, int k) { return k + a.nz * i; }

    // the entry part of the path: the segments outside the grid (m = -1), then the first cell; false for an
    // empty path
    template <class SegFn>
    __device__ static __forceinline__ bool begin(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        Cyl2dState s;
        if (!cyl2dEnter(sh.mesh, a.nx, zBorders(a, sh), a.nz, r.x, r.y, r.z, r.dx, r.dy, r.dz, s,
                        [&](int m, double ds) { seg(m, 0.0, ds); }))
            return false;
        put(r, s);
        r.rho0 = a.rho[(size_t)dev(a, s.i, s.k) * a.ncomp];
        return true;
    }

    // one grid step: emits (m, ds); false when the ray ends (left the grid or stopped by seg)
    template <class SegFn>
    __device__ static __forceinline__ bool step(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        Cyl2dState s = get(r);
        const double rho0 = r.rho0;  // loaded by the previous step (or begin), off this step's chain
        int m;
        double ds;
        const bool more = cyl2dStep(sh.mesh, a.nx, zBorders(a, sh), a.nz, s, m, ds);
        if (!seg(m, rho0, ds) || !more) return false;
        put(r, s);
        r.rho0 = a.rho[(size_t)dev(a, s.i, s.k) * a.ncomp];  // the next step's density, requested now
        return true;
    }

    __device__ static __forceinline__ int whichcell(const Args& a, const Shared& sh, double x, double y, double z) {
        return cyl2dWhichCell(sh.mesh, a.nx, zBorders(a, sh), a.nz, x, y, z);
    }
};

// Spherical shells: Sphere1DDustGrid.cpp:111-187 through device/sph_walk.hpp. The borders r (then two unused
// words, ny = nz = 0) are staged in LDS like the Cartesian mesh; r_max = maxR() travels in gx1 (a LogMesh's last
// border may miss it by a bit); device cell number = shell number. State: q, p, q_N in bx0, by0, bz0; i, i_min in
// ci, cj; inward in jx. i moves monotonically in each part of the walk, so a path has at most 2 N_r steps.
template <>
struct Grid<SKIRT_GRID_SPHERE1D> {
    __device__ static __forceinline__ Sph1dState get(const Ray& r) {
        return Sph1dState{r.bx0, r.by0, r.bz0, r.ci, r.cj, r.jx};
    }
    __device__ static __forceinline__ void put(Ray& r, const Sph1dState& s) {
        r.bx0 = s.q; r.by0 = s.p; r.bz0 = s.qN; r.ci = s.i; r.cj = s.imin; r.jx = s.inward;
    }
    __device__ static __forceinline__ int dev(const Args&, int i) { return i; }

    template <class SegFn>
    __device__ static __forceinline__ bool begin(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        Sph1dState s;
        if (!sph1dEnter(sh.mesh, a.nx, a.gx1, r.x, r.y, r.z, r.dx, r.dy, r.dz, s,
                        [&](int m, double ds) { seg(m, 0.0, ds); }))
            return false;
        put(r, s);
        r.rho0 = a.rho[(size_t)s.i * a.ncomp];
        return true;
    }

    template <class SegFn>
    __device__ static __forceinline__ bool step(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        Sph1dState s = get(r);
        const double rho0 = r.rho0;  // loaded by the previous step (or begin), off this step's chain
        int m;
        double ds;
        const bool more = sph1dStep(sh.mesh, a.nx, s, m, ds);
        if (!seg(m, rho0, ds) || !more) return false;
        put(r, s);
        r.rho0 = a.rho[(size_t)s.i * a.ncomp];  // the next step's density, requested now
        return true;
    }

    __device__ static __forceinline__ int whichcell(const Args& a, const Shared& sh, double x, double y, double z) {
        return sph1dWhichCell(sh.mesh, a.nx, x, y, z);
    }
};

// Shells x polar bins: Sphere2DDustGrid.cpp:186-359 through device/sph_walk.hpp. The borders r | cos theta | theta
// (nx = N_r, ny = nz = N_theta) are staged in LDS in the mesh layout; r_max in gx1, eps = 1e-11 r_max in a.eps;
// device cell number = reference cell number k + N_theta i. The position advances in r.x, r.y, r.z; i, k in ci,
// ck; the steps the path may still take (sph2dStepCap) in cj. A step that finds no exit nudges the position and
// emits no segment (m = -1, ds = 0).
template <>
struct Grid<SKIRT_GRID_SPHERE2D> {
    __device__ static __forceinline__ const double* cosBorders(const Args& a, const Shared& sh) {
        return sh.mesh + a.nx + 1;
    }
    __device__ static __forceinline__ const double* thetaBorders(const Args& a, const Shared& sh) {
        return sh.mesh + a.nx + 1 + a.ny + 1;
    }
    __device__ static __forceinline__ int dev(const Args& a, int i, int k) { return k + a.nz * i; }

    template <class SegFn>
    __device__ static __forceinline__ bool begin(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        Sph2dState s;
        if (!sph2dEnter(sh.mesh, a.nx, thetaBorders(a, sh), a.nz, a.gx1, a.eps, r.x, r.y, r.z, r.dx, r.dy, r.dz, s,
                        [&](int m, double ds) { seg(m, 0.0, ds); }))
            return false;
        r.x = s.x; r.y = s.y; r.z = s.z; r.ci = s.i; r.ck = s.k; r.cj = s.left;
        r.rho0 = a.rho[(size_t)dev(a, s.i, s.k) * a.ncomp];
        return true;
    }

    template <class SegFn>
    __device__ static __forceinline__ bool step(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        Sph2dState s{r.x, r.y, r.z, r.ci, r.ck, r.cj};
        const double rho0 = r.rho0;  // loaded by the previous step (or begin), off this step's chain
        int m;
        double ds;
        const bool more = sph2dStep(sh.mesh, a.nx, cosBorders(a, sh), thetaBorders(a, sh), a.nz, a.eps, r.dx, r.dy,
                                    r.dz, s, m, ds);
        if (!seg(m, rho0, ds) || !more) return false;
        r.x = s.x; r.y = s.y; r.z = s.z; r.ci = s.i; r.ck = s.k; r.cj = s.left;
        r.rho0 = a.rho[(size_t)dev(a, s.i, s.k) * a.ncomp];  // the next step's density, requested now
        return true;
    }

    __device__ static __forceinline__ int whichcell(const Args& a, const Shared& sh, double x, double y, double z) {
        return sph2dWhichCell(sh.mesh, a.nx, thetaBorders(a, sh), a.nz, x, y, z);
    }
};

#endif  // SKIRT_AMD_DEVICE_GRID_MESH2D_HPP
