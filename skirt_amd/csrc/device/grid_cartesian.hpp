// Grid<SKIRT_GRID_CARTESIAN>: the walk through a Cartesian dust grid.
// Compiles only where engine.hip includes it, inside its anonymous namespace (after Args, Shared and Ray).
#ifndef SKIRT_AMD_DEVICE_GRID_CARTESIAN_HPP
#define SKIRT_AMD_DEVICE_GRID_CARTESIAN_HPP

// Cartesian grid: CartesianDustGrid.cpp:136-283 (mesh borders staged in LDS)
template <>
struct Grid<SKIRT_GRID_CARTESIAN> {
    __device__ static __forceinline__ int locateClip(const double* v, int n, double q) {  // NR::locate_clip
        if (q < v[0]) return 0;
        int jl = -1, ju = n - 1;
        while (ju - jl > 1) {
            const int jm = (ju + jl) >> 1;
            if (q < v[jm]) ju = jm;
            else jl = jm;
        }
        return jl;
    }
    __device__ static __forceinline__ int locateFail(const double* v, int n, double q) {  // NR::locate_fail
        if (q > v[n - 1]) return -1;
        int jl = -1, ju = n - 1;
        while (ju - jl > 1) {
            const int jm = (ju + jl) >> 1;
            if (q < v[jm]) ju = jm;
            else jl = jm;
        }
        return jl;
    }

    // the entry part of the path: up to three segments outside the grid (m = -1), then the first cell;
    // false for an empty path
    template <class SegFn>
    __device__ static __forceinline__ bool begin(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        const double* xv = sh.mesh;
        const double* yv = xv + a.nx + 1;
        const double* zv = yv + a.ny + 1;
        const double kx = r.dx, ky = r.dy, kz = r.dz;
        double x = r.x, y = r.y, z = r.z, d0 = 0, d1 = 0, d2 = 0;
        if (x < a.gx0) {
            if (kx <= 0.0) return false;
            d0 = (a.gx0 - x) / kx;
            x = a.gx0 + 1e-8 * (xv[1] - xv[0]); y += ky * d0; z += kz * d0;
        } else if (x > a.gx1) {
            if (kx >= 0.0) return false;
            d0 = (a.gx1 - x) / kx;
            x = a.gx1 - 1e-8 * (xv[a.nx] - xv[a.nx - 1]); y += ky * d0; z += kz * d0;
        }
        if (y < a.gy0) {
            if (ky <= 0.0) return false;
            d1 = (a.gy0 - y) / ky;
            x += kx * d1; y = a.gy0 + 1e-8 * (yv[1] - yv[0]); z += kz * d1;
        } else if (y > a.gy1) {
            if (ky >= 0.0) return false;
            d1 = (a.gy1 - y) / ky;
            x += kx * d1; y = a.gy1 - 1e-8 * (yv[a.ny] - yv[a.ny - 1]); z += kz * d1;
        }
        if (z < a.gz0) {
            if (kz <= 0.0) return false;
            d2 = (a.gz0 - z) / kz;
            x += kx * d2; y += ky * d2; z = a.gz0 + 1e-8 * (zv[1] - zv[0]);
        } else if (z > a.gz1) {
            if (kz >= 0.0) return false;
            d2 = (a.gz1 - z) / kz;
            x += kx * d2; y += ky * d2; z = a.gz1 - 1e-8 * (zv[a.nz] - zv[a.nz - 1]);
        }
        if (x < a.gx0 || x > a.gx1 || y < a.gy0 || y > a.gy1 || z < a.gz0 || z > a.gz1) return false;
        if (d0 > 0) seg(-1, 0.0, d0);
        if (d1 > 0) seg(-1, 0.0, d1);
        if (d2 > 0) seg(-1, 0.0, d2);
        r.x = x; r.y = y; r.z = z;
        r.ci = locateClip(xv, a.nx + 1, x);
        r.cj = locateClip(yv, a.ny + 1, y);
        r.ck = locateClip(zv, a.nz + 1, z);
        r.rho0 = a.rho[(size_t)dev(a, r.ci, r.cj, r.ck) * a.ncomp];
        return true;
    }

    // device number of cell (i, j, k). Bricked: the 8 cells of each 2x2x2 brick are consecutive and
    // start on a 64-byte line of every Labs row (a ray crosses about 2.5 cells of a brick it enters,
    // whose Labs adds then share one atomic request); bricks in the reference's (i, j, k) order.
    // Unbricked: the reference's index k + Nz j + Nz Ny i (CartesianDustGrid.cpp:305-308).
    __device__ static __forceinline__ int dev(const Args& a, int i, int j, int k) {
        if (!a.brick) return k + a.nz * j + a.nz * a.ny * i;
        const int by = (a.ny + 1) >> 1, bz = (a.nz + 1) >> 1;
        return ((((i >> 1) * by + (j >> 1)) * bz + (k >> 1)) << 3) | ((i & 1) << 2) | ((j & 1) << 1) | (k & 1);
    }

    // one grid step: emits (m, ds); false when the ray ends (left the grid or stopped by seg)
    template <class SegFn>
    __device__ static __forceinline__ bool step(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        const double* xv = sh.mesh;
        const double* yv = xv + a.nx + 1;
        const double* zv = yv + a.ny + 1;
        const int i = r.ci, j = r.cj, k = r.ck;
        const int m = dev(a, i, j, k);
        const double rho0 = r.rho0;  // loaded by the previous step (or begin), off this step's chain
        const double xE = (r.dx < 0.0) ? xv[i] : xv[i + 1];
        const double yE = (r.dy < 0.0) ? yv[j] : yv[j + 1];
        const double zE = (r.dz < 0.0) ? zv[k] : zv[k + 1];
        const double dsx = (r.ix != 0.0) ? (xE - r.x) * r.ix : kDblMax;
        const double dsy = (r.iy != 0.0) ? (yE - r.y) * r.iy : kDblMax;
        const double dsz = (r.iz != 0.0) ? (zE - r.z) * r.iz : kDblMax;
        // the exit wall (the reference's order of comparisons), then one segment: lanes leaving through
        // different walls share the segment code instead of running it once per wall
        const bool ex = dsx <= dsy && dsx <= dsz;
        const bool ey = !ex && dsy < dsx && dsy <= dsz;
        const bool ez = !ex && !ey && dsz < dsx && dsz < dsy;
        if (!(ex || ey || ez)) return false;  // NaN direction; the reference would loop forever
        const double ds = ex ? dsx : ey ? dsy : dsz;
        if (!seg(m, rho0, ds)) return false;
        const int ni = i + (ex ? ((r.dx < 0.0) ? -1 : 1) : 0);
        const int nj = j + (ey ? ((r.dy < 0.0) ? -1 : 1) : 0);
        const int nk = k + (ez ? ((r.dz < 0.0) ? -1 : 1) : 0);
        if (ni >= a.nx || ni < 0 || nj >= a.ny || nj < 0 || nk >= a.nz || nk < 0) return false;
        r.ci = ni; r.cj = nj; r.ck = nk;
        r.rho0 = a.rho[(size_t)dev(a, ni, nj, nk) * a.ncomp];  // the next step's density, requested now
        r.x = ex ? xE : r.x + r.dx * ds;
        r.y = ey ? yE : r.y + r.dy * ds;
        r.z = ez ? zE : r.z + r.dz * ds;
        return true;
    }

    __device__ static __forceinline__ int whichcell(const Args& a, const Shared& sh, double x, double y, double z) {
        const double* xv = sh.mesh;
        const double* yv = xv + a.nx + 1;
        const double* zv = yv + a.ny + 1;
        const int i = locateFail(xv, a.nx + 1, x), j = locateFail(yv, a.ny + 1, y), k = locateFail(zv, a.nz + 1, z);
        if (i < 0 || j < 0 || k < 0) return -1;
        return dev(a, i, j, k);
    }
};

#endif  // SKIRT_AMD_DEVICE_GRID_CARTESIAN_HPP
