// The tree grids: Grid<kOctreeNodes> and Grid<kOctreeBookkeeping> (node arrays), LeafMapGrid behind
// Grid<SKIRT_GRID_OCTREE> and Grid<kBinTreeMap>, and buildLeafMapKernel, which fills the leaf map.
// Compiles only where engine.hip includes it, inside its anonymous namespace (after Args, Shared and Ray).
#ifndef SKIRT_AMD_DEVICE_GRID_TREE_HPP
#define SKIRT_AMD_DEVICE_GRID_TREE_HPP

// Octree grid walked through the node arrays: TreeDustGrid.cpp:390-521 (TopDown and Neighbor
// search), DustGridPath::moveInside. Used for trees the leaf map cannot hold, and by the leaf-map
// walk below for the rare steps whose exit point lies on a cell face.
template <>
struct Grid<kOctreeNodes> {
    __device__ static __forceinline__ void loadBox(const Args& a, int l, double& x0, double& y0, double& z0,
                                                   double& x1, double& y1, double& z1) {
        const double2* b = reinterpret_cast<const double2*>(a.box + 6 * (size_t)l);
        const double2 p = b[0], q = b[1], w = b[2];
        x0 = p.x; y0 = p.y; z0 = q.x; x1 = q.y; y1 = w.x; z1 = w.y;
    }

    // TreeNode::whichnode from the root + OctTreeNode::child(r) / BinTreeNode::child(r)
    // (BinTreeNode.cpp:322-331): the leaf containing (x,y,z) or -1
    __device__ static __forceinline__ int descend(const Args& a, double x, double y, double z) {
        if (!(x >= a.gx0 && x <= a.gx1 && y >= a.gy0 && y <= a.gy1 && z >= a.gz0 && z <= a.gz1)) return -1;
        int l = 0;
        int c0 = a.firstChild[0];
        while (c0 >= 0) {
            const double* cb = a.box + 6 * (size_t)c0 + 3;  // split point = rmax of child 0
            if (a.splitDir) {
                const int d = a.splitDir[l];
                l = c0 + ((d == 0 ? x : d == 1 ? y : z) < cb[d] ? 0 : 1);
            } else {
                l = c0 + (x < cb[0] ? 0 : 1) + (y < cb[1] ? 0 : 2) + (z < cb[2] ? 0 : 4);
            }
            c0 = a.firstChild[l];
        }
        return l;
    }

    // the part of the path before the grid (TreeDustGrid.cpp:404-440): up to three segments outside the
    // grid; on return (x,y,z) is the entry point. False for an empty path.
    __device__ static __forceinline__ bool enterGrid(const Args& a, double& rx, double& ry, double& rz, double kx,
                                                     double ky, double kz, double (&d)[3]) {
        const double eps = a.eps;
        d[0] = d[1] = d[2] = 0;
        if (rx <= a.gx0) {
            if (kx <= 0.0) return false;
            d[0] = (a.gx0 - rx) / kx; rx = a.gx0 + eps; ry += ky * d[0]; rz += kz * d[0];
        } else if (rx >= a.gx1) {
            if (kx >= 0.0) return false;
            d[0] = (a.gx1 - rx) / kx; rx = a.gx1 - eps; ry += ky * d[0]; rz += kz * d[0];
        }
        if (ry <= a.gy0) {
            if (ky <= 0.0) return false;
            d[1] = (a.gy0 - ry) / ky; rx += kx * d[1]; ry = a.gy0 + eps; rz += kz * d[1];
        } else if (ry >= a.gy1) {
            if (ky >= 0.0) return false;
            d[1] = (a.gy1 - ry) / ky; rx += kx * d[1]; ry = a.gy1 - eps; rz += kz * d[1];
        }
        if (rz <= a.gz0) {
            if (kz <= 0.0) return false;
            d[2] = (a.gz0 - rz) / kz; rx += kx * d[2]; ry += ky * d[2]; rz = a.gz0 + eps;
        } else if (rz >= a.gz1) {
            if (kz >= 0.0) return false;
            d[2] = (a.gz1 - rz) / kz; rx += kx * d[2]; ry += ky * d[2]; rz = a.gz1 - eps;
        }
        return true;
    }

    template <class SegFn>
    __device__ static __forceinline__ bool begin(const Args& a, const Shared&, Ray& r, SegFn seg) {
        double rx = r.x, ry = r.y, rz = r.z, d[3];
        if (!enterGrid(a, rx, ry, rz, r.dx, r.dy, r.dz, d)) return false;
        const int node = descend(a, rx, ry, rz);
        if (node < 0) return false;
        for (int q = 0; q < 3; q++)
            if (d[q] > 0) seg(-1, 0.0, d[q]);
        r.x = rx; r.y = ry; r.z = rz;
        r.ci = node;
        r.cj = a.cellnumber[node];
        loadBox(a, node, r.bx0, r.by0, r.bz0, r.bx1, r.by1, r.bz1);
        return true;
    }

    // the node after `node` for a ray leaving it through `wall` at (x,y,z) (already advanced by
    // ds + eps): TreeNode::whichnode(wall, r) over the sorted neighbour list, else the descent from the
    // root, with the reference's nextafter escape when the point has not left the node. May move
    // (x,y,z). Returns -1 when the path leaves the grid.
    __device__ static __forceinline__ int nextNode(const Args& a, int node, int wall, double& x, double& y, double& z,
                                                   double kx, double ky, double kz) {
        if (a.search == SKIRT_TREE_NEIGHBOR) {
            const int q = 6 * node + wall;
            const int nb = a.nbrOffset[q], ne = a.nbrOffset[q + 1];
            for (int n = nb; n < ne; n++) {
                const int c = a.nbrList[n];
                double x0, y0, z0, x1, y1, z1;
                loadBox(a, c, x0, y0, z0, x1, y1, z1);
                if (x >= x0 && x <= x1 && y >= y0 && y <= y1 && z >= z0 && z <= z1) return c;
            }
        }
        int next = descend(a, x, y, z);
        if (next == node) {
            // stuck: advance to the next representable coordinates (TreeDustGrid.cpp:502-519)
            x = nextafter(x, (kx < 0.0) ? -kDblMax : kDblMax);
            y = nextafter(y, (ky < 0.0) ? -kDblMax : kDblMax);
            z = nextafter(z, (kz < 0.0) ? -kDblMax : kDblMax);
            next = descend(a, x, y, z);
            if (next == node) return -1;
        }
        return next;
    }

    template <class SegFn>
    __device__ static __forceinline__ bool step(const Args& a, const Shared&, Ray& r, SegFn seg) {
        const int node = r.ci;
        const double xnext = (r.dx < 0.0) ? r.bx0 : r.bx1;
        const double ynext = (r.dy < 0.0) ? r.by0 : r.by1;
        const double znext = (r.dz < 0.0) ? r.bz0 : r.bz1;
        const double dsx = (r.ix != 0.0) ? (xnext - r.x) * r.ix : kDblMax;
        const double dsy = (r.iy != 0.0) ? (ynext - r.y) * r.iy : kDblMax;
        const double dsz = (r.iz != 0.0) ? (znext - r.z) * r.iz : kDblMax;
        double ds;
        int wall;
        if (dsx <= dsy && dsx <= dsz) { ds = dsx; wall = (r.dx < 0.0) ? 0 : 1; }
        else if (dsy <= dsx && dsy <= dsz) { ds = dsy; wall = (r.dy < 0.0) ? 2 : 3; }
        else { ds = dsz; wall = (r.dz < 0.0) ? 4 : 5; }
        if (!seg(r.cj, a.rho[(size_t)r.cj * a.ncomp], ds)) return false;
        double x = r.x + (ds + a.eps) * r.dx;
        double y = r.y + (ds + a.eps) * r.dy;
        double z = r.z + (ds + a.eps) * r.dz;
        const int next = nextNode(a, node, wall, x, y, z, r.dx, r.dy, r.dz);
        if (next < 0) return false;
        loadBox(a, next, r.bx0, r.by0, r.bz0, r.bx1, r.by1, r.bz1);
        r.x = x; r.y = y; r.z = z;
        r.ci = next;
        r.cj = a.cellnumber[next];
        return true;
    }


    __device__ static __forceinline__ int whichcell(const Args& a, const Shared&, double x, double y, double z) {
        const int l = descend(a, x, y, z);
        return l < 0 ? -1 : a.cellnumber[l];
    }
};

// Octree grid, Bookkeeping search (TreeDustGrid.cpp:523-659): the next node follows from the breadth-first
// numbering (the 8 children of a node are consecutive ids in octant order, so (l-1) % 8 is the octant of
// node l): climb while the node lies on the far side of its father, step to the sibling across the wall,
// descend with "<=" to the leaf holding the exit point. The position is put on the crossed wall exactly
// (no eps). Entry into the grid as for the other searches.
template <>
struct Grid<kOctreeBookkeeping> {
    using Nodes = Grid<kOctreeNodes>;

    template <class SegFn>
    __device__ static __forceinline__ bool begin(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        return Nodes::begin(a, sh, r, seg);
    }
    __device__ static __forceinline__ int whichcell(const Args& a, const Shared& sh, double x, double y, double z) {
        return Nodes::whichcell(a, sh, x, y, z);
    }

    __device__ static __forceinline__ const double* childBox(const Args& a, int l) {
        return a.box + 6 * (size_t)a.firstChild[l];
    }

    template <class SegFn>
    __device__ static __forceinline__ bool step(const Args& a, const Shared&, Ray& r, SegFn seg) {
        const double xnext = (r.dx < 0.0) ? r.bx0 : r.bx1;
        const double ynext = (r.dy < 0.0) ? r.by0 : r.by1;
        const double znext = (r.dz < 0.0) ? r.bz0 : r.bz1;
        const double dsx = (r.ix != 0.0) ? (xnext - r.x) * r.ix : kDblMax;
        const double dsy = (r.iy != 0.0) ? (ynext - r.y) * r.iy : kDblMax;
        const double dsz = (r.iz != 0.0) ? (znext - r.z) * r.iz : kDblMax;
        int l = r.ci;
        if (dsx <= dsy && dsx <= dsz) {
            if (!seg(r.cj, a.rho[(size_t)r.cj * a.ncomp], dsx)) return false;
            r.x = xnext; r.y += r.dy * dsx; r.z += r.dz * dsx;
            while ((r.dx < 0.0) ? (((l - 1) & 1) == 0) : (((l - 1) & 1) == 1)) {
                l = a.father[l];
                if (l == 0) return false;
            }
            l += (r.dx < 0.0) ? -1 : 1;
            while (a.cellnumber[l] < 0) {
                const double* cb = childBox(a, l);
                const int k = (r.dx < 0.0 ? 1 : 0) + (r.y <= cb[4] ? 0 : 2) + (r.z <= cb[5] ? 0 : 4);
                l = a.firstChild[l] + k;
            }
        } else if (dsy < dsx && dsy <= dsz) {
            if (!seg(r.cj, a.rho[(size_t)r.cj * a.ncomp], dsy)) return false;
            r.x += r.dx * dsy; r.y = ynext; r.z += r.dz * dsy;
            while ((r.dy < 0.0) ? (((l - 1) & 2) == 0) : (((l - 1) & 2) != 0)) {
                l = a.father[l];
                if (l == 0) return false;
            }
            l += (r.dy < 0.0) ? -2 : 2;
            while (a.cellnumber[l] < 0) {
                const double* cb = childBox(a, l);
                const int k = (r.x <= cb[3] ? 0 : 1) + (r.dy < 0.0 ? 2 : 0) + (r.z <= cb[5] ? 0 : 4);
                l = a.firstChild[l] + k;
            }
        } else if (dsz < dsx && dsz < dsy) {
            if (!seg(r.cj, a.rho[(size_t)r.cj * a.ncomp], dsz)) return false;
            r.x += r.dx * dsz; r.y += r.dy * dsz; r.z = znext;
            while ((r.dz < 0.0) ? (((l - 1) & 4) == 0) : (((l - 1) & 4) != 0)) {
                l = a.father[l];
                if (l == 0) return false;
            }
            l += (r.dz < 0.0) ? -4 : 4;
            while (a.cellnumber[l] < 0) {
                const double* cb = childBox(a, l);
                const int k = (r.x <= cb[3] ? 0 : 1) + (r.y <= cb[4] ? 0 : 2) + (r.dz < 0.0 ? 4 : 0);
                l = a.firstChild[l] + k;
            }
        } else {
            return false;  // NaN distances
        }
        r.ci = l;
        r.cj = a.cellnumber[l];
        Nodes::loadBox(a, l, r.bx0, r.by0, r.bz0, r.bx1, r.by1, r.bz1);
        return true;
    }
};

// Octree grid through the leaf map. An octree split at box centres (OctTreeNode::createchildren,
// OctTreeNode.cpp:53-56, Box::center) has, per axis, one table of 2^L + 1 split coordinates T (L the
// deepest level) such that a level-l node with integer coordinate i spans [T[i << (L-l)],
// T[(i+1) << (L-l)]] -- bit for bit, since every split is 0.5*(lo+hi) of two table entries. So:
//   - the box faces come from the T tables in LDS (no box gather);
//   - the leaf containing a point is the leaf map entry of the finest-level cell holding it: one
//     16-byte load instead of the neighbour-list walk. Locating by "T[j] <= x < T[j+1]" is exactly
//     the reference's root descent (x < split -> lower child), so the only steps where it can differ
//     from the inclusive-box neighbour search (TreeNode::whichnode(wall, r)) are those whose exit point
//     lies exactly on a lower face of the leaf found, or that have not left the current leaf; those
//     take the node-array search above. The walk is therefore the reference's, step for step.
// The host builds the map only after checking every node box against the T tables.
// A k-d tree (BinTreeNode::createchildren_splitdir also halves at the centre, one axis at a time) maps
// the same way with per-axis leaf extents (BIN): its entries carry the three shifts instead of a level.
template <bool BIN>
struct LeafMapGrid {
    using Nodes = Grid<kOctreeNodes>;

    // a leaf's extent along x, y, z in finest cells, as shifts
    __device__ static __forceinline__ void shifts(const Args& a, unsigned cl, int& sx, int& sy, int& sz) {
        if (BIN) {
            const unsigned s = cl >> kBinCellBits;
            sx = (int)(s & 7u); sy = (int)((s >> 3) & 7u); sz = (int)((s >> 6) & 7u);
        } else {
            sx = sy = sz = a.mapL - (int)(cl >> kLeafLevelShift);
        }
    }
    __device__ static __forceinline__ int cellOf(unsigned cl) { return (int)(cl & (BIN ? kBinCellMask : kLeafCellMask)); }

    // finest-level index j with T[j] <= v < T[j+1] (the last cell also holds v == T[N]); v in [T[0], T[N]].
    // The split coordinates are uniform to rounding, so the estimate is off by one at most near a
    // split; the loops only run for that rare lane.
    __device__ static __forceinline__ int estimate(int N, double t0, double inv, double v) {
        return max(0, min(N - 1, (int)((v - t0) * inv)));
    }
    __device__ static __forceinline__ int correct(const double* T, int N, int j, double v) {
        const double lo = T[j], hi = T[j + 1];
        if (v < lo) {
            do j--; while (j > 0 && v < T[j]);
            j = max(j, 0);  // v below T[0]: a point outside the grid, whose entry is fetched but not used
        } else if (v >= hi && j < N - 1) {
            do j++; while (j < N - 1 && v >= T[j + 1]);
        }
        return j;
    }

    __device__ static __forceinline__ bool inside(const Args& a, double x, double y, double z) {
        return x >= a.gx0 && x <= a.gx1 && y >= a.gy0 && y <= a.gy1 && z >= a.gz0 && z <= a.gz1;
    }

    // issues the load of the leaf map entry of the point (clamped into the grid, so any point -- even
    // NaN -- reads a valid entry); fx, fy, fz its finest-level indices. The entry of the estimated cell
    // is requested before the estimate is checked against the T tables in LDS; the rare lane whose
    // estimate was off by one requests the right entry again.
    __device__ static __forceinline__ int4 fetch(const Args& a, const Shared& sh, double x, double y, double z,
                                                 int& fx, int& fy, int& fz) {
        const int N = a.mapN;
        const double* tx = sh.mesh;
        const int ex = estimate(N, a.mapX0, a.mapInvX, x);
        const int ey = estimate(N, a.mapY0, a.mapInvY, y);
        const int ez = estimate(N, a.mapZ0, a.mapInvZ, z);
        int4 v = *reinterpret_cast<const int4*>(a.leafMap + leafIndex(N, ex, ey, ez));
        fx = correct(tx, N, ex, x);
        fy = correct(tx + (N + 1), N, ey, y);
        fz = correct(tx + 2 * (N + 1), N, ez, z);
        if (fx != ex || fy != ey || fz != ez) v = *reinterpret_cast<const int4*>(a.leafMap + leafIndex(N, fx, fy, fz));
        return v;
    }

    __device__ static __forceinline__ LeafEntry decode(int4 v) {
        // one 16-byte load: keep the compiler from splitting off the density into a later second load
        asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
        LeafEntry e;
        e.node = v.x;
        e.cl = (unsigned)v.y;
        const long long bits = ((long long)(unsigned)v.w << 32) | (unsigned)v.z;
        e.rho0 = __longlong_as_double(bits);
        return e;
    }

    // leaf map entry of the point (inside the grid); fx, fy, fz its finest-level indices
    __device__ static __forceinline__ LeafEntry lookup(const Args& a, const Shared& sh, double x, double y, double z,
                                                       int& fx, int& fy, int& fz) {
        return decode(fetch(a, sh, x, y, z, fx, fy, fz));
    }

    // r.ck: the leaf's size in finest cells (octree) or its packed shifts (k-d tree); r.bx0, r.by0,
    // r.bz0: the leaf's faces the ray leaves through along x, y, z (read from the T tables once, when
    // the leaf is entered, so the next step starts without an LDS round trip)
    __device__ static __forceinline__ void enterPlanes(Ray& r, int jx, int jy, int jz, const LeafEntry& e,
                                                       double lox, double loy, double loz,
                                                       double hix, double hiy, double hiz) {
        r.ci = e.node;
        r.cj = cellOf(e.cl);
        if (BIN) r.ck = (int)(e.cl >> kBinCellBits);
        r.jx = jx; r.jy = jy; r.jz = jz;
        r.rho0 = e.rho0;
        r.bx0 = (r.dx < 0.0) ? lox : hix;
        r.by0 = (r.dy < 0.0) ? loy : hiy;
        r.bz0 = (r.dz < 0.0) ? loz : hiz;
    }
    __device__ static __forceinline__ void enter(const Args& a, const Shared& sh, Ray& r, int fx, int fy, int fz,
                                                 const LeafEntry& e) {
        const int N1 = a.mapN + 1;
        const double* tx = sh.mesh;
        int sx, sy, sz;
        shifts(a, e.cl, sx, sy, sz);
        const int jx = (fx >> sx) << sx, jy = (fy >> sy) << sy, jz = (fz >> sz) << sz;
        enterPlanes(r, jx, jy, jz, e, tx[jx], tx[N1 + jy], tx[2 * N1 + jz], tx[jx + (1 << sx)],
                    tx[N1 + jy + (1 << sy)], tx[2 * N1 + jz + (1 << sz)]);
        if (!BIN) r.ck = 1 << sx;
    }

    template <class SegFn>
    __device__ static __forceinline__ bool begin(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        double rx = r.x, ry = r.y, rz = r.z, d[3];
        if (!Nodes::enterGrid(a, rx, ry, rz, r.dx, r.dy, r.dz, d)) return false;
        if (!inside(a, rx, ry, rz)) return false;  // the root descent finds no node
        for (int q = 0; q < 3; q++)
            if (d[q] > 0) seg(-1, 0.0, d[q]);
        int fx, fy, fz;
        const LeafEntry e = lookup(a, sh, rx, ry, rz, fx, fy, fz);
        r.x = rx; r.y = ry; r.z = rz;
        enter(a, sh, r, fx, fy, fz, e);
        prefetch(a, r);
        return true;
    }

    // the exit of the current leaf: the distance to the nearest of its three faces ahead of the ray, the wall
    // (the reference's order of comparisons) and the exit point nudged by eps
    __device__ static __forceinline__ void exitPoint(const Args& a, const Ray& r, double& ds, int& wall, double& x,
                                                     double& y, double& z) {
        const double xnext = r.bx0, ynext = r.by0, znext = r.bz0;
        const double dsx = (r.ix != 0.0) ? (xnext - r.x) * r.ix : kDblMax;
        const double dsy = (r.iy != 0.0) ? (ynext - r.y) * r.iy : kDblMax;
        const double dsz = (r.iz != 0.0) ? (znext - r.z) * r.iz : kDblMax;
        if (dsx <= dsy && dsx <= dsz) { ds = dsx; wall = (r.dx < 0.0) ? 0 : 1; }
        else if (dsy <= dsx && dsy <= dsz) { ds = dsy; wall = (r.dy < 0.0) ? 2 : 3; }
        else { ds = dsz; wall = (r.dz < 0.0) ? 4 : 5; }
        x = r.x + (ds + a.eps) * r.dx;
        y = r.y + (ds + a.eps) * r.dy;
        z = r.z + (ds + a.eps) * r.dz;
    }

    // requests the leaf-map entry of the estimated finest cell of the next exit point: issued at the end of a
    // step, before the wave's Labs drain, it is in flight during the drain and the next step's segment. A load
    // waits for every older vector-memory operation of its wave (vmcnt counts in issue order, atomics
    // included, and a no-return f64 atomic stays counted for thousands of cycles under load): requested
    // after the drain, each step's entry would wait for the previous step's Labs atomic too.
    __device__ static __forceinline__ void prefetch(const Args& a, Ray& r) {
        exitPoint(a, r, r.eds, r.ewall, r.ex, r.ey, r.ez);  // (kept for the step: the ray does not move before it)
        const int N = a.mapN;
        r.pfx = estimate(N, a.mapX0, a.mapInvX, r.ex);
        r.pfy = estimate(N, a.mapY0, a.mapInvY, r.ey);
        r.pfz = estimate(N, a.mapZ0, a.mapInvZ, r.ez);
        r.pre = *reinterpret_cast<const int4*>(a.leafMap + leafIndex(N, r.pfx, r.pfy, r.pfz));
    }

    template <class SegFn>
    __device__ static __forceinline__ bool step(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        const int N1 = a.mapN + 1;
        const double* tx = sh.mesh;
        const double* ty = tx + N1;
        const double* tz = ty + N1;
        // the exit point prefetch computed at the end of the last step (or at the grid entry): 139 -> 129 VGPRs,
        // C3 within the spread, C5 +0.5 % (profiles/r05_exit_reuse_ab.txt)
        const double ds = r.eds;
        double x = r.ex, y = r.ey, z = r.ez;
        const int wall = r.ewall;
        // the next leaf's entry is requested first; the segment's own work (optical depth, absorption)
        // runs while the load is in flight
        // the entry of the estimated finest cell; its leaf is the right one when the leaf's own faces
        // (read anyway) contain the point, since T is monotone: then the exact finest cell lies in it too
        const int N = a.mapN;
        // requested by the previous step (prefetch), for the same exit point computed the same way
        int fx = r.pfx, fy = r.pfy, fz = r.pfz;
        const int4 raw = r.pre;
        if (!seg(r.cj, r.rho0, ds)) return false;
        if (!inside(a, x, y, z)) return false;  // no neighbour and no root descent contains it
        LeafEntry e = decode(raw);
        int lx, ly, lz;
        shifts(a, e.cl, lx, ly, lz);
        int jx = (fx >> lx) << lx, jy = (fy >> ly) << ly, jz = (fz >> lz) << lz;
        // the new leaf's six faces in one LDS round trip: the lower ones decide whether the exit point
        // lies on a face, the ones ahead of the ray are the next step's exit planes
        double lox = tx[jx], loy = ty[jy], loz = tz[jz];
        double hix = tx[jx + (1 << lx)], hiy = ty[jy + (1 << ly)], hiz = tz[jz + (1 << lz)];
        if (!(x >= lox && x < hix && y >= loy && y < hiy && z >= loz && z < hiz)) {
            // the estimate fell into a neighbouring leaf (or the point is on the grid's far faces): the
            // exact finest cell, its entry and its leaf's faces
            fx = correct(tx, N, fx, x);
            fy = correct(ty, N, fy, y);
            fz = correct(tz, N, fz, z);
            e = decode(*reinterpret_cast<const int4*>(a.leafMap + leafIndex(N, fx, fy, fz)));
            shifts(a, e.cl, lx, ly, lz);
            jx = (fx >> lx) << lx; jy = (fy >> ly) << ly; jz = (fz >> lz) << lz;
            lox = tx[jx]; loy = ty[jy]; loz = tz[jz];
            hix = tx[jx + (1 << lx)]; hiy = ty[jy + (1 << ly)]; hiz = tz[jz + (1 << lz)];
        }
        r.x = x; r.y = y; r.z = z;
        if (e.node == r.ci || x == lox || y == loy || z == loz) {
            // on a face, or not out of the current leaf: the reference's own search decides
            const int next = Nodes::nextNode(a, r.ci, wall, x, y, z, r.dx, r.dy, r.dz);
            if (next < 0) return false;
            const double* b = a.box + 6 * (size_t)next;  // its lower corner is a finest cell of it
            e = lookup(a, sh, b[0], b[1], b[2], fx, fy, fz);
            enter(a, sh, r, fx, fy, fz, e);
            prefetch(a, r);
            return true;
        }
        enterPlanes(r, jx, jy, jz, e, lox, loy, loz, hix, hiy, hiz);
        if (!BIN) r.ck = 1 << lx;
        prefetch(a, r);
        return true;
    }

    __device__ static __forceinline__ int whichcell(const Args& a, const Shared& sh, double x, double y, double z) {
        if (!inside(a, x, y, z)) return -1;
        int fx, fy, fz;
        return cellOf(lookup(a, sh, x, y, z, fx, fy, fz).cl);
    }
};

template <>
struct Grid<SKIRT_GRID_OCTREE> : LeafMapGrid<false> {};
template <>
struct Grid<kBinTreeMap> : LeafMapGrid<true> {};

// fills the leaf map: one thread per finest-level cell descends the (checked) tree by its index bits
// (a k-d tree by the bit of its split axis at that axis' depth)
__global__ void __launch_bounds__(kBlock) buildLeafMapKernel(LeafEntry* map, const int* firstChild, const signed char* splitDir,
                                                             const int* cellnumber, const double* rho, int ncomp, int L) {
    const int N = 1 << L;
    const unsigned long long n = leafMapSize(N);
    for (unsigned long long q = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; q < n;
         q += (unsigned long long)gridDim.x * blockDim.x) {
        unsigned fx = 0, fy = 0, fz = 0;
        {  // inverse of leafIndex
            const unsigned long long nb = leafBricks(N), br = q >> 3;
            fx = (unsigned)(2 * (br / (nb * nb)) + ((q >> 2) & 1u));
            fy = (unsigned)(2 * ((br / nb) % nb) + ((q >> 1) & 1u));
            fz = (unsigned)(2 * (br % nb) + (q & 1u));
            fx = min(fx, (unsigned)N - 1u); fy = min(fy, (unsigned)N - 1u); fz = min(fz, (unsigned)N - 1u);
        }
        int node = 0, level = 0;
        LeafEntry e;
        if (splitDir) {
            int lv[3] = {0, 0, 0};
            const unsigned f[3] = {fx, fy, fz};
            while (firstChild[node] >= 0) {
                const int d = splitDir[node];
                const int bit = L - 1 - lv[d];
                lv[d]++;
                node = firstChild[node] + (int)((f[d] >> bit) & 1u);
            }
            e.cl = (unsigned)cellnumber[node] |
                   ((unsigned)(L - lv[0]) | (unsigned)(L - lv[1]) << 3 | (unsigned)(L - lv[2]) << 6) << kBinCellBits;
        } else {
            while (firstChild[node] >= 0) {
                const int bit = L - 1 - level;
                node = firstChild[node] + (int)((fx >> bit) & 1u) + 2 * (int)((fy >> bit) & 1u) + 4 * (int)((fz >> bit) & 1u);
                level++;
            }
            e.cl = (unsigned)cellnumber[node] | ((unsigned)level << kLeafLevelShift);
        }
        const int cell = cellnumber[node];
        e.node = node;
        e.rho0 = rho[(size_t)cell * ncomp];
        map[q] = e;
    }
}

#endif  // SKIRT_AMD_DEVICE_GRID_TREE_HPP
