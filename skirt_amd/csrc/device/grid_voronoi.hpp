// Grid<SKIRT_GRID_VORONOI>: the walk through a Voronoi dust grid and its cellIndex.
// Compiles only where engine.hip includes it, inside its anonymous namespace, after grid_tree.hpp (the box
// entry of Grid<kOctreeNodes>::enterGrid).
#ifndef SKIRT_AMD_DEVICE_GRID_VORONOI_HPP
#define SKIRT_AMD_DEVICE_GRID_VORONOI_HPP

// Voronoi grid: VoronoiMesh::path (VoronoiMesh.cpp:749-844), cellIndex (:512-541), with the
// reference's arithmetic order (bisector plane through the midpoint, Vec::dot left to right)
template <>
struct Grid<SKIRT_GRID_VORONOI> {
    __device__ static __forceinline__ bool inside(const Args& a, double x, double y, double z) {
        return x >= a.gx0 && x <= a.gx1 && y >= a.gy0 && y <= a.gy1 && z >= a.gz0 && z <= a.gz1;
    }

    // the cell whose site is nearest, over the cells listed for the point's block (Box::cellindices)
    __device__ static __forceinline__ int cellIndex(const Args& a, double x, double y, double z) {
        if (!inside(a, x, y, z)) return -1;
        const int nb = a.vnb;
        const int i = max(0, min(nb - 1, static_cast<int>(nb * (x - a.gx0) / (a.gx1 - a.gx0))));
        const int j = max(0, min(nb - 1, static_cast<int>(nb * (y - a.gy0) / (a.gy1 - a.gy0))));
        const int k = max(0, min(nb - 1, static_cast<int>(nb * (z - a.gz0) / (a.gz1 - a.gz0))));
        const int b = i * nb * nb + j * nb + k;
        int m = -1;
        double best = kDblMax;
        // the list in groups of kCellIndexGroup candidates, each {site, cell} in one 32-byte record, a group's
        // records loaded together (one round trip per group); the candidates are then taken in list order, so
        // the first of equal distances wins as in the reference's loop
        constexpr int G = kCellIndexGroup;
        const int qe = a.blockOffset[b + 1];
        for (int q0 = a.blockOffset[b]; q0 < qe; q0 += G) {
            int c[G];
            double sx[G], sy[G], sz[G];
#pragma unroll
            for (int u = 0; u < G; u++) {
                c[u] = -1;
                sx[u] = sy[u] = sz[u] = 0.0;
                if (q0 + u < qe) {
                    const double2* rec = reinterpret_cast<const double2*>(a.blockSites + q0 + u);
                    const double2 r0 = rec[0], r1 = rec[1];
                    sx[u] = r0.x; sy[u] = r0.y; sz[u] = r1.x;
                    c[u] = (int)(unsigned)__double_as_longlong(r1.y);  // the id, in the low word
                }
            }
#pragma unroll
            for (int u = 0; u < G; u++) {
                const double dx = x - sx[u], dy = y - sy[u], dz = z - sz[u];
                const double d = dx * dx + dy * dy + dz * dz;
                if (c[u] >= 0 && d < best) { best = d; m = c[u]; }
            }
        }
        return m;
    }

    template <class SegFn>
    __device__ static __forceinline__ bool begin(const Args& a, const Shared&, Ray& r, SegFn seg) {
        int none = kNoCell;
        return beginAt(a, r, none, seg);
    }

    // begin() with the cell of the ray's origin cached in `cell` (kNoCell: not known yet). A point strictly
    // inside the grid enters where it is, whatever the direction (enterGrid moves nothing), so its cellIndex
    // serves every ray from that position: the peel-offs and the FILL ray of one event, and the WALK ray
    // that retraces the FILL ray's path in the next one. A point on or outside the grid's faces enters
    // where its direction takes it, so it is located per ray and not cached.
    template <class SegFn>
    __device__ static __forceinline__ bool beginAt(const Args& a, Ray& r, int& cell, SegFn seg) {
        double rx = r.x, ry = r.y, rz = r.z, d[3];
        const bool strict = rx > a.gx0 && rx < a.gx1 && ry > a.gy0 && ry < a.gy1 && rz > a.gz0 && rz < a.gz1;
        if (!Grid<kOctreeNodes>::enterGrid(a, rx, ry, rz, r.dx, r.dy, r.dz, d)) return false;
        int m;
        if (strict && cell != kNoCell) m = cell;
        else {
            m = cellIndex(a, rx, ry, rz);
            if (strict) cell = m;
        }
        if (m < 0) return false;
        for (int q = 0; q < 3; q++)
            if (d[q] > 0) seg(-1, 0.0, d[q]);
        r.x = rx; r.y = ry; r.z = rz;
        r.ci = m;
        r.cj = a.vorStart[m];
        r.ck = 0;
        return true;
    }

    __device__ static __forceinline__ double wallDist(const Args& a, const Ray& r, int w) {
        switch (w) {
        case -1: return (a.gx0 - r.x) / r.dx;
        case -2: return (a.gx1 - r.x) / r.dx;
        case -3: return (a.gy0 - r.y) / r.dy;
        case -4: return (a.gy1 - r.y) / r.dy;
        case -5: return (a.gz0 - r.z) / r.dz;
        default: return (a.gz1 - r.z) / r.dz;
        }
    }

    // the reference's distance along the ray to the bisector plane of sites pr (the current cell) and pi
    // (a neighbour), 0 when the ray moves away from it -- VoronoiMesh.cpp:790-806, same operation order
    __device__ static __forceinline__ double planeDist(const Ray& r, double prx, double pry, double prz, double pix,
                                                       double piy, double piz) {
        const double nx = pix - prx, ny = piy - pry, nz = piz - prz;
        const double ndotk = nx * r.dx + ny * r.dy + nz * r.dz;
        if (!(ndotk > 0)) return 0;
        const double px = 0.5 * (pix + prx), py = 0.5 * (piy + pry), pz = 0.5 * (piz + prz);
        return (nx * (px - r.x) + ny * (py - r.y) + nz * (pz - r.z)) / ndotk;
    }

    __device__ static __forceinline__ void siteAt(const Args& a, int start, double& x, double& y, double& z) {
        const double2 h0 = *reinterpret_cast<const double2*>(a.vorSlots + start);
        const double2 h1 = *reinterpret_cast<const double2*>(a.vorSlots + start + 1);
        x = h0.x; y = h0.y; z = h1.x;
    }

    // the operands of a step: the cell's header (exact site, density, id, neighbour count) and, for the
    // bounds, the float offset D of the site from the ray's position and the direction in float
    struct StepIn {
        const VorEntry* B;
        double pwx, pwy, pwz, rhow;
        int idw, cnt;
        float Dx, Dy, Dz, fkx, fky, fkz;
        float eA, eA2, eB2;  // the cell's error terms: eA, 2 eA, 2 (eA |D|_1 + kVorEpsF max |n|^2)
    };
    // U: the least upper bound of the certain exits; L1 <= L2: the two least lower bounds of the possible
    // exits, w1: the first one's `next`
    struct Best {
        float U, L1, L2;
        int w1;
    };

    // the bounds [lo, hi] of one neighbour's plane distance, in single precision on coordinates scaled by
    // a.vorScale (the entries' offsets are stored scaled): each float operation adds a few 2^-24 of the sum
    // of absolute terms, which kVorEpsF covers with margin; an approximate reciprocal (1 ulp) is covered by
    // the |s| term. Walls are stored as the bisector plane with the site's mirror image (the same plane),
    // so every entry takes the same branch-free arithmetic; lo = hi = FLT_MAX: certainly no exit.
    __device__ static __forceinline__ void bounds(const StepIn& s, const VorEntry& en, bool valid, float& lo,
                                                  float& ucand) {
        // the plane distance s = (n.D + |n|^2/2) / (n.k) = (m.D + 1/2) / (m.k) with m = n / |n|^2, the stored
        // entry, and Cauchy-Schwarz error terms: |d(m.k)| <= eA and |d(m.D + 1/2)| <= eB = eA |D|_1 + kVorEpsF/2,
        // at the cell's largest |m|_1 (vor_terms.hpp; several times the float roundings of the entries, D, k
        // and the fused operations). 29 operations per entry (with n stored: 33; per-entry terms: 38; round
        // 2's sums of the absolute terms of each product: 55); tools/vor_compact_check.cpp, mode r, checks
        // the resulting steps against the reference's.
        const float mx = en.ox, my = en.oy, mz = en.oz;  // m = n / |n|^2 (vor_terms.hpp)
        const float den = fmaf(mz, s.fkz, fmaf(my, s.fky, mx * s.fkx));
        const float num = fmaf(mz, s.Dz, fmaf(my, s.Dy, fmaf(mx, s.Dx, 0.5f)));
        const float inv = __builtin_amdgcn_rcpf(den);
        const float sa = num * inv;
        const float err = fmaf(fmaf(fabsf(sa), s.eA2, s.eB2), inv, fabsf(sa) * kVorEpsF);
        // den > 2 eA: the sign of n.k and the interval [sa - err, sa + err] are certain; den <= -eA: moving away for certain; otherwise (den = 0 included: m = 0 is a
        // degenerate wall) the sign is uncertain: lo = -FLT_MAX. Entries past the count (`valid`), and the
        // NaN padding after a cell's list (den NaN, so neither sure nor maybe): no exit. ucand: the upper
        // bound of a certain exit (lo > 0), else FLT_MAX. Selected as floats, no bool temporaries.
        const float lov = sa - err, hiv = sa + err;
        const bool sure = valid && den > s.eA2;
        const bool maybe = valid && den > -s.eA;
        // (a sure interval wholly behind the ray, hiv <= 0, stays a possible exit, which the exact evaluation
        // would drop: inside the cell no plane the ray moves towards lies behind it, so this happens at
        // rounding level only -- tools/vor_compact_check.cpp, mode r: the same 297 exact re-evaluations in
        // 1,004,001 steps with and without the check; C4 +0.7 %, profiles/r05_vor_behind_ab.txt)
        lo = sure ? lov : (maybe ? -FLT_MAX : FLT_MAX);
        ucand = (sure && lov > 0.f) ? hiv : FLT_MAX;
    }

    // one entry's bounds into the running Best, in list order
    __device__ static __forceinline__ void take(Best& b, float lo, float ucand, int next) {
        b.U = fminf(b.U, ucand);
        b.w1 = lo < b.L1 ? next : b.w1;
        b.L2 = __builtin_amdgcn_fmed3f(b.L1, b.L2, lo);
        b.L1 = fminf(b.L1, lo);
    }

    // The start of a step: the cell's header h0..h2 (loaded with the first entries in the same round), the
    // pending segment (r.ck = 1: the previous cell's segment, cell r.ci, density r.rho0, site r.bx0..bz0,
    // ends on the bisector plane with this cell, whose exact site arrives with this load), and the bounds'
    // operands. False: the ray ended.
    template <class SegFn>
    __device__ static __forceinline__ bool headFrom(const Args& a, Ray& r, StepIn& s, const double2& h0, const double2& h1,
                                                    const int4& h2, SegFn seg) {
        s.pwx = h0.x; s.pwy = h0.y; s.pwz = h1.x; s.rhow = h1.y;
        s.idw = h2.x; s.cnt = h2.y;
        const float eA = __int_as_float(h2.z), eBn = __int_as_float(h2.w);  // the cell's terms (upload)
        if (r.ck) {
            const double sq = planeDist(r, r.bx0, r.by0, r.bz0, s.pwx, s.pwy, s.pwz);
            if (!seg(r.ci, r.rho0, sq)) return false;
            r.x += (sq + a.eps) * r.dx; r.y += (sq + a.eps) * r.dy; r.z += (sq + a.eps) * r.dz;
            r.ck = 0;
        }
        const float sc = a.vorScale;
        s.Dx = (float)((s.pwx - r.x) * sc); s.Dy = (float)((s.pwy - r.y) * sc); s.Dz = (float)((s.pwz - r.z) * sc);
        const float Dn = fabsf(s.Dx) + fabsf(s.Dy) + fabsf(s.Dz);  // |D|_1
        s.fkx = (float)r.dx; s.fky = (float)r.dy; s.fkz = (float)r.dz;
        s.eA = eA; s.eA2 = 2.0f * eA; s.eB2 = 2.0f * fmaf(eA, Dn, eBn);
        return true;
    }

    // The end of a step, from the bounds over all entries: a single certain exit is taken (its exact
    // distance follows from the next cell's header, r.ck = 1); otherwise the reference's rule, exactly,
    // over the possible winners.
    template <class SegFn>
    __device__ static __forceinline__ bool decide(const Args& a, Ray& r, const StepIn& s, const Best& b, SegFn seg) {
        const VorEntry* B = s.B;
        const int cnt = s.cnt;
        if (b.L1 != FLT_MAX && b.L2 > b.U) {
            if (b.w1 >= 0) {  // the exit: its exact distance when the next cell's header arrives
                r.ck = 1;
                r.ci = s.idw; r.rho0 = s.rhow;
                r.bx0 = s.pwx; r.by0 = s.pwy; r.bz0 = s.pwz;
                r.cj = b.w1;
                return true;
            }
            seg(s.idw, s.rhow, wallDist(a, r, b.w1));  // leaves the grid through a wall
            return false;
        }
        // no exit, or several possible exits. An entry whose lower bound exceeds U lies beyond a certain
        // exit, so it can neither win nor tie; a second pass over the (cached) entries collects the others
        // in list order (the first of equal distances wins) and their sites arrive in one round trip. More
        // than kVorCand of them: the whole list, in groups.
        const double kx = r.dx, ky = r.dy, kz = r.dz;
        constexpr int NO_INDEX = (int)0x80000000u;
        double sq = kDblMax;
        int mq = NO_INDEX;
        auto consider = [&](int nxt, double pix, double piy, double piz) {
            const double si = nxt < 0 ? wallDist(a, r, nxt) : planeDist(r, s.pwx, s.pwy, s.pwz, pix, piy, piz);
            if (si > 0 && si < sq) { sq = si; mq = nxt; }
        };
        if (b.L1 != FLT_MAX) {
            int c0 = 0, c1 = 0, c2 = 0, c3 = 0, nc = 0;
            VorEntry e[kVorUnroll];
            for (int q0 = 0; q0 < cnt; q0 += kVorUnroll) {
                vorEntries(B, q0, e);
#pragma unroll
                for (int u = 0; u < kVorUnroll; u++) {
                    float lo, uc;
                    bounds(s, e[u], q0 + u < cnt, lo, uc);
                    if (lo < FLT_MAX && lo <= b.U) {
                        const int nx = e[u].next;
                        c0 = nc == 0 ? nx : c0; c1 = nc == 1 ? nx : c1; c2 = nc == 2 ? nx : c2; c3 = nc == 3 ? nx : c3;
                        nc++;
                    }
                }
            }
            if (nc <= kVorCand) {
                const int cs[kVorCand] = {c0, c1, c2, c3};
                double pix[kVorCand], piy[kVorCand], piz[kVorCand];
#pragma unroll
                for (int u = 0; u < kVorCand; u++) {
                    pix[u] = piy[u] = piz[u] = 0.0;
                    if (u < nc && cs[u] >= 0) siteAt(a, cs[u], pix[u], piy[u], piz[u]);
                }
#pragma unroll
                for (int u = 0; u < kVorCand; u++)
                    if (u < nc) consider(cs[u], pix[u], piy[u], piz[u]);
            } else {
                constexpr int G = kVorFallbackGroup;
                for (int q0 = 0; q0 < cnt; q0 += G) {
                    int nxt[G];
                    double pix[G], piy[G], piz[G];
#pragma unroll
                    for (int u = 0; u < G; u++) {
                        nxt[u] = vorEntry(B, q0 + u).next;
                        pix[u] = piy[u] = piz[u] = 0.0;
                        if (q0 + u < cnt && nxt[u] >= 0) siteAt(a, nxt[u], pix[u], piy[u], piz[u]);
                    }
#pragma unroll
                    for (int u = 0; u < G; u++)
                        if (q0 + u < cnt) consider(nxt[u], pix[u], piy[u], piz[u]);
                }
            }
        }
        if (mq == NO_INDEX) {
            // no exit found: advance by eps and locate again (VoronoiMesh.cpp:831-835)
            r.x += kx * a.eps; r.y += ky * a.eps; r.z += kz * a.eps;
            const int m = cellIndex(a, r.x, r.y, r.z);
            if (m < 0) return false;
            r.ci = m;
            r.cj = a.vorStart[m];
            return true;
        }
        if (!seg(s.idw, s.rhow, sq)) return false;
        r.x += (sq + a.eps) * kx; r.y += (sq + a.eps) * ky; r.z += (sq + a.eps) * kz;
        r.cj = mq;
        return mq >= 0;
    }

    // One step (VoronoiMesh::path, VoronoiMesh.cpp:749-844), lane-serial over the cell's entries. r.cj:
    // the block of the cell the ray is in. A step issues one round of loads (this cell's header and first
    // entries) in the common case. It adds at most two segments (the pending one, and one more when the
    // bounds leave several possible winners), see kSegsPerStep.
    // the loads a step starts with: the cell's header and its first kVorGroups groups of entries (one round)
    struct Load {
        double2 h0, h1;
        int4 h2;
        VorEntry g[kVorGroups][kVorUnroll];
    };
    __device__ static __forceinline__ void stepLoad(const Args& a, const Ray& r, Load& L, bool act = true) {
        // lanes without a ray load block 0: an unconditional load needs no merge of old and new register
        // values (moves, which would wait for the loads right after their issue)
        const VorEntry* B = a.vorSlots + (act ? r.cj : 0);
        L.h0 = *reinterpret_cast<const double2*>(B);
        L.h1 = *reinterpret_cast<const double2*>(B + 1);
        L.h2 = *reinterpret_cast<const int4*>(B + 2);
#pragma unroll
        for (int gi = 0; gi < kVorGroups; gi++) vorEntries(B, gi * kVorUnroll, L.g[gi]);
    }

    template <class SegFn>
    __device__ static __forceinline__ bool step(const Args& a, const Shared& sh, Ray& r, SegFn seg) {
        Load L;
        stepLoad(a, r, L);
        return stepRest(a, sh, r, L, seg);
    }

    // the step from its loads (stepLoad): the trace kernel issues the Labs drain between the two, so the
    // header's wait does not include the drain's atomics (vmcnt counts in issue order)
    template <class SegFn>
    __device__ static __forceinline__ bool stepRest(const Args& a, const Shared&, Ray& r, Load& L, SegFn seg) {
        StepIn s;
        s.B = a.vorSlots + r.cj;
        Best b{FLT_MAX, FLT_MAX, FLT_MAX, 0};
        // kVorGroups groups of entries in flight: they load with the header, and each group's next load is
        // issued as soon as the group is consumed, so a cell with more than kVorUnroll neighbours does not
        // wait for a second round trip
        if (!headFrom(a, r, s, L.h0, L.h1, L.h2, seg)) return false;
        // (the next groups are loaded only while the list lasts: loading them unconditionally -- past the list
        // into the next block -- let the compiler drop the register moves at the join, but made C4 24 % slower,
        // 9.53e7 -> 7.37e7 pkt/s, profiles/r04_ab_c4_vor_uncond_loads_c3c5_prefetch.txt; a lane past its list
        // reading one line that all such lanes share instead: 208 -> 170 register moves, still 5 % slower,
        // profiles/r05_vor_uncond_shared_ab.txt; round 0 peeled and round 1 loaded into registers of its
        // own: 208 -> 146 moves, 245 VGPRs, C4 -0.4 %, the same file)
        constexpr int NG = kVorGroups;
        for (int q0 = 0; q0 < s.cnt; q0 += NG * kVorUnroll) {
#pragma unroll
            for (int gi = 0; gi < NG; gi++) {
                const int qb = q0 + gi * kVorUnroll;
                if (gi > 0 && qb >= s.cnt) break;
#pragma unroll
                for (int u = 0; u < kVorUnroll; u++) {
                    float lo, uc;
                    // (a cell's list is padded to whole groups with NaN entries: no count check per entry)
                    bounds(s, L.g[gi][u], true, lo, uc);
                    take(b, lo, uc, L.g[gi][u].next);
                }
                if (qb + NG * kVorUnroll < s.cnt) vorEntries(s.B, qb + NG * kVorUnroll, L.g[gi]);
            }
        }
        return decide(a, r, s, b, seg);
    }

    __device__ static __forceinline__ int whichcell(const Args& a, const Shared&, double x, double y, double z) {
        return cellIndex(a, x, y, z);
    }

    // VoronoiMesh::isPointClosestTo, over the exact sites of the cell's neighbours (their headers)
    __device__ static __forceinline__ bool closestTo(const Args& a, double x, double y, double z, int m) {
        auto d2 = [&](double sx, double sy, double sz) {
            const double dx = x - sx, dy = y - sy, dz = z - sz;
            return dx * dx + dy * dy + dz * dz;
        };
        const int start = a.vorStart[m];
        double sx, sy, sz;
        siteAt(a, start, sx, sy, sz);
        const double target = d2(sx, sy, sz);
        const int cnt = reinterpret_cast<const int4*>(a.vorSlots + start + 2)->y;
        for (int q = 0; q < cnt; q++) {
            const int nxt = vorEntry(a.vorSlots + start, q).next;
            if (nxt < 0) continue;
            siteAt(a, nxt, sx, sy, sz);
            if (d2(sx, sy, sz) < target) return false;
        }
        return true;
    }
};

#endif  // SKIRT_AMD_DEVICE_GRID_VORONOI_HPP
