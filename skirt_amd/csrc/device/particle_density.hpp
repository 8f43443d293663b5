// The dust density of an imported particle set (SKIRTcore/SPHDustDistribution.cpp with SPHGasParticle.cpp and
// SPHGasParticleGrid.cpp): the cubic-spline density at a point, and the mass in a box from the tabulated error
// function, over the particle lists of a 20 x 20 x 20 grid of cells. The arithmetic is +, -, *, sqrt, comparisons,
// one truncation to int and table loads, in the reference's order, so the same text gives the same bits where it
// compiles: for gfx950 (the two kernels of particle_kernels.hpp), for the host set-up (host/particles.hpp) and as plain
// C++ for the CPU logic test (tools/particle_density_cpu.py). It touches nothing of the engine.
//
// PartView is the uploaded particle set: per particle a packed record of the centre and the constants the host cached
// (PartRec), the 3 x 21 separators of the cell grid, the cells' particle lists as CSR (cell ((i*20)+j)*20+k, every
// list in ascending particle index) and the host-built table erf(i * 2.5 / 5000), i = 0 .. 5000.
//
// A box that lies in one cell sums that cell's list. A box that spans more cells sums every particle of the spanned
// lists once, in ascending particle index (the reference joins them through a std::set of pointers into the particle
// vector): an ordered merge of the lists with one cursor per spanned cell. The cursors are the caller's storage
// (LDS in the kernel), at most partMergeCap of them; a box that spans more cells is not summed here (partMassInBox
// returns false) and goes back to the host. The cap is the engine's own choice.
#ifndef SKIRT_AMD_DEVICE_PARTICLE_DENSITY_HPP
#define SKIRT_AMD_DEVICE_PARTICLE_DENSITY_HPP

#if !defined(__HIPCC__)
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#endif

#if defined(__HIPCC__)
#define SKIRT_PART_FN __host__ __device__ inline
#else
#define SKIRT_PART_FN inline
#endif

constexpr int partGrid = 20;         // SPHDustDistribution::setupSelfBefore: GRIDSIZE
constexpr int partErfN = 5000;       // SPHGasParticle.cpp: _N (the table has _N + 1 entries)
constexpr double partErfMax = 2.5;   // _Xmax
constexpr int partMergeCap = 64;     // spanned cells a device thread merges (4 x 4 x 4)
constexpr int partMassBlock = 64;    // threads per block of the mass kernel: partMergeCap cursors each in LDS

// a particle: the centre, then SPHGasParticle's _norm, _rho0, _rho2, _s and _MZ8
struct PartRec {
    double x, y, z, norm, rho0, rho2, s, mz8;
};

struct PartView {
    const PartRec* rec;
    const double* sep;      // 3 x (partGrid + 1): x, y, z separators
    const int* cellOffset;  // partGrid^3 + 1
    const int* cellList;
    const double* erfTable;  // partErfN + 1
    double fdust;
    int nparticles;
};

// NR::locate_clip on one axis' partGrid + 1 separators (the ends are -inf and +inf; entries the equal-count cuts never
// reached keep the array's zero fill, so the bisection runs as the reference's does on an unsorted array)
SKIRT_PART_FN int partLocate(const double* xv, double x) {
    if (x < xv[0]) return 0;
    int jl = -1, ju = partGrid;
    while (ju - jl > 1) {
        const int jm = (ju + jl) >> 1;
        if (x < xv[jm]) ju = jm;
        else jl = jm;
    }
    return jl;
}

// SPHGasParticle::metalDensity
SKIRT_PART_FN double partMetalDensity(const PartRec& p, double x, double y, double z) {
    const double dx = x - p.x, dy = y - p.y, dz = z - p.z;
    const double u2 = p.norm * (dx * dx + dy * dy + dz * dz);
    if (u2 < 1.0) {
        const double u = sqrt(u2);
        const double u1m = 1.0 - u;
        if (u < 0.5) return p.rho0 * (1.0 - 6.0 * u2 * u1m);
        return p.rho2 * u1m * u1m * u1m;
    }
    return 0.0;
}

// myerf (SPHGasParticle.cpp:37-43)
SKIRT_PART_FN double partErf(const double* table, double x) {
    if (x >= partErfMax) return 1.;
    if (x >= 0) return table[static_cast<int>(x * (partErfN / partErfMax))];
    if (x > -partErfMax) return -table[static_cast<int>(-x * (partErfN / partErfMax))];
    return -1;
}

// SPHGasParticle::metalMassInBox; b = xmin ymin zmin xmax ymax zmax
SKIRT_PART_FN double partMetalMassInBox(const PartRec& p, const double* table, const double* b) {
    const double r1x = p.s * (b[0] - p.x), r1y = p.s * (b[1] - p.y), r1z = p.s * (b[2] - p.z);
    const double r2x = p.s * (b[3] - p.x), r2y = p.s * (b[4] - p.y), r2z = p.s * (b[5] - p.z);
    return p.mz8 * (partErf(table, r2x) - partErf(table, r1x)) * (partErf(table, r2y) - partErf(table, r1y)) *
           (partErf(table, r2z) - partErf(table, r1z));
}

// SPHDustDistribution::density(bfr)
SKIRT_PART_FN double partDensity(const PartView& v, double x, double y, double z) {
    const int i = partLocate(v.sep, x), j = partLocate(v.sep + (partGrid + 1), y),
              k = partLocate(v.sep + 2 * (partGrid + 1), z);
    const int cell = ((i * partGrid) + j) * partGrid + k;
    double sum = 0.0;
    for (int q = v.cellOffset[cell]; q < v.cellOffset[cell + 1]; q++) sum += partMetalDensity(v.rec[v.cellList[q]], x, y, z);
    sum *= v.fdust;
    return sum > 0. ? sum : 0.;  // max(sum, 0.)
}

// the cell index range of a box (SPHGasParticleGrid::particlesFor(box)): lo[3], hi[3]; returns the number of cells
SKIRT_PART_FN int partBoxCells(const PartView& v, const double* b, int lo[3], int hi[3]) {
    int n = 1;
    for (int a = 0; a < 3; a++) {
        lo[a] = partLocate(v.sep + a * (partGrid + 1), b[a]);
        hi[a] = partLocate(v.sep + a * (partGrid + 1), b[3 + a]);
        // (an unsorted separator array can return a range that runs backwards: the reference's loops then visit no cell)
        n *= hi[a] >= lo[a] ? hi[a] - lo[a] + 1 : 0;
    }
    return n;
}

// SPHDustDistribution::massInBox(box) for a box spanning at most partMergeCap cells; cur[q * stride] holds the cursor
// of the q-th spanned cell. False (and no mass) when the box spans more.
SKIRT_PART_FN bool partMassInBox(const PartView& v, const double* b, int* cur, int stride, double* mass) {
    int lo[3], hi[3];
    const int ncell = partBoxCells(v, b, lo, hi);
    double sum = 0.0;
    if (lo[0] == hi[0] && lo[1] == hi[1] && lo[2] == hi[2]) {
        const int cell = ((lo[0] * partGrid) + lo[1]) * partGrid + lo[2];
        for (int q = v.cellOffset[cell]; q < v.cellOffset[cell + 1]; q++)
            sum += partMetalMassInBox(v.rec[v.cellList[q]], v.erfTable, b);
    } else {
        if (ncell > partMergeCap) return false;
        const int ny = hi[1] - lo[1] + 1, nz = hi[2] - lo[2] + 1;
        // the q-th spanned cell, in the reference's loop order (any order gives the same merge)
        auto cellOf = [&](int q) {
            const int k = q % nz, j = (q / nz) % ny, i = q / (nz * ny);
            return (((lo[0] + i) * partGrid) + lo[1] + j) * partGrid + lo[2] + k;
        };
        for (int q = 0; q < ncell; q++) cur[q * stride] = v.cellOffset[cellOf(q)];
        for (;;) {
            int next = v.nparticles;  // the smallest particle index under a cursor
            for (int q = 0; q < ncell; q++) {
                const int c = cur[q * stride];
                if (c < v.cellOffset[cellOf(q) + 1]) {
                    const int id = v.cellList[c];
                    if (id < next) next = id;
                }
            }
            if (next >= v.nparticles) break;
            for (int q = 0; q < ncell; q++) {  // every list that holds it moves on
                const int c = cur[q * stride];
                if (c < v.cellOffset[cellOf(q) + 1] && v.cellList[c] == next) cur[q * stride] = c + 1;
            }
            sum += partMetalMassInBox(v.rec[next], v.erfTable, b);
        }
    }
    sum *= v.fdust;
    *mass = sum > 0. ? sum : 0.;
    return true;
}

#endif  // SKIRT_AMD_DEVICE_PARTICLE_DENSITY_HPP
