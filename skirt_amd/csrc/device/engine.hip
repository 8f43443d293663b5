// MI355X photon-packet engine: the HIP kernels for gfx950. Their host side, the C ABI of include/skirt_mcrt.h, is
// host/engine_setup.cpp and host/engine_phase.cpp; it sees the types of engine_args.hpp and, of this file, the launch
// seam at its end (engine_launch.hpp).
//
// A photon phase (MonteCarloSimulation::dostellaremissionchunk, MonteCarloSimulation.cpp:265-301)
// runs as a wavefront pipeline over a pool of packet slots resident in HBM:
//
//   eventKernel  one thread per active slot: consumes the result of the slot's last ray and runs the
//                packet's event code in the reference's order -- launch (StellarSystem::launch),
//                escape/absorption bookkeeping and termination (simulateescapeandabsorption),
//                interaction sampling (simulatepropagation), propagation, peel-off weights
//                (peeloffscattering) and scattering (simulatescattering) -- then queues the packet's
//                next rays: its next FILL or WALK ray plus one PEEL ray per instrument. A finished
//                slot claims the next global packet index at once.
//   traceKernel  persistent: every lane pulls rays from the queue (one atomic per wave, ballot +
//                mbcnt) and walks them through the dust grid, one uniform loop body for all lanes:
//     FILL  DustSystem::fillOpticalDepth + the absorption of simulateescapeandabsorption fused in one
//           streaming pass (segment n needs only exp(-tau_{n-1}) and dtau_n,
//           MonteCarloSimulation.cpp:447-470), f64 atomics into Labs; result: tau of the path;
//     WALK  the same path again up to the sampled optical depth, interpolating inside the crossing
//           segment like DustGridPath::pathlength (DustGridPath.cpp:162-173); result: the distance;
//     PEEL  optical depth to the grid edge towards an instrument (DustSystem::opticaldepth), then
//           Instrument::detect into LDS-privatized SED sums and f64 frame atomics.
// Peel-off detections only add to tallies, so they run concurrently with the packet's next FILL ray;
// the random-number sequence of every packet is exactly the reference's. The trace kernel holds only
// the ray in registers (the heavy event code lives in the other kernel), which keeps its occupancy
// high enough to hide the latency of the density / tree gathers.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <type_traits>

#include "vor_terms.hpp"
#include "cyl2d_walk.hpp"
#include "sph_walk.hpp"
#include "geom_sample.hpp"
#include "aniso_emission.hpp"
#include "polarization.hpp"
#include "../../../include/skirt_mcrt.h"
#include "philox.hpp"
#include "engine_args.hpp"
#include "engine_launch.hpp"

using namespace skirt_dev;  // PacketRng, and the types and constants both halves of the engine share (engine_args.hpp)

namespace {

constexpr double kDblMax = 1.7976931348623157e308;
constexpr int kStepsPerPull = 4;  // grid steps between two ray pulls of a trace wave
// occupancy of the trace kernel: 3 waves per SIMD, i.e. at most 168 VGPRs (the grid entry on the pull
// path would otherwise take the octree kernel to 175 and 2 waves; C3 1.91e8 -> 2.15e8 pkt/s at 3). The
// Voronoi walk has its own kernel and attribute below.
#ifndef SKIRT_TRACE_WAVES  // (variant builds: tools/build_variant.sh TAG -DSKIRT_TRACE_WAVES=4)
#define SKIRT_TRACE_WAVES 3
#endif
#define SKIRT_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(SKIRT_TRACE_WAVES)))
#define SKIRT_NOSTORE_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(4)))
// the Voronoi trace kernel at 2 waves per SIMD: its branch-free bounds keep several entries in flight
// and run without spills in 256 VGPRs (C4 5.72e7 pkt/s at 3 waves, 6.08e7 at 2)
#ifndef SKIRT_VOR_TRACE_WAVES  // (variant builds)
#define SKIRT_VOR_TRACE_WAVES 2
#endif
#define SKIRT_VOR_TRACE_ATTR __attribute__((amdgpu_waves_per_eu(SKIRT_VOR_TRACE_WAVES)))
// the event kernel at 2 waves per SIMD: the Voronoi instantiation (cellIndex on the grid entry of every
// queued ray) would otherwise take 256 VGPRs + AGPRs and run at 1
#ifndef SKIRT_EVENT_WAVES  // (variant builds)
#define SKIRT_EVENT_WAVES 2
#endif
// One instantiation runs at 1: polarised with several components on a Voronoi grid. It needs 278 registers (256
// VGPRs + 22 AGPRs); held to 2 waves it keeps 96 bytes of scratch per lane ("Registers")
// So do the polarised kernels of an anisotropic source (ANISO) with several components: at 2 waves five of the
// eight keep 12-24 bytes of scratch per lane (profiles/aniso_first.txt)
#define SKIRT_EVENT_ATTR_FOR(GRID, ONECOMP, POL, ANISO) \
    __attribute__((amdgpu_waves_per_eu(                  \
        ((POL) && !(ONECOMP) && ((ANISO) || (GRID) == SKIRT_GRID_VORONOI)) ? 1 : SKIRT_EVENT_WAVES)))
// Whether the anisotropic event kernels (ANISO) exist for a grid: not for Voronoi grids, whose event kernel enters
// the grid itself and has no registers left (above); such a phase is refused (runPhase)
template <int GRID>
constexpr bool kAnisoGrid = GRID != SKIRT_GRID_VORONOI;

enum RayMode : unsigned { RAY_NONE = 0, RAY_PEEL = 1, RAY_FILL = 2, RAY_WALK = 3 };
enum State : int { S_NEW = 0, S_FILL = 2, S_WALK = 3 };
// peel-off categories (which FullInstrument arrays a detection adds to, FullInstrument.cpp:115-171)
enum PeelCat : unsigned { CAT_STAR_DIRECT = 0, CAT_STAR_SCATTERED = 1, CAT_DUST_DIRECT = 2, CAT_DUST_SCATTERED = 3 };

static_assert(GEOMS_SHELL == SKIRT_GEOM_SHELL && GEOMS_GAMMA == SKIRT_GEOM_GAMMA && GEOMS_GAUSSIAN == SKIRT_GEOM_GAUSSIAN &&
                  GEOMS_TTAURIDISK == SKIRT_GEOM_TTAURIDISK && GEOMS_TORUS == SKIRT_GEOM_TORUS &&
                  GEOMS_CONICALSHELL == SKIRT_GEOM_CONICALSHELL,
              "geom_sample.hpp follows the kinds of skirt_mcrt.h");
static_assert(ANISO_NETZER == SKIRT_GEOM_NETZER && ANISO_STELLARSURFACE == SKIRT_GEOM_STELLARSURFACE &&
                  ANISO_SPHEBACKGROUND == SKIRT_GEOM_SPHEBACKGROUND && ANISO_CUBBACKGROUND == SKIRT_GEOM_CUBBACKGROUND &&
                  ANISO_SOLARPATCH == SKIRT_GEOM_SOLARPATCH && ANISO_LASER == SKIRT_GEOM_LASER,
              "aniso_emission.hpp follows the kinds of skirt_mcrt.h");
template <int GRID>
constexpr bool kEnterInEvent = GRID == SKIRT_GRID_VORONOI;
// the queue's format (RayRef or RayRec): CONT is the trace kernels' template argument; in the event kernel,
// which serves both, Args::continuous (wave-uniform)
template <int GRID, bool CONT>
constexpr bool kRayRefs = !kEnterInEvent<GRID> && !CONT;
// Voronoi cellIndex: block-list candidates loaded per round trip. Round 3 chose 4; with the round-4
// registers 2 lets the Voronoi event kernel run 3 waves/SIMD (165 VGPRs): event 2.59 -> 2.26 ms, C4
// 1.0225e8 -> 1.0345e8 (8: 1.021e8), profiles/r04_cellindex_group.txt
constexpr int kCellIndexGroup = 2;  // Voronoi cellIndex: block-list candidates per load round
constexpr int kNoCell = -2;  // a cached cell index not known yet (-1 is a located point without a cell)
// most segments one Grid<GRID>::step adds (the Voronoi step may add a pending and a new segment)
template <int GRID>
constexpr int kSegsPerStep = GRID == SKIRT_GRID_VORONOI ? 2 : 1;

__device__ __forceinline__ unsigned rayMode(unsigned f) { return f & 3u; }
__device__ __forceinline__ unsigned rayCat(unsigned f) { return (f >> 2) & 3u; }
__device__ __forceinline__ int rayInstr(unsigned f) { return (int)((f >> 4) & 63u); }
__device__ __forceinline__ int rayLevel(unsigned f) { return (int)((f >> 10) & 255u); }
__device__ __forceinline__ int rayEll(unsigned f) { return (int)(f >> 18); }

// What follows a finished FILL ray: the end of fillOpticalDepth + simulateescapeandabsorption, the
// termination test and the optical depth of the interaction (Random::exponcutoff and the composite biasing
// with weight p/q, MonteCarloSimulation.cpp:519-534). One function for the event kernel, which draws from
// the packet's stream, and for the trace lane of a fused FILL ray, which holds the two deviates the event
// kernel drew ahead from a copy of that stream (FillDrawsAhead): both decide with the same operations on
// the same bits. FILL_FALLBACK: more than those deviates are needed (exponcutoff's rejection loop fired) or
// taupath is negative, NaN or infinite -- the event kernel finishes either, the lane only reports it.
enum FillStatus : int { FILL_TERMINATED = 0, FILL_NO_WALK = 1, FILL_WALK = 2, FILL_FALLBACK = 3 };
// the composite biasing's weight p/q applied to L (MonteCarloSimulation.cpp:529-533)
__device__ __forceinline__ double fillBiasWeight(double L, double tauint, double taupath, double xi) {
    const double pr = -exp(-tauint) / expm1(-taupath);
    const double q = (1.0 - xi) * pr + xi / taupath;
    return L * (pr / q);
}
// Lsca: the scattered luminosity of a multi-component path; albedo: of the one component (ONECOMP);
// thr: Lth once the packet has its minimum of scatterings, else 0; draws: biased(xi) (X < xi, asked only
// when xi != 0), then uniform(), in the stream's order. L is updated (the weight too, unless FILL_FALLBACK).
template <bool ONECOMP, class Draws>
__device__ __forceinline__ int decideFill(double taupath, double& L, double Lsca, double albedo, double thr, double xi,
                                          Draws& draws, double& tauint) {
    tauint = 0.0;  // taupath == 0: no propagation (MonteCarloSimulation.cpp:522)
    if (taupath < 0.0 || isnan(taupath) || isinf(taupath)) return FILL_FALLBACK;
    if (ONECOMP) L = L * albedo * (-expm1(-taupath));
    else L = Lsca;
    if (L <= 0 || L <= thr) return FILL_TERMINATED;
    if (taupath == 0.0) return FILL_NO_WALK;
    const bool biased = xi != 0.0 && draws.biased(xi);
    const double u = draws.uniform();
    double t;
    if (biased || taupath < 1e-10) t = u * taupath;
    else {
        const double norm = 1.0 - exp(-taupath);
        t = -log(1.0 - u * norm);
        if (t > taupath) return FILL_FALLBACK;  // exponcutoff draws again
    }
    if (xi != 0.0) L = fillBiasWeight(L, t, taupath, xi);
    tauint = t;
    return t > 0 ? FILL_WALK : FILL_NO_WALK;  // tauint == 0: the interaction point is where the packet is
}
// the deviates of decideFill from the packet's stream
struct FillDrawsStream {
    PacketRng& rng;
    __device__ __forceinline__ bool biased(double xi) { return rng.uniform() < xi; }
    __device__ __forceinline__ double uniform() { return rng.uniform(); }
};
// and as the event kernel drew them ahead for the trace lane
struct FillDrawsAhead {
    bool b;
    double u;
    __device__ __forceinline__ bool biased(double) const { return b; }
    __device__ __forceinline__ double uniform() const { return u; }
};

// entry q of the list of the cell whose block starts at B
__device__ __forceinline__ VorEntry vorEntry(const VorEntry* B, int q) {
    const float* P = reinterpret_cast<const float*>(B + kVorHead + (q & ~1));
    const int h = q & 1;
    return VorEntry{P[h], P[2 + h], P[4 + h], __float_as_int(P[6 + h])};
}

// entries q0 .. q0 + N - 1 (q0 even), two 16-byte loads per pair
template <int N>
__device__ __forceinline__ void vorEntries(const VorEntry* B, int q0, VorEntry (&e)[N]) {
#pragma unroll
    for (int p = 0; p < N / 2; p++) {
        const float4 x = *reinterpret_cast<const float4*>(B + kVorHead + q0 + 2 * p);
        const int4 y = *reinterpret_cast<const int4*>(B + kVorHead + q0 + 2 * p + 1);
        e[2 * p] = VorEntry{x.x, x.z, __int_as_float(y.x), y.z};
        e[2 * p + 1] = VorEntry{x.y, x.w, __int_as_float(y.y), y.w};
    }
}
// FILL segments: exp(-tau) carried as a product while the segments' optical depths stay below this
constexpr double kCarryTau = 0.5;
#ifndef SKIRT_POLY_EXPM1
#define SKIRT_POLY_EXPM1 1
#endif
// 1 - exp(-x) = -expm1(-x) for 0 <= x < kCarryTau (the FILL segments' absorbed fraction,
// MonteCarloSimulation.cpp:458-462) as x + x^2 q(x), q a degree-9 polynomial fitted at Chebyshev nodes of
// [0, 0.5] (approximation error 0.04 ulp): within 1 ulp of glibc's expm1 over 2e7 arguments, as ocml's is,
// in 11 VALU operations and 18 register moves against ocml's ~53 (range reduction, ldexp, the constants'
// moves): C2, C4, C5 +0.4 %, C3 +0.1 % (the trace kernels are not VALU-bound; profiles/r06_poly_expm1_ab.txt)
__device__ __forceinline__ double oneMinusExpNeg(double x) {
    double q = 2.0367415268789147e-08;
    q = fma(q, x, -2.7077568604087168e-07);
    q = fma(q, x, 2.7529604741385112e-06);
    q = fma(q, x, -2.4800612392596861e-05);
    q = fma(q, x, 0.00019841248533674491);
    q = fma(q, x, -0.0013888888604734388);
    q = fma(q, x, 0.0083333333311535578);
    q = fma(q, x, -0.04166666666658167);
    q = fma(q, x, 0.16666666666666538);
    q = fma(q, x, -0.5);
    return fma(x, x * q, x);
}
constexpr int kVorFallbackGroup = 2;  // neighbour sites loaded together by the exact re-evaluation (<= kVorUnroll)
constexpr int kVorCand = 4;  // possible winners the exact re-evaluation collects before it takes the whole list

// NR::interpolate_loglog (Fundamentals/NR.hpp:321-345): logarithmic in x, and in f when both f > 0
__device__ __forceinline__ double interpolateLogLog(double x, double x1, double x2, double f1, double f2) {
    x = log10(x);
    x1 = log10(x1);
    x2 = log10(x2);
    const bool logf = f1 > 0 && f2 > 0;
    if (logf) {
        f1 = log10(f1);
        f2 = log10(f2);
    }
    double fx = f1 + ((x - x1) / (x2 - x1)) * (f2 - f1);
    if (logf) fx = pow(10.0, fx);
    return fx;
}

__device__ __forceinline__ void atomicAddF64(double* p, double v) {
    // explicit global address space: global_atomic_add_f64 instead of a flat atomic
    __hip_atomic_fetch_add((__attribute__((address_space(1))) double*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The trace kernel's Labs drain as buffer atomics (buffer_atomic_add_f64 through a raw buffer descriptor of
// the Labs table): every lane of the drain instruction issues, the lanes without an add at an offset past
// the table, which the buffer range check drops (tools/buffer_atomic_oob.hip). A global atomic under
// `if (lane has an add)` is a branch the compiler's waitcnt pass cannot see through: the next load of the
// walk then waited with vmcnt(0), i.e. for the drain's atomics too, which stay counted for thousands of
// cycles under load (MI355X_MICROARCH.md, float atomic add row). With a fixed count of vector-memory
// operations per step the load that the previous step requested is waited for alone.
}  // namespace (the intrinsic's declaration has external linkage)
__device__ double bufferAtomicAddF64(double v, __amdgpu_buffer_rsrc_t rsrc, int voffset, int soffset, int aux)
    __asm("llvm.amdgcn.raw.ptr.buffer.atomic.fadd.f64");
namespace {

// the small tables staged in LDS
struct Shared {
    const double* mesh;   // Cartesian: mesh borders | octree with leaf map: split coordinates
    const double* kext;   // [ncomp][nlambda]
    const double* ksca;
    const double* alb;
    const double* g;
    const DevInstr* instr;
    double* sed;
};

enum StageParts : int { STAGE_MESH = 1, STAGE_TREE = 2, STAGE_OPTICS = 4, STAGE_INSTR = 8 };

__device__ __forceinline__ Shared stageTables(const Args& a, double* lds, int parts) {
    Shared sh;
    double* m = lds + a.ldsMeshOff;
    double* opt = lds + a.ldsOptOff;
    double* idst = lds + a.ldsInstrOff;
    sh.mesh = m;
    sh.kext = opt;
    sh.ksca = opt + a.ncomp * a.nlambda;
    sh.alb = opt + 2 * a.ncomp * a.nlambda;
    sh.g = opt + 3 * a.ncomp * a.nlambda;
    sh.instr = reinterpret_cast<const DevInstr*>(idst);
    sh.sed = lds + a.ldsSedOff;
    const int nmesh = (parts & STAGE_MESH) ? (a.nx + a.ny + a.nz + 3) : 0;
    for (int q = threadIdx.x; q < nmesh; q += blockDim.x) m[q] = a.mesh[q];
    const int ntree = (parts & STAGE_TREE) ? 3 * (a.mapN + 1) : 0;
    for (int q = threadIdx.x; q < ntree; q += blockDim.x) m[q] = a.treeT[q];
    const int nopt = (parts & STAGE_OPTICS) ? 4 * a.ncomp * a.nlambda : 0;
    for (int q = threadIdx.x; q < nopt; q += blockDim.x) opt[q] = a.optics[q];
    const int ninw = (parts & STAGE_INSTR) ? a.ninstr * (int)(sizeof(DevInstr) / sizeof(double)) : 0;
    const double* isrc = reinterpret_cast<const double*>(a.instr);
    for (int q = threadIdx.x; q < ninw; q += blockDim.x) idst[q] = isrc[q];
    __syncthreads();
    return sh;
}

template <int GRID>
__device__ __forceinline__ constexpr int gridParts() {
    return (GRID == SKIRT_GRID_CARTESIAN || GRID == SKIRT_GRID_CYLINDER2D || GRID == SKIRT_GRID_SPHERE1D ||
            GRID == SKIRT_GRID_SPHERE2D) ? STAGE_MESH
           : ((GRID == SKIRT_GRID_OCTREE || GRID == kBinTreeMap) ? STAGE_TREE : 0);
}

__device__ __forceinline__ void crossedAdd(const Args& a, unsigned n) {
    const unsigned wave = (blockIdx.x * (kBlock / 64) + threadIdx.x / 64) & (kCrossedCopies - 1);
    atomicAdd(a.crossed + (size_t)wave * a.crossedBins + min(n, (unsigned)a.crossedBins - 1u), 1ull);
}
__device__ __forceinline__ void flushStats(const Args& a, const unsigned long long (&vals)[8]) {
    const int lane = threadIdx.x & 63;
    unsigned long long* dst = a.stats + 8 * ((blockIdx.x * (kBlock / 64) + threadIdx.x / 64) & (kStatCopies - 1));
#pragma unroll
    for (int q = 0; q < 8; q++) {
        unsigned long long v = vals[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0 && v) atomicAdd(dst + q, v);
    }
}

// ------------------------------------------------------------------ the ray (trace kernel registers)
struct Ray {
    double x, y, z;        // current position along the ray
    double dx, dy, dz;     // direction
    double ix, iy, iz;     // 1/direction (0 where |k| <= 1e-15: that axis is never crossed)
    double tau, s;         // optical depth and path length covered so far
    double kext;           // kappa_ext at the ray's wavelength (one dust component)
    double param;          // see RayRec::param
    double f1, f2;         // FILL: exp(-tau), Lsca | WALK: tau and s at the previous segment end
    double bx0, by0, bz0, bx1, by1, bz1;  // octree walked through the node arrays: box of the node |
                                          //   cylindrical walk: q, p, k_q, k_z, q_N (Grid<SKIRT_GRID_CYLINDER2D>) |
                                          //   Sphere1D walk: q, p, q_N (Grid<SKIRT_GRID_SPHERE1D>)
    double rho0;           // density (component 0) of the current cell
    int ci, cj, ck;        // Cartesian cell indices | octree: node, cell number, leaf size in finest cells |
                           //   cylindrical walk: i, i_min, k | Sphere1D walk: i, i_min |
                           //   Sphere2D walk: i, steps left, k (the position advances in x, y, z)
    int jx, jy, jz;        // octree leaf map: finest-level index of the current leaf's lower corner |
                           //   cylindrical and Sphere1D walks: jx = 1 while the ray moves inward
    int4 pre;              // octree leaf map: the next step's leaf-map entry, requested at the end of this step
    int pfx, pfy, pfz;     //   and the finest-level cell it was requested for (LeafMapGrid::prefetch)
    double ex, ey, ez, eds;  // octree leaf map: the current leaf's exit point and distance, and its wall,
    int ewall;               //   computed once by prefetch for the next step
    int idx, ell;
    unsigned flags, mode;
    unsigned id;           // queue index of the ray (a PEEL ray writes its optical depth back there)
};

// ------------------------------------------------------------------ grids
template <int GRID>
struct Grid;

// the grid walks: headers that compile only here, inside this namespace (as detect.hpp, emission.hpp and
// density_sample.hpp below)
#include "grid_cartesian.hpp"
#include "grid_mesh2d.hpp"
#include "grid_tree.hpp"
#include "grid_voronoi.hpp"

// ================================================================== trace kernel
// GLOBAL: the Labs adds as global atomics (a table of 4 GiB or more, Args::labsGlobal), a kernel of its own:
// a run-time choice between the buffer atomic every lane issues and a global atomic only lanes with an add
// issue leaves the waitcnt pass a path with no vector-memory operation in the drain, and the next step's
// leaf-map entry then waited with vmcnt(0), i.e. for the drain's atomic as well. Now vmcnt(1): C3 +0.3 %,
// C2 +0.4 %, C4 and C5 within the spread (the atomic had mostly finished by then; profiles/r06_decode_wait_ab.txt)
template <int GRID, bool ONECOMP, bool CONT, bool STORE, bool GLOBAL = false>
struct Tracer {
    const Args& a;
    const Shared& sh;
    // statistics, kept out of the walk's registers: the lane's segments of its current ray (added per ray
    // to the wave's FILL / WALK / PEEL totals in LDS when the ray ends), and wave-uniform counts of the
    // Labs adds, lane-steps and 64-byte atomic requests (lane 0's values are the wave's)
    unsigned int nseg = 0;
    unsigned int absorbs = 0, laneSlots = 0, requests = 0;
    unsigned* waveSegs;  // LDS, [kBlock / 64][3]: FILL, WALK, PEEL segments of the wave's finished rays
    // Labs adds of this lane not yet issued. f64 atomics execute memory-side at a fixed chip-wide rate
    // of 64-byte requests; lanes of one wave instruction that hit the same 64-byte line share a
    // request. A lane's consecutive adds are consecutive cells of one ray -- spatial neighbours, and
    // with Morton-ordered device cell numbers mostly in the same or the next line -- so the adds wait
    // in LDS (kLabsBuf per lane, [slot][thread]) and are issued transposed: each wave instruction
    // carries the kLabsBuf consecutive adds of 64 / kLabsBuf lanes. A wave also waits for one
    // atomic round trip per burst instead of one per step.
    double* pendVal;    // LDS, [kLabsBuf][kBlock]
    unsigned* pendIdx;  // LDS, [kLabsBuf][kBlock]
    unsigned char* pendHi;  // LDS, [kLabsBuf][kBlock]: bits 32-39 of the element index (Args::labsHi only)
    __amdgpu_buffer_rsrc_t labsRsrc;  // the Labs table as a raw buffer of labsBytes (unless Args::labsGlobal)
    unsigned copyOff = 0;             // this wave's replica (Args::labsCopies), in bytes
    unsigned labsOob = 0;             // a byte offset past every replica: the empty lanes' adds are dropped
    int npend = 0;
    unsigned gstep = 0;  // grid steps of the wave (drainStep's round robin)
    // a fused FILL ray (Args::fuse): the deviate and the termination threshold its lane decides with when the
    // ray ends (decideFill). On a walk the lane is marked for re-entry (kLaneWalkOn in the idle lane's queue
    // index, else 0) and the deviate's place holds the optical depth to reach. They live in registers a FILL ray
    // leaves unused where there are any: with one component it sums no scattered luminosity (f2), and in a
    // kernel without Labs adds it carries no exp(-tau) (f1)
    double fu = 0, fthr = 0;
    static constexpr unsigned kLaneWalkOn = 1u << 31;  // (the queue holds fewer than 2^31 records)
    // Not with continuous scattering (Args::fuse is 0 there), and not in the node-array walk's no-store kernel:
    // at 4 waves per SIMD it has 3 registers to spare, and the decision's exp and log would spill
    // (planPhase leaves those phases unfused)
    static constexpr bool kFuse = !CONT && (STORE || GRID != kOctreeNodes);
    __device__ __forceinline__ double& fillThr(Ray& r) { return ONECOMP ? r.f2 : fthr; }
    __device__ __forceinline__ double& fillU(Ray& r) { return (ONECOMP && !STORE) ? r.f1 : fu; }

    __device__ __forceinline__ void drain() {
        static_assert(kLabsBuf >= 2 && kLabsBuf <= 64 && (kLabsBuf & (kLabsBuf - 1)) == 0, "kLabsBuf: power of 2");
#pragma unroll
        for (int i = 0; i < kLabsBuf; i++) issue(i);
        npend = 0;
    }

    // wave instruction i of a drain: the buffered adds of lanes G i .. G i + G - 1 (G = 64 / kLabsBuf),
    // kLabsBuf consecutive adds of each, transposed onto the wave's lanes
    __device__ __forceinline__ void issue(int i) {
        constexpr int G = 64 / kLabsBuf;
        const int lane = threadIdx.x & 63;
        const int wbase = threadIdx.x - lane;
        const int j = lane & (kLabsBuf - 1);
        const int src = G * i + lane / kLabsBuf;
        const int n = __shfl(npend, src);
        const int q = j * kBlock + wbase + src;
        const unsigned idx = pendIdx[q];
        // the element index: 32 bits, or 40 with the high byte of a table of 2^32 elements or more
        const size_t eidx = a.labsHi ? ((size_t)pendHi[q] << 32 | idx) : (size_t)idx;
        // the requests of this instruction: a lane starts one unless the lane before it (the same
        // ray's previous add) hit the same 64-byte line (these statistics cost nothing measurable: C3 +0.05 %,
        // C2 +0.6 % without them, timing only; profiles/r06_ab.txt)
        const unsigned line = (unsigned)(reinterpret_cast<size_t>(a.labs + eidx) >> 6);
        const unsigned prev = __shfl(line, lane - 1);
        const unsigned long long starts = __ballot(j < n && (j == 0 || prev != line));
        absorbs += (unsigned)__popcll(__ballot(j < n));
        requests += (unsigned)__popcll(starts);
        if constexpr (GLOBAL) {  // a table of 4 GiB or more: global atomics
            if (j < n) atomicAddF64(a.labs + eidx, pendVal[q]);
        } else {
            // every lane issues; a lane without an add adds 0 at the first byte past the table (dropped)
            const double v = j < n ? pendVal[q] : 0.0;
            bufferAtomicAddF64(v, labsRsrc, (int)(j < n ? idx * 8u + copyOff : labsOob), 0, 0);
        }
    }

    // One drain instruction per grid step, round robin over the lane groups: every lane's buffer is
    // emptied every kLabsBuf steps, which holds its at most kLabsBuf adds (one per step), and the adds
    // leave as a steady stream instead of a burst of kLabsBuf instructions (which stalls the issuing
    // wave behind its outstanding atomics and reaches the memory-side atomic units in clumps).
    __device__ __forceinline__ void drainStep() {
        constexpr int G = 64 / kLabsBuf;
        const int i = (int)(gstep++ & (kLabsBuf - 1));
        issue(i);
        if (((threadIdx.x & 63) / G) == i) npend = 0;
    }
    // The same for steps of up to two adds (the Voronoi walk, kSegsPerStep 2): two drain instructions every
    // step, so every lane's buffer is emptied every kLabsBuf / 2 steps. It replaces a full drain whenever a
    // buffer might overflow: the same instructions on average, but that drain sat behind a branch, and after it
    // the waitcnt pass could count no atomics with certainty, so the walk's next load waits (vmcnt(0)) covered
    // the 16 atomics of any drain before them. C4 +0.3 %, 230 -> 211 VGPRs (profiles/r06_vor_drain_ab.txt)
    __device__ __forceinline__ void drainStep2() {
        constexpr int G = 64 / kLabsBuf;
        const int i = (int)(gstep++ & (kLabsBuf / 2 - 1)) * 2;
        issue(i);
        issue(i + 1);
        const int grp = (threadIdx.x & 63) / G;
        if (grp == i || grp == i + 1) npend = 0;
    }

    __device__ __forceinline__ double rho(int m, int h) const { return a.rho[(size_t)m * a.ncomp + h]; }

    // per-segment work; false stops the ray (a WALK reached its optical depth)
    __device__ __forceinline__ bool segment(Ray& r, int m, double rho0, double ds) {
        if (!(ds > 0)) return true;  // DustGridPath::addSegment skips ds <= 0
        double kr = 0.0;  // KappaRho functor (DustSystem.cpp:465-491)
        if (m >= 0) {
            if (ONECOMP) kr = r.kext * rho0;
            else for (int h = 0; h < a.ncomp; h++) kr += sh.kext[h * a.nlambda + r.ell] * rho(m, h);
        }
        const double dtau = kr * ds;
        if (CONT && r.mode == RAY_FILL && m >= 0) {
            // the segment as the path holds it, before s and tau advance; the slot's count lives in
            // pathCnt (no register of the walk carries it)
            const int n = a.pathCnt[r.idx];
            if (n < kPathCap) {
                a.pathBuf[(size_t)r.idx * kPathCap + n] = PathRec{r.s, ds, r.tau, dtau, m, 0};
                a.pathCnt[r.idx] = n + 1;
            } else {
                atomicOr(a.error, ERR_PATH_CAP);
            }
        }
        r.s += ds;
        r.tau += dtau;
        nseg++;
        if (r.mode == RAY_FILL) {
            if (m >= 0 && (!ONECOMP || (STORE && a.store))) {
                // L_abs = (1-albedo) L exp(-tau_{n-1}) (1 - exp(-dtau_n)) (MonteCarloSimulation.cpp:458-462).
                // exp(-tau) is carried in f1 as the running product of exp(-dtau) = 1 - ef, which is exact to
                // about an ulp per segment while ef <= 1 - exp(-kCarryTau); behind a thicker segment (where
                // 1 - ef loses digits: rounds 1-3 carried it unconditionally and the thick pan_oct_sa models'
                // deep cells drifted) it is evaluated anew. One f64 exp less per segment: C2 +0.6 %, C5 +0.5 %,
                // C3 within the spread (profiles/r05_exp_carry_ab.txt)
                double ef;
                if (SKIRT_POLY_EXPM1 && dtau < kCarryTau) ef = oneMinusExpNeg(dtau);
                else ef = -expm1(-dtau);
                const double Lintm = r.param * r.f1 * ef;
                if (dtau < kCarryTau) r.f1 -= r.f1 * ef;
                else r.f1 = exp(-r.tau);
                double albedo;
                if (ONECOMP) albedo = sh.alb[r.ell];
                else {
                    double ksca = 0.0, kext = 0.0;
                    for (int h = 0; h < a.ncomp; h++) {
                        ksca += rho(m, h) * sh.ksca[h * a.nlambda + r.ell];
                        kext += rho(m, h) * sh.kext[h * a.nlambda + r.ell];
                    }
                    albedo = (kext > 0.0) ? ksca / kext : 0.0;
                    r.f2 += albedo * Lintm;
                }
#ifdef SKIRT_DEBUG_FILL  // diagnostic builds only (tools/parity_trace.py): the FILL segments, one packet per run
                printf("E S %d %.17g %.17g %.17g\n", m, ds, dtau, (1.0 - albedo) * Lintm);
#endif
                if (STORE && a.store) {
                    pendVal[npend * kBlock + threadIdx.x] = (1.0 - albedo) * Lintm;
                    if (a.labsHi) {  // (wave-uniform) a table of 2^32 elements or more
                        const unsigned long long e = (unsigned long long)r.ell * (unsigned)a.labsStride + (unsigned)m;
                        pendIdx[npend * kBlock + threadIdx.x] = (unsigned)e;
                        pendHi[npend * kBlock + threadIdx.x] = (unsigned char)(e >> 32);
                    } else {
                        pendIdx[npend * kBlock + threadIdx.x] = (unsigned)r.ell * (unsigned)a.labsStride + (unsigned)m;
                    }
                    npend++;
                }
            }
        } else if (r.mode == RAY_WALK) {
            if (r.tau > r.param) return false;  // the interaction point lies in this segment
            r.f1 = r.tau;
            r.f2 = r.s;
        }
        return true;
    }

    // load queued ray `id` and enter the grid: the part of the path before the grid (segments outside
    // it, m = -1) and the first cell (DustGrid::path); an empty path finishes the ray at once.
    // walkOn: the lane's own fused FILL record again, now as the WALK ray to the optical depth in fillU
    __device__ __forceinline__ void load(Ray& r, unsigned id, bool walkOn) {
        double2 c3;  // RayRec: s0, param | RayRef: the slot's fuseThr, and sL (FILL) or fuseU (WALK)
        int4 c6;     // RayRec: idx, flags, ci, cj | RayRef: idx, flags, and the slot's fuseU in z, w
        r.id = id;
        if constexpr (kRayRefs<GRID, CONT>) {
            // the reference, then one batch of loads through its slot for every mode: the origin, the direction
            // (the packet's, or a peel-off's instrument's) and the slot's L, deviate and threshold, which a
            // peel-off loads and does not use (an empty path's reference names its slot as well)
            const int4 q = reinterpret_cast<const int4*>(a.rays)[id];
            const int slot = q.z;
            unsigned flags = (unsigned)q.y;
            if (kFuse && walkOn) flags = (flags & ~3u) | RAY_WALK;
            const bool peel = rayMode(flags) == RAY_PEEL;
            const double* kobs = a.instr[peel ? rayInstr(flags) : 0].kobs;  // (an address only, unless a peel-off)
            const double* const px = peel ? kobs : a.skx + slot;
            const double* const py = peel ? kobs + 1 : a.sky + slot;
            const double* const pz = peel ? kobs + 2 : a.skz + slot;
            r.x = a.srx[slot]; r.y = a.sry[slot]; r.z = a.srz[slot];
            r.dx = *px; r.dy = *py; r.dz = *pz;
            double L = a.sL[slot], u = a.fuseU[slot], thr = a.fuseThr[slot];
            // (the values are wanted here: left alone, the compiler moves these three loads behind the mode's
            // branches below, a second round trip for the FILL lanes)
            asm volatile("" : "+v"(L), "+v"(u), "+v"(thr));
            c3 = make_double2(thr, rayMode(flags) == RAY_WALK ? u : L);
            c6 = make_int4(q.x, (int)flags, __double2loint(u), __double2hiint(u));
        } else {
            const double2* c = reinterpret_cast<const double2*>(a.rays + id);
            const double2 c0 = c[0], c1 = c[1], c2 = c[2];
            c3 = c[3];
            c6 = reinterpret_cast<const int4*>(c)[4];
            r.x = c0.x; r.y = c0.y; r.z = c1.x;
            r.dx = c1.y; r.dy = c2.x; r.dz = c2.y;
        }
        // 1/direction, 0 where |k| <= 1e-15 (that axis is never crossed), as the event kernel computed it
        r.ix = (fabs(r.dx) > 1e-15) ? 1.0 / r.dx : 0.0;
        r.iy = (fabs(r.dy) > 1e-15) ? 1.0 / r.dy : 0.0;
        r.iz = (fabs(r.dz) > 1e-15) ? 1.0 / r.dz : 0.0;
        r.param = c3.y;
        r.idx = c6.x;
        r.flags = (unsigned)c6.y;
        if (kFuse && walkOn) {
            r.param = fillU(r);
            r.flags = (r.flags & ~3u) | RAY_WALK;
        }
        r.mode = rayMode(r.flags);
        r.ell = rayEll(r.flags);
        r.tau = 0;
        if (CONT && r.mode == RAY_FILL) a.pathCnt[r.idx] = 0;
#ifdef SKIRT_DEBUG_FILL
        if (r.mode == RAY_FILL)
            printf("E L %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", r.ell, r.x, r.y, r.z, r.dx, r.dy, r.dz, r.param);
#endif
        // the path before the grid of a ray the event kernel entered (a fused FILL ray's threshold and deviate
        // come per slot: loaded below for those rays, above with a reference's other loads)
        r.s = kEnterInEvent<GRID> ? c3.x : 0.0;
        r.kext = sh.kext[r.ell];
        // FILL: f1 = exp(-tau) = 1, f2 = scattered luminosity; WALK: tau and s at the last segment end
        r.f1 = (r.mode == RAY_FILL) ? 1.0 : 0.0;
        r.f2 = (r.mode == RAY_WALK) ? r.s : 0.0;
        if (kFuse && a.fuse && r.mode == RAY_FILL) {
            fillU(r) = kEnterInEvent<GRID> ? a.fuseU[r.idx] : __hiloint2double(c6.w, c6.z);
            fillThr(r) = kEnterInEvent<GRID> ? a.fuseThr[r.idx] : c3.x;
        }
        // the segments before the grid of a ray the event kernel entered travel in the first cell's top bits
        // (a ray the event kernel entered brings its segments before the grid in the first cell's top bits)
        nseg = kEnterInEvent<GRID> ? ((unsigned)c6.z >> kOutsideShift) : 0u;
        if (kEnterInEvent<GRID>) {  // entered by the event kernel: the cell and its neighbour list
            r.ci = c6.z & kCellMaskOut;
            r.cj = c6.w;
            r.ck = 0;
        } else if (r.mode != RAY_NONE &&
            !Grid<GRID>::begin(a, sh, r, [&](int m, double rho0, double ds) { return segment(r, m, rho0, ds); })) {
            finish(r);  // FILL: tau = 0, no scattered luminosity; WALK: s = 0; PEEL: tau = 0
            r.mode = RAY_NONE;
        }
    }

    // the ray ended (grid edge or WALK target reached): deliver its result. The lane of a fused FILL ray
    // decides what the event kernel will decide (decideFill) and, where the packet walks, takes the WALK
    // upon itself (kLaneWalkOn: the pull block loads the lane's record again, Tracer::load)
    __device__ __forceinline__ void finish(Ray& r) {
        atomicAdd(&waveSegs[(threadIdx.x >> 6) * 3 + (r.mode == RAY_FILL ? 0 : r.mode == RAY_WALK ? 1 : 2)], nseg);
        if (a.crossed && r.mode != RAY_WALK) crossedAdd(a, nseg);
        unsigned walkOn = 0;
        double* const walked = (kFuse && a.fuse) ? a.resS : a.resA;
        if (r.mode == RAY_PEEL) {
            a.det[r.idx].tau = r.tau;  // detectKernel turns it into a detection
        } else if (r.mode == RAY_FILL) {
            a.resA[r.idx] = r.tau;
            if (!ONECOMP) a.resB[r.idx] = r.f2;
            if (kFuse && a.fuse) {
                const double u = fillU(r);
                FillDrawsAhead draws{u < 0.0, fabs(u)};
                double L = r.param, tauint;
                int st = decideFill<ONECOMP>(r.tau, L, r.f2, ONECOMP ? sh.alb[r.ell] : 0.0,
                                              ONECOMP ? r.f2 : fthr, a.xi, draws, tauint);
                if (a.fuse == 2 && (r.idx & 1)) st = FILL_FALLBACK;
                if (st == FILL_WALK) {
                    fillU(r) = tauint;
                    walkOn = kLaneWalkOn | r.id;
                } else {
                    a.resS[r.idx] = -1.0;
                }
            }
        } else {
            // DustGridPath::pathlength: interpolate inside the crossing segment; if the path ended first
            // (target >= tau of the path), the end of the last segment
            const double tauint = r.param;
            double s = 0;
            if (tauint > 0) {
                if (r.tau > tauint) s = r.f2 + ((tauint - r.f1) / (r.tau - r.f1)) * (r.s - r.f2);
                else s = r.f2;
            }
            walked[r.idx] = s;
        }
        r.id = walkOn;  // (the ray is over: its lane is idle)
    }
};

#include "detect.hpp"

// DustSystem::writeconvergence (DustSystem.cpp:195-250): the column density of the grid along a ray, as
// DustGridPath::opticalDepth (DustGridPath.hpp:97-108) sums it with DustSystem::density (the cell's
// densities summed over the components, DustSystem.cpp:925-931), over the same walk as the photon paths.
// One lane per ray; rays[6 i .. 6 i + 5] = origin, direction.
template <int GRID>
__global__ void __launch_bounds__(kBlock) columnKernel(const Args a, const double* rays, int n, double* out) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    Shared sh = stageTables(a, lds, gridParts<GRID>());
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r{};
    r.x = rays[6 * i]; r.y = rays[6 * i + 1]; r.z = rays[6 * i + 2];
    r.dx = rays[6 * i + 3]; r.dy = rays[6 * i + 4]; r.dz = rays[6 * i + 5];
    r.ix = (fabs(r.dx) > 1e-15) ? 1.0 / r.dx : 0.0;
    r.iy = (fabs(r.dy) > 1e-15) ? 1.0 / r.dy : 0.0;
    r.iz = (fabs(r.dz) > 1e-15) ? 1.0 / r.dz : 0.0;
    double tau = 0;
    auto seg = [&](int m, double, double ds) {
        if (ds > 0 && m >= 0) {  // (addSegment skips ds <= 0; a segment outside the grid adds 0 x ds)
            double rho = 0;
            for (int h = 0; h < a.ncomp; h++) rho += a.rho[(size_t)m * a.ncomp + h];
            tau += rho * ds;
        }
        return true;
    };
    if (Grid<GRID>::begin(a, sh, r, seg))
        while (Grid<GRID>::step(a, sh, r, seg)) {}
    out[i] = tau;
}

#include "emission.hpp"

// CONT: continuous scattering (the FILL rays record their dust segments); its own instantiations keep
// the recording out of the other kernels' registers
// STORE false: a phase that stores no absorption (a.store = 0), one dust component, no continuous
// scattering: no Labs buffers and no drain (its own instantiation, traceKernelNoStore)
template <int GRID, bool ONECOMP, bool CONT, bool STORE, bool GLOBAL = false>
__device__ __forceinline__ void traceBody(const Args& a) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        // reset the counters the next event iteration appends to (nobody else uses them now)
        CTR(a.ctr, CTR_RAYS + (1 - a.parity)) = 0;  // the next iteration's
        CTR(a.ctr, CTR_ACTIVE + a.parity) = 0;  // just consumed by the event kernel
        CTR(a.ctr, CTR_WALK + (1 - a.parity)) = 0;  // the next iteration's
    }
    // the iteration's rays: CTR_RAYS from the bottom of the queue, then the CTR_WALK rays from its top
    // (Args::walkBack), pulled last: the short WALK paths fill the lanes that the long FILL and peel-off
    // paths free at the end of a launch, instead of idling until the launch's longest path ends
    const unsigned int nfront = CTR(a.ctr, CTR_RAYS + a.parity);
    if (nfront + CTR(a.ctr, CTR_WALK + a.parity) == 0) return;  // an iteration after the end of the phase
    // the front rays (growing up from 0) and the WALK rays (growing down from rayCap - 1) must not meet:
    // the event and continuous peel-off kernels reserved them independently, so this is the first point
    // where both totals are final; an overflow fails the phase instead of tracing overwritten records
    if ((unsigned long long)nfront + CTR(a.ctr, CTR_WALK + a.parity) > (unsigned long long)a.rayCap) {
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.error, ERR_QUEUE);
        return;
    }
    Shared sh = stageTables(a, lds, gridParts<GRID>() | STAGE_OPTICS);

    Tracer<GRID, ONECOMP, CONT, STORE, GLOBAL> T{a, sh};
    T.labsOob = a.labsCopies > 1 ? (unsigned)a.labsCopies * a.labsCopyStride : a.labsBytes;
    T.labsRsrc = __builtin_amdgcn_make_buffer_rsrc(a.labs, 0, (int)T.labsOob, 0x00020000);
    if (a.labsCopies > 1)
        T.copyOff = (unsigned)((blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) % (unsigned)a.labsCopies) * a.labsCopyStride;
    // after the grid and optics tables: the segment counts, then the Labs buffers (STORE only)
    T.waveSegs = reinterpret_cast<unsigned*>(lds + a.ldsInstrOff);
    T.pendVal = lds + a.ldsInstrOff + kSegWords;
    T.pendIdx = reinterpret_cast<unsigned*>(T.pendVal + kLabsBuf * kBlock);
    T.pendHi = reinterpret_cast<unsigned char*>(T.pendIdx + kLabsBuf * kBlock);  // (allocated when a.labsHi)
    if (threadIdx.x < 3 * (kBlock / 64)) T.waveSegs[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const unsigned int nrays = nfront + CTR(a.ctr, CTR_WALK + a.parity);
    Ray r;
    r.mode = RAY_NONE;
    r.id = 0;
    bool done = false;
    // the wave reserves queue ids kPullChunk at a time and hands them to its idle lanes; the next
    // reservation is requested while the current one still lasts, so a pull rarely waits for the atomic
    // (128 on the tree and Cartesian grids: C3 +0.5 %, C2 +1.2 %; 64 on Voronoi grids, C4 -0.2 % at 128;
    // 256 is slower on all, profiles/r05_pull_chunk_ab.txt)
    constexpr unsigned kPullChunk = GRID == SKIRT_GRID_VORONOI ? 64 : 128;
    unsigned cur = 0, curEnd = 0, nxt = 0;
    bool haveNext = false;
    auto reserve = [&]() {
        unsigned int base = 0;
        if (lane == 0) base = atomicAdd(CTRP(a.ctr, CTR_PULL), kPullChunk);
        return __shfl(base, 0);
    };
    while (true) {
        const bool idle = (r.mode == RAY_NONE) && !done;
        const unsigned long long imask = __ballot(idle);
        const unsigned long long amask = __ballot(r.mode != RAY_NONE);
        if (imask == 0 && amask == 0) break;
        if (imask != 0 && (amask == 0 || __popcll(imask) >= a.threshold)) {
            // a lane marked for re-entry takes no queue id: it loads its own record again, as the WALK ray
            const bool walkOn = idle && (r.id & T.kLaneWalkOn) != 0;
            const unsigned long long pmask = imask & ~__ballot(walkOn);
            const unsigned int rank = (unsigned int)__popcll(pmask & ((1ull << lane) - 1ull));
            const unsigned int k = (unsigned int)__popcll(pmask);
            const unsigned int avail = curEnd - cur;
            if (avail < k && !haveNext) { nxt = reserve(); haveNext = true; }
            const unsigned int id = rank < avail ? cur + rank : nxt + (rank - avail);
            if (avail >= k) cur += k;
            else { cur = nxt + (k - avail); curEnd = nxt + kPullChunk; haveNext = false; }
            if (!haveNext && curEnd - cur < kPullChunk / 2 && cur < nrays) { nxt = reserve(); haveNext = true; }
            if (idle) {
                if (!walkOn && id >= nrays) done = true;
                else T.load(r, walkOn ? r.id & ~T.kLaneWalkOn : id < nfront ? id : (unsigned)a.rayCap - 1u - (id - nfront), walkOn);  // a RAY_NONE record (empty path) leaves the lane idle
            }
            // vmcnt(0) here, on the pull's path: without it the waitcnt pass put one at the join with the steps,
            // where a while-iteration without a pull then also waited for the last step's Labs atomic (C2 +1-2 %,
            // C3, C4, C5 within the spread; profiles/r06_pull_wait_ab.txt)
            __builtin_amdgcn_s_waitcnt(0x0F70);
        }
#pragma unroll 1
        for (int it = 0; it < kStepsPerPull; it++) {
            const unsigned long long live = __ballot(r.mode != RAY_NONE);
            if (live == 0) break;
            T.laneSlots += 64;
            auto seg = [&](int m, double rho0, double ds) { return T.segment(r, m, rho0, ds); };
            if (r.mode != RAY_NONE) {
                if (!Grid<GRID>::step(a, sh, r, seg)) {
                    T.finish(r);
                    r.mode = RAY_NONE;
                }
            }
            if constexpr (!STORE) {
            } else if constexpr (kSegsPerStep<GRID> == 1) {
                T.drainStep();  // one drain instruction per step
            } else {
                static_assert(kSegsPerStep<GRID> == 2, "two drains per step hold two adds per step");
                T.drainStep2();
            }
        }
    }
    if constexpr (STORE) T.drain();
    // (wave totals: lane 0 contributes them)
    const unsigned* ws = T.waveSegs + (threadIdx.x >> 6) * 3;
    const bool l0 = lane == 0;
    const unsigned long long vals[8] = {0, l0 ? ws[0] : 0u, l0 ? ws[1] : 0u, l0 ? ws[2] : 0u, 0,
                                        l0 ? T.absorbs : 0u, l0 ? T.laneSlots : 0u, l0 ? T.requests : 0u};
    flushStats(a, vals);
}

template <int GRID, bool ONECOMP, bool CONT, bool GLOBAL = false>
__global__ void __launch_bounds__(kBlock) SKIRT_TRACE_ATTR traceKernel(const Args a) {
    traceBody<GRID, ONECOMP, CONT, true, GLOBAL>(a);
}

// a phase that stores no absorption (the dust emission phase), one component, no continuous scattering:
// without the Labs buffers' LDS and registers, at 4 waves per SIMD
template <int GRID>
__global__ void __launch_bounds__(kBlock) SKIRT_NOSTORE_TRACE_ATTR traceKernelNoStore(const Args a) {
    traceBody<GRID, true, false, false>(a);
}

// the Voronoi walk at its own occupancy (SKIRT_VOR_TRACE_ATTR)
template <bool ONECOMP, bool CONT, bool GLOBAL = false>
__global__ void __launch_bounds__(kBlock) SKIRT_VOR_TRACE_ATTR traceKernelVor(const Args a) {
    traceBody<SKIRT_GRID_VORONOI, ONECOMP, CONT, true, GLOBAL>(a);
}

// ================================================================== event kernel
struct Packet {
    double rx, ry, rz, kx, ky, kz, L, Lth;
    int ell, nscatt, stellar, state;
    PacketRng rng;
    PolStokes sv;  // POL kernels only
};

// the deviates of polScatter from the packet's stream
struct PolDrawsStream {
    PacketRng& rng;
    __device__ __forceinline__ double uniform() { return rng.uniform(); }
};

// POL: a simulation whose dust mixes polarise (Args::pol): the packet carries a Stokes vector, scatters by the
// Mueller tables and its peel-offs carry Q, U, V. POL = false is the code as it was.
// ANISO: a stellar phase one of whose components emits anisotropically (aniso_emission.hpp): the launch takes the
// direction from the component's kind and an emission peel-off carries its probabilityForDirection. ANISO = false
// is the code as it was: those kinds are then neither launched nor weighted (upload_sources and runPhase see to it).
template <int GRID, bool ONECOMP, bool POL = false, bool ANISO = false>
struct Events {
    const Args& a;
    const Shared& sh;
    unsigned int packets = 0, detects = 0, segFill = 0, segWalk = 0, segPeel = 0;

    __device__ __forceinline__ double rho(int m, int h) const { return a.rho[(size_t)m * a.ncomp + h]; }

    // queues ray `pos`. The trace kernel enters the grid, except for Voronoi grids (kEnterInEvent): their
    // cellIndex loops over a block's site list, which costs the trace kernel more than it costs here. A
    // path found empty here (no dust system, or a Voronoi ray missing the grid) is finished here.
    // whether the queue holds references (kRayRefs): wave-uniform; known at compile time in the polarised
    // kernels, which have no continuous scattering (and no registers for both formats)
    __device__ __forceinline__ bool rayRefs() const { return !kEnterInEvent<GRID> && (POL || !a.continuous); }

    // Returns whether a ray was queued. Where the queue holds references (kRayRefs), the record is
    // {idx, flags, slot}: the trace lane finds the origin, the direction and prm through the slot, whose state
    // this visit stores (the event kernel; the continuous peel-off kernel always queues whole records)
    __device__ __forceinline__ bool emitRay(unsigned pos, const Packet& p, double dx, double dy, double dz, double prm,
                                            int idx, unsigned flags, int& vcell, int slot) {
        if (rayRefs()) {
            int4* const ref = reinterpret_cast<int4*>(a.rays) + pos;
            const unsigned mode = rayMode(flags);
            if (!a.hasDust) {  // (an empty path, as below)
                if (mode != RAY_PEEL) {
                    a.resA[idx] = 0.0;
                    if (mode == RAY_WALK && a.fuse) a.resS[idx] = 0.0;
                    if (!ONECOMP) a.resB[idx] = 0.0;
                }
                *ref = make_int4(idx, (int)RAY_NONE, slot, 0);
                return false;
            }
            *ref = make_int4(idx, (int)flags, slot, 0);
            return true;
        }
        Ray r;
        r.x = p.rx; r.y = p.ry; r.z = p.rz;
        r.dx = dx; r.dy = dy; r.dz = dz;
        r.ix = (fabs(dx) > 1e-15) ? 1.0 / dx : 0.0;
        r.iy = (fabs(dy) > 1e-15) ? 1.0 / dy : 0.0;
        r.iz = (fabs(dz) > 1e-15) ? 1.0 / dz : 0.0;
        r.s = 0;
        r.ci = r.cj = 0;
        const unsigned mode = rayMode(flags);
        int4* dst = reinterpret_cast<int4*>(a.rays + pos);
        bool entered = a.hasDust;
        unsigned nseg = 0;
        if constexpr (kEnterInEvent<GRID>) {
            if (entered) entered = Grid<GRID>::beginAt(a, r, vcell, [&](int, double, double ds) {
                if (ds > 0) { r.s += ds; nseg++; }  // outside the grid: no optical depth
                return true;
            });
            // (the trace kernel counts them with the ray's other segments: they travel in the record)
        }
        if (kEnterInEvent<GRID> && a.crossed && mode != RAY_WALK && a.hasDust) {
            if (!entered) crossedAdd(a, 0);  // (a path that misses the grid has no segments)
        }
        if (!entered) {
            if (mode != RAY_PEEL) {  // a peel-off's detection record already holds tau = 0
                a.resA[idx] = 0.0;  // FILL: tau = 0 (and no scattered luminosity); WALK: s = 0
                if (mode == RAY_WALK && a.fuse) a.resS[idx] = 0.0;
                if (!ONECOMP) a.resB[idx] = 0.0;
                if (mode == RAY_FILL && a.continuous) a.pathCnt[idx] = 0;  // an empty path: no dust segments
            }
            dst[4] = make_int4(idx, (int)RAY_NONE, 0, 0);
            return false;
        }
        double2* d2 = reinterpret_cast<double2*>(dst);
        d2[0] = make_double2(r.x, r.y);
        d2[1] = make_double2(r.z, dx);
        d2[2] = make_double2(dy, dz);
        d2[3] = make_double2(r.s, prm);
        // (the segments before the grid, for the cells-crossed histogram, in the first cell's top bits)
        dst[4] = make_int4(idx, (int)flags, r.ci | (int)(min(nseg, 7u) << kOutsideShift), r.cj);
        return true;
    }

    __device__ __forceinline__ void load(int s, Packet& p) const {
        p.rx = a.srx[s]; p.ry = a.sry[s]; p.rz = a.srz[s];
        p.kx = a.skx[s]; p.ky = a.sky[s]; p.kz = a.skz[s];
        p.L = a.sL[s]; p.Lth = a.sLth[s];
        p.ell = a.sell[s]; p.nscatt = a.snscatt[s]; p.stellar = a.sstellar[s]; p.state = a.sstate[s];
        p.rng.k0 = (uint32_t)a.seed; p.rng.k1 = (uint32_t)(a.seed >> 32); p.rng.tag = a.tag;
        p.rng.plo = a.splo[s]; p.rng.phi = a.sphi[s]; p.rng.block = a.sblock[s];
        p.rng.w2 = a.sw2[s]; p.rng.w3 = a.sw3[s]; p.rng.have = a.shave[s];
        if constexpr (POL) {
            p.sv.Q = a.sQ[s]; p.sv.U = a.sU[s]; p.sv.V = a.sV[s];
            p.sv.nx = a.snx[s]; p.sv.ny = a.sny[s]; p.sv.nz = a.snz[s];
            p.sv.pol = a.spol[s];
        }
    }
    // fresh: the slot launched a packet in this visit; its wavelength, its origin (star or dust) and its
    // termination threshold change at no other time
    __device__ __forceinline__ void store(int s, const Packet& p, bool fresh) const {
        a.srx[s] = p.rx; a.sry[s] = p.ry; a.srz[s] = p.rz;
        a.skx[s] = p.kx; a.sky[s] = p.ky; a.skz[s] = p.kz;
        a.sL[s] = p.L;
        if (fresh) { a.sLth[s] = p.Lth; a.sell[s] = p.ell; a.sstellar[s] = p.stellar; }
        a.snscatt[s] = p.nscatt; a.sstate[s] = p.state;
        a.splo[s] = p.rng.plo; a.sphi[s] = p.rng.phi; a.sblock[s] = p.rng.block;
        a.sw2[s] = p.rng.w2; a.sw3[s] = p.rng.w3; a.shave[s] = p.rng.have;
        if constexpr (POL) {
            a.sQ[s] = p.sv.Q; a.sU[s] = p.sv.U; a.sV[s] = p.sv.V;
            a.snx[s] = p.sv.nx; a.sny[s] = p.sv.ny; a.snz[s] = p.sv.nz;
            a.spol[s] = p.sv.pol;
        }
    }

    __device__ __forceinline__ int pixel(const DevInstr& ins, const Packet& p) const {
        // SingleFrameInstrument::pixelondetector (SingleFrameInstrument.cpp:130-147)
        const double xpp = -ins.sinphi * p.rx + ins.cosphi * p.ry;
        const double ypp = -ins.cosphi * ins.costheta * p.rx - ins.sinphi * ins.costheta * p.ry + ins.sintheta * p.rz;
        const double xp = ins.cospa * xpp - ins.sinpa * ypp;
        const double yp = ins.sinpa * xpp + ins.cospa * ypp;
        const int i = static_cast<int>(floor((xp - ins.xpmin) / ins.xpsiz));
        const int j = static_cast<int>(floor((yp - ins.ypmin) / ins.ypsiz));
        return (i < 0 || i >= ins.nx || j < 0 || j >= ins.ny) ? -1 : i + ins.nx * j;
    }

    // weight of the scattering peel-off towards instrument `ins` (MonteCarloSimulation.cpp:319-363,
    // unpolarized; Henyey-Greenstein value DustMix.cpp:665-669); false aborts the peel-off
    __device__ __forceinline__ bool peelWeight(const DevInstr& ins, const Packet& p, double kx, double ky, double kz,
                                               double& I) const {
        const double cosalpha = kx * ins.kobs[0] + ky * ins.kobs[1] + kz * ins.kobs[2];
        if (ONECOMP) {
            const double g = sh.g[p.ell];
            const double t = 1.0 + g * g - 2 * g * cosalpha;
            I = 0.0 + (1.0 * ((1.0 - g) * (1.0 + g) / sqrt(t * t * t))) * 1.0;
            return true;
        }
        const int m = Grid<GRID>::whichcell(a, sh, p.rx, p.ry, p.rz);
        if (m == -1) return false;
        double sum = 0;
        for (int h = 0; h < a.ncomp; h++) sum += sh.ksca[h * a.nlambda + p.ell] * rho(m, h);
        if (sum <= 0) return false;
        I = 0;
        for (int h = 0; h < a.ncomp; h++) {
            const double wv = sh.ksca[h * a.nlambda + p.ell] * rho(m, h) / sum;
            const double g = sh.g[h * a.nlambda + p.ell];
            const double t = 1.0 + g * g - 2 * g * cosalpha;
            I += (wv * ((1.0 - g) * (1.0 + g) / sqrt(t * t * t))) * 1.0;
        }
        return true;
    }

    // the cell of the peel-off round, or -1 where peeloffscattering aborts (MonteCarloSimulation.cpp:332-337): no
    // cell, or no scattering dust in it; m is whichcell of the packet's position
    __device__ __forceinline__ int peelCell(const Packet& p, int m) const {
        if (m == -1) return -1;
        double sum = 0;
        for (int h = 0; h < a.ncomp; h++) sum += sh.ksca[h * a.nlambda + p.ell] * rho(m, h);
        return sum <= 0 ? -1 : m;
    }

    // The same with polarisation (MonteCarloSimulation.cpp:347-360): I and, as PhotonPackage::setPolarized leaves
    // them, Q/I, U/I, V/I of the peel-off towards `ins` of a packet with direction k and Stokes vector sv, summed
    // over the components with the weights wv[h] phaseFunctionValue; m is the round's peelCell (the packet has not
    // moved since), so the grid is searched once per round and not once per instrument
    __device__ __forceinline__ void peelWeightPol(const DevInstr& ins, const Packet& p, int m, double kx, double ky,
                                                  double kz, const PolStokes& sv, double& I, DetPol& q) const {
        // DistantInstrument::bfky (DistantInstrument.cpp:47-49)
        const double yx = -ins.cosphi * ins.costheta * ins.cospa - ins.sinphi * ins.sinpa;
        const double yy = -ins.sinphi * ins.costheta * ins.cospa + ins.cosphi * ins.sinpa;
        const double yz = +ins.sintheta * ins.cospa;
        I = 0;
        q.Q = 0; q.U = 0; q.V = 0;
        if (ONECOMP) {
            const PolMix mx = polMixAt(a.polTab, a.ncomp, a.nlambda, a.polNtheta, 0, p.ell);
            polPeelAdd(mx, 1.0, sv, kx, ky, kz, ins.kobs[0], ins.kobs[1], ins.kobs[2], yx, yy, yz, I, q.Q, q.U, q.V);
        } else {
            double sum = 0;
            for (int h = 0; h < a.ncomp; h++) sum += sh.ksca[h * a.nlambda + p.ell] * rho(m, h);
            for (int h = 0; h < a.ncomp; h++) {
                const double wv = sh.ksca[h * a.nlambda + p.ell] * rho(m, h) / sum;
                const PolMix mx = polMixAt(a.polTab, a.ncomp, a.nlambda, a.polNtheta, h, p.ell);
                polPeelAdd(mx, wv, sv, kx, ky, kz, ins.kobs[0], ins.kobs[1], ins.kobs[2], yx, yy, yz, I, q.Q, q.U, q.V);
            }
        }
        polPeelNormalize(I, q.Q, q.U, q.V);
    }

    // Instrument::detect without a dust system (tau = 0): FullInstrument then holds only the
    // transparent arrays (FullInstrument.cpp:58-60, 115-120)
    __device__ __forceinline__ void detectNow(const DevInstr& ins, const Packet& p, double Lp, int l) {
        detects++;
        if (ins.kind != SKIRT_INSTR_FRAME) atomicAddF64(a.tally + ins.sedBase + p.ell, Lp);
        if (l >= 0 && ins.kind != SKIRT_INSTR_SED) atomicAddF64(frameAt(a, ins, p.ell, l, 0), Lp);
    }

    // SpecialFunctions::LambertW1 (SpecialFunctions.cpp:579-626), the W_{-1} branch; as the host's
    // lambertW1 (host/geometry.cpp), whose argument checks the callers here never fail
    __device__ static double lambertW1(double z) {
        const double eps = 1.0e-12;
        const double em1 = 0.3678794411714423215955237701614608;
        if (z == 0.0) return -kDblMax;
        const double q = z + em1;
        const double r = -sqrt(q);
        const double t8 = -8.401032217523977370984161688514 +
                          r * (12.250753501314460424 + r * (-18.100697012472442755 + r * 27.029044799010561650));
        const double t5 = 3.066858901050631912893148922704 +
                          r * (-4.175335600258177138854984177460 + r * (5.858023729874774148815053846119 + r * t8));
        const double t1 = 2.331643981597124203363536062168 +
                          r * (-1.812187885639363490240191647568 +
                               r * (1.936631114492359755363277457668 + r * (-2.353551201881614516821543561516 + r * t5)));
        const double w0 = -1.0 + r * t1;
        if (q < 3.0e-3) return w0;
        double w;
        if (z < -1e-6) {
            w = w0;
        } else {
            const double l1 = log(-z);
            const double l2 = log(-l1);
            w = l1 - l2 + l2 / l1;
        }
        for (int i = 0; i < 10; i++) {  // Halley iteration
            const double e = exp(w);
            double t = w * e - z;
            const double p = w + 1.0;
            t /= e * p - 0.5 * (p + 1.0) * t / p;
            w -= t;
            if (fabs(t) < eps * (1.0 + fabs(w))) break;
        }
        return w;
    }

    // ExpDiskGeometry::randomR / randomz and SepAxGeometry::generatePosition (R, phi = 2 pi u, z;
    // Position(R, phi, z, CYLINDRICAL)); gp = {hR, hz, Rmax, zmax, Rmin, rho0, 0, kind}
    __device__ __forceinline__ static void expDiskPosition(PacketRng& rng, const double* gp, double& x, double& y,
                                                           double& z) {
        const double hR = gp[0], hz = gp[1], Rmax = gp[2], zmax = gp[3], Rmin = gp[4];
        double R, X;
        do {
            X = rng.uniform();
            R = hR * (-1.0 - lambertW1((X - 1.0) / M_E));
        } while ((Rmax > 0.0 && R >= Rmax) || R <= Rmin);
        const double phi = 2.0 * M_PI * rng.uniform();
        double zz;
        do {
            X = rng.uniform();
            zz = (X <= 0.5) ? hz * log(2.0 * X) : -hz * log(2.0 * (1.0 - X));
        } while (zmax > 0.0 && fabs(zz) >= zmax);
        x = R * cos(phi);
        y = R * sin(phi);
        z = zz;
    }

    // Random::direction() (Random.cpp:179-184): theta = acos(2u-1), phi = 2 pi u', evaluated as
    // cos(theta) = 2u-1, sin(theta) = sqrt(1-cos^2) and sin/cos(2 pi u') = sinpi/cospi(2u') -- the
    // same values to rounding, without acos or a large-argument reduction. The reference's 1e-8
    // pole cut-offs in Direction(theta, phi) are never reached by a deviate in (0,1).
    __device__ __forceinline__ static void isotropic(PacketRng& rng, double& x, double& y, double& z) {
        const double ct = 2.0 * rng.uniform() - 1.0;
        const double u = rng.uniform();
        const double st = sqrt((1.0 - ct) * (1.0 + ct));
        double sp, cp;
        sincospi(2.0 * u, &sp, &cp);
        x = st * cp; y = st * sp; z = ct;
    }

    // simulatescattering: DustSystem::randomMixForPosition + DustMix::scatteringDirectionAndPolarization
    // (HG, DustMix.cpp:609-613) + Random::direction(k, costheta) (Random.cpp:188-222)
    __device__ __forceinline__ void scatter(Packet& p) const {
        scatterIn(p, ONECOMP ? -1 : Grid<GRID>::whichcell(a, sh, p.rx, p.ry, p.rz));
    }
    // the same with whichcell of the packet's position given (not looked at with one component)
    __device__ __forceinline__ void scatterIn(Packet& p, int m) const {
        int hmix = 0;
        if (!ONECOMP) {
            if (m >= 0) {
                double Xv[9];
                Xv[0] = 0.0;
                for (int h = 0; h < a.ncomp; h++) Xv[h + 1] = Xv[h] + sh.ksca[h * a.nlambda + p.ell] * rho(m, h);
                const double norm = Xv[a.ncomp];
                const double X = p.rng.uniform();
                for (int h = 1; h < a.ncomp; h++)
                    if (Xv[h] / norm <= X) hmix = h;
            }
        }
        if constexpr (POL) {  // DustMix::scatteringDirectionAndPolarization, polarized (DustMix.cpp:586-606)
            const PolMix mx = polMixAt(a.polTab, a.ncomp, a.nlambda, a.polNtheta, hmix, p.ell);
            PolDrawsStream draws{p.rng};
            polScatter(mx, p.kx, p.ky, p.kz, p.sv, draws);
            p.nscatt++;
            return;
        }
        const double g = sh.g[hmix * a.nlambda + p.ell];
        double nx, ny, nz;
        if (fabs(g) < 1e-6) {
            isotropic(p.rng, nx, ny, nz);
        } else {
            const double f = ((1.0 - g) * (1.0 + g)) / (1.0 - g + 2.0 * g * p.rng.uniform());
            const double costheta = (1.0 + g * g - f * f) / (2.0 * g);
            double sinphi, cosphi;  // phi = 2 pi u (Random.cpp:190), as sinpi/cospi(2u)
            sincospi(2.0 * p.rng.uniform(), &sinphi, &cosphi);
            const double sintheta = sqrt(fabs((1.0 - costheta) * (1.0 + costheta)));
            const double kx = p.kx, ky = p.ky, kz = p.kz;
            if (kz > 0.99999) { nx = cosphi * sintheta; ny = sinphi * sintheta; nz = costheta; }
            else if (kz < -0.99999) { nx = cosphi * sintheta; ny = sinphi * sintheta; nz = -costheta; }
            else {
                const double root = sqrt((1.0 - kz) * (1.0 + kz));
                nx = sintheta / root * (-kx * kz * cosphi + ky * sinphi) + kx * costheta;
                ny = -sintheta / root * (ky * kz * cosphi + kx * sinphi) + ky * costheta;
                nz = root * sintheta * cosphi + kz * costheta;
            }
        }
        p.nscatt++;
        p.kx = nx; p.ky = ny; p.kz = nz;
    }

    // false when no packet results (wavelength without luminosity, or a selected component without
    // luminosity)
    __device__ __forceinline__ bool launch(Packet& p, unsigned long long idx) {
        return a.phase == SKIRT_PHASE_STELLAR ? launchStellar(p, idx) : launchCell(p, idx);
    }

    // the launch of dodustemissionchunk (biased cell choice, PanMonteCarloSimulation.cpp:296-325) and of
    // dodustselfabsorptionchunk (natural choice, :207-216): a cell, a uniform position in its box
    // (Random::position, Random.cpp:226-234), an isotropic direction; a dust packet (stellar = -1)
    __device__ __forceinline__ bool launchCell(Packet& p, unsigned long long idx) {
        const int ell = (int)(idx / a.npp);
        const double Ltot = a.cellLtot[ell];
        if (!(Ltot > 0)) return false;  // the chunk emits nothing at this wavelength
        packets++;
        const double L0 = Ltot / (double)a.npp;
        p.Lth = L0 / a.minWeightReduction;
        p.rng.start(a.seed, a.tag, idx);
        p.ell = ell;
        const int N = a.ncells;
        const double* cdf = a.cellCdf + (size_t)ell * (N + 1);
        const int* guide = a.cellGuide + (size_t)ell * (N + 1);
        const double X = p.rng.uniform();
        int m;
        double L = L0;
        if (a.phase == SKIRT_PHASE_DUST_EMISSION) {
            const double xi = a.cellBias;
            if (X < xi) m = max(0, min(N - 1, static_cast<int>(N * X / xi)));
            else m = locateGuided(cdf, guide, N, (X - xi) / (1 - xi));
            const double Lmean = Ltot / N;
            const double weight = 1.0 / (1 - xi + xi * Lmean / a.cellLv[(size_t)ell * N + m]);
            L = L0 * weight;
        } else {
            m = locateGuided(cdf, guide, N, X);
        }
        if (GRID == SKIRT_GRID_VORONOI) m = a.devCell[m];  // the Voronoi arrays are in device order
        if constexpr (GRID == SKIRT_GRID_CYLINDER2D) {
            // Cylinder2DDustGrid::randomPositionInCell: three deviates in the order R, phi, z
            const double* Rv = sh.mesh;
            const double* zv = Grid<SKIRT_GRID_CYLINDER2D>::zBorders(a, sh);
            const int i = m / a.nz, k = m % a.nz;
            const double R = Rv[i] + (Rv[i + 1] - Rv[i]) * p.rng.uniform();
            const double phi = 2.0 * M_PI * p.rng.uniform();
            p.rz = zv[k] + (zv[k + 1] - zv[k]) * p.rng.uniform();
            p.rx = R * cos(phi);
            p.ry = R * sin(phi);
        } else if constexpr (GRID == SKIRT_GRID_SPHERE1D) {
            // Sphere1DDustGrid::randomPositionInCell: Random::direction() (two deviates), then r uniform in the shell
            double ux, uy, uz;
            isotropic(p.rng, ux, uy, uz);
            const double* rv = sh.mesh;
            const double rr = rv[m] + (rv[m + 1] - rv[m]) * p.rng.uniform();
            p.rx = rr * ux; p.ry = rr * uy; p.rz = rr * uz;
        } else if constexpr (GRID == SKIRT_GRID_SPHERE2D) {
            // Sphere2DDustGrid::randomPositionInCell: three deviates in the order r, theta, phi
            const double* rv = sh.mesh;
            const double* thv = Grid<SKIRT_GRID_SPHERE2D>::thetaBorders(a, sh);
            const int i = m / a.nz, k = m % a.nz;
            const double ris = rv[i] * rv[i];
            const double ri1s = rv[i + 1] * rv[i + 1];
            const double rr = sqrt(ris + (ri1s - ris) * p.rng.uniform());
            const double theta = thv[k] + (thv[k + 1] - thv[k]) * p.rng.uniform();
            const double phi = 2.0 * M_PI * p.rng.uniform();
            const double st = sin(theta);
            p.rx = rr * st * cos(phi);
            p.ry = rr * st * sin(phi);
            p.rz = rr * cos(theta);
        } else {
            double b[6];
            cellBox(m, b);
            // VoronoiMesh::randomPosition: points in the enclosing box until one lies in the cell
            for (int trial = 0; trial < (GRID == SKIRT_GRID_VORONOI ? 10000 : 1); trial++) {
                const double x = p.rng.uniform();
                const double y = p.rng.uniform();
                const double z = p.rng.uniform();
                p.rx = b[0] + x * (b[3] - b[0]);
                p.ry = b[1] + y * (b[4] - b[1]);
                p.rz = b[2] + z * (b[5] - b[2]);
                if (GRID != SKIRT_GRID_VORONOI || Grid<SKIRT_GRID_VORONOI>::closestTo(a, p.rx, p.ry, p.rz, m)) break;
            }
        }
        isotropic(p.rng, p.kx, p.ky, p.kz);
        p.L = L;
        p.nscatt = 0;
        p.stellar = -1;
        return true;
    }

    // NR::locate_clip over a table in global memory
    __device__ static __forceinline__ int locateClipGlobal(const double* v, int n, double q) {
        if (q < v[0]) return 0;
        int jl = -1, ju = n - 1;
        while (ju - jl > 1) {
            const int jm = (ju + jl) >> 1;
            if (q < v[jm]) ju = jm;
            else jl = jm;
        }
        return jl;
    }

    // the box of cell m (CartesianDustGrid::box, TreeDustGrid::getnode(m)->extent()): reference cell
    // numbers, except the Voronoi grid's device numbers
    __device__ __forceinline__ void cellBox(int m, double (&b)[6]) const {
        if (GRID == SKIRT_GRID_CARTESIAN) {
            const double* xv = sh.mesh;
            const double* yv = xv + a.nx + 1;
            const double* zv = yv + a.ny + 1;
            const int i = m / (a.nz * a.ny), j = (m / a.nz) % a.ny, k = m % a.nz;
            b[0] = xv[i]; b[1] = yv[j]; b[2] = zv[k]; b[3] = xv[i + 1]; b[4] = yv[j + 1]; b[5] = zv[k + 1];
        } else if (GRID == SKIRT_GRID_VORONOI) {
            for (int q = 0; q < 6; q++) b[q] = a.cellBbox[6 * (size_t)m + q];
        } else {
            const double* bx = a.box + 6 * (size_t)a.cellNode[m];
            for (int q = 0; q < 6; q++) b[q] = bx[q];
        }
    }

    // Geometry::generatePosition of source component h (gp: its row of the device geometry table, the kind in
    // its eighth word), shared by launchStellar and skirt_mcrt_sample_positions
    __device__ __forceinline__ static bool launchPosition(const double* gp, const double* geomTable, int h,
                                                          PacketRng& rng, double& x, double& y, double& z) {
        // the six closed-form kinds (geom_sample.hpp), the torus and the cone (the rest of whose constants start
        // their geom_table row) apart from the other four: dispatched this way every event kernel keeps its three
        // waves per SIMD (profiles/geom_first.txt). False when a rejection loop reached its cap.
        if constexpr (ANISO) {
            if ((int)gp[7] >= SKIRT_GEOM_NETZER) {
                anisoPositionOf((int)gp[7], gp[0], rng, x, y, z);
                return true;
            }
        }
        if ((int)gp[7] >= SKIRT_GEOM_TORUS) {
            return geomConePosition(gp, geomTable + (size_t)kSersicTable * h, rng, x, y, z);
        } else if ((int)gp[7] >= SKIRT_GEOM_SHELL) {
            return geomPositionOf((int)gp[7], gp, nullptr, rng, x, y, z);
        } else if ((int)gp[7] == SKIRT_GEOM_POINT) {
            x = 0.0; y = 0.0; z = 0.0;  // PointGeometry::generatePosition: no draws
        } else if ((int)gp[7] == SKIRT_GEOM_EXPDISK) {
            expDiskPosition(rng, gp, x, y, z);
        } else if ((int)gp[7] == SKIRT_GEOM_SERSIC) {
            // SersicGeometry::randomradius (SersicFunction::inversemass: locate_clip + log-log
            // interpolation of the cumulative mass table) and SpheGeometry::generatePosition
            const double* sv = geomTable + (size_t)kSersicTable * h;
            const double* Mv = sv + kSersicTable / 2;
            constexpr int Ns = kSersicTable / 2;
            const double M = rng.uniform();
            double sr;
            if (M <= Mv[0]) sr = sv[0];
            else if (M >= Mv[Ns - 1]) sr = sv[Ns - 1];
            else {
                int jl = -1, ju = Ns - 1;  // NR::locate_clip
                while (ju - jl > 1) { const int jm = (ju + jl) >> 1; if (M < Mv[jm]) ju = jm; else jl = jm; }
                sr = interpolateLogLog(M, Mv[jl], Mv[jl + 1], sv[jl], sv[jl + 1]);
            }
            const double rr = gp[0] * sr;
            double ux, uy, uz;
            isotropic(rng, ux, uy, uz);
            x = rr * ux; y = rr * uy; z = rr * uz;
        } else {
            // PlummerGeometry::randomradius (t = u^(1/3)) and SpheGeometry::generatePosition
            const double c = gp[0];
            const double t = cbrt(rng.uniform());
            const double rr = c * t / sqrt((1.0 - t) * (1.0 + t));
            double ux, uy, uz;
            isotropic(rng, ux, uy, uz);
            x = rr * ux; y = rr * uy; z = rr * uz;
        }
        return true;
    }

    // GeometricStellarComp::launch's direction for a packet leaving (x, y, z) of the component of row gp:
    // _geom->generateDirection for the anisotropic kinds (netzer: the table behind the rows, upload_sources),
    // Random::direction() for the others; shared by launchStellar and skirt_mcrt_sample_launches
    __device__ __forceinline__ static void launchDirection(const double* gp, const double* netzer, PacketRng& rng,
                                                           double x, double y, double z, double& kx, double& ky,
                                                           double& kz) {
        if constexpr (ANISO) {
            if ((int)gp[7] >= SKIRT_GEOM_NETZER) {
                anisoDirectionOf((int)gp[7], gp[0], netzer, rng, x, y, z, kx, ky, kz);
                return;
            }
        }
        isotropic(rng, kx, ky, kz);
    }
    // PhotonPackage::launchEmissionPeelOff's factor for a stellar packet: the component's probabilityForDirection
    // towards the instrument (1 for an isotropic kind)
    __device__ __forceinline__ double emissionWeight(const Packet& p, const DevInstr& ins) const {
        if constexpr (ANISO) {
            if (p.stellar >= 0)
                return emissionProbability(a.geomParam + 8 * p.stellar, p.rx, p.ry, p.rz, ins.kobs[0], ins.kobs[1],
                                           ins.kobs[2]);
        }
        return 1.0;
    }
    // the same for the component of row gp, a position and a direction; shared with skirt_mcrt_sample_launches
    __device__ __forceinline__ static double emissionProbability(const double* gp, double x, double y, double z,
                                                                 double kx, double ky, double kz) {
        if constexpr (ANISO) {
            if ((int)gp[7] >= SKIRT_GEOM_NETZER) return anisoProbabilityOf((int)gp[7], gp[0], x, y, z, kx, ky, kz);
        }
        return 1.0;
    }

    // StellarSystem::launch + GeometricStellarComp::launch + PlummerGeometry sampling (see below)
    __device__ __forceinline__ bool launchStellar(Packet& p, unsigned long long idx) {
        const int ell = (int)(idx / a.npp);
        const double L0 = a.lumtot[ell] / (double)a.npp;
        if (!(L0 > 0)) return false;  // dostellaremissionchunk skips such wavelengths
        packets++;
        p.Lth = L0 / a.minWeightReduction;
        p.rng.start(a.seed, a.tag, idx);
        p.ell = ell;
        int h = 0;
        double L = L0;
        const int N = a.nstar;
        if (N > 1) {
            const double X = p.rng.uniform();
            const double xi = a.emissionBias;
            if (X < xi) h = max(0, min(N - 1, static_cast<int>(N * X / xi)));
            else {
                const double* Xv = a.cdf + (size_t)ell * (N + 1);
                const double q = (X - xi) / (1.0 - xi);
                if (!(q < Xv[0])) {
                    int lo = -1, hi = N;
                    while (hi - lo > 1) { const int jm = (hi + lo) >> 1; if (q < Xv[jm]) hi = jm; else lo = jm; }
                    h = lo;
                }
            }
            const double Lh = a.lum[(size_t)h * a.nlambda + ell];
            if (!(Lh > 0)) return false;
            const double Lmean = a.lumtot[ell] / N;
            L = L0 * (1.0 / (1.0 - xi + xi * Lmean / Lh));
        }
        if (!launchPosition(a.geomParam + 8 * h, a.geomTable, h, p.rng, p.rx, p.ry, p.rz)) {
            atomicOr(a.error, ERR_GEOM);  // a torus or cone whose rejection loop reached its cap: SKIRT_ERR_NUMERIC
            return false;
        }
        // the emission direction: Random::direction(), or the component's generateDirection (ANISO)
        launchDirection(a.geomParam + 8 * h, a.geomParam + 8 * a.nstar, p.rng, p.rx, p.ry, p.rz, p.kx, p.ky, p.kz);
        p.L = L;
        p.nscatt = 0;
        p.stellar = h;
        return true;
    }

    // decideFill's termination threshold: Lth once the packet has scattered minScatt times
    __device__ __forceinline__ double fillThreshold(const Packet& p) const { return p.nscatt >= a.minScatt ? p.Lth : 0.0; }

    // simulatepropagation part 1 where decideFill left off (FILL_FALLBACK): Random::exponcutoff draws until
    // a deviate falls inside the path, then the composite biasing's weight
    __device__ __forceinline__ double exponCutoffAgain(Packet& p, double taupath) const {
        const double norm = 1.0 - exp(-taupath);
        double x = -log(1.0 - p.rng.uniform() * norm);
        while (x > taupath) x = -log(1.0 - p.rng.uniform() * norm);
        if (a.xi != 0.0) p.L = fillBiasWeight(p.L, x, taupath, a.xi);
        return x;
    }
};

// peel-off set queued by a slot in this iteration
enum PeelKind : int { PEEL_NONE = 0, PEEL_EMISSION = 1, PEEL_SCATTER = 2 };

// Block-wide reservation on N shared counters of one type: every thread of the block calls it with its counts
// c (any may be 0); one atomic per counter per block (a device-wide counter serializes its atomics, so one per
// block instead of one per wave), issued by the first lane of wave q for counter q, returns each thread's
// first index in r. Wave totals and the block's bases go through `scratch` (static LDS,
// N * (kBlock / 64) + N words).
template <class T, int N>
__device__ __forceinline__ void blockReserve(T* const (&ctr)[N], const T (&c)[N], T (&r)[N], unsigned long long* scratch) {
    static_assert(kBlock >= 64 * N, "blockReserve needs one wave per counter");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int W = kBlock / 64;
    T in[N];
#pragma unroll
    for (int q = 0; q < N; q++) in[q] = c[q];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        T v[N];
#pragma unroll
        for (int q = 0; q < N; q++) v[q] = __shfl_up(in[q], off);
        if (lane >= off) {
#pragma unroll
            for (int q = 0; q < N; q++) in[q] += v[q];
        }
    }
    if (lane == 63) {
#pragma unroll
        for (int q = 0; q < N; q++) scratch[q * W + wave] = in[q];
    }
    __syncthreads();
    T w[N] = {}, t[N] = {};
#pragma unroll
    for (int ww = 0; ww < W; ww++) {
#pragma unroll
        for (int q = 0; q < N; q++) {
            const T sv = (T)scratch[q * W + ww];
            if (ww < wave) w[q] += sv;
            t[q] += sv;
        }
    }
#pragma unroll
    for (int q = 0; q < N; q++)
        if (threadIdx.x == 64 * q) scratch[N * W + q] = t[q] ? atomicAdd(ctr[q], t[q]) : T(0);
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; q++) r[q] = (T)scratch[N * W + q] + w[q] + in[q] - c[q];
    __syncthreads();  // the scratch words are reused by the next call
}

// Global packet index of the j-th packet of this call. A sharded call (IdenticalAssigner,
// IdenticalAssigner.cpp:37-58: every process runs its block of chunks at every wavelength) shoots
// packets [sliceLo, sliceLo + sliceCnt) of each wavelength; the Philox stream is keyed on the global
// index, so the packets are the same whatever the number of ranks.
__device__ __forceinline__ unsigned long long globalPacket(const Args& a, unsigned long long j) {
    if (a.sliceCnt == a.npp) return j;
    const unsigned long long ell = j / a.sliceCnt;
    return ell * a.npp + a.sliceLo + (j - ell * a.sliceCnt);
}

template <int GRID, bool ONECOMP, bool POL = false, bool ANISO = false>
__global__ void __launch_bounds__(kBlock) SKIRT_EVENT_ATTR_FOR(GRID, ONECOMP, POL, ANISO) eventKernel(const Args a) {
    __shared__ unsigned long long resv[4 * (kBlock / 64) + 4];
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (blockIdx.x == 0 && threadIdx.x == 0) CTR(a.ctr, CTR_PULL) = 0;
    if (!a.init && CTR(a.ctr, CTR_ACTIVE + a.parity) == 0) return;  // an iteration after the end of the phase
    Shared sh = stageTables(a, lds, gridParts<GRID>() | STAGE_OPTICS | STAGE_INSTR);
    Events<GRID, ONECOMP, POL, ANISO> E{a, sh};
    const int lane = threadIdx.x & 63;
    const unsigned long long total = a.end - a.first;
    const unsigned int nwork = a.init ? (unsigned)a.nslots : CTR(a.ctr, CTR_ACTIVE + a.parity);
    const int* actIn = a.act[a.parity];
    int* actOut = a.act[1 - a.parity];
    const unsigned int stride = gridDim.x * blockDim.x;
    // every lane of a wave runs the same number of rounds (wave-collective claims and appends below)
    const unsigned int rounds = (nwork + stride - 1) / stride;
    // the active-list entry of the lane's next round is loaded a round ahead, so a round's first round trip
    // is its slot's state (and the trace result, loaded with it)
    const unsigned int w0 = blockIdx.x * blockDim.x + threadIdx.x;
    int slotNext = (w0 < nwork) ? (a.init ? (int)w0 : actIn[w0]) : 0;
    for (unsigned int round = 0; round < rounds; round++) {
        const unsigned int w = round * stride + w0;
        const bool valid = w < nwork;
        const int slot = slotNext;
        const unsigned int wn = w + stride;
        if (round + 1 < rounds) slotNext = (wn < nwork) ? (a.init ? (int)wn : actIn[wn]) : 0;
        Packet p;
        p.state = S_NEW;
        double resA = 0.0, resB = 0.0, resS = -1.0;
        int vcell = kNoCell;  // Voronoi: the cell of the packet's position, while it stays there
        if (valid && !a.init) {
            E.load(slot, p);
            resA = a.resA[slot];
            if (!ONECOMP) resB = a.resB[slot];
            if (a.fuse) {
                resS = a.resS[slot];
                if (p.state == S_WALK) resA = resS;  // (a queued WALK ray's distance)
            }
            if (kEnterInEvent<GRID>) vcell = a.svcell[slot];
        }
        int peel = PEEL_NONE;
        unsigned mainMode = RAY_NONE;
        double mainParam = 0;
        double ox = 0, oy = 0, oz = 0;  // direction before scattering (peel-off weights)
        PolStokes osv;                  // and the Stokes vector (POL)
        int pcell = -1;                 // and the cell of the peel-off round (POL, several components)
        if constexpr (POL) polSetUnpolarized(osv);
        if (valid && !a.init) {
            if (p.state == S_FILL) {
                // end of fillOpticalDepth + simulateescapeandabsorption; termination; simulatepropagation
                const double taupath = resA;
                FillDrawsStream draws{p.rng};
                double tauint;
                int st = decideFill<ONECOMP>(taupath, p.L, resB, ONECOMP ? sh.alb[p.ell] : 0.0, E.fillThreshold(p), a.xi,
                                             draws, tauint);
                if (st == FILL_FALLBACK) {
                    if (taupath < 0.0 || isnan(taupath) || isinf(taupath)) {
                        atomicOr(a.error, ERR_TAU);
                        st = FILL_TERMINATED;
                    } else {
                        tauint = E.exponCutoffAgain(p, taupath);
                        st = tauint > 0 ? FILL_WALK : FILL_NO_WALK;
                    }
                    resS = -1.0;  // (what the lane of a fused ray left there)
                }
                if (st == FILL_TERMINATED) {
                    p.state = S_NEW;
                } else {
                    p.state = S_WALK;
                    // a fused ray's lane walked on to the interaction point, unless it fell back
                    if (st == FILL_WALK && resS >= 0.0) resA = resS;
                    else if (st == FILL_WALK) { mainMode = RAY_WALK; mainParam = tauint; }
                    else resA = 0.0;  // no walk: the interaction point is where the packet is
                }
            }
            if (p.state == S_WALK && mainMode == RAY_NONE) {
                // propagate to the interaction point; peel-off round; scatter; next FILL
                const double s = resA;
                vcell = kNoCell;  // the packet moves
                p.rx = p.rx + s * p.kx;
                p.ry = p.ry + s * p.ky;
                p.rz = p.rz + s * p.kz;
                // peeloffscattering, unless the continuous peel-off replaces it (MonteCarloSimulation.cpp:291)
                bool ok = a.ninstr > 0 && a.peel && !a.continuous;
                int scell = -1;  // POL, several components: the grid is searched once for the round and the scattering
                if constexpr (POL) {
                    if (!ONECOMP) {
                        scell = Grid<GRID>::whichcell(a, sh, p.rx, p.ry, p.rz);
                        if (ok) { pcell = E.peelCell(p, scell); ok = pcell >= 0; }
                    }
                    osv = p.sv;
                } else {
                    if (ok && !ONECOMP) { double I; ok = E.peelWeight(sh.instr[0], p, p.kx, p.ky, p.kz, I); }
                }
                if (ok) { peel = PEEL_SCATTER; ox = p.kx; oy = p.ky; oz = p.kz; }
                if constexpr (POL && !ONECOMP) E.scatterIn(p, scell);
                else E.scatter(p);
                mainMode = RAY_FILL;
                mainParam = p.L;
                p.state = S_FILL;
            }
        }
        // slots without a packet claim the next global packet indices (one atomic per block)
        bool need = valid && p.state == S_NEW && mainMode == RAY_NONE;
        bool fresh = false;  // the slot launches a packet in this visit (Events::store)
        while (__syncthreads_or(need)) {
            unsigned long long* const ctrs[1] = {a.claim};
            const unsigned long long cnt[1] = {need ? 1ull : 0ull};
            unsigned long long res[1];
            blockReserve(ctrs, cnt, res, resv);
            const unsigned long long idx = res[0];
            if (need) {
                if (idx >= total) need = false;  // exhausted: the slot retires
                else if (E.launch(p, globalPacket(a, a.first + idx))) {
                    vcell = kNoCell;  // a new position
                    fresh = true;
                    if constexpr (POL) polSetUnpolarized(p.sv);  // PhotonPackage::launch
                    if (!(p.L > 0) && !a.crossed) {
                        // a zero-weight dust packet (a cell without emission drawn uniformly): every
                        // tally it would touch receives 0, so it ends here -- unless the cells-crossed
                        // statistics are on: the reference still traces its paths (dodustemissionchunk,
                        // PanMonteCarloSimulation.cpp:316-329), which count in ds_crossed
                    } else if (a.hasDust) {
                        peel = (a.ninstr > 0 && a.peel) ? PEEL_EMISSION : PEEL_NONE;
                        mainMode = RAY_FILL;
                        mainParam = p.L;
                        p.state = S_FILL;
                        need = false;
                    } else {
                        // no dust system: tau = 0 for every peel-off and the packet ends here
                        for (int i = 0; i < a.ninstr; i++) {
                            const DevInstr& ins = sh.instr[i];
                            const int l = ins.kind == SKIRT_INSTR_SED ? -1 : E.pixel(ins, p);
                            if (ins.kind == SKIRT_INSTR_FRAME && l < 0) continue;
                            if constexpr (ANISO) E.detectNow(ins, p, p.L * E.emissionWeight(p, ins), l);
                            else E.detectNow(ins, p, p.L, l);
                        }
                    }
                }
            }
        }
        // rays this lane queues: its peel-offs and its next FILL/WALK ray
        int nray = 0;
        if (peel != PEEL_NONE) {
            for (int i = 0; i < a.ninstr; i++) {
                const DevInstr& ins = sh.instr[i];
                if (ins.kind == SKIRT_INSTR_FRAME && E.pixel(ins, p) < 0) continue;
                nray++;
            }
        }
        if (mainMode != RAY_NONE) nray++;
        // the queue space of the block's rays, the slots staying active and the detection records of
        // the peel-offs: one atomic each per block
        const bool active = mainMode != RAY_NONE;
        const int npeel = nray - (mainMode != RAY_NONE ? 1 : 0);
        // a WALK ray goes to the top of the queue (Args::walkBack)
        const bool back = a.walkBack && mainMode == RAY_WALK;
        unsigned int pos, apos, dpos, wpos;
        {
            unsigned* const ctrs[4] = {CTRP(a.ctr, CTR_RAYS + a.parity), CTRP(a.ctr, CTR_ACTIVE + (1 - a.parity)),
                                       CTRP(a.ctr, CTR_DET + a.parity), CTRP(a.ctr, CTR_WALK + a.parity)};
            const unsigned cnt[4] = {(unsigned)nray - (back ? 1u : 0u), active ? 1u : 0u, (unsigned)npeel, back ? 1u : 0u};
            unsigned res[4];
            blockReserve(ctrs, cnt, res, resv);
            pos = res[0]; apos = res[1]; dpos = res[2]; wpos = res[3];
        }
        // the queue holds rayCap records (ensurePool sizes it for the slots' most rays per iteration): a
        // lane whose records would fall outside it writes none and fails the phase (ERR_QUEUE); the trace
        // kernel checks that the front and the WALK region do not meet
        if ((unsigned long long)pos + (unsigned)(nray - (back ? 1 : 0)) > (unsigned long long)a.rayCap ||
            (back && wpos >= (unsigned)a.rayCap) ||
            (unsigned long long)dpos + (unsigned)npeel > (unsigned long long)(a.rayCap - a.nslots)) {
            atomicOr(a.error, ERR_QUEUE);
            nray = 0;
        }
        int inext = 0;  // next instrument to consider for a peel-off
        int fillAt = -1;  // where the lane's FILL ray was queued, if it enters the grid
        for (int k = 0; k < nray; k++) {
            double dx, dy, dz, prm;
            int idx;
            unsigned flags, at;
            if (k < npeel) {
                int i = inext, l;
                while (true) {  // the next instrument that receives this peel-off
                    const DevInstr& ins = sh.instr[i];
                    l = ins.kind == SKIRT_INSTR_SED ? -1 : E.pixel(ins, p);
                    if (ins.kind == SKIRT_INSTR_FRAME && l < 0) { i++; continue; }
                    break;
                }
                inext = i + 1;
                const DevInstr& ins = sh.instr[i];
                double Lp = p.L;
                unsigned cat, level = 0;
                DetPol dq{0.0, 0.0, 0.0};  // (an emission peel-off is unpolarized)
                if (peel == PEEL_EMISSION) {
                    if constexpr (ANISO) Lp = p.L * E.emissionWeight(p, ins);  // PhotonPackage::launchEmissionPeelOff
                    cat = p.stellar >= 0 ? CAT_STAR_DIRECT : CAT_DUST_DIRECT;
                } else {
                    double I = 0;
                    // the direction (and the Stokes vector) before scattering
                    if constexpr (POL) E.peelWeightPol(ins, p, pcell, ox, oy, oz, osv, I, dq);
                    else E.peelWeight(ins, p, ox, oy, oz, I);
                    Lp = p.L * I;
                    cat = p.stellar >= 0 ? CAT_STAR_SCATTERED : CAT_DUST_SCATTERED;
                    level = (unsigned)min(p.nscatt, 255);  // nscatt already counts this scattering
                }
                dx = ins.kobs[0]; dy = ins.kobs[1]; dz = ins.kobs[2];
                prm = Lp;
                flags = RAY_PEEL | (cat << 2) | ((unsigned)i << 4) | (level << 10) | ((unsigned)p.ell << 18);
                // its detection record (the trace kernel adds the optical depth; a path that misses the
                // grid leaves tau = 0)
                idx = (int)(dpos + k);
                a.det[idx] = DetRec{Lp, 0.0, l, flags};
                if constexpr (POL) a.detPol[idx] = dq;
                at = pos++;
            } else {
                dx = p.kx; dy = p.ky; dz = p.kz;
                prm = mainParam;
                idx = slot;
                flags = mainMode | ((unsigned)p.ell << 18);
                at = back ? (unsigned)a.rayCap - 1u - wpos : pos++;
            }
            const bool in = E.emitRay(at, p, dx, dy, dz, prm, idx, flags, vcell, slot);  // (one call site: one inlined grid entry)
            if (k >= npeel && in && mainMode == RAY_FILL) fillAt = (int)at;
        }
        // the slot stays active while it has a FILL/WALK ray in flight
        if (active) actOut[apos] = slot;
        if (valid) E.store(slot, p, fresh);
        // a queued WALK ray's optical depth, where the queue holds references (kRayRefs): the slot's FILL ray,
        // whose deviate lay there, is over
        if (E.rayRefs() && mainMode == RAY_WALK) a.fuseU[slot] = mainParam;
        if (kEnterInEvent<GRID> && valid) a.svcell[slot] = vcell;
        // A fused FILL ray: its lane gets the deviates that this packet's next visit will draw (from a copy
        // of the counter-based stream: the packet's own does not advance; X < xi as the sign of u) and that
        // visit's termination threshold (decideFill). Written per slot here, where the round holds little else
        // in registers; the lane finds them through the ray's slot, whatever the queue's format
        if (a.fuse && fillAt >= 0) {
            PacketRng ahead = p.rng;
            const bool biased = a.xi != 0.0 && ahead.uniform() < a.xi;
            const double u = ahead.uniform();
            const double fu = biased ? -u : u, fthr = E.fillThreshold(p);
            a.fuseU[slot] = fu;
            a.fuseThr[slot] = fthr;
        }
    }
    const unsigned long long vals[8] = {E.packets, E.segFill, E.segWalk, E.segPeel, E.detects, 0, 0, 0};
    flushStats(a, vals);
}

// MonteCarloSimulation::continuouspeeloffscattering (MonteCarloSimulation.cpp:367-434), unpolarized. Runs
// before the event kernel of an iteration: every slot whose FILL ray just returned peels off, from a
// uniformly drawn point of every recorded path segment with scattering dust, toward every instrument,
// with the luminosity the segment scatters (albedo e^-tau0 (1 - e^-dtau)) times the phase function. The
// draws are the first of the packet's stream after the FILL, as in the reference (fillOpticalDepth,
// continuouspeeloffscattering, simulateescapeandabsorption, ...); the event kernel continues the stream.
// Two passes over the segments with the same draws: one counts the rays (a frame instrument skips a point
// outside its field), one writes them into the space reserved for the block.
template <int GRID, bool ONECOMP>
__global__ void __launch_bounds__(kBlock) contKernel(const Args a) {
    __shared__ unsigned long long resv[2 * (kBlock / 64) + 2];
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const unsigned int nwork = CTR(a.ctr, CTR_ACTIVE + a.parity);
    if (nwork == 0) return;
    Shared sh = stageTables(a, lds, gridParts<GRID>() | STAGE_OPTICS | STAGE_INSTR);
    Events<GRID, ONECOMP> E{a, sh};
    const int* actIn = a.act[a.parity];
    const unsigned int stride = gridDim.x * blockDim.x;
    const unsigned int rounds = (nwork + stride - 1) / stride;  // every lane runs every round (block reserves)
    const int Nl = a.nlambda;
    for (unsigned int round = 0; round < rounds; round++) {
        const unsigned int w = round * stride + blockIdx.x * blockDim.x + threadIdx.x;
        const int slot = w < nwork ? actIn[w] : 0;
        Packet p;
        p.state = S_NEW;
        if (w < nwork) E.load(slot, p);
        const bool fill = w < nwork && p.state == S_FILL;
        const int nrec = fill ? a.pathCnt[slot] : 0;
        const PathRec* rec = a.pathBuf + (size_t)slot * kPathCap;
        // the weights of one segment (rho(m,h) kappa_sca(h) / ksca) and its albedo; false: no scattering dust
        auto weights = [&](int m, double* wv, double& albedo) {
            double ksca = 0.0, kext = 0.0;
            for (int h = 0; h < a.ncomp; h++) {
                const double rho = a.rho[(size_t)m * a.ncomp + h];
                wv[h] = rho * sh.ksca[h * Nl + p.ell];
                ksca += rho * sh.ksca[h * Nl + p.ell];
                kext += rho * sh.kext[h * Nl + p.ell];
            }
            if (!(ksca > 0.0)) return false;
            for (int h = 0; h < a.ncomp; h++) wv[h] /= ksca;
            albedo = ksca / kext;
            return true;
        };
        // pass 1: the rays this slot emits
        const PacketRng rng0 = p.rng;
        unsigned int nray = 0;
        for (int n = 0; n < nrec; n++) {
            double wv[8], albedo;
            if (!weights(rec[n].m, wv, albedo)) continue;
            const double s = rec[n].s0 + p.rng.uniform() * rec[n].ds;
            Packet q = p;
            q.rx = p.rx + s * p.kx; q.ry = p.ry + s * p.ky; q.rz = p.rz + s * p.kz;
            for (int i = 0; i < a.ninstr; i++)
                if (!(sh.instr[i].kind == SKIRT_INSTR_FRAME && E.pixel(sh.instr[i], q) < 0)) nray++;
        }
        // a ray and a detection record per peel-off
        unsigned* const ctrs[2] = {CTRP(a.ctr, CTR_RAYS + a.parity), CTRP(a.ctr, CTR_DET + a.parity)};
        const unsigned cnt[2] = {nray, nray};
        unsigned res[2];
        blockReserve(ctrs, cnt, res, resv);
        unsigned int pos = res[0], dpos = res[1];
        // (the WALK rays of the event kernel that follows are reserved from the queue's top later: the trace
        // kernel checks that the two regions do not meet)
        if (nray && (pos + nray > (unsigned)a.rayCap || dpos + nray > (unsigned)(a.rayCap - a.nslots))) {
            atomicOr(a.error, ERR_QUEUE);  // cannot happen with the pool sized for kPathCap (ensurePool)
            nray = 0;
        }
        // pass 2: the same draws again, now writing the rays and their detection records
        if (nray) {
            PacketRng rng = rng0;
            for (int n = 0; n < nrec; n++) {
                double wv[8], albedo;
                if (!weights(rec[n].m, wv, albedo)) continue;
                const double factorm = albedo * exp(-rec[n].tau0) * (-expm1(-rec[n].dtau));
                const double s = rec[n].s0 + rng.uniform() * rec[n].ds;
                Packet q = p;
                q.rx = p.rx + s * p.kx; q.ry = p.ry + s * p.ky; q.rz = p.rz + s * p.kz;
                int qcell = kNoCell;  // the point's cell (Voronoi), located once for all instruments
                for (int i = 0; i < a.ninstr; i++) {
                    const DevInstr& ins = sh.instr[i];
                    const int l = ins.kind == SKIRT_INSTR_SED ? -1 : E.pixel(ins, q);
                    if (ins.kind == SKIRT_INSTR_FRAME && l < 0) continue;
                    const double cosalpha = p.kx * ins.kobs[0] + p.ky * ins.kobs[1] + p.kz * ins.kobs[2];
                    double I = 0;
                    for (int h = 0; h < a.ncomp; h++) {
                        const double g = sh.g[h * Nl + p.ell];
                        const double t = 1.0 + g * g - 2 * g * cosalpha;
                        const double wgt = wv[h] * ((1.0 - g) * (1.0 + g) / sqrt(t * t * t));
                        I += wgt * 1.0;
                    }
                    // PhotonPackage::launchScatteringPeelOff(pp, bfrnew, bfkobs, factorm * I)
                    const double Lp = p.L * (factorm * I);
                    const unsigned cat = p.stellar >= 0 ? CAT_STAR_SCATTERED : CAT_DUST_SCATTERED;
                    const unsigned level = (unsigned)min(p.nscatt + 1, 255);
                    const unsigned flags = RAY_PEEL | (cat << 2) | ((unsigned)i << 4) | (level << 10) | ((unsigned)p.ell << 18);
                    a.det[dpos] = DetRec{Lp, 0.0, l, flags};
                    E.emitRay(pos++, q, ins.kobs[0], ins.kobs[1], ins.kobs[2], Lp, (int)dpos, flags, qcell, slot);
                    dpos++;
                }
            }
        }
        if (fill) {  // the stream continues after the continuous draws
            a.sblock[slot] = p.rng.block; a.sw2[slot] = p.rng.w2; a.sw3[slot] = p.rng.w3; a.shave[slot] = p.rng.have;
        }
    }
    const unsigned long long vals[8] = {0, E.segFill, E.segWalk, E.segPeel, 0, 0, 0, 0};
    flushStats(a, vals);
}

#include "density_sample.hpp"
#include "particle_kernels.hpp"

// polProbeOne (polarization.hpp) on n packet states, one per thread (skirt_mcrt_scatterings)
__global__ void __launch_bounds__(kBlock)
    scatteringsKernel(const double* tab, int ncomp, int nlambda, int nt, const double* states, const double* deviates,
                      double kox, double koy, double koz, double kyx, double kyy, double kyz, size_t n, double* out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double kobs[3] = {kox, koy, koz}, ky[3] = {kyx, kyy, kyz};
    polProbeOne(tab, ncomp, nlambda, nt, states + polStateWords * i, deviates + 2 * i, kobs, ky, out + polResultWords * i);
}

}  // namespace

// the Labs replicas of an absorbing phase (Args::labsCopies) added into the table, in replica order, and
// zeroed for the next phase
extern "C" __global__ void labsFoldKernel(double* dst, double* rep, size_t n, int copies, size_t strideElems) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double sum = 0.0;
        for (int k = 0; k < copies; k++) {
            sum += rep[k * strideElems + i];
            rep[k * strideElems + i] = 0.0;
        }
        dst[i] += sum;
    }
}

// ====================================================================== the launch seam (engine_launch.hpp)
// All the host side (host/engine_*.cpp) sees of the kernels above: the address of a templated kernel for its
// runtime arguments, launched through hipLaunchKernel, and one typed launch function per one-off kernel.
namespace {

// f(std::integral_constant<int, G>{}) for the walk kind G = kind: the one place where a runtime grid kind
// turns into a template argument. A generic lambda is instantiated for every kind, so it names only the
// kernels that exist for each (if constexpr). The kinds are instantiated in the table's order, which is
// the order the kernels have always had in the code object.
template <int I = 0, class F>
auto withWalk(int kind, F&& f) {
    if constexpr (I + 1 < kNumWalks) {
        if (kind == kWalks[I].kind) return f(std::integral_constant<int, kWalks[I].kind>{});
        return withWalk<I + 1>(kind, f);
    } else {
        return f(std::integral_constant<int, kWalks[I].kind>{});
    }
}

// f(std::true_type{}) or f(std::false_type{}): a runtime flag as a template argument
template <class F>
auto withBool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

}  // namespace

namespace skirt_dev {

// the trace kernel of a walk; a phase storing no absorption may run traceKernelNoStore (no Voronoi one exists)
const void* traceKernelOf(int kind, bool one, bool continuous, bool global, bool noStore) {
    return withWalk(kind, [&](auto g) {
        constexpr int G = decltype(g)::value;
        if constexpr (G != SKIRT_GRID_VORONOI)
            if (noStore) return (const void*)traceKernelNoStore<G>;
        return withBool(global, [&](auto gl) {
            constexpr bool L = decltype(gl)::value;
            if constexpr (G == SKIRT_GRID_VORONOI) {
                if (!continuous) return one ? (const void*)traceKernelVor<true, false, L> : (const void*)traceKernelVor<false, false, L>;
                return one ? (const void*)traceKernelVor<true, true, L> : (const void*)traceKernelVor<false, true, L>;
            } else {
                if (!continuous) return one ? (const void*)traceKernel<G, true, false, L> : (const void*)traceKernel<G, false, false, L>;
                return one ? (const void*)traceKernel<G, true, true, L> : (const void*)traceKernel<G, false, true, L>;
            }
        });
    });
}

// the event kernel of a walk; the ANISO kernels where the grid has them (runPhase has refused the others)
const void* eventKernelOf(int kind, bool one, bool pol, bool aniso) {
    return withWalk(kind, [&](auto g) {
        return withBool(one, [&](auto o) {
            constexpr int G = decltype(g)::value;
            constexpr bool O = decltype(o)::value;
            if constexpr (kAnisoGrid<G>)
                if (aniso) return pol ? (const void*)eventKernel<G, O, true, true> : (const void*)eventKernel<G, O, false, true>;
            return pol ? (const void*)eventKernel<G, O, true> : (const void*)eventKernel<G, O>;
        });
    });
}

const void* contKernelOf(int kind, bool one) {
    return withWalk(kind, [&](auto g) {
        return withBool(one, [&](auto o) { return (const void*)contKernel<decltype(g)::value, decltype(o)::value>; });
    });
}

const void* detectKernelOf(bool pol) { return pol ? (const void*)detectKernel<true> : (const void*)detectKernel<false>; }

// columnKernel(Args, rays, n, out): the walks of the photon paths, through the node arrays for trees (equal to the
// leaf-map walk, tests/test_gpu_parity.py::test_leaf_map_walk_equals_node_walk)
const void* columnKernelOf(int kind) {
    return withWalk(kind, [&](auto g) {
        constexpr int G = decltype(g)::value;
        constexpr int W = (G == SKIRT_GRID_OCTREE || G == kBinTreeMap) ? kOctreeNodes : G;  // no leaf maps here
        return (const void*)columnKernel<W>;
    });
}

void launchBuildLeafMap(dim3 grid, hipStream_t st, LeafEntry* map, const int* firstChild, const signed char* splitDir,
                        const int* cellnumber, const double* rho, int ncomp, int L) {
    hipLaunchKernelGGL(buildLeafMapKernel, grid, dim3(kBlock), 0, st, map, firstChild, splitDir, cellnumber, rho, ncomp, L);
}

void launchLabsFold(dim3 grid, hipStream_t st, double* dst, double* rep, size_t n, int copies, size_t strideElems) {
    hipLaunchKernelGGL(labsFoldKernel, grid, dim3(kBlock), 0, st, dst, rep, n, copies, strideElems);
}

void launchCellSpectra(dim3 grid, hipStream_t st, const EmisArgs& e) {
    hipLaunchKernelGGL(cellSpectraKernel, grid, dim3(kBlock), 0, st, e);
}
void launchCellBlockSum(dim3 grid, hipStream_t st, const EmisArgs& e) {
    hipLaunchKernelGGL(cellBlockSumKernel, grid, dim3(kBlock), 0, st, e);
}
void launchCellScanBlocks(dim3 grid, hipStream_t st, const EmisArgs& e) {
    hipLaunchKernelGGL(cellScanBlocksKernel, grid, dim3(kBlock), 0, st, e);
}
void launchCellCdf(dim3 grid, hipStream_t st, const EmisArgs& e) {
    hipLaunchKernelGGL(cellCdfKernel, grid, dim3(kBlock), 0, st, e);
}
void launchCellGuide(dim3 grid, hipStream_t st, const double* cdf, int* guide, int N) {
    hipLaunchKernelGGL(cellGuideKernel, grid, dim3(kBlock), 0, st, cdf, guide, N);
}

void launchSamplePositions(dim3 grid, hipStream_t st, const double* geomParam, const double* geomTable, int h,
                           unsigned long long seed, unsigned long long first, size_t n, double* pos, int* draws,
                           unsigned* error) {
    hipLaunchKernelGGL(samplePositionsKernel, grid, dim3(kBlock), 0, st, geomParam, geomTable, h, seed, first, n, pos, draws,
                       error);
}
void launchSampleLaunches(dim3 grid, hipStream_t st, const double* geomParam, const double* geomTable, int nstar, int h,
                          unsigned long long seed, unsigned long long first, size_t n, double* pos, double* dir, int* draws,
                          size_t nprob, const double* ppos, const double* pdir, double* prob, unsigned* error) {
    hipLaunchKernelGGL(sampleLaunchesKernel, grid, dim3(kBlock), 0, st, geomParam, geomTable, nstar, h, seed, first, n, pos,
                       dir, draws, nprob, ppos, pdir, prob, error);
}
void launchScatterings(dim3 grid, hipStream_t st, const double* tab, int ncomp, int nlambda, int nt, const double* states,
                       const double* deviates, double kox, double koy, double koz, double kyx, double kyy, double kyz,
                       size_t n, double* out) {
    hipLaunchKernelGGL(scatteringsKernel, grid, dim3(kBlock), 0, st, tab, ncomp, nlambda, nt, states, deviates, kox, koy, koz,
                       kyx, kyy, kyz, n, out);
}
void launchDensitySample(dim3 grid, hipStream_t st, const DensArgs& d) {
    hipLaunchKernelGGL(densitySampleKernel, grid, dim3(kBlock), 0, st, d);
}
void launchParticleSample(dim3 grid, hipStream_t st, const PartArgs& a) {
    hipLaunchKernelGGL(particleSampleKernel, grid, dim3(kBlock), 0, st, a);
}
void launchParticleMass(dim3 grid, hipStream_t st, const PartArgs& a, unsigned* handedBack) {
    hipLaunchKernelGGL(particleMassKernel, grid, dim3(partMassBlock), 0, st, a, handedBack);
}

}  // namespace skirt_dev
