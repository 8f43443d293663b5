// The engine's host-side arithmetic that touches no GPU: where the pool's arrays lie, how the instruments' tallies
// are laid out, how tree leaves and Voronoi cells are numbered and packed for the device, and the Labs and LDS plans
// of a phase. Each is a function from plain inputs to a small result; the upload and plan functions of
// engine_setup.cpp and engine_phase.cpp call them and then allocate and copy. No HIP header is included here, so the
// same functions run in CPU tests (tools/engine_layout_cpu.py) and tools.
//
// A function returning int returns SKIRT_OK or the engine's error code, with the message in `err`.
#ifndef SKIRT_AMD_HOST_ENGINE_LAYOUT_HPP
#define SKIRT_AMD_HOST_ENGINE_LAYOUT_HPP

#include <string>
#include <vector>

#include "../device/engine_args.hpp"

#pragma GCC visibility push(hidden)
namespace skirt_dev {

int envInt(const char* name, int dflt);
// SKIRT_AMD_CELL_ALIGN=0: the reference's cell order, without the line-aligned device numbering
bool cellAlign();

// ---- slot pool
constexpr size_t kPoolSpare = 4096;
// the ray queue's length for nslots slots, and its format, as the kernels choose it (kRayRefs)
size_t poolRayCap(size_t nslots, size_t ninstr, bool continuous);
inline bool poolRefs(bool continuous, int gridKind) { return !continuous && gridKind != SKIRT_GRID_VORONOI; }
size_t poolLayout(char* base, size_t nslots, size_t rayCap, bool refs, bool detPair, bool path, bool pol, Args& a);

// ---- instrument tallies
struct InstrLayout {
    std::vector<DevInstr> instr;
    size_t nInstrTally = 0;  // doubles of the global instrument tally
    int nsed = 0;            // doubles of one copy of the SED sums in LDS
};
// pol: a polarised simulation (FullInstruments carry Stokes Q, U, V after the scattering levels)
int instrLayout(const SkirtInstrDesc* in, int n, int nlambda, bool pol, InstrLayout& out, std::string& err);

// ---- trees
// the index arrays checked so that the kernels never read out of bounds; father: of every node, for the
// Bookkeeping search (else left empty)
int checkTree(const SkirtGridDesc* g, std::vector<int>& father, std::string& err);
struct CellNumbering {
    std::vector<int> devCell;  // reference cell -> device cell
    int ndev = 0;              // device cell numbers in use, gaps included
};
int numberTreeLeaves(const SkirtGridDesc* g, CellNumbering& out, std::string& err);
struct LeafMapPlan {
    int L = -1, N = 0;      // L < 0: no leaf map, the tree is walked through its node arrays
    std::vector<double> T;  // split coordinates per axis, 3 x (N + 1)
    double inv[3] = {0, 0, 0}, origin[3] = {0, 0, 0};
};
LeafMapPlan planLeafMapTables(const SkirtGridDesc* g, int ndev);

// ---- Voronoi
struct VoronoiPack {
    std::vector<int> devCell;
    std::vector<double> site, bbox;  // device cell order: 3 and 6 per cell
    std::vector<int> start;          // where each device cell's block of slots starts, ncells + 1
    std::vector<VorEntry> slots;     // headers, neighbour entries in pairs, padding, kVorPad tail
    std::vector<BlockSite> blocks;   // the block lists, device cell ids
    double vorScale = 1.0;
};
int packVoronoi(const SkirtGridDesc* g, VoronoiPack& out, std::string& err);

// ---- Labs addressing of a phase
struct LabsPlan {
    int hi = 0, global = 0;  // Args::labsHi, Args::labsGlobal
    unsigned bytes = 0;      // Args::labsBytes
    int copies = 1;          // Args::labsCopies; > 1: replicas `stride` bytes apart
    unsigned stride = 0;     // Args::labsCopyStride
};
int planLabsMode(uint64_t labsElems, bool store, bool selfAbsorption, LabsPlan& out, std::string& err);

// ---- LDS of a phase
struct LdsInputs {
    int meshWords = 0, treeWords = 0;  // the walk's mesh or the leaf map's split tables, in doubles
    int ncomp = 1, nlambda = 0, ninstr = 0, nsed = 0;
    bool store = false, continuous = false, voronoi = false, labsHi = false;
    size_t budget = 0;  // what one workgroup may allocate
};
struct LdsPlan {
    int meshOff = 0, optOff = 0, instrOff = 0, sedOff = 0;  // Args::lds*Off, in doubles
    bool noStore = false;
    size_t trace = 0, event = 0, detect = 0;  // dynamic LDS of the trace, event / continuous and detect kernels
    int detCopies = 0;
};
int planLdsLayout(const LdsInputs& in, LdsPlan& out, std::string& err);

}  // namespace skirt_dev
#pragma GCC visibility pop

#endif
