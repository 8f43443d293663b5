// Internal to the host set-up (build.cpp and the files it drives): the parse context, the .ski attribute helpers,
// the stage timer, and the stages that loadSki calls, each defined in the file of its subject.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "model.hpp"
#include "xml.hpp"

#pragma GCC visibility push(hidden)  // the library's own: not among its dynamic symbols
namespace skirt {

// SKIRT_AMD_SETUP_TIMES=1 prints the duration of every setup stage to stderr
struct StageTimer {
    const char* name;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit StageTimer(const char* n) : name(n) {}
    ~StageTimer() {
        static const bool on = std::getenv("SKIRT_AMD_SETUP_TIMES") != nullptr;
        if (on)
            std::fprintf(stderr, "[setup] %-24s %.3f s\n", name,
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
};

struct Ctx {
    Units units;
    std::string datadir;
    UniformSource* rng;
    DensitySampler* sampler = nullptr;  // device density sampling (null: host threads)
    std::string inputdir;               // where relative input file names are looked up
};

// ------------------------------------------------------------ .ski attributes
inline double attr(const Ctx& c, const XmlElement* e, const char* key, const char* qty, double def) {
    if (!e->has(key)) return def;
    return c.units.parse(e->get(key), qty);
}
inline int attrInt(const XmlElement* e, const char* key, int def) {
    if (!e->has(key)) return def;
    return (int)std::lround(std::strtod(e->get(key).c_str(), nullptr));
}
inline bool attrBool(const XmlElement* e, const char* key, bool def) {
    if (!e->has(key)) return def;
    std::string v = e->get(key);
    std::transform(v.begin(), v.end(), v.begin(), ::tolower);
    return v == "true" || v == "yes" || v == "1";
}
inline std::vector<double> attrList(const Ctx& c, const XmlElement* e, const char* key, const char* qty) {
    std::vector<double> out;
    std::string s = e->get(key);
    std::stringstream ss(s);
    std::string item;
    while (std::getline(ss, item, ',')) out.push_back(c.units.parse(item, qty));
    return out;
}
inline const XmlElement* need(const XmlElement* e, const char* prop) {
    const XmlElement* it = e->item(prop);
    if (!it) throw std::runtime_error(std::string("missing property '") + prop + "' in " + e->name);
    return it;
}

// ------------------------------------------------------------ the stages, in loadSki's order
// sources.cpp: the wavelength grid; the stellar components' geometries and luminosities (m.star*)
WavelengthGrid parseWavelengthGrid(const Ctx& c, const XmlElement* w);
void parseStellarSystem(const Ctx& c, const XmlElement* ss, Model& m);
// geometry.cpp
Geometry parseGeometry(const Ctx& c, const XmlElement* g);
// dustmix.cpp: a packaged resource table (rows x columns of doubles), the mixes, DustMix::kappaext(lambda)
struct Table {
    long nrows = 0, ncols = 0;
    std::vector<double> v;
    double at(long r, long c) const { return v[r * ncols + c]; }
};
Table readTable(const std::string& datadir, const std::string& name);
DustMix parseMix(const Ctx& c, const XmlElement* e, const WavelengthGrid& wl);
double mixKappaext(const DustMix& mix, const WavelengthGrid& wl, double lambda);
// dustgrid.cpp: the dust grid of every kind (m.grid), after the grid/geometry dimension check; the tree kinds
// through treegrid.cpp, which samples the dust density on c.rng as it subdivides
void parseDustGrid(const Ctx& c, const XmlElement* ge, Model& m);
void buildOctree(const Ctx& c, const XmlElement* e, const Model& model, OctreeGrid& t, bool binary);
// treegrid.cpp: particle dust's massInBox of n boxes, on the sampler's device or on worker threads
void particleMasses(const Ctx& c, const ParticleSet& ps, const double* boxes, size_t n, double* out);
// densities.cpp: DustSystem::setupSelfAfter, the cell volumes and the sampled densities (m.volume, m.rho)
void sampleDensities(const Ctx& c, Model& m);

}  // namespace skirt
#pragma GCC visibility pop
