// .ski file -> Model, including every setup step that consumes random numbers.
//
// The reference performs these steps in SimulationItem::setup() order (SimulationItem.cpp:18-31):
// wavelength grid, stellar system (StellarSystem.cpp:35-52), dust mixes (DustMix.cpp:44-264), the dust
// grid (TreeDustGrid.cpp:50-164 draws density samples while subdividing), then the cell densities
// (DustSystem.cpp:63-178, 100 random positions per cell) and the instruments. Random draws happen only
// in the tree subdivision and the cell density sampling, in that order; both are reproduced here on the
// caller's UniformSource so that a single-threaded reference run and this setup produce bit-identical
// densities and trees.
//
// loadSki below is the driver: it reads the simulation's own attributes and calls the stages in that order. Each
// stage lives in the file of its subject (ski_parse.hpp lists them); what remains here are the dust system's
// components, the instruments, and the members of WavelengthGrid, Instrument and Model.
#include <cmath>
#include <dlfcn.h>
#include <fstream>
#include <stdexcept>

#include "ski_parse.hpp"

namespace skirt {

double WavelengthGrid::lambdamin(int ell) const {
    return (ell == 0) ? lambda[0] : std::sqrt(lambda[ell - 1] * lambda[ell]);
}
double WavelengthGrid::lambdamax(int ell) const {
    int N = n();
    return (ell == N - 1) ? lambda[N - 1] : std::sqrt(lambda[ell] * lambda[ell + 1]);
}

int Instrument::pixel(double x, double y, double z) const {
    double xpp = -sinphi * x + cosphi * y;
    double ypp = -cosphi * costheta * x - sinphi * costheta * y + sintheta * z;
    double xp = cospa * xpp - sinpa * ypp;
    double yp = sinpa * xpp + cospa * ypp;
    int i = static_cast<int>(std::floor((xp - xpmin) / xpsiz));
    int j = static_cast<int>(std::floor((yp - ypmin) / ypsiz));
    if (i < 0 || i >= Nx || j < 0 || j >= Ny) return -1;
    return i + Nx * j;
}

double Model::kapparho(int m, int ell) const {
    if (m < 0) return 0;
    double result = 0;
    int nc = ncomp();
    for (int h = 0; h < nc; h++) result += dust[h].mix.kext[ell] * rho[(size_t)m * nc + h];
    return result;
}

namespace {

// ------------------------------------------------------------ instruments
Instrument parseInstrument(const Ctx& c, const XmlElement* e) {
    Instrument ins;
    ins.name = e->get("instrumentName", "");
    if (e->name == "FullInstrument") ins.kind = InstrumentKind::Full;
    else if (e->name == "SimpleInstrument") ins.kind = InstrumentKind::Simple;
    else if (e->name == "SEDInstrument") ins.kind = InstrumentKind::SED;
    else if (e->name == "FrameInstrument") ins.kind = InstrumentKind::Frame;
    else throw std::runtime_error("unsupported instrument " + e->name);
    ins.distance = attr(c, e, "distance", "distance", 0);
    ins.inclination = attr(c, e, "inclination", "posangle", 0);
    ins.azimuth = attr(c, e, "azimuth", "posangle", 0);
    ins.positionAngle = attr(c, e, "positionAngle", "posangle", 0);
    if (ins.distance <= 0) throw std::runtime_error("instrument distance was not set");
    // DistantInstrument::setupSelfBefore (DistantInstrument.cpp:27-50)
    ins.costheta = std::cos(ins.inclination);
    ins.sintheta = std::sin(ins.inclination);
    ins.cosphi = std::cos(ins.azimuth);
    ins.sinphi = std::sin(ins.azimuth);
    ins.cospa = std::cos(ins.positionAngle);
    ins.sinpa = std::sin(ins.positionAngle);
    // Direction(theta, phi) (Direction.cpp)
    if (ins.inclination < -1e-8 || ins.inclination > M_PI + 1e-8)
        throw std::runtime_error("theta should be between 0 and pi");
    direction(ins.inclination, ins.azimuth, ins.kobs[0], ins.kobs[1], ins.kobs[2]);
    ins.kx[0] = +ins.cosphi * ins.costheta * ins.sinpa - ins.sinphi * ins.cospa;
    ins.kx[1] = +ins.sinphi * ins.costheta * ins.sinpa + ins.cosphi * ins.cospa;
    ins.kx[2] = -ins.sintheta * ins.sinpa;
    ins.ky[0] = -ins.cosphi * ins.costheta * ins.cospa - ins.sinphi * ins.sinpa;
    ins.ky[1] = -ins.sinphi * ins.costheta * ins.cospa + ins.cosphi * ins.sinpa;
    ins.ky[2] = +ins.sintheta * ins.cospa;
    if (ins.kind != InstrumentKind::SED) {
        ins.fovx = attr(c, e, "fieldOfViewX", "length", 0);
        ins.fovy = attr(c, e, "fieldOfViewY", "length", 0);
        ins.Nx = attrInt(e, "pixelsX", 250);
        ins.Ny = attrInt(e, "pixelsY", 250);
        ins.xc = attr(c, e, "centerX", "length", 0);
        ins.yc = attr(c, e, "centerY", "length", 0);
        if (ins.Nx <= 0 || ins.Ny <= 0) throw std::runtime_error("number of pixels was not set");
        if (ins.fovx <= 0 || ins.fovy <= 0) throw std::runtime_error("field of view was not set");
        // SingleFrameInstrument::setupSelfBefore (SingleFrameInstrument.cpp:24-38)
        ins.xpmin = ins.xc - 0.5 * ins.fovx;
        ins.xpmax = ins.xc + 0.5 * ins.fovx;
        ins.xpsiz = ins.fovx / ins.Nx;
        ins.ypmin = ins.yc - 0.5 * ins.fovy;
        ins.ypmax = ins.yc + 0.5 * ins.fovy;
        ins.ypsiz = ins.fovy / ins.Ny;
    } else {
        ins.Nx = ins.Ny = 0;  // an SEDInstrument has no frame (SEDInstrument.cpp)
    }
    if (ins.kind == InstrumentKind::Full) ins.scatteringLevels = attrInt(e, "scatteringLevels", 0);
    return ins;
}

// SPHDustDistribution::setupSelfBefore: the imported particles as the dust system's one component. A relative file
// name is looked up in the input folder (FilePaths::input), by default the .ski file's own folder.
void parseParticleDust(const Ctx& c, const XmlElement* dd, Model& m) {
    const double fdust = attr(c, dd, "dustFraction", "", 0);
    const double Tmax = attr(c, dd, "maximumTemperature", "temperature", 0);
    if (fdust <= 0.0) throw std::runtime_error("The dust fraction should be positive");
    const XmlElement* mixEl = dd->item("dustMix");
    if (!mixEl) throw std::runtime_error("Dust mix was not set");
    std::string file = dd->get("filename", "");
    if (file.empty()) throw std::runtime_error("SPHDustDistribution has no filename");
    if (file[0] != '/') file = (c.inputdir.empty() ? std::string(".") : c.inputdir) + "/" + file;
    DustComp comp;
    comp.mix = parseMix(c, mixEl, m.wl);
    m.particles = readParticles(file, fdust, Tmax);
    comp.particles = m.particles;
    comp.nf = m.particles->mass();  // DustDistribution::mass(): what the grids and the outputs take as the total
    m.dust.push_back(comp);
    m.polarization = comp.mix.polarization;
    if (m.polarization && m.continuousScattering)
        throw std::runtime_error("continuous scattering is not supported with polarised dust mixes (ElectronDustMix)");
    if (m.polarization && m.dustEmission)
        throw std::runtime_error("dust emission is not supported with polarised dust mixes (ElectronDustMix)");
}

// The dust system's properties and its components (geometry, mix, normalization), with DustSystem::setupSelfBefore's
// checks on the mixes; the grid and the densities follow in loadSki
void parseDustSystem(const Ctx& c, const XmlElement* ds, Model& m) {
    m.hasDust = true;
    bool pds = ds->name == "PanDustSystem";
    if (pds != m.pan) throw std::runtime_error("dust system type does not match the simulation type");
    m.sampleCount = attrInt(ds, "sampleCount", 100);
    m.writeConvergence = attrBool(ds, "writeConvergence", true);
    m.writeCellProperties = attrBool(ds, "writeCellProperties", false);
    m.writeCellsCrossed = attrBool(ds, "writeCellsCrossed", false);
    if (pds) {
        m.dustEmission = ds->item("dustEmissivity") != nullptr;
        m.selfAbsorption = m.dustEmission && attrBool(ds, "selfAbsorption", false);
        m.dustEmissionBias = attr(c, ds, "emissionBias", "", 0.5);
        m.emissionBoost = attr(c, ds, "emissionBoost", "", 1);
        m.cycles = attrInt(ds, "cycles", 0);
        m.writeISRF = attrBool(ds, "writeISRF", false);
        m.storeAbsorption = m.dustEmission;
    } else {
        m.writeMeanIntensity = attrBool(ds, "writeMeanIntensity", false);
        m.storeAbsorption = m.writeMeanIntensity;
    }
    const XmlElement* dd = need(ds, "dustDistribution");
    if (dd->name == "SPHDustDistribution") {
        parseParticleDust(c, dd, m);
        return;
    }
    if (dd->name != "CompDustDistribution") throw std::runtime_error("unsupported dust distribution " + dd->name);
    for (const XmlElement* dc : dd->items("components")) {
        DustComp comp;
        comp.geom = parseGeometry(c, need(dc, "geometry"));
        if (comp.geom.kind == GeometryKind::Point)  // a delta density cannot be sampled on a dust grid
            throw std::runtime_error("PointGeometry is not supported for dust components");
        if (isAnisotropic(comp.geom.kind))  // (densities 0 or infinite as well)
            throw std::runtime_error(need(dc, "geometry")->name + " is not supported for dust components");
        comp.mix = parseMix(c, need(dc, "mix"), m.wl);
        const XmlElement* nrm = need(dc, "normalization");
        if (nrm->name == "DustMassDustCompNormalization") {
            comp.nf = attr(c, nrm, "dustMass", "mass", 0);
        } else if (nrm->name == "FaceOnDustCompNormalization" || nrm->name == "EdgeOnDustCompNormalization" ||
                   nrm->name == "RadialDustCompNormalization") {
            // {FaceOn,EdgeOn,Radial}DustCompNormalization::normalizationFactor:
            // tau / (Sigma * kappaext(lambda)), Sigma = SigmaZ / SigmaR / Sigmar
            const double tau = attr(c, nrm, "opticalDepth", "", 0);
            const double lambda = attr(c, nrm, "wavelength", "wavelength", 0);
            const double Sigma = nrm->name[0] == 'F' ? comp.geom.SigmaZ()
                                 : nrm->name[0] == 'E' ? comp.geom.SigmaR() : comp.geom.Sigmar();
            comp.nf = tau / (Sigma * mixKappaext(comp.mix, m.wl, lambda));
        } else {
            throw std::runtime_error("unsupported dust normalization " + nrm->name);
        }
        m.dust.push_back(comp);
    }
    if (m.dust.empty()) throw std::runtime_error("dust distribution has no components");
    // DustSystem::setupSelfBefore (DustSystem.cpp:71-75), in the reference's words
    for (const DustComp& comp : m.dust)
        if (comp.mix.polarization != m.dust[0].mix.polarization)
            throw std::runtime_error("All dust mixes must consistenly support polarization, or not support polarization");
    m.polarization = m.dust[0].mix.polarization;
    for (const DustComp& comp : m.dust)  // (the engine's tables are [component][wavelength][angle])
        if (m.polarization && comp.mix.ntheta != m.dust[0].mix.ntheta)
            throw std::runtime_error("polarised dust mixes with different numbers of scattering angles are not supported");
    // beyond the engine's polarised kernels (MonteCarloSimulation.cpp:420-428; the dust emission phases)
    if (m.polarization && m.continuousScattering)
        throw std::runtime_error("continuous scattering is not supported with polarised dust mixes (ElectronDustMix)");
    if (m.polarization && m.dustEmission)
        throw std::runtime_error("dust emission is not supported with polarised dust mixes (ElectronDustMix)");
}

}  // namespace

// ============================================================ loadSki

Model loadSki(const std::string& path, UniformSource& rng, const std::string& datadir, DensitySampler* sampler,
              const std::string& inputdir) {
    auto doc = parseXmlFile(path);
    if (doc->children.empty()) throw std::runtime_error("empty ski file");
    const XmlElement* sim = doc->children.front().get();
    Model m;
    if (sim->name == "OligoMonteCarloSimulation") m.pan = false;
    else if (sim->name == "PanMonteCarloSimulation") m.pan = true;
    else throw std::runtime_error("unsupported simulation type " + sim->name);

    const XmlElement* unitsEl = sim->item("units");
    m.units_system = unitsEl ? unitsEl->name : "ExtragalacticUnits";
    Ctx c{Units(m.units_system), datadir, &rng, sampler, inputdir};
    if (c.inputdir.empty()) {  // the .ski file's own folder (the engine's choice)
        const size_t slash = path.rfind('/');
        c.inputdir = slash == std::string::npos ? "." : path.substr(0, slash);
    }

    if (const XmlElement* r = sim->item("random")) m.seed = (unsigned long)attrInt(r, "seed", 4357);
    m.packages = attr(c, sim, "packages", "", 1e6);
    m.minWeightReduction = attr(c, sim, "minWeightReduction", "", 1e4);
    m.minScattEvents = (int)attr(c, sim, "minScattEvents", "", 0);
    m.scattBias = attr(c, sim, "scattBias", "", 0.5);
    m.continuousScattering = attrBool(sim, "continuousScattering", false);
    if (m.packages < 0 || m.packages > 1e15) throw std::runtime_error("invalid number of photon packages");
    if (m.minWeightReduction < 1e3) throw std::runtime_error("the minimum weight reduction factor should be larger than 1000");
    if (m.scattBias < 0 || m.scattBias > 1) throw std::runtime_error("the scattering bias should be between 0 and 1");

    m.wl = parseWavelengthGrid(c, need(sim, "wavelengthGrid"));
    parseStellarSystem(c, need(sim, "stellarSystem"), m);

    if (const XmlElement* ds = sim->item("dustSystem")) {
        parseDustSystem(c, ds, m);
        parseDustGrid(c, need(ds, "dustGrid"), m);
        sampleDensities(c, m);
    }

    // ---- instruments
    if (const XmlElement* is = sim->item("instrumentSystem"))
        for (const XmlElement* ie : is->items("instruments")) m.instruments.push_back(parseInstrument(c, ie));
    // FullInstrument::setupSelfBefore (FullInstrument.cpp:51-54, 79-87): Stokes arrays with a polarising dust system
    for (Instrument& ins : m.instruments) ins.polarization = ins.kind == InstrumentKind::Full && m.hasDust && m.polarization;
    return m;
}

std::string defaultDataDir() {
    Dl_info info;
    if (dladdr((void*)&defaultDataDir, &info) && info.dli_fname) {
        std::string p(info.dli_fname);
        size_t s = p.rfind('/');
        std::string dir = (s == std::string::npos) ? "." : p.substr(0, s);
        // the library lives in skirt_amd/ (or skirt_amd/lib); data is skirt_amd/data
        for (const char* cand : {"/data", "/../data"}) {
            std::string d = dir + cand;
            std::ifstream f(d + "/SunSED.bin");
            if (f) return d;
        }
    }
    return "skirt_amd/data";
}

}  // namespace skirt
