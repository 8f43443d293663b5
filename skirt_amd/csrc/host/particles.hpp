// Imported particle dust: SKIRTcore/SPHDustDistribution.cpp with SPHGasParticle.cpp, SPHGasParticleGrid.cpp and
// TextInFile.cpp. A text file of gas particles (x y z h M Z [T]; pc, pc, pc, pc, Msun, -, K), each smoothed with a
// cubic-spline kernel, behind a 20 x 20 x 20 grid of particle lists. The density at a point and the mass in a box are
// device/particle_density.hpp's, compiled here for the host, so the host, the device and the CPU logic test run one
// text. All inline: the CPU checker compiles a fixed list of host sources.
#pragma once

#include <algorithm>
#include <cmath>
#include <fstream>
#include <limits>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "nr.hpp"
#include "units.hpp"
#include "../device/particle_density.hpp"

namespace skirt {

struct ParticleSet {
    std::string path;              // the file the particles came from
    std::vector<PartRec> rec;      // per kept particle: centre and cached constants
    std::vector<double> h;         // smoothing lengths
    std::vector<double> metal;     // SPHGasParticle::metalMass: M * Z
    double fdust = 0;
    bool negativeMasses = false;   // some M < 0: no DustMassInBoxInterface
    int nignored = 0;              // rows above the maximum temperature
    double sep[3 * (partGrid + 1)] = {};  // the cell grid's separators per axis
    double cmin[3] = {0, 0, 0}, cmax[3] = {0, 0, 0};  // SPHGasParticleGrid::xmin() .. zmax()
    std::vector<int> cellOffset, cellList;            // the cells' particle lists, CSR
    std::vector<double> cum;       // normalized cumulative metal masses (generatePosition)
    std::vector<double> erfTable;  // erf(i * 2.5 / 5000) by the C library

    int size() const { return (int)rec.size(); }
    bool massInterface() const { return !negativeMasses; }  // SPHDustDistribution::interfaceCandidates
    PartView view() const {
        return PartView{rec.data(), sep, cellOffset.data(), cellList.data(), erfTable.data(), fdust, size()};
    }
    // SPHDustDistribution::density(bfr)
    double density(double x, double y, double z) const { return partDensity(view(), x, y, z); }
    // the number of grid cells a box spans (beyond partMergeCap a device hands the box back)
    int boxCells(const double b[6]) const {
        int lo[3], hi[3];
        const int n = partBoxCells(view(), b, lo, hi);
        return (lo[0] == hi[0] && lo[1] == hi[1] && lo[2] == hi[2]) ? 1 : n;
    }
    // SPHDustDistribution::massInBox(box), any box: the spanned lists joined as the reference's std::set orders
    // them, every particle once in ascending index
    double massInBox(const double b[6]) const {
        const PartView v = view();
        int lo[3], hi[3];
        const int ncell = partBoxCells(v, b, lo, hi);
        if ((lo[0] == hi[0] && lo[1] == hi[1] && lo[2] == hi[2]) || ncell <= partMergeCap) {
            int cur[partMergeCap];
            double mass = 0;
            partMassInBox(v, b, cur, 1, &mass);
            return mass;
        }
        std::vector<int> joined;
        for (int i = lo[0]; i <= hi[0]; i++)
            for (int j = lo[1]; j <= hi[1]; j++)
                for (int k = lo[2]; k <= hi[2]; k++) {
                    const int cell = ((i * partGrid) + j) * partGrid + k;
                    joined.insert(joined.end(), cellList.begin() + cellOffset[cell], cellList.begin() + cellOffset[cell + 1]);
                }
        std::sort(joined.begin(), joined.end());
        joined.erase(std::unique(joined.begin(), joined.end()), joined.end());
        double sum = 0.0;
        for (int id : joined) sum += partMetalMassInBox(rec[id], erfTable.data(), b);
        sum *= fdust;
        return std::max(sum, 0.);
    }
    // SPHDustDistribution::mass
    double mass() const {
        double sum = 0.0;
        for (double mz : metal) sum += mz;
        sum *= fdust;
        return std::max(sum, 0.);
    }
    // SPHDustDistribution::SigmaX / SigmaY / SigmaZ: 10000 samples along the axis between the grid's ends
    double Sigma(int axis) const {
        const int NSAMPLES = 10000;
        double sum = 0;
        const double lo = cmin[axis], hi = cmax[axis];
        for (int k = 0; k < NSAMPLES; k++) {
            const double t = lo + k * (hi - lo) / NSAMPLES;
            sum += density(axis == 0 ? t : 0, axis == 1 ? t : 0, axis == 2 ? t : 0);
        }
        return (sum / NSAMPLES) * (hi - lo);
    }
    // SPHDustDistribution::generatePosition: a particle by metal mass, then three Random::gauss
    template <class R, class Gauss>
    void generatePosition(R& rng, Gauss gauss, double& x, double& y, double& z) const {
        const int i = nr::locateClip(cum, rng.uniform());
        const double gx = gauss(rng);
        const double gy = gauss(rng);
        const double gz = gauss(rng);
        const double f = h[i] / 2.42 / M_SQRT2;
        x = rec[i].x + gx * f;
        y = rec[i].y + gy * f;
        z = rec[i].z + gz * f;
    }
};

namespace particles_detail {

// SPHGasParticleGrid.cpp makegrid: the separators of one axis from the centres binned into 100 bins per cell and
// cut at equal counts; the ends are -inf and +inf, separators never reached keep the zero fill
inline void makeGrid(const ParticleSet& s, int dir, double* grid, double& cmin, double& cmax) {
    const int n = s.size(), gridsize = partGrid;
    auto center = [&](int p) { return dir == 0 ? s.rec[p].x : dir == 1 ? s.rec[p].y : s.rec[p].z; };
    cmin = +std::numeric_limits<double>::infinity();
    cmax = -std::numeric_limits<double>::infinity();
    for (int p = 0; p < n; p++) {
        cmin = std::min(cmin, center(p) - s.h[p]);
        cmax = std::max(cmax, center(p) + s.h[p]);
    }
    const int nbins = gridsize * 100;
    const double binwidth = (cmax - cmin) / nbins;
    std::vector<int> bins(nbins);
    for (int p = 0; p < n; p++) {
        // (a centre at the very end, h = 0, would index one past the reference's vector: kept in the last bin)
        const int b = int((center(p) - cmin) / binwidth);
        bins[std::max(0, std::min(nbins - 1, b))] += 1;
    }
    for (int i = 0; i <= gridsize; i++) grid[i] = 0.0;
    grid[0] = -std::numeric_limits<double>::infinity();
    const int percell = n / gridsize;
    int cumul = 0, gridindex = 1;
    for (int binindex = 0; binindex < nbins; binindex++) {
        cumul += bins[binindex];
        if (cumul > percell * gridindex) {
            grid[gridindex] = cmin + (binindex + 1) * binwidth;
            gridindex += 1;
            if (gridindex >= gridsize) break;
        }
    }
    grid[gridsize] = std::numeric_limits<double>::infinity();
}

inline double square(double v) { return v * v; }

// Arvo's box-sphere test (SPHGasParticleGrid.cpp intersects)
inline bool intersects(double xmin, double xmax, double ymin, double ymax, double zmin, double zmax, double xc, double yc,
                       double zc, double r) {
    double squaredist = square(r);
    if (xc < xmin) squaredist -= square(xc - xmin);
    else if (xc > xmax) squaredist -= square(xc - xmax);
    if (yc < ymin) squaredist -= square(yc - ymin);
    else if (yc > ymax) squaredist -= square(yc - ymax);
    if (zc < zmin) squaredist -= square(zc - zmin);
    else if (zc > zmax) squaredist -= square(zc - zmax);
    return squaredist > 0.;
}

}  // namespace particles_detail

// SPHDustDistribution::setupSelfBefore: reads the file (TextInFile::readRow with one optional column), drops the
// particles hotter than Tmax, caches the particles' constants, builds the cell grid and the cumulative metal masses
inline std::shared_ptr<ParticleSet> readParticles(const std::string& path, double fdust, double Tmax) {
    using namespace particles_detail;
    auto sp = std::make_shared<ParticleSet>();
    ParticleSet& s = *sp;
    s.path = path;
    s.fdust = fdust;
    std::ifstream in(path.c_str());
    if (!in.is_open()) throw std::runtime_error("Could not open the SPH gas particles data file " + path);
    const double pc = constants::pc, Msun = constants::Msun;
    std::string line;
    while (in.good()) {
        std::getline(in, line);
        const auto pos = line.find_first_not_of(" \t");
        if (pos == std::string::npos || line[pos] == '#') continue;
        double v[7] = {0, 0, 0, 0, 0, 0, 0};
        std::stringstream ls(line);
        for (int i = 0; i < 7; i++) {
            if (ls.eof()) {
                if (i < 6) throw std::runtime_error("One or more required value(s) on text line are missing in " + path);
                break;
            }
            double value;
            ls >> value;
            if (ls.fail()) throw std::runtime_error("Input text is not formatted as a floating point number in " + path);
            v[i] = value;
        }
        const double T = v[6];
        if (T > 0 && Tmax > 0 && T > Tmax) {
            s.nignored++;
            continue;
        }
        // SPHGasParticle(Vec(x, y, z) * pc, h * pc, M * Msun, Z)
        const double h = v[3] * pc, M = v[4] * Msun, Z = v[5];
        PartRec r;
        r.x = v[0] * pc; r.y = v[1] * pc; r.z = v[2] * pc;
        r.norm = 1 / (h * h);
        r.rho0 = 8.0 / M_PI * M / (h * h * h) * Z;
        r.rho2 = r.rho0 * 2.0;
        r.s = 2.42 / h;
        r.mz8 = M * Z / 8.;
        s.rec.push_back(r);
        s.h.push_back(h);
        s.metal.push_back(M * Z);
        if (v[4] < 0) s.negativeMasses = true;
    }
    if (s.rec.empty()) throw std::runtime_error("the SPH gas particles data file " + path + " holds no particle");

    // SPHGasParticleGrid::SPHGasParticleGrid
    for (int a = 0; a < 3; a++) makeGrid(s, a, s.sep + a * (partGrid + 1), s.cmin[a], s.cmax[a]);
    const double *xg = s.sep, *yg = s.sep + (partGrid + 1), *zg = s.sep + 2 * (partGrid + 1);
    const int ncell = partGrid * partGrid * partGrid, n = s.size();
    // every particle joins the cells its sphere intersects, in particle order: count, then fill
    std::vector<int> count(ncell + 1, 0);
    for (int pass = 0; pass < 2; pass++) {
        for (int p = 0; p < n; p++) {
            const PartRec& r = s.rec[p];
            const double h = s.h[p];
            const int i1 = partLocate(xg, r.x - h), i2 = partLocate(xg, r.x + h);
            const int j1 = partLocate(yg, r.y - h), j2 = partLocate(yg, r.y + h);
            const int k1 = partLocate(zg, r.z - h), k2 = partLocate(zg, r.z + h);
            for (int i = i1; i <= i2; i++)
                for (int j = j1; j <= j2; j++)
                    for (int k = k1; k <= k2; k++)
                        if (intersects(xg[i], xg[i + 1], yg[j], yg[j + 1], zg[k], zg[k + 1], r.x, r.y, r.z, h)) {
                            const int cell = ((i * partGrid) + j) * partGrid + k;
                            if (pass == 0) count[cell + 1]++;
                            else s.cellList[count[cell]++] = p;
                        }
        }
        if (pass == 0) {
            for (int c = 0; c < ncell; c++) count[c + 1] += count[c];
            s.cellOffset = count;
            s.cellList.assign(count[ncell], 0);
        }
    }
    // NR::cdf over the metal masses
    nr::cdf(s.cum, s.metal);
    // initialize_myerf
    s.erfTable.resize(partErfN + 1);
    for (int i = 0; i <= partErfN; i++) s.erfTable[i] = std::erf((i * partErfMax) / partErfN);
    return sp;
}

}  // namespace skirt
