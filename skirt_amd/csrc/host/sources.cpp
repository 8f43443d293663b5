// Sources: the wavelength grids, the stellar components' SEDs and luminosities, and the stellar system
// (StellarSystem.cpp:35-52).
#include <algorithm>
#include <cmath>
#include <stdexcept>

#include "dustemission.hpp"
#include "nr.hpp"
#include "ski_parse.hpp"

namespace skirt {

// ------------------------------------------------------------ wavelength grids
WavelengthGrid parseWavelengthGrid(const Ctx& c, const XmlElement* w) {
    WavelengthGrid wl;
    if (w->name == "OligoWavelengthGrid") {
        wl.pan = false;
        wl.lambda = attrList(c, w, "wavelengths", "wavelength");
        std::sort(wl.lambda.begin(), wl.lambda.end());
        wl.dlambda.resize(wl.lambda.size());
        for (size_t ell = 0; ell < wl.lambda.size(); ell++) wl.dlambda[ell] = 0.001 * wl.lambda[ell];
    } else if (w->name == "LogWavelengthGrid") {
        wl.pan = true;
        double lmin = attr(c, w, "minWavelength", "wavelength", 0);
        double lmax = attr(c, w, "maxWavelength", "wavelength", 0);
        int N = attrInt(w, "points", 0);
        if (lmin <= 0 || lmax <= lmin || N < 3) throw std::runtime_error("invalid LogWavelengthGrid");
        // NR::loggrid(_lambdav, lmin, lmax, N-1)  (LogWavelengthGrid.cpp, NR.hpp:269-275)
        int n = N - 1;
        wl.lambda.resize(n + 1);
        double logxmin = std::log10(lmin);
        double dlogx = std::log10(lmax / lmin) / n;
        for (int i = 0; i <= n; i++) wl.lambda[i] = std::pow(10, logxmin + i * dlogx);
        wl.dlambda.resize(N);
        for (int ell = 0; ell < N; ell++) wl.dlambda[ell] = wl.lambdamax(ell) - wl.lambdamin(ell);
    } else {
        throw std::runtime_error("unsupported wavelength grid " + w->name);
    }
    for (int ell = 1; ell < wl.n(); ell++)
        if (wl.lambda[ell] <= wl.lambda[ell - 1]) throw std::runtime_error("wavelengths should be sorted");
    return wl;
}

namespace {

// ------------------------------------------------------------ stellar components
std::vector<double> sunLuminosityOligo(const Ctx& c, const WavelengthGrid& wl, const std::vector<double>& lum) {
    // OligoStellarComp.cpp setupSelfBefore
    Table t = readTable(c.datadir, "SunSED.bin");
    int Ns = (int)t.nrows;
    std::vector<double> lsun(Ns), Lsun(Ns);
    for (int k = 0; k < Ns; k++) {
        lsun[k] = t.at(k, 0) / 1e6;
        Lsun[k] = t.at(k, 1) * 1e6;
    }
    std::vector<double> Lv(wl.n());
    for (int ell = 0; ell < wl.n(); ell++) {
        double lambda = wl.lambda[ell];
        int k = nr::locateFail(lsun, lambda);
        if (k < 0) throw std::runtime_error("the sun does not emit at the wavelength of the simulation");
        double L = nr::interpolateLinLin(lambda, lsun[k], lsun[k + 1], Lsun[k], Lsun[k + 1]);
        Lv[ell] = lum[ell] * L * wl.dlambda[ell];
    }
    return Lv;
}

// SED::setluminosities (SED.cpp): normalized to unit sum
std::vector<double> normalizedSed(std::vector<double> Lv) {
    const double s = nr::sum(Lv);
    if (s <= 0) throw std::runtime_error("the total luminosity in the SED is zero or negative");
    for (auto& v : Lv) v /= s;
    return Lv;
}

std::vector<double> sunSedNormalized(const Ctx& c, const WavelengthGrid& wl) {
    // SunSED.cpp setupSelfBefore -> SED::setemissivities (SED.cpp) -> setluminosities
    Table t = readTable(c.datadir, "SunSED.bin");
    int Ns = (int)t.nrows;
    std::vector<double> lv(Ns), jv(Ns);
    for (int k = 0; k < Ns; k++) {
        lv[k] = t.at(k, 0) / 1e6;
        jv[k] = t.at(k, 1);
    }
    std::vector<double> j = nr::resample<nr::interpolateLogLog>(wl.lambda, lv, jv);
    std::vector<double> Lv(wl.n());
    for (int ell = 0; ell < wl.n(); ell++) Lv[ell] = j[ell] * wl.dlambda[ell];
    return normalizedSed(Lv);
}

std::vector<double> blackBodySedNormalized(double T, const WavelengthGrid& wl) {
    // BlackBodySED.cpp setupSelfBefore: per wavelength bin, the 101-point trapezoid rule of B(lambda)
    // lambda over log10(lambda) between lambdamin and lambdamax, times ln 10 dloglambda
    if (T <= 0) throw std::runtime_error("the black body temperature T should be positive");
    std::vector<double> Lv(wl.n());
    for (int ell = 0; ell < wl.n(); ell++) {
        const int N = 100;
        const double loglambdamin = std::log10(wl.lambdamin(ell));
        const double loglambdamax = std::log10(wl.lambdamax(ell));
        const double dloglambda = (loglambdamax - loglambdamin) / N;
        double sum = 0;
        for (int i = 0; i <= N; i++) {
            double weight = 1.0;
            if (i == 0 || i == N) weight = 0.5;
            const double loglambda = loglambdamin + i * dloglambda;
            const double lambda = std::pow(10, loglambda);
            sum += weight * planckFunction(T, lambda) * lambda;
        }
        Lv[ell] = sum * M_LN10 * dloglambda;
    }
    return normalizedSed(Lv);
}

std::vector<double> quasarSedNormalized(const WavelengthGrid& wl) {
    // QuasarSED.cpp setupSelfBefore: a broken power law in micron, then SED::setemissivities
    std::vector<double> Lv(wl.n());
    for (int ell = 0; ell < wl.n(); ell++) {
        double lambda = wl.lambda[ell];
        lambda *= 1e6;
        double j = 0.0;
        const double a = 1.0, b = 0.003981072, cq = 0.001258926, d = 0.070376103;
        if (lambda < 0.001) j = 0.0;
        else if (lambda < 0.01) j = a * std::pow(lambda, 0.2);
        else if (lambda < 0.1) j = b * std::pow(lambda, -1.0);
        else if (lambda < 5.0) j = cq * std::pow(lambda, -1.5);
        else if (lambda < 1000.0) j = d * std::pow(lambda, -4.0);
        else j = 0.0;
        Lv[ell] = j * wl.dlambda[ell];
    }
    return normalizedSed(Lv);
}

}  // namespace

void parseStellarSystem(const Ctx& c, const XmlElement* ss, Model& m) {
    const int Nlambda = m.wl.n();
    m.starEmissionBias = attr(c, ss, "emissionBias", "", 0.5);
    for (const XmlElement* sc : ss->items("components")) {
        if (sc->name == "SPHStellarComp")  // imported star particles take an SED family
            throw std::runtime_error("SPHStellarComp is not supported: its SED family tables (Bruzual-Charlot) are "
                                     "not packaged");
        m.starGeom.push_back(parseGeometry(c, need(sc, "geometry")));
        if (sc->name == "OligoStellarComp") {
            if (m.pan) throw std::runtime_error("OligoStellarComp requires an oligochromatic simulation");
            std::vector<double> lum = attrList(c, sc, "luminosities", "");
            if ((int)lum.size() != Nlambda) throw std::runtime_error("number of luminosities differs from number of wavelengths");
            m.starL.push_back(sunLuminosityOligo(c, m.wl, lum));
        } else if (sc->name == "PanStellarComp") {
            const XmlElement* sed = need(sc, "sed");
            const XmlElement* norm = need(sc, "normalization");
            if (norm->name != "BolLuminosityStellarCompNormalization")
                throw std::runtime_error("unsupported stellar normalization " + norm->name);
            double Lsunits = attr(c, norm, "luminosity", "", 0);
            if (Lsunits <= 0) throw std::runtime_error("the bolometric luminosity should be positive");
            double Ltot = Lsunits * constants::Lsun;
            std::vector<double> sedL;
            if (sed->name == "SunSED") sedL = sunSedNormalized(c, m.wl);
            else if (sed->name == "BlackBodySED") sedL = blackBodySedNormalized(attr(c, sed, "temperature", "temperature", 0), m.wl);
            else if (sed->name == "QuasarSED") sedL = quasarSedNormalized(m.wl);
            else throw std::runtime_error("unsupported stellar SED " + sed->name);
            std::vector<double> Lv(Nlambda);
            for (int ell = 0; ell < Nlambda; ell++) Lv[ell] = Ltot * sedL[ell];
            m.starL.push_back(Lv);
        } else {
            throw std::runtime_error("unsupported stellar component " + sc->name);
        }
    }
    if (m.starL.empty()) throw std::runtime_error("there are no stellar components");
    {
        int Ncomp = (int)m.starL.size();
        m.starLtot.assign(Nlambda, 0.0);
        m.starX.assign(Nlambda, {});
        for (int ell = 0; ell < Nlambda; ell++) {
            for (int h = 0; h < Ncomp; h++) m.starLtot[ell] += m.starL[h][ell];
            std::vector<double> pv(Ncomp);
            for (int h = 0; h < Ncomp; h++) pv[h] = m.starL[h][ell];
            nr::cdf(m.starX[ell], pv);
        }
    }
}

}  // namespace skirt
