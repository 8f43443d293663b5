// Dust mixes: the packaged resource tables, the four mixes of the .ski files with what DustMix::setupSelfAfter
// derives from them (DustMix.cpp:44-264), the polarisation tables, and DustMix::kappaext(lambda).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <stdexcept>

#include "nr.hpp"
#include "ski_parse.hpp"

namespace skirt {

Table readTable(const std::string& datadir, const std::string& name) {
    std::string path = datadir + "/" + name;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open resource table " + path);
    Table t;
    int64_t hdr[2];
    if (std::fread(hdr, sizeof(int64_t), 2, f) != 2) { std::fclose(f); throw std::runtime_error("bad table " + path); }
    t.nrows = hdr[0];
    t.ncols = hdr[1];
    t.v.resize(t.nrows * t.ncols);
    size_t got = std::fread(t.v.data(), sizeof(double), t.v.size(), f);
    std::fclose(f);
    if (got != t.v.size()) throw std::runtime_error("truncated table " + path);
    return t;
}

namespace {

// DustMix::setupSelfAfter part 1 (DustMix.cpp:47-89): population sums, albedo, g, kappa = sigma/mu
void finishMix(DustMix& mix, const std::vector<double>& muv, const std::vector<std::vector<double>>& sabs,
               const std::vector<std::vector<double>>& ssca, const std::vector<std::vector<double>>& gv, int Nlambda) {
    int Npop = (int)muv.size();
    if (Npop < 1) throw std::runtime_error("dust mixture must contain at least one dust population");
    std::vector<double> sigmaabs(Nlambda), sigmasca(Nlambda), sigmaext(Nlambda);
    mix.albedo.assign(Nlambda, 0);
    mix.g.assign(Nlambda, 0);
    for (int ell = 0; ell < Nlambda; ell++) {
        double sumabs = 0.0, sumsca = 0.0, sumgsca = 0.0;
        for (int c = 0; c < Npop; c++) {
            sumabs += sabs[c][ell];
            sumsca += ssca[c][ell];
            sumgsca += gv[c][ell] * ssca[c][ell];
        }
        double sumext = sumabs + sumsca;
        sigmaabs[ell] = sumabs;
        sigmasca[ell] = sumsca;
        sigmaext[ell] = sumext;
        mix.albedo[ell] = sumext ? sumsca / sumext : 0.;
        mix.g[ell] = sumsca ? sumgsca / sumsca : 0.;
    }
    double mu = 0.0;
    for (int c = 0; c < Npop; c++) mu += muv[c];
    mix.mu = mu;
    mix.sigmaabs = sigmaabs;
    mix.kabs.resize(Nlambda);
    mix.ksca.resize(Nlambda);
    mix.kext.resize(Nlambda);
    for (int ell = 0; ell < Nlambda; ell++) {
        mix.kabs[ell] = sigmaabs[ell] / mu;
        mix.ksca[ell] = sigmasca[ell] / mu;
        mix.kext[ell] = sigmaext[ell] / mu;
    }
}

// What DustMix::setupSelfAfter derives from a polarising mix's Mueller tables (DustMix.cpp:96-123), in its
// operations and order: the normalized cumulative distribution of theta (NR::cdf over S11(t+1) sin theta(t+1) dt)
// and the phase function normalization per wavelength. (The phi tables, the same for every mix, are the engine's:
// device/polarization.hpp polPhiTables.)
void finishPolarization(DustMix& mix, int Nlambda) {
    const int Ntheta = mix.ntheta;
    std::vector<double> thetav(Ntheta);
    const double dt = M_PI / (Ntheta - 1);
    for (int t = 0; t < Ntheta; t++) thetav[t] = t * dt;
    mix.thetaX.assign((size_t)Nlambda * Ntheta, 0.0);
    mix.pfnorm.assign(Nlambda, 0.0);
    for (int ell = 0; ell < Nlambda; ell++) {
        const double* S11 = &mix.S11[(size_t)ell * Ntheta];
        double* Pv = &mix.thetaX[(size_t)ell * Ntheta];
        for (int i = 0; i < Ntheta - 1; i++) Pv[i + 1] = Pv[i] + S11[i + 1] * sin(thetav[i + 1]) * dt;
        const double norm = Pv[Ntheta - 1];
        for (int i = 0; i < Ntheta; i++) Pv[i] /= norm;
    }
    for (int ell = 0; ell < Nlambda; ell++) {
        const double* S11 = &mix.S11[(size_t)ell * Ntheta];
        double sum = 0.;
        for (int t = 0; t < Ntheta; t++) sum += S11[t] * sin(thetav[t]) * dt;
        mix.pfnorm[ell] = 2.0 / sum;
    }
}

}  // namespace

DustMix parseMix(const Ctx& c, const XmlElement* e, const WavelengthGrid& wl) {
    DustMix mix;
    mix.type = e->name;
    int Nlambda = wl.n();
    std::vector<double> muv;
    std::vector<std::vector<double>> sabs, ssca, gv;
    if (e->name == "SimpleOligoDustMix") {
        // SimpleOligoDustMix.cpp setupSelfBefore: kappaabs = kext*(albedo+1), kappasca = kext*albedo,
        // population mass 1/kext[0] (the reference's quirk is kept on purpose)
        if (wl.pan) throw std::runtime_error("SimpleOligoDustMix requires an oligochromatic wavelength grid");
        std::vector<double> kext = attrList(c, e, "opacities", "opacity");
        std::vector<double> alb = attrList(c, e, "albedos", "");
        std::vector<double> asy = attrList(c, e, "asymmetryParameters", "");
        if ((int)kext.size() != Nlambda || (int)alb.size() != Nlambda || (int)asy.size() != Nlambda)
            throw std::runtime_error("SimpleOligoDustMix property list length differs from the number of wavelengths");
        std::vector<double> ka(Nlambda), ks(Nlambda), g(Nlambda);
        for (int ell = 0; ell < Nlambda; ell++) {
            ka[ell] = kext[ell] * (alb[ell] + 1.0);
            ks[ell] = kext[ell] * alb[ell];
            g[ell] = asy[ell];
        }
        double Mdust = 1.0 / kext[0];
        if (Mdust > 0) { muv.push_back(Mdust); sabs.push_back(ka); ssca.push_back(ks); gv.push_back(g); }
    } else if (e->name == "InterstellarDustMix") {
        // InterstellarDustMix.cpp setupSelfBefore + DustMix::addpopulation with resampling
        Table t = readTable(c.datadir, "InterstellarDustMix.bin");
        const int N = 1064;
        if (t.nrows != N || t.ncols != 6) throw std::runtime_error("unexpected InterstellarDustMix table shape");
        std::vector<double> lambdav(N), kabsv(N), kscav(N), gvv(N);
        for (int row = 0, k = N - 1; k >= 0; k--, row++) {
            double lambda = t.at(row, 0), albedo = t.at(row, 1), asymmpar = t.at(row, 2), Kabs = t.at(row, 4);
            lambda *= 1e-6;
            Kabs *= 1e-1;
            lambdav[k] = lambda;
            kabsv[k] = Kabs;
            kscav[k] = Kabs * albedo / (1.0 - albedo);
            gvv[k] = asymmpar;
        }
        double eps = 0.5e-5;
        if (wl.lambda[0] < lambdav[0] * (1 - eps) || wl.lambda[Nlambda - 1] > lambdav[N - 1] * (1 + eps))
            throw std::runtime_error("dust properties not defined over the simulation's wavelength range");
        muv.push_back(1.);
        sabs.push_back(nr::resample<nr::interpolateLogLog>(wl.lambda, lambdav, kabsv));
        ssca.push_back(nr::resample<nr::interpolateLogLog>(wl.lambda, lambdav, kscav));
        gv.push_back(nr::resample<nr::interpolateLogLin>(wl.lambda, lambdav, gvv));
    } else if (e->name == "MeanZubkoDustMix" || e->name == "DraineLiDustMix") {
        // MeanZubkoDustMix.cpp / DraineLiDustMix.cpp setupSelfBefore: cross sections per H atom, then
        // DustMix::addpopulation(mu, ...) (DustMix.cpp:300-321) with its wavelength check and resampling
        const bool zubko = e->name == "MeanZubkoDustMix";
        Table t = readTable(c.datadir, zubko ? "MeanZubkoDustMix.bin" : "DraineLiDustMix.bin");
        const int N = zubko ? 1201 : 800;
        if (t.nrows != N || t.ncols != 6) throw std::runtime_error("unexpected " + e->name + " table shape");
        std::vector<double> lambdav(N), sabsv(N), sscav(N), gvv(N);
        for (int k = 0; k < N; k++) {
            lambdav[k] = t.at(k, 0) * 1e-6;
            if (zubko) {
                const double sigmaext = t.at(k, 3) * 1e-4;
                const double albedo = t.at(k, 4);
                sabsv[k] = (1. - albedo) * sigmaext;
                sscav[k] = albedo * sigmaext;
            } else {
                sabsv[k] = t.at(k, 1) * 1e-4;
                sscav[k] = t.at(k, 2) * 1e-4;
            }
            gvv[k] = t.at(k, 5);
        }
        double eps = 0.5e-5;
        if (wl.lambda[0] < lambdav[0] * (1 - eps) || wl.lambda[Nlambda - 1] > lambdav[N - 1] * (1 + eps))
            throw std::runtime_error("dust properties not defined over the simulation's wavelength range");
        const double MdustoverMH = 5.4e-4 + 5.4e-4 + 1.8e-4 + 2.33e-3 + 8.27e-3;
        muv.push_back(zubko ? 1.44e-29 : MdustoverMH * constants::mproton);
        sabs.push_back(nr::resample<nr::interpolateLogLog>(wl.lambda, lambdav, sabsv));
        ssca.push_back(nr::resample<nr::interpolateLogLog>(wl.lambda, lambdav, sscav));
        gv.push_back(nr::resample<nr::interpolateLogLin>(wl.lambda, lambdav, gvv));
    } else if (e->name == "ElectronDustMix") {
        // ElectronDustMix.cpp setupSelfBefore: Thomson scattering, no absorption, one population of electrons, and
        // the Mueller matrix of equation (C.7) of Wolf 2003 at 181 angles, the same at every wavelength
        const int Ntheta = 181;
        std::vector<double> zero(Nlambda, 0.0), sigmasca(Nlambda, constants::sigmaThomson);
        mix.polarization = true;
        mix.ntheta = Ntheta;
        for (std::vector<double>* S : {&mix.S11, &mix.S12, &mix.S33, &mix.S34}) S->assign((size_t)Nlambda * Ntheta, 0.0);
        const double dt = M_PI / (Ntheta - 1);
        for (int t = 0; t < Ntheta; t++) {
            const double theta = t * dt;
            const double costheta = cos(theta);
            const double S11 = 0.5 * (costheta * costheta + 1.);
            const double S12 = 0.5 * (costheta * costheta - 1.);
            const double S33 = costheta;
            for (int ell = 0; ell < Nlambda; ell++) {
                mix.S11[(size_t)ell * Ntheta + t] = S11;
                mix.S12[(size_t)ell * Ntheta + t] = S12;
                mix.S33[(size_t)ell * Ntheta + t] = S33;
            }
        }
        muv.push_back(constants::melectron);
        sabs.push_back(zero);
        ssca.push_back(sigmasca);
        gv.push_back(zero);
    } else {
        throw std::runtime_error("unsupported dust mix " + e->name);
    }
    finishMix(mix, muv, sabs, ssca, gv, Nlambda);
    if (mix.polarization) finishPolarization(mix, Nlambda);
    return mix;
}

// DustMix::kappaext(lambda) (DustMix.cpp:482-522): log-log interpolation on a panchromatic grid, the
// matching wavelength (to 1e-5) of an oligochromatic one
double mixKappaext(const DustMix& mix, const WavelengthGrid& wl, double lambda) {
    if (wl.pan) {
        const int ell = nr::locateFail(wl.lambda, lambda);
        if (ell < 0) throw std::runtime_error("Optical properties are not defined for this wavelength");
        const double p = (std::log10(lambda) - std::log10(wl.lambda[ell])) /
                         (std::log10(wl.lambda[ell + 1]) - std::log10(wl.lambda[ell]));
        const double kL = mix.kext[ell], kR = mix.kext[ell + 1];
        if (kL > 0 && kR > 0) {
            const double lL = std::log10(kL), lR = std::log10(kR);
            return std::pow(10, lL + p * (lR - lL));
        }
        return kL + p * (kR - kL);
    }
    for (int ell = 0; ell < wl.n(); ell++)
        if (std::fabs(lambda / wl.lambda[ell] - 1.0) < 1e-5) return mix.kext[ell];
    throw std::runtime_error("Optical properties are not defined for this wavelength");
}

}  // namespace skirt
