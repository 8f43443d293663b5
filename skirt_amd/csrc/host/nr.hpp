// Small numeric helpers of the reference's Fundamentals/NR.hpp, as the host set-up and the dust emission use them.
#pragma once

#include <cmath>
#include <numeric>
#include <vector>

#pragma GCC visibility push(hidden)  // the library's own: not among its dynamic symbols
namespace skirt {
namespace nr {

// NR::locate_basic_impl / locate / locate_clip / locate_fail (NR.hpp Array versions)
inline int locateBasic(const std::vector<double>& xv, double x, int n) {
    int jl = -1, ju = n;
    while (ju - jl > 1) {
        int jm = (ju + jl) >> 1;
        if (x < xv[jm]) ju = jm;
        else jl = jm;
    }
    return jl;
}
inline int locate(const std::vector<double>& xv, double x) {
    int n = (int)xv.size();
    if (x == xv[n - 1]) return n - 2;
    return locateBasic(xv, x, n);
}
inline int locateClip(const std::vector<double>& xv, double x) {
    if (x < xv[0]) return 0;
    return locateBasic(xv, x, (int)xv.size() - 1);
}
inline int locateFail(const std::vector<double>& xv, double x) {
    int n = (int)xv.size();
    if (x > xv[n - 1]) return -1;
    return locateBasic(xv, x, n - 1);
}
inline double interpolateLinLin(double x, double x1, double x2, double f1, double f2) {
    return f1 + ((x - x1) / (x2 - x1)) * (f2 - f1);
}
inline double interpolateLogLin(double x, double x1, double x2, double f1, double f2) {
    x = std::log10(x);
    x1 = std::log10(x1);
    x2 = std::log10(x2);
    return f1 + ((x - x1) / (x2 - x1)) * (f2 - f1);
}
inline double interpolateLogLog(double x, double x1, double x2, double f1, double f2) {
    x = std::log10(x);
    x1 = std::log10(x1);
    x2 = std::log10(x2);
    bool logf = f1 > 0 && f2 > 0;
    if (logf) {
        f1 = std::log10(f1);
        f2 = std::log10(f2);
    }
    double fx = f1 + ((x - x1) / (x2 - x1)) * (f2 - f1);
    if (logf) fx = std::pow(10, fx);
    return fx;
}
// NR::resample (NR.hpp:355-378)
template <double interp(double, double, double, double, double)>
std::vector<double> resample(const std::vector<double>& xres, const std::vector<double>& xori,
                             const std::vector<double>& yori) {
    int Nori = (int)xori.size();
    double xmin = xori[0], xmax = xori[Nori - 1];
    std::vector<double> yres(xres.size(), 0.0);
    for (size_t l = 0; l < xres.size(); l++) {
        double x = xres[l];
        if (std::fabs(1.0 - x / xmin) < 1e-5) yres[l] = yori[0];
        else if (std::fabs(1.0 - x / xmax) < 1e-5) yres[l] = yori[Nori - 1];
        else if (x < xmin || x > xmax) yres[l] = 0.0;
        else {
            int k = locate(xori, x);
            yres[l] = interp(x, xori[k], xori[k + 1], yori[k], yori[k + 1]);
        }
    }
    return yres;
}
// NR::cdf with a source vector (NR.hpp:388-394)
inline void cdf(std::vector<double>& Pv, const std::vector<double>& pv) {
    size_t n = pv.size();
    Pv.assign(n + 1, 0.0);
    for (size_t i = 0; i < n; i++) Pv[i + 1] = Pv[i] + pv[i];
    double norm = Pv[n];
    for (auto& v : Pv) v /= norm;
}
inline double sum(const std::vector<double>& v) { return std::accumulate(v.begin(), v.end(), 0.); }

}  // namespace nr
}  // namespace skirt
#pragma GCC visibility pop
