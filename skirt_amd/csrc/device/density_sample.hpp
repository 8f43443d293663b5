// The setup's sampling kernels (DensArgs: engine_args.hpp): geomDensity, samplePositionsKernel, sampleLaunchesKernel and
// densitySampleKernel. Compiles only where engine.hip includes it, inside its anonymous namespace, after Events
// (Events::launchPosition, launchDirection, emissionProbability).
#ifndef SKIRT_AMD_DEVICE_DENSITY_SAMPLE_HPP
#define SKIRT_AMD_DEVICE_DENSITY_SAMPLE_HPP

// ================================================================== setup: density sampling
// The setup's hot loop (skirt_mcrt_sample_density): one thread per item (a cell or a tree node), its
// samples in order, so that every sum is accumulated as the host loop accumulates it (host/densities.cpp cell
// densities, host/treegrid.cpp tree subdivision). The geometry densities follow the host's Geometry::density
// operation for operation (PlummerGeometry.cpp:49-54, ExpDiskGeometry::density, SersicGeometry::density with the
// SersicFunction log-log interpolation, PointGeometry).
__device__ double geomDensity(const DensArgs& d, int h, double x, double y, double z) {
    const double* p = d.param + 8 * h;
    switch (d.kind[h]) {
    case SKIRT_GEOM_PLUMMER: {
        const double r = sqrt(x * x + y * y + z * z);
        const double s = r / p[0];
        return p[1] * pow(1.0 + s * s, -2.5);
    }
    case SKIRT_GEOM_EXPDISK: {
        const double R = sqrt(x * x + y * y);
        const double absz = fabs(z);
        const double hR = p[0], hz = p[1], Rmax = p[2], zmax = p[3], Rmin = p[4], rho0 = p[5];
        if (Rmax > 0.0 && R > Rmax) return 0.0;
        if (zmax > 0.0 && absz > zmax) return 0.0;
        if (R < Rmin) return 0.0;
        return rho0 * exp(-R / hR) * exp(-absz / hz);
    }
    case SKIRT_GEOM_SERSIC: {
        const double r = sqrt(x * x + y * y + z * z);
        const double s = r / p[0];
        const double* sv = d.table + (size_t)2 * d.ntab * h;
        const double* Sv = sv + d.ntab;
        const int Ns = d.ntab;
        if (s <= sv[0]) return p[2] * Sv[0];
        if (s >= sv[Ns - 1]) return p[2] * Sv[Ns - 1];
        int jl = -1, ju = Ns - 1;  // NR::locate_clip (s >= sv[0] here)
        while (ju - jl > 1) {
            const int jm = (ju + jl) >> 1;
            if (s < sv[jm]) ju = jm;
            else jl = jm;
        }
        // NR::interpolate_loglog
        const double lx = log10(s), x1 = log10(sv[jl]), x2 = log10(sv[jl + 1]);
        double f1 = Sv[jl], f2 = Sv[jl + 1];
        const bool logf = f1 > 0 && f2 > 0;
        if (logf) { f1 = log10(f1); f2 = log10(f2); }
        double fx = f1 + ((lx - x1) / (x2 - x1)) * (f2 - f1);
        if (logf) fx = pow(10.0, fx);
        return p[2] * fx;
    }
    case SKIRT_GEOM_POINT:
        return (x * x + y * y + z * z) == 0 ? INFINITY : 0.0;
    default:  // the six closed-form kinds (geom_sample.hpp)
        return geomDensityOf(d.kind[h], p, d.table ? d.table + (size_t)2 * d.ntab * h : nullptr, x, y, z);
    }
}

// Geometry::generatePosition of one source component on fresh per-packet streams (skirt_mcrt_sample_positions):
// the routines Events::launchStellar runs, one packet per thread
__global__ void __launch_bounds__(kBlock)
    samplePositionsKernel(const double* geomParam, const double* geomTable, int h, unsigned long long seed,
                          unsigned long long first, size_t n, double* pos, int* draws, unsigned* error) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PacketRng rng;
    rng.start(seed, SKIRT_POSITIONS_TAG, first + i);
    double x = 0.0, y = 0.0, z = 0.0;
    if (!Events<SKIRT_GRID_CARTESIAN, true>::launchPosition(geomParam + 8 * h, geomTable, h, rng, x, y, z))
        atomicOr(error, ERR_GEOM);
    pos[3 * i] = x; pos[3 * i + 1] = y; pos[3 * i + 2] = z;
    draws[i] = (int)(2u * rng.block - (rng.have ? 1u : 0u));
}

// GeometricStellarComp::launch of one source component on fresh per-packet streams (skirt_mcrt_sample_launches): the
// position and the direction by the routines Events::launchStellar runs in a phase with an anisotropic component,
// one packet per thread; then probabilityForDirection, by the emission peel-off's routine, of nprob given
// directions at given positions (ppos) or at the positions just launched (ppos null, nprob <= n)
__global__ void __launch_bounds__(kBlock)
    sampleLaunchesKernel(const double* geomParam, const double* geomTable, int nstar, int h, unsigned long long seed,
                         unsigned long long first, size_t n, double* pos, double* dir, int* draws, size_t nprob,
                         const double* ppos, const double* pdir, double* prob, unsigned* error) {
    using E = Events<SKIRT_GRID_CARTESIAN, true, false, true>;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double* gp = geomParam + 8 * h;
    double x = 0.0, y = 0.0, z = 0.0;
    if (i < n) {
        PacketRng rng;
        rng.start(seed, SKIRT_LAUNCHES_TAG, first + i);
        double kx = 0.0, ky = 0.0, kz = 1.0;
        if (!E::launchPosition(gp, geomTable, h, rng, x, y, z)) atomicOr(error, ERR_GEOM);
        else E::launchDirection(gp, geomParam + 8 * nstar, rng, x, y, z, kx, ky, kz);
        pos[3 * i] = x; pos[3 * i + 1] = y; pos[3 * i + 2] = z;
        dir[3 * i] = kx; dir[3 * i + 1] = ky; dir[3 * i + 2] = kz;
        draws[i] = (int)(2u * rng.block - (rng.have ? 1u : 0u));
    }
    if (i < nprob) {
        if (ppos) { x = ppos[3 * i]; y = ppos[3 * i + 1]; z = ppos[3 * i + 2]; }
        prob[i] = E::emissionProbability(gp, x, y, z, pdir[3 * i], pdir[3 * i + 1], pdir[3 * i + 2]);
    }
}

__global__ void __launch_bounds__(kBlock) densitySampleKernel(const DensArgs d) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= d.n) return;
    const double* b = d.boxes + 6 * q;
    const uint32_t* w = d.words + (size_t)3 * d.nsample * q;
    constexpr double kWordMax = 4294967295.0;  // MTRandom::deviate
    if (d.mode == SKIRT_DENS_COMPONENTS) {
        double* o = d.out + (size_t)d.ncomp * q;
        for (int h = 0; h < d.ncomp; h++) o[h] = 0.0;
        for (int k = 0; k < d.nsample; k++) {
            const double fx = (double)w[3 * k] / kWordMax, fy = (double)w[3 * k + 1] / kWordMax,
                         fz = (double)w[3 * k + 2] / kWordMax;
            const double x = b[0] + fx * (b[3] - b[0]), y = b[1] + fy * (b[4] - b[1]), z = b[2] + fz * (b[5] - b[2]);
            for (int h = 0; h < d.ncomp; h++) o[h] += d.norm[h] * geomDensity(d, h, x, y, z);
        }
    } else {
        double sum = 0, sx = 0, sy = 0, sz = 0, mn = 0, mx = 0;
        for (int k = 0; k < d.nsample; k++) {
            const double fx = (double)w[3 * k] / kWordMax, fy = (double)w[3 * k + 1] / kWordMax,
                         fz = (double)w[3 * k + 2] / kWordMax;
            const double x = b[0] + fx * (b[3] - b[0]), y = b[1] + fy * (b[4] - b[1]), z = b[2] + fz * (b[5] - b[2]);
            double rho = 0;
            for (int h = 0; h < d.ncomp; h++) rho += d.norm[h] * geomDensity(d, h, x, y, z);
            sum += rho;
            sx += rho * x;
            sy += rho * y;
            sz += rho * z;
            if (k == 0 || rho < mn) mn = rho;  // std::min_element / max_element: the first extreme
            if (k == 0 || mx < rho) mx = rho;
        }
        double* o = d.out + 6 * q;
        o[0] = sum; o[1] = sx; o[2] = sy; o[3] = sz; o[4] = mn; o[5] = mx;
    }
}

#endif  // SKIRT_AMD_DEVICE_DENSITY_SAMPLE_HPP
