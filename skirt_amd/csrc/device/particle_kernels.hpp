// The set-up's two kernels for imported particle dust (PartArgs: engine_args.hpp; the arithmetic: particle_density.hpp):
// particleSampleKernel and particleMassKernel. Compiles only where engine.hip includes it, inside its anonymous
// namespace, beside density_sample.hpp.
#ifndef SKIRT_AMD_DEVICE_PARTICLE_KERNELS_HPP
#define SKIRT_AMD_DEVICE_PARTICLE_KERNELS_HPP

// densitySampleKernel's two modes with the particle density as the source (one component): one thread per item, its
// samples in order and each cell list in order, so every sum is the host's. PART_POINTS: the items are points (three
// doubles each, no words), the output their densities.
__global__ void __launch_bounds__(kBlock) particleSampleKernel(const PartArgs a) {
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.n) return;
    if (a.mode == SKIRT_PART_POINTS) {
        const double* p = a.boxes + 3 * q;
        a.out[q] = partDensity(a.view, p[0], p[1], p[2]);
        return;
    }
    const double* b = a.boxes + 6 * q;
    const uint32_t* w = a.words + (size_t)3 * a.nsample * q;
    constexpr double kWordMax = 4294967295.0;  // MTRandom::deviate
    double sum = 0, sx = 0, sy = 0, sz = 0, mn = 0, mx = 0;
    for (int k = 0; k < a.nsample; k++) {
        const double fx = (double)w[3 * k] / kWordMax, fy = (double)w[3 * k + 1] / kWordMax,
                     fz = (double)w[3 * k + 2] / kWordMax;
        const double x = b[0] + fx * (b[3] - b[0]), y = b[1] + fy * (b[4] - b[1]), z = b[2] + fz * (b[5] - b[2]);
        double rho = 0;  // (the host adds the one component's density to 0 as well)
        rho += partDensity(a.view, x, y, z);
        sum += rho;
        if (a.mode == SKIRT_DENS_NODE) {
            sx += rho * x;
            sy += rho * y;
            sz += rho * z;
            if (k == 0 || rho < mn) mn = rho;
            if (k == 0 || mx < rho) mx = rho;
        }
    }
    if (a.mode == SKIRT_DENS_NODE) {
        double* o = a.out + 6 * q;
        o[0] = sum; o[1] = sx; o[2] = sy; o[3] = sz; o[4] = mn; o[5] = mx;
    } else {
        a.out[q] = sum;
    }
}

// One mass per box, one thread per box; a box beyond the merge cap gets -1 (no mass is negative) and is counted
__global__ void __launch_bounds__(partMassBlock) particleMassKernel(const PartArgs a, unsigned* handedBack) {
    __shared__ int cursors[partMergeCap * partMassBlock];
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.n) return;
    double mass = 0.0;
    if (partMassInBox(a.view, a.boxes + 6 * q, cursors + threadIdx.x, partMassBlock, &mass)) {
        a.out[q] = mass;
    } else {
        a.out[q] = -1.0;
        atomicAdd(handedBack, 1u);
    }
}

#endif  // SKIRT_AMD_DEVICE_PARTICLE_KERNELS_HPP
