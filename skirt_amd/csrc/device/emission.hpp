// Dust emission sources on the device (their arguments: EmisArgs, engine_args.hpp): the cell-spectra, scan, CDF and
// guide kernels, and the guided table lookups the event side draws cells with.
// Compiles only where engine.hip includes it, inside its anonymous namespace.
#ifndef SKIRT_AMD_DEVICE_EMISSION_HPP
#define SKIRT_AMD_DEVICE_EMISSION_HPP

// ================================================================== dust emission sources on the device
// The grey-body emission spectrum of every cell and the per-wavelength cell distribution of the dust
// phases (DustLib::calculate with AllCellsDustLib + GreyBodyDustEmissivity, DustLib.cpp:60-185,
// GreyBodyDustEmissivity.cpp:19-43, DustMix::equilibrium DustMix.cpp:689-712; cell luminosities and
// NR::cdf of PanMonteCarloSimulation.cpp:193-205, 273-294), computed from the device tallies so the
// self-absorption cycles never leave the GPU. Reference cell order, like the host restatement
// (host/dustemission.cpp), which the tests compare against.
__device__ __forceinline__ double planckB(double T, double lambda) {  // PlanckFunction
    const double h = 6.62606957e-34, c = 2.99792458e8, k = 1.3806488e-23;
    const double x = h * c / (lambda * k * T);
    return 2.0 * h * c * c / pow(lambda, 5) / (exp(x) - 1.0);
}

__global__ void __launch_bounds__(kBlock) cellSpectraKernel(const EmisArgs e) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= e.ncells) return;
    const int Nl = e.nlambda;
    const size_t S = e.labsStride;
    const int dm = e.devCell ? e.devCell[m] : m;
    // PanDustSystem::Labs(m): stellar sum, continued by the dust sum
    double Labsbol = 0;
    for (int ell = 0; ell < Nl; ell++) Labsbol += e.labs[ell * S + dm];
    if (e.labsDust)
        for (int ell = 0; ell < Nl; ell++) Labsbol += e.labsDust[ell * S + dm];
    // J_lambda is needed only for the absorbed power of each component, and the emission spectrum Lv is
    // accumulated in the cell's own column of the output (the arithmetic of the host restatement, one
    // operation at a time), so any number of wavelengths fits
    const double fac = 4.0 * M_PI * e.volume[m];
    auto meanIntensity = [&](int ell) {  // DustSystem::meanintensityv
        double L = 0;
        L += e.labs[ell * S + dm];
        if (e.labsDust) L += e.labsDust[ell * S + dm];
        double kr = 0.0;
        for (int h = 0; h < e.ncomp; h++) kr += e.kabs[h * Nl + ell] * e.rho[(size_t)dm * e.ncomp + h];
        const double J = L / (kr * fac) / e.dlambda[ell];
        return isfinite(J) ? J : 0.0;
    };
    double* Lv = e.lv + m;  // Lv[ell] at Lv[ell * ncells]
    const size_t N = e.ncells;
    for (int ell = 0; ell < Nl; ell++) Lv[ell * N] = 0.0;
    for (int h = 0; h < e.ncomp; h++) {
        // DustMix::equilibrium -> invplanckabs (NR::locate_clip + linear interpolation)
        const double* sa = e.sigmaabs + h * Nl;
        double pa = 0.0;
        for (int ell = 0; ell < Nl; ell++) pa += sa[ell] * meanIntensity(ell) * e.dlambda[ell];
        const double* tab = e.planckabs + (size_t)h * e.ntemp;
        int p;
        if (pa < tab[0]) p = 0;
        else {
            int jl = -1, ju = e.ntemp - 1;
            while (ju - jl > 1) { const int jm = (ju + jl) >> 1; if (pa < tab[jm]) ju = jm; else jl = jm; }
            p = jl;
        }
        const double T = e.Tv[p] + ((pa - tab[p]) / (tab[p + 1] - tab[p])) * (e.Tv[p + 1] - e.Tv[p]);
        const double w = e.ncomp > 1 ? e.rho[(size_t)dm * e.ncomp + h] : 1.0;
        for (int ell = 0; ell < Nl; ell++) {
            double ev = 0.0;
            ev += sa[ell] * planckB(T, e.lambda[ell]);
            ev /= e.mu[h];
            if (e.ncomp > 1) Lv[ell * N] += ev * w;
            else Lv[ell * N] = ev;
        }
    }
    double total = 0.0;
    for (int ell = 0; ell < Nl; ell++) {
        const double v = Lv[ell * N] * e.dlambda[ell];
        Lv[ell * N] = v;
        total += v;
    }
    for (int ell = 0; ell < Nl; ell++) {
        const double lum = total > 0 ? Lv[ell * N] / total : Lv[ell * N];
        Lv[ell * N] = Labsbol > 0.0 ? Labsbol * lum : 0.0;
    }
}

// per wavelength: sums of kBlock consecutive cells
__global__ void __launch_bounds__(kBlock) cellBlockSumKernel(const EmisArgs e) {
    __shared__ double red[kBlock];
    const int ell = blockIdx.y, b = blockIdx.x, m = b * kBlock + threadIdx.x;
    red[threadIdx.x] = m < e.ncells ? e.lv[(size_t)ell * e.ncells + m] : 0.0;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) e.blockSums[(size_t)ell * e.nblocks + b] = red[0];
}

// per wavelength (one block each): exclusive scan of the block sums and the total. Each thread sums a
// contiguous chunk of the block sums, the chunk sums are scanned in LDS, and each thread then writes its
// chunk's exclusive prefixes (a single thread walking all block sums took 3 ms per call on C5).
__global__ void __launch_bounds__(kBlock) cellScanBlocksKernel(const EmisArgs e) {
    __shared__ double part[kBlock];
    const int ell = blockIdx.x;
    double* bs = e.blockSums + (size_t)ell * e.nblocks;
    const int per = (e.nblocks + kBlock - 1) / kBlock;
    const int b0 = min(e.nblocks, (int)threadIdx.x * per), b1 = min(e.nblocks, b0 + per);
    double sum = 0;
    for (int b = b0; b < b1; b++) sum += bs[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {  // inclusive Hillis-Steele scan of the chunk sums
        const double v = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0.0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    double run = threadIdx.x ? part[threadIdx.x - 1] : 0.0;
    for (int b = b0; b < b1; b++) {
        const double v = bs[b];
        bs[b] = run;
        run += v;
    }
    if (threadIdx.x == kBlock - 1) e.ltot[ell] = part[kBlock - 1];
}

// the normalized cumulative distribution: X[0] = 0, X[m+1] = (sum of Lv[0..m]) / Ltot
__global__ void __launch_bounds__(kBlock) cellCdfKernel(const EmisArgs e) {
    __shared__ double sc[kBlock];
    const int ell = blockIdx.y, b = blockIdx.x, m = b * kBlock + threadIdx.x;
    const int N = e.ncells;
    sc[threadIdx.x] = m < N ? e.lv[(size_t)ell * N + m] : 0.0;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {  // inclusive Hillis-Steele scan
        const double v = threadIdx.x >= off ? sc[threadIdx.x - off] : 0.0;
        __syncthreads();
        sc[threadIdx.x] += v;
        __syncthreads();
    }
    const double total = e.ltot[ell];
    double* X = e.cdf + (size_t)ell * (N + 1);
    if (m < N) X[m + 1] = total > 0 ? (e.blockSums[(size_t)ell * e.nblocks + b] + sc[threadIdx.x]) / total : 0.0;
    if (m == 0) X[0] = 0.0;
}

// NR::locate_clip over a table in global memory (n entries): the largest j <= n - 2 with v[j] <= q, 0 below v[0]
__device__ __forceinline__ int locateClipTable(const double* v, int n, double q) {
    if (q < v[0]) return 0;
    int jl = -1, ju = n - 1;
    while (ju - jl > 1) {
        const int jm = (ju + jl) >> 1;
        if (q < v[jm]) ju = jm;
        else jl = jm;
    }
    return jl;
}

// A guide table over a CDF of N + 1 entries: G[k] = locate_clip(v, k / N), k = 0 .. N. A draw q then only
// bisects [G[k], G[k + 1]] with k = floor(q N) -- two or three dependent loads instead of log2(N) ~ 20 (the
// dust-phase launch draws a cell from 622,490 per packet in C5).
__global__ void __launch_bounds__(kBlock) cellGuideKernel(const double* cdf, int* guide, int N) {
    const int ell = blockIdx.y, k = blockIdx.x * kBlock + threadIdx.x;
    if (k > N) return;
    const double* v = cdf + (size_t)ell * (N + 1);
    guide[(size_t)ell * (N + 1) + k] = locateClipTable(v, N + 1, (double)k / (double)N);
}

// locate_clip(v, N + 1, q) through the guide table: the bracket [G[k], G[k + 1] + 1) holds the answer when
// v[G[k]] <= q and q < v[G[k + 1] + 1] (or the bracket ends at the table's last index) -- checked, since
// floor(q N) may round across a bucket edge; otherwise the whole table is bisected. Within a valid bracket
// the bisection finds the same largest j with v[j] <= q as the full one.
__device__ __forceinline__ int locateGuided(const double* v, const int* G, int N, double q) {
    const int k = max(0, min(N - 1, static_cast<int>(q * (double)N)));
    const int lo = G[k], hi = G[k + 1] + 1;
    if (!(v[lo] <= q) || (hi < N && !(q < v[hi]))) return locateClipTable(v, N + 1, q);
    int jl = lo, ju = hi;
    while (ju - jl > 1) {
        const int jm = (ju + jl) >> 1;
        if (q < v[jm]) ju = jm;
        else jl = jm;
    }
    return jl;
}

#endif  // SKIRT_AMD_DEVICE_EMISSION_HPP
