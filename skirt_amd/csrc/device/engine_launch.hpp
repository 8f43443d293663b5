// The launch seam between the engine's kernels (device/engine.hip, which defines these functions) and its host side
// (host/engine_*.cpp, which calls them): runtime API types only, so the host compiler can include it.
//
// The templated kernels take one Args (columnKernel: Args, rays, n, out). The *KernelOf functions turn the runtime
// choices into the kernel's address, for hipLaunchKernel, hipFuncSetAttribute and the occupancy query alike; every
// launch is of kBlock threads. The one-off kernels have a typed launch function each. None of them is part of the
// library's ABI.
#ifndef SKIRT_AMD_DEVICE_ENGINE_LAUNCH_HPP
#define SKIRT_AMD_DEVICE_ENGINE_LAUNCH_HPP

#include <hip/hip_runtime_api.h>

#include "engine_args.hpp"

namespace skirt_dev {

// kind: a walk kind of kWalks (any other: the node-array walk)
SKIRT_HIDDEN const void* traceKernelOf(int kind, bool one, bool continuous, bool global, bool noStore);
SKIRT_HIDDEN const void* eventKernelOf(int kind, bool one, bool pol, bool aniso);
SKIRT_HIDDEN const void* contKernelOf(int kind, bool one);
SKIRT_HIDDEN const void* detectKernelOf(bool pol);
SKIRT_HIDDEN const void* columnKernelOf(int kind);

SKIRT_HIDDEN void launchBuildLeafMap(dim3 grid, hipStream_t st, LeafEntry* map, const int* firstChild,
                                     const signed char* splitDir, const int* cellnumber, const double* rho, int ncomp, int L);
SKIRT_HIDDEN void launchLabsFold(dim3 grid, hipStream_t st, double* dst, double* rep, size_t n, int copies,
                                 size_t strideElems);
SKIRT_HIDDEN void launchCellSpectra(dim3 grid, hipStream_t st, const EmisArgs& e);
SKIRT_HIDDEN void launchCellBlockSum(dim3 grid, hipStream_t st, const EmisArgs& e);
SKIRT_HIDDEN void launchCellScanBlocks(dim3 grid, hipStream_t st, const EmisArgs& e);
SKIRT_HIDDEN void launchCellCdf(dim3 grid, hipStream_t st, const EmisArgs& e);
SKIRT_HIDDEN void launchCellGuide(dim3 grid, hipStream_t st, const double* cdf, int* guide, int N);
SKIRT_HIDDEN void launchSamplePositions(dim3 grid, hipStream_t st, const double* geomParam, const double* geomTable, int h,
                                        unsigned long long seed, unsigned long long first, size_t n, double* pos, int* draws,
                                        unsigned* error);
SKIRT_HIDDEN void launchSampleLaunches(dim3 grid, hipStream_t st, const double* geomParam, const double* geomTable, int nstar,
                                       int h, unsigned long long seed, unsigned long long first, size_t n, double* pos,
                                       double* dir, int* draws, size_t nprob, const double* ppos, const double* pdir,
                                       double* prob, unsigned* error);
SKIRT_HIDDEN void launchScatterings(dim3 grid, hipStream_t st, const double* tab, int ncomp, int nlambda, int nt,
                                    const double* states, const double* deviates, double kox, double koy, double koz,
                                    double kyx, double kyy, double kyz, size_t n, double* out);
SKIRT_HIDDEN void launchDensitySample(dim3 grid, hipStream_t st, const DensArgs& d);
// (blocks of kBlock threads; the mass kernel's are of partMassBlock)
SKIRT_HIDDEN void launchParticleSample(dim3 grid, hipStream_t st, const PartArgs& a);
SKIRT_HIDDEN void launchParticleMass(dim3 grid, hipStream_t st, const PartArgs& a, unsigned* handedBack);

}  // namespace skirt_dev

#endif
