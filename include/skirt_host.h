/* skirt_host.h -- C API of the host side: .ski file -> model -> MI355X engine -> SKIRT-format outputs.
 *
 * This is the native replacement of the reference's simulation driver for the photon-shooting phases
 * (Simulation::setupAndRun, SKIRTcore/Simulation.cpp:65-75; MonteCarloSimulation::runstellaremission,
 * MonteCarloSimulation.cpp:251-261; MonteCarloSimulation::write, :553-558). Setup (ski parsing, grid
 * construction, cell density sampling, optical tables, instrument geometry) runs on the host exactly as
 * in the reference; the photon loop runs on the GPU through include/skirt_mcrt.h.
 *
 * Multi-GPU: one process per GPU. Each process loads the same ski, attaches its device, sets the
 * engine's reducer (e.g. an RCCL all-reduce) and runs its shard of every phase
 * (skirt_sim_run_stellar_shard, skirt_sim_run_dust_shard); skirt_sim_fetch then returns the whole
 * simulation's tallies on every rank, and one rank calls skirt_sim_write.
 */
#ifndef SKIRT_HOST_H
#define SKIRT_HOST_H

#include <stdint.h>

#include "skirt_mcrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct SkirtSim SkirtSim;

typedef struct {
    int pan;                    /* PanMonteCarloSimulation (1) or Oligo (0) */
    int ncells, nlambda, ncomp, ninstruments, grid_kind;
    int nnodes;                 /* octree nodes (0 for Cartesian) */
    uint64_t npp;               /* photon packets per wavelength (ceil(packages)) */
    uint64_t total_packets;     /* npp * nlambda for the stellar phase */
    uint64_t seed;
    int store_absorption, has_dust;
    double setup_seconds;
} SkirtSimInfo;

/* Parses the ski file and performs the host setup. packages > 0 overrides the ski's packages,
 * seed != 0 overrides its random seed. datadir NULL = the packaged skirt_amd/data. Returns NULL on
 * failure (skirt_sim_error). */
SkirtSim* skirt_sim_load(const char* ski, const char* datadir, double packages, uint64_t seed);
/* As skirt_sim_load; setup_device >= 0 runs the setup's density sampling (tree subdivision and cell
 * densities, the setup's hot loop) on that HIP device through skirt_mcrt_sample_density. The host still
 * draws the reference's random numbers and takes the subdivision decisions; densities may differ from the
 * host's by an ulp (the device's exp/pow/log10). -1: on the host, bit-identical to the reference. */
SkirtSim* skirt_sim_load_ex(const char* ski, const char* datadir, double packages, uint64_t seed, int setup_device);
/* As skirt_sim_load_ex; input_path is the folder where a relative file name of the model (the particle file of an
 * SPHDustDistribution) is looked up, as the reference's -i option. NULL or "": the .ski file's own folder. With
 * particle dust, setup_device >= 0 also runs the tree subdivision and the tree's cell densities by mass in box on
 * the device (skirt_mcrt_particles_mass_in_box; boxes beyond its merge cap on host worker threads beside it) and the
 * sampled densities of Cartesian, tree and Voronoi grids (skirt_mcrt_particles_sample), all equal to the host's
 * bit for bit. */
SkirtSim* skirt_sim_load_in(const char* ski, const char* datadir, double packages, uint64_t seed, int setup_device,
                            const char* input_path);
int skirt_sim_info(SkirtSim* sim, SkirtSimInfo* info);
/* Imported particle dust (SPHDustDistribution). skirt_sim_particle_info: the number of particles kept, the number
 * ignored for their temperature, whether the distribution offers massInBox to the grids (no negative mass) and the
 * 3 x 21 separators of its cell grid (x, y, z; any pointer may be NULL); SKIRT_ERR_ARG for a model without
 * particle dust. skirt_sim_particle_density: SPHDustDistribution::density at n points (3 doubles each);
 * skirt_sim_particle_mass_in_box: massInBox of n boxes (6 doubles each: min xyz, max xyz), *handed_back (may be
 * NULL) the number of boxes a device left to the host. device < 0: the host's functions; else that HIP device
 * (the particle set is uploaded once per simulation and device). */
int skirt_host_particle_merge_cap(void);  /* the cells of the particle grid a box may span on a device (64) */
int skirt_sim_particle_info(SkirtSim* sim, int* nparticles, int* nignored, int* mass_interface, double* separators);
int skirt_sim_particle_density(SkirtSim* sim, int device, size_t n, const double* points, double* out);
int skirt_sim_particle_mass_in_box(SkirtSim* sim, int device, size_t n, const double* boxes, double* out,
                                   size_t* handed_back);
/* The seed of the photon phases' Philox streams (default: the setup seed). The grid, densities and every
 * other setup draw stay those of the setup seed, so runs that differ only in this seed are independent
 * Monte Carlo realisations on one and the same grid (per-cell statistics against a reference run). */
int skirt_sim_set_photon_seed(SkirtSim* sim, uint64_t seed);
/* creates the engine on HIP device `device` and uploads grid, media, sources and instruments */
int skirt_sim_attach(SkirtSim* sim, int device);
SkirtMcrt* skirt_sim_engine(SkirtSim* sim);
/* stellar emission over global packets [first, first+count) (count 0 = all); asynchronous */
int skirt_sim_run_stellar(SkirtSim* sim, uint64_t first, uint64_t count);
/* PanMonteCarloSimulation::runSelf after the stellar phase (PanMonteCarloSimulation.cpp:96-105): for a
 * Pan dust system with dust emission, the self-absorption cycles (if enabled; host-side grey-body
 * spectra and cell sources between cycles, convergence as the reference) and the dust emission phase,
 * whose detections add to the instrument tallies. Single process; fetches the stellar Labs first.
 * Returns after launching the dust emission phase (asynchronous, like run_stellar). */
int skirt_sim_run_dust(SkirtSim* sim);
/* Multi-GPU: the same phases on rank `rank` of `world` processes (one per GPU). Every phase shoots this
 * rank's slice of EVERY wavelength (skirt_mcrt_run_phase_shard, the reference's IdenticalAssigner), and
 * the engine's reducer (skirt_mcrt_set_reducer, required for world > 1) sums the stellar Labs after the
 * stellar phase, the dust Labs after every self-absorption cycle and the instruments before they are
 * read, so every rank follows the same self-absorption schedule as one process would. */
int skirt_sim_run_stellar_shard(SkirtSim* sim, int rank, int world);
int skirt_sim_run_dust_shard(SkirtSim* sim, int rank, int world);
/* dust Labs of the last self-absorption cycle (row-major cell x wavelength), or NULL; downloads it
 * (waiting for the device) when skirt_sim_fetch has not done so since the last skirt_sim_run_dust */
const double* skirt_sim_labs_dust(SkirtSim* sim);
/* Labsdusttot after every self-absorption cycle; returns the number of cycles */
int skirt_sim_selfabs_totals(SkirtSim* sim, const double** totals);
/* waits and copies the device tallies into the host accumulators */
int skirt_sim_fetch(SkirtSim* sim);
/* host accumulators after skirt_sim_fetch (same layouts as include/skirt_mcrt.h) */
const double* skirt_sim_labs(SkirtSim* sim);
/* the cell densities of the setup, ncells x ncomp row-major (DustSystem::_rhovv); NULL without dust */
const double* skirt_sim_density(SkirtSim* sim);
const double* skirt_sim_instrument(SkirtSim* sim, int i, int* nslots, int* nframe, int* has_frames, int* has_seds);
/* replaces the host accumulators (e.g. after an all-reduce done by the caller) */
int skirt_sim_set_tallies(SkirtSim* sim, const double* labs, const double* instr);
/* writes <prefix>_<instrument>_sed.dat, FITS frames and ds_isrf / ds_cellprops files */
int skirt_sim_write(SkirtSim* sim, const char* prefix);
const char* skirt_sim_error(void);
void skirt_sim_free(SkirtSim* sim);

/* Voronoi dust grids for a binding inside SKIRT. The reference's VoronoiMesh
 * keeps its cells' neighbour lists in an implementation type private to VoronoiMesh.cpp, so a binding
 * hands over the generating sites (VoronoiMesh::particlePosition, in cell order) and the domain, and this
 * host library tessellates them again (the same tessellation, neighbour order and block lists as the .ski
 * driver, pinned to the reference's Voronoi fixtures). skirt_host_voronoi_describe fills the Voronoi fields
 * of a SkirtGridDesc, valid while the SkirtVoronoi lives. */
typedef struct SkirtVoronoi SkirtVoronoi;
SkirtVoronoi* skirt_host_voronoi_build(const double* sites, int nsites, const double extent[6]);
/* As skirt_host_voronoi_build, with the cells computed on HIP device `device` (skirt_mcrt_voronoi_cells) and
 * the ones outgrowing its capacities on the host (*host_cells of them, if host_cells is not NULL); device < 0:
 * every cell on the host. The tessellation is the host build's, bit for bit, either way. */
SkirtVoronoi* skirt_host_voronoi_build_ex(const double* sites, int nsites, const double extent[6], int device,
                                          int* host_cells);
/* copies the cells' volumes (ncells) and centroids (3 per cell); either pointer may be NULL */
int skirt_host_voronoi_cells(const SkirtVoronoi* v, double* volume, double* centroid);
int skirt_host_voronoi_describe(const SkirtVoronoi* v, SkirtGridDesc* grid);
void skirt_host_voronoi_free(SkirtVoronoi* v);

/* The engine's input descriptors without a device (tests of the maintainer binding's extraction,
 * INTEGRATION.md): skirt_sim_describe writes the SkirtGridDesc, SkirtMediaDesc, SkirtSourceDesc and
 * SkirtInstrDesc that skirt_sim_attach would upload for this model to `path` (truncated first);
 * skirt_host_write_descriptors appends the given descriptors in the same canonical form (NULL pointers
 * and ninstr < 0 are skipped): one record per field, "<name> <type> <count>\n" followed by count raw
 * values (type d double, i int32, b int8), array lengths as skirt_mcrt.h states them. */
int skirt_sim_describe(SkirtSim* sim, const char* path);
int skirt_host_write_descriptors(const char* path, const SkirtGridDesc* grid, const SkirtMediaDesc* media,
                                 const SkirtSourceDesc* sources, const SkirtInstrDesc* instr, int ninstr);

/* appends a polarising model's SkirtMuellerDesc in the same form (fields mueller.*), followed by the four 361-entry
 * phi tables of DustMix::setupSelfAfter as the engine builds them; skirt_sim_describe calls it for polarising
 * models only, so the dumps of the others stay as they were */
int skirt_host_write_mueller(const char* path, const SkirtMuellerDesc* mueller);

/* 1 if the simulation's dust mixes polarise (DustSystem::polarization; ElectronDustMix), else 0: its packets then
 * carry Stokes vectors and every FullInstrument has three more slots, Stokes Q, U, V, after its scattering levels
 * (files _stokesQ/U/V.fits, SED columns 8-10) */
int skirt_sim_polarization(SkirtSim* sim);
/* One scattering and one scattering peel-off towards instrument `instrument` of n given packet states
 * (skirt_mcrt_scatterings, which documents the 12 words of a state, the 2 deviates and the 14 words of a result): on
 * the attached engine of HIP device `device` (which must be the device of skirt_sim_attach; another one is
 * SKIRT_ERR_ARG), or with device < 0 by the host's compilation of the same routines (device/polarization.hpp). */
int skirt_sim_scatterings(SkirtSim* sim, int instrument, int device, size_t n, const double* states,
                          const double* deviates, double* out);

/* Random positions of stellar component `comp` (skirt_mcrt_sample_positions): on the attached engine of HIP
 * device `device` (which must be the device of skirt_sim_attach), or with device < 0 on the host, through the
 * host's position templates on the same per-packet streams. pos is n x 3, draws n (or NULL). */
int skirt_sim_sample_positions(SkirtSim* sim, int comp, int device, uint64_t seed, uint64_t first, size_t n,
                               double* pos, int32_t* draws);
/* Launches of stellar component `comp` and its probabilityForDirection (skirt_mcrt_sample_launches, which documents
 * the arguments): on the attached engine of HIP device `device`, or with device < 0 on the host, through the host's
 * compilation of the same routines (device/aniso_emission.hpp; the host's position templates and Random::direction
 * for the isotropic kinds) on the same per-packet streams. */
int skirt_sim_sample_launches(SkirtSim* sim, int comp, int device, uint64_t seed, uint64_t first, size_t n, double* pos,
                              double* dir, int32_t* draws, size_t nprob, const double* prob_pos, const double* prob_dir,
                              double* prob);

/* The cross-GPU sums in C++: RCCL (NCCL API) all-reduces over xGMI, the MI355X counterpart of the
 * reference's MPI_Allreduce of the absorption tables and instrument arrays (PanDustSystem.cpp:394-404,
 * Instrument.cpp:57-66, MPIsupport/ProcessManager.cpp:133-137).
 * skirt_rccl_create makes one communicator per device of this process (ncclCommInitAll over `devices`);
 * skirt_rccl_reducer is the engine's reducer callback (skirt_mcrt_set_reducer) and skirt_rccl_rank(r, rank)
 * its user pointer for the engine of rank `rank`: the callback sums the tally in place, ncclSum of doubles,
 * on the stream the engine hands it. Each rank's engine must then be driven by its own host thread (the
 * collectives of the ranks meet on the devices). A process that runs one rank of a multi-process job
 * creates its communicator through its own bootstrap (e.g. ncclCommInitRank, or torch.distributed) and can
 * use the same callback through skirt_rccl_wrap. */
typedef struct SkirtRccl SkirtRccl;
int skirt_rccl_create(int ndev, const int* devices, SkirtRccl** out);
/* wraps an existing communicator (an ncclComm_t) of one rank: ndev = 1, rank 0 */
int skirt_rccl_wrap(void* nccl_comm, SkirtRccl** out);
void* skirt_rccl_rank(SkirtRccl* r, int rank);
SkirtReduceTallyFn skirt_rccl_reducer(void);
/* The reference's Parallel::call stops every worker at the first exception and rethrows it in the parent
 * (SKIRTcore/Parallel.cpp:181-193). Across devices: skirt_rccl_abort marks the job failed (`why` is kept as the
 * first failure's message), after which no rank of `r` enqueues another all-reduce (the reducer returns
 * non-zero, also to ranks waiting for the others before one), and aborts owned communicators
 * (ncclCommAbort), which returns ranks already waiting in an all-reduce on the device. Idempotent.
 * The reducer of several ranks in one process waits, before each all-reduce, until every rank has arrived
 * or one has failed, so a rank that fails between two collectives leaves none of its peers waiting. */
int skirt_rccl_abort(SkirtRccl* r, const char* why);
void skirt_rccl_destroy(SkirtRccl* r);
/* The driver of `skirt-mi355x -g N`: loads the ski once per device, runs every phase of the simulation
 * with each device shooting its rank's slice of every wavelength (one host thread per device) and the
 * tallies summed by skirt_rccl at each phase end, then writes the outputs from rank 0. The first device
 * thread that fails stops the others (skirt_rccl_abort) and its error is returned; SKIRT_AMD_FAIL_DEVICE=d
 * makes device d's thread fail before its first phase (tests). packages > 0 and
 * seed != 0 override the ski's. stats (may be NULL) receives rank 0's statistics; seconds (may be NULL)
 * the wall time of the photon phases. */
int skirt_sim_run_devices(const char* ski, const char* datadir, int ndev, double packages, uint64_t seed,
                          const char* outprefix, SkirtStats* stats, double* seconds);

#ifdef __cplusplus
}
#endif
#endif
