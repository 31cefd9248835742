/*! @file sphexa_hip.h
 * @brief C-ABI of libsphexa_hip.so -- the MI355X (gfx950) hot path of SPH-EXA's VE propagator.
 *
 * Plain C, POD structs and raw device pointers only.  Each entry point replaces one GPU seam of the
 * reference (paths relative to the SPH-EXA tree, lks1248/SPH-EXA @ 2024-10-16):
 *
 *   sx_sfc_keys            cstone::computeSfcKeysGpu            domain/include/cstone/sfc/sfc_gpu.h, sfc_gpu.cu:47
 *   sx_sort_keys           cstone::GpuSfcSorter::setMapFromCodes domain/include/cstone/primitives/primitives_gpu.cu:271-283
 *   sx_gather              cstone::gatherGpu                    primitives/primitives_gpu.cu:86
 *   sx_compute_octree      cstone::computeOctreeGpu / updateOctreeGpu (converged)  tree/csarray_gpu.cu:100-264
 *   sx_build_octree        cstone::buildOctreeGpu               tree/octree_gpu.cu:153-170
 *   sx_node_centers        cstone::computeGeoCentersGpu         focus/source_center_gpu.cu:117-135
 *   sx_compute_groups      cstone::computeFixedGroups (64)      domain/include/cstone/traversal/groups.cuh:13-41
 *   sx_spatial_groups      sph::computeSpatialGroups            sph/include/sph/groups.cu:30-47 (computeGroupSplits<64>,
 *                                                               traversal/groups.cuh:195-310)
 *   sx_find_neighbors      cstone::findNeighbors (+ sph h-nc iteration) findneighbors.hpp:167-188,
 *                                                               sph/include/sph/find_neighbors.hpp:10-44
 *   sx_xmass               sph::cuda::computeXMass              sph/include/sph/sph_gpu.hpp:25, hydro_ve/xmass_gpu.cu:103
 *   sx_ve_def_gradh        sph::cuda::computeVeDefGradh         sph_gpu.hpp:37, hydro_ve/ve_def_gradh_gpu.cu:86
 *   sx_eos                 sph::cuda::computeEOS (VE)           sph_gpu.hpp:40-43, hydro_ve/eos_gpu.cu:74
 *   sx_iad_divv_curlv      sph::cuda::computeIadDivvCurlv       sph_gpu.hpp:45, hydro_ve/iad_divv_curlv_gpu.cu:91
 *   sx_av_switches         sph::cuda::computeAVswitches         sph_gpu.hpp:48, hydro_ve/av_switches_gpu.cu:103
 *   sx_momentum_energy     sph::cuda::computeMomentumEnergy<avClean=false> sph_gpu.hpp:51-53, momentum_energy_gpu.cu:121
 *   sx_momentum_energy_avclean  sph::cuda::computeMomentumEnergy<avClean=true>  (same seam, second instantiation)
 *   sx_density             sph::cuda::computeDensity (std)      sph_gpu.hpp:32, hydro_ve/xmass_gpu.cu:150-164
 *   sx_eos_std             sph::cuda::computeEOS_HydroStd       sph_gpu.hpp:46-47, hydro_std/eos_gpu.cu:54-62
 *   sx_iad                 sph::computeIADGpu (std)             sph_gpu.hpp:19-20, hydro_std/iad_gpu.cu:111-124
 *   sx_momentum_energy_std sph::computeMomentumEnergyStdGpu     sph_gpu.hpp:22-23, hydro_std/momentum_energy_gpu.cu:109
 *   sx_positions           sph::computePositionsGpu             sph_gpu.hpp:64-72, positions_gpu.cu:167-179
 *   sx_mark_ramp           sph::cuda::computeMarkRamp           sph_gpu.hpp:54, hydro_ve/additional_fields.cu:86-98
 *   sx_positions_rungs     sph::computePositionsGpu (rungs)     sph_gpu.hpp:64-72, positions_gpu.cu:110-179
 *   sx_drift_positions     sph::driftPositionsGpu               sph_gpu.hpp:57-62, positions_gpu.cu:45-108
 *   sx_group_divv_timestep sph::groupDivvTimestepGpu            sph_gpu.hpp:80, ts_groups.cu:17-46
 *   sx_group_acc_timestep  sph::groupAccTimestepGpu             sph_gpu.hpp:83, ts_groups.cu:48-81
 *   sx_store_rung          sph::storeRungGpu                    sph_gpu.hpp:86, ts_groups.cu:84-108
 *   sx_rung_timestep       sph::rungTimestep                    sph/include/sph/ts_rungs.hpp:132-145 (sortGroupDt :67-78,
 *                                                               computeMinTimestep :89-105, findRungRanges :116-130)
 *   sx_minimum_group_dt    sph::minimumGroupDt                  ts_rungs.hpp:147-157
 *   sx_extract_groups      sph::extractGroupGpu                 sph/include/sph/groups.hpp:31-48
 *   sx_update_h            sph::updateSmoothingLengthGpu        sph_gpu.hpp:78, update_h_gpu.cu:49-60
 *   sx_max_divv            cstone::MinMaxGpu (rhoTimestep)      sph/ts_global.hpp:72-94
 *   sx_turb_*              sph::TurbulenceData, updateNoise, computePhases  sph/include/sph/hydro_turb/turbulence_data.hpp:46-184,
 *                                                               driver.hpp:80-92, phases.hpp:47-72, create_modes.hpp:59-244
 *   sx_stir                sph::computeStirringGpu              hydro_turb/stirring.hpp:123-126 (stirParticle :44-79)
 *   sx_gravity_direct      ryoanji::directSum                   ryoanji/interface/multipole_holder.cuh:72-74, nbody/direct.cuh:52-123
 *                                                               (CPU form: nbody/traversal_cpu.hpp:234-270)
 *   sx_sim_set_turbulence  TurbVeProp::computeForces            main/src/propagator/turb_ve.hpp:114-119
 *   sx_cool, sx_sim_set_cooling  the energy sink of HydroGrackleProp, main/src/propagator/std_hydro_grackle.hpp:155-226, as an
 *                                                               exact integration of a tabulated cooling function on the device
 *   sx_observables         sphexa::gpuGrowthRate, machSquareSumGpu, survivorsGpu  main/src/observables/gpu_reductions.cu:69-168;
 *                                                               d2QuadpoleMomentum grav_waves_calculations.hpp:87-121
 *   sx_sim_observe         IObservables::computeAndWrite        main/src/observables/factory.hpp:46-69
 *   sx_nbody_positions     computePositions without temp / u    main/src/propagator/nbody.hpp:161, sph/positions.hpp:77-110
 *   sx_sim_* (propagator 3) one NbodyProp step (computeForces + integrate), main/src/propagator/nbody.hpp:115-163
 *   sx_sim_*               one HydroVeProp step (sync + computeForces + integrate), main/src/propagator/ve_hydro.hpp:132-218
 *
 * Conventions (reference semantics preserved):
 *  - Field types follow sph::SphTypes (sph/types.hpp:39-46): x,y,z,temp,u,du double; other hydro fields float.
 *  - Neighbor criterion is the reference CPU one (cstone/findneighbors.hpp:111,133-158):
 *    |r_ij|^2 (double) < float(4 h_i^2), j != i, periodic folding when the particle is within 2h of the box edge.
 *  - nc[i] counts neighbors INCLUDING self (sph/find_neighbors.hpp:26); kernels use min(nc-1, ngmax) of them.
 *  - sx_xmass runs the neighbor search with the coupled h-nc iteration (mutates h, writes nc), exactly like
 *    sph::cuda::computeXMass.  The neighbor list it builds is cached in the context and reused by the later pair
 *    kernels of the same step (the reference GPU re-traverses the tree in each kernel; positions and h do not change
 *    between computeXMass and computeMomentumEnergy in ve_hydro.hpp:132-205).  Call sx_find_neighbors again if x,y,z
 *    or h change.
 *  - Every call is asynchronous on the context stream unless it returns a host scalar (sx_momentum_energy,
 *    sx_max_divv, sx_compute_octree), which synchronises that stream -- like the reference, whose entry points
 *    synchronise (e.g. xmass_gpu.cu:113).
 *  - Return value: SX_OK, or an SX_ERR_* code; sx_last_error() has the message.  The reference turns the same
 *    conditions into std::runtime_error (xmass_gpu.cu:126-127) or exit() (cuda/errorcheck.cuh:30-42).
 */
#ifndef SPHEXA_HIP_H
#define SPHEXA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SX_OK 0
#define SX_ERR_TRAVERSAL 1   /* neighbor-search candidate buffer exhausted ("GPU traversal stack exhausted") */
#define SX_ERR_NOT_CONVERGED 2 /* coupled h-nc iteration failed to converge (xmass_gpu.cu:127) */
#define SX_ERR_HIP 3         /* HIP runtime error */
#define SX_ERR_ARG 4         /* invalid argument (sizes, missing buffers, no neighbor list) */
#define SX_ERR_NOMEM 5

/*! cstone::Box<double> (sfc/box.hpp:111-191). bnd[k]: 0 open, 1 periodic, 2 fixed (cstone::BoundaryType). */
typedef struct sx_box
{
    double  lim[6]; /* xmin xmax ymin ymax zmin zmax */
    int32_t bnd[3];
} sx_box;

/*! ParticlesData physics members (sph/particles_data.hpp:86-138) used by the VE kernels. */
typedef struct sx_params
{
    double   K;        /* kernel normalisation; sx_kernel_constant() returns the reference value */
    uint32_t ng0;      /* target neighbor count, 100 */
    uint32_t ngmax;    /* max stored neighbors, 150 */
    double   Kcour;    /* 0.2 */
    double   Krho;     /* 0.06 */
    double   gamma;    /* 5/3 */
    float    muiConst; /* 10 */
    float    alphamin, alphamax, decay_constant; /* 0.05, 1.0, 0.2 */
    float    Atmin, Atmax, ramp;                 /* 0.1, 0.2, 10 */
    double   maxDtIncrease;                      /* 1.1 */
    int32_t  avClean; /* sx_sim only: HydroVeProp<avClean=true> (ve_hydro.hpp:50, factory.hpp:56), 0 = off */
    float    theta;   /* gravity opening parameter (sphexa.cpp:127: 0.5 with gravity) */
    double   g;       /* gravitational constant (ParticlesData::g); sx_sim adds self-gravity when != 0 */
    double   eps, etaAcc; /* accelerationTimestep (ts_global.hpp:47-67): 0.005, 0.2 */
    int32_t  propagator;  /* sx_sim only: 0 = ve (HydroVeProp), 1 = std (HydroProp, std_hydro.hpp), 2 = ve-bdt
                             (HydroVeBdtProp, ve_hydro_bdt.hpp: block time-steps, one substep per sx_sim_step),
                             3 = nbody (NbodyProp, nbody.hpp: gravity only, needs g != 0; no thermal or hydro field is
                             allocated); factory.hpp:50-84 */
} sx_params;

/*! Device pointers in sphexa::ParticlesData field order (particles_data.hpp:247-251); NULL where unused.
 *  n = number of particles INCLUDING halos (every array has this length). */
typedef struct sx_fields
{
    size_t    n;
    double *  x, *y, *z;
    float *   x_m1, *y_m1, *z_m1;
    float *   vx, *vy, *vz;
    float*    rho;
    double*   u;
    float *   p, *prho, *tdpdTrho, *h, *m, *c;
    float *   ax, *ay, *az;
    double*   du;
    float*    du_m1;
    float *   c11, *c12, *c13, *c22, *c23, *c33;
    float *   mue, *mui;
    double*   temp;
    float *   cv, *xm, *kx, *divv, *curlv, *alpha, *gradh;
    uint64_t* keys;
    uint32_t* nc;
    float *   dV11, *dV12, *dV13, *dV22, *dV23, *dV33;
    float*    markRamp;
    uint8_t*  rung;
} sx_fields;

/*! cstone::OctreeNsView<double, uint64_t> (tree/octree.hpp:296-316), device pointers. centers/sizes are
 *  Vec3<double> arrays (3 doubles per node). */
typedef struct sx_tree
{
    int32_t         numLeafNodes;
    int32_t         numNodes;
    const uint64_t* prefixes;
    const int32_t*  childOffsets;
    const int32_t*  internalToLeaf;
    const int32_t*  levelRange;
    const uint64_t* leaves;
    const uint32_t* layout; /* leaf -> first particle; numLeafNodes + 1 entries */
    const double*   centers;
    const double*   sizes;
    float           searchExtFactor;
} sx_tree;

/*! sph::GroupView (cstone/traversal/groups.hpp:19-55). The MI355X path partitions [firstBody, lastBody) into
 *  fixed 64-particle SFC blocks (one wavefront each); groupStart/groupEnd are accepted for interface parity. */
typedef struct sx_groups
{
    uint32_t        firstBody, lastBody, numGroups;
    const uint32_t* groupStart;
    const uint32_t* groupEnd;
} sx_groups;

/*! Linked octree arrays (cstone::OctreeData, tree/octree.hpp:318-375), device pointers, caller-owned.
 *  Sizes: numNodes = numLeaves + (numLeaves-1)/7; childOffsets numNodes+1; parents max(1,(numNodes-1)/8);
 *  levelRange 23; internalToLeaf, leafToInternal numNodes. */
typedef struct sx_octree
{
    uint64_t* prefixes;
    int32_t*  childOffsets;
    int32_t*  parents;
    int32_t*  levelRange;
    int32_t*  internalToLeaf;
    int32_t*  leafToInternal;
} sx_octree;

/*! neighbor-search statistics (cstone::NcStats, traversal/find_neighbors.cuh:346-357) */
typedef struct sx_nbstats
{
    uint64_t sumNeighbors;   /* sum over targets of stored neighbors */
    uint32_t maxNeighbors;   /* max true count (excluding self) */
    uint32_t numFailed;      /* h-nc iteration failures */
    uint64_t sumCandidates;  /* candidate particles tested (per target, summed) */
    uint64_t sumUnion;       /* cluster neighbor-union entries, summed over 256-particle clusters */
    uint32_t build;          /* search build used: 0 compact, 1 large, 2 compact overflowed and redone by the large */
    uint32_t maxUnion;       /* largest cluster neighbor union (local lists; 0 otherwise) */
} sx_nbstats;

typedef struct sx_ctx sx_ctx;

/* ---- context --------------------------------------------------------------------------------------------- */
int         sx_create(sx_ctx** ctx, int device);
void        sx_destroy(sx_ctx* ctx);
int         sx_set_stream(sx_ctx* ctx, void* hipStream); /* NULL = the context's own stream */
void*       sx_get_stream(sx_ctx* ctx);
const char* sx_last_error(sx_ctx* ctx); /* ctx NULL: the calling thread's last refused host-only call (sx_map_check) */
/*! 1: bit-reproducible arithmetic (no FMA contraction; matches the CPU reference bit-for-bit given the same neighbor
 *  order); 0 (default): FMA-contracted kernels. */
int    sx_set_exact(sx_ctx* ctx, int exact);
double sx_kernel_constant(void); /* K of the sinc^6 kernel, particles_data.hpp:366 */
/*! host evaluation of the register-resident kernel W(v), dW/dv of the fast pair kernels (sx_kernel_poly.hpp), for
 *  checking it against the reference tables */
int    sx_kernel_poly(const float* v, size_t n, float* w, float* dw);
/*! packed12 cluster neighbor lists (sx_pack12.hpp): 12-bit union positions, eight per three words.  A cluster's lists
 *  are packed12 when its union holds at most maxUnion entries, else u16 pairs.  Default: 4095, the largest value; 0
 *  (every list u16) for a context with sx_set_exact(1), whose gather kernels decode one entry at a time.  Tests set it
 *  to reach both formats with either variant (0xffffffff: back to the default).  It takes effect with the context's next search; an sx_sim reads it when
 *  it is created. */
int      sx_set_pack12_max(sx_ctx* ctx, uint32_t maxUnion);
/*! host side of the format, for checking it: words per target of a row with up to ngmax entries; the cnt positions
 *  pos[] (each < 4096) packed into 3 * ceil(cnt / 8) words (the last group's tail repeats the last position); the
 *  first n entries of such a list */
uint32_t sx_pack12_row_words(uint32_t ngmax);
int      sx_pack12_pack(const uint32_t* pos, uint32_t cnt, uint32_t* words);
int      sx_pack12_unpack(const uint32_t* words, uint32_t n, uint32_t* pos);
int    sx_copy_tables(sx_ctx* ctx, float* wh_host, float* whd_host); /* 20000-entry f32 tables */
int    sx_synchronize(sx_ctx* ctx);

/* ---- device memory plumbing (for hosts without their own allocator, e.g. ctypes bindings) --------------- */
void* sx_device_alloc(sx_ctx* ctx, size_t bytes);
int   sx_device_free(sx_ctx* ctx, void* ptr);
/*! kind: 1 host->device, 2 device->host, 3 device->device; synchronous w.r.t. the context stream */
int   sx_memcpy(sx_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
int   sx_memset(sx_ctx* ctx, void* dst, int value, size_t bytes);

/* ---- cstone: SFC keys, sorting, tree -------------------------------------------------------------------- */
int sx_sfc_keys(sx_ctx* ctx, const double* x, const double* y, const double* z, uint64_t* keys, size_t n,
                const sx_box* box);
/*! sort keys ascending in place (stable) and write the permutation: order[i] = old index of sorted element i */
int sx_sort_keys(sx_ctx* ctx, uint64_t* keys, uint32_t* order, size_t n);
/*! dst[i] = src[order[i]] for elements of elemBytes (1,2,4,8,16) */
int sx_gather(sx_ctx* ctx, const uint32_t* order, size_t n, const void* src, void* dst, int elemBytes);
/*! fully converged cornerstone leaves of sorted keys (the unique tree of csarray.hpp:456-467).
 *  leaves: capacity+1 entries, counts: capacity. *numLeaves receives the count; SX_ERR_ARG if capacity is short. */
int sx_compute_octree(sx_ctx* ctx, const uint64_t* sortedKeys, size_t n, uint32_t bucketSize, uint64_t* leaves,
                      uint32_t* counts, int32_t capacity, int32_t* numLeaves);
int sx_build_octree(sx_ctx* ctx, const uint64_t* leaves, int32_t numLeaves, const sx_octree* out);
int sx_node_centers(sx_ctx* ctx, const uint64_t* prefixes, int32_t numNodes, const sx_box* box, double* centers,
                    double* sizes);
/*! layout[i] = exclusive prefix sum of counts (layout has numLeaves+1 entries) */
int sx_leaf_layout(sx_ctx* ctx, const uint32_t* counts, int32_t numLeaves, uint32_t* layout);

/* ---- sph ------------------------------------------------------------------------------------------------- */
/*! fixed groups of 64 SFC-consecutive targets (one wavefront each); groupStart/groupEnd = NULL (implicit) */
int sx_compute_groups(sx_ctx* ctx, uint32_t first, uint32_t last, sx_groups* groups);
/*! computeSpatialGroups: the fixed 64-groups split where consecutive particles are farther apart than
 *  tolFactor * cbrt(smallest leaf volume of the group) in box-scaled coordinates (the reference passes
 *  tolFactor = 2).  Writes groups[0..numGroups] (device array of capacity cap >= last - first + 1) and sets
 *  out->groupStart = groups, out->groupEnd = groups + 1. */
int sx_spatial_groups(sx_ctx* ctx, uint32_t first, uint32_t last, const double* x, const double* y, const double* z,
                      const sx_tree* tree, const sx_box* box, float tolFactor, uint32_t* groups, uint32_t cap,
                      sx_groups* out);
/*! neighbor search for targets [first,last) into the context's list; iterate_h != 0 runs the h-nc iteration
 *  (mutates h). nc has length fields->n (written at [first,last)). stats may be NULL. */
/*! which neighbor-search build sx_find_neighbors runs: 0 automatic (the compact build, four workgroups per CU,
 *  with a device-side fallback to the large build on a capacity overflow; the large one after an overflow or at
 *  > 105 neighbors per target), 1 large only, 2 compact first, 3 compact with a forced overflow of every cluster
 *  (test hook for the fallback).  All give identical h, nc and neighbor lists. */
int sx_set_search_mode(sx_ctx* ctx, int mode);
int sx_find_neighbors(sx_ctx* ctx, const sx_fields* f, const sx_tree* tree, const sx_box* box,
                      const sx_params* p, uint32_t first, uint32_t last, int iterate_h, sx_nbstats* stats);
/*! copy the cached list out / in, CPU layout neighbors[(i-first)*ngmax + k] (device pointers); export zero-fills
 *  slots k >= min(nc[i]-1, ngmax) */
int sx_export_neighbors(sx_ctx* ctx, const uint32_t* nc, uint32_t first, uint32_t last, uint32_t ngmax,
                        uint32_t* neighbors);
int sx_import_neighbors(sx_ctx* ctx, uint32_t first, uint32_t last, uint32_t ngmax, const uint32_t* neighbors);

int sx_xmass(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p, const sx_box* box,
             const sx_tree* tree);
/*! xmass on the cached (or imported) neighbor list, without a new search */
int sx_xmass_only(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p, const sx_box* box);
int sx_ve_def_gradh(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p, const sx_box* box);
int sx_eos(sx_ctx* ctx, uint32_t first, uint32_t last, float mui, double gamma, const double* temp, const float* m,
           const float* kx, const float* xm, const float* gradh, float* prho, float* c, float* rho, float* p);
/*! also writes the velocity gradient dV11..dV33 when f->dV11 != NULL (doGradV: dV11.size() == x.size(),
 *  iad_divv_curlv_gpu.cu:96-97, divv_curlv_kern.hpp:113-121) */
int sx_iad_divv_curlv(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p, const sx_box* box);
int sx_av_switches(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p, const sx_box* box,
                   double minDt);
/*! writes ax,ay,az,du; *minDtCourant receives the min Courant time-step (float, like minDt_ve_device) */
int sx_momentum_energy(sx_ctx* ctx, const sx_groups* g, float* groupDt, const sx_fields* f, const sx_params* p,
                       const sx_box* box, float* minDtCourant);
/*! computeMomentumEnergy<avClean=true> (sph_gpu.hpp:51-53, momentum_energy_gpu.cu:147-152): adds the
 *  avRvCorrection of the AV-cleaning propagator (momentum_energy_kern.hpp:43-63); needs f->dV11..dV33 */
int sx_momentum_energy_avclean(sx_ctx* ctx, const sx_groups* g, float* groupDt, const sx_fields* f,
                               const sx_params* p, const sx_box* box, float* minDtCourant);
/* ---- std propagator (HydroProp, main/src/propagator/std_hydro.hpp:124-184) ----------------------------- */
/*! sph::cuda::computeDensity (sph_gpu.hpp:32, hydro_ve/xmass_gpu.cu:150-164): neighbor search with the h-nc
 *  iteration (like sx_xmass), the XMass loop written to rho, then rho = m / rho.  Needs f->rho. */
int sx_density(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p, const sx_box* box,
               const sx_tree* tree);
/*! density on the cached (or imported) neighbor list, without a new search */
int sx_density_only(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p, const sx_box* box);
/*! sph::cuda::computeEOS_HydroStd (sph_gpu.hpp:46-47, hydro_std/eos_gpu.cu:54-62): p, c from temp and rho */
int sx_eos_std(sx_ctx* ctx, uint32_t first, uint32_t last, float mui, double gamma, const double* temp,
               const float* m, float* rho, float* p, float* c);
/*! sph::computeIADGpu (sph_gpu.hpp:19-20, hydro_std/iad_gpu.cu:111-124): c11..c33 with volumes m/rho */
int sx_iad(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p, const sx_box* box);
/*! sph::computeMomentumEnergyStdGpu (sph_gpu.hpp:22-23, hydro_std/momentum_energy_gpu.cu:109-129): ax,ay,az,du
 *  (alpha = 1, gradh = 1); *minDtCourant receives the min Courant time-step */
int sx_momentum_energy_std(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p,
                           const sx_box* box, float* minDtCourant);

/*! 2nd-order Press position update + AB2 energy update on temp (positions.hpp:54-139, F2-correct); dt, dt_m1 double
 *  as in the CPU path (the reference GPU path passes them as float). */
int sx_positions(sx_ctx* ctx, uint32_t first, uint32_t last, double dt, double dt_m1, const sx_fields* f,
                 double gamma, float muiConst, const sx_box* box);
/*! the position update of the gravity-only propagator (NbodyProp::integrate, nbody.hpp:161: computePositions with
 *  neither temp nor u): the Press update of x, v and x_m1 over [first, last) from f->ax, ay, az, the fixed-boundary skip
 *  (f->h is read only in a box with a fixed axis) and putInBox.  keys (nullable, indexed like the fields): the SFC
 *  keys of the updated coordinates in box.  No thermal field of f is read or written. */
int sx_nbody_positions(sx_ctx* ctx, uint32_t first, uint32_t last, double dt, double dt_m1, const sx_fields* f,
                       const sx_box* box, uint64_t* keys);
int sx_update_h(sx_ctx* ctx, uint32_t first, uint32_t last, uint32_t ng0, const uint32_t* nc, float* h);
/*! updateSmoothingLengthGpu over the targets of a group view (update_h_gpu.cu:49-60; ve_hydro_bdt.hpp:369 passes the
 *  active rungs): explicit groups, or fixed 64-blocks of [firstBody, lastBody) when groupStart is NULL */
int sx_update_h_groups(sx_ctx* ctx, const sx_groups* g, uint32_t ng0, const uint32_t* nc, float* h);

/*! computeMarkRamp (sph_gpu.hpp:54, hydro_ve/additional_fields.cu:47-98): per target the mean over its neighbors of
 *  1 (Atwood > Atmax) or ramp*(Atwood - Atmin) (Atmin <= Atwood <= Atmax), rho = kx m / xm; uses the cached list */
int sx_mark_ramp(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_params* p, const sx_box* box,
                 float* markRamp);

/* ---- block time-steps (HydroVeBdtProp, main/src/propagator/ve_hydro_bdt.hpp) ------------------------------------
 * Groups: explicit [groupStart[g], groupEnd[g]) (sx_spatial_groups, or a slice of a rung-sorted group list) or, with
 * groupStart == NULL, fixed 64-particle blocks of [firstBody, lastBody).  dt_m1[SX_MAX_RUNGS] holds the previous
 * time-step of each rung; rung (nullable) selects dt_m1[rung[i]], else dt_m1[0].  constCv < 0: cv from f->mui
 * (idealGasCv per particle).  f->temp NULL: the update acts on f->u instead. */
#define SX_MAX_RUNGS 4 /* sph::Timestep::maxNumRungs (sph/timestep.h:42) */
/*! computePositionsGpu (sph_gpu.hpp:64-72, positions_gpu.cu:110-179): Press position update + AB2 energy */
int sx_positions_rungs(sx_ctx* ctx, const sx_groups* g, float dt, const float* dt_m1, const uint8_t* rung,
                       const sx_fields* f, double gamma, double constCv, const sx_box* box);
/*! driftPositionsGpu (sph_gpu.hpp:57-62, positions_gpu.cu:45-108): back by dt_back, forward by dt, open box */
int sx_drift_positions(sx_ctx* ctx, const sx_groups* g, float dt, float dt_back, const float* dt_m1,
                       const uint8_t* rung, const sx_fields* f, double gamma, double constCv);
/*! groupDivvTimestepGpu (ts_groups.cu:17-46): groupDt[g] = min(groupDt[g], Krho / |max divv over g|) */
int sx_group_divv_timestep(sx_ctx* ctx, float Krho, const sx_groups* g, const float* divv, float* groupDt);
/*! groupAccTimestepGpu (ts_groups.cu:48-81): groupDt[g] = min(groupDt[g], etaAcc / |a|max^(1/2)) */
int sx_group_acc_timestep(sx_ctx* ctx, float etaAcc, const sx_groups* g, const float* ax, const float* ay,
                          const float* az, float* groupDt);
/*! storeRungGpu (ts_groups.cu:84-108) */
int sx_store_rung(sx_ctx* ctx, const sx_groups* g, uint8_t rung, uint8_t* rungs);
int sx_max_divv(sx_ctx* ctx, uint32_t first, uint32_t last, const float* divv, float* maxDivv);

/* ---- observables ---------------------------------------------------------------------------------------- */
/*! conservedQuantitiesGpu (main/src/observables/conserved_gpu.cu:71-94) and the nc sum of
 *  computeConservedQuantities (conserved_quantities.hpp:118-131) over [first, last) of f, in double:
 *  out = {0.5 sum m v^2, internal energy, linear momentum x y z, angular momentum x y z, sum nc}.  Internal energy
 *  is sum u m when f->u is set, else sum cv T m with cv = idealGasCv(muiConst, gamma).  Synchronises. */
int sx_conserved_quantities(sx_ctx* ctx, const sx_fields* f, uint32_t first, uint32_t last, float muiConst,
                            double gamma, double out[9]);

/*! the observables of observablesFactory (main/src/observables/factory.hpp:46-69) */
#define SX_OBS_TIME_ENERGY 0 /* TimeAndEnergy, time_energies.hpp */
#define SX_OBS_MACH_RMS 1    /* TurbulenceMachRMS, turbulence_mach_rms.hpp */
#define SX_OBS_KH_GROWTH 2   /* TimeEnergyGrowth, time_energy_growth.hpp */
#define SX_OBS_WIND_BUBBLE 3 /* WindBubble, wind_bubble_fraction.hpp */
#define SX_OBS_GRAV_WAVES 4  /* GravWaves, gravitational_waves.hpp */
#define SX_OBS_MAX_SUMS 15   /* the nine conserved sums + at most six of the kind */
#define SX_OBS_MAX_COLUMNS 16 /* longest row of sx_sim_observe */
/*! what the observables read besides the fields (the constructor arguments of factory.hpp:48-66) */
typedef struct sx_obs_settings
{
    double rhoBubble;     /* wind bubble: initial density inside the cloud (rhoInt) */
    double tempWind;      /* wind bubble: temperature of the wind, uExt * idealGasCv(muiConst, gamma) */
    double initialMass;   /* wind bubble: initial mass of the cloud, 4/3 pi rSphere^3 rhoInt */
    double particleMass;  /* wind bubble: the reference's m[0] (equal masses, wind_bubble_fraction.hpp:96) */
    double gravWaveTheta; /* viewing angles of the gravitational-wave polarisations */
    double gravWavePhi;
} sx_obs_settings;
/*! zeros, and 1 for the masses (a fraction that is a particle count until the caller sets them) */
int sx_obs_default_settings(sx_obs_settings* s);
/*! extra sums of a kind: 0, 1, 3, 1, 6; -1 for an unknown kind */
int sx_obs_num_sums(int kind);
/*! one fused, deterministic pass over [first, last) of f (replaces gpuGrowthRate, machSquareSumGpu and survivorsGpu,
 *  main/src/observables/gpu_reductions.cu:69-168, each together with conservedQuantitiesGpu, conserved_gpu.cu:71-94;
 *  and d2QuadpoleMomentum, grav_waves_calculations.hpp:87-121, which the reference runs on host vectors,
 *  gravitational_waves.hpp:114).  out receives this rank's sums, all double: the nine of sx_conserved_quantities,
 *  then
 *    SX_OBS_MACH_RMS     sum |v|^2 / c^2 (float per term, as MachSquareSum)
 *    SX_OBS_KH_GROWTH    sum si, sum ci, sum di with ybox = box->lim[3] - box->lim[2] (localGrowthRate,
 *                        time_energy_growth.hpp:57-63: xm / kx in float, the rest in double)
 *    SX_OBS_WIND_BUBBLE  the number of particles with kx / xm * m >= 0.64 rhoBubble and temp <= 0.9 tempWind
 *    SX_OBS_GRAV_WAVES   d2Q xx, yy, zz, xy, xz, yz (the diagonal times 2/3 after the sum, as :108)
 *  SX_ERR_ARG with a message when cap < 9 + sx_obs_num_sums(kind) or a field of the kind is NULL: c for the Mach RMS,
 *  kx, xm for the KH growth and the wind bubble (and temp for the latter), ax, ay, az for the gravitational waves.
 *  A caller that holds only the kind's fields (the signatures of gpu_reductions.h) may leave fields of the conserved
 *  sums NULL (x y z vx vy vz m, temp or u): the nine conserved sums are then zero and only the kind's fields are read
 *  (SX_OBS_TIME_ENERGY needs them all).  settings may be NULL unless kind is SX_OBS_WIND_BUBBLE.  The result does not
 *  depend on the device or the run: fixed grid, fixed order, no atomics.  Synchronises. */
int sx_observables(sx_ctx* ctx, const sx_fields* f, const sx_box* box, uint32_t first, uint32_t last, int kind,
                   const sx_obs_settings* settings, float muiConst, double gamma, double* out, int cap);
/*! computeHtt (grav_waves_calculations.hpp:50-84): out = {h+, hx} of the quadrupole's second derivative q (xx, yy,
 *  zz, xy, xz, yz) seen from (theta, phi), in the reference's units (10 kpc).  Host arithmetic, needs no GPU. */
int sx_grav_wave_htt(const double q[6], double theta, double phi, double out[2]);
/*! the observable from the sums of sx_observables added over the ranks (globalSums: nine conserved + the kind's) and
 *  the global particle count.  Host arithmetic, needs no GPU.  out receives
 *    SX_OBS_TIME_ENERGY  nothing
 *    SX_OBS_MACH_RMS     sqrt(sum / N)                            (turbulence_mach_rms.hpp:84)
 *    SX_OBS_KH_GROWTH    2 sqrt(s^2 + c^2) / d                    (time_energy_growth.hpp:109)
 *    SX_OBS_WIND_BUBBLE  count * particleMass / initialMass       (wind_bubble_fraction.hpp:96)
 *    SX_OBS_GRAV_WAVES   h+, hx at (gravWaveTheta, gravWavePhi)   (gravitational_waves.hpp:86) */
int sx_obs_finalize(int kind, const sx_obs_settings* settings, const double* globalSums, uint64_t numParticlesGlobal,
                    double* out);

/* ---- maps: column density and slices of the particles as images (sph-exa_amd/csrc/sx_map.hpp) -----------------
 * The device-side counterpart of the reference's in-situ "Density" scene (viz::execute, main/src/insitu_viz.h:35;
 * ascent_adaptor.h:41-48, 109-132, which renders host copies through Ascent): the state reduced to an image without
 * leaving the device.  For an image plane with normal `axis` the in-plane axes (u, v) are its cyclic successors: (y, z),
 * (z, x), (x, y).  With W(q) = sinc(pi q / 2)^6, Y(q) = 2 int_0^sqrt(4 - q^2) W(sqrt(q^2 + s^2)) ds and the pixel
 * centre P:
 *   SX_MAP_COLUMN  sum0(P) = sum_j m_j K Y(b_j / he_j) / he_j^2, b_j the in-plane distance, he_j = max(h_j, half the
 *                  larger pixel size) so that no particle falls between the pixel centres: the column density.  depth > 0
 *                  keeps the particles whose normal coordinate lies within depth / 2 of center's.
 *   SX_MAP_SLICE   sum0(P) = sum_j m_j K W(r_j / h_j) / h_j^3, r_j the distance to P on the plane through center: the
 *                  SPH mass density there (h is not clamped).
 *   sum1(P) = sum_j w_j a_j over the same weights w_j: sum1 / sum0 is the mass-weighted mean of the column a.
 * Distances are minimum-image on periodic axes, plain on open and fixed ones; the window may straddle a periodic edge.
 * Neither map reads rho or a volume element, so the VE, std and gravity-only layouts are served alike (the last with h
 * as the softening length).  Accumulation is in float in ascending particle index per pixel, stored as double: the
 * image does not depend on the run, the device's scheduling or the pair cap. */
#define SX_MAP_COLUMN 0
#define SX_MAP_SLICE 1
typedef struct sx_map
{
    int32_t  kind, axis; /* axis = normal: 0 x, 1 y, 2 z */
    double   center[3];  /* window centre; its normal component is the slice plane / slab centre */
    double   width[2];   /* extent along u, v */
    double   depth;      /* column: slab thickness, 0 = unbounded; slice: ignored */
    uint32_t npix[2];    /* pixels along u, v; image is npix[1] rows of npix[0], u fastest */
} sx_map;
/*! host only, needs no GPU: SX_OK, or SX_ERR_ARG with the reason in sx_last_error(NULL) (per thread).  Refused, each
 *  with its own message: a NULL argument, an unknown kind, an unknown axis, npix of 0 or above 4096, a width that is
 *  not positive, a width above the box length on a periodic axis, a negative depth. */
int sx_map_check(const sx_map* map, const sx_box* box);
/*! host evaluation of the register-resident Y(t), t = q^2, of the column maps (mapKernelY, sx_kernel_poly.hpp), for
 *  checking it against a quadrature; like sx_kernel_poly */
int sx_map_kernel(const float* t, size_t n, float* y);
/*! records the render kernel stages through LDS at a time (tests place a tile's list length around its multiples) */
uint32_t sx_map_chunk_records(void);
/*! pairs (tile, particle) produced and sorted at a time: a render works through the image in bands of whole rows of
 *  16 x 16-pixel tiles whose pairs stay within this cap; 0 = the default (2^27: 24 B per pair with the sort's storage, 3.2 GB at most).  The
 *  image is bit-identical for every cap.  A render in which one tile row alone exceeds the cap (or 2^31 - 1 pairs)
 *  returns SX_ERR_ARG. */
int sx_set_map_pair_cap(sx_ctx* ctx, uint64_t pairs);
/*! renders map over the particles [first, last) of f into sum0 (and sum1), device arrays of npix[0] * npix[1] doubles.
 *  Reads x y z h m of f and K (sx_params.K); a: any device column of length f->n, float or double (aIsDouble), or NULL:
 *  then sum1 is not touched.  sum0 and sum1 are overwritten, not added to.  Runs on the context stream and synchronises
 *  it once, after counting the pairs (the bands are planned on the host); the images are complete when the stream is.
 *  The scratch (pairs, sort buffers) lives in the context.  SX_ERR_ARG: whatever sx_map_check refuses, missing fields,
 *  first > last or last > f->n, a tile row beyond the pair cap. */
int sx_map_render(sx_ctx* ctx, const sx_fields* f, const sx_box* box, uint32_t first, uint32_t last, double K,
                  const sx_map* map, const void* a, int aIsDouble, double* sum0, double* sum1);
/*! the context's last render: {pairs, bands, longest tile list, particles with a footprint in the window};
 *  synchronises.  SX_ERR_ARG before the first render. */
int sx_map_stats(sx_ctx* ctx, uint64_t out[4]);
/*! measurement: with on != 0 the following renders time their stages with HIP events (and synchronise after every
 *  band); sx_map_times: {binning, sort, render} in ms and out[3] = the scratch bytes of the last render */
int sx_set_map_timing(sx_ctx* ctx, int on);
int sx_map_times(sx_ctx* ctx, double out[4]);

/* ---- power spectra: mesh deposit, 3-D FFT, shell sums (sph-exa_amd/csrc/sx_spectrum.hpp) ----------------------
 * The reference carries an SPH_EXA_WITH_FFTW switch (CMakeLists.txt:84-89) that nothing in it uses; like the maps this
 * is a counterpart of our own design: the state reduced on the device, here to a few hundred numbers.
 * Box and mesh.  The box must be periodic on all three axes and cubic, with edge L.  The mesh has n^3 cells,
 *   n in {16, 32, 64, 128, 256}.  Cell size is D = L / n.  Cell (ix, iy, iz) has its centre at lim_lo + (i + 1/2) D per
 *   axis.  Cells are stored [iz][iy][ix], x fastest.
 * Deposit.  S0(c) = sum_j m_j K W(r_jc / he_j) / he_j^3, with W = sinc^6 (the pair kernels' kernelWt).  r is the
 *   minimum-image distance to the cell centre.  he_j = max(h_j, D / 2): with this clamp every particle reaches at least
 *   one centre, as the column maps clamp theirs.  Up to three further sums S1_a(c) = sum_j w_jc a_j use the same
 *   weights, for three device columns a (float or double).  Neither rho nor a volume element is read, so the VE, std and
 *   gravity-only layouts are served alike.  Each cell sums in float, FMA, in ascending particle index, and stores a
 *   double.  A cell is exactly 0 where no support contains its centre.  There are no float atomics.  The result is
 *   bit-identical from run to run and for every pair cap.
 * Field that is transformed.  SX_SPEC_VELOCITY: W_a = S0^p S1_a / S0 for a = vx, vy, vz.  weight 0 means p = 0, the
 *   mass-weighted mean velocity; weight 1 means p = 1/2, the kinetic-energy spectrum; weight 2 means p = 1/3.  The
 *   prefactor is 1/2.  SX_SPEC_SCALAR: one column, or the mesh density S0 itself when no column is given.  weight must
 *   be 0.  The prefactor is 1.  W = 0 where S0 = 0.  W is computed in double from the stored sums.
 * Transform and shells.  What(n) = n^-3 sum_c W(c) exp(-2 pi i n.c / n), a complex-to-complex FFT in double.  Integer
 *   wave vectors are n_i in [-n/2, n/2).  Shell index: s = floor(|n| + 1/2).  Shell count: numShells =
 *   floor(sqrt(3) n / 2 + 1/2) + 1.  power[s] = prefactor sum_a sum_{n in s} |What_a(n)|^2.  modes[s] = the number of
 *   wave vectors in shell s, a u64.  It follows that sum_s power[s] = prefactor <sum_a W_a^2> over the cells (Parseval).
 *   The physical wave number of shell s is 2 pi s / L.  The shell sums have a fixed order: the same bits every run. */
#define SX_SPEC_VELOCITY 0
#define SX_SPEC_SCALAR 1
typedef struct sx_spectrum
{
    int32_t  kind, weight; /* weight: the p of SX_SPEC_VELOCITY (0: 0, 1: 1/2, 2: 1/3) */
    uint32_t n;            /* cells per axis */
} sx_spectrum;
/*! host only, needs no GPU: SX_OK, or SX_ERR_ARG with the reason in sx_last_error(NULL) (per thread).  Refused, each
 *  with its own message: a NULL argument, an unknown kind, an unknown weight, a non-zero weight with SX_SPEC_SCALAR, an n
 *  that is not one of the five sizes, a box with an open or fixed axis, a non-cubic box. */
int sx_spectrum_check(const sx_spectrum* spec, const sx_box* box);
/*! host only: floor(sqrt(3) n / 2 + 1/2) + 1, or 0 for an n that is not one of the five sizes */
uint32_t sx_spectrum_num_shells(uint32_t n);
/*! host only: the wave vectors per shell into modes[sx_spectrum_num_shells(n)]; SX_ERR_ARG for another n */
int sx_spectrum_modes(uint32_t n, uint64_t* modes);
/*! pairs (block, particle) the deposit produces and sorts at a time: it works through the mesh in bands of whole layers
 *  of 8 x 8 x 4-cell blocks along z whose pairs stay within this cap; 0 = the default (2^27).  The mesh is bit-identical
 *  for every cap.  A deposit in which one layer alone exceeds the cap (or 2^31 - 1 pairs) returns SX_ERR_ARG. */
int sx_set_spectrum_pair_cap(sx_ctx* ctx, uint64_t pairs);
/*! records the gather kernel stages through LDS at a time (tests place a block's list length around its multiples) */
uint32_t sx_spectrum_chunk_records(void);
/*! the deposit over the particles [first, last) of f onto the n^3 mesh: sum0 (n^3 doubles) and sum1 (numA meshes of n^3
 *  doubles, one behind the other), device arrays, overwritten.  Reads x y z h m of f and K; a[0 .. numA): device columns
 *  of length f->n, all float or all double (aIsDouble); numA in 0 .. 3 (0: a and sum1 may be NULL).  The box is checked
 *  as by sx_spectrum_check.  Runs on the context stream and synchronises it once, after counting the pairs. */
int sx_mesh_deposit(sx_ctx* ctx, const sx_fields* f, const sx_box* box, uint32_t first, uint32_t last, double K,
                    uint32_t n, const void* const a[3], int numA, int aIsDouble, double* sum0, double* sum1);
/*! in place, forward, scaled by n^-3: complexMesh holds n^3 interleaved complex doubles (device, 16-byte aligned).  A
 *  kernel of our own (Stockham, radix 4 and 2, in LDS; the twiddle table is built once per n on the host in double and
 *  kept in the context); the library links no FFT package. */
int sx_fft3d(sx_ctx* ctx, double* complexMesh, uint32_t n);
/*! power[s] = (accumulate ? power[s] : 0) + prefactor sum_{n in s} |complexMesh(n)|^2 over the transformed mesh, and
 *  modes[s] (nullable); device arrays of sx_spectrum_num_shells(n) entries.  Fixed order of the sums: a mode permutation
 *  grouped by shell (built once per n, kept in the context), leaves of 2048 modes reduced by a fixed tree, the leaves of
 *  a shell added in ascending order. */
int sx_shell_sums(sx_ctx* ctx, const double* complexMesh, uint32_t n, double prefactor, int accumulate, double* power,
                  uint64_t* modes);
/*! all stages: deposit, field, transform, shell sums; power and modes (nullable) are device arrays of
 *  sx_spectrum_num_shells(spec->n) entries.  SX_SPEC_VELOCITY: a[0 .. 3) are the velocity columns, a NULL: f->vx, vy, vz
 *  (float).  SX_SPEC_SCALAR: a[0] is the column, a or a[0] NULL: the mesh density.  The velocity kinds transform
 *  W_x + i W_y as one complex field and W_z as another: every shell is symmetric under n -> -n, so the shell sums of
 *  |FFT(W_x + i W_y)|^2 equal those of |What_x|^2 + |What_y|^2.  The meshes live in the context from the first call on:
 *  (2 + 4 n^3) doubles of sums, one complex mesh of 2 n^3 doubles, the permutation of n^3 u32 -- 805 MB + 67 MB at
 *  n = 256 -- and the deposit's pair scratch (24 B per pair).  Synchronises. */
int sx_spectrum_compute(sx_ctx* ctx, const sx_fields* f, const sx_box* box, uint32_t first, uint32_t last, double K,
                        const sx_spectrum* spec, const void* const a[3], int aIsDouble, double* power, uint64_t* modes);
/*! the context's last deposit: {pairs, bands, longest block list, particles clamped to D / 2}; synchronises.
 *  SX_ERR_ARG before the first deposit. */
int sx_spectrum_stats(sx_ctx* ctx, uint64_t out[4]);
/*! measurement: with on != 0 the following calls time their stages with HIP events (and synchronise after each);
 *  sx_spectrum_times: {binning, sort, gather, fft, shells} in ms, summed since the last deposit began */
int sx_set_spectrum_timing(sx_ctx* ctx, int on);
int sx_spectrum_times(sx_ctx* ctx, double out[5]);

/* ---- binned profiles and analytic L1 with exact sums (sph-exa_amd/csrc/sx_profile.hpp) -------------------------
 * The device-side counterpart of main/src/analytical_solutions/compare_solutions.py:85-89 (computeL1Error) and
 * compare_noh.py:141-148, which run on HDF5 dumps: a binned reduction over the particles that returns a few numbers per
 * bin.  The bin coordinate is a radius, an axis coordinate or a quantity (the last gives PDFs).
 * Arithmetic rule.  All per-particle arithmetic below is IEEE double unless it says float; every operation is rounded
 *   on its own (no FMA contraction); sqrt and / are correctly rounded.  (a op b) op c is written with its brackets.
 * Displacement.  d_a = x_a - center_a; on a periodic axis of length L_a = lim_hi - lim_lo then
 *   d_a <- d_a - L_a * rint(d_a / L_a), rint to nearest, ties to even.  Open and fixed axes are plain.
 * Coordinate c.  SX_PROF_RADIUS: r = sqrt((dx*dx + dy*dy) + dz*dz).  SX_PROF_X, _Y, _Z: d_a.  SX_PROF_QUANTITY: the
 *   value of the quantity coordQ below.
 * Bins.  edges[nbins + 1], a host array, finite and strictly ascending; 1 <= nbins <= 4096.  A particle is in bin b iff
 *   edges[b] <= c < edges[b + 1].  Every array of the result has nbins + 2 entries per row: entry nbins holds the
 *   particles with c < edges[0] (underflow), entry nbins + 1 those with c >= edges[nbins] (overflow); all moments are
 *   kept for these two as for any bin.
 * Quantities q[k], k < nq <= SX_PROF_MAX_Q.  cv = (double)(float)((double)(8.317e7f / muiConst) / (gamma - 1.0)), the
 *   EOS kernels' constant; gm1 = gamma - 1.0.
 *     SX_PROF_RHO    VE, ve-bdt (std = 0): the float (kx * m) / xm; std: the float column rho.  Then widened.
 *     SX_PROF_P      (float)((double)rho * ((cv * temp) * gm1)) with rho as above, then widened.
 *     SX_PROF_U      cv * temp.          SX_PROF_TEMP   temp.
 *     SX_PROF_VEL    sqrt((vx*vx + vy*vy) + vz*vz), the float velocities widened first.
 *     SX_PROF_VRAD   ((dx*vx + dy*vy) + dz*vz) / r, and 0 where r = 0.
 *     SX_PROF_C, _H, _DIVV, _CURLV, _ALPHA   the float column, widened.
 *   A quantity whose columns are NULL in sx_fields is refused with a reason.
 * Weight.  w = 1.0 (SX_PROF_NUMBER) or (double)m (SX_PROF_MASS).
 * Solution sol[k] of quantity slot k, evaluated at xi = c * rscale.
 *     SX_PROF_SOL_NONE   no solution; the series D of the slot is zero.
 *     SX_PROF_SOL_TABLE  host arrays r[nt], y[nt], r ascending (equal neighbours allowed), 2 <= nt <= 2^20; numpy.interp:
 *                        xi < r[0]: y[0]; xi >= r[nt-1]: y[nt-1]; else with j the last index with r[j] <= xi: y[j] if
 *                        xi == r[j], otherwise ((y[j+1] - y[j]) / (r[j+1] - r[j])) * (xi - r[j]) + y[j].  A Sedov table
 *                        of time t_sol serves time t with rscale = (t_sol / t)^0.4.
 *     SX_PROF_SOL_NOH_RHO  compare_noh.py:49-60 with (gamma, rho0, vel0, time, xgeom in 1..3): r2 = ((0.5 * (gamma - 1))
 *                        * |vel0|) * time; xi > r2: rho0 * b^(xgeom-1) with b = 1.0 - (vel0 * time) / max(xi, 1e-300)
 *                        and the power 1.0, b or b * b; otherwise rho0 * pow((gamma + 1) / (gamma - 1), xgeom), computed
 *                        once on the host with the C library's pow.
 * Series.  1 + 3 nq series of terms per particle: W: w; per slot S1 = w * q, S2 = (w * q) * q, D = w * |q - s(c)|.
 *   count[b] (u64) is the number of particles of the bin, min and max of q per bin are exact; an empty bin has count 0,
 *   sums 0, min +inf, max -inf.  A particle whose coordinate, any requested quantity, solution value or term is not
 *   finite enters no bin and is counted in `nonfinite` instead.
 * The exact sum of a series.  M = the largest |term| of the series over all finite particles of all ranks; E = the
 *   smallest integer with M < 2^E (M = 2^k gives E = k + 1; M = 0: every sum is 0).  fixed(t) = sign(t) *
 *   floor(|t| * 2^(96 - E)), formed by shifting the mantissa, so bits below 2^(E - 96) are dropped.  Each bin
 *   accumulates sum fixed(t) in a 128-bit two's-complement integer, which cannot overflow below 2^31 particles (more are
 *   refused).  The stored result is the double nearest (ties to even) to sum * 2^(E - 96), subnormals included.
 *   It follows that a sum differs from the exact real sum by less than count * 2^(E - 96) plus one final rounding, and
 *   that it does not depend on the order, the launch shape, any internal capacity or the number of ranks.
 * Derived by the caller, sums in ascending index: mean_k[b] = S1_k[b] / W[b]; l1_k = (sum over all nbins + 2 entries of
 *   D_k) / (sum of W): with SX_PROF_NUMBER the reference's mean |solution - q| over all particles, whatever the edges. */
#define SX_PROF_RADIUS 0
#define SX_PROF_X 1
#define SX_PROF_Y 2
#define SX_PROF_Z 3
#define SX_PROF_QUANTITY 4
#define SX_PROF_RHO 0
#define SX_PROF_P 1
#define SX_PROF_U 2
#define SX_PROF_TEMP 3
#define SX_PROF_VEL 4
#define SX_PROF_VRAD 5
#define SX_PROF_C 6
#define SX_PROF_H 7
#define SX_PROF_DIVV 8
#define SX_PROF_CURLV 9
#define SX_PROF_ALPHA 10
#define SX_PROF_NUMBER 0
#define SX_PROF_MASS 1
#define SX_PROF_SOL_NONE 0
#define SX_PROF_SOL_TABLE 1
#define SX_PROF_SOL_NOH_RHO 2
#define SX_PROF_MAX_Q 4
typedef struct sx_profile_solution
{
    int32_t       kind;
    uint32_t      nt;     /* table: entries of r and y */
    const double *r, *y;  /* table: host arrays */
    double        rscale; /* xi = c * rscale */
    double        gamma, rho0, vel0, time; /* Noh */
    int32_t       xgeom;                   /* Noh: 1 planar, 2 cylindrical, 3 spherical */
} sx_profile_solution;
typedef struct sx_profile
{
    int32_t             coord, coordQ, weight; /* coordQ: the quantity of SX_PROF_QUANTITY */
    double              center[3];
    uint32_t            nbins;
    const double*       edges; /* host, nbins + 1 */
    uint32_t            nq;
    int32_t             q[SX_PROF_MAX_Q];
    sx_profile_solution sol[SX_PROF_MAX_Q];
} sx_profile;
/*! every pointer nullable (then not written); device pointers for sx_profile_compute, host pointers for sx_sim_profile */
typedef struct sx_profile_result
{
    uint64_t* count;     /* [nbins + 2] */
    uint64_t* nonfinite; /* one */
    double*   W;         /* [nbins + 2] */
    double *  S1, *S2, *D, *min, *max; /* [nq][nbins + 2] */
} sx_profile_result;
/*! host only, needs no GPU: SX_OK, or SX_ERR_ARG with the reason in sx_last_error(NULL) (per thread).  Refused, each
 *  with its own message: a NULL argument, an unknown coord, quantity, weight or solution kind, nbins of 0 or above 4096,
 *  edges that are not finite or not strictly ascending, nq above SX_PROF_MAX_Q, a table with nt below 2 or above 2^20 or
 *  without its arrays, a table whose r descends or is not finite, an xgeom outside 1..3, a solution on a slot >= nq. */
int sx_profile_check(const sx_profile* prof, const sx_box* box);
/*! host only, the number format of the exact sums: *E = the window of n terms (the smallest E with max |t| < 2^E, and
 *  -1074 where every term is 0); SX_ERR_ARG for a term that is not finite */
int sx_profile_window(const double* t, size_t n, int32_t* E);
/*! host only: fixed(t[i]) of window E as two words, lohi[2 i] the low and lohi[2 i + 1] the high half of the 128-bit
 *  two's-complement integer; SX_ERR_ARG for a term that is not finite or not below 2^E in magnitude */
int sx_profile_to_fixed(const double* t, size_t n, int32_t E, uint64_t* lohi);
/*! host only: acc (low, high) += the n integers of lohi, modulo 2^128 */
int sx_profile_add_fixed(uint64_t acc[2], const uint64_t* lohi, size_t n);
/*! host only: *out = the double nearest (ties to even) to acc * 2^(E - 96), subnormals included */
int sx_profile_from_fixed(const uint64_t acc[2], int32_t E, double* out);
/*! the largest nbins for which the bins of nq quantities fit one block-private LDS tile (64 KB less 128 bytes per
 *  workgroup, so that two workgroups stay resident per CU; 24 + 64 nq bytes per bin, nbins + 2 bins); above it the bins
 *  are split into ceil((nbins + 2) / (that + 2)) tiles and pass 2 runs once per tile.  The result has the same bits
 *  either way.  0 for an nq outside 0 .. 4. */
uint32_t sx_profile_lds_bins(int nq);
/*! measurement and tests: on = 0 makes the following sx_profile_compute calls of the context add straight into the
 *  global array with global atomics (one pass 2, no tiles: the same bits, far slower), 1 (the default) in LDS */
int sx_set_profile_lds(sx_ctx* ctx, int on);
/*! the profile of the particles [first, last) of f (at most 2^31 - 1) into the device arrays of deviceOut.  gamma and
 *  muiConst are read from params; std != 0 reads the rho column.  Two passes over the particles (the windows, then the
 *  integer sums; 64-bit integer atomics in LDS and in global memory) and one conversion kernel.  The accumulators and
 *  the uploaded edges and tables live in the context.  SX_ERR_ARG: whatever sx_profile_check refuses, a quantity whose
 *  columns are NULL, first > last or last > f->n.  Synchronises. */
int sx_profile_compute(sx_ctx* ctx, const sx_fields* f, const sx_box* box, uint32_t first, uint32_t last,
                       const sx_params* params, int std, const sx_profile* prof, sx_profile_result* deviceOut);
/*! the context's last profile: {particles read, 1 if the bins were in LDS, passes over the particles (1 + tiles),
 *  nonfinite};
 *  SX_ERR_ARG before the first */
int sx_profile_stats(sx_ctx* ctx, uint64_t out[4]);
/*! measurement: with on != 0 the following calls time their kernels with HIP events; sx_profile_times: {pass 1, pass 2,
 *  conversion} in ms of the last call and out[3] = the bytes one pass reads */
int sx_set_profile_timing(sx_ctx* ctx, int on);
int sx_profile_times(sx_ctx* ctx, double out[4]);

/* ---- friends-of-friends groups: cell grid, lock-free union-find, catalogue (sph-exa_amd/csrc/sx_fof.hpp) ---------
 *
 * Link.      Particles i != j of [first, last) are friends iff dx^2 + dy^2 + dz^2 < linking^2 (strict), in double, the
 *            squares summed in this order.  d_a = a_i - a_j; on an axis with bnd == 1 it is the minimum image (L_a added
 *            or subtracted once where |d_a| > L_a / 2), on open (0) and fixed (2) axes the plain difference.
 * Groups.    The connected components of that relation.  Every particle belongs to exactly one; a particle without
 *            friends is a group of one.  The partition is a property of the particle set, not of the algorithm.
 * Label.     The smallest id among the members when an id column is given, else the smallest particle index (the index
 *            in the columns of f, first included).  With ids the labels do not depend on the order of storage.
 * Catalogue. The groups with at least minMembers members, ordered by member count descending, ties by label ascending:
 *            label, count, mass M = sum m, centre of mass, mass-weighted mean velocity.
 *            Centre of mass: x_ref + (sum m minimage(x - x_ref)) / M with x_ref the label particle's position, folded
 *            back into [min, max) on periodic axes.  EXACT ONLY FOR A GROUP THAT SPANS LESS THAN HALF THE BOX on every
 *            periodic axis: beyond that the minimum image of a member is not its image in the group.
 *            Velocity: (sum m v) / M.  m, m * v and the sums are doubles (m * v of two floats is exact).
 * Order.     The members of a catalogue group are summed in ascending id (or index) order: 256 partial sums, partial k
 *            taking members k, k + 256, ... in turn, then a pairwise tree over the partials.  No floating-point atomic
 *            anywhere, so the catalogue has the same bits on every run and, with ids, under any permutation of the input.
 * One rank.  Components that cross rank boundaries need an iterated label exchange: sx_sim_fof refuses a sim with a
 *            communicator of more than one rank. */
typedef struct sx_fof
{
    double   linking;    /* the linking length, absolute */
    uint32_t minMembers; /* the catalogue lists groups with at least this many members (0 counts as 1) */
    uint32_t maxGroups;  /* capacity of the catalogue arrays */
} sx_fof;
/*! every pointer nullable (then not written); device pointers for sx_fof_compute, host pointers for sx_sim_fof */
typedef struct sx_fof_result
{
    uint64_t* label;      /* [last - first], in the order of the columns */
    uint64_t* groupLabel; /* [maxGroups] */
    uint32_t* groupCount; /* [maxGroups] */
    double*   groupMass;  /* [maxGroups] */
    double*   groupCom;   /* [maxGroups][3] */
    double*   groupVel;   /* [maxGroups][3] */
    uint64_t* numGroups;  /* [0] groups with count >= minMembers (may exceed maxGroups: the first maxGroups are written),
                             [1] all groups, singles included */
} sx_fof_result;
/*! host only, needs no GPU: SX_OK, or SX_ERR_ARG with the reason and its figures in sx_last_error(NULL) (per thread).
 *  Refused: a NULL argument, a linking length that is not finite or not positive, one above a third of the box length on
 *  a periodic axis (three distinct cells and an unambiguous minimum image need it). */
int sx_fof_check(const sx_fof* fof, const sx_box* box);
/*! host only: the cell grid a call on n particles uses.  Per axis floor(L_a / linking * (1 - 2^-20)) cells, at least 1
 *  (3 on a periodic axis) and at most 1024, so that a cell's edge L_a / dims[a] exceeds the linking length and friends
 *  lie in the same or in adjacent cells whatever the rounding of a cell coordinate; then, while the cells number more
 *  than max(27, 2 n), the axis with the most cells (the first of equals) takes ceil(dims / 2), not below its minimum.
 *  So the dense cell-start array stays below 8 bytes per particle.  SX_ERR_ARG: whatever sx_fof_check refuses. */
int sx_fof_grid(const sx_fof* fof, const sx_box* box, uint64_t n, uint32_t dims[3]);
/*! the groups of the particles [first, last) of f (x, y, z; m, vx, vy, vz for the catalogue's mass, centre and velocity:
 *  no other column is read, so the gravity-only layout serves) into the device arrays of deviceOut.  id: device, f->n
 *  entries, or NULL.  Particles outside [first, last) link nothing.  A particle outside an open box is binned into the
 *  edge cell (clamping is monotone: friends stay in the same or in adjacent cells); on a periodic axis it is wrapped.
 *  Stages: cell keys, count and sort (hipcub); link (one wave per 64 consecutive sorted targets, each unordered pair
 *  tested once from its earlier member, union by compare-and-swap of the larger root under the smaller); compress, the
 *  labels (64-bit integer minimum) and the member counts (integer adds); the catalogue (two stable sorts each for the
 *  groups and for the members, one workgroup per group).  The scratch lives in the context under the tags fof.*, about
 *  285 bytes per particle once a catalogue has been asked for.  SX_ERR_ARG: whatever sx_fof_check refuses, maxGroups == 0 with a catalogue pointer set,
 *  missing columns, first > last or last > f->n, more than 2^31 - 1 particles.  Synchronises (twice). */
int sx_fof_compute(sx_ctx* ctx, const sx_fields* f, const sx_box* box, uint32_t first, uint32_t last,
                   const uint64_t* id, const sx_fof* fof, const sx_fof_result* deviceOut);
/*! the context's last call: {pair tests, union retries (a compare-and-swap that lost against another wave), all groups,
 *  groups with count >= minMembers}; SX_ERR_ARG before the first */
int sx_fof_stats(sx_ctx* ctx, uint64_t out[4]);
/*! measurement: with on != 0 the following calls time their stages with HIP events; sx_fof_times: {grid, link,
 *  compress, catalogue} in ms of the last call */
int sx_set_fof_timing(sx_ctx* ctx, int on);
int sx_fof_times(sx_ctx* ctx, double out[4]);

/* ---- group properties: density cut, shape, dispersion, spin, self-energy (sph-exa_amd/csrc/sx_halo.hpp) ----------
 *
 * Arithmetic. IEEE double, every operation rounded on its own (the file is built with -ffp-contract=off), brackets as
 *             written, unless a line says float.  Float columns are widened first; that conversion is exact.
 * Selection.  A particle of [first, last) is selected iff rhoMin <= 0 or rho >= rhoMin, rho by the rule of SX_PROF_RHO:
 *             the float (kx * m) / xm, or the float column rho when std != 0, then widened.  A NaN rho is not selected.
 *             Unselected particles link nothing and belong to no group: their label is UINT64_MAX and they count in
 *             neither entry of numGroups.  (A selected particle with a NaN x counts as unselected.)
 * Groups, labels, catalogue order, mass, com, vel.  Exactly sx_fof's, over the selected particles; with rhoMin <= 0
 *             the same bits as sx_fof_compute returns for the same input.
 * Moments (SX_HALO_MOMENTS), per catalogue group with X = com, V = vel, M = mass as returned:
 *             d_a = minimage(x_a - X_a) by the rule of sx_fof (L_a added or subtracted once where |d_a| > L_a / 2),
 *             w_a = (double)v_a - V_a, and with the components ab in the order xx, xy, xz, yy, yz, zz
 *               sigma[ab] = (sum (m * w_a) * w_b) / M        shape[ab] = (sum (m * d_a) * d_b) / M
 *               angmom    = sum m * ((d_y * w_z) - (d_z * w_y)),  m * ((d_z * w_x) - (d_x * w_z)),
 *                               m * ((d_x * w_y) - (d_y * w_x))
 *               rmax      = sqrt(max ((d_x * d_x + d_y * d_y) + d_z * d_z)), the exact maximum, one sqrt.
 *             The caveat of com applies: a group must span less than half a periodic box.
 * Thermal (SX_HALO_THERMAL).  eint = sum m * (cv * temp), cv as the profile section defines it.
 * Potential (SX_HALO_POTENTIAL).  epot = -(G * sum over the unordered member pairs i < j of m_i m_j r^2 / r_eff^3), r^2
 *             from the minimum-image differences (formed in double), r_eff^2 = max(r^2, (h_i + h_j)^2) with h_i + h_j
 *             and its square formed in float: the P2P of sx_gravity_direct, so a group uploaded alone has epot == egrav of that call up
 *             to rounding.  A pair with r^2 = 0 contributes 0.  A group with more than maxPairMembers members gets
 *             epot = NaN.
 *             Accuracy contract: |epot - W| <= 2^-15 |W| with W the sum in exact arithmetic (every term has the same
 *             sign).  The kernel rounds the double differences to float, evaluates a term in float with the hardware's
 *             reciprocal square root (1 ulp), adds at most 64 terms in one float accumulator and goes on in double:
 *             (23 + 63) 2^-24 = 2^-17.6 at worst, so the contract has a factor 5 of margin.  It assumes
 *             that m_j / r_eff and the squares of the differences stay inside the float range.
 * Order.      Moments and eint: the members in ascending id (or index), 256 partial sums, partial k taking members
 *             k, k + 256, ..., then a pairwise tree: the catalogue's rule.  epot: the members of a group in ascending id
 *             in tiles of 256; work item k = b (b + 1) / 2 + a of the group is the pair of tiles a <= b (the diagonal
 *             item takes j > i only); inside an item target lane t adds its sources s ascending into accumulator s % 4,
 *             the lanes are added by a pairwise tree, and the group's items by 256 partial sums over k, k + 256, ... and
 *             a pairwise tree.  All of it is a function of the member count alone; no floating-point atomic anywhere:
 *             the same bits on every run and, with ids, under any permutation of the input.
 * One rank.   As sx_sim_fof, sx_sim_halos refuses a communicator of more than one rank. */
#define SX_HALO_MOMENTS 1u
#define SX_HALO_THERMAL 2u
#define SX_HALO_POTENTIAL 4u
typedef struct sx_halo
{
    double   linking;        /* as in sx_fof */
    uint32_t minMembers;     /* as in sx_fof */
    uint32_t maxGroups;      /* as in sx_fof */
    double   rhoMin;         /* the density cut; <= 0: none */
    int32_t  std;            /* which density rule applies, as sx_profile_compute takes it */
    float    G;              /* gravitational constant of epot */
    uint32_t flags;          /* SX_HALO_* */
    float    muiConst;       /* thermal only */
    double   gamma;          /* thermal only */
    uint32_t maxPairMembers; /* groups above it get epot = NaN; 0 means 2^20 */
} sx_halo;
/*! every pointer nullable (then not written); device pointers for sx_halo_compute, host pointers for sx_sim_halos.  An
 *  array whose flag is clear is not written either. */
typedef struct sx_halo_result
{
    uint64_t* label;      /* the seven of sx_fof_result */
    uint64_t* groupLabel;
    uint32_t* groupCount;
    double*   groupMass;
    double*   groupCom;
    double*   groupVel;
    uint64_t* numGroups;
    double*   groupSigma;  /* [maxGroups][6]  SX_HALO_MOMENTS */
    double*   groupShape;  /* [maxGroups][6]  SX_HALO_MOMENTS */
    double*   groupAngmom; /* [maxGroups][3]  SX_HALO_MOMENTS */
    double*   groupRmax;   /* [maxGroups]     SX_HALO_MOMENTS */
    double*   groupEint;   /* [maxGroups]     SX_HALO_THERMAL */
    double*   groupEpot;   /* [maxGroups]     SX_HALO_POTENTIAL */
} sx_halo_result;
/*! host only, needs no GPU: SX_OK, or SX_ERR_ARG with the reason in sx_last_error(NULL) (per thread).  Refused: whatever
 *  sx_fof_check refuses for (linking, minMembers, maxGroups), a rhoMin or G that is not finite, unknown flags, and with
 *  SX_HALO_THERMAL a gamma <= 1 or a muiConst <= 0 (or either not finite). */
int sx_halo_check(const sx_halo* halo, const sx_box* box);
/*! the groups of the particles [first, last) of f and their properties into the device arrays of deviceOut.  Columns:
 *  sx_fof_compute's; kx, m, xm (or rho with std) for rhoMin > 0; temp and m for the thermal energy; h and m for the
 *  potential.  Stages: sx_fof_compute's (the cut is a pass behind its gather), one workgroup per catalogue group for the
 *  moments, then for the potential a scan of the groups' work items, one workgroup of 256 lanes per pair of member tiles
 *  (the sources staged in 8 KB of LDS) and one workgroup per group for its items.  The search's scratch is the context's
 *  fof.* (sx_fof_stats then reports this call's search); the rest lives under halo.*: 144 bytes per catalogue entry and
 *  8 bytes per work item.  SX_ERR_ARG: whatever sx_halo_check or sx_fof_compute refuses and a flag or cut whose columns
 *  are NULL, each with its reason.  Synchronises. */
int sx_halo_compute(sx_ctx* ctx, const sx_fields* f, const sx_box* box, uint32_t first, uint32_t last,
                    const uint64_t* id, const sx_halo* halo, const sx_halo_result* deviceOut);
/*! the context's last call: {pair terms evaluated (= sum c (c - 1) / 2 over the groups that got an epot), pair work
 *  items, groups with an epot, groups over maxPairMembers}; SX_ERR_ARG before the first */
int sx_halo_stats(sx_ctx* ctx, uint64_t out[4]);
/*! measurement: with on != 0 the following calls time their stages with HIP events; sx_halo_times: {group search,
 *  moments, pair kernel (with the scan and the host's read of the item count), combination and copies} in ms */
int sx_set_halo_timing(sx_ctx* ctx, int on);
int sx_halo_times(sx_ctx* ctx, double out[4]);

/* ---- two-point statistics: pair counts and velocity structure functions (sph-exa_amd/csrc/sx_twopoint.hpp) -------
 *
 * Arithmetic. Double precision, every operation rounded on its own (the file is built with -ffp-contract=off), brackets
 *             as written.  Float columns (v, m) are converted to double first; that conversion is exact.
 * Particles.  The range [first, last) of f.  A particle whose x, y, z, vx, vy or vz is not finite takes part in no pair
 *             and is counted once in nonfinite; the same holds for a non-finite m where the mass series (WW) is asked
 *             for.  The other particles are the finite ones, n_f in number.
 * Targets.    stride >= 1, phase < stride.  A particle is a target iff key % stride == phase, key being its id where an
 *             id column is given, else its index in the columns of f (first included, as the labels of sx_fof).
 *             targets is the number of finite targets.
 * Pairs.      Every unordered pair {i, j}, i != j, of finite particles with at least one target member enters once.  With
 *             stride = 1 that is every pair.
 * Separation. d_a = a_j - a_i; on an axis with bnd == 1 it is the minimum image exactly as sx_fof defines it (L_a added
 *             or subtracted once where |d_a| > L_a / 2), on the other axes the plain difference.
 *             r2 = (dx^2 + dy^2) + dz^2 and r = sqrt(r2).  A pair with r2 == 0 enters no bin and is counted in
 *             coincident.
 * Bins.       edges[0 .. nbins], finite, strictly ascending, edges[0] >= 0, nbins <= 256.  A pair belongs to bin b iff
 *             edges[b] <= r < edges[b + 1]: the bin of np.searchsorted(edges, r, "right") - 1.  Pairs outside
 *             [edges[0], edges[nbins]) enter nothing; there are no underflow and overflow bins, because pairs beyond
 *             r_max = edges[nbins] are never enumerated.
 * Pair terms. dv_a = v_a,j - v_a,i;  u = ((dvx dx + dvy dy) + dvz dz) / r, the longitudinal velocity difference.  It is
 *             symmetric under i <-> j (both factors change sign, and IEEE products and sums are sign-symmetric), so
 *             "unordered" is well defined.
 * Series.     Per bin:  count = the number of pairs (u64, exact);  U1 = sum u;  U2 = sum u u;  U3 = sum (u u) u;
 *             A3 = sum |(u u) u|;  T2 = sum ((dvx^2 + dvy^2) + dvz^2);  WW = sum m_i m_j (the product of two floats in
 *             double is exact).  The flag word `series` selects which are computed; count is always on, and a call
 *             without velocity series loads no velocity per pair.
 * Exact sums. The format of the profiles (above) with a window that is known before the pair pass, so that the pairs are
 *             walked once.  vmax = the largest of |vx|, |vy|, |vz| over the finite particles of the range, ev = the
 *             smallest integer with vmax < 2^ev (-1074 where vmax is 0), Eu = ev + 2.  The windows: E(U1) = Eu,
 *             E(U2) = E(T2) = 2 Eu, E(U3) = E(A3) = 3 Eu.  They bound every term: |u| <= |dv| <= sqrt(3) 2^(ev + 1)
 *             = 0.87 2^Eu, and the margin covers the roundings.  mmax and em likewise over |m|, E(WW) = 2 em.
 *             fixed(t) = sign(t) floor(|t| 2^(64 - E)), made by shifting the mantissa; a 128-bit two's-complement sum per
 *             bin and series; one rounding to the nearest double at the end (ties to even, subnormals included), built
 *             bit by bit as sx_profile_from_fixed does.  A term is below 2^64 in magnitude (a product that underflows
 *             may round up to 2^E itself, i.e. to 2^64: still far inside the 128 bits) and a bin holds fewer than 2^62
 *             pairs (n <= 2^31 - 1), so no sum can overflow whatever the input.  A sum differs from the real sum of
 *             its rounded terms by less than count 2^(E - 64).
 * Result.     Only integers are added: the result does not depend on launch shape, atomics order or run, and with an id
 *             column not on the order of storage either.
 * One rank.   Pairs across a rank boundary need halos of width r_max: sx_sim_twopoint refuses a sim with a communicator
 *             of more than one rank. */
#define SX_TP_U1 1u
#define SX_TP_U2 2u
#define SX_TP_U3 4u
#define SX_TP_A3 8u
#define SX_TP_T2 16u
#define SX_TP_WW 32u
#define SX_TP_VEL (SX_TP_U1 | SX_TP_U2 | SX_TP_U3 | SX_TP_A3 | SX_TP_T2)
#define SX_TP_ALL (SX_TP_VEL | SX_TP_WW)
#define SX_TP_MAX_BINS 256
typedef struct sx_twopoint
{
    const double* edges;  /* host, nbins + 1 */
    uint32_t      nbins;
    uint32_t      series; /* SX_TP_* flags; count is always computed */
    uint32_t      stride, phase;
} sx_twopoint;
/*! every pointer nullable (then not written); device pointers for sx_twopoint_compute, host pointers for
 *  sx_sim_twopoint.  A series whose flag is not set is not written either. */
typedef struct sx_twopoint_result
{
    uint64_t* count;                     /* [nbins] */
    double *  U1, *U2, *U3, *A3, *T2, *WW; /* [nbins] each */
    uint64_t* totals;                    /* [3]: targets, nonfinite, coincident */
} sx_twopoint_result;
/*! host only, needs no GPU: SX_OK, or SX_ERR_ARG with the reason and its figures in sx_last_error(NULL) (per thread).
 *  Refused, each with its own message: a NULL argument, nbins of 0 or above 256, an edge that is not finite, edges that
 *  do not ascend strictly, a negative first edge, stride == 0, phase >= stride, unknown series flags, r_max above a third
 *  of the box length on a periodic axis (three distinct cells and an unambiguous minimum image need it). */
int sx_twopoint_check(const sx_twopoint* tp, const sx_box* box);
/*! host only: the cell grid a call on n particles uses: the rule of sx_fof_grid with r_max = edges[nbins] in the place
 *  of the linking length.  SX_ERR_ARG: whatever sx_twopoint_check refuses. */
int sx_twopoint_grid(const sx_twopoint* tp, const sx_box* box, uint64_t n, uint32_t dims[3]);
/*! the series of the particles [first, last) of f (x, y, z, vx, vy, vz; m for WW: no other column is read, so the
 *  gravity-only layout serves) into the device arrays of deviceOut.  id: device, f->n entries, or NULL.  Stages: the cell
 *  grid of sx_fof (keys, count, sort); one pass over the particles for the windows, nonfinite and targets (integer maxima
 *  on exponent keys) and a gather into the sorted order; the pair kernel (a lane per sorted particle, every unordered
 *  pair visited once from its earlier member, the bins as 128-bit integers in block-private LDS, 64-bit integer atomics
 *  only); the conversion.  The scratch lives in the context under the tags twopoint.*, about 90 bytes per particle.
 *  SX_ERR_ARG: whatever sx_twopoint_check refuses, missing columns, first > last or last > f->n, more than 2^31 - 1
 *  particles.  Synchronises. */
int sx_twopoint_compute(sx_ctx* ctx, const sx_fields* f, const sx_box* box, uint32_t first, uint32_t last,
                        const uint64_t* id, const sx_twopoint* tp, const sx_twopoint_result* deviceOut);
/*! the context's last call: {pairs tested (separations evaluated: both members finite, one a target, the later one in
 *  the 27 cells round the earlier), pairs binned, targets, nonfinite, coincident}; SX_ERR_ARG before the first */
int sx_twopoint_stats(sx_ctx* ctx, uint64_t out[5]);
/*! measurement: with on != 0 the following calls time their stages with HIP events; sx_twopoint_times: {grid,
 *  windows + gather, pairs, conversion} in ms of the last call */
int sx_set_twopoint_timing(sx_ctx* ctx, int on);
int sx_twopoint_times(sx_ctx* ctx, double out[4]);
/*! host only, the number format of the exact sums (shift 64): *E = the smallest integer with max |t| < 2^E over the n
 *  terms (-1074 where every term is 0); SX_ERR_ARG for a term that is not finite */
int sx_twopoint_window(const double* t, size_t n, int32_t* E);
/*! host only: sign(t[i]) floor(|t[i]| 2^(64 - E)) as two words, lohi[2 i] the low and lohi[2 i + 1] the high half of the
 *  128-bit two's-complement integer; SX_ERR_ARG for a term that is not finite or above 2^E in magnitude */
int sx_twopoint_to_fixed(const double* t, size_t n, int32_t E, uint64_t* lohi);
/*! host only: acc (low, high) += the n integers of lohi, modulo 2^128 */
int sx_twopoint_add_fixed(uint64_t acc[2], const uint64_t* lohi, size_t n);
/*! host only: *out = the double nearest (ties to even) to acc * 2^(E - 64), subnormals included */
int sx_twopoint_from_fixed(const uint64_t acc[2], int32_t E, double* out);

/* ---- self-gravity: ryoanji MultipoleHolder seam (multipole_holder.cuh:40-66, gravity_wrapper.hpp:104-174) ----- */
/*! expansion centers (mass centers, {x,y,z,mac^2}, numNodes x 4 doubles; mac = 2 max(node size)/theta + |com-geo|,
 *  setMac, source_center.hpp:130-143) and Cartesian quadrupoles (numNodes x 8 floats, Cqi order,
 *  cartesian_qpole.hpp:59-126) of every node of the linked octree over f's particles (single rank: the focus tree
 *  of syncGrav is the local tree).  Bit-identical to the reference CPU upsweep. */
int sx_gravity_upsweep(sx_ctx* ctx, const sx_fields* f, const sx_tree* tree, float theta, double* centers,
                       float* multipoles);
/*! Barnes-Hut traversal for targets [g->firstBody, g->lastBody) (computeGravity, traversal_cpu.hpp:166-230: groups
 *  of 16, vector MAC, quadrupole M2P, P2P softened by h_i + h_j): adds G * acc to f->ax, ay, az and returns the
 *  potential energy 0.5 sum G m phi in *egrav.  With explicit groups (g->groupStart, e.g. the active rungs of
 *  ve-bdt, MultipoleHolder::traverse(gravGroup, ...), ve_hydro_bdt.hpp:279-285) only the targets of those groups are
 *  traversed (the others keep their acceleration) and egrav sums over them.  Open boxes (a periodic box:
 *  sx_gravity_traverse_pbc). */
int sx_gravity_traverse(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_tree* tree, const sx_box* box,
                        const double* centers, const float* multipoles, float G, double* egrav);
/*! the walk over the periodic images (MultipoleHolder::compute(..., numShells, box, ...), gravity_wrapper.hpp:139-141;
 *  traversal_cpu.hpp:200-216 / traversal.cuh:485-513): as sx_gravity_traverse, the targets shifted by every
 *  (ix Lx, iy Ly, iz Lz), |ix|, |iy|, |iz| <= numShells (0..4); numShells 0 = the box alone.  Periodic self-gravity
 *  is this walk with numShells = EwaldSettings::numReplicaShells followed by sx_gravity_ewald.  No interaction
 *  counting on this path. */
int sx_gravity_traverse_pbc(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_tree* tree,
                            const sx_box* box, const double* centers, const float* multipoles, float G, int numShells,
                            double* egrav);

/*! ryoanji::directSum (interface/multipole_holder.cuh:72-74, nbody/direct.cuh:52-123, traversal_cpu.hpp:234-270): the
 *  O(N^2) sum for the targets of g over the sources [0, f->n), the softened P2P of kernel.hpp:514-535 (h_i + h_j formed
 *  in float), every target shifted by (ix Lx, iy Ly, iz Lz), |ix|, |iy|, |iz| <= numShells (0..4; iz outermost, ix
 *  innermost).  Reads x, y, z, m, h.  With numShells > 0 the lengths come from box->lim (any shape: no Ewald sum here);
 *  box may be NULL when numShells == 0.  The view is that of sx_stir: [firstBody, lastBody) or explicit groups of any
 *  size >= 0; particles outside it are not touched.
 *  Output: f->ax, ay, az (all three, or none) get (float)((double)ax + G acc), as the walk's; out4 (device, 4 doubles
 *  per particle of f, or NULL) gets {G m_i phi_i, G ax, G ay, G az} of the reference's CPU function, un-accumulated;
 *  *egrav = 0.5 sum_i G m_i phi_i over the view (0 for an empty view).  At least one of the two outputs is required.
 *  sx_set_exact(1): double throughout, 1/sqrt, the reference's order of operations; sources ascending inside a source
 *  split, splits combined ascending -- with one split the additions per target are those of the CPU loop.  Default:
 *  packed float with rsqrt on sources relative to their tile's first source, folded into double once per 256-source
 *  tile.
 *  The grid is (blocks of 256 targets) x (source splits); a second kernel adds the splits in ascending order, so the
 *  result is deterministic for a given split count.  Automatic rule: splits = clamp(ceil(16 * 256 / targetBlocks), 1,
 *  sourceTiles), sourceTiles = ceil(n / 256), targetBlocks = ceil(targets / 256): sixteen workgroups per CU;
 *  sx_set_direct_splits(ctx, k) overrides it (0: automatic; a k beyond sourceTiles is clamped).  Runs on the context
 *  stream; synchronises to return *egrav.
 *  SX_ERR_ARG: numShells out of range, x/y/z/m/h missing, no output, a view reaching beyond f->n. */
int sx_gravity_direct(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_box* box, int numShells, float G,
                      double* out4, double* egrav);
int sx_set_direct_splits(sx_ctx* ctx, uint32_t splits);

/*! ryoanji::EwaldSettings (nbody/ewald.h:15-22); the reference's defaults: 1, 2.6, 2.8, 2.0, 3e-3 */
typedef struct
{
    int    numReplicaShells; /* image shells the tree walk covered (their -erf correction) */
    double lCut;             /* real-space cutoff (box lengths) */
    double hCut;             /* k-space cutoff, ceil(hCut) <= 3 */
    double alphaScale;       /* Ewald splitting alpha = alphaScale / L */
    double smallRScaleFactor;
} sx_ewald_settings;

/*! Ewald correction of periodic self-gravity (computeGravityEwaldGpu, ryoanji/interface/ewald.cu:60-95, i.e.
 *  computeGravityEwald, nbody/ewald.hpp:380-413) for the targets of g: the root's expansion (centers[0..2],
 *  multipoles[0..7], device arrays of sx_gravity_upsweep) summed over the images in real space and in k space; adds
 *  G * correction to f->ax, ay, az and 0.5 G sum m phi to *egrav.  SX_ERR_ARG unless the box is cubic and
 *  ceil(hCut) <= 3.  Only targets of g (explicit groups: their targets) are corrected.  The correction completes a
 *  walk over numReplicaShells image shells (sx_gravity_traverse_pbc). */
int sx_gravity_ewald(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_box* box, const double* centers,
                     const float* multipoles, float G, const sx_ewald_settings* settings, double* egrav);

/* ---- multi-GPU transport (replaces the reference's MPI calls, see sph-exa_amd/csrc/sx_comm.hpp) ---------- */
typedef struct sx_comm sx_comm;
/*! host-staged collectives supplied by the caller (e.g. torch.distributed gloo): buffers are host memory,
 *  send/recv segments contiguous in rank order; return 0 on success. op: 0 = u32 sum, 1 = f64 min, 2 = f64 sum,
 *  3 = u32 min, 4 = u32 max. */
typedef int (*sx_alltoallv_cb)(void* user, const void* sendHost, const uint64_t* sendBytes, void* recvHost,
                               const uint64_t* recvBytes);
typedef int (*sx_allreduce_cb)(void* user, void* bufHost, uint64_t count, int op);
/*! RCCL unique id (128 bytes) created on rank 0 and broadcast by the caller's control plane */
int  sx_comm_unique_id(void* id128);
/*! RCCL communicator over the node's GPUs (the calling process must have selected its device via sx_create) */
int  sx_comm_create_rccl(sx_comm** comm, int rank, int size, const void* id128);
int  sx_comm_create_host(sx_comm** comm, int rank, int size, sx_alltoallv_cb a2a, sx_allreduce_cb ar, void* user);
void sx_comm_destroy(sx_comm* comm);
/*! the transport's two operations on device buffers, as the domain sync uses them (sx_comm.hpp): every rank sends
 *  sendBytes[q] bytes from send + sendOff[q] to rank q and receives recvBytes[q] at recv + recvOff[q] (MPI_Alltoallv
 *  shape of the reference's Isend/Recv halo and particle exchange, halos/exchange_halos_gpu.cuh:51-143,
 *  domain/domaindecomp_mpi_gpu.cuh:86-171), enqueued on hipStream; and an in-place allreduce of count elements, op 0 =
 *  u32 sum (tree counts, update_mpi_gpu.cuh:75), 1 = f64 min (time-step, ts_global.hpp:106), 2 = f64 sum
 *  (conserved quantities, conserved_quantities.hpp:163-165).  Results are complete when the stream is. */
int  sx_comm_alltoallv(sx_comm* comm, const void* send, const uint64_t* sendBytes, const uint64_t* sendOff, void* recv,
                       const uint64_t* recvBytes, const uint64_t* recvOff, void* hipStream);
int  sx_comm_allreduce(sx_comm* comm, void* dev, uint64_t count, int op, void* hipStream);

/* ---- block time-step host bookkeeping (HydroVeBdtProp::computeRungs, ve_hydro_bdt.hpp:292-331) ---------------- */
/*! sph::Timestep (sph/timestep.h:38-48) */
typedef struct sx_timestep
{
    float    nextDt, elapsedDt, totDt;
    int      numRungs, substep;
    uint32_t rungRanges[SX_MAX_RUNGS + 1];
    float    dt_m1[SX_MAX_RUNGS], dt_drift[SX_MAX_RUNGS];
} sx_timestep;
/*! rungTimestep (ts_rungs.hpp:132-145): sorts groupDt[0, numGroups) ascending in place with groupIndices (the group
 *  of each sorted entry), min-reduces {groupDt[0], groupDt[(uint32_t)(0.4f * numGroups)]} over comm's ranks
 *  (comm NULL: this rank only), numRungs = min(int(log2(dt40 / dtMin)) + 1, SX_MAX_RUNGS), rungRanges by lower bound
 *  of 2^r dtMin, nextDt = min(maxDt, dtMin), totDt = nextDt 2^numRungs; elapsedDt, substep, dt_m1, dt_drift = 0.
 *  numGroups >= 1.  Synchronises the context stream (the results are host values, as in the reference). */
int sx_rung_timestep(sx_ctx* ctx, float* groupDt, uint32_t* groupIndices, uint32_t numGroups, float maxDt,
                     sx_comm* comm, sx_timestep* out);
/*! minimumGroupDt (ts_rungs.hpp:147-157) for the numGroups active groups of substep ts->substep: sorts them as
 *  above, groupIndices[numGroups, ts->rungRanges[SX_MAX_RUNGS]) = the identity; *dt = min(dtMin, (totDt -
 *  elapsedDt) / substeps left), rungRanges over all SX_MAX_RUNGS rungs.  numGroups may be 0 (a rank without active
 *  groups on a substep: it contributes nothing to the min over the ranks).  Synchronises the context stream. */
int sx_minimum_group_dt(sx_ctx* ctx, const sx_timestep* ts, float* groupDt, uint32_t* groupIndices, uint32_t numGroups,
                        sx_comm* comm, float* dt, uint32_t* rungRanges);
/*! extractGroupGpu (groups.hpp:31-48): group k of the output = group indices[first + k] of grp, k < last - first
 *  (device arrays outStart/outEnd; the view they form has firstBody = lastBody = 0) */
int sx_extract_groups(sx_ctx* ctx, const sx_groups* grp, const uint32_t* indices, uint32_t first, uint32_t last,
                      uint32_t* outStart, uint32_t* outEnd);

/* ---- host-side decisions of the SFC domain decomposition (sph-exa_amd/csrc/sx_domain.cpp) -------------- */
/*! equal-count SFC splitters from the all-reduced histogram of 2^histBits key bins (bin = key >> (63-histBits)):
 *  rank q owns keys [split[q], split[q+1]); split has nranks+1 entries.  Replaces cstone::makeSfcAssignment,
 *  domain/include/cstone/domain/domaindecomp.hpp:120. */
int sx_domain_splitters(const uint32_t* hist, uint32_t histBits, int nranks, uint64_t* split);
/*! halo receive layout [lower ranks | numLocal locals | higher ranks] (domain.hpp:196-244): recvOff[q] for each
 *  peer (0 for rank itself), out = {first local, last local, total}. */
int sx_domain_halo_layout(const uint64_t* recvCounts, int nranks, int rank, uint64_t numLocal, uint64_t* recvOff,
                          uint64_t out[3]);

/* ---- device-resident simulation: one HydroVeProp step per call ----------------------------------------- */
typedef struct sx_sim sx_sim;
/*! a simulation of up to capacity particles in box.  Self-gravity (p->g != 0) in a periodic box: the walk over one
 *  image shell + the Ewald correction with the reference's EwaldSettings defaults (gravity_wrapper.hpp:135-157), one
 *  rank, VE or std propagator (SX_ERR_ARG for ve-bdt; several ranks: at sx_sim_set_comm).
 *  Propagator 3 (NbodyProp, gravity only): SX_ERR_ARG when g == 0; a periodic box under the same rule (all three axes
 *  periodic, cubic).  Only x y z h m, v, x_m1, id (with their sort buffers), keys, the sort order and ax ay az are
 *  allocated.  Under it sx_sim_set_state ignores temp, du_m1 and alpha (NULL allowed), sx_sim_fields leaves every field
 *  that is not kept NULL, sx_sim_scalars reads INFINITY for minDtCourant and minDtRho, the hydro stages of
 *  sx_sim_stage_times read 0, the internal energy of sx_sim_conserved / sx_sim_observe is 0, and sx_sim_kernel_times has
 *  an eighth entry, nbodyIntegrate.  Refused with SX_ERR_ARG and a reason in sx_last_error: sx_sim_init_sedov,
 *  sx_sim_set_turbulence, sx_sim_set_skin, sx_sim_rebuild_lists, sx_sim_export_neighbors, sx_sim_last_stats,
 *  sx_sim_timestep, sx_sim_set_timestep and the observables that need kx or c (SX_OBS_MACH_RMS, SX_OBS_KH_GROWTH,
 *  SX_OBS_WIND_BUBBLE). */
int    sx_sim_create(sx_sim** sim, sx_ctx* ctx, size_t capacity, const sx_params* p, const sx_box* box,
                     uint32_t bucketSize);
void   sx_sim_destroy(sx_sim* sim);
int    sx_sim_init_sedov(sx_sim* sim, uint32_t side);
/*! distribute the step over a communicator: SFC assignment by a global key histogram (all ranks equal counts),
 *  particle exchange, halo discovery and the reference's five halo exchanges per step
 *  (ve_hydro.hpp:150-186), global time-step min.  rank/size come from the communicator. */
int    sx_sim_set_comm(sx_sim* sim, sx_comm* comm);
/*! this rank's share of a Sedov lattice of side^3 particles (contiguous lattice-index slab; the first step's
 *  sync moves particles to their SFC owner) */
int    sx_sim_init_sedov_rank(sx_sim* sim, uint32_t side, int rank, int size);
/*! overlap of the halo exchanges with the pair kernels (default on; several ranks, fast kernels): each exchange of
 *  ve_hydro.hpp:150-186 runs on a communication stream while the clusters whose neighbor union holds no halo are
 *  computed, the rest after it lands.  Results are bitwise identical with it off. */
int    sx_sim_set_overlap(sx_sim* sim, int on);
/*! interior and boundary cluster counts of the last distributed step (0, 0 without overlap) */
int    sx_sim_overlap_stats(sx_sim* sim, uint32_t out[2]);
/*! bytes the sim holds in its arenas: out[0] device memory, out[1] pinned host memory */
int    sx_sim_memory(sx_sim* sim, uint64_t out[2]);
/*! local particle range [first,last) and total (with halos) of the last step */
int    sx_sim_layout(sx_sim* sim, uint64_t out[4]);
/*! upload a host state (conserved fields, length n) */
int    sx_sim_set_state(sx_sim* sim, size_t n, const double* x, const double* y, const double* z, const float* h,
                        const float* m, const double* temp, const float* vx, const float* vy, const float* vz,
                        const float* x_m1, const float* y_m1, const float* z_m1, const float* du_m1,
                        const float* alpha, const uint64_t* id, double minDt, double minDt_m1);
/*! device field pointers of the current state (valid until the next step).  After a one-rank VE or std step the
 *  keys are those of the updated coordinates (computed by the position update for the next sync), not of the
 *  step's tree; writing x, y or z through these pointers between steps is not supported on that path */
int    sx_sim_fields(sx_sim* sim, sx_fields* f, uint64_t** id);
size_t sx_sim_size(sx_sim* sim);
/*! one VE step; the time-step scalars stay on the device (no host sync unless stats are requested) */
int    sx_sim_step(sx_sim* sim);
/*! minDt, minDt_m1, ttot, minDtCourant, minDtRho (synchronises) */
int    sx_sim_scalars(sx_sim* sim, double out[6]);
/*! per-stage device time of the last step (ms) measured with HIP events, names in stage order */
int    sx_sim_stage_times(sx_sim* sim, float* ms, int cap, const char** names);
int    sx_sim_last_stats(sx_sim* sim, sx_nbstats* stats);
/*! multi-rank self-gravity of the last step: {gravity halos received, remote level-6 cells used as far-field
 *  multipoles, remote cells in total} (zeros on one rank) */
int    sx_sim_gravity_stats(sx_sim* sim, uint64_t out[3]);
/*! count the self-gravity interactions of the following steps (the reference's BhStats, collected only when its
 *  stats are requested, traversal.cuh:346-357): off by default -- the counting traversal is a separate kernel
 *  instantiation, ~8 % slower.  SX_ERR_ARG without gravity. */
int    sx_sim_set_gravity_counting(sx_sim* sim, int enable);
/*! self-gravity interactions of the last VE step on this rank (zeros when counting was off), counted per target as
 *  the reference's BhStats (nbody/traversal.cuh:346-357, 614-620): {sumP2P (source particles), sumM2P (multipole
 *  nodes)}; synchronises.  SX_ERR_ARG without gravity. */
int    sx_sim_gravity_interactions(sx_sim* sim, uint64_t out[2]);
/*! force-error check of the walk: arms the next step (numTargets = 0 disarms).  Right after its gravity walk, on the
 *  same positions, tree, centers and multipoles, the armed step takes every s-th of its own 64-particle target blocks
 *  (about numTargets targets), runs the walk once more for them into zeroed scratch accelerations and sx_gravity_direct
 *  for the same view into a second scratch (periodic box: both with the walk's shell count, both without the Ewald
 *  correction), and copies the two samples to the host.  Nothing the step computes changes.  One rank, VE and std
 *  propagators: SX_ERR_ARG (sx_last_error has the reason) without gravity, with a communicator, under ve-bdt. */
int    sx_sim_set_gravity_check(sx_sim* sim, uint32_t numTargets);
/*! the last armed step's sample: {targets, mean, median, 99th percentile, max of |a_walk - a_direct| / |a_direct|,
 *  sqrt(sum |a_walk - a_direct|^2 / sum |a_direct|^2)}.  SX_ERR_ARG when no armed step has run. */
int    sx_sim_gravity_check(sx_sim* sim, double out[6]);
/*! computeConservedQuantities (conserved_quantities.hpp:110-179) of the current state, summed over the ranks of the
 *  communicator: {ecin, eint, egrav, etot, |linmom|, |angmom|, totalNeighbors, linmom x y z, angmom x y z}
 *  (egrav of the last step; synchronises) */
int    sx_sim_conserved(sx_sim* sim, double out[13]);
/*! select the observable of sx_sim_observe (observablesFactory, factory.hpp:46-69; the default is
 *  SX_OBS_TIME_ENERGY).  For SX_OBS_WIND_BUBBLE the settings carry the reference's three inputs and the driver forms
 *  the derived ones as wind_bubble_fraction.hpp:114-131 and factory.hpp:59-63 do: rhoBubble = rhoInt, tempWind = uExt
 *  (the driver stores uExt * idealGasCv(muiConst, gamma)), initialMass = rSphere (stored: 4/3 pi rSphere^3 rhoInt);
 *  particleMass <= 0 takes the mass of the rank's first particle at each sx_sim_observe, the reference's m[0].
 *  settings NULL: the defaults.  Every propagator and any number of ranks; SX_ERR_ARG for SX_OBS_KH_GROWTH and
 *  SX_OBS_WIND_BUBBLE with the std propagator, which has no kx (the reference's reason, time_energy_growth.hpp:88-91,
 *  wind_bubble_fraction.hpp:125-129). */
int    sx_sim_set_observable(sx_sim* sim, int kind, const sx_obs_settings* settings);
/*! the row IObservables::computeAndWrite writes to constants.txt for the current state (one fused pass over the local
 *  particles, the last step's egrav and the local particle count added, ONE sum over the communicator, finalised on
 *  the host; synchronises).  Columns, in the reference's order:
 *    iteration ttot minDt etot ecin eint egrav |linmom| |angmom|          SX_OBS_TIME_ENERGY (time_energies.hpp)
 *    ... machRms                                                         SX_OBS_MACH_RMS (turbulence_mach_rms.hpp:112)
 *    ... khGrowthRate                                                    SX_OBS_KH_GROWTH (time_energy_growth.hpp:137)
 *    ... bubbleFraction ttot/0.0937                                      SX_OBS_WIND_BUBBLE (wind_bubble_fraction.hpp:141)
 *    iteration ttot minDt etot ecin eint egrav h+ hx d2xx d2yy d2zz d2xy d2xz d2yz   SX_OBS_GRAV_WAVES (no momenta,
 *                                                                        gravitational_waves.hpp:122-123)
 *  iteration counts the completed steps (sx_sim_set_iteration after a restart).  *ncols receives the number of columns;
 *  SX_ERR_ARG when cap is smaller.  Nothing is computed on steps after which this is not called. */
int    sx_sim_observe(sx_sim* sim, double* row, int cap, int* ncols);
/*! the iteration a restarted run continues from (the restart file's "iteration" attribute) */
int    sx_sim_set_iteration(sx_sim* sim, uint64_t iteration);
/*! the column a of sx_sim_render */
#define SX_MAP_FIELD_NONE 0
#define SX_MAP_FIELD_TEMP 1
#define SX_MAP_FIELD_P 2
#define SX_MAP_FIELD_C 3
#define SX_MAP_FIELD_VX 4
#define SX_MAP_FIELD_VY 5
#define SX_MAP_FIELD_VZ 6
#define SX_MAP_FIELD_DIVV 7
#define SX_MAP_FIELD_CURLV 8
#define SX_MAP_FIELD_ALPHA 9
#define SX_MAP_FIELD_H 10
/*! sx_map_render of this rank's local particles in their current positions, one f64-sum reduction per image over the
 *  communicator when one is set, and the images copied to the host arrays hostSum0, hostSum1 (npix[0] * npix[1] doubles
 *  each; hostSum1 is not touched for SX_MAP_FIELD_NONE and may be NULL); synchronises.  Every propagator, any number
 *  of ranks (every rank calls it and receives the whole image); under ve-bdt between any two substeps.  Nothing in
 *  sx_sim_step calls it and it changes no state.  The dependent fields (p, c, divv, curlv) are those of the last force
 *  stage: stale by the one position update that followed it.  A field the layout does not keep is refused with
 *  SX_ERR_ARG and a reason: under the gravity-only propagator everything except NONE, VX, VY, VZ, H; p under VE, which
 *  keeps p / rho only.  A refusal that only one rank meets (a tile row of its particles above the pair cap, no memory for
 *  its pairs) travels with the images through the reduction: that rank returns its code, every other rank SX_ERR_ARG,
 *  none waits for ever; a rank that cannot allocate the image buffers themselves does not take part, which is fatal for
 *  the communicator.  The image buffers and the pair scratch are allocated by the first render and counted by
 *  sx_sim_memory from then on.  sx_sim_map_stats: sx_map_stats of the sim's last render (this rank's figures). */
int    sx_sim_render(sx_sim* sim, const sx_map* map, int field, double* hostSum0, double* hostSum1);
int    sx_sim_map_stats(sx_sim* sim, uint64_t out[4]);
int    sx_sim_set_map_pair_cap(sx_sim* sim, uint64_t pairs);
/*! sx_spectrum_compute of the current state over all ranks: each rank deposits its locals, one f64-sum reduction
 *  (sx_comm_allreduce op 2) runs over the meshes when a communicator is set -- one leading double counts the ranks whose
 *  own deposit was refused, so nobody waits in the reduction for a rank that left early: that rank returns its code,
 *  every other rank SX_ERR_ARG --, every rank then transforms and sums redundantly, and power (numShells doubles) and
 *  modes (numShells u64, nullable) reach the host arrays through a pinned buffer; synchronises.  SX_SPEC_VELOCITY reads
 *  vx, vy, vz (field is ignored); SX_SPEC_SCALAR takes field, a code of sx_sim_render (SX_MAP_FIELD_NONE: the mesh
 *  density itself); a field the layout does not keep is refused as sx_sim_render refuses it.  Every propagator; under
 *  ve-bdt between any two substeps.  Nothing in sx_sim_step calls it and it changes no state.  The buffers live in the
 *  sim's arena, are allocated by the first call and counted by sx_sim_memory from then on (what a 256^3 call keeps:
 *  see sx_spectrum_compute).  sx_sim_spectrum_stats: sx_spectrum_stats of the sim's last call (this rank's figures);
 *  sx_sim_set_spectrum_pair_cap: sx_set_spectrum_pair_cap. */
int    sx_sim_spectrum(sx_sim* sim, const sx_spectrum* spec, int field, double* hostPower, uint64_t* hostModes);
int    sx_sim_spectrum_stats(sx_sim* sim, uint64_t out[4]);
int    sx_sim_set_spectrum_pair_cap(sx_sim* sim, uint64_t pairs);
/*! sx_profile_compute of the current state over all ranks: each rank reads its locals; the windows agree through one
 *  u32-max reduction (sx_comm_allreduce op 4) of 14 words whatever the specification -- the first word counts a rank
 *  that must refuse (whatever sx_profile_check refuses for it, a quantity its layout does not keep), so nobody waits in
 *  a reduction for a rank that left early: that rank returns its code, every other rank SX_ERR_ARG --; the integer
 *  accumulators and counts travel as 16-bit limbs through one u32-sum reduction (exact for up to 2^16 ranks) and the
 *  carries are propagated afterwards; min and max through one f64-min reduction (max as -min(-x)).  Every rank receives
 *  the whole result, bit-identical to the profile of the merged particles on one rank, in the host arrays of hostOut
 *  through a pinned buffer; synchronises.  gamma and muiConst are the sim's; rho is the rho column under the std
 *  propagator and (kx * m) / xm otherwise.  Every propagator (under the gravity-only one only VEL, VRAD and H exist);
 *  under ve-bdt between any two substeps.  Nothing in sx_sim_step calls it and it changes no state.  The dependent
 *  fields (kx, xm, rho, c, divv, curlv) are those of the last force stage.  The buffers live in the sim's arena under
 *  the tags prof.*, are allocated by the first call and counted by sx_sim_memory from then on.  More than 2^31 - 1
 *  particles over all ranks are refused.  sx_sim_profile_stats: sx_profile_stats of the sim's last call (this rank's
 *  particles; nonfinite over all ranks). */
int    sx_sim_profile(sx_sim* sim, const sx_profile* prof, sx_profile_result* hostOut);
int    sx_sim_profile_stats(sx_sim* sim, uint64_t out[4]);
/*! sx_fof_compute of the locals of the current state with the sim's id column, into the host arrays of hostOut; labels
 *  in the sim's current particle order (pair them with the id field).  Reads x, y, z, m, vx, vy, vz and id only: every
 *  propagator, the gravity-only one included; nothing in sx_sim_step calls it and it changes no field and no scalar.
 *  The buffers live in the sim's arena under the tags fof.*, are allocated by the first call and counted by
 *  sx_sim_memory from then on.  A sim with a communicator of more than one rank is refused on every rank before any
 *  collective (SX_ERR_ARG): groups that cross rank boundaries are not merged.  sx_sim_fof_stats: sx_fof_stats of the
 *  sim's last call. */
int    sx_sim_fof(sx_sim* sim, const sx_fof* fof, const sx_fof_result* hostOut);
int    sx_sim_fof_stats(sx_sim* sim, uint64_t out[4]);
/*! sx_halo_compute of the locals of the current state with the sim's id column, into the host arrays of hostOut (the
 *  properties through a pinned buffer); synchronises.  G, muiConst, gamma and std are taken from the sim's parameters
 *  (those fields of `halo` are ignored); rhoMin, flags and the rest from `halo`.  Every propagator: the gravity-only
 *  layout serves with rhoMin <= 0 and without the thermal energy, and is refused with a reason otherwise.  Nothing in
 *  sx_sim_step calls it and it changes no field and no scalar.  The buffers live in the sim's arena under the tags fof.*
 *  (shared with sx_sim_fof) and halo.*, are allocated by the first call and counted by sx_sim_memory from then on.  A
 *  communicator of more than one rank is refused on every rank before any collective.  sx_sim_halos_stats:
 *  sx_halo_stats of the sim's last call. */
int    sx_sim_halos(sx_sim* sim, const sx_halo* halo, const sx_halo_result* hostOut);
int    sx_sim_halos_stats(sx_sim* sim, uint64_t out[4]);
/*! sx_twopoint_compute of the locals of the current state with the sim's id column, into the host arrays of hostOut
 *  through a pinned buffer; synchronises.  Reads x, y, z, vx, vy, vz, m and id only: every propagator, the gravity-only
 *  one included, under ve-bdt between any two substeps; nothing in sx_sim_step calls it and it changes no field and no
 *  scalar.  The buffers live in the sim's arena under the tags twopoint.*, are allocated by the first call and counted
 *  by sx_sim_memory from then on.  A sim with a communicator of more than one rank is refused on every rank before any
 *  collective (SX_ERR_ARG): pairs across rank boundaries are not counted.  sx_sim_twopoint_stats: sx_twopoint_stats of
 *  the sim's last call. */
int    sx_sim_twopoint(sx_sim* sim, const sx_twopoint* tp, const sx_twopoint_result* hostOut);
int    sx_sim_twopoint_stats(sx_sim* sim, uint64_t out[5]);
/*! device time (ms) of each hot kernel alone in the last step (HIP events on the launch stream, bracketing just the
 *  launch): findNeighbors, xmass, veDefGradh, iadDivvCurlv, avSwitches, momentumEnergy */
int    sx_sim_kernel_times(sx_sim* sim, float* ms, int cap, const char** names);
/*! propagator 2 (ve-bdt): the Timestep after the last substep (sph::Timestep, timestep_ of HydroVeBdtProp,
 *  ve_hydro_bdt.hpp:380).  A substep with activeRung(substep, numRungs) == 0 starts a new hierarchy (full sync,
 *  every particle active); the others drift the inactive rungs and compute the active ones (partial sync: halo
 *  x,y,z,h refreshed, order, tree and halo lists kept).  SX_ERR_ARG for the other propagators. */
int    sx_sim_timestep(sx_sim* sim, sx_timestep* ts);
/*! the simulation time d.ttot (a restart's "time" attribute, particles_data.hpp:170-190; set_state starts at 0) */
int    sx_sim_set_time(sx_sim* sim, double ttot);
/*! propagator 2: restart state after sx_sim_set_state (HydroVeBdtProp::load, ve_hydro_bdt.hpp:155-168): the Timestep
 *  saved with the file and the `rung` of each set_state particle (host array, set_state order; NULL keeps rung 0).
 *  SX_ERR_ARG unless activeRung(ts->substep, ts->numRungs) == 0: restart files exist only at hierarchy boundaries
 *  (the reference writes them only when isSynced(), sphexa.cpp:165). */
int    sx_sim_set_timestep(sx_sim* sim, const sx_timestep* ts, const uint8_t* rung);
/*! neighbor lists behind a skin (VE or std propagator, one rank or several, with or without self-gravity -- not with
 *  periodic self-gravity; sph-exa_amd/csrc/sx_skin.hpp):
 *  replaces the per-step Domain::sync + findNeighborsSph of ve_hydro.hpp:140-149 by a filter of the last build's
 *  lists within 2h(1 + factor) while no particle can have entered a target's 2h sphere since that build; stale
 *  clusters are rebuilt at once.  Neighbor sets, h and nc stay those of findNeighbors; between builds the particle
 *  order and tree are kept.  factor 0 restores a sync + search every step; a full sync + build of every cluster
 *  happens at least every maxReuse steps.  Default: factor 0.05, maxReuse 24.  Takes effect at the next step (full
 *  build). */
int    sx_sim_set_skin(sx_sim* sim, float factor, int maxReuse);
/*! the next step does a full sync and builds every cluster's skin (e.g. after writing a restart file, so a run that
 *  continues and one restarted from the file take identical steps) */
int    sx_sim_rebuild_lists(sx_sim* sim);
/*! {full builds, steps served by the filter, clusters rebuilt as stale, clusters sent to the exact search, stale
 *  clusters of the last step, of them exact, skin-list capacity per target, steps searched without the skin while
 *  backing off, the current skin's s and the next build's s (both in millionths), reuse steps redone from a full sync
 *  (clusters stale again after their rebuild), clusters of reuse steps whose targets all kept the hits of the last
 *  step, so the filter kept their exact lists in place, of them frozen: no skin entry could have crossed its target's
 *  2h sphere, so their skin lists were not walked, clusters whose exact search ran concurrently with the rebuild of
 *  the other stale clusters}.  A skin that does not outlast
 *  two steps makes the next build's twice as wide (up to 0.16), then the steps back off to a plain search. */
int    sx_sim_skin_stats(sx_sim* sim, uint64_t out[14]);
/*! the last step's neighbor lists of the local particles as global indices into the state of sx_sim_fields, row-major
 *  out[(i - first) * ngmax + k] for k < min(nc - 1, ngmax) (device buffer of (last - first) * ngmax words; the lists
 *  the step's pair kernels used, cstone::findNeighbors' layout) */
int    sx_sim_export_neighbors(sx_sim* sim, uint32_t* out);

/* ---- turbulence stirring (TurbVeProp, main/src/propagator/turb_ve.hpp:98-136, over sph/include/sph/hydro_turb/) ----
 * An Ornstein-Uhlenbeck process per Fourier mode drives a large-scale acceleration field.  The host object sx_turb is
 * sph::TurbulenceData (turbulence_data.hpp:46-184) without its device vectors; everything is double and follows the
 * reference's order of operations, the generator is std::mt19937 with std::normal_distribution<double> /
 * std::uniform_real_distribution<double>, so seeds give the reference's sequences. */
/*! the entries of TurbulenceConstants() (main/src/init/turbulence_init.hpp:48-71) that TurbulenceData::initModes
 *  reads (turbulence_data.hpp:150-183); numDim is 3 */
typedef struct sx_turb_settings
{
    double   solWeight;      /* 0.5 */
    uint64_t stMaxModes;     /* 100000 */
    double   Lbox;           /* 1.0 */
    double   stEnergyPrefac; /* 5.0e-3 */
    double   stMachVelocity; /* 0.3 */
    double   epsilon;        /* 1e-15 */
    uint64_t rngSeed;        /* 251299 */
    uint32_t stSpectForm;    /* 1: parabola; 0: band; 2: power law, randomly sampled angles */
    double   powerLawExp;    /* 5/3 */
    double   anglesExp;      /* 2.0 */
} sx_turb_settings;
typedef struct sx_turb sx_turb;
/*! the defaults above */
int sx_turb_default_settings(sx_turb_settings* s);
/*! TurbulenceData's constructor: initModes (turbulence_data.hpp:150-183) with createStirringModes
 *  (create_modes.hpp:59-244, spectral forms 0, 1, 2, its mode cap included), then the 6 numModes OU phases drawn with
 *  mean 0 and standard deviation `variance`.  SX_ERR_ARG for a spectral form > 2, stMaxModes == 0 or Lbox,
 *  stMachVelocity <= 0. */
int  sx_turb_create(sx_turb** turb, const sx_turb_settings* s);
void sx_turb_destroy(sx_turb* turb);
/*! what TurbulenceData::loadOrStore saves (turbulence_data.hpp:90-120).  sx_turb_get_scalars: {variance, decayTime,
 *  solWeight, solWeightNorm}; sx_turb_get_arrays: modes (3 numModes), amplitudes (numModes), phases (6 numModes), each
 *  nullable; sx_turb_get_rng: the generator in the text form of operator<< on std::mt19937 (the reference's
 *  rngEngineState), NUL-terminated into buf of cap bytes, returns the length without the NUL (call with cap 0 for the
 *  size).  sx_turb_set_state restores all of it (rng NULL: the generator is kept); SX_ERR_ARG for text that is not a
 *  generator state. */
uint64_t sx_turb_num_modes(const sx_turb* turb);
int      sx_turb_get_scalars(const sx_turb* turb, double out[4]);
int      sx_turb_get_arrays(const sx_turb* turb, double* modes, double* amplitudes, double* phases);
int64_t  sx_turb_get_rng(const sx_turb* turb, char* buf, size_t cap);
int      sx_turb_set_state(sx_turb* turb, const double scalars[4], uint64_t numModes, const double* modes,
                           const double* amplitudes, const double* phases, const char* rng);
/*! largest |i|, |j|, |k| of the mode table on its own lattice w0 (i, j, k): w0 is the largest (smallest nonzero
 *  |component|) / n, n <= 16, that every component is a multiple of -- 2 pi / Lbox for the tables sx_turb_create makes;
 *  taken from the table, not from the settings, so it holds after sx_turb_set_state.  -1 when there is no such w0. */
int sx_turb_max_index(const sx_turb* turb);
/*! the largest lattice index the fast variant of sx_stir keeps in registers (tables beyond it run the exact one) */
int sx_turb_fast_limit(void);
/*! updateNoise (driver.hpp:80-92): one OU step of every phase over dt with 6 numModes fresh normal draws */
int sx_turb_update_noise(sx_turb* turb, double dt);
/*! computePhases (phases.hpp:47-72): the projected phases, 3 numModes each, from the current OU phases */
int sx_turb_compute_phases(const sx_turb* turb, double* phasesReal, double* phasesImag);
/*! computeStirringGpu<double, float, double> (stirring.hpp:123-126, :44-121) with the projected phases of turb's
 *  current OU phases: adds solWeightNorm sum_m amplitude_m (Re_m cos(k_m x) - Im_m sin(k_m x)) to f->ax, ay, az of the
 *  view's particles: [firstBody, lastBody), or the explicit groups when groupStart is set (particles outside the view
 *  are not touched).  sx_set_exact(1): the reference's loop (per-mode cos/sin in double, float accumulators, no
 *  contraction).  Otherwise, for tables on an integer lattice with indices up to sx_turb_fast_limit(): three sincos
 *  per particle (angles reduced in double), harmonics by recurrence and the sum in float; other tables run the exact
 *  loop.
 *  Synchronises (as driveTurbulence does, driver.hpp:120). */
int sx_stir(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, const sx_turb* turb);
/*! the same with the reference's arguments: device arrays modes, phaseReal, phaseImag (3 numModes each), amplitudes
 *  (numModes) */
int sx_stir_device(sx_ctx* ctx, const sx_groups* g, const sx_fields* f, uint64_t numModes, const double* modes,
                   const double* phaseReal, const double* phaseImag, const double* amplitudes, double solWeightNorm);
/*! from now on every step of sim stirs as TurbVeProp::computeForces (turb_ve.hpp:114-119): after momentum/energy and
 *  self-gravity, before the time-step and the position update, driveTurbulence (driver.hpp:102-128) with the minDt
 *  current at that point.  The host draws the step's normals, the OU update and the projection run on the device (no
 *  host synchronisation).  SX_ERR_ARG (sx_last_error has the reason) for the std and ve-bdt propagators and for a sim
 *  with a communicator; sx_sim_set_comm on a stirred sim is refused likewise. */
int sx_sim_set_turbulence(sx_sim* sim, const sx_turb_settings* s);
/*! the sim's turbulence state, owned by the sim (valid until the sim is destroyed): synchronises and brings the OU
 *  phases back from the device.  SX_ERR_ARG without sx_sim_set_turbulence. */
int sx_sim_turbulence(sx_sim* sim, sx_turb** turb);
/*! restart: sx_turb_set_state on the sim's turbulence state, uploaded to the device */
int sx_sim_set_turbulence_state(sx_sim* sim, const double scalars[4], uint64_t numModes, const double* modes,
                                const double* amplitudes, const double* phases, const char* rng);
/*! device time (ms, HIP events) of the last step's {noise advance, stirring kernel}; both are part of the
 *  UpdateQuantities stage of sx_sim_stage_times */
int sx_sim_turbulence_times(sx_sim* sim, float out[2]);

/* ---- optically thin radiative cooling (no line-by-line counterpart: the reference's std-cooling propagator,
 * main/src/propagator/std_hydro_grackle.hpp:155-226, drives GRACKLE on the host; its time-step criterion ct_crit is
 * physics/cooling/include/cooling/cooler.hpp:103, cooler.cpp:79-83) ----
 * A tabulated cooling function in code units, integrated exactly over the step for every particle (Townsend 2009,
 * ApJS 181, 391) on the device.  Model: dT/dt = -rho L(T) / cv at the rho of the step, L(T) = L_k (T / T_k)^alpha_k on
 * [T_k, T_k+1]; the last segment's law continues above T_N; below T_1, the temperature floor, L = 0.  T is the sim's
 * temp column (u / cv), so du/dt = -rho L. */
#define SX_COOLING_MAX_NODES 256
typedef struct sx_cooling sx_cooling;

/*! host only, needs no GPU.  n nodes T_1 < ... < T_n, 2 <= n <= SX_COOLING_MAX_NODES, with values lambda_k > 0.
 *  Builds, in double, alpha_k = ln(lambda_k+1 / lambda_k) / ln(T_k+1 / T_k) and Townsend's temporal evolution function
 *  Y_k = (lambda_n / T_n) int_{T_k}^{T_n} dT / L(T): dimensionless, Y_n = 0, growing as T falls.  SX_ERR_ARG for n out of
 *  range, T not strictly increasing, an entry that is not finite or not positive, and a table whose Y does not come
 *  out finite and strictly decreasing in k (exponents or ratios beyond double). */
int      sx_cooling_create(sx_cooling** out, const double* T, const double* lambda, uint32_t n);
void     sx_cooling_destroy(sx_cooling* c);
uint32_t sx_cooling_num_nodes(const sx_cooling* c);
/*! the table: n entries each, every pointer nullable; alpha[n - 1] repeats alpha[n - 2], the law above T_n */
int      sx_cooling_get_table(const sx_cooling* c, double* T, double* lambda, double* alpha, double* Y);
/*! the arithmetic of the kernels on the host, operation by operation (libm's log, exp, log1p, expm1 in place of the
 *  device's): L(T), and T after s = rho dt / cv */
double   sx_cooling_rate_host(const sx_cooling* c, double T);
double   sx_cooling_integrate_host(const sx_cooling* c, double T0, double s);
/*! *minTc = min over i < n of cv temp_i / (rho_i L(temp_i)), +inf where L = 0 everywhere (and for n == 0).  rho, temp:
 *  device arrays (float, double); minTc: host.  Synchronises. */
int sx_cooling_time(sx_ctx* ctx, const sx_cooling* c, uint32_t n, const float* rho, const double* temp, double cv,
                    double* minTc);
/*! temp_i <- the exact solution after dt at rho_i, in place (device arrays; rho, m float, temp double).  stats (host):
 *  {sum_i m_i cv (T_old - T_new), the energy radiated; particles that ended on the floor T_1; particles on or above
 *  the floor before the call}.  The sum is taken in a fixed order (block partials in a buffer whose length depends on
 *  n alone, folded by one block; no floating-point atomics): the same bits on every run of the same input.  Exact
 *  whatever rounding does: T_new <= T_old; T_new >= T_1 where T_old >= T_1; a particle with T_old < T_1 is left
 *  unchanged; dt == 0 leaves every bit unchanged.  Synchronises. */
int sx_cool(sx_ctx* ctx, const sx_cooling* c, uint32_t n, const float* rho, const float* m, double* temp, double cv,
            double dt, double stats[3]);
/*! sx_set_cooling_timing(1): sx_cool and sx_cooling_time record HIP events round their kernels (the table is uploaded
 *  only when it differs from the last call's and lies outside them).  sx_cooling_times: device ms of the kernels of the
 *  last {sx_cool, sx_cooling_time}; zeros with the timing off. */
int sx_set_cooling_timing(sx_ctx* ctx, int on);
int sx_cooling_times(sx_ctx* ctx, double out[2]);
/*! from now on every VE or std step of sim cools: an operator-split update of temp directly after the position and
 *  energy update, with the rho of the step's force stage (VE: (kx m) / xm) and the step's minDt read on the device; du
 *  and du_m1 stay purely hydrodynamic.  Before the step's time-step, ct_crit min_i t_cool,i of the locals joins the
 *  rank's time-step candidates (ct_crit <= 0: no limiter).  The table is copied: c stays the caller's.  c NULL: off
 *  again, and the sim steps as one that never cooled.  Any number of ranks.  SX_ERR_ARG (sx_last_error has the reason)
 *  for the ve-bdt and gravity-only propagators. */
int sx_sim_set_cooling(sx_sim* sim, const sx_cooling* c, double ct_crit);
/*! this rank's {ct_crit min t_cool of the last step (+inf without the limiter), energy radiated in the last step,
 *  energy radiated since sx_sim_set_state / sx_sim_init_sedov / sx_sim_set_cooling_radiated, particles on the floor
 *  after the last step}; the caller sums over ranks.  Synchronises.  SX_ERR_ARG without sx_sim_set_cooling. */
int sx_sim_cooling_stats(sx_sim* sim, double out[4]);
/*! restart: the running total of the energy radiated */
int sx_sim_set_cooling_radiated(sx_sim* sim, double erad);
/*! device time (ms, HIP events; the step timer's own slots) of the last step's {cooling-time kernel, cooling kernel};
 *  both are part of the UpdateQuantities stage of sx_sim_stage_times */
int sx_sim_cooling_times(sx_sim* sim, float out[2]);

#ifdef __cplusplus
}
#endif

#endif
