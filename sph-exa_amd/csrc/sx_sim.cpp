/*! @file sx_sim.cpp
 * @brief Device-resident VE time step (sx_sim_*): HydroVeProp::computeForces + integrate
 *        (main/src/propagator/ve_hydro.hpp:132-218), on one GPU or SFC-decomposed over several.
 *
 * Step = sync -> neighbor search with h-nc iteration -> XMass -> [halo xm] -> VeDefGradh -> EOS
 *        -> [halo v,prho,c,kx] -> IAD+divv/curlv -> [halo c_ij,divv] -> AV switches -> [halo alpha]
 *        -> momentum/energy -> [cooling time] -> global time-step min -> positions/energy -> [cooling] -> h update.
 *
 * This file: the sx_sim_* C API and the step, stepImpl, an orchestrator over named stages (searchStage, forcesStd /
 * forcesVe, gravityStage, integrateStage, finishStep).  The sync is sx_sim_domain.cpp, self-gravity
 * sx_sim_gravity.cpp, the skin-list driver sx_sim_skin.cpp; sx_sim_internal.hpp declares what they share.
 *
 * sync, one GPU: Hilbert keys, radix sort, reorder of every conserved field, converged tree.
 * sync, P GPUs (replaces cstone::Domain::sync, domain.hpp:196-244, with an MI355X-first design):
 *   1. sort local particles by key;
 *   2. global key histogram (2^18 bins, allreduce) -> equal-count SFC splitters, identical on every rank
 *      (the reference's global cornerstone tree + MPI_Allreduce of counts, update_mpi_gpu.cuh:75);
 *   3. particle exchange to the SFC owner (alltoallv of 80-byte AoS records; skipped when nothing moves);
 *   4. halo discovery: each rank publishes request boxes = AABB of every 2048-particle SFC chunk grown by
 *      2*hmax(chunk)*margin; every rank marks (wave-cooperative tree traversal of its own tree) the particles
 *      inside each peer's boxes -> send lists; halos land in place, [halos of lower ranks | local | higher];
 *   5. the combined array is key-sorted by construction -> one tree over locals + halos, built from the halos' keys
 *      (sent first, 8 B each) while their coordinates, h and m are exchanged on the communication stream.
 *   After the h iteration the request margin is checked; if some particle outgrew it, discovery is redone.
 * Halo exchanges carry exactly the reference's fields (ve_hydro.hpp:150-186): x,y,z,h,m at setup, then xm,
 * then vx,vy,vz,prho,c,kx, then c11..c33,divv, then alpha.
 */
#include "sx_sim_internal.hpp"

using namespace sx;
using namespace sx::sim;

namespace
{

DevBox toDevBox(const sx_box* b)
{
    DevBox d{};
    for (int k = 0; k < 6; ++k)
        d.lim[k] = b->lim[k];
    for (int k = 0; k < 3; ++k)
    {
        d.l[k]   = b->lim[2 * k + 1] - b->lim[2 * k];
        d.il[k]  = 1.0 / (b->lim[2 * k + 1] - b->lim[2 * k]);
        d.pbc[k] = b->bnd[k] == 1;
        d.fbc[k] = b->bnd[k] == 2;
        d.anyPbc |= d.pbc[k];
    }
    return d;
}

// ---- time step --------------------------------------------------------------------------------------------

//! rhoTimestep (ts_global.hpp:72-94) and the rank-local part of computeTimestep (:97-112)
//! useRho = 0: the std propagator, which never sets minDtRho (std_hydro.hpp:170-178: stays INFINITY)
//! useCourant = 0: the gravity-only propagator, which sets minDtCourant = INFINITY (nbody.hpp:158)
__global__ void dtCandidateKernel(Scalars* s, double Krho, double maxDtIncrease, double g, double eps, double etaAcc,
                                  int useRho, int useCourant)
{
    unsigned u = s->maxDivvU;
    u          = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    float maxDivv   = __uint_as_float(u);
    s->minDtRho     = useRho ? Krho / (double)fabsf(maxDivv) : INFINITY;
    s->minDtCourant = useCourant ? (double)s->courant : INFINITY;
    double minDtAcc = INFINITY;
    if (g != 0.0) minDtAcc = etaAcc * sqrt(eps / sqrt(__longlong_as_double((long long)s->maxAccSqBits)));
    double m       = INFINITY;
    // minDtCool: the cooling-time criterion of a sim that cools (sx_sim_set_cooling), INFINITY otherwise
    double cand[5] = {minDtAcc, s->minDtCourant, s->minDtRho, maxDtIncrease * s->minDt, s->minDtCool};
    for (int k = 0; k < 5; ++k)
        m = cand[k] < m ? cand[k] : m;
    s->dtCand = m;
}

//! after the (MPI_Allreduce-equivalent) global min: ttot, minDt_m1, minDt
__global__ void dtApplyKernel(Scalars* s)
{
    double m = s->dtCand;
    s->ttot += m;
    s->minDt_m1 = s->minDt;
    s->minDt    = m;
}

__global__ void resetScalarsKernel(Scalars* s)
{
    s->courant      = 1e10f;
    s->maxDivvU     = 0;
    s->egrav        = 0.0;
    s->maxAccSqBits = 0;
    s->gravErr      = 0;
}

// ---- initial conditions -----------------------------------------------------------------------------------

//! Sedov lattice (grid.hpp:102-132, sedov_init.hpp:48-96); particles [lfirst, lfirst + n) of the z-major lattice
__global__ void sedovInitKernel(uint32_t side, size_t lfirst, size_t n, double* x, double* y, double* z, float* h,
                                float* m, double* temp, float* vx, float* vy, float* vz, float* xm1, float* ym1,
                                float* zm1, float* dum1, float* alpha, uint64_t* id, float hInit, float mPart,
                                double ener0, double width2, double u0, float cv)
{
    size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= n) return;
    size_t       li = lfirst + t;
    const double r = 0.5, step = (2. * r) / side, r_ini = -r + 0.5 * step;
    size_t       i = li / ((size_t)side * side), j = (li / side) % side, k = li % side;
    double       lz = r_ini + (i * step), ly = r_ini + (j * step), lx = r_ini + (k * step);
    x[t] = lx;
    y[t] = ly;
    z[t] = lz;
    h[t] = hInit;
    m[t] = mPart;
    double r2 = lx * lx + ly * ly + lz * lz;
    double ui = ener0 * exp(-(r2 / width2)) + u0;
    temp[t]   = ui / (double)cv;
    vx[t] = vy[t] = vz[t] = 0.f;
    xm1[t] = ym1[t] = zm1[t] = 0.f;
    dum1[t]  = 0.f;
    alpha[t] = 0.05f;
    id[t]    = li;
}

} // namespace

namespace sx::sim
{

void allocFields(sx_sim* s, size_t cap)
{
    auto& a  = s->mem;
    // the gravity-only propagator (NbodyProp, nbody.hpp:74-77) keeps x y z h m, v, x_m1, a and keys: no thermal
    // field, no hydro dependent field, no packed records and no neighbor lists are requested for it
    const bool hydro = s->p.propagator != 3;
    s->x     = a.get<double>("x", cap);
    s->y     = a.get<double>("y", cap);
    s->z     = a.get<double>("z", cap);
    s->temp  = hydro ? a.get<double>("temp", cap) : nullptr;
    s->h     = a.get<float>("h", cap);
    s->m     = a.get<float>("m", cap);
    s->vx    = a.get<float>("vx", cap);
    s->vy    = a.get<float>("vy", cap);
    s->vz    = a.get<float>("vz", cap);
    s->xm1   = a.get<float>("x_m1", cap);
    s->ym1   = a.get<float>("y_m1", cap);
    s->zm1   = a.get<float>("z_m1", cap);
    s->dum1  = hydro ? a.get<float>("du_m1", cap) : nullptr;
    s->alpha = hydro ? a.get<float>("alpha", cap) : nullptr;
    s->id    = a.get<uint64_t>("id", cap);
    s->keys  = a.get<uint64_t>("keys", cap);
    s->order = a.get<uint32_t>("order", cap);
    s->nc    = hydro ? a.get<uint32_t>("nc", cap) : nullptr;
    s->xm    = hydro ? a.get<float>("xm", cap) : nullptr;
    s->kx    = hydro ? a.get<float>("kx", cap) : nullptr;
    s->gradh = hydro ? a.get<float>("gradh", cap) : nullptr;
    s->prho  = hydro ? a.get<float>("prho", cap) : nullptr;
    s->c     = hydro ? a.get<float>("c", cap) : nullptr;
    s->divv  = hydro ? a.get<float>("divv", cap) : nullptr;
    s->curlv = hydro ? a.get<float>("curlv", cap) : nullptr;
    s->c11   = hydro ? a.get<float>("c11", cap) : nullptr;
    s->c12   = hydro ? a.get<float>("c12", cap) : nullptr;
    s->c13   = hydro ? a.get<float>("c13", cap) : nullptr;
    s->c22   = hydro ? a.get<float>("c22", cap) : nullptr;
    s->c23   = hydro ? a.get<float>("c23", cap) : nullptr;
    s->c33   = hydro ? a.get<float>("c33", cap) : nullptr;
    s->ax    = a.get<float>("ax", cap);
    s->ay    = a.get<float>("ay", cap);
    s->az    = a.get<float>("az", cap);
    s->du    = hydro ? a.get<double>("du", cap) : nullptr;
    if (hydro && s->p.avClean)
    {
        // GradVFields, allocated only with avClean (ve_hydro.hpp:80-85)
        s->dV[0] = a.get<float>("dV11", cap);
        s->dV[1] = a.get<float>("dV12", cap);
        s->dV[2] = a.get<float>("dV13", cap);
        s->dV[3] = a.get<float>("dV22", cap);
        s->dV[4] = a.get<float>("dV23", cap);
        s->dV[5] = a.get<float>("dV33", cap);
    }
    if (s->p.propagator == 1)
    {
        s->rho  = a.get<float>("rho", cap);
        s->pres = a.get<float>("p", cap);
    }
    s->rx    = hydro ? a.get<RecX>("rx", cap) : nullptr;
    s->rv    = hydro ? a.get<RecV>("rv", cap) : nullptr;
    s->rt    = hydro ? a.get<RecT>("rt", cap) : nullptr;
    s->rs    = reinterpret_cast<RecS*>(s->rt);
    s->rc    = hydro ? a.get<RecC>("rc", cap) : nullptr;
    // a field the propagator does not keep has no spare either: the sort, the particle exchange and the halo moves
    // go over this list
    auto spare = [&](auto*& field, const char* tag) {
        using T = std::remove_reference_t<decltype(*field)>;
        if (!field) return;
        s->spares.push_back(
            {reinterpret_cast<void**>(&field), a.get<T>(std::string(tag) + ".alt", cap), (int)sizeof(T)});
    };
    spare(s->x, "x");
    spare(s->y, "y");
    spare(s->z, "z");
    spare(s->h, "h");
    spare(s->m, "m");
    spare(s->temp, "temp");
    spare(s->vx, "vx");
    spare(s->vy, "vy");
    spare(s->vz, "vz");
    spare(s->xm1, "x_m1");
    spare(s->ym1, "y_m1");
    spare(s->zm1, "z_m1");
    spare(s->dum1, "du_m1");
    spare(s->alpha, "alpha");
    spare(s->id, "id");
    if (s->p.propagator == 2)
    {
        s->rung = a.get<uint8_t>("rung", cap);
        spare(s->rung, "rung");
    }
    if (hydro) s->nb.reserve(a, 0, (uint32_t)cap, s->p.ngmax, true);
    s->stats      = a.get<uint32_t>("stats", kStatsWords);
    s->statsHost  = a.pinned<uint32_t>("statsHost", kStatsWords);
    s->clsHost    = a.pinned<uint32_t>("ovl.countHost", 2);
    if (s->statsHost) std::fill(s->statsHost, s->statsHost + kStatsWords, 0u);
    s->sc         = a.get<Scalars>("scalars", 1);
    s->scHost     = a.pinned<Scalars>("scalarsHost", 1);
}

PairArgs simPairArgs(sx_sim* s)
{
    PairArgs a = pairArgsCommon((uint32_t)s->first, (uint32_t)s->last, simFields(s), s->nb, s->p, s->dbox);
    a.lb       = s->skin.lb; // the step's second set of lists (skin filter), or none
    a.rx       = s->rx;
    a.rv       = s->rv;
    a.rt       = s->rt;
    a.rc       = s->rc;
    a.rs       = s->rs;
    a.wh       = sx_ctx_table_internal(s->ctx, 0);
    a.whd      = sx_ctx_table_internal(s->ctx, 1);
    a.minDt    = &s->sc->courant;
    a.blockDt  = s->mem.get<float>("pair.blockdt", std::max<size_t>(1, (s->last - s->first + kCluster - 1) / kCluster));
    a.dtPtr    = &s->sc->minDt;
    a.avClean  = s->p.avClean ? 1 : 0;
    return a;
}

/*! halo exchange of `fields` followed by the pair kernel `launch`, which needs the exchanged halo values.  Without
 *  overlap: exchange, pack(0, n), launch over all clusters.  With overlap: the exchange runs on commStream after the
 *  producer's kernels (event); meanwhile the compute stream packs the locals' records and runs the interior
 *  clusters; then it waits for the exchange, packs the halos' records and runs the boundary clusters.  Every cluster
 *  is computed exactly as in the serial order, so results are bitwise identical. */
template<class Pack, class Launch>
int exchangeThen(sx_sim* s, const HydroLaunch& H, std::initializer_list<std::pair<void*, int>> fields, Pack&& pack,
                 Launch&& launch, PairArgs pa, hipStream_t st)
{
    if (!overlapping(s, H))
    {
        if (int e = haloExchange(s, fields, st)) return e;
        pack(size_t(0), s->n);
        launch(pa);
        return SX_OK;
    }
    SIM_HIP(hipEventRecord(s->evProd, st));
    SIM_HIP(hipStreamWaitEvent(s->commStream, s->evProd, 0));
    if (int e = haloExchange(s, fields, s->commStream)) return e;
    SIM_HIP(hipEventRecord(s->evComm, s->commStream));
    pack(s->first, s->last);
    const uint32_t nc = (uint32_t)((s->last - s->first + kCluster - 1) / kCluster);
    pa.clusterList    = s->clsList;
    pa.listCount      = s->nInterior;
    launch(pa);
    SIM_HIP(hipStreamWaitEvent(st, s->evComm, 0));
    pack(size_t(0), s->first);
    pack(s->last, s->n);
    pa.clusterList = s->clsList + nc;
    pa.listCount   = s->nBoundary;
    launch(pa);
    return SX_OK;
}

// ---- turbulence stirring (sx_turb.hpp) ----------------------------------------------------------------------------

void turbDestroy(sx::turb::SimTurb* T)
{
    if (!T) return;
    for (auto& e : T->ringEv)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : T->ev)
        if (e) (void)hipEventDestroy(e);
    sx_turb_destroy(T->host);
    delete T;
}

//! the host turbulence state onto the device (sx_sim_set_turbulence, a restart): buffers for its mode count, the mode
//! table, the OU phases and, for a table on the lattice, the slot of each mode.  Synchronous.
int turbUpload(sx_sim* s)
{
    using namespace sx::turb;
    SimTurb&       T = *s->turb;
    const sx_turb& h = *T.host;
    const size_t   M = h.numModes;
    hipStream_t    st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
    SIM_HIP(hipStreamSynchronize(st));
    T.phases     = s->mem.get<double>("turb.phases", 6 * M);
    T.modes      = s->mem.get<double>("turb.modes", 3 * M);
    T.amplitudes = s->mem.get<double>("turb.amplitudes", M);
    T.phasesReal = s->mem.get<double>("turb.phasesReal", 3 * M);
    T.phasesImag = s->mem.get<double>("turb.phasesImag", 3 * M);
    T.normals    = s->mem.get<double>("turb.normals", 6 * M);
    T.table      = s->mem.get<float>("turb.table", kSlots * kSlotCoefs);
    T.slot       = s->mem.get<int32_t>("turb.slot", M);
    bool ok      = T.phases && T.modes && T.amplitudes && T.phasesReal && T.phasesImag && T.normals && T.table && T.slot;
    for (int k = 0; k < SimTurb::kRing; ++k)
    {
        T.ring[k]     = s->mem.pinned<double>("turb.ring" + std::to_string(k), 6 * M);
        T.ringBusy[k] = false;
        ok            = ok && T.ring[k];
    }
    if (!ok) return SX_ERR_NOMEM;
    T.lat = latticeOf(M, h.modes.data());
    if (M)
    {
        SIM_HIP(hipMemcpy(T.phases, h.phases.data(), 6 * M * 8, hipMemcpyHostToDevice));
        SIM_HIP(hipMemcpy(T.modes, h.modes.data(), 3 * M * 8, hipMemcpyHostToDevice));
        SIM_HIP(hipMemcpy(T.amplitudes, h.amplitudes.data(), M * 8, hipMemcpyHostToDevice));
        if (T.lat.ok) SIM_HIP(hipMemcpy(T.slot, T.lat.slot.data(), M * 4, hipMemcpyHostToDevice));
    }
    return SX_OK;
}

/*! driveTurbulence (driver.hpp:102-128) inside the step: the host draws the step's normals (they do not depend on dt)
 *  and queues them; one small kernel reads minDt from the device scalars -- the previous step's, or set_state's, as
 *  d.minDt at driver.hpp:106 -- and does updateNoise, computePhases and the coefficient table; then the stirring kernel
 *  over the locals.  Nothing here waits for work of this step.  The one wait is the ring slot's event, four steps old;
 *  as long as sx_sim_step ends in a stream synchronise it has always completed and a single buffer would do -- the ring
 *  is what keeps this function correct should that final synchronise go. */
int turbStep(sx_sim* s, hipStream_t st)
{
    using namespace sx::turb;
    SimTurb&     T = *s->turb;
    sx_turb&     h = *T.host;
    const size_t M = h.numModes;
    SIM_HIP(hipEventRecord(T.ev[0], st));
    if (M)
    {
        const int k = T.next;
        // the copy queued from this slot kRing steps ago (see above)
        if (T.ringBusy[k]) SIM_HIP(hipEventSynchronize(T.ringEv[k]));
        drawNormals(h.gen, T.ring[k], 6 * M);
        SIM_HIP(hipMemcpyAsync(T.normals, T.ring[k], 6 * M * 8, hipMemcpyHostToDevice, st));
        SIM_HIP(hipEventRecord(T.ringEv[k], st));
        T.ringBusy[k] = true;
        T.next        = (k + 1) % SimTurb::kRing;
        NoiseArgs na{};
        na.dt       = &s->sc->minDt;
        na.variance = h.variance, na.decayTime = h.decayTime, na.solWeight = h.solWeight;
        na.solWeightNorm = h.solWeightNorm;
        na.numModes      = M;
        na.normals = T.normals, na.phases = T.phases, na.modes = T.modes, na.amplitudes = T.amplitudes;
        na.phasesReal = T.phasesReal, na.phasesImag = T.phasesImag;
        na.slot  = T.lat.ok ? T.slot : nullptr;
        na.table = T.table;
        SIM_HIP(advanceNoise(na, st));
    }
    SIM_HIP(hipEventRecord(T.ev[1], st));
    if (M && s->last > s->first)
    {
        StirArgs a{};
        a.first = (uint32_t)s->first, a.last = (uint32_t)s->last;
        a.numGroups = (a.last - a.first + 63) / 64;
        a.x = s->x, a.y = s->y, a.z = s->z, a.ax = s->ax, a.ay = s->ay, a.az = s->az;
        a.numModes = M, a.solWeightNorm = h.solWeightNorm;
        a.modes = T.modes, a.phasesReal = T.phasesReal, a.phasesImag = T.phasesImag, a.amplitudes = T.amplitudes;
        a.table = T.table, a.present = T.lat.present, a.w0 = T.lat.w0;
        const bool exact = sx_ctx_exact_internal(s->ctx) || !T.lat.ok;
        SIM_HIP(exact ? stirExact(a, st) : stirFast(a, st));
    }
    SIM_HIP(hipEventRecord(T.ev[2], st));
    if (s->p.g != 0.0)
    {
        // accelerationTimestep takes the stirred accelerations (computeForces ends with the stirring)
        SIM_HIP(hipMemsetAsync(&s->sc->maxAccSqBits, 0, sizeof(unsigned long long), st));
        maxAccSq(s, st);
    }
    return SX_OK;
}

// ---- radiative cooling (sx_cool.hpp) --------------------------------------------------------------------------------

//! rho of the step's force stage: the std propagator's column, (kx m) / xm under VE
sx::cool::Density coolDensity(const sx_sim* s)
{
    const size_t f = s->first;
    if (s->p.propagator == 1) return {s->rho + f, nullptr, nullptr, nullptr};
    return {nullptr, s->kx + f, s->xm + f, s->m + f};
}

/*! the cooling-time criterion (cooler.cpp:79-83: ct_crit times the shortest cooling time) of the locals' temp and this
 *  step's rho into Scalars::minDtCool, where dtCandidateKernel reads it.  Without the limiter minDtCool stays INFINITY
 *  (freshScalars, sx_sim_set_cooling) and nothing is launched */
int coolTimeStage(sx_sim* s, hipStream_t st)
{
    const CoolState& C = s->cool;
    if (!C.on || !(C.ctCrit > 0.0)) return SX_OK;
    sx::cool::CoolTimeArgs a{};
    a.n = (uint32_t)(s->last - s->first), a.d = coolDensity(s), a.temp = s->temp + s->first;
    a.cv    = (double)idealGasCv(s->p.muiConst, s->p.gamma);
    a.table = C.table, a.numNodes = C.numNodes, a.minBits = C.minBits;
    SIM_HIP(s->timer.coolingBegin(Cooling::coolingTime, st));
    SIM_HIP(sx::cool::coolingTimeLaunch(a, st));
    SIM_HIP(sx::cool::scaledMin(C.minBits, C.ctCrit, &s->sc->minDtCool, st));
    SIM_HIP(s->timer.coolingEnd(Cooling::coolingTime, st));
    return SX_OK;
}

/*! the operator-split energy sink, directly after the position and energy update: temp of the locals over the step's
 *  minDt (read on the device) at the rho of this step's force stage.  A deviation from the reference, which adds
 *  (u_cooled - u) / dt to du (std_hydro_grackle.hpp:214-219) and lets the AB2 energy update extrapolate it: here du and
 *  du_m1 stay purely hydrodynamic, gas at rest follows the exact cooling curve for any dt, and AB2 cannot carry a
 *  strongly cooling particle below zero */
int coolStage(sx_sim* s, hipStream_t st)
{
    const CoolState& C = s->cool;
    if (!C.on) return SX_OK;
    sx::cool::CoolArgs a{};
    a.n = (uint32_t)(s->last - s->first), a.d = coolDensity(s), a.m = s->m + s->first, a.temp = s->temp + s->first;
    a.cv    = (double)idealGasCv(s->p.muiConst, s->p.gamma);
    a.dtPtr = &s->sc->minDt;
    a.table = C.table, a.numNodes = C.numNodes;
    a.ePart = C.ePart, a.cPart = C.cPart, a.stats = C.stats, a.total = C.stats + 3;
    SIM_HIP(s->timer.coolingBegin(Cooling::cool, st));
    SIM_HIP(sx::cool::coolLaunch(a, st));
    SIM_HIP(s->timer.coolingEnd(Cooling::cool, st));
    return SX_OK;
}

//! a new state (sx_sim_set_state, sx_sim_init_sedov): nothing radiated yet
int coolResetStats(sx_sim* s, hipStream_t st)
{
    if (s->cool.stats) SIM_HIP(hipMemsetAsync(s->cool.stats, 0, 4 * sizeof(double), st));
    return SX_OK;
}

// ---- the step's scalars (shared with the gravity-only step, sx_sim_nbody.cpp) ---------------------------------------

void resetStepScalars(sx_sim* s, hipStream_t st) { resetScalarsKernel<<<1, 1, 0, st>>>(s->sc); }

int globalTimestep(sx_sim* s, bool dist, hipStream_t st)
{
    dtCandidateKernel<<<1, 1, 0, st>>>(s->sc, s->p.Krho, s->p.maxDtIncrease, s->p.g, s->p.eps, s->p.etaAcc,
                                       s->p.propagator != 1 && s->p.propagator != 3, s->p.propagator != 3);
    if (dist) SIM_COMM(s->comm->allreduceMinF64(&s->sc->dtCand, 1, st));
    dtApplyKernel<<<1, 1, 0, st>>>(s->sc);
    return SX_OK;
}

// ---- the step: an orchestrator (stepImpl) over named stages --------------------------------------------------------

namespace
{

//! what the stages of one step share
struct StepCtx
{
    hipStream_t        st;
    const HydroLaunch& H;
    bool               dist;   // several ranks
    bool               skinOn; // the step searches through skin lists (sx_skin.hpp)
    bool               reuse;  // ... as a reuse step: order and tree of the last full build are kept, the skin lists
                               // filtered (false again when the step's search is redone from a full sync)
    const float*       powTab; // the h-update table of the step's search
};

//! the targets, counts and lists of the last search (s->nb)
NsArgs listArgs(sx_sim* s)
{
    NsArgs a{};
    a.first = (uint32_t)s->first, a.last = (uint32_t)s->last, a.ngmax = s->p.ngmax, a.nc = s->nc;
    a.setLists(s->nb);
    return a;
}

//! the step's search arguments: neighbors + h iteration on the local targets, over the step's tree
int buildSearchArgs(sx_sim* s, NsArgs& na)
{
    if (!s->nb.reserve(s->mem, (uint32_t)s->first, (uint32_t)s->last, s->p.ngmax, true)) return SX_ERR_NOMEM;
    na                = listArgs(s);
    na.numGroups      = (uint32_t)((s->last - s->first + kGroupSize - 1) / kGroupSize);
    na.ng0            = s->p.ng0;
    na.iterateH       = 1;
    na.x              = s->x;
    na.y              = s->y;
    na.z              = s->z;
    na.h              = s->h;
    na.childOffsets   = s->tree.childOffsets;
    na.internalToLeaf = s->tree.internalToLeaf;
    na.layout         = s->tree.layout;
    na.centers        = s->tree.centers;
    na.sizes          = s->tree.sizes;
    na.box            = s->dbox;
    na.margin         = quantMargin(s->dbox);
    na.stats          = s->stats;
    na.powTab         = sx_ctx_powtab_internal(s->ctx, s->p.ng0);
    na.prefilter      = 1;
    na.hSave          = s->mem.get<float>("ns.hsave", std::max<size_t>(2 * ((s->last - s->first) / kCluster + 2), s->last - s->first)); // the two redo lists
    na.policy         = &s->nsPolicy;
    na.clStats        = s->mem.get<uint4>("ns.clstats", (na.numGroups + kClusterWaves - 1) / kClusterWaves);
    na.work           = s->mem.get<uint32_t>("ns.work", 16);
    na.hitMasks       = s->mem.get<uint64_t>("ns.masks", searchScratchBytes() / sizeof(uint64_t));
    na.rxOut          = s->rx; // the locals' RecX: packed by the search itself (packXHalos below)
    na.m              = s->m;
    if (!na.hSave || !na.clStats || !na.work || !na.hitMasks) return SX_ERR_NOMEM;
    return SX_OK;
}

//! a reuse step that cannot stand (the exact search over capacity on the drifted tree; several ranks: on some rank, or
//! a sphere searched again outside the build's halo region): h as before the filter, then this step's search again
//! after a full sync + build
int skinRedoFromSync(sx_sim* s, StepCtx& c)
{
    SIM_HIP(hipMemcpyAsync(s->h + s->first, s->skinBuf.h0, (s->last - s->first) * 4, hipMemcpyDeviceToDevice, c.st));
    s->skin.resyncs++;
    if (s->skin.cleanSinceBuild < 2) skinTooThin(s->skin);
    c.reuse = false;
    return SX_OK;
}

//! the domain state of one search attempt: a reuse step keeps order and tree (several ranks: refreshes the halos);
//! else the distributed sync with the request margin (h0: the locals' h before the h iteration, restored for a retry
//! with a larger margin and saved again), or, once per step, the local sync
int syncForSearch(sx_sim* s, StepCtx& c, float* h0, bool restoreH0, double reqMargin, bool& synced)
{
    hipStream_t st = c.st;
    if (c.dist && c.reuse) return skinHaloRefresh(s, st);
    if (c.dist)
    {
        // restore pre-iteration h of the locals, then rediscover halos with a larger margin
        if (restoreH0)
            SIM_HIP(hipMemcpyAsync(s->h + s->first, h0, (s->last - s->first) * 4, hipMemcpyDeviceToDevice, st));
        if (int e = distributedSync(s, st, reqMargin)) return e;
        SIM_HIP(hipMemcpyAsync(h0, s->h + s->first, (s->last - s->first) * 4, hipMemcpyDeviceToDevice, st));
        if (c.skinOn) return skinBuildSnapshot(s, st);
    }
    else if (!c.reuse && !synced)
    {
        if (int e = localSync(s, st)) return e;
        synced = true;
    }
    return SX_OK;
}

//! one attempt's search: through the skin lists (one rank: with its bookkeeping) or plain, the statistics on their way
//! to the host.  resync: this rank's reuse step must be redone from a full sync + build (one rank: set up here, and
//! nothing more is enqueued)
int searchOnce(sx_sim* s, StepCtx& c, const NsArgs& na, SkinCounts& skc, bool& resync)
{
    hipStream_t st = c.st;
    SIM_HIP(hipMemsetAsync(s->stats, 0, kStatsWords * 4, st));
    resetScalarsKernel<<<1, 1, 0, st>>>(s->sc);
    // a repeated attempt begins the interval again; one given up below (skinRedoFromSync) never ends it
    SIM_HIP(s->timer.begin(Kernel::findNeighbors, st));
    resync = false;
    if (c.skinOn)
    {
        // the fast variant's XMass (or the std density's xmass pass) rides on the filter's final pass
        const bool fastXm = !sx_ctx_exact_internal(s->ctx);
        float*     xmOut  = fastXm ? (s->p.propagator == 1 ? s->rho : s->xm) : nullptr;
        // no RecT {xm} for the locals: VeDefGradh reads xm from the dense field and writes the records
        RecT*      rtXm   = nullptr;
        const int e = skinSearch(s, na, c.reuse, st, xmOut, rtXm, skc);
        resync      = e == kSkinResync;
        if (e && !resync) return e;
        if (!c.dist)
        {
            if (resync) return skinRedoFromSync(s, c);
            skinBookkeeping(s->skin, c.reuse, skc, skc.stale, skc.clusters);
            s->skin.stepClusters = skc.clusters;
        }
    }
    else
    {
        s->skin.xmFused   = false;
        s->skin.listsKept = false;
        s->skin.lb        = ListsB{}; // the plain search writes the primary set
        SIM_HIP(findNeighbors(na, st));
    }
    SIM_HIP(s->timer.end(Kernel::findNeighbors, st));
    SIM_HIP(hipMemcpyAsync(s->statsHost, s->stats, kStatsWords * 4, hipMemcpyDeviceToHost, st));
    if (s->evStats) SIM_HIP(hipEventRecord(s->evStats, st));
    return SX_OK;
}

/*! several ranks, after an attempt's search.  Halo sufficiency: every local particle's final h within its chunk's
 *  request margin (a build or a plain search); on a reuse step, the spheres of the clusters searched again this step
 *  (coverListKernel).  One exchange of five words carries every decision the ranks take together: [0] halo margin too
 *  small, [1] the reuse step must be redone from a full sync + build, [2] stale clusters, [3] clusters, [4] clusters
 *  whose skin would not survive another such drift (the filter's kStatSkinThin).  dec: the summed words (host) */
int exchangeDecisions(sx_sim* s, StepCtx& c, const SkinCounts& skc, bool resync, double reqMargin, uint32_t*& dec)
{
    hipStream_t st  = c.st;
    unsigned*   flg = s->dom.hflag;
    dec             = s->work.pinned<uint32_t>("dom.dech", 8);
    if (!flg || !dec) return SX_ERR_NOMEM;
    dec[0] = 0, dec[1] = resync ? 1u : 0u, dec[2] = skc.stale, dec[3] = skc.clusters, dec[4] = 0;
    SIM_HIP(hipMemcpyAsync(flg, dec, 5 * 4, hipMemcpyHostToDevice, st));
    if (!c.reuse) chunkCheck(s, reqMargin, flg, st);
    else if (int e = skinCoverCheck(s, skc, flg + 1, st)) return e;
    if (c.skinOn) SIM_HIP(hipMemcpyAsync(flg + 4, s->stats + kStatSkinThin, 4, hipMemcpyDeviceToDevice, st));
    // the retry decision must be global: a rank redoing the sync alone would deadlock the collectives
    SIM_COMM(s->comm->allreduceSumU32(flg, 5, st));
    SIM_HIP(hipMemcpyAsync(dec, flg, 5 * 4, hipMemcpyDeviceToHost, st));
    if (overlapping(s, c.H))
        if (int e = classifyClusters(s, st)) return e;
    if (int e = syncErrEnqueue(s, st)) return e;
    SIM_HIP(hipStreamSynchronize(st));
    if (syncErrFailed(s)) return SX_ERR_TRAVERSAL;
    if (overlapping(s, c.H)) s->nInterior = s->clsHost[0], s->nBoundary = s->clsHost[1];
    s->statsHost[kStatHaloShort] = dec[0];
    return SX_OK;
}

//! sync (or halo refresh) and neighbor search with h iteration, repeated while the ranks decide that the halo margin
//! was too small or that a reuse step must be redone from a full sync
int searchStage(sx_sim* s, StepCtx& c)
{
    hipStream_t st = c.st;
    // h before a reuse step's filter (its h iteration), for a search redone from a full sync (kSkinResync)
    if (c.reuse)
    {
        float* hReuse = s->skinBuf.h0 = s->mem.get<float>("skin.h0", s->cap);
        if (!hReuse) return SX_ERR_NOMEM;
        SIM_HIP(hipMemcpyAsync(hReuse, s->h + s->first, (s->last - s->first) * 4, hipMemcpyDeviceToDevice, st));
    }
    bool synced = false;
    // h before the h iteration, to redo the search if the halo margin proves too small
    float* h0     = c.dist ? s->work.get<float>("h0", s->cap) : nullptr;
    double margin = kHaloMargin;
    bool   restoreH0 = false; // a retry with a larger halo margin: the locals' h as before the last search
    SkinCounts skc{};
    for (int attempt = 0;; ++attempt)
    {
        // a skin build requests its halos within the skin radius: the build's lists see every particle within
        // 2 h (1 + s) of a target (several ranks)
        const double skinMargin = c.skinOn ? 1.0 + (double)s->skin.cur : 1.0;
        if (int e = syncForSearch(s, c, h0, restoreH0, margin * skinMargin, synced)) return e;
        if (attempt == 0) SIM_HIP(s->timer.stageEnd(Stage::sync, st));

        NsArgs na{};
        if (int e = buildSearchArgs(s, na)) return e;
        c.powTab = na.powTab;
        bool resync = false;
        if (int e = searchOnce(s, c, na, skc, resync)) return e;
        if (!c.dist)
        {
            if (resync) continue;
            break;
        }
        uint32_t* dec = nullptr;
        if (int e = exchangeDecisions(s, c, skc, resync, margin * skinMargin, dec)) return e;
        if (c.skinOn && dec[1])
        {
            // every rank restores h and redoes the step from a full sync + build
            if (int e = skinRedoFromSync(s, c)) return e;
            restoreH0 = false;
            continue;
        }
        if (dec[0])
        {
            if (attempt >= 3) return SX_ERR_NOT_CONVERGED;
            margin *= 1.5;
            restoreH0 = true;
            s->haloRetries++;
            continue;
        }
        if (c.skinOn)
        {
            skinBookkeeping(s->skin, c.reuse, skc, dec[2], dec[3]);
            s->skin.stepClusters = dec[3];
            s->skin.stepS13      = dec[4];
        }
        break;
    }
    SIM_HIP(s->timer.stageEnd(Stage::FindNeighbors, st));
    return SX_OK;
}

/*! HydroProp::computeForces (std_hydro.hpp:124-166): density, EOS, [v,rho,p,c] halos, IAD, [c_ij] halos, momentum +
 *  energy.  The times go under the VE names: density under XMass / xmass, IAD under IadDivvCurlv / iadDivvCurlv,
 *  momentumEnergySTD under MomentumEnergy / momentumEnergy. */
int forcesStd(sx_sim* s, StepCtx& c, const PairArgs& pa)
{
    hipStream_t        st = c.st;
    const HydroLaunch& H  = c.H;
    StepTimer&         T  = s->timer;
    packXHalos(s, st);
    SIM_HIP(T.begin(Kernel::xmass, st));
    PairArgs da = pa;
    da.xm       = s->rho; // computeDensity: xmass written to rho (xmass_gpu.cu:151-153)
    xmassRest(s, H, da, st);
    H.xmassToRho((uint32_t)s->first, (uint32_t)s->last, s->m, s->rho, st);
    SIM_HIP(T.end(Kernel::xmass, st));
    SIM_HIP(T.stageEnd(Stage::XMass, st));
    EosArgs ea{(uint32_t)s->first, (uint32_t)s->last, s->p.muiConst, s->p.gamma, s->temp, s->m, nullptr, nullptr,
               nullptr, nullptr, s->c, s->rho, s->pres};
    H.eosStd(ea, st);
    // the std EOS is what this propagator reports as the VeDefGradh stage (consumers read it there); the EOS and
    // AVswitches stages and the veDefGradh and avSwitches kernels are not marked and read 0
    SIM_HIP(T.stageEnd(Stage::VeDefGradh, st));
    SIM_HIP(T.begin(Kernel::iadDivvCurlv, st));
    if (int e = exchangeThen(
            s, H, {{s->vx, 4}, {s->vy, 4}, {s->vz, 4}, {s->rho, 4}, {s->pres, 4}, {s->c, 4}},
            [&](size_t a, size_t b)
            {
                packV(b - a, s->vx + a, s->vy + a, s->vz + a, s->c + a, s->rv + a, st);
                packS(b - a, s->rho + a, s->pres + a, s->rs + a, st);
            },
            [&](const PairArgs& p) { H.iadStd(p, st); }, pa, st))
        return e;
    SIM_HIP(T.end(Kernel::iadDivvCurlv, st));
    SIM_HIP(T.stageEnd(Stage::IadDivvCurlv, st));
    SIM_HIP(T.begin(Kernel::momentumEnergy, st));
    if (int e = exchangeThen(
            s, H, {{s->c11, 4}, {s->c12, 4}, {s->c13, 4}, {s->c22, 4}, {s->c23, 4}, {s->c33, 4}},
            [&](size_t a, size_t b)
            {
                packC(b - a, s->c11 + a, s->c12 + a, s->c13 + a, s->c22 + a, s->c23 + a, s->c33 + a, nullptr,
                      s->rc + a, st);
            },
            [&](const PairArgs& p) { H.momentumStd(p, st); }, pa, st))
        return e;
    SIM_HIP(T.end(Kernel::momentumEnergy, st));
    SIM_HIP(T.stageEnd(Stage::MomentumEnergy, st));
    return SX_OK;
}

//! HydroVeProp::computeForces without gravity (ve_hydro.hpp:132-190): XMass, VeDefGradh, EOS, IAD + divv/curlv, AV
//! switches, momentum + energy, each after the halo exchange of its inputs
int forcesVe(sx_sim* s, StepCtx& c, PairArgs pa)
{
    hipStream_t        st = c.st;
    const HydroLaunch& H  = c.H;
    StepTimer&         T  = s->timer;
    // ---- XMass
    packXHalos(s, st);
    // the cluster kernels write the locals' records as they produce them (PairArgs::rtOut / rcOut, EosArgs):
    // the packing passes below then cover only the halos (halo()); the exact kernels leave it to them
    // only the cluster kernels write records; they run when the lists are in the local (union) format, and
    // ngmax > 256 keeps the global format, whose gather kernels read packed records of every particle
    const bool fused = H.clusterLists && pa.localLists && !pa.active;
    auto       halo  = [&](size_t a, size_t b, auto&& fn) {
        if (!fused) return fn(a, b);
        if (a < s->first) fn(a, std::min(b, (size_t)s->first));
        if (b > s->last) fn(std::max(a, (size_t)s->last), b);
    };
    SIM_HIP(T.begin(Kernel::xmass, st));
    {
        PairArgs xa = pa;
        xa.rtOut    = fused ? s->rt : nullptr;
        xmassRest(s, H, xa, st);
    }
    SIM_HIP(T.end(Kernel::xmass, st));
    // ---- [xm] halos, VeDefGradh (overlapped: interior clusters while the halos are in flight)
    SIM_HIP(T.stageEnd(Stage::XMass, st));
    SIM_HIP(T.begin(Kernel::veDefGradh, st));
    // the cluster VeDefGradh also runs the EOS of its targets (PairArgs::eos): kx and gradh stay in registers
    PairArgs va = pa;
    if (fused)
        va.eos = EosFuse{s->temp,  (double)idealGasCv(s->p.muiConst, s->p.gamma), s->p.gamma, s->prho, s->c,
                         s->vx,    s->vy, s->vz, s->alpha, s->rv, s->rt};
    if (int e = exchangeThen(
            s, H, {{s->xm, 4}},
            [&](size_t a, size_t b)
            {
                halo(a, b, [&](size_t u, size_t v)
                     { packT(v - u, s->xm + u, nullptr, nullptr, nullptr, s->rt + u, st); });
            },
            [&](const PairArgs& p) { H.veDefGradh(p, st); }, va, st))
        return e;
    SIM_HIP(T.end(Kernel::veDefGradh, st));
    SIM_HIP(T.stageEnd(Stage::VeDefGradh, st));
    // ---- EOS (unless fused above), then the v/prho/c/kx halo exchange
    if (!fused)
    {
        EosArgs ea{(uint32_t)s->first, (uint32_t)s->last, s->p.muiConst, s->p.gamma, s->temp, s->m, s->kx,
                   s->xm, s->gradh, s->prho, s->c, nullptr, nullptr};
        H.eos(ea, st);
    }
    SIM_HIP(T.stageEnd(Stage::EOS, st));
    // ---- [v, prho, c, kx] halos, IAD + divv/curlv, rho time-step
    auto packVT = [&](size_t a, size_t b)
    {
        halo(a, b,
             [&](size_t u, size_t v)
             {
                 packV(v - u, s->vx + u, s->vy + u, s->vz + u, s->c + u, s->rv + u, st);
                 packT(v - u, s->xm + u, s->kx + u, s->prho + u, s->alpha + u, s->rt + u, st);
             });
    };
    pa.rcOut = fused ? s->rc : nullptr; // IAD writes the locals' {c_ij, divv}
    SIM_HIP(T.begin(Kernel::iadDivvCurlv, st));
    if (int e = exchangeThen(s, H, {{s->vx, 4}, {s->vy, 4}, {s->vz, 4}, {s->prho, 4}, {s->c, 4}, {s->kx, 4}},
                             packVT, [&](const PairArgs& p) { H.iadDivvCurlv(p, st); }, pa, st))
        return e;
    SIM_HIP(T.end(Kernel::iadDivvCurlv, st));
    SIM_HIP(maxFloat(s->divv, (uint32_t)s->first, (uint32_t)s->last, &s->sc->maxDivvU, st));
    SIM_HIP(T.stageEnd(Stage::IadDivvCurlv, st));
    // ---- [c_ij, divv] halos, AV switches
    SIM_HIP(T.begin(Kernel::avSwitches, st));
    if (int e = exchangeThen(
            s, H, {{s->c11, 4}, {s->c12, 4}, {s->c13, 4}, {s->c22, 4}, {s->c23, 4}, {s->c33, 4}, {s->divv, 4}},
            [&](size_t a, size_t b)
            {
                halo(a, b,
                     [&](size_t u, size_t v)
                     {
                         packC(v - u, s->c11 + u, s->c12 + u, s->c13 + u, s->c22 + u, s->c23 + u, s->c33 + u,
                               s->divv + u, s->rc + u, st, s->xm + u, s->kx + u);
                     });
            },
            [&](const PairArgs& p)
            {
                PairArgs q = p;
                q.rcOut    = nullptr;
                q.rtOut    = fused ? s->rt : nullptr; // AV writes the locals' records with the new alpha
                // the largest union of this step's search: the host waits here for the search to finish
                // (long done on the device when the kernels queued before AV still run, so nothing idles)
                if (s->evStats && hipEventSynchronize(s->evStats) == hipSuccess) q.unionMax = s->statsHost[kStatMaxUnion];
                H.avSwitches(q, st);
            },
            pa, st))
        return e;
    pa.rcOut = nullptr;
    SIM_HIP(T.end(Kernel::avSwitches, st));
    SIM_HIP(T.stageEnd(Stage::AVswitches, st));
    // ---- [alpha (+ dV)] halos, momentum + energy.  With avClean the reference exchanges dV11,dV12,dV22,
    //      dV23,dV33 + alpha (ve_hydro.hpp:182-185) and leaves the halo dV13 undefined; all six are exchanged
    //      here so the result does not depend on the decomposition
    auto packTa = [&](size_t a, size_t b)
    {
        halo(a, b, [&](size_t u, size_t v)
             { packT(v - u, s->xm + u, s->kx + u, s->prho + u, s->alpha + u, s->rt + u, st); });
    };
    auto launchMe = [&](const PairArgs& p) { H.momentumEnergy(p, st); };
    SIM_HIP(T.begin(Kernel::momentumEnergy, st));
    if (s->p.avClean)
    {
        if (int e = exchangeThen(s, H,
                                 {{s->dV[0], 4}, {s->dV[1], 4}, {s->dV[2], 4}, {s->dV[3], 4}, {s->dV[4], 4},
                                  {s->dV[5], 4}, {s->alpha, 4}},
                                 packTa, launchMe, pa, st))
            return e;
    }
    else if (int e = exchangeThen(s, H, {{s->alpha, 4}}, packTa, launchMe, pa, st)) return e;
    SIM_HIP(T.end(Kernel::momentumEnergy, st));
    SIM_HIP(T.stageEnd(Stage::MomentumEnergy, st));
    return SX_OK;
}

//! integrate: global time-step, positions (with the next sync's keys or the skin's displacements), h
int integrateStage(sx_sim* s, StepCtx& c)
{
    hipStream_t st = c.st;
    if (int e = coolTimeStage(s, st)) return e;
    if (int e = globalTimestep(s, c.dist, st)) return e;
    PosArgs qa = posArgs((uint32_t)s->first, (uint32_t)s->last, simFields(s), s->dbox, s->p.muiConst, s->p.gamma);
    qa.dtPtr   = &s->sc->minDt;
    // one rank: the next localSync's keys come from this pass (the coordinates are in registers here)
    // (not when the next step will be served by the skin filter: it does not sync; should it resync after all,
    // localSync computes the keys itself, keysFresh being false)
    const SkinState& K = s->skin;
    const bool reuseNext = c.skinOn && K.valid && !K.forceBuild && K.sinceBuild < K.maxReuse && K.backoff == 0;
    qa.keys    = (!c.dist && s->p.propagator != 2 && !reuseNext) ? s->keys : nullptr;
    if (c.skinOn && !skinParticleBuffers(s, qa, st)) return SX_ERR_NOMEM;
    c.H.positions(qa, st);
    if (int e = coolStage(s, st)) return e;
    s->keysFresh = qa.keys != nullptr;
    c.H.updateH((uint32_t)s->first, (uint32_t)s->last, s->p.ng0, s->nc, s->h, c.powTab, st);
    SIM_HIP(s->timer.stageEnd(Stage::UpdateQuantities, st));
    return SX_OK;
}

//! the end of the step: wait for it, stage and kernel times, the search statistics, the skin's "outlast two steps"
//! test, and the errors the device reported
int finishStep(sx_sim* s, const StepCtx& c)
{
    SIM_HIP(hipGetLastError());
    SIM_HIP(hipStreamSynchronize(c.st));

    s->timer.collect();
    if (s->turb)
        for (int k = 0; k < 2; ++k)
            (void)hipEventElapsedTime(&s->turb->ms[k], s->turb->ev[k], s->turb->ev[k + 1]);
    const uint32_t* sh = s->statsHost;
    if (c.skinOn && c.reuse) s->skin.keptClusters += sh[kStatKept], s->skin.frozenClusters += sh[kStatFrozen];
    s->nsPolicy.observe(sh, (uint32_t)(s->last - s->first));
    s->lastStats = nbStats(sh, s->nsPolicy.lastBuild);
    if (c.reuse && s->skin.cleanSinceBuild <= 1 && !s->skin.forceBuild)
    {
        // the first clean step after a build, but most clusters would not survive another such drift: the skin
        // cannot outlast two steps; stop using it now rather than after a stale-heavy step (several ranks: the
        // counts of all ranks, exchanged with the step's decisions)
        const double s13 = c.dist ? (double)s->skin.stepS13 : (double)sh[kStatSkinThin];
        if (s13 > s->skin.staleLimit * (double)s->skin.stepClusters) skinTooThin(s->skin);
    }
    if (sh[kStatFlags] & kFlagError)
    {
        fprintf(stderr, "sx_sim_step: neighbor search capacity exceeded (flags 0x%x: %x walk capacity -- 0x%x traversal "
                        "queue, 0x%x candidate leaves, 0x%x search regions --, %x candidate space, %x union); cluster "
                        "%d: %u candidate leaves, %u search regions\n",
                sh[kStatFlags], kFlagWalk, kFlagQueue, kFlagLeaves, kFlagRegions, kFlagCandSpace, kFlagUnion,
                (int)sh[kStatOverCluster] - 1, sh[kStatOverLeaves], sh[kStatOverRegions]);
        return SX_ERR_TRAVERSAL;
    }
    if (s->p.g != 0.0)
    {
        SIM_HIP(hipMemcpy(s->scHost, s->sc, sizeof(Scalars), hipMemcpyDeviceToHost));
        if (s->scHost->gravErr)
        {
            fprintf(stderr, "sx_sim_step: GPU traversal stack exhausted in Barnes-Hut\n");
            return SX_ERR_TRAVERSAL;
        }
    }
    return SX_OK;
}

} // namespace

//! one VE or std step (ve-bdt: sx_bdt.cpp; gravity only: sx_sim_nbody.cpp)
static int stepImpl(sx_sim* s)
{
    if (s->p.propagator >= 2) return s->p.propagator == 2 ? stepBdt(s) : stepNbody(s);
    StepCtx c{(hipStream_t)sx_ctx_stream_internal(s->ctx),
              sx_ctx_exact_internal(s->ctx) ? hydro_exact() : hydro_fast(),
              s->comm && s->comm->size() > 1, /*skinOn*/ skinUsable(s), /*reuse*/ false, /*powTab*/ nullptr};
    hipStream_t st = c.st;
    SIM_HIP(s->timer.start(st));

    // skin lists (sx_skin.hpp): a reuse step keeps the order and tree of the last full build and filters the
    // skin lists instead of syncing and searching
    if (c.skinOn && s->skin.backoff > 0)
    {
        s->skin.backoff--;
        s->skin.plainSteps++;
        c.skinOn = false;
    }
    c.reuse = c.skinOn && s->skin.valid && !s->skin.forceBuild && s->skin.sinceBuild < s->skin.maxReuse;
    if (!c.skinOn) s->skin.valid = false;

    if (int e = searchStage(s, c)) return e;
    const PairArgs pa = simPairArgs(s);
    if (int e = s->p.propagator == 1 ? forcesStd(s, c, pa) : forcesVe(s, c, pa)) return e;
    // ---- self-gravity (ve_hydro.hpp:193-202), added to ax, ay, az
    SIM_HIP(s->timer.begin(Kernel::gravity, st));
    if (s->p.g != 0.0)
        if (int e = gravityStage(s, st, c.dist, c.reuse)) return e;
    SIM_HIP(s->timer.end(Kernel::gravity, st));
    SIM_HIP(s->timer.stageEnd(Stage::Gravity, st));
    // ---- turbulence stirring (TurbVeProp::computeForces, turb_ve.hpp:114-119)
    if (s->turb)
        if (int e = turbStep(s, st)) return e;
    if (int e = integrateStage(s, c)) return e;
    return finishStep(s, c);
}

} // namespace sx::sim

//! the gravity-only propagator has no neighbor lists, skins, rungs or stirring: SX_ERR_ARG with the reason
static bool refusedForNbody(sx_sim* s, const char* why)
{
    if (!s || s->p.propagator != 3) return false;
    sx_ctx_set_error_internal(s->ctx, why);
    return true;
}

extern "C"
{

    int sx_sim_create(sx_sim** out, sx_ctx* ctx, size_t capacity, const sx_params* p, const sx_box* box,
                      uint32_t bucketSize)
    {
        if (p->propagator < 0 || p->propagator > 3) return SX_ERR_ARG;
        if (p->propagator == 3 && p->g == 0.0)
        {
            sx_ctx_set_error_internal(ctx, "sx_sim_create: the gravity-only propagator (3) needs g != 0");
            return SX_ERR_ARG;
        }
        // self-gravity in a periodic box: the image walk + Ewald correction of the VE / std step (single rank).  The
        // reference decides on boundaryX alone (gravity_wrapper.hpp:77,135) and walks images along all three axes;
        // here a mixed box (some axes periodic, some not) is refused rather than given images along open axes, the
        // Ewald sum needs a cubic box (ewald.hpp:149-214), and the ve-bdt driver's gravity has no image walk
        if (p->g != 0.0 && (box->bnd[0] == 1 || box->bnd[1] == 1 || box->bnd[2] == 1))
        {
            const bool allPbc = box->bnd[0] == 1 && box->bnd[1] == 1 && box->bnd[2] == 1;
            const double lx = box->lim[1] - box->lim[0], ly = box->lim[3] - box->lim[2], lz = box->lim[5] - box->lim[4];
            if (!allPbc || lx != ly || lx != lz || p->propagator == 2)
            {
                sx_ctx_set_error_internal(ctx, !allPbc ? "sx_sim_create: self-gravity needs a box that is open or "
                                                         "periodic along all three axes"
                                               : (p->propagator == 2
                                                      ? "sx_sim_create: ve-bdt has no periodic self-gravity"
                                                      : "sx_sim_create: periodic self-gravity (Ewald) needs a cubic box"));
                return SX_ERR_ARG;
            }
        }
        auto* s   = new sx_sim;
        s->ctx    = ctx;
        s->p      = *p;
        s->box    = *box;
        s->dbox   = toDevBox(box);
        s->bucket = bucketSize;
        s->cap    = capacity;
        s->nb.packMax = sx_ctx_pack12_max_internal(ctx); // (sx_set_pack12_max: before the sim is created)
        allocFields(s, capacity);
        if (s->p.propagator == 2) allocBdt(s);
        if (s->mem.failed())
        {
            delete s;
            return SX_ERR_NOMEM;
        }
        if (hipStreamCreateWithFlags(&s->commStream, hipStreamNonBlocking) != hipSuccess) s->commStream = nullptr;
        (void)hipEventCreateWithFlags(&s->evProd, hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&s->evComm, hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&s->evStats, hipEventDisableTiming);
        {
            // the highest priority: its few workgroups (one per directly stale cluster) are dispatched ahead of the
            // rebuild's persistent grid instead of sharing the CUs with it
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            if (hipStreamCreateWithPriority(&s->auxStream, hipStreamNonBlocking, greatest) != hipSuccess) s->auxStream = nullptr;
        }
        (void)hipEventCreateWithFlags(&s->evAuxIn, hipEventDisableTiming);
        (void)hipEventCreateWithFlags(&s->evAuxOut, hipEventDisableTiming);
        const Scalars init = freshScalars();
        (void)hipMemcpy(s->sc, &init, sizeof(Scalars), hipMemcpyHostToDevice);
        *out = s;
        return SX_OK;
    }

    void sx_sim_destroy(sx_sim* s)
    {
        if (!s) return;
        (void)hipDeviceSynchronize();
        if (s->evProd) (void)hipEventDestroy(s->evProd);
        if (s->evComm) (void)hipEventDestroy(s->evComm);
        if (s->evStats) (void)hipEventDestroy(s->evStats);
        if (s->commStream) (void)hipStreamDestroy(s->commStream);
        if (s->evAuxIn) (void)hipEventDestroy(s->evAuxIn);
        if (s->evAuxOut) (void)hipEventDestroy(s->evAuxOut);
        if (s->auxStream) (void)hipStreamDestroy(s->auxStream);
        turbDestroy(s->turb);
        sx::pairbin::release(s->mapBuf.bin);
        sx::pairbin::release(s->specBuf.bin);
        sx::profile::release(s->profBuf);
        sx::fof::release(s->fofBuf);
        sx::halo::release(s->haloBuf);
        sx::twopoint::release(s->tpBuf);
        delete s;
    }

    int sx_sim_set_comm(sx_sim* s, sx_comm* c)
    {
        if (s->gravCheckTargets)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_set_comm: the gravity check (sx_sim_set_gravity_check) runs on "
                                              "one rank");
            return SX_ERR_ARG;
        }
        if (s->turb)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_set_comm: a stirred sim (sx_sim_set_turbulence) runs on one rank");
            return SX_ERR_ARG;
        }
        sx::Transport* T = sx_comm_transport_internal(c);
        if (T && T->size() > 1)
        {
            // the sync's small per-rank buffers, allocated here so that no rank fails alone between two collectives
            // of a step (its peers would wait in the next one)
            if (!domReserveComm(s, (size_t)T->size())) return SX_ERR_NOMEM;
        }
        s->keysFresh  = false;
        s->skin.valid = false;
        s->comm       = T;
        s->commHandle = c;
        return SX_OK;
    }

    int sx_sim_set_overlap(sx_sim* s, int on)
    {
        s->overlap = on != 0;
        return SX_OK;
    }

    int sx_sim_overlap_stats(sx_sim* s, uint32_t out[2])
    {
        out[0] = s->nInterior;
        out[1] = s->nBoundary;
        return SX_OK;
    }

    int sx_sim_set_skin(sx_sim* s, float factor, int maxReuse)
    {
        if (!s || !(factor >= 0.0f) || factor > 1.0f || maxReuse < 1) return SX_ERR_ARG;
        if (refusedForNbody(s, "sx_sim_set_skin: the gravity-only propagator has no neighbor lists")) return SX_ERR_ARG;
        s->skin.factor   = factor;
        s->skin.cur      = factor;
        s->skin.built    = factor;
        s->skin.maxReuse = maxReuse;
        s->skin.valid    = false;
        return SX_OK;
    }

    //! test switch of the frozen kernel's staging (SkinState::frozenStage): entries staged, 0: the default
    int sx_sim_set_skin_frozen_stage_internal(sx_sim* s, uint32_t entries)
    {
        if (!s || entries > (uint32_t)kSkinFrozenCap) return SX_ERR_ARG;
        s->skin.frozenStage = entries;
        return SX_OK;
    }

    int sx_sim_rebuild_lists(sx_sim* s)
    {
        if (!s) return SX_ERR_ARG;
        if (refusedForNbody(s, "sx_sim_rebuild_lists: the gravity-only propagator has no neighbor lists"))
            return SX_ERR_ARG;
        s->skin.forceBuild = true;
        return SX_OK;
    }

    int sx_sim_skin_stats(sx_sim* s, uint64_t out[14])
    {
        if (!s) return SX_ERR_ARG;
        const auto& K = s->skin;
        out[0] = K.builds, out[1] = K.reuseSteps, out[2] = K.staleClusters, out[3] = K.exactClusters;
        out[4] = K.lastStale, out[5] = K.lastExact, out[6] = K.ngmaxS, out[7] = K.plainSteps;
        out[8] = (uint64_t)std::lround(1e6 * K.built), out[9] = (uint64_t)std::lround(1e6 * K.cur);
        out[10] = K.resyncs, out[11] = K.keptClusters, out[12] = K.frozenClusters, out[13] = K.earlyExact;
        return SX_OK;
    }

    int sx_sim_export_neighbors(sx_sim* s, uint32_t* out)
    {
        if (!s || !out) return SX_ERR_ARG;
        if (refusedForNbody(s, "sx_sim_export_neighbors: the gravity-only propagator has no neighbor lists"))
            return SX_ERR_ARG;
        if (s->nb.first != s->first || s->nb.last != s->last || s->nb.ngmax != s->p.ngmax) return SX_ERR_ARG;
        NsArgs a = listArgs(s);
        a.lb     = s->skin.lb; // the lists the last step's pair kernels read
        hipStream_t st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        SIM_HIP(exportNeighbors(a, out, st));
        SIM_HIP(hipStreamSynchronize(st));
        return SX_OK;
    }

    size_t sx_sim_size(sx_sim* s) { return s->last - s->first; }

    int sx_sim_layout(sx_sim* s, uint64_t out[4])
    {
        out[0] = s->first;
        out[1] = s->last;
        out[2] = s->n;
        out[3] = s->haloRetries + s->bdt.haloShort;
        return SX_OK;
    }

    int sx_sim_memory(sx_sim* s, uint64_t out[2])
    {
        if (!s || !out) return SX_ERR_ARG;
        out[0] = out[1] = 0;
        for (const sx::Arena* a : {&s->mem, &s->work, &s->farMem, &s->gravWork})
            out[0] += a->bytesAllocated(), out[1] += a->bytesPinned();
        return SX_OK;
    }

    int sx_sim_init_sedov_rank(sx_sim* s, uint32_t side, int rank, int size)
    {
        if (refusedForNbody(s, "sx_sim_init_sedov: the Sedov blast needs the thermal fields the gravity-only "
                               "propagator does not keep"))
            return SX_ERR_ARG;
        s->keysFresh  = false;
        s->skin.valid = false;
        size_t N  = (size_t)side * side * side;
        size_t f  = N * rank / size, l = N * (rank + 1) / size;
        size_t n  = l - f;
        if (n > s->cap) return SX_ERR_ARG;
        s->n          = n;
        s->first      = 0;
        s->last       = n;
        double r      = 0.5;
        double hInit  = std::cbrt(3.0 / (4 * M_PI) * s->p.ng0 * std::pow(2 * r, 3) / N) * 0.5;
        double width  = 0.1;
        double ener0  = 1.0 / std::pow(M_PI, 1.5) / 1. / std::pow(width, 3.0);
        float  cv     = idealGasCv(s->p.muiConst, s->p.gamma);
        auto   st     = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        if (n)
            sedovInitKernel<<<grid(n), 256, 0, st>>>(side, f, n, s->x, s->y, s->z, s->h, s->m, s->temp, s->vx, s->vy,
                                                     s->vz, s->xm1, s->ym1, s->zm1, s->dum1, s->alpha, s->id,
                                                     (float)hInit, (float)(1.0 / N), ener0, width * width, 1e-8, cv);
        if (s->rung && n) SIM_HIP(hipMemsetAsync(s->rung, 0, n, st));
        s->bdt.started = false;
        const Scalars init = freshScalars();
        SIM_HIP(hipMemcpyAsync(s->sc, &init, sizeof(Scalars), hipMemcpyHostToDevice, st));
        if (int e = coolResetStats(s, st)) return e;
        SIM_HIP(hipStreamSynchronize(st));
        return SX_OK;
    }

    int sx_sim_init_sedov(sx_sim* s, uint32_t side) { return sx_sim_init_sedov_rank(s, side, 0, 1); }

    int sx_sim_set_state(sx_sim* s, size_t n, const double* x, const double* y, const double* z, const float* h,
                         const float* m, const double* temp, const float* vx, const float* vy, const float* vz,
                         const float* x_m1, const float* y_m1, const float* z_m1, const float* du_m1,
                         const float* alpha, const uint64_t* id, double minDt, double minDt_m1)
    {
        s->keysFresh  = false;
        s->skin.valid = false;
        if (n > s->cap) return SX_ERR_ARG;
        if (s->p.propagator == 2)
        {   // ve-bdt carries the rung in the id's top byte through the particle exchange (PRec): ids must fit 56 bits
            for (size_t i = 0; i < n; ++i)
                if (id[i] >> 56) return SX_ERR_ARG;
        }
        s->n     = n;
        s->first = 0;
        s->last  = n;
        auto cp  = [n](void* d, const void* h, size_t es) { return hipMemcpy(d, h, n * es, hipMemcpyHostToDevice); };
        SIM_HIP(cp(s->x, x, 8));
        SIM_HIP(cp(s->y, y, 8));
        SIM_HIP(cp(s->z, z, 8));
        SIM_HIP(cp(s->h, h, 4));
        SIM_HIP(cp(s->m, m, 4));
        // the gravity-only propagator keeps no temp, du_m1, alpha: the arguments may be NULL and are ignored
        if (s->temp) SIM_HIP(cp(s->temp, temp, 8));
        SIM_HIP(cp(s->vx, vx, 4));
        SIM_HIP(cp(s->vy, vy, 4));
        SIM_HIP(cp(s->vz, vz, 4));
        SIM_HIP(cp(s->xm1, x_m1, 4));
        SIM_HIP(cp(s->ym1, y_m1, 4));
        SIM_HIP(cp(s->zm1, z_m1, 4));
        if (s->dum1) SIM_HIP(cp(s->dum1, du_m1, 4));
        if (s->alpha) SIM_HIP(cp(s->alpha, alpha, 4));
        SIM_HIP(cp(s->id, id, 8));
        if (s->rung) SIM_HIP(hipMemset(s->rung, 0, n));
        s->bdt.started = false;
        const Scalars init = freshScalars(minDt, minDt_m1);
        SIM_HIP(hipMemcpy(s->sc, &init, sizeof(Scalars), hipMemcpyHostToDevice));
        const double nothingRadiated[4] = {0.0, 0.0, 0.0, 0.0};
        if (s->cool.stats) SIM_HIP(hipMemcpy(s->cool.stats, nothingRadiated, sizeof(nothingRadiated), hipMemcpyHostToDevice));
        return SX_OK;
    }

    int sx_sim_fields(sx_sim* s, sx_fields* f, uint64_t** id)
    {
        // pointers to the LOCAL particles [first, last) of the last step
        *f   = simFields(s, s->first);
        f->n = s->last - s->first;
        if (id) *id = s->id + s->first;
        return SX_OK;
    }

    int sx_sim_conserved(sx_sim* s, double out[13])
    {
        hipStream_t   st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        const ConservedArgs a = conservedArgs(s->first, s->last, simFields(s), s->p.muiConst, s->p.gamma);
        double* scratch = s->work.get<double>("obs.scratch", conservedScratch(s->last - s->first));
        double* q       = s->work.get<double>("obs.q", 10);
        SIM_HIP(conservedQuantities(a, scratch, q, st));
        // egrav of the last step joins the sum (computeConservedQuantities, conserved_quantities.hpp:145-153)
        SIM_HIP(hipMemcpyAsync(q + 9, &s->sc->egrav, 8, hipMemcpyDeviceToDevice, st));
        if (s->comm && s->comm->size() > 1) SIM_COMM(s->comm->allreduceSumF64(q, 10, st));
        double h[10];
        SIM_HIP(hipMemcpyAsync(h, q, sizeof(h), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        const double ecin = h[0], eint = h[1], egrav = h[9];
        out[0] = ecin, out[1] = eint, out[2] = egrav, out[3] = ecin + eint + egrav;
        out[4] = std::sqrt(h[2] * h[2] + h[3] * h[3] + h[4] * h[4]);
        out[5] = std::sqrt(h[5] * h[5] + h[6] * h[6] + h[7] * h[7]);
        out[6] = h[8];
        for (int k = 0; k < 6; ++k)
            out[7 + k] = h[2 + k];
        return SX_OK;
    }

    int sx_sim_set_gravity_counting(sx_sim* s, int enable)
    {
        if (!s || s->p.g == 0.0) return SX_ERR_ARG;
        // the ve-bdt substeps (sx_bdt.cpp) do not count: refusing beats zeros that read as valid counts
        if (enable && s->p.propagator == 2) return SX_ERR_ARG;
        s->gravCount = enable != 0;
        if (s->gravCount)
        {
            // counts of a step without counting read as zeros, not as stale values
            hipStream_t st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
            SIM_HIP(hipMemsetAsync(gravReserveInteractions(s), 0, 16, st));
        }
        return SX_OK;
    }

    int sx_sim_set_gravity_check(sx_sim* s, uint32_t numTargets)
    {
        if (!s) return SX_ERR_ARG;
        const char* why = nullptr;
        if (s->p.g == 0.0) why = "sx_sim_set_gravity_check: the sim has no self-gravity";
        else if (s->p.propagator == 2)
            why = "sx_sim_set_gravity_check: not supported with block time-steps (ve-bdt): its substeps walk the "
                  "active rungs";
        else if (s->comm)
            why = "sx_sim_set_gravity_check: the direct sum needs all sources: the check runs on one rank (a "
                  "communicator is set)";
        if (why && numTargets) // disarming is always accepted
        {
            sx_ctx_set_error_internal(s->ctx, why);
            return SX_ERR_ARG;
        }
        s->gravCheckTargets = numTargets;
        return SX_OK;
    }

    int sx_sim_gravity_check(sx_sim* s, double out[6])
    {
        if (!s || !out) return SX_ERR_ARG;
        if (!s->gravCheckValid)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_gravity_check: no armed step has run (sx_sim_set_gravity_check)");
            return SX_ERR_ARG;
        }
        std::copy(s->gravCheck, s->gravCheck + 6, out);
        return SX_OK;
    }

    int sx_sim_gravity_interactions(sx_sim* s, uint64_t out[2])
    {
        if (!s || s->p.g == 0.0) return SX_ERR_ARG;
        if (!s->gravCount)
        {
            out[0] = out[1] = 0;
            return SX_OK;
        }
        hipStream_t st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        SIM_HIP(hipMemcpyAsync(out, s->grav.inter, 16, hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        return SX_OK;
    }

    int sx_sim_gravity_stats(sx_sim* s, uint64_t out[3])
    {
        out[0] = s->gravHalos;
        out[1] = s->gravFarCells;
        out[2] = s->gravRemoteCells;
        return SX_OK;
    }

    int sx_sim_set_observable(sx_sim* s, int kind, const sx_obs_settings* set)
    {
        if (!s) return SX_ERR_ARG;
        const char* why = nullptr;
        if (kind < 0 || kind >= kObsKinds) why = "sx_sim_set_observable: unknown kind";
        else if (kind == kObsKhGrowth && s->p.propagator == 1)
            why = "kx was empty. KHGrowthRate only supported with volume elements (--prop ve)";
        else if (kind == kObsWindBubble && s->p.propagator == 1)
            why = "kx was empty. Wind Shock surviving fraction is only supported with volume elements (--prop ve)";
        else if (s->p.propagator == 3 && kind != kObsTimeEnergy && kind != kObsGravWaves)
            why = "sx_sim_set_observable: the gravity-only propagator keeps neither kx nor c (time_energy and "
                  "grav_waves are supported)";
        if (why)
        {
            sx_ctx_set_error_internal(s->ctx, why);
            return SX_ERR_ARG;
        }
        sx_obs_settings o;
        sx_obs_default_settings(&o);
        if (set) o = *set;
        if (kind == kObsWindBubble && set)
        {
            // WindBubble's constructor and computeAndWrite (wind_bubble_fraction.hpp:114-131; factory.hpp:59-63)
            const double rhoInt = set->rhoBubble, uExt = set->tempWind, rSphere = set->initialMass;
            const double bubbleVolume = std::pow(rSphere, 3) * 4.0 / 3.0 * M_PI;
            o.initialMass = bubbleVolume * rhoInt;
            o.tempWind    = uExt * idealGasCv(s->p.muiConst, s->p.gamma);
        }
        s->obsKind = kind;
        s->obsSet  = o;
        return SX_OK;
    }

    int sx_sim_set_iteration(sx_sim* s, uint64_t iteration)
    {
        if (!s) return SX_ERR_ARG;
        s->iteration = iteration;
        return SX_OK;
    }

    int sx_sim_observe(sx_sim* s, double* row, int cap, int* ncols)
    {
        if (!s || !row) return SX_ERR_ARG;
        const int kind = s->obsKind;
        const int nx   = obsExtraSums(kind);
        const int nq   = kObsConserved + nx;
        const int nrow = kind == kObsGravWaves ? 15 : kind == kObsWindBubble ? 11 : kind == kObsTimeEnergy ? 9 : 10;
        if (ncols) *ncols = nrow;
        if (cap < nrow)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_observe: the row is longer than cap");
            return SX_ERR_ARG;
        }
        hipStream_t st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        ObsArgs     a{};
        a.c         = conservedArgs(s->first, s->last, simFields(s), s->p.muiConst, s->p.gamma);
        a.conserved = true;
        a.cs = s->c, a.kx = s->kx, a.xm = s->xm, a.ax = s->ax, a.ay = s->ay, a.az = s->az;
        a.ybox    = s->box.lim[3] - s->box.lim[2];
        a.rhoMin  = 0.64 * s->obsSet.rhoBubble;
        a.tempMax = 0.9 * s->obsSet.tempWind;
        double* scratch = s->work.get<double>("obs.fused", observablesScratch());
        // [nq sums | particle count | egrav]: one reduction over the ranks for all of it
        double* q = s->work.get<double>("obs.fusedQ", kObsMaxSums + 2);
        SIM_HIP(observables(kind, a, scratch, q, st));
        // egrav of the last step joins the sum (computeConservedQuantities, conserved_quantities.hpp:145-153)
        SIM_HIP(hipMemcpyAsync(q + nq + 1, &s->sc->egrav, 8, hipMemcpyDeviceToDevice, st));
        if (s->comm && s->comm->size() > 1) SIM_COMM(s->comm->allreduceSumF64(q, nq + 2, st));
        double h[kObsMaxSums + 2];
        float  m0 = 0.0f;
        SIM_HIP(hipMemcpyAsync(h, q, (nq + 2) * sizeof(double), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipMemcpyAsync(s->scHost, s->sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        if (kind == kObsWindBubble && !(s->obsSet.particleMass > 0.0) && s->last > s->first)
            SIM_HIP(hipMemcpyAsync(&m0, s->m + s->first, 4, hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));

        const double   ecin = h[0], eint = h[1], egrav = h[nq + 1];
        const uint64_t numGlobal = (uint64_t)h[nq];
        int            k = 0;
        row[k++] = (double)s->iteration;
        row[k++] = s->scHost->ttot;
        row[k++] = s->scHost->minDt;
        row[k++] = ecin + eint + egrav;
        row[k++] = ecin, row[k++] = eint, row[k++] = egrav;
        if (kind != kObsGravWaves)
        {
            row[k++] = std::sqrt(h[2] * h[2] + h[3] * h[3] + h[4] * h[4]);
            row[k++] = std::sqrt(h[5] * h[5] + h[6] * h[6] + h[7] * h[7]);
        }
        sx_obs_settings set = s->obsSet;
        if (!(set.particleMass > 0.0)) set.particleMass = m0;
        if (sx_obs_finalize(kind, &set, h, numGlobal, row + k) != SX_OK) return SX_ERR_ARG;
        k += kind == kObsGravWaves ? 2 : kind == kObsTimeEnergy ? 0 : 1;
        if (kind == kObsWindBubble) row[k++] = s->scHost->ttot / 0.0937; // normalizedTime, wind_bubble_fraction.hpp:138-139
        if (kind == kObsGravWaves)
            for (int j = 0; j < 6; ++j)
                row[k++] = h[kObsConserved + j];
        return SX_OK;
    }

    int sx_sim_step(sx_sim* s)
    {
        const int rc = stepImpl(s);
        if (rc == SX_OK) ++s->iteration;
        return rc;
    }

    int sx_sim_set_time(sx_sim* s, double ttot)
    {
        if (!s) return SX_ERR_ARG;
        hipStream_t st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        SIM_HIP(hipMemcpyAsync(s->scHost, s->sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        s->scHost->ttot = ttot;
        SIM_HIP(hipMemcpyAsync(s->sc, s->scHost, sizeof(Scalars), hipMemcpyHostToDevice, st));
        SIM_HIP(hipStreamSynchronize(st));
        s->bdt.ttot = ttot; // ve-bdt keeps d.ttot on the host between substeps
        return SX_OK;
    }

    int sx_sim_scalars(sx_sim* s, double out[6])
    {
        hipStream_t st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        SIM_HIP(hipMemcpyAsync(s->scHost, s->sc, sizeof(Scalars), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        out[0] = s->scHost->minDt;
        out[1] = s->scHost->minDt_m1;
        out[2] = s->scHost->ttot;
        out[3] = s->scHost->minDtCourant;
        out[4] = s->scHost->minDtRho;
        out[5] = s->scHost->egrav;
        return SX_OK;
    }

    int sx_sim_kernel_times(sx_sim* s, float* ms, int cap, const char** names)
    {
        // Kernel::nbodyIntegrate, the last one, is the gravity-only propagator's alone
        const int n = s->p.propagator == 3 ? kNumKernels : kNumKernels - 1;
        int       k = 0;
        for (; k < cap && k < n; ++k)
        {
            ms[k] = s->timer.kernelMs[k];
            if (names) names[k] = kKernelNames[k];
        }
        return k;
    }

    int sx_sim_stage_times(sx_sim* s, float* ms, int cap, const char** names)
    {
        int k = 0;
        for (; k < cap && k < kNumStages; ++k)
        {
            ms[k] = s->timer.stageMs[k];
            if (names) names[k] = kStageNames[k];
        }
        return k;
    }

    int sx_sim_last_stats(sx_sim* s, sx_nbstats* st)
    {
        if (refusedForNbody(s, "sx_sim_last_stats: the gravity-only propagator does no neighbor search"))
            return SX_ERR_ARG;
        *st = s->lastStats;
        return SX_OK;
    }

    // ---- turbulence stirring ----------------------------------------------------------------------------------------

    int sx_sim_set_turbulence(sx_sim* s, const sx_turb_settings* set)
    {
        if (!s) return SX_ERR_ARG;
        const char* why = nullptr;
        if (!set) why = "sx_sim_set_turbulence: no settings";
        else if (s->p.propagator == 3) why = "sx_sim_set_turbulence: the gravity-only propagator is not stirred (the "
                                             "reference stirs the VE propagators, turb_ve.hpp)";
        else if (s->p.propagator == 1) why = "sx_sim_set_turbulence: the std propagator has no stirred counterpart "
                                             "(the reference stirs the VE propagators, turb_ve.hpp)";
        else if (s->p.propagator == 2) why = "sx_sim_set_turbulence: stirring with block time-steps (ve-bdt) is not "
                                             "supported by sx_sim; sx_stir takes the active-rung views";
        else if (s->comm) why = "sx_sim_set_turbulence: a stirred sim runs on one rank (a communicator is set)";
        if (why)
        {
            sx_ctx_set_error_internal(s->ctx, why);
            return SX_ERR_ARG;
        }
        sx_turb* host = nullptr;
        if (sx_turb_create(&host, set) != SX_OK)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_set_turbulence: invalid settings (sx_turb_create)");
            return SX_ERR_ARG;
        }
        if (!s->turb)
        {
            auto* T  = new sx::turb::SimTurb;
            T->host  = host;
            bool made = true;
            for (auto& e : T->ringEv)
                made = made && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
            for (auto& e : T->ev)
                made = made && hipEventCreate(&e) == hipSuccess;
            if (!made)
            {
                turbDestroy(T); // with the host state
                return SX_ERR_HIP;
            }
            s->turb = T;
        }
        else
        {
            if (hipStreamSynchronize((hipStream_t)sx_ctx_stream_internal(s->ctx)) != hipSuccess)
            {
                sx_turb_destroy(host);
                return SX_ERR_HIP;
            }
            sx_turb_destroy(s->turb->host);
            s->turb->host = host;
        }
        return turbUpload(s);
    }

    int sx_sim_turbulence(sx_sim* s, sx_turb** out)
    {
        if (!s || !out) return SX_ERR_ARG;
        if (!s->turb)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_turbulence: sx_sim_set_turbulence was not called");
            return SX_ERR_ARG;
        }
        sx_turb& h = *s->turb->host;
        SIM_HIP(hipStreamSynchronize((hipStream_t)sx_ctx_stream_internal(s->ctx)));
        if (h.numModes) SIM_HIP(hipMemcpy(h.phases.data(), s->turb->phases, h.phases.size() * 8, hipMemcpyDeviceToHost));
        *out = &h;
        return SX_OK;
    }

    int sx_sim_set_turbulence_state(sx_sim* s, const double scalars[4], uint64_t numModes, const double* modes,
                                    const double* amplitudes, const double* phases, const char* rng)
    {
        if (!s) return SX_ERR_ARG;
        if (!s->turb)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_set_turbulence_state: sx_sim_set_turbulence was not called");
            return SX_ERR_ARG;
        }
        if (sx_turb_set_state(s->turb->host, scalars, numModes, modes, amplitudes, phases, rng) != SX_OK)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_set_turbulence_state: bad arrays or generator text");
            return SX_ERR_ARG;
        }
        return turbUpload(s);
    }

    int sx_sim_turbulence_times(sx_sim* s, float out[2])
    {
        if (!s || !out || !s->turb) return SX_ERR_ARG;
        out[0] = s->turb->ms[0], out[1] = s->turb->ms[1];
        return SX_OK;
    }

    // ---- radiative cooling ------------------------------------------------------------------------------------------

    int sx_sim_set_cooling(sx_sim* s, const sx_cooling* c, double ctCrit)
    {
        if (!s) return SX_ERR_ARG;
        const char* why = nullptr;
        if (s->p.propagator == 3) why = "sx_sim_set_cooling: the gravity-only propagator does not cool (it keeps no "
                                        "thermal field, nbody.hpp:74-77)";
        else if (s->p.propagator == 2) why = "sx_sim_set_cooling: cooling with block time-steps (ve-bdt) is not "
                                             "supported by sx_sim; sx_cool takes the columns of the active rungs";
        if (why && c) // switching off is always accepted
        {
            sx_ctx_set_error_internal(s->ctx, why);
            return SX_ERR_ARG;
        }
        hipStream_t st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        CoolState&  C  = s->cool;
        SIM_HIP(hipStreamSynchronize(st));
        // without the limiter, and without cooling, the candidate is INFINITY: the step's time-step is what it was
        const double inf = INFINITY;
        SIM_HIP(hipMemcpy(&s->sc->minDtCool, &inf, sizeof(double), hipMemcpyHostToDevice));
        if (!c)
        {
            C.on = false;
            return SX_OK;
        }
        const std::vector<double> p = sx::cool::packedTable(*c);
        C.table   = s->mem.get<double>("cool.table", 4 * sx::cool::kMaxNodes);
        C.minBits = s->mem.get<unsigned long long>("cool.min", 1);
        C.ePart   = s->mem.get<double>("cool.epart", sx::cool::partialBlocks((uint32_t)s->cap));
        C.cPart   = s->mem.get<uint32_t>("cool.cpart", 2 * sx::cool::partialBlocks((uint32_t)s->cap));
        const bool fresh = !C.stats;
        C.stats          = s->mem.get<double>("cool.stats", 4);
        if (!C.table || !C.minBits || !C.ePart || !C.cPart || !C.stats)
        {
            C.on = false;
            return SX_ERR_NOMEM;
        }
        SIM_HIP(hipMemcpy(C.table, p.data(), p.size() * sizeof(double), hipMemcpyHostToDevice));
        // a second table continues the first one's account of the energy radiated
        const double nothingRadiated[4] = {0.0, 0.0, 0.0, 0.0};
        if (fresh) SIM_HIP(hipMemcpy(C.stats, nothingRadiated, sizeof(nothingRadiated), hipMemcpyHostToDevice));
        C.numNodes = (uint32_t)c->T.size();
        C.ctCrit   = ctCrit;
        C.on       = true;
        return SX_OK;
    }

    int sx_sim_cooling_stats(sx_sim* s, double out[4])
    {
        if (!s || !out) return SX_ERR_ARG;
        if (!s->cool.on)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_cooling_stats: sx_sim_set_cooling was not called");
            return SX_ERR_ARG;
        }
        hipStream_t st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        double      h[4];
        SIM_HIP(hipMemcpyAsync(h, s->cool.stats, sizeof(h), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipMemcpyAsync(out, &s->sc->minDtCool, sizeof(double), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        out[1] = h[0], out[2] = h[3], out[3] = h[1];
        return SX_OK;
    }

    int sx_sim_set_cooling_radiated(sx_sim* s, double erad)
    {
        if (!s || !std::isfinite(erad)) return SX_ERR_ARG;
        if (!s->cool.on)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_set_cooling_radiated: sx_sim_set_cooling was not called");
            return SX_ERR_ARG;
        }
        hipStream_t st = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        SIM_HIP(hipStreamSynchronize(st));
        SIM_HIP(hipMemcpy(s->cool.stats + 3, &erad, sizeof(double), hipMemcpyHostToDevice));
        return SX_OK;
    }

    int sx_sim_cooling_times(sx_sim* s, float out[2])
    {
        if (!s || !out) return SX_ERR_ARG;
        if (!s->cool.on)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_cooling_times: sx_sim_set_cooling was not called");
            return SX_ERR_ARG;
        }
        out[0] = s->timer.coolingMs[(int)Cooling::coolingTime], out[1] = s->timer.coolingMs[(int)Cooling::cool];
        return SX_OK;
    }

} // extern "C"
