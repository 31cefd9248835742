/*! @file sx_sim_nbody.cpp
 * @brief The gravity-only step of sx_sim (propagator 3): NbodyProp::computeForces + integrate
 *        (main/src/propagator/nbody.hpp:115-163) on one GPU or SFC-decomposed over several.
 *
 * Step = sync -> a = 0 -> upsweep + walk (+ Ewald in a periodic box) -> acceleration time-step, min over the ranks
 *        -> positions.  The sync, the gravity stage and the time-step are the VE step's (sx_sim_domain.cpp,
 *        sx_sim_gravity.cpp, globalTimestep); the position update is nbodyIntegrateKernel (sx_nbody.hip), which touches
 *        no thermal field.  h is never updated, as in the reference.
 *
 * Several ranks: distributedSync as it is.  Its SPH halo discovery (request boxes grown by 2 h, here twice the
 * softening length) is kept although the walk does not read those halos: the request boxes it leaves (DomBuffers::mybox)
 * are what distributedGravity classifies near and far cells against, and with h a softening length the halos are few.
 * The halo masses are not overwritten with m[first] (nbody.hpp:127-129): gravity halos carry their own mass.
 *
 * Times (sx_step_timer.hpp): the step marks the stages sync, Gravity and UpdateQuantities and the kernels gravity and
 * nbodyIntegrate.  The names and their order are the VE step's (consumers index by position); the hydro stages and
 * kernels are not marked and read 0.
 */
#include "sx_sim_internal.hpp"

using namespace sx;
using namespace sx::sim;

namespace sx::sim
{

int stepNbody(sx_sim* s)
{
    hipStream_t st   = (hipStream_t)sx_ctx_stream_internal(s->ctx);
    const bool  dist = s->comm && s->comm->size() > 1;
    StepTimer&  T    = s->timer;
    SIM_HIP(T.start(st));

    // ---- sync: keys, sort, tree (nbody.hpp:118)
    if (int e = dist ? distributedSync(s, st, kHaloMargin) : localSync(s, st)) return e;
    SIM_HIP(T.stageEnd(Stage::sync, st));

    // ---- computeForces: a = 0 for the locals, then upsweep and walk add G acc (nbody.hpp:131-138)
    resetStepScalars(s, st);
    const size_t nl = s->last - s->first;
    if (nl)
    {
        SIM_HIP(hipMemsetAsync(s->ax + s->first, 0, nl * sizeof(float), st));
        SIM_HIP(hipMemsetAsync(s->ay + s->first, 0, nl * sizeof(float), st));
        SIM_HIP(hipMemsetAsync(s->az + s->first, 0, nl * sizeof(float), st));
    }
    SIM_HIP(T.begin(Kernel::gravity, st));
    if (int e = gravityStage(s, st, dist, false)) return e;
    SIM_HIP(T.end(Kernel::gravity, st));
    SIM_HIP(T.stageEnd(Stage::Gravity, st));

    // ---- integrate: minDtCourant = INFINITY, computeTimestep, computePositions (nbody.hpp:152-163)
    if (int e = globalTimestep(s, dist, st)) return e;
    NbodyPosArgs qa = nbodyPosArgs((uint32_t)s->first, (uint32_t)s->last, simFields(s), s->dbox);
    qa.dtPtr        = &s->sc->minDt;
    // one rank: the next localSync's keys come from this pass (the coordinates are in registers here)
    qa.keys = dist ? nullptr : s->keys;
    SIM_HIP(T.begin(Kernel::nbodyIntegrate, st));
    SIM_HIP(nbodyIntegrate(qa, st));
    SIM_HIP(T.end(Kernel::nbodyIntegrate, st));
    s->keysFresh = qa.keys != nullptr;
    SIM_HIP(T.stageEnd(Stage::UpdateQuantities, st));

    // ---- the end of the step: wait for it, stage and kernel times, the walk's error flag
    SIM_HIP(hipGetLastError());
    SIM_HIP(hipStreamSynchronize(st));
    T.collect();
    SIM_HIP(hipMemcpy(s->scHost, s->sc, sizeof(Scalars), hipMemcpyDeviceToHost));
    if (s->scHost->gravErr)
    {
        fprintf(stderr, "sx_sim_step: GPU traversal stack exhausted in Barnes-Hut\n");
        return SX_ERR_TRAVERSAL;
    }
    return SX_OK;
}

} // namespace sx::sim
