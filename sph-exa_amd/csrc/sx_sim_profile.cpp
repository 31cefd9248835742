/*! @file sx_sim_profile.cpp
 * @brief sx_sim_profile: the binned profile of the current state over all ranks (sx_profile.hpp).  Each rank reads its
 *        locals; the windows agree through a u32-max reduction whose first word carries a refusal, the integer
 *        accumulators travel as 16-bit limbs through a u32 sum, min and max through an f64 min.  The arena tags
 *        ("prof.*") are requested in sx_profile.hip, each at one site, and kept in s->profBuf.
 */
#include "sx_sim_internal.hpp"

extern "C"
{
    int sx_sim_profile_stats(sx_sim* s, uint64_t out[4])
    {
        if (!s || !out) return SX_ERR_ARG;
        if (!s->profBuf.done)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_profile_stats: no profile has been computed");
            return SX_ERR_ARG;
        }
        std::copy(s->profBuf.stats, s->profBuf.stats + 4, out);
        return SX_OK;
    }

    int sx_sim_profile(sx_sim* s, const sx_profile* p, sx_profile_result* res)
    {
        if (!s || !res) return SX_ERR_ARG;
        hipStream_t     st   = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        const bool      dist = s->comm && s->comm->size() > 1;
        const int       std  = s->p.propagator == 1;
        const sx_fields f    = sx::sim::simFields(s);
        // a refusal is this rank's alone until the first reduction has carried it to the others
        const char* why = sx::profile::checkSpec(p, &s->box);
        std::string reason;
        if (!why && (why = sx::profile::whyRefused(p, &s->box, f, std, s->last - s->first)) && s->p.propagator == 3)
        {
            // a column the layout does not keep: say what the propagator does keep, as sx_sim_render does
            reason = std::string(why) + " (the gravity-only propagator keeps vel, vrad and h only)";
            why    = reason.c_str();
        }
        sx::profile::Reduce reduce;
        if (dist)
        {
            reduce.maxU32 = [s, st](uint32_t* buf, size_t count) { return s->comm->allreduceMaxU32(buf, count, st); };
            reduce.sumU32 = [s, st](uint32_t* buf, size_t count) { return s->comm->allreduceSumU32(buf, count, st); };
            reduce.minF64 = [s, st](double* buf, size_t count) { return s->comm->allreduceMinF64(buf, count, st); };
        }
        static const sx_profile none{};
        std::string             err;
        const int rc = sx::profile::compute(s->work, s->profBuf, p ? *p : none, f, s->box, (uint32_t)s->first,
                                            (uint32_t)s->last, s->p.muiConst, s->p.gamma, std, why, reduce, st, err);
        if (rc != SX_OK)
        {
            sx_ctx_set_error_internal(s->ctx, err.c_str());
            return rc;
        }
        // compute has synchronised and left the packed result in pinned memory
        sx::profile::Piece pc[8];
        const int          np = sx::profile::pieces(p->nbins, p->nq, *res, pc);
        for (int k = 0; k < np; ++k)
            std::memcpy(pc[k].dst, s->profBuf.outHost + pc[k].off, pc[k].words * 8);
        return SX_OK;
    }
}
