/*! @file sx_sim_twopoint.cpp
 * @brief sx_sim_twopoint: the two-point statistics of the locals of the current state (sx_twopoint.hpp), targets chosen
 *        by the sim's id column.  One rank only: pairs across a rank boundary would need halos of width r_max.
 *        The arena tags ("twopoint.*") are requested in sx_twopoint.hip, each at one site, and kept in s->tpBuf.
 */
#include "sx_sim_internal.hpp"

extern "C" sx::twopoint::TwoPointBuffers* sx_ctx_twopoint_buffers_internal(sx_ctx* c);

extern "C"
{
    int sx_sim_twopoint_stats(sx_sim* s, uint64_t out[5])
    {
        if (!s || !out) return SX_ERR_ARG;
        if (!s->tpBuf.done)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_twopoint_stats: no pairs have been counted");
            return SX_ERR_ARG;
        }
        std::copy(s->tpBuf.stats, s->tpBuf.stats + 5, out);
        return SX_OK;
    }

    int sx_sim_twopoint(sx_sim* s, const sx_twopoint* p, const sx_twopoint_result* res)
    {
        if (!s) return SX_ERR_ARG;
        // before anything a rank could wait in: every rank of the communicator takes this exit
        if (s->comm && s->comm->size() > 1)
        {
            sx_ctx_set_error_internal(s->ctx, ("sx_sim_twopoint: the communicator has " + std::to_string(s->comm->size()) +
                                               " ranks; pairs that cross rank boundaries are not counted (one rank only)")
                                                  .c_str());
            return SX_ERR_ARG;
        }
        sx_fields f = sx::sim::simFields(s);
        f.n         = s->n;
        if (std::string why = sx::twopoint::whyRefused(p, &s->box, &f, (uint32_t)s->first, (uint32_t)s->last, res);
            !why.empty())
        {
            sx_ctx_set_error_internal(s->ctx, why.c_str());
            return SX_ERR_ARG;
        }
        // sx_set_twopoint_timing and sx_twopoint_times of the context serve the sim's calls as well
        sx::twopoint::TwoPointBuffers* cb = sx_ctx_twopoint_buffers_internal(s->ctx);
        s->tpBuf.clock.on                 = cb->clock.on;
        std::string err;
        const int   rc = sx::twopoint::compute(s->work, s->tpBuf, *p, f, s->box, (uint32_t)s->first, (uint32_t)s->last,
                                               s->id, *res, true, (hipStream_t)sx_ctx_stream_internal(s->ctx), err);
        std::copy(s->tpBuf.clock.ms, s->tpBuf.clock.ms + 4, cb->clock.ms);
        if (rc != SX_OK) sx_ctx_set_error_internal(s->ctx, err.c_str());
        return rc;
    }
}
