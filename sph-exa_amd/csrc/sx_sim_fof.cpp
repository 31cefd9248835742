/*! @file sx_sim_fof.cpp
 * @brief sx_sim_fof: the friends-of-friends groups of the locals of the current state (sx_fof.hpp), labelled by the
 *        sim's id column.  One rank only: a group that crosses a rank boundary would need an iterated label exchange.
 *        The arena tags ("fof.*") are requested in sx_fof.hip, each at one site, and kept in s->fofBuf.
 */
#include "sx_sim_internal.hpp"

extern "C" sx::fof::FofBuffers* sx_ctx_fof_buffers_internal(sx_ctx* c);

extern "C"
{
    int sx_sim_fof_stats(sx_sim* s, uint64_t out[4])
    {
        if (!s || !out) return SX_ERR_ARG;
        if (!s->fofBuf.done)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_fof_stats: no groups have been computed");
            return SX_ERR_ARG;
        }
        std::copy(s->fofBuf.stats, s->fofBuf.stats + 4, out);
        return SX_OK;
    }

    int sx_sim_fof(sx_sim* s, const sx_fof* p, const sx_fof_result* res)
    {
        if (!s) return SX_ERR_ARG;
        // before anything a rank could wait in: every rank of the communicator takes this exit
        if (s->comm && s->comm->size() > 1)
        {
            sx_ctx_set_error_internal(s->ctx, ("sx_sim_fof: the communicator has " + std::to_string(s->comm->size()) +
                                               " ranks; groups that cross rank boundaries are not merged (one rank only)")
                                                  .c_str());
            return SX_ERR_ARG;
        }
        sx_fields f = sx::sim::simFields(s);
        f.n         = s->n;
        if (std::string why = sx::fof::whyRefused(p, &s->box, &f, (uint32_t)s->first, (uint32_t)s->last, res); !why.empty())
        {
            sx_ctx_set_error_internal(s->ctx, why.c_str());
            return SX_ERR_ARG;
        }
        // sx_set_fof_timing and sx_fof_times of the context serve the sim's calls as well
        sx::fof::FofBuffers* cb = sx_ctx_fof_buffers_internal(s->ctx);
        s->fofBuf.clock.on      = cb->clock.on;
        std::string err;
        const int   rc = sx::fof::compute(s->work, s->fofBuf, *p, f, s->box, (uint32_t)s->first, (uint32_t)s->last, s->id,
                                          *res, true, (hipStream_t)sx_ctx_stream_internal(s->ctx), err);
        std::copy(s->fofBuf.clock.ms, s->fofBuf.clock.ms + 4, cb->clock.ms);
        if (rc != SX_OK) sx_ctx_set_error_internal(s->ctx, err.c_str());
        return rc;
    }
}
