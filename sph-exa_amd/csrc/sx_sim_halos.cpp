/*! @file sx_sim_halos.cpp
 * @brief sx_sim_halos: the friends-of-friends groups of the locals of the current state and their properties
 *        (sx_halo.hpp), labelled by the sim's id column.  One rank only, as sx_sim_fof.  G, muiConst, gamma and the
 *        density rule are the sim's.  The arena tags ("fof.*", "halo.*") are requested in sx_fof.hip and sx_halo.hip,
 *        each at one site, and kept in s->fofBuf (shared with sx_sim_fof) and s->haloBuf.
 */
#include "sx_sim_internal.hpp"

extern "C" sx::halo::HaloBuffers* sx_ctx_halo_buffers_internal(sx_ctx* c);

extern "C"
{
    int sx_sim_halos_stats(sx_sim* s, uint64_t out[4])
    {
        if (!s || !out) return SX_ERR_ARG;
        if (!s->haloBuf.done)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_halos_stats: no group properties have been computed");
            return SX_ERR_ARG;
        }
        std::copy(s->haloBuf.stats, s->haloBuf.stats + 4, out);
        return SX_OK;
    }

    int sx_sim_halos(sx_sim* s, const sx_halo* spec, const sx_halo_result* res)
    {
        if (!s) return SX_ERR_ARG;
        // before anything a rank could wait in: every rank of the communicator takes this exit
        if (s->comm && s->comm->size() > 1)
        {
            sx_ctx_set_error_internal(s->ctx, ("sx_sim_halos: the communicator has " + std::to_string(s->comm->size()) +
                                               " ranks; groups that cross rank boundaries are not merged (one rank only)")
                                                  .c_str());
            return SX_ERR_ARG;
        }
        if (!spec)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_halos: null specification");
            return SX_ERR_ARG;
        }
        sx_halo p  = *spec;
        p.G        = (float)s->p.g;
        p.muiConst = s->p.muiConst;
        p.gamma    = s->p.gamma;
        p.std      = s->p.propagator == 1;
        sx_fields f = sx::sim::simFields(s);
        f.n         = s->n;
        if (std::string why = sx::halo::whyRefused(&p, &s->box, &f, (uint32_t)s->first, (uint32_t)s->last, res); !why.empty())
        {
            sx_ctx_set_error_internal(s->ctx, why.c_str());
            return SX_ERR_ARG;
        }
        // sx_set_halo_timing and sx_halo_times of the context serve the sim's calls as well
        sx::halo::HaloBuffers* cb = sx_ctx_halo_buffers_internal(s->ctx);
        s->haloBuf.clock.on       = cb->clock.on;
        std::string err;
        const int   rc = sx::halo::compute(s->work, s->fofBuf, s->haloBuf, p, f, s->box, (uint32_t)s->first, (uint32_t)s->last,
                                           s->id, *res, true, (hipStream_t)sx_ctx_stream_internal(s->ctx), err);
        std::copy(s->haloBuf.clock.ms, s->haloBuf.clock.ms + 4, cb->clock.ms);
        if (rc != SX_OK) sx_ctx_set_error_internal(s->ctx, err.c_str());
        return rc;
    }
}
