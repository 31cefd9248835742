/*! @file sx_sim_map.cpp
 * @brief sx_sim_render: a map of the current state over all ranks (sx_map.hpp).  Each rank renders its locals, one
 *        f64-sum reduction runs over the images, with a refusal count in front.  The images' arena tags ("map.img",
 *        "map.imgHost") are requested here, the pair scratch's by the render; all are kept in s->mapBuf.
 */
#include "sx_sim_internal.hpp"

extern "C"
{
    int sx_sim_set_map_pair_cap(sx_sim* s, uint64_t pairs)
    {
        if (!s) return SX_ERR_ARG;
        s->mapBuf.bin.pairCap = pairs;
        return SX_OK;
    }

    int sx_sim_map_stats(sx_sim* s, uint64_t out[4])
    {
        if (!s || !out) return SX_ERR_ARG;
        std::string why;
        const int   rc = sx::pairbin::statsCode(sx::pairbin::stats(s->mapBuf.bin, (hipStream_t)sx_ctx_stream_internal(s->ctx), out),
                                                "sx_sim_map_stats", sx::map::kNames, why);
        if (rc != SX_OK) sx_ctx_set_error_internal(s->ctx, why.c_str());
        return rc;
    }

    int sx_sim_render(sx_sim* s, const sx_map* map, int field, double* hostSum0, double* hostSum1)
    {
        if (!s || !map || !hostSum0) return SX_ERR_ARG;
        sx::sim::MapField f;
        std::string       err;
        if (!sx::sim::mapField(s, field, "sx_sim_render", f, err))
        {
            sx_ctx_set_error_internal(s->ctx, err.c_str());
            return SX_ERR_ARG;
        }
        const void* a = f.a;
        if (a && !hostSum1)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_render: a field needs hostSum1");
            return SX_ERR_ARG;
        }
        if (const char* why = sx::map::checkSpec(map, &s->box))
        {
            sx_ctx_set_error_internal(s->ctx, why);
            return SX_ERR_ARG;
        }
        hipStream_t  st   = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        const size_t npix = (size_t)map->npix[0] * map->npix[1];
        const bool   dist = s->comm && s->comm->size() > 1;
        // [refusals | sum0 | sum1]: the word in front travels with the images through the one reduction, so a rank whose
        // render was refused (a tile row of ITS particles above the pair cap, no memory for ITS pairs) still takes part
        // and every rank learns of it
        s->mapBuf.img     = s->work.get<double>("map.img", 2 * npix + 1);
        s->mapBuf.imgHost = s->work.pinned<double>("map.imgHost", 2 * npix + 1);
        if (!s->mapBuf.img || !s->mapBuf.imgHost)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_render: image buffers");
            return SX_ERR_NOMEM;
        }
        double *      d0 = s->mapBuf.img + 1, *d1 = d0 + npix;
        sx::map::Args args{*map, s->box, s->x, s->y, s->z, s->h, s->m, a, f.isDouble, (uint32_t)s->first, (uint32_t)s->last,
                           s->p.K, d0, d1};
        const int     rc = sx::map::render(s->work, s->mapBuf, args, st, err);
        if (rc != SX_OK)
        {
            sx_ctx_set_error_internal(s->ctx, err.c_str());
            if (!dist) return rc;
        }
        const size_t count = 1 + (a ? 2 * npix : npix);
        if (dist)
        {
            // the images and the refusal count are adjacent: one f64 sum over the ranks serves all of it
            const double refused = rc != SX_OK ? 1.0 : 0.0;
            if (rc != SX_OK) SIM_HIP(hipMemsetAsync(s->mapBuf.img, 0, count * sizeof(double), st));
            SIM_HIP(hipMemcpyAsync(s->mapBuf.img, &refused, sizeof(double), hipMemcpyHostToDevice, st));
            SIM_COMM(s->comm->allreduceSumF64(s->mapBuf.img, count, st));
        }
        // through pinned memory: a copy into the caller's pageable arrays runs at a tenth of the link's rate
        SIM_HIP(hipMemcpyAsync(s->mapBuf.imgHost, s->mapBuf.img, count * sizeof(double), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        if (rc != SX_OK) return rc;
        if (dist && s->mapBuf.imgHost[0] != 0.0)
        {
            sx_ctx_set_error_internal(s->ctx, "sx_sim_render: refused on another rank (its sx_last_error has the reason)");
            return SX_ERR_ARG;
        }
        std::memcpy(hostSum0, s->mapBuf.imgHost + 1, npix * sizeof(double));
        if (a) std::memcpy(hostSum1, s->mapBuf.imgHost + 1 + npix, npix * sizeof(double));
        return SX_OK;
    }
}
