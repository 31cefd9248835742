/*! @file sx_sim_spectrum.cpp
 * @brief sx_sim_spectrum: the power spectrum of the current state over all ranks (sx_spectrum.hpp).  Each rank deposits
 *        its locals, one f64-sum reduction runs over the meshes, every rank transforms and sums redundantly.  The arena
 *        tags ("spec.*") are requested in sx_spectrum.hip and, for the pair scratch, by the pair-binning engine
 *        (sx_pairbin.hip), each at one site, and kept in s->specBuf.
 */
#include "sx_sim_internal.hpp"

extern "C"
{
    int sx_sim_set_spectrum_pair_cap(sx_sim* s, uint64_t pairs)
    {
        if (!s) return SX_ERR_ARG;
        s->specBuf.bin.pairCap = pairs;
        return SX_OK;
    }

    int sx_sim_spectrum_stats(sx_sim* s, uint64_t out[4])
    {
        if (!s || !out) return SX_ERR_ARG;
        std::string why;
        const int   rc = sx::pairbin::statsCode(sx::pairbin::stats(s->specBuf.bin, (hipStream_t)sx_ctx_stream_internal(s->ctx), out),
                                                "sx_sim_spectrum_stats", sx::spectrum::kNames, why);
        if (rc != SX_OK) sx_ctx_set_error_internal(s->ctx, why.c_str());
        return rc;
    }

    int sx_sim_spectrum(sx_sim* s, const sx_spectrum* sp, int field, double* hostPower, uint64_t* hostModes)
    {
        if (!s || !sp || !hostPower) return SX_ERR_ARG;
        if (const char* why = sx::spectrum::checkSpec(sp, &s->box))
        {
            sx_ctx_set_error_internal(s->ctx, why);
            return SX_ERR_ARG;
        }
        sx::spectrum::DepositArgs args{s->box, s->x, s->y, s->z, s->h, s->m, {nullptr, nullptr, nullptr}, 0, 0,
                                       (uint32_t)s->first, (uint32_t)s->last, s->p.K, sp->n, nullptr, nullptr};
        if (sp->kind == SX_SPEC_VELOCITY)
        {
            args.numA = 3;
            args.a[0] = s->vx, args.a[1] = s->vy, args.a[2] = s->vz;
        }
        else
        {
            sx::sim::MapField f;
            std::string       why;
            if (!sx::sim::mapField(s, field, "sx_sim_spectrum", f, why))
            {
                sx_ctx_set_error_internal(s->ctx, why.c_str());
                return SX_ERR_ARG;
            }
            if (f.a) args.numA = 1, args.a[0] = f.a, args.aIsDouble = f.isDouble;
        }
        hipStream_t st   = (hipStream_t)sx_ctx_stream_internal(s->ctx);
        const bool  dist = s->comm && s->comm->size() > 1;
        std::function<bool(double*, size_t)> reduce;
        if (dist) reduce = [s, st](double* buf, size_t count) { return s->comm->allreduceSumF64(buf, count, st); };
        std::string err;
        const int   rc = sx::spectrum::compute(s->work, s->specBuf, *sp, args, nullptr, nullptr, reduce, st, err);
        if (rc != SX_OK)
        {
            sx_ctx_set_error_internal(s->ctx, err.c_str());
            return rc;
        }
        // through pinned memory, as the maps' images
        const uint32_t ns = sx::spectrum::numShells(sp->n);
        SIM_HIP(hipMemcpyAsync(s->specBuf.outHost, s->specBuf.out, 2 * ns * sizeof(double), hipMemcpyDeviceToHost, st));
        SIM_HIP(hipStreamSynchronize(st));
        std::memcpy(hostPower, s->specBuf.outHost, ns * sizeof(double));
        if (hostModes) std::memcpy(hostModes, s->specBuf.outHost + ns, ns * sizeof(uint64_t));
        return SX_OK;
    }
}
