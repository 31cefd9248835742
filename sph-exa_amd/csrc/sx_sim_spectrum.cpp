/*! @file sx_sim_spectrum.cpp
 * @brief sx_sim_spectrum: the power spectrum of the current state over all ranks (sx_spectrum.hpp).  Each rank deposits
 *        its locals, one f64-sum reduction runs over the meshes, every rank transforms and sums redundantly.  The arena
 *        tags ("spec.*") are requested in sx_spectrum.hip, each at one site, and kept in s->specBuf.
 */
#include "sx_sim_internal.hpp"

extern "C"
{
    int sx_sim_set_spectrum_pair_cap(sx_sim* s, uint64_t pairs)
    {
        if (!s) return SX_ERR_ARG;
        s->specBuf.pairCap = pairs;
        return SX_OK;
    }

    int sx_sim_spectrum_stats(sx_sim* s, uint64_t out[4])
    {
        if (!s || !out) return SX_ERR_ARG;
        const int rc = sx::spectrum::stats(s->specBuf, (hipStream_t)sx_ctx_stream_internal(s->ctx), out);
        if (rc == SX_ERR_ARG) sx_ctx_set_error_internal(s->ctx, "sx_sim_spectrum_stats: nothing has been deposited");
        if (rc == sx::spectrum::kStatsMismatch)
        {
            sx_ctx_set_error_internal(s->ctx, (std::string("sx_sim_spectrum_stats: ") + sx::spectrum::kStatsMismatchText).c_str());
            return SX_ERR_HIP;
        }
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
            // the column: {pointer, is double}; a field the propagator's layout does not keep is a null pointer
            const void* a    = nullptr;
            const char* name = nullptr;
            switch (field)
            {
                case SX_MAP_FIELD_NONE: break;
                case SX_MAP_FIELD_TEMP: a = s->temp, args.aIsDouble = 1, name = "temp"; break;
                case SX_MAP_FIELD_P: a = s->pres, name = "p"; break;
                case SX_MAP_FIELD_C: a = s->c, name = "c"; break;
                case SX_MAP_FIELD_VX: a = s->vx, name = "vx"; break;
                case SX_MAP_FIELD_VY: a = s->vy, name = "vy"; break;
                case SX_MAP_FIELD_VZ: a = s->vz, name = "vz"; break;
                case SX_MAP_FIELD_DIVV: a = s->divv, name = "divv"; break;
                case SX_MAP_FIELD_CURLV: a = s->curlv, name = "curlv"; break;
                case SX_MAP_FIELD_ALPHA: a = s->alpha, name = "alpha"; break;
                case SX_MAP_FIELD_H: a = s->h, name = "h"; break;
                default: sx_ctx_set_error_internal(s->ctx, "sx_sim_spectrum: unknown field"); return SX_ERR_ARG;
            }
            if (field != SX_MAP_FIELD_NONE && !a)
            {
                const std::string why =
                    std::string("sx_sim_spectrum: the field ") + name + " is not kept by " +
                    (s->p.propagator == 3 ? "the gravity-only propagator (none, vx, vy, vz and h are supported)"
                                          : "this propagator (p exists under the std propagator only: VE keeps p / rho)");
                sx_ctx_set_error_internal(s->ctx, why.c_str());
                return SX_ERR_ARG;
            }
            if (a) args.numA = 1, args.a[0] = a;
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
