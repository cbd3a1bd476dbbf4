// sampler.cpp -- validation of sampler and runner configurations (the reference's @asserts); what else the runtime
// asks about a sampler kind is the sampler table's (tables.hpp).
#include <cstdio>

#include "internal.hpp"

extern "C" int mcmc_sampler_validate(const mcmc_sampler_cfg* s) {
    if (!s) return mcmc_set_error(MCMC_E_INVALID_ARG, "sampler cfg is NULL");
    if (!mcmc::sampler_row(s->kind)) return mcmc_set_error(MCMC_E_UNSUPPORTED, "unknown sampler kind");
    const mcmc::SamplerInfo& si = sampler_info(s->kind);
    switch (s->kind) {
        case MCMC_RWM:
            if (!(s->scale > 0)) return mcmc_set_error(MCMC_E_INVALID_ARG, "scale should be > 0");               // RWM.jl:29
            if (s->tuner) return mcmc_set_error(MCMC_E_UNSUPPORTED, "RWM has no tuner in the reference (RWMTuner is abstract)");
            break;
        case MCMC_MALA:
        case MCMC_SMMALA:
        case MCMC_PMALA:                                             // MALA.jl:55, SMMALA.jl:27, PMALA.jl:30
            if (!(s->drift_step > 0)) return mcmc_set_error(MCMC_E_INVALID_ARG, std::string(si.name) + " drift step should be > 0");
            break;
        case MCMC_HMC:
            if (!(s->n_leaps > 0)) return mcmc_set_error(MCMC_E_INVALID_ARG, "inner steps should be > 0");        // HMC.jl:60
            if (!(s->leap_step > 0)) return mcmc_set_error(MCMC_E_INVALID_ARG, "inner steps scaling should be > 0"); // HMC.jl:61
            break;
        case MCMC_RMHMC:
        case MCMC_ERMLMC:
        case MCMC_RMLMC:                                             // RMHMC.jl:35-37, ERMLMC.jl:31-32, RMLMC.jl:35
            if (!(s->n_leaps > 0)) return mcmc_set_error(MCMC_E_INVALID_ARG, "Number of leapfrog steps should be > 0");
            if (!(s->leap_step > 0)) return mcmc_set_error(MCMC_E_INVALID_ARG, "Leapfrog step size should be > 0");
            if (si.newton_in_t0) {
                if (!(s->t0 > 0)) return mcmc_set_error(MCMC_E_INVALID_ARG, "Number of Newton steps should be > 0");
                if (!(s->t0 <= 2147483647.0) || s->t0 != (double)(int64_t)s->t0)
                    return mcmc_set_error(MCMC_E_INVALID_ARG, std::string(si.name) +
                                                        ": t0 carries nNewton and should hold an integer in 1 .. 2^31 - 1");
            }
            if (s->n_leaps > ((int64_t)1 << 20))
                return mcmc_set_error(MCMC_E_UNSUPPORTED, std::string(si.name) + " is built for nLeaps <= 2^20");
            break;
        case MCMC_RAM: {
            if (!(s->scale > 0)) return mcmc_set_error(MCMC_E_INVALID_ARG, "scale should be > 0");               // RAM.jl:27
            if (!(s->rate > 0.0 && s->rate < 1.0)) {
                char buf[160];
                snprintf(buf, sizeof buf, "target acceptance rate (%g) should be between 0 and 1", s->rate);
                return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                    // RAM.jl:28
            }
            if (s->tuner) return mcmc_set_error(MCMC_E_UNSUPPORTED, "RAM takes no tuner");
            break;
        }
        case MCMC_HMCDA: {
            char buf[160];
            if (!(0.0 < s->rate && s->rate < 1.0)) {
                snprintf(buf, sizeof buf, "Target acceptance rate (%g) should be between 0 and 1", s->rate);
                return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                    // HMCDA.jl:33
            }
            if (!(s->len > 0)) {
                snprintf(buf, sizeof buf, "len parameter of HMCDA sampler (%g) must be non-negative", s->len);
                return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                    // HMCDA.jl:34
            }
            if (!(s->shrinkage > 0)) {
                snprintf(buf, sizeof buf, "shrinkage parameter of HMCDA sampler (%g) must be positive", s->shrinkage);
                return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                    // HMCDA.jl:35
            }
            if (!(s->t0 >= 0)) {
                snprintf(buf, sizeof buf, "t0 parameter of HMCDA sampler (%g) must be non-negative", s->t0);
                return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                    // HMCDA.jl:36
            }
            if (s->tuner) return mcmc_set_error(MCMC_E_UNSUPPORTED, "HMCDA takes no tuner");
            break;
        }
        case MCMC_NUTS:
            // n_leaps carries maxdoublings
            if (!(s->n_leaps > 0)) return mcmc_set_error(MCMC_E_INVALID_ARG, "max doublings should be > 0");            // NUTS.jl:35
            if (!(s->n_leaps < 20)) return mcmc_set_error(MCMC_E_INVALID_ARG, "max doublings reasonably be < 20");      // NUTS.jl:36
            if (s->n_leaps > mcmc_nuts_max_doublings())
                return mcmc_set_error(MCMC_E_UNSUPPORTED, "NUTS is built for maxdoublings <= " +
                                                    std::to_string(mcmc_nuts_max_doublings()) +
                                                    " (1 023 leapfrogs a step; the reference accepts up to 19)");
            if (s->tuner) return mcmc_set_error(MCMC_E_UNSUPPORTED, "NUTS takes no tuner (NUTSTuner is abstract in the reference)");
            break;
    }
    if (s->tuner) {
        char buf[160];
        if (!(s->adapt_step > 0)) {
            snprintf(buf, sizeof buf, "Adaptation step size (%lld) should be > 0", (long long)s->adapt_step);
            return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                        // samplers.jl:40
        }
        if (!(s->max_step > 0)) {
            snprintf(buf, sizeof buf, "Adaptation step size (%lld) should be > 0", (long long)s->max_step);
            return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                        // samplers.jl:41
        }
        if (!(0.0 < s->target_rate && s->target_rate < 1.0)) {
            snprintf(buf, sizeof buf, "Target acceptance rate (%g) should be between 0 and 1", s->target_rate);
            return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                        // samplers.jl:42
        }
    }
    if (s->max_leaps < 0) return mcmc_set_error(MCMC_E_INVALID_ARG, "max_leaps should be >= 0");
    return MCMC_OK;
}

extern "C" int mcmc_runner_validate(const mcmc_runner_cfg* r) {
    if (!r) return mcmc_set_error(MCMC_E_INVALID_ARG, "runner cfg is NULL");
    char buf[160];
    if (!(r->burnin >= 0)) {
        snprintf(buf, sizeof buf, "Burnin rounds (%lld) should be >= 0", (long long)r->burnin);
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                            // SerialMC.jl:25
    }
    if (!(r->len > r->burnin)) {
        snprintf(buf, sizeof buf, "Total MCMC length (%lld) should be > to burnin (%lld)", (long long)r->len,
                 (long long)r->burnin);
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                            // SerialMC.jl:26
    }
    if (!(r->thinning >= 1)) {
        snprintf(buf, sizeof buf, "Thinning (%lld) should be >= 1", (long long)r->thinning);
        return mcmc_set_error(MCMC_E_INVALID_ARG, buf);                                                            // SerialMC.jl:27
    }
    if (r->len > 0x7fffffffLL) return mcmc_set_error(MCMC_E_INVALID_ARG, "len exceeds the 2^31 step counter");
    return MCMC_OK;
}
