// nuts.hip -- dispatch of the NUTS kernels (nuts.hpp, nuts_impl.hpp) on the model kind: the step loop (init == 0) or
// the initial epsilon search (init != 0).  Built for the lane-per-chain and two-lanes-per-chain targets, d <= 32.
#include "layout_api.hpp"

hipError_t mcmc_launch_nuts(const mcmc::KernelArgs& a, int init, hipStream_t st) {
    using namespace mcmc;
    if (a.s.d < 1 || a.s.d > mcmc_nuts_max_d()) return hipErrorInvalidValue;
    switch (a.m.kind) {
        case MK_ISO: return mcmc_nuts_iso(a, init, st);
        case MK_NORMAL: return mcmc_nuts_normal(a, init, st);
        case MK_ABS_NORMAL: return mcmc_nuts_absnormal(a, init, st);
        case MK_DIST: return mcmc_nuts_dist(a, init, st);
        case MK_DIST_OBS: return mcmc_nuts_distobs(a, init, st);
        case MK_OU: return mcmc_nuts_ou(a, init, st);
        default: return hipErrorInvalidValue;
    }
}

int mcmc_nuts_max_d() { return 32; }
int mcmc_nuts_max_doublings() { return 10; }
