// nuts.hip -- the unit table of the NUTS kernels (nuts.hpp, nuts_impl.hpp): the step loop (init == 0) or the initial
// epsilon search (init != 0).  Built for the lane-per-chain and two-lanes-per-chain targets, d <= 32.
#include "layout_api.hpp"

using namespace mcmc;

static const UnitRow kNutsUnits[] = {
    {MK_ISO, nuts_iso, nullptr},   {MK_NORMAL, nuts_normal, nullptr},     {MK_ABS_NORMAL, nuts_absnormal, nullptr},
    {MK_DIST, nuts_dist, nullptr}, {MK_DIST_OBS, nuts_distobs, nullptr},  {MK_OU, nuts_ou, nullptr},
};

hipError_t mcmc_launch_nuts(const KernelArgs& a, int init, hipStream_t st) {
    LaunchPlan p;
    const KernelUnit u = unit_for(kNutsUnits, a, init ? OP_NUTS_INIT : OP_STEP, false, p);
    return u.step ? u.step(a, p, st) : hipErrorInvalidValue;
}

int mcmc_nuts_max_d() { return kNutsMaxD; }
int mcmc_nuts_max_doublings() { return 10; }
