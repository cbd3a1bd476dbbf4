// wpc.hip -- the unit table of the wave- and block-per-chain kernels (32 < d <= 16384): a launch is planned
// (launch_plan.hpp) and handed to the model's unit; the kernels live in wpc_impl.hpp and wpc_ram.hip, instantiated per
// model by wpc_<model>.hip.  DistObs and OU have no wave kernels.
#include "layout_api.hpp"

using namespace mcmc;

static const UnitRow kWpcUnits[] = {
    {MK_ISO, wpc_iso, wpc_ram_iso},
    {MK_NORMAL, wpc_normal, wpc_ram_normal},
    {MK_ABS_NORMAL, wpc_absnormal, wpc_ram_absnormal},
    {MK_DIST, wpc_dist, wpc_ram_dist},
};

hipError_t mcmc_launch_wpc_step(const KernelArgs& a, hipStream_t st) {
    LaunchPlan p;
    const KernelUnit u = unit_for(kWpcUnits, a, OP_STEP, true, p);
    return u.step ? u.step(a, p, st) : hipErrorInvalidValue;
}

hipError_t mcmc_launch_wpc_eval(const KernelArgs& a, const double* xin, double* lp, double* g, int check,
                                hipStream_t st) {
    LaunchPlan p;
    const KernelUnit u = unit_for(kWpcUnits, a, OP_EVAL, true, p);
    return u.eval ? u.eval(a, p, xin, lp, g, check, st) : hipErrorInvalidValue;
}

hipError_t mcmc_launch_wpc_record(const KernelArgs& a, const LeapRec& r, hipStream_t st) {
    LaunchPlan p;
    const KernelUnit u = unit_for(kWpcUnits, a, OP_RECORD, true, p);
    return u.record ? u.record(a, p, r, st) : hipErrorInvalidValue;
}

int mcmc_wpc_max_d() { return kBlockMaxD; }
int mcmc_wpc_ram_max_d() { return kRamMaxD; }
