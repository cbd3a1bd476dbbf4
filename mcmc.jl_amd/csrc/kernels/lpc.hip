// lpc.hip -- the unit table of the lane-per-chain kernels (d <= 32): a launch is planned (launch_plan.hpp) and handed to
// the model's unit; the kernels live in lpc_impl.hpp, instantiated per model by lpc_<model>.hip and lpc_ram_*.hip.
#include "layout_api.hpp"

using namespace mcmc;

static const UnitRow kLpcUnits[] = {
    {MK_ISO, lpc_iso, lpc_ram_iso},
    {MK_NORMAL, lpc_normal, lpc_ram_normal},
    {MK_ABS_NORMAL, lpc_absnormal, lpc_ram_absnormal},
    {MK_DIST, lpc_dist, lpc_ram_dist},
    {MK_DIST_OBS, lpc_distobs, nullptr},
    {MK_OU, lpc_ou, lpc_ram_ou},
};

hipError_t mcmc_launch_lpc_step(const KernelArgs& a, hipStream_t st) {
    LaunchPlan p;
    const KernelUnit u = unit_for(kLpcUnits, a, OP_STEP, false, p);
    return u.step ? u.step(a, p, st) : hipErrorInvalidValue;
}

hipError_t mcmc_launch_lpc_eval(const KernelArgs& a, const double* xin, double* lp, double* g, int check,
                                hipStream_t st) {
    LaunchPlan p;
    const KernelUnit u = unit_for(kLpcUnits, a, OP_EVAL, false, p);
    return u.eval ? u.eval(a, p, xin, lp, g, check, st) : hipErrorInvalidValue;
}

hipError_t mcmc_launch_lpc_record(const KernelArgs& a, const LeapRec& r, hipStream_t st) {
    LaunchPlan p;
    const KernelUnit u = unit_for(kLpcUnits, a, OP_RECORD, false, p);
    return u.record ? u.record(a, p, r, st) : hipErrorInvalidValue;
}

int mcmc_lpc_max_d() { return kPairMaxD; }
