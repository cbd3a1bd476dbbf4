// slice.hip -- the unit table of the slice-sampling kernels (slice_impl.hpp).  Built for the lane-per-chain and
// two-lanes-per-chain targets, d <= 32.
#include "layout_api.hpp"

using namespace mcmc;

static const struct {
    int32_t kind;
    SliceFn* launch;
} kSliceUnits[] = {
    {MK_ISO, slice_iso},   {MK_NORMAL, slice_normal},     {MK_ABS_NORMAL, slice_absnormal},
    {MK_DIST, slice_dist}, {MK_DIST_OBS, slice_distobs},  {MK_OU, slice_ou},
};

hipError_t mcmc_launch_slice(const SliceKernelArgs& a, hipStream_t st) {
    const LaunchPlan p = launch_plan(a.m.kind, 0, a.s.d, a.s.C, false, OP_SLICE);
    if (p.built)
        for (const auto& r : kSliceUnits)
            if (r.kind == a.m.kind) return r.launch(a, p, st);
    return hipErrorInvalidValue;
}

int mcmc_slice_max_d() { return kSliceMaxD; }
