// slice-sampling kernels of one model (slice_impl.hpp); separate units compile in parallel
#include "slice_impl.hpp"
SLICE_UNIT(distobs, DistObsDSL, MK_DIST_OBS)
