// slice-sampling kernels of one model (slice_impl.hpp); separate units compile in parallel
#include "slice_impl.hpp"
SLICE_UNIT(ou, OUDSL, MK_OU)
