// NUTS kernels of one model (nuts_impl.hpp); separate units compile in parallel
#include "nuts_impl.hpp"
NUTS_UNIT(normal, NormalDSL, MK_NORMAL)
