// ops.net_scatter_slices / ops.local_scatter_slices / ops.key_mix (ScatterOps.cpp).
#pragma once

#include <torch/extension.h>

void bindScatterOps(pybind11::module_ &ops);
