// kernels_rows_filter_g0.hip -- multi-map spectral-row kernels with a spectral filter, configurations of group 0 of fast_paths.hpp
// (one translation unit per kernel family and group: they compile in parallel, and each defines its group's entry points).
#define FC_TU_GROUP 0
#include "kernels_rows_filter.inc"
