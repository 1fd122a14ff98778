// kernels_rows_images_g0.hip -- image-walk spectral-row kernels, row lengths of group 0 of fast_paths.hpp
// (one translation unit per kernel family and group: they compile in parallel, and each defines its group's entry points).
#define FC_TU_GROUP 0
#include "kernels_rows_images.inc"
