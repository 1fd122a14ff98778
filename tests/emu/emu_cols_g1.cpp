// TEST-ONLY: column configurations of group 1 of fast_paths.hpp for the host emulator (see emu_runners.hpp)
#include "emu_runners.hpp"
namespace emu {
template <> bool fast_cols_group<1>(int M, int T, EmuFastCols& run) { return fast_cols_dispatch_group<1>(M, T, run); }
template <> bool fast_cols_fwd_group<1>(int M, int T, bool pruned, EmuFastColsFwd& run) {
    return fast_cols_fwd_dispatch_group<1>(M, T, pruned, run);
}
}  // namespace emu
