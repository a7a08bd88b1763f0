// step_amd/csrc/conv_tap_ph_f16.hip -- the two-phase (anti-phase wave groups) instantiations of conv_tap_kernel for f16 storage
#include "conv_tap_narrow.h"
namespace step {
template <> int conv_tap_ph_launch<f16_t>(const ConvPlan& pl, const ConvParams& p, int kd, dim3 grid, step_stream_t stream) {
    return conv_tap_ph_launch_impl<f16_t>(pl, p, kd, grid, stream);
}
template <> int conv_tap_group_launch<f16_t>(int twl, int NB, const ConvGroupParams& g, dim3 grid, step_stream_t stream) {
    bool narrow = false;
    for (int k = 0; k < g.n; ++k) narrow = narrow || g.p[k].narrow != 0;
    if (narrow) return twl == 0 ? conv_tap_group_narrow_launch_impl<f16_t>(NB, g, grid, stream) : STEP_E_UNSUPPORTED;
    return conv_tap_group_launch_impl<f16_t>(twl, NB, g, grid, stream);
}
}  // namespace step
