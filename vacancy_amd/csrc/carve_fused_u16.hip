// The other half of the instances of carve_fused_kernel: update_num in TWO bytes (voxel_max_update_num > 254 once more
// than 255 views have been applied), behind launch_fused_counts16.  See carve_fused_u8.hip.
#include "carve_fused_kernel.h"

namespace vcy {
void launch_fused_counts16(const CarveLaunch& launch) { launch_fused<uint16_t>(launch); }
}  // namespace vcy
