// plane_seg_shared.h -- what plane_seg.hip offers plane_map.hip inside the library (not part of the HIP-free plane_seg_internal.h, which the walk program builds)
#pragma once
#include <cstdint>
#include <mutex>

#include "../../include/eao_fusion.h"

namespace eao {
// plane_seg.hip, for plane_map.hip's eao_plane_map_*_from_seg: the voxel cloud of plane `plane` of the handle's last run, four floats per point in device memory the
// handle owns.  On EAO_OK the handle's mutex is held through `lock` (no run replaces the cloud while it is copied); a plane that is out of range or not kept, and a
// handle without results, are EAO_ERR_INVALID.
eao_status plane_seg_kept_cloud(eao_plane_seg* h, int32_t plane, std::unique_lock<std::mutex>& lock, const float** pts, int32_t* n);
}  // namespace eao
