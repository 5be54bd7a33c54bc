// lo_gmap_host.cpp — util::VoxelGrid::filter (src/util/PointCloudUtils.h:462-557) on one core: the CPU baseline and
// the host-side parity anchor of the device map builder (lo_gmap.hip).  Built with -ffp-contract=off: every fp32
// operation below is separately rounded, as in the reference's build (-O3, no -march, so no FMA).
#include <cmath>
#include <cstddef>
#include <map>
#include <tuple>

#include "../../include/lo_gmap.h"

namespace {

struct Centroid {
    float x = 0.0f, y = 0.0f, z = 0.0f;
    float w = 0.0f;
};

// get_voxel_key's one axis (:548-553); false outside the stated key range (lo_gmap.h), where the cast is undefined
bool axis_key(float p, float leaf, int& k) {
    const float f = std::floor(p / leaf);
    if (!(f >= -1048576.0f && f < 1048576.0f)) return false;   // NaN and +-inf fail this too
    k = static_cast<int>(f);
    return true;
}

}  // namespace

extern "C" long long lo_gmap_voxelgrid_host(const float* xyz, size_t n, float voxel_size, float* out_xyz, size_t cap) {
    if (n > 0 && !xyz) return LO_ERR_ARG;
    if (n == 0 || !(voxel_size > 0.0f)) return 0;              // filter(): output.clear()
    std::map<std::tuple<int, int, int>, Centroid> voxels;      // VoxelKey's operator<: x, then y, then z
    for (size_t i = 0; i < n; ++i) {
        const float px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
        int kx, ky, kz;
        if (!std::isfinite(px) || !std::isfinite(py) || !std::isfinite(pz) || !axis_key(px, voxel_size, kx) ||
            !axis_key(py, voxel_size, ky) || !axis_key(pz, voxel_size, kz))
            return LO_ERR_ARG;
        Centroid& c = voxels[std::make_tuple(kx, ky, kz)];
        if (c.w == 0.0f) {                                     // WeightedCentroid::add_point (:504-521)
            c.x = px;
            c.y = py;
            c.z = pz;
            c.w = 1.0f;
        } else {
            const float tw = c.w + 1.0f;
            const float a = c.w / tw;
            const float b = 1.0f / tw;
            c.x = a * c.x + b * px;
            c.y = a * c.y + b * py;
            c.z = a * c.z + b * pz;
            c.w = tw;
        }
    }
    if (!out_xyz) return static_cast<long long>(voxels.size());
    size_t k = 0;
    for (const auto& v : voxels) {
        if (k >= cap) break;
        out_xyz[3 * k] = v.second.x;
        out_xyz[3 * k + 1] = v.second.y;
        out_xyz[3 * k + 2] = v.second.z;
        ++k;
    }
    return static_cast<long long>(k);
}
