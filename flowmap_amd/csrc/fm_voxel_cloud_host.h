// The voxel-fused point cloud (include/flowmap_hip.h, ABI version 15) for a HOST build of the C ABI.
//
// fm_math.h includes this file when it is compiled by a plain host compiler — the serial build of the ABI that the CPU test-suite links
// the package against instead of libflowmap_hip.so — and never under hipcc.  Per pixel it calls world_point_at, voxel_point, voxel_hash,
// voxel_color and voxel_finalize (fm_math.h), the very functions the device kernels (fm_voxel_cloud.hip) call, on the same table in the
// same workspace: keys claimed and records summed serially in frame and pixel order, rows drawn in slot order.  Which slot a key lands in
// and which row a slot draws depend on that order; the records, and the cloud once sorted by its lowest indices, do not.
#pragma once

#include <cstddef>
#include <cstring>

#include "../../include/flowmap_hip.h"
#include "fm_residual_args.h"

extern "C" {

int fm_voxel_cloud_workspace(long capacity, long* slots, long* bytes) {
  if (!fm::voxel_cloud_workspace_args_ok(capacity, slots, bytes)) return 1;
  slots[0] = fm::voxel_cloud_slots(capacity);
  bytes[0] = fm::voxel_cloud_workspace_bytes(capacity);
  return 0;
}

int fm_voxel_cloud(const float* depth, const float* kinv, const float* ext, const float* colors, const uint8_t* keep, int frames, int height, int width,
                   double voxel_size, int min_count, long capacity, float* xyz, float* rgb, int32_t* count, int64_t* first, int32_t* slot,
                   int32_t* pixel_slot, unsigned long long* counters, void* workspace, void*) {
  if (!fm::voxel_cloud_args_ok(depth, kinv, ext, colors, keep, frames, height, width, voxel_size, min_count, capacity, xyz, rgb, count, first, slot,
                               pixel_slot, counters, workspace))
    return 1;
  const size_t n = (size_t)height * width, slots = (size_t)fm::voxel_cloud_slots(capacity), mask = slots - 1;
  unsigned long long* records = static_cast<unsigned long long*>(workspace);
  unsigned long long* keys = records + slots * fm::kVoxelRecord;
  memset(records, 0, slots * 64);
  memset(keys, 0xFF, slots * 8);
  memset(counters, 0, fm::kVoxelCounters * 8);
  const float inv = (float)(1.0 / voxel_size);
  for (int frame = 0; frame < frames; ++frame) {
    fm::Mat3 ki;
    fm::Pose e;
    fm::load_mat3(kinv + (size_t)frame * 9, ki);
    fm::load_pose44(ext + (size_t)frame * 16, e);
    for (int r = 0; r < height; ++r)
      for (int c = 0; c < width; ++c) {
        const size_t px = (size_t)r * width + c, index = (size_t)frame * n + px;
        const float z = depth[index];
        float xw[3];
        fm::world_point_at(ki, e, fm::pixel_center(c, width), fm::pixel_center(r, height), z, xw);
        const fm::VoxelPoint v = fm::voxel_point(keep ? keep[index] != 0 : true, z, xw, inv);
        long s = -1;
        if (v.cls == fm::kVoxelLive) {
          size_t at = (size_t)fm::voxel_hash(v.key) & mask;
          for (size_t probe = 0; probe < slots; ++probe, at = (at + 1) & mask) {
            if (keys[at] == fm::kVoxelEmpty) keys[at] = v.key;
            if (keys[at] == v.key) {
              s = (long)at;
              break;
            }
          }
          if (s >= 0) {
            unsigned long long* rec = records + (size_t)s * fm::kVoxelRecord;
            for (int a = 0; a < 3; ++a) rec[a] += v.q[a];
            if (colors)
              for (int a = 0; a < 3; ++a) rec[3 + a] += fm::voxel_color(colors[((size_t)frame * 3 + a) * n + px]);
            rec[6] += 1;
            const unsigned long long inverted = ~(unsigned long long)index;
            rec[7] = inverted > rec[7] ? inverted : rec[7];
          } else {
            counters[1] += 1;
          }
        } else {
          counters[1 + v.cls] += 1;
        }
        if (pixel_slot) pixel_slot[index] = (int32_t)s;
      }
  }
  for (size_t s = 0; s < slots; ++s) {
    const unsigned long long* rec = records + s * fm::kVoxelRecord;
    if (keys[s] == fm::kVoxelEmpty || rec[6] < (unsigned long long)min_count) continue;
    const unsigned long long row = counters[0]++;
    if (row >= (unsigned long long)capacity) continue;
    first[row] = fm::voxel_finalize(keys[s], rec, voxel_size, xyz + row * 3, rgb ? rgb + row * 3 : nullptr);
    count[row] = (int32_t)rec[6];
    slot[row] = (int32_t)s;
  }
  return 0;
}

}  // extern "C"
