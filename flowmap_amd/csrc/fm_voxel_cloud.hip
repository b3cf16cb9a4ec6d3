// Voxel-fused point cloud (export.voxel_point_cloud; include/flowmap_hip.h: fm_voxel_cloud): the world points of the depth maps merged
// per cell of a world-space grid, in ONE pass over depth — no point cloud is formed.
//
// Every point adds INTEGERS to its voxel's record (fm_math.h: voxel_point — fixed-point position inside the cell, fixed-point colour, a
// count, the minimum linear index), so a record is a function of the SET of the voxel's points, never of their arrival order, and the
// finished cloud, sorted by the voxels' lowest index, is bit-reproducible.
//
// The table: open addressing with linear probing over `slots` (a power of two >= 2·capacity) 8-byte keys, all-ones = empty, home slot =
// voxel_hash(key) & (slots − 1); beside it one 64-byte record per slot, zeroed.
//
// voxel_insert_kernel: the geometry of render_splat_kernel.  A workgroup of 256 threads owns kVoxelInsertTile = 1024 consecutive pixels
// of ONE frame; the depth comes in with one 16-byte load per thread when width % 4 == 0 and the base is aligned (handed round through
// 4 KB of LDS so that a wave's lanes take neighbouring pixels, which mostly share a voxel and its 64-byte record), else with a scalar,
// bounds-checked load per pixel.  A live point walks its probe chain: a plain load of the key first — the slot already holds its key for
// all but a voxel's first point —, one 8-byte compare-and-swap only into an EMPTY slot; a lost swap means the slot now holds a key (this
// one or another) and the walk goes on from what the swap returned.  No thread ever waits for another: the walk visits every slot at
// most once and a point that finds none counts into `overflow`.  Then 8 no-return 8-byte atomics into the record (5 without colours).
//
// voxel_compact_kernel: one thread per slot; an occupied slot with count >= min_count draws an output row from a counter — one atomic
// per wave, the lanes' ranks from the ballot — and writes the finished record (fm_math.h: voxel_finalize) unless the row is past capacity.
#include <hip/hip_runtime.h>

#include "../../include/flowmap_hip.h"
#include "fm_device.h"
#include "fm_residual_args.h"

namespace fm {

constexpr int kVoxelThreads = 256;
constexpr int kVoxelInsertTile = kVoxelThreads * 4;  // pixels per workgroup: four per thread
static_assert(kVoxelInsertTile == kVoxelTile, "fm_residual_args.h states the tile");

struct VoxelInsertParams {
  const float* depth;
  const float* kinv;
  const float* ext;
  const float* colors;     // (F,3,H,W) or null
  const uint8_t* keep;     // (F,H,W) or null
  unsigned long long* keys;     // (slots)
  unsigned long long* records;  // (slots, 8)
  unsigned long long* counters;
  int32_t* pixel_slot;  // (F,H,W) or null
  int height, width;
  unsigned int slot_mask;  // slots − 1
  float inv;
};

struct VoxelCompactParams {
  const unsigned long long* keys;
  const unsigned long long* records;
  unsigned long long* counters;
  float* xyz;
  float* rgb;  // or null
  int32_t* count;
  int64_t* first;
  int32_t* slot;
  unsigned int slots;
  long capacity;
  unsigned long long min_count;
  double voxel_size;
};

__device__ __forceinline__ void voxel_add(unsigned long long* at, unsigned long long v) {
  __hip_atomic_fetch_add(at, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (result unused: a no-return atomic)
}

// The slot of `key`, claiming an empty one if the table does not hold it yet; −1: every slot holds another key.
__device__ __forceinline__ int voxel_slot_of(unsigned long long* keys, unsigned int mask, unsigned long long key) {
  unsigned int s = (unsigned int)voxel_hash(key) & mask;
  for (unsigned int probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {  // (bounded by the slot count: never a wait)
    unsigned long long held = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (held == kVoxelEmpty) {
      unsigned long long expected = kVoxelEmpty;
      if (__hip_atomic_compare_exchange_strong(&keys[s], &expected, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return (int)s;
      held = expected;  // (what won the slot: keys never change once set)
    }
    if (held == key) return (int)s;
  }
  return -1;
}

template <int VEC>
__global__ void __launch_bounds__(kVoxelThreads) voxel_insert_kernel(VoxelInsertParams p) {
  const int frame = blockIdx.y;
  const int n = p.height * p.width;
  const int tile0 = blockIdx.x * kVoxelInsertTile;  // (< n: the grid is render_blocks(n))
  const float* depth = p.depth + (size_t)frame * n;

  __shared__ float staged[VEC == 4 ? kVoxelInsertTile : 1];
  __shared__ unsigned int dropped[4];  // [VoxelClass], [0]: overflow
  if (threadIdx.x < 4) dropped[threadIdx.x] = 0u;
  if (VEC == 4) {  // width % 4 == 0: the quad lies inside the frame or past it, the base is 16-byte aligned
    const int px0 = tile0 + (int)threadIdx.x * 4;
    if (px0 < n) *reinterpret_cast<float4*>(&staged[threadIdx.x * 4]) = *reinterpret_cast<const float4*>(depth + px0);
  }
  __syncthreads();

  Mat3 ki;
  Pose e;
  load_mat3(p.kinv + (size_t)frame * 9, ki);
  load_pose44(p.ext + (size_t)frame * 16, e);
  const size_t index0 = (size_t)frame * n;  // (frames·height·width < 2^31)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int local = q * kVoxelThreads + (int)threadIdx.x, px = tile0 + local;
    if (px < n) {
      const float z = VEC == 4 ? staged[local] : depth[px];
      const int r = px / p.width, c = px - r * p.width;
      float xw[3];
      world_point_at(ki, e, pixel_center(c, p.width), pixel_center(r, p.height), z, xw);
      const bool kept = p.keep ? p.keep[index0 + px] != 0 : true;
      const VoxelPoint v = voxel_point(kept, z, xw, p.inv);
      int s = -1;
      if (v.cls == kVoxelLive) {
        s = voxel_slot_of(p.keys, p.slot_mask, v.key);
        if (s >= 0) {
          unsigned long long* rec = p.records + (size_t)s * kVoxelRecord;
          voxel_add(rec + 0, v.q[0]);
          voxel_add(rec + 1, v.q[1]);
          voxel_add(rec + 2, v.q[2]);
          if (p.colors) {
            const float* col = p.colors + (size_t)frame * 3 * n + px;
            voxel_add(rec + 3, voxel_color(col[0]));
            voxel_add(rec + 4, voxel_color(col[n]));
            voxel_add(rec + 5, voxel_color(col[2 * (size_t)n]));
          }
          voxel_add(rec + 6, 1ULL);
          __hip_atomic_fetch_max(rec + 7, ~(unsigned long long)(index0 + px), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
          atomicAdd(&dropped[0], 1u);
        }
      } else {
        atomicAdd(&dropped[v.cls], 1u);
      }
      if (p.pixel_slot) p.pixel_slot[index0 + px] = s;
    }
  }
  __syncthreads();  // (every thread arrives: nothing above returns)
  if (threadIdx.x < 4 && dropped[threadIdx.x] != 0u) voxel_add(p.counters + 1 + threadIdx.x, dropped[threadIdx.x]);
}

__global__ void __launch_bounds__(kVoxelThreads) voxel_compact_kernel(VoxelCompactParams p) {
  const unsigned int s = blockIdx.x * kVoxelThreads + threadIdx.x;
  const bool in = s < p.slots;
  const unsigned long long key = in ? p.keys[s] : kVoxelEmpty;
  const unsigned long long* rec = p.records + (size_t)(in ? s : 0u) * kVoxelRecord;
  const bool take = key != kVoxelEmpty && rec[6] >= p.min_count;
  const unsigned long long ballot = __ballot(take);  // (every lane of the wave arrives: nothing above returns)
  if (ballot == 0ULL) return;                        // (wave-uniform)
  const int lane = threadIdx.x & (kWave - 1), leader = __ffsll((long long)ballot) - 1;
  unsigned long long base = 0ULL;
  if (lane == leader) base = __hip_atomic_fetch_add(p.counters, (unsigned long long)__popcll(ballot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  base = __shfl(base, leader, kWave);
  if (!take) return;
  const unsigned long long row = base + (unsigned long long)__popcll(ballot & ((1ULL << lane) - 1ULL));
  if (row >= (unsigned long long)p.capacity) return;  // (counted, not written: the caller sees rows drawn > capacity)
  p.first[row] = voxel_finalize(key, rec, p.voxel_size, p.xyz + row * 3, p.rgb ? p.rgb + row * 3 : nullptr);
  p.count[row] = (int32_t)rec[6];
  p.slot[row] = (int32_t)s;
}

}  // namespace fm

using namespace fm;

extern "C" {

int fm_voxel_cloud_workspace(long capacity, long* slots, long* bytes) {
  FM_CHECK_ARG(voxel_cloud_workspace_args_ok(capacity, slots, bytes));
  slots[0] = voxel_cloud_slots(capacity);
  bytes[0] = voxel_cloud_workspace_bytes(capacity);
  return FM_OK;
}

int fm_voxel_cloud(const float* depth, const float* kinv, const float* ext, const float* colors, const uint8_t* keep, int frames, int height, int width,
                   double voxel_size, int min_count, long capacity, float* xyz, float* rgb, int32_t* count, int64_t* first, int32_t* slot,
                   int32_t* pixel_slot, unsigned long long* counters, void* workspace, void* stream) {
  FM_CHECK_ARG(voxel_cloud_args_ok(depth, kinv, ext, colors, keep, frames, height, width, voxel_size, min_count, capacity, xyz, rgb, count, first, slot,
                                   pixel_slot, counters, workspace));
  const long n = (long)height * width, slots = voxel_cloud_slots(capacity);
  unsigned long long* records = static_cast<unsigned long long*>(workspace);  // (slots, 8), then the keys (slots)
  unsigned long long* keys = records + (size_t)slots * kVoxelRecord;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(records, 0, (size_t)slots * 64, st) != hipSuccess) return FM_ERR_LAUNCH;
  if (hipMemsetAsync(keys, 0xFF, (size_t)slots * 8, st) != hipSuccess) return FM_ERR_LAUNCH;
  if (hipMemsetAsync(counters, 0, kVoxelCounters * 8, st) != hipSuccess) return FM_ERR_LAUNCH;
  VoxelInsertParams p{depth, kinv, ext, colors, keep, keys, records, counters, pixel_slot, height, width, (unsigned int)(slots - 1), (float)(1.0 / voxel_size)};
  const dim3 grid((unsigned)render_blocks(n), (unsigned)frames);
  if (width % 4 == 0 && aligned(depth, 16)) hipLaunchKernelGGL(voxel_insert_kernel<4>, grid, dim3(kVoxelThreads), 0, st, p);
  else hipLaunchKernelGGL(voxel_insert_kernel<1>, grid, dim3(kVoxelThreads), 0, st, p);
  VoxelCompactParams c{keys, records, counters, xyz, rgb, count, first, slot, (unsigned int)slots, capacity, (unsigned long long)min_count, voxel_size};
  hipLaunchKernelGGL(voxel_compact_kernel, dim3((unsigned)((slots + kVoxelThreads - 1) / kVoxelThreads)), dim3(kVoxelThreads), 0, st, c);
  FM_LAUNCH_STATUS();
}

}  // extern "C"
