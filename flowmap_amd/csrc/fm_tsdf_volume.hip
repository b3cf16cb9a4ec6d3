// TSDF fusion (export.tsdf_volume, TsdfVolume.surface_points; include/flowmap_hip.h: fm_tsdf_volume, fm_tsdf_surface_count,
// fm_tsdf_surface_emit): the depth maps averaged into a signed-distance grid, and the grid's zero crossings as oriented points.
//
// The fused passes before this one SCATTER from pixels with atomics; this is the GATHER dual.  One thread owns one voxel (x fastest: a
// wave's 64 voxels are neighbours along x, so their projections into a frame lie on a short image line and the depth reads share cache
// lines), walks the frames of the window in ascending order, projects its centre (fm_math.h: tsdf_pixel_of), reads ONE depth, and keeps
// its sums in registers.  No atomics, no table, no capacity: every output element is written once, by one thread, from sums taken in a
// fixed order — bit-reproducible by construction.
//
// tsdf_poses_kernel: one thread per frame inverts E_f in fp64 (fm_math.h: tsdf_world_to_camera) into `world_to_camera`, which is an
// OUTPUT of the call as well as the integrate pass's pose table.
//
// tsdf_integrate_kernel: the per-frame constants — 12 pose values, 6 entries of K, the frame's depth / colour / keep bases — are
// indexed by the loop counter alone, so they are wave-uniform and the compiler keeps them in scalar registers (s_load): nothing is
// staged through LDS and the frames are not chunked.
//
// tsdf_surface_count_kernel / tsdf_surface_emit_kernel: a workgroup owns kTsdfTile consecutive voxels, that is 3·kTsdfTile consecutive
// edge ids (edge = voxel·3 + axis).  The count pass writes the crossings of each workgroup; the caller turns the counts into exclusive
// offsets (the one synchronisation that sizes the output); the emit pass repeats the decisions, ranks its threads with a scan through
// LDS and writes each row at offset + rank — rows in ascending edge id with no atomics and no sort.
//
// tsdf_mesh_count_kernel / tsdf_mesh_vertex_kernel / tsdf_mesh_face_kernel (TsdfVolume.mesh; fm_tsdf_mesh_count, fm_tsdf_mesh_emit): the
// surface-nets mesh of the volume by the same count, cumulative sum, emit scheme.  The vertex pass writes one vertex per active cell in
// ascending cell id and, for EVERY voxel, its row or −1 into `cell_vertex`; the face pass, after it on the same stream, looks the four
// cells of each quad up there and writes two triangles per quad in ascending edge id.
#include <hip/hip_runtime.h>

#include "../../include/flowmap_hip.h"
#include "fm_device.h"
#include "fm_residual_args.h"
#include "fm_tsdf_mesh.h"

namespace fm {

constexpr int kTsdfThreads = 256;
static_assert(kTsdfThreads == kTsdfTile, "fm_residual_args.h states the tile");

struct TsdfIntegrateParams {
  const float* __restrict__ depth;
  const float* __restrict__ k;
  const float* __restrict__ w2c;  // (F, 16)
  const float* __restrict__ colors;  // (F,3,H,W) or null
  const uint8_t* __restrict__ keep;  // (F,H,W) or null
  float* __restrict__ tsdf;
  int32_t* __restrict__ weight;
  float* __restrict__ color;  // (voxels, 3) or null
  int32_t* __restrict__ color_weight;
  int height, width, first_frame, count;
  int nx, ny;
  unsigned int voxels;
  float origin[3];
  float voxel_size, truncation, near;
};

__global__ void __launch_bounds__(kWave) tsdf_poses_kernel(const float* ext, float* w2c, int frames) {
  const int f = blockIdx.x * kWave + threadIdx.x;
  if (f >= frames) return;
  float m[16];
  tsdf_world_to_camera(ext + (size_t)f * 16, m);
  for (int e = 0; e < 16; ++e) w2c[(size_t)f * 16 + e] = m[e];
}

template <bool COLOR>
__global__ void __launch_bounds__(kTsdfThreads) tsdf_integrate_kernel(TsdfIntegrateParams p) {
  const unsigned int voxel = blockIdx.x * kTsdfThreads + threadIdx.x;
  if (voxel >= p.voxels) return;
  const unsigned int i = voxel % (unsigned int)p.nx, rest = voxel / (unsigned int)p.nx;
  const unsigned int j = rest % (unsigned int)p.ny, kz = rest / (unsigned int)p.ny;
  float c[3];
  c[0] = tsdf_centre(p.origin[0], (int)i, p.voxel_size);
  c[1] = tsdf_centre(p.origin[1], (int)j, p.voxel_size);
  c[2] = tsdf_centre(p.origin[2], (int)kz, p.voxel_size);
  const size_t n = (size_t)p.height * p.width;
  float sum = 0.f, rgb[3] = {0.f, 0.f, 0.f};
  int weight = 0, color_weight = 0;
  for (int f = p.first_frame; f < p.first_frame + p.count; ++f) {  // (uniform: the constants below are scalar loads)
    Pose wc;
    Mat3 km;
    load_pose44(p.w2c + (size_t)f * 16, wc);
    load_mat3(p.k + (size_t)f * 9, km);
    float pz;
    const int pixel = tsdf_pixel_of(wc, km, c, p.near, p.height, p.width, pz);
    if (pixel < 0) continue;  // (0 <= pixel < height·width otherwise: the row and the column are clamped into the frame)
    const size_t at = (size_t)f * n + (size_t)pixel;
    if (p.keep && p.keep[at] == 0) continue;
    float t;
    bool coloured;
    if (!tsdf_term(p.depth[at], pz, p.truncation, t, coloured)) continue;
    sum += t;
    weight += 1;
    if (COLOR && coloured) {
      const float* from = p.colors + (size_t)f * 3 * n + (size_t)pixel;
      rgb[0] += from[0];
      rgb[1] += from[n];
      rgb[2] += from[2 * n];
      color_weight += 1;
    }
  }
  p.tsdf[voxel] = tsdf_finish(sum, weight);
  p.weight[voxel] = weight;
  if (COLOR) {
    float* to = p.color + (size_t)voxel * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) to[a] = color_weight > 0 ? rgb[a] / (float)color_weight : 0.f;
    p.color_weight[voxel] = color_weight;
  }
}

// The crossings among the three edges of this thread's voxel, as a bit per axis (0 past the grid).
__device__ __forceinline__ int tsdf_thread_crossings(const TsdfGrid& g, long voxels, long voxel, int ijk[3]) {
  if (voxel >= voxels) return 0;
  tsdf_voxel_ijk(g, voxel, ijk);
  int bits = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) bits |= tsdf_edge_crosses(g, voxel, ijk, a) ? 1 << a : 0;
  return bits;
}

// Inclusive scan of one int per thread over the workgroup, in thread order (Hillis-Steele through LDS; every thread arrives).
__device__ __forceinline__ int tsdf_block_scan(int value, int* lds) {
  lds[threadIdx.x] = value;
  __syncthreads();
  for (int off = 1; off < kTsdfThreads; off <<= 1) {
    const int left = (int)threadIdx.x >= off ? lds[threadIdx.x - off] : 0;
    __syncthreads();
    lds[threadIdx.x] += left;
    __syncthreads();
  }
  return lds[threadIdx.x];
}

__global__ void __launch_bounds__(kTsdfThreads) tsdf_surface_count_kernel(TsdfGrid g, long voxels, int64_t* block_counts) {
  __shared__ int lds[kTsdfThreads];
  int ijk[3];
  const long voxel = (long)blockIdx.x * kTsdfThreads + threadIdx.x;
  const int bits = tsdf_thread_crossings(g, voxels, voxel, ijk);
  const int total = tsdf_block_scan(__popc(bits), lds);
  if (threadIdx.x == kTsdfThreads - 1) block_counts[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kTsdfThreads) tsdf_surface_emit_kernel(TsdfGrid g, long voxels, const int64_t* block_offsets, long rows, float* xyz,
                                                                        float* normals, float* rgb, int64_t* edge) {
  __shared__ int lds[kTsdfThreads];
  int ijk[3];
  const long voxel = (long)blockIdx.x * kTsdfThreads + threadIdx.x;
  const int bits = tsdf_thread_crossings(g, voxels, voxel, ijk);
  const int mine = __popc(bits);
  long row = block_offsets[blockIdx.x] + (long)(tsdf_block_scan(mine, lds) - mine);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(bits & (1 << a))) continue;
    if (row >= 0 && row < rows) {  // (the caller sized the outputs from the count pass on the same volume: always true then)
      float point[3], normal[3], colour[3];
      tsdf_edge_point(g, voxel, ijk, a, rgb != nullptr, point, normal, colour);
      for (int e = 0; e < 3; ++e) {
        xyz[row * 3 + e] = point[e];
        normals[row * 3 + e] = normal[e];
        if (rgb) rgb[row * 3 + e] = colour[e];
      }
      edge[row] = (int64_t)voxel * 3 + a;
    }
    ++row;
  }
}

// ---- the mesh (fm_tsdf_mesh.h: surface nets) — the same tiling: the thread owns the cell whose low corner is its voxel, and that voxel's
// three edges.  A workgroup holds at most 256 active cells and 768 quads, so the two counts share one scan, 16 bits each.

// The crossings of this thread's cell (12 bits; 0 past the grid or where the cell does not exist).
__device__ __forceinline__ int tsdf_thread_cell(const TsdfGrid& g, long voxels, long voxel, int ijk[3]) {
  if (voxel >= voxels) return 0;
  tsdf_voxel_ijk(g, voxel, ijk);
  return tsdf_cell_crossings(g, voxel, ijk);
}

__global__ void __launch_bounds__(kTsdfThreads) tsdf_mesh_count_kernel(TsdfGrid g, long voxels, int64_t* cell_counts, int64_t* quad_counts) {
  __shared__ int lds[kTsdfThreads];
  int ijk[3] = {0, 0, 0};
  const long voxel = (long)blockIdx.x * kTsdfThreads + threadIdx.x;
  const int bits = tsdf_thread_cell(g, voxels, voxel, ijk);
  const int quads = bits ? tsdf_voxel_quads(g, ijk, bits) : 0;
  const int total = tsdf_block_scan((bits ? 1 : 0) | (__popc(quads) << 16), lds);
  if (threadIdx.x == kTsdfThreads - 1) {
    cell_counts[blockIdx.x] = total & 0xffff;
    quad_counts[blockIdx.x] = total >> 16;
  }
}

template <bool COLOR>
__global__ void __launch_bounds__(kTsdfThreads) tsdf_mesh_vertex_kernel(TsdfGrid g, long voxels, const int64_t* cell_offsets, long rows, float* xyz, float* normals,
                                                                        float* rgb, int64_t* cell, int32_t* cell_vertex) {
  __shared__ int lds[kTsdfThreads];
  int ijk[3] = {0, 0, 0};
  const long voxel = (long)blockIdx.x * kTsdfThreads + threadIdx.x;
  const int bits = tsdf_thread_cell(g, voxels, voxel, ijk);
  const int mine = bits ? 1 : 0;
  const long row = cell_offsets[blockIdx.x] + (long)(tsdf_block_scan(mine, lds) - mine);
  const bool write = mine && row >= 0 && row < rows;  // (the caller sized the outputs from the count pass on the same volume: always true then)
  if (voxel < voxels) cell_vertex[voxel] = write ? (int32_t)row : -1;  // EVERY voxel: the face pass reads it without a memset before
  if (!write) return;
  float point[3], normal[3], colour[3];
  tsdf_cell_vertex(g, voxel, ijk, bits, COLOR, point, normal, colour);  // (a compile-time flag: a run-time one kept `colour` on the stack)
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    xyz[row * 3 + e] = point[e];
    normals[row * 3 + e] = normal[e];
    if (COLOR) rgb[row * 3 + e] = colour[e];
  }
  cell[row] = (int64_t)voxel;
}

__global__ void __launch_bounds__(kTsdfThreads) tsdf_mesh_face_kernel(TsdfGrid g, long voxels, const int64_t* quad_offsets, long rows,
                                                                      const int32_t* cell_vertex, int32_t* faces, int64_t* edge) {
  __shared__ int lds[kTsdfThreads];
  int ijk[3] = {0, 0, 0};
  const long voxel = (long)blockIdx.x * kTsdfThreads + threadIdx.x;
  const int bits = tsdf_thread_cell(g, voxels, voxel, ijk);
  const int quads = bits ? tsdf_voxel_quads(g, ijk, bits) : 0;
  const int mine = __popc(quads);
  long row = quad_offsets[blockIdx.x] + (long)(tsdf_block_scan(mine, lds) - mine);
  if (!quads) return;
  const bool low_negative = g.tsdf[voxel] < 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!(quads & (1 << a))) continue;
    if (row >= 0 && row < rows) {
      long cells[4];
      tsdf_quad_cells(g, voxel, a, low_negative, cells);  // (inside the grid: tsdf_edge_has_quad)
      const int32_t q0 = cell_vertex[cells[0]], q1 = cell_vertex[cells[1]], q2 = cell_vertex[cells[2]], q3 = cell_vertex[cells[3]];
      int32_t* to = faces + row * 6;
      to[0] = q0, to[1] = q1, to[2] = q2;
      to[3] = q0, to[4] = q2, to[5] = q3;
      edge[row] = (int64_t)voxel * 3 + a;
    }
    ++row;
  }
}

static TsdfGrid tsdf_grid(const float* tsdf, const int32_t* weight, const float* color, const int32_t* color_weight, int nx, int ny, int nz, int min_weight,
                          float ox, float oy, float oz, float voxel_size) {
  TsdfGrid g{tsdf, weight, color, color_weight, nx, ny, nz, min_weight, {ox, oy, oz}, voxel_size};
  return g;
}

}  // namespace fm

using namespace fm;

extern "C" {

int fm_tsdf_volume(const float* depth, const float* k, const float* ext, const float* colors, const uint8_t* keep, int frames, int height, int width,
                   int first_frame, int count, float ox, float oy, float oz, int nx, int ny, int nz, float voxel_size, float truncation, float near,
                   float* world_to_camera, float* tsdf, int32_t* weight, float* color, int32_t* color_weight, void* stream) {
  FM_CHECK_ARG(tsdf_volume_args_ok(depth, k, ext, colors, keep, frames, height, width, first_frame, count, ox, oy, oz, nx, ny, nz, voxel_size, truncation,
                                   near, world_to_camera, tsdf, weight, color, color_weight));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(tsdf_poses_kernel, dim3((unsigned)((frames + kWave - 1) / kWave)), dim3(kWave), 0, st, ext, world_to_camera, frames);
  const long voxels = (long)nx * ny * nz;
  TsdfIntegrateParams p{depth, k, world_to_camera, colors, keep, tsdf, weight, color, color_weight, height, width, first_frame, count, nx, ny,
                        (unsigned int)voxels, {ox, oy, oz}, voxel_size, truncation, near};
  const dim3 grid((unsigned)tsdf_blocks(voxels));
  if (colors) hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, dim3(kTsdfThreads), 0, st, p);
  else hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, dim3(kTsdfThreads), 0, st, p);
  FM_LAUNCH_STATUS();
}

int fm_tsdf_surface_blocks(int nx, int ny, int nz, long* blocks) {
  FM_CHECK_ARG(tsdf_surface_blocks_args_ok(nx, ny, nz, blocks));
  blocks[0] = tsdf_blocks((long)nx * ny * nz);
  return FM_OK;
}

int fm_tsdf_surface_count(const float* tsdf, const int32_t* weight, int nx, int ny, int nz, int min_weight, int64_t* block_counts, void* stream) {
  FM_CHECK_ARG(tsdf_surface_count_args_ok(tsdf, weight, nx, ny, nz, min_weight, block_counts));
  const long voxels = (long)nx * ny * nz;
  const TsdfGrid g = tsdf_grid(tsdf, weight, nullptr, nullptr, nx, ny, nz, min_weight, 0.f, 0.f, 0.f, 1.f);
  hipLaunchKernelGGL(tsdf_surface_count_kernel, dim3((unsigned)tsdf_blocks(voxels)), dim3(kTsdfThreads), 0, (hipStream_t)stream, g, voxels, block_counts);
  FM_LAUNCH_STATUS();
}

int fm_tsdf_surface_emit(const float* tsdf, const int32_t* weight, const float* color, const int32_t* color_weight, int nx, int ny, int nz, float ox, float oy,
                         float oz, float voxel_size, int min_weight, const int64_t* block_offsets, long rows, float* xyz, float* normals, float* rgb,
                         int64_t* edge, void* stream) {
  FM_CHECK_ARG(tsdf_surface_emit_args_ok(tsdf, weight, color, color_weight, nx, ny, nz, ox, oy, oz, voxel_size, min_weight, block_offsets, rows, xyz, normals,
                                         rgb, edge));
  const long voxels = (long)nx * ny * nz;
  const TsdfGrid g = tsdf_grid(tsdf, weight, color, color_weight, nx, ny, nz, min_weight, ox, oy, oz, voxel_size);
  hipLaunchKernelGGL(tsdf_surface_emit_kernel, dim3((unsigned)tsdf_blocks(voxels)), dim3(kTsdfThreads), 0, (hipStream_t)stream, g, voxels, block_offsets, rows,
                     xyz, normals, rgb, edge);
  FM_LAUNCH_STATUS();
}

int fm_tsdf_mesh_count(const float* tsdf, const int32_t* weight, int nx, int ny, int nz, int min_weight, int64_t* cell_counts, int64_t* quad_counts,
                       void* stream) {
  FM_CHECK_ARG(tsdf_mesh_count_args_ok(tsdf, weight, nx, ny, nz, min_weight, cell_counts, quad_counts));
  const long voxels = (long)nx * ny * nz;
  const TsdfGrid g = tsdf_grid(tsdf, weight, nullptr, nullptr, nx, ny, nz, min_weight, 0.f, 0.f, 0.f, 1.f);
  hipLaunchKernelGGL(tsdf_mesh_count_kernel, dim3((unsigned)tsdf_blocks(voxels)), dim3(kTsdfThreads), 0, (hipStream_t)stream, g, voxels, cell_counts,
                     quad_counts);
  FM_LAUNCH_STATUS();
}

int fm_tsdf_mesh_emit(const float* tsdf, const int32_t* weight, const float* color, const int32_t* color_weight, int nx, int ny, int nz, float ox, float oy,
                      float oz, float voxel_size, int min_weight, const int64_t* cell_offsets, const int64_t* quad_offsets, long vertex_rows, long quad_rows,
                      float* xyz, float* normals, float* rgb, int64_t* cell, int32_t* cell_vertex, int32_t* faces, int64_t* edge, void* stream) {
  FM_CHECK_ARG(tsdf_mesh_emit_args_ok(tsdf, weight, color, color_weight, nx, ny, nz, ox, oy, oz, voxel_size, min_weight, cell_offsets, quad_offsets,
                                      vertex_rows, quad_rows, xyz, normals, rgb, cell, cell_vertex, faces, edge));
  const long voxels = (long)nx * ny * nz;
  const TsdfGrid g = tsdf_grid(tsdf, weight, color, color_weight, nx, ny, nz, min_weight, ox, oy, oz, voxel_size);
  const dim3 grid((unsigned)tsdf_blocks(voxels));
  if (rgb) hipLaunchKernelGGL(tsdf_mesh_vertex_kernel<true>, grid, dim3(kTsdfThreads), 0, (hipStream_t)stream, g, voxels, cell_offsets, vertex_rows, xyz, normals,
                              rgb, cell, cell_vertex);
  else hipLaunchKernelGGL(tsdf_mesh_vertex_kernel<false>, grid, dim3(kTsdfThreads), 0, (hipStream_t)stream, g, voxels, cell_offsets, vertex_rows, xyz, normals,
                          rgb, cell, cell_vertex);
  if (quad_rows > 0)  // (the same stream: the face pass reads the cell_vertex the vertex pass has just filled)
    hipLaunchKernelGGL(tsdf_mesh_face_kernel, grid, dim3(kTsdfThreads), 0, (hipStream_t)stream, g, voxels, quad_offsets, quad_rows, cell_vertex, faces, edge);
  FM_LAUNCH_STATUS();
}

}  // extern "C"
