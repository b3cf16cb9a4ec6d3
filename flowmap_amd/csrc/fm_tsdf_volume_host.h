// TSDF fusion (include/flowmap_hip.h, ABI versions 16 and 17) for a HOST build of the C ABI.
//
// fm_math.h includes this file when it is compiled by a plain host compiler — the serial build of the ABI that the CPU test-suite links
// the package against instead of libflowmap_hip.so — and never under hipcc.  Per voxel and frame it calls tsdf_centre, tsdf_pixel_of,
// tsdf_term and tsdf_finish, per edge tsdf_edge_crosses and tsdf_edge_point (fm_math.h): the very functions the device kernels
// (fm_tsdf_volume.hip) call, in the same order — voxels ascending, frames ascending inside a voxel, edges ascending.  The count pass
// writes the same per-workgroup counts (kTsdfTile voxels each) and the emit pass starts each workgroup at its offset, so the two builds
// take the same `block_counts` / `block_offsets`.  The mesh entries (ABI version 17: fm_tsdf_mesh_count, fm_tsdf_mesh_emit) do the same
// with the per-cell and per-quad functions of fm_tsdf_mesh.h: the vertex pass over all workgroups, then the face pass.
#pragma once

#include <cstddef>

#include "../../include/flowmap_hip.h"
#include "fm_residual_args.h"
#include "fm_tsdf_mesh.h"

extern "C" {

int fm_tsdf_volume(const float* depth, const float* k, const float* ext, const float* colors, const uint8_t* keep, int frames, int height, int width,
                   int first_frame, int count, float ox, float oy, float oz, int nx, int ny, int nz, float voxel_size, float truncation, float near,
                   float* world_to_camera, float* tsdf, int32_t* weight, float* color, int32_t* color_weight, void*) {
  if (!fm::tsdf_volume_args_ok(depth, k, ext, colors, keep, frames, height, width, first_frame, count, ox, oy, oz, nx, ny, nz, voxel_size, truncation, near,
                               world_to_camera, tsdf, weight, color, color_weight))
    return 1;
  for (int f = 0; f < frames; ++f) fm::tsdf_world_to_camera(ext + (size_t)f * 16, world_to_camera + (size_t)f * 16);
  const size_t n = (size_t)height * width;
  size_t voxel = 0;
  for (int kz = 0; kz < nz; ++kz)
    for (int j = 0; j < ny; ++j)
      for (int i = 0; i < nx; ++i, ++voxel) {
        const float c[3] = {fm::tsdf_centre(ox, i, voxel_size), fm::tsdf_centre(oy, j, voxel_size), fm::tsdf_centre(oz, kz, voxel_size)};
        float sum = 0.f, rgb[3] = {0.f, 0.f, 0.f};
        int w = 0, cw = 0;
        for (int f = first_frame; f < first_frame + count; ++f) {
          fm::Pose wc;
          fm::Mat3 km;
          fm::load_pose44(world_to_camera + (size_t)f * 16, wc);
          fm::load_mat3(k + (size_t)f * 9, km);
          float pz;
          const int pixel = fm::tsdf_pixel_of(wc, km, c, near, height, width, pz);
          if (pixel < 0) continue;
          const size_t at = (size_t)f * n + (size_t)pixel;
          if (keep && keep[at] == 0) continue;
          float t;
          bool coloured;
          if (!fm::tsdf_term(depth[at], pz, truncation, t, coloured)) continue;
          sum += t;
          w += 1;
          if (colors && coloured) {
            for (int a = 0; a < 3; ++a) rgb[a] += colors[((size_t)f * 3 + a) * n + (size_t)pixel];
            cw += 1;
          }
        }
        tsdf[voxel] = fm::tsdf_finish(sum, w);
        weight[voxel] = w;
        if (colors) {
          for (int a = 0; a < 3; ++a) color[voxel * 3 + a] = cw > 0 ? rgb[a] / (float)cw : 0.f;
          color_weight[voxel] = cw;
        }
      }
  return 0;
}

int fm_tsdf_surface_blocks(int nx, int ny, int nz, long* blocks) {
  if (!fm::tsdf_surface_blocks_args_ok(nx, ny, nz, blocks)) return 1;
  blocks[0] = fm::tsdf_blocks((long)nx * ny * nz);
  return 0;
}

int fm_tsdf_surface_count(const float* tsdf, const int32_t* weight, int nx, int ny, int nz, int min_weight, int64_t* block_counts, void*) {
  if (!fm::tsdf_surface_count_args_ok(tsdf, weight, nx, ny, nz, min_weight, block_counts)) return 1;
  const fm::TsdfGrid g{tsdf, weight, nullptr, nullptr, nx, ny, nz, min_weight, {0.f, 0.f, 0.f}, 1.f};
  const long voxels = (long)nx * ny * nz, blocks = fm::tsdf_blocks(voxels);
  for (long b = 0; b < blocks; ++b) {
    int64_t total = 0;
    for (long voxel = b * fm::kTsdfTile; voxel < voxels && voxel < (b + 1) * fm::kTsdfTile; ++voxel) {
      int ijk[3];
      fm::tsdf_voxel_ijk(g, voxel, ijk);
      for (int a = 0; a < 3; ++a) total += fm::tsdf_edge_crosses(g, voxel, ijk, a) ? 1 : 0;
    }
    block_counts[b] = total;
  }
  return 0;
}

int fm_tsdf_surface_emit(const float* tsdf, const int32_t* weight, const float* color, const int32_t* color_weight, int nx, int ny, int nz, float ox, float oy,
                         float oz, float voxel_size, int min_weight, const int64_t* block_offsets, long rows, float* xyz, float* normals, float* rgb,
                         int64_t* edge, void*) {
  if (!fm::tsdf_surface_emit_args_ok(tsdf, weight, color, color_weight, nx, ny, nz, ox, oy, oz, voxel_size, min_weight, block_offsets, rows, xyz, normals, rgb,
                                     edge))
    return 1;
  const fm::TsdfGrid g{tsdf, weight, color, color_weight, nx, ny, nz, min_weight, {ox, oy, oz}, voxel_size};
  const long voxels = (long)nx * ny * nz, blocks = fm::tsdf_blocks(voxels);
  for (long b = 0; b < blocks; ++b) {
    long row = (long)block_offsets[b];
    for (long voxel = b * fm::kTsdfTile; voxel < voxels && voxel < (b + 1) * fm::kTsdfTile; ++voxel) {
      int ijk[3];
      fm::tsdf_voxel_ijk(g, voxel, ijk);
      for (int a = 0; a < 3; ++a) {
        if (!fm::tsdf_edge_crosses(g, voxel, ijk, a)) continue;
        if (row >= 0 && row < rows) {
          float colour[3];
          fm::tsdf_edge_point(g, voxel, ijk, a, rgb != nullptr, xyz + row * 3, normals + row * 3, colour);
          if (rgb)
            for (int e = 0; e < 3; ++e) rgb[row * 3 + e] = colour[e];
          edge[row] = (int64_t)voxel * 3 + a;
        }
        ++row;
      }
    }
  }
  return 0;
}

int fm_tsdf_mesh_count(const float* tsdf, const int32_t* weight, int nx, int ny, int nz, int min_weight, int64_t* cell_counts, int64_t* quad_counts, void*) {
  if (!fm::tsdf_mesh_count_args_ok(tsdf, weight, nx, ny, nz, min_weight, cell_counts, quad_counts)) return 1;
  const fm::TsdfGrid g{tsdf, weight, nullptr, nullptr, nx, ny, nz, min_weight, {0.f, 0.f, 0.f}, 1.f};
  const long voxels = (long)nx * ny * nz, blocks = fm::tsdf_blocks(voxels);
  for (long b = 0; b < blocks; ++b) {
    int64_t cells = 0, quads = 0;
    for (long voxel = b * fm::kTsdfTile; voxel < voxels && voxel < (b + 1) * fm::kTsdfTile; ++voxel) {
      int ijk[3];
      fm::tsdf_voxel_ijk(g, voxel, ijk);
      const int bits = fm::tsdf_cell_crossings(g, voxel, ijk);
      if (!bits) continue;
      cells += 1;
      quads += __builtin_popcount(fm::tsdf_voxel_quads(g, ijk, bits));
    }
    cell_counts[b] = cells;
    quad_counts[b] = quads;
  }
  return 0;
}

int fm_tsdf_mesh_emit(const float* tsdf, const int32_t* weight, const float* color, const int32_t* color_weight, int nx, int ny, int nz, float ox, float oy,
                      float oz, float voxel_size, int min_weight, const int64_t* cell_offsets, const int64_t* quad_offsets, long vertex_rows, long quad_rows,
                      float* xyz, float* normals, float* rgb, int64_t* cell, int32_t* cell_vertex, int32_t* faces, int64_t* edge, void*) {
  if (!fm::tsdf_mesh_emit_args_ok(tsdf, weight, color, color_weight, nx, ny, nz, ox, oy, oz, voxel_size, min_weight, cell_offsets, quad_offsets, vertex_rows,
                                  quad_rows, xyz, normals, rgb, cell, cell_vertex, faces, edge))
    return 1;
  const fm::TsdfGrid g{tsdf, weight, color, color_weight, nx, ny, nz, min_weight, {ox, oy, oz}, voxel_size};
  const long voxels = (long)nx * ny * nz, blocks = fm::tsdf_blocks(voxels);
  for (long b = 0; b < blocks; ++b) {  // the vertex pass: every voxel's cell_vertex is written
    long row = (long)cell_offsets[b];
    for (long voxel = b * fm::kTsdfTile; voxel < voxels && voxel < (b + 1) * fm::kTsdfTile; ++voxel) {
      int ijk[3];
      fm::tsdf_voxel_ijk(g, voxel, ijk);
      const int bits = fm::tsdf_cell_crossings(g, voxel, ijk);
      const bool write = bits != 0 && row >= 0 && row < vertex_rows;
      cell_vertex[voxel] = write ? (int32_t)row : -1;
      if (write) {
        float colour[3];
        fm::tsdf_cell_vertex(g, voxel, ijk, bits, rgb != nullptr, xyz + row * 3, normals + row * 3, colour);
        if (rgb)
          for (int e = 0; e < 3; ++e) rgb[row * 3 + e] = colour[e];
        cell[row] = (int64_t)voxel;
      }
      row += bits != 0;
    }
  }
  if (quad_rows == 0) return 0;
  for (long b = 0; b < blocks; ++b) {  // the face pass
    long row = (long)quad_offsets[b];
    for (long voxel = b * fm::kTsdfTile; voxel < voxels && voxel < (b + 1) * fm::kTsdfTile; ++voxel) {
      int ijk[3];
      fm::tsdf_voxel_ijk(g, voxel, ijk);
      const int bits = fm::tsdf_cell_crossings(g, voxel, ijk);
      const int quads = bits ? fm::tsdf_voxel_quads(g, ijk, bits) : 0;
      for (int a = 0; a < 3; ++a) {
        if (!(quads & (1 << a))) continue;
        if (row >= 0 && row < quad_rows) {
          long cells[4];
          fm::tsdf_quad_cells(g, voxel, a, tsdf[voxel] < 0.f, cells);
          const int32_t q[4] = {cell_vertex[cells[0]], cell_vertex[cells[1]], cell_vertex[cells[2]], cell_vertex[cells[3]]};
          int32_t* to = faces + row * 6;
          to[0] = q[0], to[1] = q[1], to[2] = q[2];
          to[3] = q[0], to[4] = q[2], to[5] = q[3];
          edge[row] = (int64_t)voxel * 3 + a;
        }
        ++row;
      }
    }
  }
  return 0;
}

}  // extern "C"
