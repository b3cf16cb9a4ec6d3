// The triangle mesh of a TSDF volume by surface nets (TsdfVolume.mesh; include/flowmap_hip.h: fm_tsdf_mesh_count, fm_tsdf_mesh_emit): ONE
// cell and ONE quad of the finished volume.  Included by fm_tsdf_volume.hip and by fm_tsdf_volume_host.h only, after fm_math.h (whose
// TsdfGrid, tsdf_edge_crosses and tsdf_edge_point these functions call as they are): the device kernels and the serial host twin run the
// same decisions and the same sums in the same order.
//
//   cell c     voxel c is its low corner, the seven voxels at +1 along the axes its other corners; it exists when i+1 < nx, j+1 < ny and
//              k+1 < nz, and is ACTIVE when one of its 12 edges crosses (tsdf_edge_crosses).
//   the edges  in this fixed order: axis a = 0, 1, 2; with b = (a+1)%3 and c = (a+2)%3 the edge along a that starts at the low corner
//              moved by (db, dc) = (0,0), (1,0), (0,1), (1,1) along (b, c).  Bit a·4 + db + 2·dc of tsdf_cell_crossings.
//   vertex     one per active cell: xyz = the fp32 sum, in that order, of the crossing edges' points (tsdf_edge_point) divided by their
//              number; normal = the sum of their normals divided by its length (0 where it has none); rgb = the sum of theirs / number.
//   quad       a crossing edge voxel·3 + a has one when the four cells around it exist: 1 <= index_b <= size_b − 2 and likewise for c.
//              Its corners are the cells at (db, dc) = (−1,−1), (0,−1), (0,0), (−1,0) from the edge's voxel when the tsdf at the edge's low
//              end is negative, in the reverse order otherwise: counter-clockwise seen from up the field, so the triangles (q0, q1, q2) and
//              (q0, q2, q3) face out of the surface, toward the cameras, as the normals of the edge points do.
#pragma once

namespace fm {

FM_HD bool tsdf_cell_exists(const TsdfGrid& g, const int ijk[3]) { return ijk[0] + 1 < g.nx && ijk[1] + 1 < g.ny && ijk[2] + 1 < g.nz; }

// The start of edge (axis, db, dc) of the cell at `voxel`: its linear index and its (i, j, k).  `axis`, db and dc are compile-time
// constants at every call (the loops over them are unrolled), so the indexed stores below are to fixed registers.
FM_HD long tsdf_cell_edge_start(const TsdfGrid& g, long voxel, const int ijk[3], int axis, int db, int dc, int start[3]) {
  const int b = (axis + 1) % 3, c = (axis + 2) % 3;
#pragma unroll
  for (int d = 0; d < 3; ++d) start[d] = ijk[d] + (d == b ? db : (d == c ? dc : 0));  // (selects, as tsdf_pick: no indexed store)
  return voxel + (db ? tsdf_axis_stride(g, b) : 0L) + (dc ? tsdf_axis_stride(g, c) : 0L);
}

// The crossings among the 12 edges of the cell at `voxel`, a bit each (0 where the cell does not exist).
FM_HD int tsdf_cell_crossings(const TsdfGrid& g, long voxel, const int ijk[3]) {
  if (!tsdf_cell_exists(g, ijk)) return 0;
  int bits = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int start[3];
      const long from = tsdf_cell_edge_start(g, voxel, ijk, a, e & 1, e >> 1, start);
      bits |= tsdf_edge_crosses(g, from, start, a) ? 1 << (a * 4 + e) : 0;
    }
  }
  return bits;
}

// The vertex of an active cell (bits != 0) from the points of its crossing edges; rgb is written with `with_color` only.
FM_HD void tsdf_cell_vertex(const TsdfGrid& g, long voxel, const int ijk[3], int bits, bool with_color, float xyz[3], float normal[3], float rgb[3]) {
  FM_NO_CONTRACT
  float sum_p[3] = {0.f, 0.f, 0.f}, sum_n[3] = {0.f, 0.f, 0.f}, sum_c[3] = {0.f, 0.f, 0.f};
  int n = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (!(bits & (1 << (a * 4 + e)))) continue;
      int start[3];
      const long from = tsdf_cell_edge_start(g, voxel, ijk, a, e & 1, e >> 1, start);
      float p[3], q[3], c[3];
      tsdf_edge_point(g, from, start, a, with_color, p, q, c);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        sum_p[d] = sum_p[d] + p[d];
        sum_n[d] = sum_n[d] + q[d];
        if (with_color) sum_c[d] = sum_c[d] + c[d];
      }
      ++n;
    }
  }
  const float count = (float)n;
  const float xx = sum_n[0] * sum_n[0], yy = sum_n[1] * sum_n[1], zz = sum_n[2] * sum_n[2];
  const float length = sqrtf((xx + yy) + zz);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    xyz[d] = sum_p[d] / count;
    normal[d] = length > 0.f ? sum_n[d] / length : 0.f;
    if (with_color) rgb[d] = sum_c[d] / count;
  }
}

// Do the four cells around the edge along `axis` that starts at voxel (i, j, k) exist (the edge itself is inside the grid)?
FM_HD bool tsdf_edge_has_quad(const TsdfGrid& g, const int ijk[3], int axis) {
  const int b = (axis + 1) % 3, c = (axis + 2) % 3;
  return ijk[b] >= 1 && ijk[b] + 2 <= tsdf_axis_size(g, b) && ijk[c] >= 1 && ijk[c] + 2 <= tsdf_axis_size(g, c);
}

// The four cells of the quad of the edge (voxel, axis), in corner order; `low_negative`: the tsdf at `voxel` is negative.
FM_HD void tsdf_quad_cells(const TsdfGrid& g, long voxel, int axis, bool low_negative, long cells[4]) {
  const long sb = tsdf_axis_stride(g, (axis + 1) % 3), sc = tsdf_axis_stride(g, (axis + 2) % 3);
  const long q0 = voxel - sb - sc, q1 = voxel - sc, q2 = voxel, q3 = voxel - sb;
  cells[0] = low_negative ? q0 : q3;
  cells[1] = low_negative ? q1 : q2;
  cells[2] = low_negative ? q2 : q1;
  cells[3] = low_negative ? q3 : q0;
}

// The quads among the three edges of `voxel`, a bit per axis, given the crossings of ITS cell (tsdf_cell_crossings: an edge with a quad
// has index + 2 <= size on its two other axes and, crossing, index + 1 < size on its own, so that cell exists and bit a·4 is the edge).
FM_HD int tsdf_voxel_quads(const TsdfGrid& g, const int ijk[3], int bits) {
  int quads = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) quads |= (bits & (1 << (a * 4))) && tsdf_edge_has_quad(g, ijk, a) ? 1 << a : 0;
  return quads;
}

}  // namespace fm
