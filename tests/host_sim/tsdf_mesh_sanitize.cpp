// A stand-alone driver of the host build of fm_tsdf_mesh_count and fm_tsdf_mesh_emit (flowmap_amd/csrc/fm_tsdf_volume_host.h over
// fm_tsdf_mesh.h) for the sanitizers:
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/host_sim/tsdf_mesh_sanitize.cpp -o /tmp/tsdf_mesh_sanitize
//   /tmp/tsdf_mesh_sanitize
//
// Every buffer is sized exactly, and the volumes are hand-made.  Cases: (1) a 1-voxel grid: no cell; (2) a 2 x 2 x 2 grid with one negative
// corner: one active cell, no quad — the emit pass runs without quad_offsets, faces and edge; (3) a 4 x 4 x 4 grid with no crossing;
// (4) a 3 x 3 x 3 grid whose negative voxels are the centre and five of its six neighbours: exactly one quad, around the edge from the
// centre to +x; (5) 257 x 1 x 1 with alternating signs: crossings but no cell, two workgroups, the second holding one voxel; (6) a
// 9 x 7 x 5 grid (a partial second workgroup) of random signs, weights 0 to 2 and colours.  Exit status 0: the counts add up, every
// vertex, face and cell_vertex element was written, and every face indexes a vertex.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fm_host_sim.cpp"  // the whole serial build of the ABI (fm_math.h's host entries lean on its definitions), compiled into this program

static unsigned long long state = 0x9e3779b97f4a7c15ULL;
static float uniform() {  // [0, 1)
  state = state * 6364136223846793005ULL + 1442695040888963407ULL;
  return (float)(state >> 40) / 16777216.f;
}

static int run(const char* what, int nx, int ny, int nz, const std::vector<float>& tsdf, const std::vector<int32_t>& weight, bool with_colors, long expect_vertices,
               long expect_quads) {
  const size_t voxels = (size_t)nx * ny * nz;
  if (tsdf.size() != voxels || weight.size() != voxels) return 1;
  std::vector<float> color(with_colors ? voxels * 3 : 0);
  std::vector<int32_t> color_weight(with_colors ? voxels : 0);
  for (auto& c : color) c = uniform();
  for (auto& w : color_weight) w = uniform() < 0.8f;
  long blocks = 0;
  if (fm_tsdf_surface_blocks(nx, ny, nz, &blocks) != 0 || blocks != ((long)voxels + 255) / 256) return 1;
  std::vector<int64_t> cell_counts(blocks, -1), quad_counts(blocks, -1), cell_offsets(blocks), quad_offsets(blocks);
  if (fm_tsdf_mesh_count(tsdf.data(), weight.data(), nx, ny, nz, 1, cell_counts.data(), quad_counts.data(), nullptr) != 0) return 1;
  long vertices = 0, quads = 0;
  for (long b = 0; b < blocks; ++b) {
    if (cell_counts[b] < 0 || cell_counts[b] > 256 || quad_counts[b] < 0 || quad_counts[b] > 768) return 1;
    cell_offsets[b] = vertices, quad_offsets[b] = quads;
    vertices += (long)cell_counts[b], quads += (long)quad_counts[b];
  }
  printf("%s: %d x %d x %d, %ld vertices, %ld quads in %ld workgroups\n", what, nx, ny, nz, vertices, quads, blocks);
  if ((expect_vertices >= 0 && vertices != expect_vertices) || (expect_quads >= 0 && quads != expect_quads)) return 1;
  if (vertices == 0) return quads == 0 ? 0 : 1;  // (the caller does not launch the emit pass for an empty mesh: it refuses vertex_rows == 0)
  std::vector<float> xyz(vertices * 3, NAN), normals(vertices * 3, NAN), rgb(with_colors ? vertices * 3 : 0, NAN);
  std::vector<int64_t> cell(vertices, -1), edge(quads, -1);
  std::vector<int32_t> cell_vertex(voxels, -2), faces(quads * 6, -1);
  if (fm_tsdf_mesh_emit(tsdf.data(), weight.data(), with_colors ? color.data() : nullptr, with_colors ? color_weight.data() : nullptr, nx, ny, nz, -0.4f, 0.3f, 1.7f,
                        0.1f, 1, cell_offsets.data(), quads ? quad_offsets.data() : nullptr, vertices, quads, xyz.data(), normals.data(),
                        with_colors ? rgb.data() : nullptr, cell.data(), cell_vertex.data(), quads ? faces.data() : nullptr, quads ? edge.data() : nullptr,
                        nullptr) != 0)
    return 1;
  long rows_named = 0;
  for (size_t v = 0; v < voxels; ++v) {
    if (cell_vertex[v] < -1 || cell_vertex[v] >= vertices) return 1;  // every element written: the row, or -1
    if (cell_vertex[v] >= 0 && (cell[cell_vertex[v]] != (int64_t)v || cell_vertex[v] != rows_named++)) return 1;  // rows in ascending cell id
  }
  if (rows_named != vertices) return 1;
  for (long r = 0; r < vertices; ++r)
    for (int a = 0; a < 3; ++a)
      if (std::isnan(xyz[r * 3 + a]) || std::isnan(normals[r * 3 + a]) || (with_colors && std::isnan(rgb[r * 3 + a]))) return 1;
  for (long q = 0; q < quads; ++q) {
    if (edge[q] < 0 || edge[q] >= (int64_t)voxels * 3 || (q > 0 && edge[q] <= edge[q - 1])) return 1;  // written, in range, ascending
    const int32_t* f = &faces[q * 6];
    for (int e = 0; e < 6; ++e)
      if (f[e] < 0 || f[e] >= vertices) return 1;
    if (f[3] != f[0] || f[4] != f[2]) return 1;  // (q0, q1, q2) and (q0, q2, q3)
    if (f[0] == f[1] || f[0] == f[2] || f[0] == f[5] || f[1] == f[2] || f[1] == f[5] || f[2] == f[5]) return 1;  // four distinct vertices
  }
  return 0;
}

int main() {
  const auto ones = [](size_t n) { return std::vector<int32_t>(n, 1); };
  if (run("one voxel", 1, 1, 1, {-0.5f}, ones(1), true, 0, 0) != 0) return 1;
  {
    std::vector<float> t(8, 0.5f);
    t[0] = -0.5f;
    if (run("one cell", 2, 2, 2, t, ones(8), true, 1, 0) != 0) return 1;
  }
  if (run("no crossing", 4, 4, 4, std::vector<float>(64, 0.25f), ones(64), false, 0, 0) != 0) return 1;
  {
    std::vector<float> t(27, 0.5f);
    const int at[6][3] = {{1, 1, 1}, {0, 1, 1}, {1, 0, 1}, {1, 2, 1}, {1, 1, 0}, {1, 1, 2}};
    for (const auto& v : at) t[(v[2] * 3 + v[1]) * 3 + v[0]] = -0.5f;
    if (run("one quad", 3, 3, 3, t, ones(27), true, 8, 1) != 0) return 1;
  }
  {
    std::vector<float> t(257);
    for (int i = 0; i < 257; ++i) t[i] = i % 2 ? 0.3f : -0.3f;
    if (run("a row", 257, 1, 1, t, ones(257), false, 0, 0) != 0) return 1;
  }
  {
    std::vector<float> t(9 * 7 * 5);
    std::vector<int32_t> w(t.size());
    for (auto& x : t) x = uniform() - 0.5f;
    for (auto& x : w) x = (int32_t)(uniform() * 3.f);
    if (run("random", 9, 7, 5, t, w, true, -1, -1) != 0) return 1;
  }
  puts("ok");
  return 0;
}
