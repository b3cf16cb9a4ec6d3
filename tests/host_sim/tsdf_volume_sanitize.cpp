// A stand-alone driver of the host build of fm_tsdf_volume, fm_tsdf_surface_count and fm_tsdf_surface_emit
// (flowmap_amd/csrc/fm_tsdf_volume_host.h) for the sanitizers:
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/host_sim/tsdf_volume_sanitize.cpp -o /tmp/tsdf_volume_sanitize
//   /tmp/tsdf_volume_sanitize
//
// Every buffer is sized exactly.  Cases: (1) three frames of 17 x 23 (no multiple of four) with colours into a 9 x 7 x 5 grid around the
// surface — crossings exist, the emit pass fills exactly the counted rows; (2) the same with a keep mask, depths of 0, NaN, inf and −1, no
// colours and a window of one frame; (3) a 1-voxel grid; (4) a grid no frame sees (behind the cameras): weight 0, tsdf exactly 1, the
// count pass reports zero crossings and the emit pass is not needed; (5) 257 x 1 x 1: two workgroups, the second holding one voxel.
// Exit status 0: the counts add up and every row was written.
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

static int run(int frames, int height, int width, bool with_colors, bool with_keep, bool spoil, int first, int count, float oz, int nx, int ny, int nz,
               float voxel_size, bool expect_surface, bool expect_unseen) {
  const size_t n = (size_t)frames * height * width, voxels = (size_t)nx * ny * nz;
  std::vector<float> depth(n), k(frames * 9, 0.f), ext(frames * 16, 0.f), colors(with_colors ? n * 3 : 0);
  std::vector<uint8_t> keep(with_keep ? n : 0);
  for (auto& z : depth) z = 1.9f + 0.2f * uniform();
  for (auto& c : colors) c = uniform();
  for (auto& m : keep) m = uniform() < 0.6f;
  if (spoil) {
    depth[3] = 0.f;
    depth[5] = NAN;
    depth[7] = INFINITY;
    depth[n - 1] = -1.f;
  }
  for (int f = 0; f < frames; ++f) {
    float* km = &k[f * 9];
    km[0] = 0.9f, km[2] = 0.5f, km[4] = 1.1f, km[5] = 0.5f, km[8] = 1.f;
    float* e = &ext[f * 16];
    const float a = 0.05f * f;
    e[0] = cosf(a), e[2] = sinf(a), e[5] = 1.f, e[8] = -sinf(a), e[10] = cosf(a), e[15] = 1.f;
    e[3] = 0.05f * f, e[7] = -0.02f * f, e[11] = 0.01f * f;
  }
  std::vector<float> w2c(frames * 16), tsdf(voxels), color(with_colors ? voxels * 3 : 0);
  std::vector<int32_t> weight(voxels), color_weight(with_colors ? voxels : 0);
  const float ox = -0.5f * nx * voxel_size, oy = -0.5f * ny * voxel_size;
  if (fm_tsdf_volume(depth.data(), k.data(), ext.data(), with_colors ? colors.data() : nullptr, with_keep ? keep.data() : nullptr, frames, height, width, first,
                     count, ox, oy, oz, nx, ny, nz, voxel_size, 4.f * voxel_size, 0.f, w2c.data(), tsdf.data(), weight.data(),
                     with_colors ? color.data() : nullptr, with_colors ? color_weight.data() : nullptr, nullptr) != 0)
    return 1;
  long seen = 0;
  for (size_t v = 0; v < voxels; ++v) {
    if (weight[v] < 0 || weight[v] > count || !(tsdf[v] >= -1.f && tsdf[v] <= 1.f)) return 1;
    if (weight[v] == 0 && tsdf[v] != 1.f) return 1;
    if (with_colors && (color_weight[v] < 0 || color_weight[v] > weight[v])) return 1;
    seen += weight[v] > 0;
  }
  if (expect_unseen && seen != 0) return 1;
  long blocks = 0;
  if (fm_tsdf_surface_blocks(nx, ny, nz, &blocks) != 0 || blocks != ((long)voxels + 255) / 256) return 1;
  std::vector<int64_t> counts(blocks), offsets(blocks);
  if (fm_tsdf_surface_count(tsdf.data(), weight.data(), nx, ny, nz, 1, counts.data(), nullptr) != 0) return 1;
  long rows = 0;
  for (long b = 0; b < blocks; ++b) {
    offsets[b] = rows;
    rows += (long)counts[b];
  }
  printf("%d x %d x %d frames, grid %d x %d x %d at %g: %ld voxels seen, %ld crossings in %ld workgroups\n", frames, height, width, nx, ny, nz, voxel_size, seen,
         rows, blocks);
  if (expect_surface != (rows > 0)) return 1;
  if (rows == 0) return 0;  // (the caller does not launch the emit pass for an empty surface: it refuses rows == 0)
  std::vector<float> xyz(rows * 3, NAN), normals(rows * 3, NAN), rgb(with_colors ? rows * 3 : 0, NAN);
  std::vector<int64_t> edge(rows, -1);
  if (fm_tsdf_surface_emit(tsdf.data(), weight.data(), with_colors ? color.data() : nullptr, with_colors ? color_weight.data() : nullptr, nx, ny, nz, ox, oy, oz,
                           voxel_size, 1, offsets.data(), rows, xyz.data(), normals.data(), with_colors ? rgb.data() : nullptr, edge.data(), nullptr) != 0)
    return 1;
  for (long r = 0; r < rows; ++r) {
    if (edge[r] < 0 || edge[r] >= (int64_t)voxels * 3 || (r > 0 && edge[r] <= edge[r - 1])) return 1;  // written, in range, ascending
    for (int a = 0; a < 3; ++a)
      if (std::isnan(xyz[r * 3 + a]) || std::isnan(normals[r * 3 + a]) || (with_colors && std::isnan(rgb[r * 3 + a]))) return 1;
  }
  return 0;
}

int main() {
  if (run(3, 17, 23, true, false, false, 0, 3, 1.6f, 9, 7, 5, 0.16f, true, false) != 0) return 1;
  if (run(3, 17, 23, false, true, true, 1, 1, 1.6f, 9, 7, 5, 0.16f, true, false) != 0) return 1;
  if (run(2, 5, 7, true, false, false, 0, 2, 1.9f, 1, 1, 1, 0.2f, false, false) != 0) return 1;
  if (run(3, 8, 16, true, false, false, 0, 3, -9.f, 6, 5, 4, 0.25f, false, true) != 0) return 1;
  if (run(2, 8, 16, true, false, false, 0, 2, 1.95f, 257, 1, 1, 0.004f, false, false) != 0) return 1;
  puts("ok");
  return 0;
}
