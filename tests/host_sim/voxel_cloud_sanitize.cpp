// A stand-alone driver of the host build of fm_voxel_cloud (flowmap_amd/csrc/fm_voxel_cloud_host.h) for the sanitizers:
//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all tests/host_sim/voxel_cloud_sanitize.cpp -o /tmp/voxel_cloud_sanitize
//   /tmp/voxel_cloud_sanitize
//
// Two cases, every buffer sized exactly: (1) three frames of 17 x 23 (no multiple of four) with colours, details and a table sized to the
// cloud; (2) two frames of 8 x 16 with a keep mask, depths of 0, NaN and inf, no colours, and a capacity of 2 — four slots for dozens of
// voxels, so the probe walk runs its full length, points overflow and rows are drawn past capacity.  Exit status 0: every point accounted for.
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

static int run(int frames, int height, int width, bool with_colors, bool with_keep, bool spoil, double voxel_size, long capacity, bool must_fit) {
  const size_t n = (size_t)frames * height * width;
  std::vector<float> depth(n), kinv(frames * 9, 0.f), ext(frames * 16, 0.f), colors(with_colors ? n * 3 : 0);
  std::vector<uint8_t> keep(with_keep ? n : 0);
  for (auto& z : depth) z = 1.f + uniform();
  for (auto& c : colors) c = uniform();
  for (auto& m : keep) m = uniform() < 0.6f;
  if (spoil) {
    depth[3] = 0.f;
    depth[5] = NAN;
    depth[7] = INFINITY;
    depth[n - 1] = -1.f;
  }
  for (int f = 0; f < frames; ++f) {
    float* k = &kinv[f * 9];
    k[0] = 1.2f, k[2] = -0.6f, k[4] = 0.9f, k[5] = -0.45f, k[8] = 1.f;
    float* e = &ext[f * 16];
    const float a = 0.1f * f;
    e[0] = cosf(a), e[2] = sinf(a), e[5] = 1.f, e[8] = -sinf(a), e[10] = cosf(a), e[15] = 1.f;
    e[3] = 0.05f * f, e[7] = -0.02f * f, e[11] = 0.01f * f;
  }
  long slots = 0, bytes = 0;
  if (fm_voxel_cloud_workspace(capacity, &slots, &bytes) != 0) return 1;
  void* workspace = nullptr;
  if (posix_memalign(&workspace, 64, (size_t)bytes) != 0) return 1;  // (exactly the stated size)
  std::vector<float> xyz(capacity * 3), rgb(with_colors ? capacity * 3 : 0);
  std::vector<int32_t> count(capacity), slot(capacity), pixel_slot(n);
  std::vector<int64_t> first(capacity);
  unsigned long long counters[8];
  const int status = fm_voxel_cloud(depth.data(), kinv.data(), ext.data(), with_colors ? colors.data() : nullptr, with_keep ? keep.data() : nullptr, frames, height,
                                    width, voxel_size, 1, capacity, xyz.data(), with_colors ? rgb.data() : nullptr, count.data(), first.data(), slot.data(),
                                    pixel_slot.data(), counters, workspace, nullptr);
  free(workspace);
  if (status != 0) return 1;
  const unsigned long long rows = counters[0], written = rows < (unsigned long long)capacity ? rows : (unsigned long long)capacity;
  unsigned long long merged = 0, placed = 0;
  for (unsigned long long r = 0; r < written; ++r) merged += (unsigned long long)count[r];
  for (size_t i = 0; i < n; ++i) placed += pixel_slot[i] >= 0;
  const unsigned long long dropped = counters[1] + counters[2] + counters[3] + counters[4];
  printf("%d x %d x %d at %g, capacity %ld: %llu rows, %llu points placed, overflow %llu, masked %llu, invalid %llu, out of range %llu\n", frames, height, width,
         voxel_size, capacity, rows, placed, counters[1], counters[2], counters[3], counters[4]);
  if (placed + dropped != n) return 1;
  if (must_fit && (rows > (unsigned long long)capacity || counters[1] != 0 || merged != placed)) return 1;
  if (!must_fit && counters[1] == 0) return 1;  // (the case is there for the full table)
  return 0;
}

int main() {
  if (run(3, 17, 23, true, false, false, 0.05, 3 * 17 * 23, true) != 0) return 1;
  if (run(2, 8, 16, false, true, true, 0.01, 2, false) != 0) return 1;
  puts("ok");
  return 0;
}
