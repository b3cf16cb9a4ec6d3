// The two facts the fused flow pass's coordinates rest on (fm_math.h), checked exhaustively on the CPU.  Stand-alone: built and run by
// tests/test_pixel_center_exact.py, once plain and once under the sanitizers; or by hand
//   g++ -O2 -std=c++17 -ffp-contract=off tests/host_checks/pixel_center_exact.cpp -o /tmp/pixel_center_exact && /tmp/pixel_center_exact
//
// (a) pixel_center_recip(i, n, 1.0f / n) is pixel_center(i, n), bit for bit, for every length n in 1..kPixelCenterRecipMax and every i < n.
// (b) item_walk reproduces item / items_per_row and item % items_per_row along a thread's items (256 apart), for every items_per_row in
//     1..1024 and 1025, 2048, 4097, iterations 0..7, every starting item of the first three workgroups.
#include <stdio.h>
#include <string.h>

#include "../host_sim/fm_host_sim.cpp"  // the whole serial build of the ABI (fm_math.h's host entries lean on its definitions), compiled into this program

static uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, sizeof u);
  return u;
}

int main() {
  long quotients = 0, quotient_mismatches = 0;
  for (int n = 1; n <= fm::kPixelCenterRecipMax; ++n) {
    const float nf = (float)n, inv = 1.0f / nf;
    for (int i = 0; i < n; ++i) {
      ++quotients;
      if (bits(fm::pixel_center_recip(i, nf, inv)) != bits(fm::pixel_center(i, n))) {
        if (quotient_mismatches++ < 10) printf("pixel_center_recip(%d, %d) = %.9g, pixel_center = %.9g\n", i, n, fm::pixel_center_recip(i, nf, inv), fm::pixel_center(i, n));
      }
    }
  }
  printf("pixel centres: %ld quotients, %ld mismatches\n", quotients, quotient_mismatches);

  const int threads = 256, iters = 8, workgroups = 3;
  long steps = 0, walk_mismatches = 0;
  for (int k = 1; k <= 1024 + 3; ++k) {
    const int extra[3] = {1025, 2048, 4097};
    const int items_per_row = k <= 1024 ? k : extra[k - 1025];
    const int step_div = threads / items_per_row, step_mod = threads % items_per_row;
    for (int start = 0; start < workgroups * threads * iters; ++start) {
      if (start % (threads * iters) >= threads) continue;  // a workgroup's threads start on its first 256 items
      int row = start / items_per_row, col = start - row * items_per_row;
      for (int it = 0; it < iters; ++it) {
        const int item = start + it * threads;
        ++steps;
        if (row != item / items_per_row || col != item % items_per_row) {
          if (walk_mismatches++ < 10) printf("items_per_row %d, item %d: walked to (%d, %d), is (%d, %d)\n", items_per_row, item, row, col, item / items_per_row, item % items_per_row);
        }
        fm::item_walk(row, col, items_per_row, step_div, step_mod);
      }
    }
  }
  printf("item walk: %ld steps, %ld mismatches\n", steps, walk_mismatches);
  return quotient_mismatches || walk_mismatches ? 1 : 0;
}
