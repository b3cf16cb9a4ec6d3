// The ordered two-stage fp64 sum of the residual passes (fm_flow_residuals.hip, fm_alignment_residuals.hip, fm_depth_consistency.hip):
// no atomics.
//
// Stage 1, at the end of the map kernel: a thread has added its terms in fp64; the wave butterfly and the workgroup's wave totals follow
// in fp64, and thread 0 leaves the workgroup's pair of doubles in the workgroup's OWN workspace slot with one 16-byte store.  Stage 2,
// ordered_slot_sums_kernel: a row's slots are added in ascending slot order.  THE ORDER IS THE CONTRACT: which elements a workgroup owns
// depends on the size of a row alone — not on the window, not on the batch — and every addition above the thread happens in a fixed
// order, so a row's sums do not depend on how the first launch was scheduled and are the same bits however the row is reached.
#pragma once

#include "fm_device.h"

namespace fm {

// Stage 1.  Every thread of the workgroup calls it (one __syncthreads); `slot` is the workgroup's own, 16-byte aligned.
template <int THREADS>
__device__ __forceinline__ void block_sum_to_slot(double a, double b, double* slot) {
  __shared__ double red[THREADS / kWave][2];
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = a;
    red[wave][1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double2 tot = make_double2(0.0, 0.0);
    for (int w = 0; w < THREADS / kWave; ++w) {
      tot.x += red[w][0];
      tot.y += red[w][1];
    }
    *reinterpret_cast<double2*>(slot) = tot;  // a plain 16-byte store, no atomics
  }
}

// Stage 1 for a workgroup that owns the same elements in up to ROWS rows (fm_depth_consistency.hip: one row per frame offset).  In round
// `row` every thread calls wave_partial_to_lds — wave butterflies only, no barrier between the rounds —, then, once, every thread calls
// block_rows_to_slots (one __syncthreads): thread r adds row r's wave partials in ascending wave order, exactly the additions of
// block_sum_to_slot, and leaves them in the slot of row r, `slot_stride` doubles after row r − 1's.
template <int THREADS, int ROWS>
struct RowPartials {
  double v[ROWS][THREADS / kWave][2];
};

template <int THREADS, int ROWS>
__device__ __forceinline__ void wave_partial_to_lds(RowPartials<THREADS, ROWS>& lds, int row, double a, double b) {
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    lds.v[row][threadIdx.x >> 6][0] = a;
    lds.v[row][threadIdx.x >> 6][1] = b;
  }
}

template <int THREADS, int ROWS>
__device__ __forceinline__ void block_rows_to_slots(const RowPartials<THREADS, ROWS>& lds, int rows, double* slot0, size_t slot_stride) {
  __syncthreads();
  if ((int)threadIdx.x < rows) {
    double2 tot = make_double2(0.0, 0.0);
    for (int w = 0; w < THREADS / kWave; ++w) {
      tot.x += lds.v[threadIdx.x][w][0];
      tot.y += lds.v[threadIdx.x][w][1];
    }
    *reinterpret_cast<double2*>(slot0 + threadIdx.x * slot_stride) = tot;  // a plain 16-byte store, no atomics
  }
}

// Stage 2.  One workgroup of 64 threads per row of `slots_per_row` slots: the lanes fetch 64 slots at a time, lane 0 adds them in
// ascending order.  (static: defined here once, launched from both sources.)
static __global__ void __launch_bounds__(kWave) ordered_slot_sums_kernel(const double* __restrict__ work, int slots_per_row, double* __restrict__ out_a,
                                                                         double* __restrict__ out_b) {
  __shared__ double2 slots[kWave];
  const double2* mine = reinterpret_cast<const double2*>(work) + (size_t)blockIdx.x * slots_per_row;
  double a = 0.0, b = 0.0;
  for (int base = 0; base < slots_per_row; base += kWave) {
    const int i = base + threadIdx.x;
    if (i < slots_per_row) slots[threadIdx.x] = mine[i];
    __syncthreads();
    if (threadIdx.x == 0) {
      const int have = min(kWave, slots_per_row - base);
      for (int j = 0; j < have; ++j) {
        a += slots[j].x;
        b += slots[j].y;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out_a[blockIdx.x] = a;
    out_b[blockIdx.x] = b;
  }
}

}  // namespace fm
