// The per-tensor fold of the layer-wise optimizers (lars_ops.hip: clite_lars_norms; lamb_ops.hip: clite_lamb_moments). Both take two squared
// norms per adapted tensor in two fixed-order stages over the update path's item table: every item's workgroup stores its pair of partial sums
// with plain stores, then the kernel below folds each tensor's pairs. One copy, so that the two optimizers cannot drift apart in the order of
// the additions.
#ifndef CLITE_NORM_FOLD_H
#define CLITE_NORM_FOLD_H
#include "vec.h"
#include "clite.h"

namespace clite {

// The workgroup of a tensor's FIRST item folds that tensor's pairs; every other workgroup leaves at once. Thread t adds the pairs of
// the tensor's items t, t + 256, ... in that order (a tensor's items are contiguous in the table, so a thread stops at the first item of
// another slot), then the fixed wave / workgroup fold. The order depends on the tensor's own items only: a launch of a sub-range of the table
// that holds the tensor whole gives the same bits as a launch of the whole table. The embedding's 2862 pairs take 12 trips.
static __global__ __launch_bounds__(256) void norm_fold_kernel(const clite_optim_item* __restrict__ items, uint32_t n_items, const float* __restrict__ partials,
                                                               float* __restrict__ norms, uint32_t n_slots) {
  __shared__ float red[2][4];
  const uint32_t head = blockIdx.x, slot1 = items[head].reserved;
  if (slot1 == 0 || slot1 > n_slots) return;
  if (head > 0 && items[head - 1].reserved == slot1) return;
  float sp = 0.f, sg = 0.f;
  for (uint32_t j = head + threadIdx.x; j < n_items && items[j].reserved == slot1; j += 256) {
    sp += partials[2 * (size_t)j];
    sg += partials[2 * (size_t)j + 1];
  }
  sp = wave_sum(sp);
  sg = wave_sum(sg);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sp; red[1][threadIdx.x >> 6] = sg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    norms[2 * (size_t)(slot1 - 1)] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    norms[2 * (size_t)(slot1 - 1) + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

}  // namespace clite
#endif  // CLITE_NORM_FOLD_H
