// xent_reduce (softmax.hip) run by one 256-thread block of another kernel (the solver tail).
// xent_reduce is one block of 1024 threads: thread v sums rows v, v + 1024, ..., each of its
// 16 waves reduces with wave_sum, thread 0 adds the 16 wave sums in order.  Here thread t
// stands in for threads t, t + 256, t + 512, t + 768 (whole waves map to whole waves: wave
// w of the block plays waves w, w + 4, w + 8, w + 12), so every partial sum is formed from
// the same terms in the same order and the scalar is bitwise xent_reduce's.
#pragma once
#include "common.h"

SN_DEV void xent_reduce_block256(const float* __restrict__ row_loss, const float* __restrict__ row_valid, int M,
                                 int normalize, float outer_num, float* __restrict__ out_loss,
                                 float* __restrict__ out_norm, float* ls, float* vs) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int v = threadIdx.x + 256 * q;
    float l = 0.f, s = 0.f;
    for (int i = v; i < M; i += 1024) {
      l += row_loss[i];
      s += row_valid[i];
    }
    l = wave_sum(l);
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) {
      ls[v >> 6] = l;
      vs[v >> 6] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float L = 0.f, V = 0.f;
    for (int w = 0; w < 16; ++w) { L += ls[w]; V += vs[w]; }
    float norm = normalize ? V : outer_num;
    norm = fmaxf(norm, 1.f);
    out_loss[0] = L / norm;
    out_norm[0] = norm;
  }
}
