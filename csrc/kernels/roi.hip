// Region-of-interest kernels of the detection nets (gfx950): ROIPooling (Fast / Faster R-CNN), ROIAlign
// (Detectron / Caffe2, aligned = false) and SmoothL1Loss, on the NHWC storage.
//
//   x / dx  [N][H][W][C] bf16          rois  [R][5] fp32 (batch index, x1, y1, x2, y2), image coordinates
//   y / dy  [R][PH][PW][C] bf16        argmax [R][PH][PW][C] int32: h * W + w of the maximum, or -1
//
// No atomics, no scratch, no host read: every kernel is deterministic and capturable.  Element offsets are
// 64-bit; pixel and bin indices stay below 2^30 (checked by geometry(), which refuses the launch).  V = 8:
// 16-byte accesses of 8 channels (C % 8 == 0 and aligned pointers); V = 1: one channel per lane.  The file is
// built with -ffp-contract=off: bin edges and sample positions are DEFINED by their fp32 order of operations
// (fp32 3 * (7 / 3) is 7 + 2^-21 and its ceil is 8), so no product may be fused into a following sum.
//
// A ROI is ignored — zeros, argmax -1, no gradient — when its batch index is not in [0, N) or a scaled
// coordinate is not finite or beyond 2^20 in magnitude (upstream aborts on the first; a kernel cannot).
//
// roi_pool_fwd_k<V>, roi_align_fwd_k<V>.  A persistent block owns one (ROI, bin row) at a time; the ROI's
// box and bin sizes are decoded once per item into registers (uniform over the block), the lanes run along
// (pw, channel vector).  ROIPooling: a lane walks the rows of its window with 16-byte loads, maximum by strict
// > in (h, w) order.  ROIAlign: the samples of the bin row, (pw, iy, ix), are decoded one per lane into LDS —
// four corner offsets, four weights — in chunks of 256, and every channel lane of a bin reads them from there.
//
// roi_pool_bwd_k<V>, roi_align_bwd_k<V>: gather form.  A block owns a tile of pixels of one image times all
// channel vectors.  Per chunk of 256 ROIs each lane decodes one ROI and tests its box (grown by one pixel for
// ROIAlign) against the tile; the survivors are compacted into LDS in ROI order (wave ballot + prefix over the
// four waves).  A lane then visits, per survivor, only the bins that can hold its pixel: ROIPooling compares
// the exact bin edges and adds dy where the stored argmax is its pixel; ROIAlign narrows the bin range
// arithmetically, recomputes the samples' corners exactly and adds dy * (sum of its corner weights) / count —
// the weights are separable, so a bin's weight is a row sum times a column sum.  fp32 accumulation in (ROI,
// ph, pw) order, one bf16 rounding; dx is written once for every pixel, zeros included: no memset.
//
// smooth_l1_fwd_k + smooth_l1_sum_k, smooth_l1_bwd_k.  d = in_w (pred - target), f(d) = 0.5 sigma^2 d^2 below
// 1 / sigma^2, else |d| - 0.5 / sigma^2; loss = sum(out_w f) / num.  Per-block partials (the grid depends on
// the element count alone), summed by one block in a fixed order.  pred bf16 or fp32; the rest fp32.
#include <float.h>

#include "row_io.h"

namespace {

constexpr int RC = 256;           // ROIs per staged chunk of the backward kernels: one per lane
constexpr int MAX_GRID = 64;      // ROIAlign samples per bin and axis
constexpr float COORD_MAX = 1048576.f;  // 2^20
constexpr int L1_BLOCKS = 256;    // most partial sums of the SmoothL1 forward

struct Geo {
  int N, H, W, C, R, PH, PW, CV;  // CV: channel vectors of a pixel
  float scale;
  int sampling;
  int TH, TW, tiles_h, tiles_w, ntiles, rounds;  // backward: pixel tile, rounds of 256 (pixel, vector) units
  FDiv fcv, fph, ftw, ftiles_h, ftiles_w;
};

SN_DEV bool coord_ok(float v) { return fabsf(v) <= COORD_MAX; }  // false for NaN

// ROIPooling's integer box: image n, first row / column, bin sizes
struct PoolBox {
  int n, hs, ws;
  float bh, bw;
};

SN_DEV bool pool_box(const float* __restrict__ roi, const Geo& g, PoolBox& b) {
  const float bi = roi[0];
  const float x1 = roi[1] * g.scale, y1 = roi[2] * g.scale, x2 = roi[3] * g.scale, y2 = roi[4] * g.scale;
  if (!(bi >= 0.f && bi < (float)g.N) || !coord_ok(x1) || !coord_ok(y1) || !coord_ok(x2) || !coord_ok(y2)) return false;
  b.n = (int)bi;
  b.ws = (int)roundf(x1);
  b.hs = (int)roundf(y1);
  const int rw = max((int)roundf(x2) - b.ws + 1, 1), rh = max((int)roundf(y2) - b.hs + 1, 1);
  b.bh = (float)rh / (float)g.PH;
  b.bw = (float)rw / (float)g.PW;
  return true;
}

// bin p of an axis: [lo, hi) clipped to [0, L]
SN_DEV void pool_bin(int p, float bin, int start, int L, int& lo, int& hi) {
  lo = min(max((int)floorf((float)p * bin) + start, 0), L);
  hi = min(max((int)ceilf((float)(p + 1) * bin) + start, 0), L);
}

// ROIAlign's box: image n, start, bin sizes and sampling grid per axis
struct AlignBox {
  int n, gh, gw;
  float sh, sw, bh, bw;
};

SN_DEV bool align_box(const float* __restrict__ roi, const Geo& g, AlignBox& b) {
  const float bi = roi[0];
  const float x1 = roi[1] * g.scale, y1 = roi[2] * g.scale, x2 = roi[3] * g.scale, y2 = roi[4] * g.scale;
  if (!(bi >= 0.f && bi < (float)g.N) || !coord_ok(x1) || !coord_ok(y1) || !coord_ok(x2) || !coord_ok(y2)) return false;
  b.n = (int)bi;
  b.sh = y1;
  b.sw = x1;
  const float rw = fmaxf(x2 - x1, 1.f), rh = fmaxf(y2 - y1, 1.f);
  b.bh = rh / (float)g.PH;
  b.bw = rw / (float)g.PW;
  b.gh = g.sampling > 0 ? g.sampling : (int)ceilf(rh / (float)g.PH);
  b.gw = g.sampling > 0 ? g.sampling : (int)ceilf(rw / (float)g.PW);
  b.gh = min(b.gh, MAX_GRID);
  b.gw = min(b.gw, MAX_GRID);
  return true;
}

// sample i of bin p of an axis
SN_DEV float sample_at(float start, int p, float bin, int i, int grid) {
  return start + (float)p * bin + ((float)i + .5f) * bin / (float)grid;
}

// Bilinear corners of coordinate v on an axis of length L: rows lo, hi with weights wl, wh; false outside
// [-1, L] (the sample is zero).
SN_DEV bool axis_corners(float v, int L, int& lo, int& hi, float& wl, float& wh) {
  if (v < -1.f || v > (float)L) return false;
  if (v <= 0.f) v = 0.f;
  lo = (int)v;
  if (lo >= L - 1) {
    lo = hi = L - 1;
    v = (float)lo;
  } else {
    hi = lo + 1;
  }
  wh = v - (float)lo;
  wl = 1.f - wh;
  return true;
}

// ---------------------------------------------------------------------------------------
// ROIPooling forward
// ---------------------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(256) roi_pool_fwd_k(const bf16_t* __restrict__ x, const float* __restrict__ rois,
                                                      bf16_t* __restrict__ y, int* __restrict__ amax, const Geo g) {
  const int items = g.R * g.PH, units = g.PW * g.CV;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int r = (int)udiv((uint32_t)item, g.fph), ph = item - r * g.PH;
    PoolBox b;
    const bool ok = pool_box(rois + (long long)r * 5, g, b);
    int h0 = 0, h1 = 0;
    if (ok) pool_bin(ph, b.bh, b.hs, g.H, h0, h1);
    for (int u = threadIdx.x; u < units; u += 256) {
      const int pw = (int)udiv((uint32_t)u, g.fcv), c = (u - pw * g.CV) * V;
      int w0 = 0, w1 = 0;
      if (ok) pool_bin(pw, b.bw, b.ws, g.W, w0, w1);
      const bool empty = h1 <= h0 || w1 <= w0;
      float m[V];
      int am[V];
#pragma unroll
      for (int k = 0; k < V; ++k) {
        m[k] = empty ? 0.f : -FLT_MAX;
        am[k] = -1;
      }
      if (!empty) {
        for (int h = h0; h < h1; ++h) {
          const long long row = (((long long)b.n * g.H + h) * g.W) * g.C + c;
          for (int w = w0; w < w1; ++w) {
            float f[V];
            ldx<V, 0>(x, row + (long long)w * g.C, f);
#pragma unroll
            for (int k = 0; k < V; ++k) {
              if (f[k] > m[k]) {
                m[k] = f[k];
                am[k] = h * g.W + w;
              }
            }
          }
        }
      }
      const long long o = ((long long)item * g.PW + pw) * g.C + c;
      stx<V, 0>(y, o, m);
      if constexpr (V == 8) {
        int4* d = reinterpret_cast<int4*>(amax + o);
        d[0] = make_int4(am[0], am[1], am[2], am[3]);
        d[1] = make_int4(am[4], am[5], am[6], am[7]);
      } else {
        amax[o] = am[0];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// The backward kernels' tile and compaction
// ---------------------------------------------------------------------------------------
struct Tile {
  int n, h0, w0;
};

SN_DEV Tile tile_of(const Geo& g, int t) {
  const uint32_t a = udiv((uint32_t)t, g.ftiles_w);
  const uint32_t b = udiv(a, g.ftiles_h);
  Tile r;
  r.w0 = (t - (int)a * g.tiles_w) * g.TW;
  r.h0 = ((int)a - (int)b * g.tiles_h) * g.TH;
  r.n = (int)b;
  return r;
}

// Slot of a surviving lane in the block's compacted list, in lane order, or -1; total: the survivors.
// Two barriers; every lane of the block calls it.
SN_DEV int compact(bool keep, int* swave, int& total) {
  const unsigned long long ball = __ballot(keep);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // the previous chunk's readers of the list
  if (lane == 0) swave[wave] = __popcll(ball);
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = swave[q];
    base += q < wave ? n : 0;
    total += n;
  }
  return keep ? base + __popcll(ball & ((1ull << lane) - 1ull)) : -1;
}

// the (pixel, channel vector) unit of a lane in round k of a tile; false past the tile or the image
SN_DEV bool unit_of(const Geo& g, const Tile& tl, int k, int& h, int& w, int& c, int V) {
  const int u = (k << 8) + (int)threadIdx.x;
  const int p = (int)udiv((uint32_t)u, g.fcv);
  c = (u - p * g.CV) * V;
  const int i = (int)udiv((uint32_t)p, g.ftw);
  h = tl.h0 + i;
  w = tl.w0 + p - i * g.TW;
  return i < g.TH && h < g.H && w < g.W;
}

// ---------------------------------------------------------------------------------------
// ROIPooling backward
// ---------------------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(256) roi_pool_bwd_k(const bf16_t* __restrict__ dy, const float* __restrict__ rois,
                                                      const int* __restrict__ amax, bf16_t* __restrict__ dx,
                                                      const Geo g) {
  __shared__ int swave[4], s_r[RC], s_hs[RC], s_ws[RC];
  __shared__ float s_bh[RC], s_bw[RC];
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    const Tile tl = tile_of(g, t);
    for (int k = 0; k < g.rounds; ++k) {
      int h, w, c;
      const bool valid = unit_of(g, tl, k, h, w, c, V);
      float acc[V];
#pragma unroll
      for (int q = 0; q < V; ++q) acc[q] = 0.f;
      for (int r0 = 0; r0 < g.R; r0 += RC) {
        const int r = r0 + (int)threadIdx.x;
        PoolBox b;
        bool keep = false;
        if (r < g.R && pool_box(rois + (long long)r * 5, g, b) && b.n == tl.n) {
          // rows / columns the bins cover: from bin 0's start to the last bin's end, clipped
          int lo, hi, a0, a1;
          pool_bin(0, b.bh, b.hs, g.H, lo, a1);
          pool_bin(g.PH - 1, b.bh, b.hs, g.H, a0, hi);
          keep = lo < tl.h0 + g.TH && hi > tl.h0;
          pool_bin(0, b.bw, b.ws, g.W, lo, a1);
          pool_bin(g.PW - 1, b.bw, b.ws, g.W, a0, hi);
          keep = keep && lo < tl.w0 + g.TW && hi > tl.w0;
        }
        int total;
        const int slot = compact(keep, swave, total);
        if (slot >= 0) {
          s_r[slot] = r; s_hs[slot] = b.hs; s_ws[slot] = b.ws; s_bh[slot] = b.bh; s_bw[slot] = b.bw;
        }
        __syncthreads();
        if (!valid) continue;
        const int me = h * g.W + w;
        for (int s = 0; s < total; ++s) {
          const float bh = s_bh[s], bw = s_bw[s];
          const int hs = s_hs[s], ws = s_ws[s];
          // a superset of the bins that hold the pixel (one bin of slack each way for the fp32 quotient)
          const float dh = (float)(h - hs), dw = (float)(w - ws);
          const int p0 = max((int)floorf(dh / bh) - 1, 0), p1 = min((int)ceilf((dh + 1.f) / bh) + 1, g.PH);
          const int q0 = max((int)floorf(dw / bw) - 1, 0), q1 = min((int)ceilf((dw + 1.f) / bw) + 1, g.PW);
          for (int ph = p0; ph < p1; ++ph) {
            int lo, hi;
            pool_bin(ph, bh, hs, g.H, lo, hi);
            if (h < lo || h >= hi) continue;
            for (int pw = q0; pw < q1; ++pw) {
              pool_bin(pw, bw, ws, g.W, lo, hi);
              if (w < lo || w >= hi) continue;
              const long long o = (((long long)s_r[s] * g.PH + ph) * g.PW + pw) * g.C + c;
              float d[V];
              ldx<V, 0>(dy, o, d);
              if constexpr (V == 8) {
                const int4 a = *reinterpret_cast<const int4*>(amax + o), e = *reinterpret_cast<const int4*>(amax + o + 4);
                const int am[8] = {a.x, a.y, a.z, a.w, e.x, e.y, e.z, e.w};
#pragma unroll
                for (int q = 0; q < 8; ++q) acc[q] += am[q] == me ? d[q] : 0.f;
              } else {
                acc[0] += amax[o] == me ? d[0] : 0.f;
              }
            }
          }
        }
      }
      if (valid) stx<V, 0>(dx, (((long long)tl.n * g.H + h) * g.W + w) * g.C + c, acc);
    }
  }
}

// ---------------------------------------------------------------------------------------
// ROIAlign forward
// ---------------------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(256) roi_align_fwd_k(const bf16_t* __restrict__ x, const float* __restrict__ rois,
                                                       bf16_t* __restrict__ y, const Geo g) {
  __shared__ int s_o[4][256];    // corner pixels of a sample: (lo, lo), (lo, hi), (hi, lo), (hi, hi); [0] < 0: zero
  __shared__ float s_w[4][256];
  const int items = g.R * g.PH, units = g.PW * g.CV;
  const int rounds = (units + 255) >> 8;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int r = (int)udiv((uint32_t)item, g.fph), ph = item - r * g.PH;
    AlignBox b;
    const bool ok = align_box(rois + (long long)r * 5, g, b);
    const int per = ok ? b.gh * b.gw : 0;   // samples of a bin
    const int samples = g.PW * per;         // of the bin row: (pw, iy, ix), <= 2^12 PW
    const float count = (float)max(per, 1);
    for (int k = 0; k < rounds; ++k) {
      const int u = (k << 8) + (int)threadIdx.x;
      const int pw = (int)udiv((uint32_t)u, g.fcv), c = (u - pw * g.CV) * V;
      const bool valid = u < units;
      float acc[V];
#pragma unroll
      for (int q = 0; q < V; ++q) acc[q] = 0.f;
      for (int s0 = 0; s0 < samples; s0 += 256) {
        __syncthreads();  // the previous chunk's readers
        const int s = s0 + (int)threadIdx.x;
        if (s < samples) {
          const int spw = s / per, rest = s - spw * per, iy = rest / b.gw, ix = rest - iy * b.gw;
          int yl, yh, xl, xh;
          float wyl, wyh, wxl, wxh;
          const bool in = axis_corners(sample_at(b.sh, ph, b.bh, iy, b.gh), g.H, yl, yh, wyl, wyh) &&
                          axis_corners(sample_at(b.sw, spw, b.bw, ix, b.gw), g.W, xl, xh, wxl, wxh);
          const int t = threadIdx.x;
          if (in) {
            s_o[0][t] = yl * g.W + xl; s_o[1][t] = yl * g.W + xh; s_o[2][t] = yh * g.W + xl; s_o[3][t] = yh * g.W + xh;
            s_w[0][t] = wyl * wxl; s_w[1][t] = wyl * wxh; s_w[2][t] = wyh * wxl; s_w[3][t] = wyh * wxh;
          } else {
            s_o[0][t] = -1;
          }
        }
        __syncthreads();
        if (!valid) continue;
        // the samples of this lane's bin inside the chunk, in (iy, ix) order
        const int a0 = max(pw * per, s0) - s0, a1 = min((pw + 1) * per, min(s0 + 256, samples)) - s0;
        const long long img = (long long)b.n * g.H * g.W;
        for (int a = a0; a < a1; ++a) {
          if (s_o[0][a] < 0) continue;
          float val[V];
#pragma unroll
          for (int q = 0; q < V; ++q) val[q] = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float f[V];
            ldx<V, 0>(x, (img + s_o[j][a]) * g.C + c, f);
            const float wj = s_w[j][a];
#pragma unroll
            for (int q = 0; q < V; ++q) val[q] = fmaf(wj, f[q], val[q]);
          }
#pragma unroll
          for (int q = 0; q < V; ++q) acc[q] += val[q];
        }
      }
      if (valid) {
#pragma unroll
        for (int q = 0; q < V; ++q) acc[q] = acc[q] / count;
        stx<V, 0>(y, ((long long)item * g.PW + pw) * g.C + c, acc);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// ROIAlign backward
// ---------------------------------------------------------------------------------------
// Bins p0 <= p < p1 of an axis whose samples can have row `px` as a corner: their span meets [px - 1, px + 1]
// (one bin of slack each way for the fp32 quotient).
SN_DEV void align_bins(int px, float start, float bin, int P, int& p0, int& p1) {
  const float lim = (float)P + 2.f;
  const float a = fminf(fmaxf(((float)(px - 1) - start) / bin, -2.f), lim);
  const float e = fminf(fmaxf(((float)(px + 1) - start) / bin, -2.f), lim);
  p0 = max((int)floorf(a) - 1, 0);
  p1 = min((int)floorf(e) + 2, P);
}

// Sum over the samples of bin p of the weight their corners give to row `px`.
SN_DEV float align_weight(int px, float start, int p, float bin, int grid, int L) {
  float wsum = 0.f;
  for (int i = 0; i < grid; ++i) {
    int lo, hi;
    float wl, wh;
    if (!axis_corners(sample_at(start, p, bin, i, grid), L, lo, hi, wl, wh)) continue;
    wsum += (lo == px ? wl : 0.f) + (hi == px ? wh : 0.f);
  }
  return wsum;
}

template <int V>
__global__ void __launch_bounds__(256) roi_align_bwd_k(const bf16_t* __restrict__ dy, const float* __restrict__ rois,
                                                       bf16_t* __restrict__ dx, const Geo g) {
  __shared__ int swave[4], s_r[RC], s_gh[RC], s_gw[RC];
  __shared__ float s_sh[RC], s_sw[RC], s_bh[RC], s_bw[RC];
  for (int t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    const Tile tl = tile_of(g, t);
    for (int k = 0; k < g.rounds; ++k) {
      int h, w, c;
      const bool valid = unit_of(g, tl, k, h, w, c, V);
      float acc[V];
#pragma unroll
      for (int q = 0; q < V; ++q) acc[q] = 0.f;
      for (int r0 = 0; r0 < g.R; r0 += RC) {
        const int r = r0 + (int)threadIdx.x;
        AlignBox b;
        bool keep = false;
        if (r < g.R && align_box(rois + (long long)r * 5, g, b) && b.n == tl.n) {
          // the samples lie in [start, start + PH bin]; their corners one pixel further at most
          keep = b.sh - 2.f < (float)(tl.h0 + g.TH) && b.sh + (float)g.PH * b.bh + 2.f > (float)tl.h0 &&
                 b.sw - 2.f < (float)(tl.w0 + g.TW) && b.sw + (float)g.PW * b.bw + 2.f > (float)tl.w0;
        }
        int total;
        const int slot = compact(keep, swave, total);
        if (slot >= 0) {
          s_r[slot] = r; s_gh[slot] = b.gh; s_gw[slot] = b.gw;
          s_sh[slot] = b.sh; s_sw[slot] = b.sw; s_bh[slot] = b.bh; s_bw[slot] = b.bw;
        }
        __syncthreads();
        if (!valid) continue;
        for (int s = 0; s < total; ++s) {
          const float sh = s_sh[s], sw = s_sw[s], bh = s_bh[s], bw = s_bw[s];
          const int gh = s_gh[s], gw = s_gw[s];
          const float count = (float)(gh * gw);
          int p0, p1, q0, q1;
          align_bins(h, sh, bh, g.PH, p0, p1);
          align_bins(w, sw, bw, g.PW, q0, q1);
          for (int ph = p0; ph < p1; ++ph) {
            const float wy = align_weight(h, sh, ph, bh, gh, g.H);
            if (wy == 0.f) continue;
            for (int pw = q0; pw < q1; ++pw) {
              const float wx = align_weight(w, sw, pw, bw, gw, g.W);
              if (wx == 0.f) continue;
              const float wgt = wy * wx / count;
              float d[V];
              ldx<V, 0>(dy, (((long long)s_r[s] * g.PH + ph) * g.PW + pw) * g.C + c, d);
#pragma unroll
              for (int q = 0; q < V; ++q) acc[q] = fmaf(wgt, d[q], acc[q]);
            }
          }
        }
      }
      if (valid) stx<V, 0>(dx, (((long long)tl.n * g.H + h) * g.W + w) * g.C + c, acc);
    }
  }
}

// ---------------------------------------------------------------------------------------
// SmoothL1Loss
// ---------------------------------------------------------------------------------------
template <int DT>
SN_DEV float l1_diff(const void* pred, const float* __restrict__ target, const float* __restrict__ in_w, long long i) {
  float p;
  ldx<1, DT>(pred, i, &p);
  const float d = p - target[i];
  return in_w ? in_w[i] * d : d;
}

// part[block] = the block's sum of out_w f(d); thread sums by stride, waves by butterfly, the four wave
// sums in order
template <int DT>
__global__ void __launch_bounds__(256) smooth_l1_fwd_k(const void* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ in_w, const float* __restrict__ out_w,
                                                       float* __restrict__ part, long long n, float sigma2) {
  __shared__ float sw[4];
  const float cut = 1.f / sigma2, half = 0.5f / sigma2;
  float a = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float d = l1_diff<DT>(pred, target, in_w, i), ad = fabsf(d);
    const float f = ad < cut ? 0.5f * sigma2 * d * d : ad - half;
    a += out_w ? out_w[i] * f : f;
  }
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

// loss = (part[0] + part[1] + ...) / num: lane t sums t, t + 64, ..., then the butterfly
__global__ void __launch_bounds__(64) smooth_l1_sum_k(const float* __restrict__ part, int blocks, float num,
                                                      float* __restrict__ loss) {
  float a = 0.f;
  for (int i = threadIdx.x; i < blocks; i += 64) a += part[i];
  a = wave_sum(a);
  if (threadIdx.x == 0) loss[0] = a / num;
}

// dpred = lw / num * in_w out_w f'(d) (bf16 or fp32 as pred), dtarget (fp32, may be null) its negative
template <int DT>
__global__ void __launch_bounds__(256) smooth_l1_bwd_k(const void* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ in_w, const float* __restrict__ out_w,
                                                       const float* __restrict__ lw, void* __restrict__ dpred,
                                                       float* __restrict__ dtarget, long long n, float num,
                                                       float sigma2) {
  const float cut = 1.f / sigma2, sc = lw[0] / num;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float d = l1_diff<DT>(pred, target, in_w, i);
    float gd = fabsf(d) < cut ? sigma2 * d : (float)((d > 0.f) - (d < 0.f));
    gd *= sc;
    if (in_w) gd *= in_w[i];
    if (out_w) gd *= out_w[i];
    if (dpred) stx<1, DT>(dpred, i, &gd);
    if (dtarget) dtarget[i] = -gd;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Sizes and the limits of the index arithmetic; false for a geometry the kernels do not take.
inline bool geometry(long long N, long long H, long long W, long long C, long long R, long long PH, long long PW,
                     float scale, long long sampling, bool vec, Geo& g) {
  const long long lim = 1LL << 30;
  if (N < 1 || H < 1 || W < 1 || C < 1 || R < 1 || PH < 1 || PW < 1 || PH > 4096 || PW > 4096) return false;
  if (N * H * W >= lim || R * PH * PW >= lim || C > (1 << 20) || sampling < 0 || sampling > MAX_GRID) return false;
  if (!(scale > 0.f) || !(scale <= COORD_MAX)) return false;
  g.N = (int)N; g.H = (int)H; g.W = (int)W; g.C = (int)C; g.R = (int)R; g.PH = (int)PH; g.PW = (int)PW;
  g.scale = scale; g.sampling = (int)sampling;
  g.CV = vec ? (int)C / 8 : (int)C;
  if ((long long)g.PW * g.CV >= (1 << 24)) return false;
  g.fcv = make_fdiv((uint32_t)g.CV); g.fph = make_fdiv((uint32_t)g.PH);
  // backward: about 256 / CV pixels of at most 8 columns, 64 pixels at the most
  int tp = 256 / g.CV;
  tp = tp < 1 ? 1 : (tp > 64 ? 64 : tp);
  g.TW = tp < 8 ? tp : 8;
  if (g.TW > g.W) g.TW = g.W;
  g.TH = tp / g.TW;
  if (g.TH > g.H) g.TH = g.H;
  g.tiles_h = cdiv(g.H, g.TH); g.tiles_w = cdiv(g.W, g.TW);
  g.ntiles = g.N * g.tiles_h * g.tiles_w;  // < 2^30: at most one per pixel
  g.rounds = cdiv(g.TH * g.TW * g.CV, 256);
  g.ftw = make_fdiv((uint32_t)g.TW); g.ftiles_h = make_fdiv((uint32_t)g.tiles_h);
  g.ftiles_w = make_fdiv((uint32_t)g.tiles_w);
  return true;
}

inline int persistent(int items) { return sn_blocks(items, 1, sn_cu_count() * 8); }

}  // namespace

extern "C" {

// ROIs per staged chunk of the backward kernels.
int sn_roi_chunk() { return RC; }

// y[R][PH][PW][C] and argmax (int32, h * W + w or -1) of ROIPooling over x[N][H][W][C] and rois[R][5].
int sn_roi_pool_fwd(const bf16_t* x, const float* rois, bf16_t* y, int* amax, long long N, long long H, long long W,
                    long long C, long long R, long long PH, long long PW, float scale, hipStream_t st) {
  if (!x || !rois || !y || !amax) return 2;
  const bool vec = C % 8 == 0 && al16(x) && al16(y) && al16(amax);
  Geo g;
  if (!geometry(N, H, W, C, R, PH, PW, scale, 0, vec, g)) return 3;
  const dim3 grid((unsigned)persistent(g.R * g.PH));
  if (vec) hipLaunchKernelGGL((roi_pool_fwd_k<8>), grid, dim3(256), 0, st, x, rois, y, amax, g);
  else hipLaunchKernelGGL((roi_pool_fwd_k<1>), grid, dim3(256), 0, st, x, rois, y, amax, g);
  return SN_CHECK_LAUNCH();
}

// dx[N][H][W][C], every pixel written, from dy[R][PH][PW][C] and the forward's argmax.
int sn_roi_pool_bwd(const bf16_t* dy, const float* rois, const int* amax, bf16_t* dx, long long N, long long H,
                    long long W, long long C, long long R, long long PH, long long PW, float scale, hipStream_t st) {
  if (!dy || !rois || !amax || !dx) return 2;
  const bool vec = C % 8 == 0 && al16(dy) && al16(dx) && al16(amax);
  Geo g;
  if (!geometry(N, H, W, C, R, PH, PW, scale, 0, vec, g)) return 3;
  const dim3 grid((unsigned)persistent(g.ntiles));
  if (vec) hipLaunchKernelGGL((roi_pool_bwd_k<8>), grid, dim3(256), 0, st, dy, rois, amax, dx, g);
  else hipLaunchKernelGGL((roi_pool_bwd_k<1>), grid, dim3(256), 0, st, dy, rois, amax, dx, g);
  return SN_CHECK_LAUNCH();
}

// y[R][PH][PW][C] of ROIAlign (aligned = false); sampling: samples per bin and axis, 0 = ceil(roi / pooled).
int sn_roi_align_fwd(const bf16_t* x, const float* rois, bf16_t* y, long long N, long long H, long long W, long long C,
                     long long R, long long PH, long long PW, float scale, long long sampling, hipStream_t st) {
  if (!x || !rois || !y) return 2;
  const bool vec = C % 8 == 0 && al16(x) && al16(y);
  Geo g;
  if (!geometry(N, H, W, C, R, PH, PW, scale, sampling, vec, g)) return 3;
  const dim3 grid((unsigned)persistent(g.R * g.PH));
  if (vec) hipLaunchKernelGGL((roi_align_fwd_k<8>), grid, dim3(256), 0, st, x, rois, y, g);
  else hipLaunchKernelGGL((roi_align_fwd_k<1>), grid, dim3(256), 0, st, x, rois, y, g);
  return SN_CHECK_LAUNCH();
}

int sn_roi_align_bwd(const bf16_t* dy, const float* rois, bf16_t* dx, long long N, long long H, long long W, long long C,
                     long long R, long long PH, long long PW, float scale, long long sampling, hipStream_t st) {
  if (!dy || !rois || !dx) return 2;
  const bool vec = C % 8 == 0 && al16(dy) && al16(dx);
  Geo g;
  if (!geometry(N, H, W, C, R, PH, PW, scale, sampling, vec, g)) return 3;
  const dim3 grid((unsigned)persistent(g.ntiles));
  if (vec) hipLaunchKernelGGL((roi_align_bwd_k<8>), grid, dim3(256), 0, st, dy, rois, dx, g);
  else hipLaunchKernelGGL((roi_align_bwd_k<1>), grid, dim3(256), 0, st, dy, rois, dx, g);
  return SN_CHECK_LAUNCH();
}

inline int l1_blocks(long long n) { return sn_blocks(n, 1024, L1_BLOCKS); }

// loss[0] = sum(out_w f(in_w (pred - target))) / num over n elements; pred bf16 (fp32_pred == 0) or fp32;
// in_w / out_w may be null (ones); part: workspace of at least 256 floats.
int sn_smooth_l1_fwd(const void* pred, long long fp32_pred, const float* target, const float* in_w, const float* out_w,
                     float* part, float* loss, long long n, long long num, float sigma, hipStream_t st) {
  if (!pred || !target || !part || !loss) return 2;
  if (n < 1 || num < 1 || !(sigma > 0.f)) return 3;
  const int blocks = l1_blocks(n);
  const float s2 = sigma * sigma;
  if (fp32_pred) hipLaunchKernelGGL((smooth_l1_fwd_k<1>), dim3(blocks), dim3(256), 0, st, pred, target, in_w, out_w, part, n, s2);
  else hipLaunchKernelGGL((smooth_l1_fwd_k<0>), dim3(blocks), dim3(256), 0, st, pred, target, in_w, out_w, part, n, s2);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(smooth_l1_sum_k, dim3(1), dim3(64), 0, st, part, blocks, (float)num, loss);
  return SN_CHECK_LAUNCH();
}

// dpred (the dtype of pred; may be null) = lw[0] / num * in_w out_w f'(d), dtarget (fp32; may be null) = -that.
int sn_smooth_l1_bwd(const void* pred, long long fp32_pred, const float* target, const float* in_w, const float* out_w,
                     const float* lw, void* dpred, float* dtarget, long long n, long long num, float sigma,
                     hipStream_t st) {
  if (!pred || !target || !lw || (!dpred && !dtarget)) return 2;
  if (n < 1 || num < 1 || !(sigma > 0.f)) return 3;
  const int blocks = sn_blocks(n, 256, sn_cu_count() * 8);
  const float s2 = sigma * sigma;
  if (fp32_pred)
    hipLaunchKernelGGL((smooth_l1_bwd_k<1>), dim3(blocks), dim3(256), 0, st, pred, target, in_w, out_w, lw, dpred, dtarget, n, (float)num, s2);
  else
    hipLaunchKernelGGL((smooth_l1_bwd_k<0>), dim3(blocks), dim3(256), 0, st, pred, target, in_w, out_w, lw, dpred, dtarget, n, (float)num, s2);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
