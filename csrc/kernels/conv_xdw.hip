// Wide-window depthwise convolution (gfx950): groups == C == K, one filter per channel, NHWC bf16,
// windows whose dilated extents (R - 1) dh + 1 and (S - 1) dw + 1 are at most 7 — the 5x5 and 7x7
// layers of MnasNet / EfficientNet / MixNet / MobileNetV3 and DeepLab's dilated 3x3.
//
// conv_dw.hip keeps a lane's 72 weights in registers and reads every tap from global memory; at
// 7x7 that would be 392 registers and 49 reads of each element.  Here a block keeps both the
// source patch and the weights of its channel tile in LDS:
//   forward   y = relu?(sum_rs x w + bias)
//   dgrad     dx = sum over the taps that reach the input pixel, gathered — nothing is scattered;
//             dx = 0 where gate <= 0
//   wgrad     pass 1: per-(slab, channel) R S tap sums and the dy sum; finalize: the slabs in a
//             fixed order -> fp32 dw[C][R][S], db[C]
//
// Geometry: C % 8 == 0, strides 1 or 2 per axis, any pad, dilation only with both strides 1.  The
// weights are read in place as [C][R][S] bf16.
//
// Work split.  A block of 256 lanes is 4 channel lanes (8 channels each: a tile of CT = 32
// channels, 64 contiguous bytes per pixel) x 64 pixel lanes.  A tile of the written tensor is
// TN images x TH rows x TW columns (TW a multiple of 4, at most 32), sized on the host so that
// the patch it reads — PH x PW source pixels per image, PH = (TH - 1) sh + extent for the forward —
// fits the patch buffer; small images (14 x 14, 7 x 7) put several images in one tile.  A
// block stages the patch with 16-byte loads, zeros outside the image, rows at an odd pitch (lanes
// take the strips of a tile rows-first, so neighbouring lanes read rows an odd number of 64-byte
// pixels apart and spread over the LDS banks), and its tile's weights once as fp32 [tap][channel]:
// a tap's 8 weights of a lane are two 16-byte reads that all pixel lanes share.  Blocks are
// persistent over pixel tiles (grid.y) and keep their channel tile (grid.x), so the weights are
// staged once per block.  LDS: 48 KB patch + 6.1 KB weights (forward, dgrad), 32 + 16 KB (wgrad):
// two blocks and more per CU's 160 KB.  The largest patch, 7x7 at stride 2, fits from a 7 x 16 tile.
//
// conv_xdw_slide_k<SW, S> (forward; data gradient at stride 1, which is the forward over the
// flipped taps with pad' = extent - 1 - pad): a lane computes strips of 4 neighbouring outputs of a
// row.  Per tap row it reads that row's S weights, then each of the strip's 3 SW + S patch columns
// once, unpacks it once and slides the window: column c feeds output j through tap c - j SW.
// S is a template argument for 3, 5 and 7 (S = 0: any S, uniform guards); column dilation goes to
// the gather kernel.
// conv_xdw_gather_k (data gradient with a stride of 2, and every column-dilated product): per
// strip the tap rows that reach the lane's row are r0, r0 + sh, ... with r0 = (h + ph) mod sh
// decided once per strip, and likewise the tap columns of each of its 4 pixels; the patch row of
// the a-th of them is base - a dh.  The forward is the same walk with r0 = 0, step 1 and base + a dh.
// conv_xdw_wgrad_k<T>: the R S taps do not fit a lane's registers, so they are split over the four
// waves of a block, T consecutive taps each (T = 3, 7 or 13 >= R S / 4: 5x5 is 7 + 7 + 7 + 4).  This
// departs from a split by tap rows (2 + 1 + 1 + 1 rows for 5x5) because the flat split is balanced
// and needs 104 instead of 112 accumulators at 7x7.  A wave is 4 channel lanes x 16 pixel lanes
// over the staged x patch and dy tile (zeros outside, so no pixel is special); its accumulators
// stay live over all tiles of the block's slab, are combined across the pixel lanes by a fixed
// butterfly and stored as part[slab][tap][C]; the last wave, which has the fewest taps, also forms
// sum dy (part[slab][R S][C]).
//
// Accumulation is fp32; every reduction order is fixed (butterfly, then the finalize launch's
// lanes over contiguous runs of slabs, then the lanes in lane order).  No float atomics.  Element
// offsets are 64-bit; pixel, tile and strip indices stay below 2^31 (checked by geometry()).
#include "common.h"

namespace {

enum { GRAD_SKIP = 0, GRAD_STORE = 1, GRAD_ACC = 2 };
constexpr int CT = 32;          // channels of a block's tile
constexpr int CL = CT / 8;      // channel lanes
constexpr int PL = 256 / CL;    // pixel lanes of a block
constexpr int WPL = 64 / CL;    // pixel lanes of a wave
constexpr int QS = 4;           // pixels of a strip
constexpr int EMAX = 7;         // largest dilated extent
constexpr int IO_OUT = 512, IO_PATCH = 768;    // pixels of a tile / of its patch: forward, dgrad
constexpr int RED_OUT = 256, RED_PATCH = 512;  // weight gradient
constexpr int FO = 8;           // finalize block: FO outputs x FL slab lanes
constexpr int FL = 32;

struct Geo {
  int N, C;
  int IH, IW;  // rows, columns of the staged tensor
  int OH, OW;  // of the written tensor (wgrad: of dy)
  int R, S, sh, sw, ph, pw, dh, dw, eh, ew;
  int TN, TH, TW, PH, PW, pitch, nsw;  // tile, its patch, strips per tile row
  int tiles_h, tiles_w, ntiles, tps;   // tps: tiles per slab (wgrad)
  FDiv fph, fpw, fth, ftw, fnsw, ftiles_h, ftiles_w;
};

// ceil(a / s) for s in {1, 2}, any sign of a
SN_DEV int cdiv12(int a, int s) { return s == 2 ? (a + 1) >> 1 : a; }

// Stage TN images x rows x cols pixels x CT channels of src[N][SH][SW][C], first image n0, origin
// (ro, co), zeros outside the tensor: pixel (img, r, c) goes to dst[((img * rows + r) * pitch + c) * CL].
SN_DEV void stage(const bf16_t* __restrict__ src, uint4* dst, int N, int SH, int SW, int C, int cblk, int n0, int TN,
                  int ro, int co, int rows, int cols, int pitch, const FDiv& frows, const FDiv& fcols) {
  const int chunk = threadIdx.x & (CL - 1);
  const int c = cblk + chunk * 8;
  const int total = TN * rows * cols;
  for (int i = threadIdx.x / CL; i < total; i += PL) {
    const uint32_t line = udiv((uint32_t)i, fcols);
    const int pc = i - (int)line * cols;
    const int img = (int)udiv(line, frows);
    const int pr = (int)line - img * rows;
    const int n = n0 + img, h = ro + pr, w = co + pc;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (c < C && n < N && h >= 0 && h < SH && w >= 0 && w < SW)
      v = *reinterpret_cast<const uint4*>(src + (((long long)n * SH + h) * SW + w) * C + c);
    dst[((img * rows + pr) * pitch + pc) * CL + chunk] = v;
  }
}

// The tile's weights as fp32 [tap][CT]; flip: tap (r, s) holds w[R - 1 - r][S - 1 - s].
SN_DEV void stage_w(const bf16_t* __restrict__ w, float* dst, int RS, int C, int cblk, bool flip) {
  for (int i = threadIdx.x; i < RS * CT; i += 256) {
    const int tap = i / CT, c = cblk + (i & (CT - 1));
    dst[i] = c < C ? bf2f(w[(long long)c * RS + (flip ? RS - 1 - tap : tap)]) : 0.f;
  }
}

struct Tile {
  int n0, h0, w0;
};

SN_DEV Tile tile_of(const Geo& g, int t) {
  const uint32_t a = udiv((uint32_t)t, g.ftiles_w);
  const uint32_t b = udiv(a, g.ftiles_h);
  Tile r;
  r.w0 = (t - (int)a * g.tiles_w) * g.TW;
  r.h0 = ((int)a - (int)b * g.tiles_h) * g.TH;
  r.n0 = (int)b * g.TN;
  return r;
}

// strip st of a tile, rows first: image, row, first column, all tile-local
SN_DEV void strip_of(const Geo& g, int st, int& img, int& hl, int& wl) {
  const uint32_t a = udiv((uint32_t)st, g.fth);
  hl = st - (int)a * g.TH;
  img = (int)udiv(a, g.fnsw);
  wl = ((int)a - img * g.nsw) * QS;
}

SN_DEV void load8(const float* p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// ReLU and the gate of a strip's accumulators (they start from the bias), then 16-byte stores
SN_DEV void store_strip(const Geo& g, float (*acc)[8], int relu, const bf16_t* __restrict__ gate,
                        bf16_t* __restrict__ out, int n, int h, int w, int c) {
  const long long o = (((long long)n * g.OH + h) * g.OW + w) * g.C + c;
#pragma unroll
  for (int j = 0; j < QS; ++j) {
    if (w + j >= g.OW) break;  // the strip tail
    const long long e = o + (long long)j * g.C;
    if (relu) {
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[j][k] = fmaxf(acc[j][k], 0.f);
    }
    if (gate) {
      float gv[8];
      unpack8(*reinterpret_cast<const uint4*>(gate + e), gv);
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[j][k] = gv[k] > 0.f ? acc[j][k] : 0.f;
    }
    *reinterpret_cast<uint4*>(out + e) = pack8(acc[j]);
  }
}

// ---------------------------------------------------------------------------------------
// Forward (and the stride-1 data gradient as the forward over flipped taps): sliding window
// ---------------------------------------------------------------------------------------
template <int SW, int S_>
__global__ void __launch_bounds__(256) conv_xdw_slide_k(const bf16_t* __restrict__ src, const bf16_t* __restrict__ w,
                                                        const float* __restrict__ bias,
                                                        const bf16_t* __restrict__ gate, bf16_t* __restrict__ out,
                                                        const Geo g, int relu, int flip) {
  __shared__ uint4 sp[IO_PATCH * CL];
  __shared__ float swt[EMAX * EMAX * CT];
  constexpr int SM = S_ ? S_ : EMAX;
  constexpr int NC = (QS - 1) * SW + SM;
  const int cblk = blockIdx.x * CT, cl = threadIdx.x & (CL - 1), pl = threadIdx.x / CL;
  const int c = cblk + cl * 8;
  const bool act = c < g.C;  // C % 8 == 0: an active lane's 8 channels are all inside
  stage_w(w, swt, g.R * g.S, g.C, cblk, flip != 0);
  float bv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) bv[k] = (bias && act) ? bias[c + k] : 0.f;
  const int nstrips = g.TN * g.TH * g.nsw;
  const int ncols = (QS - 1) * SW + g.S;
  for (int t = blockIdx.y; t < g.ntiles; t += gridDim.y) {
    const Tile tl = tile_of(g, t);
    __syncthreads();  // the previous tile's reads
    stage(src, sp, g.N, g.IH, g.IW, g.C, cblk, tl.n0, g.TN, tl.h0 * g.sh - g.ph, tl.w0 * SW - g.pw, g.PH, g.PW, g.pitch,
          g.fph, g.fpw);
    __syncthreads();
    if (!act) continue;
    for (int st = pl; st < nstrips; st += PL) {
      int img, hl, wl;
      strip_of(g, st, img, hl, wl);
      const int n = tl.n0 + img, h = tl.h0 + hl, wq = tl.w0 + wl;
      if (n >= g.N || h >= g.OH || wq >= g.OW) continue;
      float acc[QS][8];
#pragma unroll
      for (int j = 0; j < QS; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[j][k] = bv[k];
      const uint4* row = sp + ((img * g.PH + hl * g.sh) * g.pitch + wl * SW) * CL + cl;
      const float* wr = swt + cl * 8;
      for (int r = 0; r < g.R; ++r, row += g.dh * g.pitch * CL, wr += g.S * CT) {
        float wv[SM][8];
#pragma unroll
        for (int s = 0; s < SM; ++s)
          if (S_ || s < g.S) load8(wr + s * CT, wv[s]);
#pragma unroll
        for (int ci = 0; ci < NC; ++ci) {
          if (S_ || ci < ncols) {
            float f[8];
            unpack8(row[ci * CL], f);
#pragma unroll
            for (int j = 0; j < QS; ++j) {
              const int s = ci - j * SW;
              if (s >= 0 && s < SM && (S_ || s < g.S)) {
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[j][k] = fmaf(f[k], wv[s][k], acc[j][k]);
              }
            }
          }
        }
      }
      store_strip(g, acc, relu, gate, out, n, h, wq, c);
    }
  }
}

// ---------------------------------------------------------------------------------------
// The general walk: the data gradient in gather form (input pixel (h, w) receives
// dy[(h + ph - r dh) / sh][(w + pw - s dw) / sw] w[r][s] from every tap whose quotients are exact;
// the staged dy patch is zero outside the output), and the column-dilated forward.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) conv_xdw_gather_k(const bf16_t* __restrict__ src, const bf16_t* __restrict__ w,
                                                         const float* __restrict__ bias,
                                                         const bf16_t* __restrict__ gate, bf16_t* __restrict__ out,
                                                         const Geo g, int relu, int dgrad) {
  __shared__ uint4 sp[IO_PATCH * CL];
  __shared__ float swt[EMAX * EMAX * CT];
  const int cblk = blockIdx.x * CT, cl = threadIdx.x & (CL - 1), pl = threadIdx.x / CL;
  const int c = cblk + cl * 8;
  const bool act = c < g.C;
  stage_w(w, swt, g.R * g.S, g.C, cblk, false);
  float bv[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) bv[k] = (bias && act) ? bias[c + k] : 0.f;
  const int nstrips = g.TN * g.TH * g.nsw;
  const int rstep = dgrad ? g.sh : 1, sstep = dgrad ? g.sw : 1;
  const int rinc = dgrad ? -g.dh : g.dh, cinc = dgrad ? -g.dw : g.dw;
  for (int t = blockIdx.y; t < g.ntiles; t += gridDim.y) {
    const Tile tl = tile_of(g, t);
    const int ro = dgrad ? cdiv12(tl.h0 + g.ph - (g.eh - 1), g.sh) : tl.h0 * g.sh - g.ph;
    const int co = dgrad ? cdiv12(tl.w0 + g.pw - (g.ew - 1), g.sw) : tl.w0 * g.sw - g.pw;
    __syncthreads();
    stage(src, sp, g.N, g.IH, g.IW, g.C, cblk, tl.n0, g.TN, ro, co, g.PH, g.PW, g.pitch, g.fph, g.fpw);
    __syncthreads();
    if (!act) continue;
    for (int st = pl; st < nstrips; st += PL) {
      int img, hl, wl;
      strip_of(g, st, img, hl, wl);
      const int n = tl.n0 + img, h = tl.h0 + hl, wq = tl.w0 + wl;
      if (n >= g.N || h >= g.OH || wq >= g.OW) continue;
      // tap rows r0, r0 + rstep, ... at patch rows rbase, rbase + rinc, ...; per pixel the same in s
      int r0 = 0, rbase = hl * g.sh;
      if (dgrad) {
        r0 = (h + g.ph) & (g.sh - 1);
        rbase = ((h + g.ph - r0 * g.dh) >> (g.sh - 1)) - ro;
      }
      int s0[QS], cbase[QS];
#pragma unroll
      for (int j = 0; j < QS; ++j) {
        s0[j] = 0;
        cbase[j] = (wl + j) * g.sw;
        if (dgrad) {
          s0[j] = (wq + j + g.pw) & (g.sw - 1);
          cbase[j] = ((wq + j + g.pw - s0[j] * g.dw) >> (g.sw - 1)) - co;
        }
      }
      float acc[QS][8];
#pragma unroll
      for (int j = 0; j < QS; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[j][k] = bv[k];
      const uint4* row = sp + ((img * g.PH + rbase) * g.pitch) * CL + cl;
      for (int r = r0; r < g.R; r += rstep, row += rinc * g.pitch * CL) {
        const float* wr = swt + r * g.S * CT + cl * 8;
#pragma unroll
        for (int j = 0; j < QS; ++j) {
          const uint4* px = row + cbase[j] * CL;
          for (int s = s0[j]; s < g.S; s += sstep, px += cinc * CL) {
            float f[8], wv[8];
            unpack8(*px, f);
            load8(wr + s * CT, wv);
#pragma unroll
            for (int k = 0; k < 8; ++k) acc[j][k] = fmaf(f[k], wv[k], acc[j][k]);
          }
        }
      }
      store_strip(g, acc, relu, gate, out, n, h, wq, c);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Weight / bias gradient pass 1: part[slab][k][C], k = r * S + s: sum dy x(tap), k = R S: sum dy
// ---------------------------------------------------------------------------------------
template <int T_>
__global__ void __launch_bounds__(256) conv_xdw_wgrad_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                        float* __restrict__ part, const Geo g) {
  __shared__ uint4 sx[RED_PATCH * CL];
  __shared__ uint4 sd[RED_OUT * CL];
  const int cblk = blockIdx.x * CT, lane = threadIdx.x & 63, cl = lane & (CL - 1), pxl = lane / CL;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = cblk + cl * 8;
  const int RS = g.R * g.S, tap0 = wave * T_;
  // patch offset of the wave's t-th tap; a tap past the window reads pixel 0 and is never stored
  int off[T_];
#pragma unroll
  for (int t = 0; t < T_; ++t) {
    const int tap = tap0 + t, r = tap / g.S, s = tap - r * g.S;
    off[t] = tap < RS ? (r * g.dh * g.pitch + s * g.dw) * CL : 0;
  }
  float acc[T_][8], sum[8];
#pragma unroll
  for (int t = 0; t < T_; ++t)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[t][k] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) sum[k] = 0.f;
  const int npx = g.TN * g.TH * g.TW;
  const int t1 = min(g.ntiles, ((int)blockIdx.y + 1) * g.tps);
  for (int t = blockIdx.y * g.tps; t < t1; ++t) {
    const Tile tl = tile_of(g, t);
    __syncthreads();
    stage(x, sx, g.N, g.IH, g.IW, g.C, cblk, tl.n0, g.TN, tl.h0 * g.sh - g.ph, tl.w0 * g.sw - g.pw, g.PH, g.PW, g.pitch,
          g.fph, g.fpw);
    stage(dy, sd, g.N, g.OH, g.OW, g.C, cblk, tl.n0, g.TN, tl.h0, tl.w0, g.TH, g.TW, g.TW, g.fth, g.ftw);
    __syncthreads();
    if (tap0 >= RS && wave != 3) continue;  // a wave without taps (uniform)
    for (int p = pxl; p < npx; p += WPL) {
      const uint32_t a = udiv((uint32_t)p, g.ftw);
      const int wl = p - (int)a * g.TW;
      const int img = (int)udiv(a, g.fth);
      const int hl = (int)a - img * g.TH;
      float d[8];
      unpack8(sd[p * CL + cl], d);
      if (wave == 3) {
#pragma unroll
        for (int k = 0; k < 8; ++k) sum[k] += d[k];
      }
      const uint4* xb = sx + ((img * g.PH + hl * g.sh) * g.pitch + wl * g.sw) * CL + cl;
#pragma unroll
      for (int tp = 0; tp < T_; ++tp) {
        float f[8];
        unpack8(xb[off[tp]], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[tp][k] = fmaf(d[k], f[k], acc[tp][k]);
      }
    }
  }
  // the pixel lanes of the wave (lanes CL apart share their channels) by a fixed butterfly
  float* dst = part + (long long)blockIdx.y * (RS + 1) * g.C + c;
#pragma unroll
  for (int tp = 0; tp <= T_; ++tp) {
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = tp < T_ ? acc[tp < T_ ? tp : 0][k] : sum[k];
#pragma unroll
    for (int o = CL; o < 64; o <<= 1) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] += __shfl_xor(v[k], o, 64);
    }
    const int tap = tp < T_ ? tap0 + tp : RS;
    if (pxl == 0 && c < g.C && (tp < T_ ? tap < RS : wave == 3)) {
      float* d = dst + (long long)tap * g.C;
      *reinterpret_cast<float4*>(d) = make_float4(v[0], v[1], v[2], v[3]);
      *reinterpret_cast<float4*>(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
  }
}

// Slab sums in a fixed order; output o = k * C + c of the NQ * C per-slab partials goes to
// dw[c][k] (k < NQ - 1) or db[c] (k == NQ - 1), stored, accumulated or skipped.
__global__ void __launch_bounds__(FO * FL) conv_xdw_wgrad_finalize_k(const float* __restrict__ part, int slabs, int C,
                                                                     int NQ, float* __restrict__ dw, int wflag,
                                                                     float* __restrict__ db, int bflag) {
  __shared__ float sa[FL][FO];
  const int oj = threadIdx.x % FO, k = threadIdx.x / FO;
  const long long total = (long long)NQ * C;
  const long long o = (long long)blockIdx.x * FO + oj;
  const int chunk = (slabs + FL - 1) / FL, s0 = k * chunk, s1 = min(slabs, s0 + chunk);
  float a = 0.f;
  if (o < total) {
#pragma unroll 4
    for (int s = s0; s < s1; ++s) a += part[(long long)s * total + o];
  }
  sa[k][oj] = a;
  __syncthreads();
  if (k != 0 || o >= total) return;
  for (int q = 1; q < FL; ++q) a += sa[q][oj];
  const int tap = (int)(o / C), c = (int)(o % C);
  if (tap < NQ - 1) {
    if (wflag != GRAD_SKIP) {
      float* d = dw + (long long)c * (NQ - 1) + tap;
      *d = wflag == GRAD_ACC ? *d + a : a;
    }
  } else if (bflag != GRAD_SKIP) {
    db[c] = bflag == GRAD_ACC ? db[c] + a : a;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Output size and the limits of the index arithmetic; false for a geometry the kernels do not
// take.  On success g describes the forward: x staged, y written.
inline bool geometry(long long N, long long H, long long W, long long C, long long R, long long S, long long sh,
                     long long sw, long long ph, long long pw, long long dh, long long dw, Geo& g) {
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 != 0 || R < 1 || S < 1 || dh < 1 || dw < 1) return false;
  if (R > EMAX || S > EMAX || dh > EMAX || dw > EMAX) return false;
  const long long eh = (R - 1) * dh + 1, ew = (S - 1) * dw + 1;
  if (eh > EMAX || ew > EMAX) return false;
  if (sh < 1 || sh > 2 || sw < 1 || sw > 2) return false;
  if ((dh > 1 || dw > 1) && (sh != 1 || sw != 1)) return false;
  const long long lim = 1LL << 30;
  if (ph < 0 || pw < 0 || ph > (1 << 20) || pw > (1 << 20) || C > lim / 16) return false;
  if (H + 2 * ph < eh || W + 2 * pw < ew) return false;
  const long long P = (H + 2 * ph - eh) / sh + 1, Q = (W + 2 * pw - ew) / sw + 1;
  if (N * H * W >= lim || N * P * Q >= lim) return false;
  g.N = (int)N; g.C = (int)C; g.IH = (int)H; g.IW = (int)W; g.OH = (int)P; g.OW = (int)Q;
  g.R = (int)R; g.S = (int)S; g.sh = (int)sh; g.sw = (int)sw; g.ph = (int)ph; g.pw = (int)pw;
  g.dh = (int)dh; g.dw = (int)dw; g.eh = (int)eh; g.ew = (int)ew;
  return true;
}

// The data gradient's geometry from the forward's: dy staged, dx written.
inline Geo dgrad_geo(Geo g) {
  const int P = g.OH, Q = g.OW;
  g.OH = g.IH; g.OW = g.IW; g.IH = P; g.IW = Q;
  return g;
}

// Tile of the written tensor and its patch: at most max_out pixels reading at most max_patch.
// gather: the patch of a strided data gradient, (T + extent - 2) / stride + 1 rows of dy.
inline void plan_tiles(Geo& g, bool gather, int max_out, int max_patch) {
  auto span = [&](int t, int stride, int extent) {
    return gather ? (t + extent - 2) / stride + 1 : (t - 1) * stride + extent;
  };
  int TW = ((g.OW + QS - 1) / QS) * QS;
  if (TW > 32) TW = 32;
  int TH = max_out / TW;
  if (TH > g.OH) TH = g.OH;
  if (TH < 1) TH = 1;
  auto patch = [&]() { return span(TH, g.sh, g.eh) * (span(TW, g.sw, g.ew) | 1); };
  while (patch() > max_patch) {  // 1 x 4 always fits: 7 x 13 pixels at most
    if (TH > 1) --TH; else TW -= QS;
  }
  int TN = max_out / (TH * TW);
  if (TN > max_patch / patch()) TN = max_patch / patch();
  if (TN > g.N) TN = g.N;
  if (TN < 1) TN = 1;
  g.TN = TN; g.TH = TH; g.TW = TW; g.nsw = TW / QS;
  g.PH = span(TH, g.sh, g.eh);
  g.PW = span(TW, g.sw, g.ew);
  g.pitch = g.PW | 1;
  g.tiles_h = (g.OH + TH - 1) / TH;
  g.tiles_w = (g.OW + TW - 1) / TW;
  g.ntiles = ((g.N + TN - 1) / TN) * g.tiles_h * g.tiles_w;  // < 2^30: at most one per pixel
  g.tps = 1;
  g.fph = make_fdiv((uint32_t)g.PH); g.fpw = make_fdiv((uint32_t)g.PW);
  g.fth = make_fdiv((uint32_t)TH); g.ftw = make_fdiv((uint32_t)TW); g.fnsw = make_fdiv((uint32_t)g.nsw);
  g.ftiles_h = make_fdiv((uint32_t)g.tiles_h); g.ftiles_w = make_fdiv((uint32_t)g.tiles_w);
}

inline dim3 grid_of(const Geo& g, int blocks_y, int cap) {
  const int gx = (g.C + CT - 1) / CT;
  int gy = cap / gx;
  if (gy < 1) gy = 1;
  if (gy > blocks_y) gy = blocks_y;
  return dim3((unsigned)gx, (unsigned)gy);
}

// slabs of the weight gradient: contiguous runs of g.tps tiles
inline int plan_slabs(Geo& g) {
  plan_tiles(g, false, RED_OUT, RED_PATCH);
  const int want = (int)grid_of(g, g.ntiles, 1024).y;
  g.tps = (g.ntiles + want - 1) / want;
  return (g.ntiles + g.tps - 1) / g.tps;
}

// forward or data gradient: the sliding-window kernel where it applies, else the general walk
inline void launch_walk(const bf16_t* src, const bf16_t* w, const float* bias, const bf16_t* gate, bf16_t* out, Geo& g,
                        int relu, bool dgrad, hipStream_t st) {
  const bool gather = g.dw != 1 || (dgrad && (g.sh != 1 || g.sw != 1));
  if (dgrad && !gather) {  // the forward over flipped taps with pad' = extent - 1 - pad (may be negative)
    g.ph = g.eh - 1 - g.ph;
    g.pw = g.ew - 1 - g.pw;
  }
  plan_tiles(g, gather && dgrad, IO_OUT, IO_PATCH);
  const dim3 grid = grid_of(g, g.ntiles, 2048);
#define SN_XDW_SLIDE(SW, S_) \
  hipLaunchKernelGGL((conv_xdw_slide_k<SW, S_>), grid, dim3(256), 0, st, src, w, bias, gate, out, g, relu, (int)dgrad)
  if (gather) {
    hipLaunchKernelGGL(conv_xdw_gather_k, grid, dim3(256), 0, st, src, w, bias, gate, out, g, relu, (int)dgrad);
  } else if (g.sw == 1) {
    if (g.S == 3) SN_XDW_SLIDE(1, 3);
    else if (g.S == 5) SN_XDW_SLIDE(1, 5);
    else if (g.S == 7) SN_XDW_SLIDE(1, 7);
    else SN_XDW_SLIDE(1, 0);
  } else {
    if (g.S == 3) SN_XDW_SLIDE(2, 3);
    else if (g.S == 5) SN_XDW_SLIDE(2, 5);
    else if (g.S == 7) SN_XDW_SLIDE(2, 7);
    else SN_XDW_SLIDE(2, 0);
  }
#undef SN_XDW_SLIDE
}

}  // namespace

extern "C" {

// Floats the weight-gradient workspace needs; 0 for a geometry the kernels do not take.
long long sn_conv_xdw_part_floats(long long N, long long H, long long W, long long C, long long R, long long S,
                                  long long sh, long long sw, long long ph, long long pw, long long dh, long long dw) {
  Geo g;
  if (!geometry(N, H, W, C, R, S, sh, sw, ph, pw, dh, dw, g)) return 0;
  return (long long)plan_slabs(g) * (R * S + 1) * C;
}

// y[N][P][Q][C] = relu?(depthwise R x S of x[N][H][W][C] with w[C][R][S] + bias); bias may be null.
int sn_conv_xdw_fwd(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, long long N, long long H,
                    long long W, long long C, long long R, long long S, long long sh, long long sw, long long ph,
                    long long pw, long long dh, long long dw, long long relu, hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, R, S, sh, sw, ph, pw, dh, dw, g)) return 3;
  if (!al16(x) || !al16(w) || !al16(y)) return 2;
  launch_walk(x, w, bias, nullptr, y, g, (int)relu, false, st);
  return SN_CHECK_LAUNCH();
}

// dx[N][H][W][C] = the data gradient of dy[N][P][Q][C], zeroed where gate <= 0 (gate shaped like
// dx; may be null).
int sn_conv_xdw_dgrad(const bf16_t* dy, const bf16_t* w, const bf16_t* gate, bf16_t* dx, long long N, long long H,
                      long long W, long long C, long long R, long long S, long long sh, long long sw, long long ph,
                      long long pw, long long dh, long long dw, hipStream_t st) {
  Geo f;
  if (!geometry(N, H, W, C, R, S, sh, sw, ph, pw, dh, dw, f)) return 3;
  if (!al16(dy) || !al16(w) || !al16(gate) || !al16(dx)) return 2;
  Geo g = dgrad_geo(f);
  launch_walk(dy, w, nullptr, gate, dx, g, 0, true, st);
  return SN_CHECK_LAUNCH();
}

// dw[C][R][S] and db[C] (fp32) from dy and x.  dw_flag / db_flag: 0 skip, 1 store, 2 accumulate.
// part: workspace of part_floats >= sn_conv_xdw_part_floats(...) floats.
int sn_conv_xdw_wgrad(const bf16_t* dy, const bf16_t* x, float* part, long long part_floats, float* dw,
                      long long dw_flag, float* db, long long db_flag, long long N, long long H, long long W,
                      long long C, long long R, long long S, long long sh, long long sw, long long ph, long long pw,
                      long long dh, long long dil_w, hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, R, S, sh, sw, ph, pw, dh, dil_w, g)) return 3;
  if (!al16(dy) || !al16(x) || !al16(part)) return 2;
  if ((dw_flag != GRAD_SKIP && !dw) || (db_flag != GRAD_SKIP && !db)) return 2;
  const int slabs = plan_slabs(g), NQ = (int)(R * S) + 1;
  if ((long long)slabs * NQ * C > part_floats) return 3;
  const dim3 grid((unsigned)((g.C + CT - 1) / CT), (unsigned)slabs);
  const int per_wave = (NQ - 1 + 3) / 4;
  if (per_wave <= 3)
    hipLaunchKernelGGL((conv_xdw_wgrad_k<3>), grid, dim3(256), 0, st, dy, x, part, g);
  else if (per_wave <= 7)
    hipLaunchKernelGGL((conv_xdw_wgrad_k<7>), grid, dim3(256), 0, st, dy, x, part, g);
  else
    hipLaunchKernelGGL((conv_xdw_wgrad_k<13>), grid, dim3(256), 0, st, dy, x, part, g);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(conv_xdw_wgrad_finalize_k, dim3((unsigned)(((long long)NQ * C + FO - 1) / FO)), dim3(FO * FL), 0, st,
                     part, slabs, (int)C, NQ, dw, (int)dw_flag, db, (int)db_flag);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
