// Depthwise transposed convolution (gfx950): the learned-upsampling Deconvolution of the fully
// convolutional segmentation nets (FCN-8s' upscore2 / upscore_pool4 4x4 / 2 and upscore8 16x16 / 8 on
// 21 channels): groups == C == K, one R x S filter per channel, strides 1..8 per axis (free to differ),
// windows 1..16, any pad that leaves an output, no dilation, ANY channel count.  NHWC bf16, weights read
// in place as [C][R][S] bf16, fp32 accumulation.  x[N][P][Q][C] is the layer's bottom, y[N][H][W][C]
// its top, H = (P - 1) sh + R - 2 ph.  And the Crop layer's window copy (crop_k) each way.
//
//   forward   y[n, oh, ow, c] = bias[c] + sum x[n, ih, iw, c] w[c, r, s] over oh + ph - r == ih sh, ...
//   dgrad     dx[n, h, w, c] = sum_rs dy[n, h sh - ph + r, w sw - pw + s, c] w[c, r, s]
//   wgrad     dw[c, r, s] = sum_nhw x[n, h, w, c] dy[n, h sh - ph + r, w sw - pw + s, c], db[c] = sum dy
//
// A block of 256 lanes owns a channel tile (cs = min(C, 32) channels, so the 21 classes are one tile)
// and walks tiles of input cells; blocks are persistent over the tiles (grid.y) and keep their channel
// tile (grid.x), so the tile's weights are staged once per block as fp32 [tap][channel].
//
// conv_updw_fwd_k<VEC>.  Cell (i, j) is the set of output pixels with (oh + ph) / sh == i and
// (ow + pw) / sw == j: the cells partition the output, so a block that writes the footprint of its
// TH x TW cells writes every pixel once — no zero fill, no read-modify-write, no atomics.  A pixel of
// phase a = (oh + ph) % sh has only the taps r = a + sh t, reading x row i - t: at most TR = ceil(R / sh)
// rows, none when R <= a (bias only).  The block stages the x patch, (TH + TR - 1) x (TW + TS - 1) pixels
// with the halo above and to the left and zeros outside the image, as fp32 in LDS, then walks the
// footprint row by row.  The output is sh sw times the input, so the lanes are laid along the stores:
// VEC (C % 8 == 0): a lane owns 8 channels of a pixel, one 16-byte store; otherwise the lanes run along
// the flattened (column, channel) run of an output row, two elements each, paired so that a pair starts
// at an even element of y: a wave stores one contiguous 256-byte span in 4-byte pieces (21 channels
// would otherwise be 42-byte islands).  Tiles aim at 16 x 32 output pixels and shrink until weights
// and patch fit 64 KB.
//
// conv_updw_dgrad_k.  A strided correlation with up to 256 taps per cell, in which a dy element serves
// at most TR TS cells.  The dy patch of a tile, ((TH - 1) sh + R) x ((TW - 1) sw + S) pixels, is staged
// in LDS as bf16 with the channel tile narrow enough that the 16x16 / 8 case fits (2 x 4 cells x 21
// channels: 24 x 40 pixels, 40 KB; the 4x4 / 2 layers take 8 x 16 cells), so dy comes from HBM once per
// block and only the halo is re-read (through L2) by neighbours.  An output is summed by LG = 1..16
// neighbouring lanes that take the tap rows r = l, l + LG, ... and are combined by a fixed butterfly.
//
// conv_updw_wgrad_k<NA> + conv_updw_wgrad_finalize_k.  Same patch; a lane owns up to NA (tap, channel)
// pairs (pair = lane + 256 k) and keeps their fp32 accumulators over all cells of all tiles of its slab
// (a contiguous run of tiles); part[slab][tap][C] holds the slab partials, part[slab][R S][C] the slab's
// sum of dy.  For that sum the patch is staged max(R, sh) rows deep per cell row, so that the patches
// cover the output, and a tile counts the patch rows below (TH sh) (every row for the last tile), which
// assigns each output pixel to exactly one tile.  The finalize launch sums the slabs in a fixed order
// and writes dw[C][R][S] / db[C] in store or accumulate form.  No float atomics anywhere: the result
// is deterministic.
//
// Element offsets are 64-bit; pixel, tile and item indices stay below 2^30 (checked by geometry(),
// which refuses the launch otherwise).
#include "row_io.h"

namespace {

enum { GRAD_SKIP = 0, GRAD_STORE = 1, GRAD_ACC = 2 };
constexpr int CT = 32;               // channels of a block's tile (16 where the forward's LDS needs it)
constexpr int WMAX = 16, SMAX = 8;   // largest window, largest stride
constexpr int LDS_MAX = 64 * 1024;
constexpr int GATHER_PATCH = 40 * 1024;  // bytes of the staged dy patch (dgrad, wgrad)
constexpr int FO = 8, FL = 32;       // finalize block: FO outputs x FL slab lanes

struct Geo {
  int N, C, P, Q, H, W, R, S, sh, sw, ph, pw;
  int cs;                 // channels of a block's tile, and of a pixel in LDS: min(C, CT)
  int TH, TW, PH, PW;     // tile of cells, its patch
  int ci0, cj0;           // first cell row / column (forward)
  int TR, TS;             // forward: taps per phase; gather kernels: patch depth per cell max(R, sh)
  int tiles_h, tiles_w, ntiles, tps, LG;
  FDiv fcs, fsh, fsw, fpw, ftw, ftiles_h, ftiles_w;
};

struct Tile {
  int n, i0, j0;
};

SN_DEV Tile tile_of(const Geo& g, int t) {
  const uint32_t a = udiv((uint32_t)t, g.ftiles_w);
  const uint32_t b = udiv(a, g.ftiles_h);
  Tile r;
  r.j0 = (t - (int)a * g.tiles_w) * g.TW;
  r.i0 = ((int)a - (int)b * g.tiles_h) * g.TH;
  r.n = (int)b;
  return r;
}

// The tile's weights as fp32 [tap][cs], zeros past C.
SN_DEV void stage_w(const bf16_t* __restrict__ w, float* dst, const Geo& g, int c0) {
  const int RS = g.R * g.S;
  for (int i = threadIdx.x; i < RS * g.cs; i += 256) {
    const int tap = (int)udiv((uint32_t)i, g.fcs), c = c0 + i - tap * g.cs;
    dst[i] = c < g.C ? bf2f(w[(long long)c * RS + tap]) : 0.f;
  }
}

// Stage rows x cols pixels x cs channels of image n of src[N][SH][SW][C], origin (ro, co), zeros outside
// the image and past C: pixel (r, c) goes to dst[(r * cols + c) * cs].  OUT: float or bf16_t.  VEC: 16-byte
// loads of 8 channels (C % 8 == 0, so cs % 8 == 0), else one element per lane along the flat run.
template <bool VEC, typename OUT>
SN_DEV void stage(const bf16_t* __restrict__ src, OUT* dst, const Geo& g, int c0, int n, int SH, int SW, int ro, int co,
                  int rows, int cols, const FDiv& fcols) {
  constexpr int V = VEC ? 8 : 1;
  const int upp = g.cs / V;  // units per pixel
  const float iupp = 1.f / (float)upp;
  const int total = rows * cols * upp;  // < 2^24: the patch fits LDS
  for (int i = threadIdx.x; i < total; i += 256) {
    const uint32_t px = VEC ? (uint32_t)fdiv(i, upp, iupp) : udiv((uint32_t)i, g.fcs);
    const int ch = (i - (int)px * upp) * V;
    const int pr = (int)udiv(px, fcols), pc = (int)px - pr * cols;
    const int h = ro + pr, wq = co + pc, c = c0 + ch;
    float f[V];
#pragma unroll
    for (int k = 0; k < V; ++k) f[k] = 0.f;
    if (c < g.C && h >= 0 && h < SH && wq >= 0 && wq < SW)
      ldx<V, 0>(src, (((long long)n * SH + h) * SW + wq) * g.C + c, f);
    OUT* d = dst + (int)px * g.cs + ch;
    if constexpr (VEC && sizeof(OUT) == 2) {
      *reinterpret_cast<uint4*>(d) = pack8(f);  // exact: the values are bf16
    } else {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        if constexpr (sizeof(OUT) == 4) d[k] = f[k]; else d[k] = f2bf(f[k]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------------------
struct FwdRow {
  int a, lr0;     // phase of the output row, patch row of its tap t = 0
  int colbase;    // first patch column's x column
};

// V channels ch.. of output column ow: bias + the taps of the pixel's phase
template <int V>
SN_DEV void fwd_value(const Geo& g, const float* swt, const float* sx, const float* sb, const FwdRow& fr, int ow, int ch,
                      float* acc) {
  const int jw = (int)udiv((uint32_t)(ow + g.pw), g.fsw);
  const int b = ow + g.pw - jw * g.sw;
#pragma unroll
  for (int k = 0; k < V; ++k) acc[k] = sb[ch + k];
  int lr = fr.lr0;
  for (int r = fr.a; r < g.R; r += g.sh, --lr) {
    const float* xr = sx + (lr * g.PW + (jw - fr.colbase)) * g.cs + ch;
    const float* wr = swt + (r * g.S + b) * g.cs + ch;
    for (int s = b; s < g.S; s += g.sw, xr -= g.cs, wr += g.sw * g.cs) {
#pragma unroll
      for (int k = 0; k < V; ++k) acc[k] = fmaf(xr[k], wr[k], acc[k]);
    }
  }
}

template <bool VEC>
__global__ void __launch_bounds__(256) conv_updw_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                       const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                       const Geo g) {
  extern __shared__ float4 smem4[];
  float* swt = reinterpret_cast<float*>(smem4);
  float* sb = swt + g.R * g.S * g.cs;
  float* sx = sb + CT;
  const int c0 = blockIdx.x * g.cs, ct = min(g.cs, g.C - c0);
  stage_w(w, swt, g, c0);
  if (threadIdx.x < CT) sb[threadIdx.x] = (bias && c0 + (int)threadIdx.x < g.C) ? bias[c0 + threadIdx.x] : 0.f;
  for (int t = blockIdx.y; t < g.ntiles; t += gridDim.y) {
    const Tile tl = tile_of(g, t);
    const int ci = g.ci0 + tl.i0, cj = g.cj0 + tl.j0;  // first cell of the tile
    __syncthreads();  // the previous tile's reads
    stage<VEC, float>(x, sx, g, c0, tl.n, g.P, g.Q, ci - (g.TR - 1), cj - (g.TS - 1), g.PH, g.PW, g.fpw);
    __syncthreads();
    // the footprint of the tile's cells, clipped to the output
    const int oh0 = max(0, ci * g.sh - g.ph), oh1 = min(g.H, (ci + g.TH) * g.sh - g.ph);
    const int ow0 = max(0, cj * g.sw - g.pw), ow1 = min(g.W, (cj + g.TW) * g.sw - g.pw);
    const int ncols = ow1 - ow0;
    if (oh1 <= oh0 || ncols <= 0) continue;
    // units of a row: VEC 8-channel chunks, else pairs of the flat (column, channel) run
    const int nch = g.cs >> 3;
    const int upr = VEC ? ncols * nch : (ncols * g.cs + 1) / 2 + 1;
    const float iupr = 1.f / (float)upr, inch = 1.f / (float)(nch > 0 ? nch : 1);
    const int total = (oh1 - oh0) * upr;  // < 2^24: a tile's footprint
    for (int it = threadIdx.x; it < total; it += 256) {
      const int row = fdiv(it, upr, iupr), u = it - row * upr;
      const int oh = oh0 + row;
      FwdRow fr;
      const int iq = (int)udiv((uint32_t)(oh + g.ph), g.fsh);
      fr.a = oh + g.ph - iq * g.sh;
      fr.lr0 = iq - ci + g.TR - 1;
      fr.colbase = cj - (g.TS - 1);
      const long long rowbase = ((long long)tl.n * g.H + oh) * g.W * g.C;
      if constexpr (VEC) {
        const int col = fdiv(u, nch, inch), ch = (u - col * nch) * 8;
        if (ch >= ct) continue;
        float acc[8];
        fwd_value<8>(g, swt, sx, sb, fr, ow0 + col, ch, acc);
        stx<8, 0>(y, rowbase + (long long)(ow0 + col) * g.C + c0 + ch, acc);
      } else {
        // pair u holds run elements e0 = 2 u - par and e0 + 1, par chosen so that a whole-tile run
        // (cs == C) starts its pairs at even elements of y
        const int par = (int)((rowbase + (long long)ow0 * g.C + c0) & 1);
        float v[2];
        long long at[2];
        bool ok[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int e = 2 * u - par + q;
          ok[q] = e >= 0 && e < ncols * g.cs;
          at[q] = 0;
          v[q] = 0.f;
          if (ok[q]) {
            const int col = (int)udiv((uint32_t)e, g.fcs), ch = e - col * g.cs;
            ok[q] = ch < ct;
            if (ok[q]) {
              fwd_value<1>(g, swt, sx, sb, fr, ow0 + col, ch, &v[q]);
              at[q] = rowbase + (long long)(ow0 + col) * g.C + c0 + ch;
            }
          }
        }
        if (ok[0] && ok[1] && at[1] == at[0] + 1 && (at[0] & 1) == 0) {
          *reinterpret_cast<uint32_t*>(y + at[0]) = pack2(v[0], v[1]);
        } else {
          if (ok[0]) y[at[0]] = f2bf(v[0]);
          if (ok[1]) y[at[1]] = f2bf(v[1]);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Bottom gradient
// ---------------------------------------------------------------------------------------
template <bool VEC>
__global__ void __launch_bounds__(256) conv_updw_dgrad_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
                                                         bf16_t* __restrict__ dx, const Geo g) {
  extern __shared__ float4 smem4[];
  float* swt = reinterpret_cast<float*>(smem4);
  bf16_t* sd = reinterpret_cast<bf16_t*>(swt + g.R * g.S * g.cs);
  const int c0 = blockIdx.x * g.cs;
  stage_w(w, swt, g, c0);
  const int lgs = 31 - __builtin_clz(g.LG);  // LG is a power of two
  const int items = (g.TH * g.TW * g.cs) << lgs;
  const int rounds = (items + 255) >> 8;
  const int l = threadIdx.x & (g.LG - 1);
  for (int t = blockIdx.y; t < g.ntiles; t += gridDim.y) {
    const Tile tl = tile_of(g, t);
    __syncthreads();
    stage<VEC, bf16_t>(dy, sd, g, c0, tl.n, g.H, g.W, tl.i0 * g.sh - g.ph, tl.j0 * g.sw - g.pw, g.PH, g.PW, g.fpw);
    __syncthreads();
    for (int k = 0; k < rounds; ++k) {  // the same trip count for every lane: the butterfly below
      const int it = (k << 8) + (int)threadIdx.x;
      const int o = it >> lgs;
      const int cell = (int)udiv((uint32_t)o, g.fcs), ch = o - cell * g.cs;
      const int i = (int)udiv((uint32_t)cell, g.ftw), j = cell - i * g.TW;
      const bool valid = it < items;
      float acc = 0.f;
      if (valid) {
        for (int r = l; r < g.R; r += g.LG) {
          const bf16_t* row = sd + ((i * g.sh + r) * g.PW + j * g.sw) * g.cs + ch;
          const float* wr = swt + r * g.S * g.cs + ch;
          for (int s = 0; s < g.S; ++s) acc = fmaf(bf2f(row[s * g.cs]), wr[s * g.cs], acc);
        }
      }
      for (int q = 1; q < g.LG; q <<= 1) acc += __shfl_xor(acc, q, 64);
      const int h = tl.i0 + i, wq = tl.j0 + j, c = c0 + ch;
      if (valid && l == 0 && h < g.P && wq < g.Q && c < g.C)
        dx[(((long long)tl.n * g.P + h) * g.Q + wq) * g.C + c] = f2bf(acc);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Weight / bias gradient pass 1: part[slab][k][C], k = r * S + s: sum x dy(tap), k = R S: sum dy
// ---------------------------------------------------------------------------------------
template <bool VEC, int NA>
__global__ void __launch_bounds__(256) conv_updw_wgrad_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                         float* __restrict__ part, const Geo g) {
  extern __shared__ float4 smem4[];
  float* sred = reinterpret_cast<float*>(smem4);                 // [256]
  bf16_t* sxs = reinterpret_cast<bf16_t*>(sred + 256);           // [TH TW][cs]
  bf16_t* sd = sxs + ((g.TH * g.TW * g.cs + 7) & ~7);            // [PH PW][cs]
  const int c0 = blockIdx.x * g.cs, tid = threadIdx.x;
  const int RS = g.R * g.S, pairs = RS * g.cs;
  float acc[NA];
#pragma unroll
  for (int k = 0; k < NA; ++k) acc[k] = 0.f;
  const float inv_s = 1.f / (float)g.S;
  // the sum of dy: G lane groups of cs lanes stride over the patch pixels
  const int G = 256 / g.cs, gg = (int)udiv((uint32_t)tid, g.fcs), gch = tid - gg * g.cs;
  float dbs = 0.f;
  const int t1 = min(g.ntiles, ((int)blockIdx.y + 1) * g.tps);
  for (int t = blockIdx.y * g.tps; t < t1; ++t) {
    const Tile tl = tile_of(g, t);
    __syncthreads();
    stage<VEC, bf16_t>(dy, sd, g, c0, tl.n, g.H, g.W, tl.i0 * g.sh - g.ph, tl.j0 * g.sw - g.pw, g.PH, g.PW, g.fpw);
    stage<VEC, bf16_t>(x, sxs, g, c0, tl.n, g.P, g.Q, tl.i0, tl.j0, g.TH, g.TW, g.ftw);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      const int idx = tid + k * 256;
      if (idx < pairs) {
        const int tap = (int)udiv((uint32_t)idx, g.fcs), ch = idx - tap * g.cs;
        const int r = fdiv(tap, g.S, inv_s), s = tap - r * g.S;
        float a = acc[k];
        const bf16_t* xp = sxs + ch;
        const bf16_t* d0 = sd + (r * g.PW + s) * g.cs + ch;
        for (int i = 0; i < g.TH; ++i) {
          const bf16_t* dp = d0 + i * g.sh * g.PW * g.cs;
          for (int j = 0; j < g.TW; ++j, xp += g.cs, dp += g.sw * g.cs) a = fmaf(bf2f(*xp), bf2f(*dp), a);
        }
        acc[k] = a;
      }
    }
    if (gg < G) {
      // patch rows / columns this tile counts: below TH sh (TW sw), all of them for the last tile
      const int hr = tl.i0 + g.TH >= g.P ? g.PH : g.TH * g.sh, hc = tl.j0 + g.TW >= g.Q ? g.PW : g.TW * g.sw;
      const int npx = g.PH * g.PW;
      for (int p = gg; p < npx; p += G) {
        const int pr = (int)udiv((uint32_t)p, g.fpw), pc = p - pr * g.PW;
        if (pr < hr && pc < hc) dbs += bf2f(sd[p * g.cs + gch]);
      }
    }
  }
  float* dst = part + (long long)blockIdx.y * (RS + 1) * g.C;
#pragma unroll
  for (int k = 0; k < NA; ++k) {
    const int idx = tid + k * 256;
    const int tap = (int)udiv((uint32_t)idx, g.fcs), c = c0 + idx - tap * g.cs;
    if (idx < pairs && c < g.C) dst[(long long)tap * g.C + c] = acc[k];
  }
  __syncthreads();
  sred[tid] = dbs;
  __syncthreads();
  if (tid < g.cs && c0 + tid < g.C) {
    float a = 0.f;
    for (int q = 0; q < G; ++q) a += sred[q * g.cs + tid];
    dst[(long long)RS * g.C + c0 + tid] = a;
  }
}

// Slab sums in a fixed order; output o = k * C + c of the NQ * C per-slab partials goes to
// dw[c][k] (k < NQ - 1) or db[c] (k == NQ - 1), stored, accumulated or skipped.
__global__ void __launch_bounds__(FO * FL) conv_updw_wgrad_finalize_k(const float* __restrict__ part, int slabs, int C,
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

// ---------------------------------------------------------------------------------------
// Crop: a window copy between a large tensor big[N][H][W][C] and a small one win[n][h][w][c] that sits
// at offset (on, oh, ow, oc) of it.  Forward (bwd == 0): win = big's window, one unit of V channels
// per lane over win.  Backward: big = win inside the window and zero outside, one unit per lane over
// the whole of big, so no separate clear is needed.  V = 8: 16-byte moves (both channel counts and
// the channel offset multiples of 8).
// ---------------------------------------------------------------------------------------
struct CropGeo {
  int H, W, C, n, h, w, c, on, oh, ow, oc;
  FDiv fw, fh;  // columns, rows of the tensor the lanes run over
};

template <int V>
__global__ void __launch_bounds__(256) crop_k(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, const CropGeo g,
                                              long long units, int bwd) {
  const int LC = bwd ? g.C : g.c, LW = bwd ? g.W : g.w, LH = bwd ? g.H : g.h;
  for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
    // u = ((n * LH + h) * LW + w) * (LC / V) + cu, decoded 32 bits at a time: pixels stay below 2^30
    const uint32_t upp = (uint32_t)(LC / V);
    const long long px = u / upp;
    const int cc = (int)(u - px * upp) * V;
    const uint32_t a = udiv((uint32_t)px, g.fw);
    const int wq = (int)((uint32_t)px - a * (uint32_t)LW);
    const uint32_t b = udiv(a, g.fh);
    const int h = (int)(a - b * (uint32_t)LH), n = (int)b;
    float f[V];
    if (!bwd) {
      ldx<V, 0>(src, ((((long long)(n + g.on) * g.H + h + g.oh) * g.W + wq + g.ow) * g.C) + cc + g.oc, f);
      stx<V, 0>(dst, u * V, f);
    } else {
      const int wn = n - g.on, wh = h - g.oh, ww = wq - g.ow, wc = cc - g.oc;
      const bool in = wn >= 0 && wn < g.n && wh >= 0 && wh < g.h && ww >= 0 && ww < g.w && wc >= 0 && wc < g.c;
#pragma unroll
      for (int k = 0; k < V; ++k) f[k] = 0.f;
      if (in) ldx<V, 0>(src, ((((long long)wn * g.h + wh) * g.w + ww) * g.c) + wc, f);
      stx<V, 0>(dst, u * V, f);
    }
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool al4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Sizes and the limits of the index arithmetic; false for a geometry the kernels do not take.
inline void set_cs(Geo& g, int tile);
inline bool geometry(long long N, long long P, long long Q, long long C, long long R, long long S, long long sh,
                     long long sw, long long ph, long long pw, Geo& g) {
  if (N < 1 || P < 1 || Q < 1 || C < 1 || R < 1 || S < 1 || R > WMAX || S > WMAX) return false;
  if (sh < 1 || sw < 1 || sh > SMAX || sw > SMAX || ph < 0 || pw < 0) return false;
  const long long lim = 1LL << 30;
  if (P >= lim || Q >= lim || ph >= (1 << 20) || pw >= (1 << 20) || C > (1 << 20) || N >= lim) return false;
  const long long H = (P - 1) * sh + R - 2 * ph, W = (Q - 1) * sw + S - 2 * pw;
  if (H < 1 || W < 1 || H >= lim || W >= lim) return false;
  if (N * H * W >= lim || N * P * Q >= lim) return false;
  g.N = (int)N; g.C = (int)C; g.P = (int)P; g.Q = (int)Q; g.H = (int)H; g.W = (int)W;
  g.R = (int)R; g.S = (int)S; g.sh = (int)sh; g.sw = (int)sw; g.ph = (int)ph; g.pw = (int)pw;
  set_cs(g, CT);
  g.fsh = make_fdiv((uint32_t)sh); g.fsw = make_fdiv((uint32_t)sw);
  g.tps = 1; g.LG = 1; g.ci0 = g.cj0 = 0;
  return true;
}

inline void set_cs(Geo& g, int tile) {
  g.cs = g.C < tile ? g.C : tile;
  g.fcs = make_fdiv((uint32_t)g.cs);
}

inline void finish_tiles(Geo& g, int cells_h, int cells_w) {
  g.tiles_h = cdiv(cells_h, g.TH);
  g.tiles_w = cdiv(cells_w, g.TW);
  g.ntiles = g.N * g.tiles_h * g.tiles_w;  // < 2^30: at most one per pixel
  g.fpw = make_fdiv((uint32_t)g.PW); g.ftw = make_fdiv((uint32_t)g.TW);
  g.ftiles_h = make_fdiv((uint32_t)g.tiles_h); g.ftiles_w = make_fdiv((uint32_t)g.tiles_w);
}

// Forward: cells ci0.. of the output, tiles of about 16 x 32 output pixels that shrink until the weights,
// the bias and the fp32 patch fit LDS_MAX (1 x 1 always does: TR TS <= R S).  Returns the LDS bytes.
inline int plan_fwd(Geo& g) {
  g.TR = cdiv(g.R, g.sh); g.TS = cdiv(g.S, g.sw);
  g.ci0 = g.ph / g.sh; g.cj0 = g.pw / g.sw;
  const int cells_h = (g.H - 1 + g.ph) / g.sh - g.ci0 + 1, cells_w = (g.W - 1 + g.pw) / g.sw - g.cj0 + 1;
  if ((g.R * g.S + g.TR * g.TS) * g.cs * 4 + CT * 4 > LDS_MAX) set_cs(g, CT / 2);  // 16 x 16 at strides 1
  int TH = 16 / g.sh, TW = 32 / g.sw;
  if (TH < 1) TH = 1;
  if (TW < 1) TW = 1;
  if (TH > cells_h) TH = cells_h;
  if (TW > cells_w) TW = cells_w;
  auto bytes = [&]() { return (g.R * g.S + (TH + g.TR - 1) * (TW + g.TS - 1)) * g.cs * 4 + CT * 4; };
  while (bytes() > LDS_MAX && (TH > 1 || TW > 1)) {
    if (TH * g.sh >= TW * g.sw && TH > 1) --TH; else if (TW > 1) --TW; else --TH;
  }
  g.TH = TH; g.TW = TW; g.PH = TH + g.TR - 1; g.PW = TW + g.TS - 1;
  finish_tiles(g, cells_h, cells_w);
  return bytes();
}

// Gather kernels: tiles of cells (= pixels of x) of at most 8 x 16 whose dy patch, RE x SE deep per cell,
// fits `budget` bytes as bf16 (1 x 1 always does: 16 x 16 x 32 x 2 = 16 KB).
inline void plan_gather(Geo& g, int RE, int SE, int budget) {
  int TH = g.P < 8 ? g.P : 8, TW = g.Q < 16 ? g.Q : 16;
  auto bytes = [&]() { return ((TH - 1) * g.sh + RE) * ((TW - 1) * g.sw + SE) * g.cs * 2; };
  while (bytes() > budget && (TH > 1 || TW > 1)) {
    if (TH * g.sh >= TW * g.sw && TH > 1) --TH; else if (TW > 1) --TW; else --TH;
  }
  g.TH = TH; g.TW = TW; g.TR = RE; g.TS = SE;
  g.PH = (TH - 1) * g.sh + RE; g.PW = (TW - 1) * g.sw + SE;
  finish_tiles(g, g.P, g.Q);
}

inline int plan_dgrad(Geo& g) {  // returns the LDS bytes
  const int wbytes = g.R * g.S * g.cs * 4;
  plan_gather(g, g.R, g.S, LDS_MAX - wbytes < GATHER_PATCH ? LDS_MAX - wbytes : GATHER_PATCH);
  int LG = 1;
  while (LG < g.R) LG <<= 1;
  g.LG = LG;  // <= 16
  return wbytes + g.PH * g.PW * g.cs * 2;
}

inline int wgrad_lds(const Geo& g) { return 256 * 4 + ((g.TH * g.TW * g.cs + 7) & ~7) * 2 + g.PH * g.PW * g.cs * 2; }

// slabs of the weight gradient: contiguous runs of g.tps tiles
inline int plan_wgrad(Geo& g) {
  plan_gather(g, g.R > g.sh ? g.R : g.sh, g.S > g.sw ? g.S : g.sw, GATHER_PATCH);
  int want = 1024 / cdiv(g.C, g.cs);
  if (want < 1) want = 1;
  if (want > g.ntiles) want = g.ntiles;
  g.tps = cdiv(g.ntiles, want);
  return cdiv(g.ntiles, g.tps);
}

inline dim3 grid_of(const Geo& g, int cap) {
  const int gx = cdiv(g.C, g.cs);
  int gy = cap / gx;
  if (gy < 1) gy = 1;
  if (gy > g.ntiles) gy = g.ntiles;
  return dim3((unsigned)gx, (unsigned)gy);
}

}  // namespace

extern "C" {

// Floats the weight-gradient workspace needs; 0 for a geometry the kernels do not take.
long long sn_conv_updw_part_floats(long long N, long long P, long long Q, long long C, long long R, long long S,
                                   long long sh, long long sw, long long ph, long long pw) {
  Geo g;
  if (!geometry(N, P, Q, C, R, S, sh, sw, ph, pw, g)) return 0;
  return (long long)plan_wgrad(g) * (R * S + 1) * C;
}

// y[N][H][W][C] = bias + the depthwise transposed convolution of x[N][P][Q][C] with w[C][R][S]; bias
// (fp32) may be null.
int sn_conv_updw_fwd(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, long long N, long long P,
                     long long Q, long long C, long long R, long long S, long long sh, long long sw, long long ph,
                     long long pw, hipStream_t st) {
  Geo g;
  if (!geometry(N, P, Q, C, R, S, sh, sw, ph, pw, g)) return 3;
  if (!x || !w || !y || !al4(y)) return 2;
  const int lds = plan_fwd(g);
  if (lds > LDS_MAX) return 3;
  const dim3 grid = grid_of(g, 2048);
  if (C % 8 == 0 && al16(x) && al16(y))
    hipLaunchKernelGGL((conv_updw_fwd_k<true>), grid, dim3(256), lds, st, x, w, bias, y, g);
  else
    hipLaunchKernelGGL((conv_updw_fwd_k<false>), grid, dim3(256), lds, st, x, w, bias, y, g);
  return SN_CHECK_LAUNCH();
}

// dx[N][P][Q][C] from dy[N][H][W][C].
int sn_conv_updw_dgrad(const bf16_t* dy, const bf16_t* w, bf16_t* dx, long long N, long long P, long long Q,
                       long long C, long long R, long long S, long long sh, long long sw, long long ph, long long pw,
                       hipStream_t st) {
  Geo g;
  if (!geometry(N, P, Q, C, R, S, sh, sw, ph, pw, g)) return 3;
  if (!dy || !w || !dx) return 2;
  const int lds = plan_dgrad(g);
  if (lds > LDS_MAX) return 3;
  const dim3 grid = grid_of(g, 2048);
  if (C % 8 == 0 && al16(dy))
    hipLaunchKernelGGL((conv_updw_dgrad_k<true>), grid, dim3(256), lds, st, dy, w, dx, g);
  else
    hipLaunchKernelGGL((conv_updw_dgrad_k<false>), grid, dim3(256), lds, st, dy, w, dx, g);
  return SN_CHECK_LAUNCH();
}

// dw[C][R][S] and db[C] (fp32) from dy[N][H][W][C] and x[N][P][Q][C].  dw_flag / db_flag: 0 skip, 1 store,
// 2 accumulate.  part: workspace of part_floats >= sn_conv_updw_part_floats(...) floats.
int sn_conv_updw_wgrad(const bf16_t* dy, const bf16_t* x, float* part, long long part_floats, float* dw,
                       long long dw_flag, float* db, long long db_flag, long long N, long long P, long long Q,
                       long long C, long long R, long long S, long long sh, long long sw, long long ph, long long pw,
                       hipStream_t st) {
  Geo g;
  if (!geometry(N, P, Q, C, R, S, sh, sw, ph, pw, g)) return 3;
  if (!dy || !x || !part) return 2;
  if ((dw_flag != GRAD_SKIP && !dw) || (db_flag != GRAD_SKIP && !db)) return 2;
  const int slabs = plan_wgrad(g), NQ = (int)(R * S) + 1;
  if ((long long)slabs * NQ * C > part_floats) return 3;
  const int lds = wgrad_lds(g);
  if (lds > LDS_MAX) return 3;
  const dim3 grid((unsigned)cdiv(g.C, g.cs), (unsigned)slabs);
  const bool vec = C % 8 == 0 && al16(dy) && al16(x);
  const int na = cdiv((NQ - 1) * g.cs, 256);  // <= 32
#define SN_UPDW_WGRAD(NA) \
  do { \
    if (vec) hipLaunchKernelGGL((conv_updw_wgrad_k<true, NA>), grid, dim3(256), lds, st, dy, x, part, g); \
    else hipLaunchKernelGGL((conv_updw_wgrad_k<false, NA>), grid, dim3(256), lds, st, dy, x, part, g); \
  } while (0)
  if (na <= 2) SN_UPDW_WGRAD(2);
  else if (na <= 8) SN_UPDW_WGRAD(8);
  else SN_UPDW_WGRAD(32);
#undef SN_UPDW_WGRAD
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(conv_updw_wgrad_finalize_k, dim3((unsigned)(((long long)NQ * C + FO - 1) / FO)), dim3(FO * FL), 0, st,
                     part, slabs, (int)C, NQ, dw, (int)dw_flag, db, (int)db_flag);
  return SN_CHECK_LAUNCH();
}

// Crop between big[N][H][W][C] and its window win[n][h][w][c] at (on, oh, ow, oc).  bwd == 0: win = the
// window of big.  bwd != 0: big = win inside the window, zero elsewhere.
int sn_crop(const bf16_t* src, bf16_t* dst, long long N, long long H, long long W, long long C, long long n,
            long long h, long long w, long long c, long long on, long long oh, long long ow, long long oc,
            long long bwd, hipStream_t st) {
  if (N < 1 || H < 1 || W < 1 || C < 1 || n < 1 || h < 1 || w < 1 || c < 1 || on < 0 || oh < 0 || ow < 0 || oc < 0)
    return 3;
  if (on + n > N || oh + h > H || ow + w > W || oc + c > C) return 3;
  const long long lim = 1LL << 30;
  if (N * H * W >= lim || C > (1 << 20) || !src || !dst) return 3;
  CropGeo g;
  g.H = (int)H; g.W = (int)W; g.C = (int)C; g.n = (int)n; g.h = (int)h; g.w = (int)w; g.c = (int)c;
  g.on = (int)on; g.oh = (int)oh; g.ow = (int)ow; g.oc = (int)oc;
  g.fw = make_fdiv((uint32_t)(bwd ? W : w));
  g.fh = make_fdiv((uint32_t)(bwd ? H : h));
  const bool vec = C % 8 == 0 && c % 8 == 0 && oc % 8 == 0 && al16(src) && al16(dst);
  const long long elems = bwd ? N * H * W * C : n * h * w * c;
  const long long units = vec ? elems / 8 : elems;
  const int blocks = sn_blocks(units, 256, sn_cu_count() * 16);
  if (vec) hipLaunchKernelGGL((crop_k<8>), dim3(blocks), dim3(256), 0, st, src, dst, g, units, (int)bwd);
  else hipLaunchKernelGGL((crop_k<1>), dim3(blocks), dim3(256), 0, st, src, dst, g, units, (int)bwd);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
