// 32-wide grouped 3x3 convolution (gfx950): Cg == Kg == 32 channels per group, NHWC bf16 (the last
// stage of ResNeXt-50 / -101 32x4d and 64x4d).
//
// csrc/kernels/conv_grouped.hip packs 16 / Cg narrow groups into a block-diagonal 16 x 16 bundle.
// At Cg = 32 that trick has nothing left to pack: one tap of one group is a dense 32 x 32 matrix,
// exactly the K = 32 of v_mfma_f32_16x16x32_bf16, so these kernels are dense per group and no MFMA
// multiplies a structural zero.  An Inf or NaN stays inside the 32 outputs of its group.
//
// Work split.  A wave owns one group for its whole life, a block of four waves owns four
// consecutive groups = 128 channels and walks 8 x 8 pixel tiles of the tensor it writes.  Per tile
// the block stages the source pixels every tap of the tile reads, 128 channels each and zero
// outside the image, in LDS with whole-line 16-byte loads.  A staged pixel is padded from 256 to
// 272 bytes: 17 bank quads, so the 16 pixels of one operand read start on 16 different quads.
//
//   forward   The wave keeps its group's nine 32 x 32 tap matrices as MFMA row operands: 9 taps x
//             2 tiles of 16 output channels = 18 fragments, 72 VGPRs, loaded once with 16-byte
//             loads from the weights in place [K][3][3][32].  The activation operand of a tap is
//             one 16-byte LDS read per lane (pixel l & 15, channels 8 (l >> 4) .. + 7) and feeds
//             both output tiles.  Row 4 q + i of output tile t is channel 8 q + 4 t + i, so a lane
//             ends with 8 consecutive channels of one pixel: fp32 bias, ReLU, one 16-byte store.
//   dgrad     the same kernel in gather form over dy, by output phase.  Write h + ph = sh i + a:
//             (i, j) is a cell, (a, b) its phase, and only taps r = a + sh t reach phase a, reading
//             dy row i - t.  The tiles walk 8 x 8 cells; per phase the kernel issues MFMAs for the
//             taps of that parity only (9 tap products per cell at any stride, where zeroing the
//             inexact quotients of all nine taps per pixel costs sh sw times that), and stores the
//             phase's pixel of every cell.  Cells whose dy rows lie outside dy read staged zeros and
//             store zeros through the same code; strides (2, 1) and (1, 2) decompose one axis.
//             With a 3x3 window and strides <= 2 every phase has a tap.  The weight operand has the
//             roles swapped (rows = input channel, k = output channel); in memory the input channel
//             is the contiguous one, so each tap's 32 x 32 block goes through LDS once per wave and
//             is read back transposed (ds_read_b64_tr_b16).  Nothing is flipped.  dx = 0 where
//             gate <= 0, 16-byte gate loads and stores.
//   wgrad     the reduction runs over pixels.  The block stages the dy tile next to the x patch; a
//             wave reads both operands of its group transposed from the staged pixels (pixels
//             along k) and keeps the group's 9 x 32 x 32 fp32 result in 36 accumulator fragments
//             (144 registers per lane; the compiler places what it wants in AGPRs).  A block sums a
//             slab of consecutive tiles in tile order and writes a partial; a finalize launch sums
//             the slabs in slab order and stores or accumulates onto dw [K][3][3][32] fp32.  No
//             float atomics: bitwise reproducible.  The bias gradient stays on the column sum.
//
// Departures from the plan this file was written to: the block is persistent only in the sense of
// conv_grouped.hip (an even share of the tiles per block, capped at about 4096 blocks in all), and
// the only tile shape built is 8 x 8 (77 % full on a 7 x 7 image; row-major pixel runs and two
// images per tile were not built, see docs/PERF_NOTES.md).  Stride-2 forward and weight-gradient
// patches are 17 x 17 pixels = 77 KB (94 KB with the dy tile): above the default 64 KB of dynamic
// LDS, so the launchers raise the limit once per device.
//
// Geometry: strides 1 or 2 per axis, any pad, no dilation, C % 32 == 0, every tensor dense and
// 16-byte aligned.  Pixel counts stay below 2^30 (checked), element offsets are 64-bit.
#include "common.h"

namespace {

constexpr int BW = 4;          // groups (waves) of a block
constexpr int GC = 32;         // channels of a group
constexpr int TR = 8, TC = 8;  // pixels (cells) of a tile: four MFMA tiles of 16, two reduction steps of 32
constexpr int PIXB = 272;      // LDS bytes of a staged pixel: 128 channels and 16 bytes of padding
constexpr int WROW = 80;       // LDS bytes of a staged weight row: 32 channels and 16 bytes of padding
constexpr int NT = 64 * BW;
// weight-gradient blocks aimed at: one per CU measured best at both stage-5 shapes of the sweep over
// 16 .. 512 in docs/PERF_NOTES.md; sn_conv_wgroup_tune changes it
constexpr int DEFAULT_WG_BLOCKS = 256;
int g_wg_blocks = DEFAULT_WG_BLOCKS;

struct Geo {
  int N, H, W, C, P, Q, sh, sw, ph, pw;
};

struct Axis {
  int n, tiles, ext;     // walked positions (output pixels, or cells of the data gradient), tiles, staged extent
  int first;             // first walked position
  int src_n, dst_n;      // extent of the source tensor and of the tensor written
  int mul, add;          // source origin of the tile at walked position t0: t0 * mul + add
  int stride, pad;
};

struct Tiling {
  Axis r, c;
  int C;
  uint32_t ntiles;
  FDiv fimg, ftc, fext;  // tiles per image, tiles per tile row, source columns of a staged patch
};

SN_DEV uint4 ld8(const bf16_t* __restrict__ p, long long e, bool ok) {
  return ok ? *reinterpret_cast<const uint4*>(p + e) : make_uint4(0u, 0u, 0u, 0u);
}

// tile t -> image, first walked row and column, origin of its source patch
SN_DEV void tile_of(const Tiling& g, uint32_t t, int& n, int& r0, int& c0, int& sr0, int& sc0) {
  const uint32_t img = udiv(t, g.fimg), ti = t - img * g.fimg.d, tr = udiv(ti, g.ftc);
  n = (int)img;
  r0 = g.r.first + (int)tr * TR;
  c0 = g.c.first + (int)(ti - tr * g.ftc.d) * TC;
  sr0 = r0 * g.r.mul + g.r.add;
  sc0 = c0 * g.c.mul + g.c.add;
}

// Stage rows x cols pixels from (r0, c0) of image n of src [.][src_r][src_c][C], channels
// cb0 .. cb0 + 127, at sm; zero outside the image and past C.  16 lanes load the 256 bytes of a pixel.
SN_DEV void stage(const bf16_t* __restrict__ src, int n, int r0, int c0, int rows, int cols, const FDiv& fcols,
                  int src_r, int src_c, int C, int cb0, unsigned char* sm) {
  const int chunk = threadIdx.x & 15;
  const bool cok = cb0 + chunk * 8 < C;
  for (int i = threadIdx.x >> 4; i < rows * cols; i += NT / 16) {
    const int pr = (int)udiv((uint32_t)i, fcols), pc = i - pr * cols;
    const int r = r0 + pr, c = c0 + pc;
    const bool ok = cok && r >= 0 && r < src_r && c >= 0 && c < src_c;
    *reinterpret_cast<uint4*>(sm + i * PIXB + chunk * 16) =
        ld8(src, (((long long)n * src_r + r) * src_c + c) * C + cb0 + chunk * 8, ok);
  }
}

// 8 rows of LDS as an MFMA operand with the rows along k: a0 addresses 4 columns of row q of the
// lane's 8, a0 + second the same of row q + 4.  ds_read_b64_tr_b16: lane 4q + p of a 16-lane group
// addresses row q, its own 4 columns, and receives column (lane & 15) of the 4 x 16 block the 16
// lanes name, from each of its 4 rows.
SN_DEV bf16x8_t tr_frag(const unsigned char* a0, int second) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + second));
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, r);
}

// ---------------------------------------------------------------------------------------
// Forward (src = x, dst = y: the tiles walk y) and data gradient (src = dy, dst = dx: the tiles
// walk cells).  SH, SW: the strides of the data gradient (the forward reads them from g).
// ---------------------------------------------------------------------------------------
template <bool DGRAD, int SH, int SW>
__global__ void __launch_bounds__(NT) conv_wgroup_io_k(const bf16_t* __restrict__ src, const bf16_t* __restrict__ w,
                                                       const float* __restrict__ bias,
                                                       const bf16_t* __restrict__ gate, bf16_t* __restrict__ dst,
                                                       const Tiling g, int relu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  constexpr int TMR = DGRAD ? (SH == 1 ? 3 : 2) : 1, TMC = DGRAD ? (SW == 1 ? 3 : 2) : 1;  // tap offsets per axis
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane >> 4, ln = lane & 15;
  const int cb0 = blockIdx.y * (GC * BW), ch0 = cb0 + wave * GC;
  const bool live = ch0 < g.C;  // C % 32 == 0: a live wave's group is all inside

  // wf[tap][t]: rows are the channels the wave writes, row 4 q + i of tile t = channel 8 q + 4 t + i
  bf16x8_t wf[9][2];
  if (!DGRAD) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int co = ch0 + 8 * (ln >> 2) + 4 * t + (ln & 3);
        wf[tap][t] = __builtin_bit_cast(bf16x8_t, ld8(w, ((long long)co * 9 + tap) * GC + 8 * lg, live));
      }
  } else {
    // per tap: the wave's 32 (output channel) x 32 (input channel) block through its own LDS rows,
    // read back with the output channels along k
    unsigned char* const smw = sm + wave * (GC * WROW);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      __syncthreads();  // the previous tap's reads are done
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        const int u = lane + 64 * x, ko = u >> 2, part = u & 3;
        *reinterpret_cast<uint4*>(smw + ko * WROW + part * 16) =
            ld8(w, ((long long)(ch0 + ko) * 9 + tap) * GC + part * 8, live);
      }
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 2; ++t)
        wf[tap][t] = tr_frag(smw + (8 * lg + (ln >> 2)) * WROW + (ln & 3) * 16 + t * 8, 4 * WROW);
    }
  }

  const int co = ch0 + 8 * lg;                 // the lane's 8 output channels
  const int lane_off = wave * (2 * GC) + 16 * lg;  // its 8 operand channels in a staged pixel
  float bv[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) bv[i] = (live && bias) ? bias[co + i] : 0.f;

  for (uint32_t t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    int n, r0, c0, sr0, sc0;
    tile_of(g, t, n, r0, c0, sr0, sc0);
    __syncthreads();  // the previous tile's (or the weights') reads are done
    stage(src, n, sr0, sc0, g.r.ext, g.c.ext, g.fext, g.r.src_n, g.c.src_n, g.C, cb0, sm);
    __syncthreads();
    if (!live) continue;
#pragma unroll
    for (int a = 0; a < (DGRAD ? SH : 1); ++a)
#pragma unroll
      for (int b = 0; b < (DGRAD ? SW : 1); ++b)
#pragma unroll
        for (int mt = 0; mt < TR * TC / 16; ++mt) {
          const int idx = mt * 16 + ln, lr = idx / TC, lc = idx % TC;
          // the lane's pixel in the patch at tap offset 0, and the pixel it writes
          const unsigned char* base;
          int r, c;
          if (DGRAD) {
            base = sm + ((lr + TMR - 1) * g.c.ext + lc + TMC - 1) * PIXB + lane_off;
            r = SH * (r0 + lr) + a - g.r.pad;
            c = SW * (c0 + lc) + b - g.c.pad;
          } else {
            base = sm + (lr * g.r.stride * g.c.ext + lc * g.c.stride) * PIXB + lane_off;
            r = r0 + lr;
            c = c0 + lc;
          }
          f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
          for (int kr = 0; kr < 3; ++kr)
#pragma unroll
            for (int kc = 0; kc < 3; ++kc) {
              int off;
              if (DGRAD) {  // tap (a + SH t, b + SW u) reads dy at (i - t, j - u)
                if (kr % SH != a % SH || kc % SW != b % SW) continue;
                off = -((kr / SH) * g.c.ext + kc / SW) * PIXB;
              } else {
                off = (kr * g.c.ext + kc) * PIXB;
              }
              const bf16x8_t v = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const uint4*>(base + off));
#pragma unroll
              for (int u = 0; u < 2; ++u)
                acc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[kr * 3 + kc][u], v, acc[u], 0, 0, 0);
            }
          if (r >= 0 && r < g.r.dst_n && c >= 0 && c < g.c.dst_n) {
            const long long e = (((long long)n * g.r.dst_n + r) * g.c.dst_n + c) * g.C + co;
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
              v[i] = acc[i >> 2][i & 3] + bv[i];
              if (relu) v[i] = fmaxf(v[i], 0.f);
            }
            if (gate) {
              float gf[8];
              unpack8(*reinterpret_cast<const uint4*>(gate + e), gf);
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] = gf[i] > 0.f ? v[i] : 0.f;
            }
            *reinterpret_cast<uint4*>(dst + e) = pack8(v);
          }
        }
  }
}

// ---------------------------------------------------------------------------------------
// Weight gradient pass 1: part[slab][K][3][3][32], the sum over the slab's tiles of output pixels.
// g: the forward tiling (the tiles walk the output pixels, the patch is x's)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(NT) conv_wgroup_wgrad_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                          float* __restrict__ part, const Tiling g, int per) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];  // the x patch, then the dy tile
  unsigned char* smd = sm + g.r.ext * g.c.ext * PIXB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cb0 = blockIdx.y * (GC * BW), ch0 = cb0 + wave * GC;
  const bool live = ch0 < g.C;
  f32x4 acc[9][2][2];  // [tap][tile of output channels][tile of input channels]
#pragma unroll
  for (int k = 0; k < 9; ++k)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[k][i >> 1][i & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
  const FDiv ftile = {TC, 0u, 3};  // udiv by TC = 8: a shift
  // the lane's address in a transposed read: pixel q (then q + 4) of the 8 of its 16-lane group,
  // channels 4p .. 4p + 3 of a 16-channel tile of the wave's group
  const int q = (lane & 15) >> 2, lane_off = wave * (2 * GC) + 8 * (lane & 3);
  const uint32_t t0 = blockIdx.x * (uint32_t)per, t1 = min(g.ntiles, t0 + (uint32_t)per);
  for (uint32_t t = t0; t < t1; ++t) {
    int n, r0, c0, sr0, sc0;
    tile_of(g, t, n, r0, c0, sr0, sc0);
    __syncthreads();  // the previous tile's reads are done
    stage(x, n, sr0, sc0, g.r.ext, g.c.ext, g.fext, g.r.src_n, g.c.src_n, g.C, cb0, sm);
    stage(dy, n, r0, c0, TR, TC, ftile, g.r.n, g.c.n, g.C, cb0, smd);  // zero past the edge: no contribution
    __syncthreads();
    if (!live) continue;
#pragma unroll
    for (int ck = 0; ck < TR * TC / 32; ++ck) {
      const int lr = ck * 4 + (lane >> 4);  // the 16-lane group's 8 pixels are row lr of the tile
      bf16x8_t a[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) a[kt] = tr_frag(smd + (lr * TC + q) * PIXB + lane_off + kt * 32, 4 * PIXB);
      const unsigned char* b0 = sm + ((lr * g.r.stride) * g.c.ext + q * g.c.stride) * PIXB + lane_off;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const bf16x8_t b = tr_frag(b0 + ((tap / 3) * g.c.ext + tap % 3) * PIXB + ct * 32, 4 * g.c.stride * PIXB);
#pragma unroll
          for (int kt = 0; kt < 2; ++kt)
            acc[tap][kt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kt], b, acc[tap][kt][ct], 0, 0, 0);
        }
    }
  }
  if (!live) return;
  // acc[tap][kt][ct][i]: output channel 16 kt + 4 (lane >> 4) + i (the row), input channel 16 ct + (lane & 15)
  const long long total = (long long)g.C * 9 * GC;
  float* const p0 = part + blockIdx.x * total + (long long)ch0 * 9 * GC + (lane & 15);
#pragma unroll
  for (int kt = 0; kt < 2; ++kt)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float* dst = p0 + (16 * kt + 4 * (lane >> 4) + i) * (9 * GC);
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) dst[tap * GC + 16 * ct] = acc[tap][kt][ct][i];
    }
}

// The slabs in slab order, stored or accumulated onto dw.
__global__ void __launch_bounds__(256) conv_wgroup_wgrad_finalize_k(const float* __restrict__ part, int slabs,
                                                                    long long total, float* __restrict__ dw, int acc) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  float a = 0.f;
#pragma unroll 4
  for (int s = 0; s < slabs; ++s) a += part[(long long)s * total + o];
  dw[o] = acc ? dw[o] + a : a;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Output size and the limits of the index arithmetic; false for a geometry the kernels do not take.
inline bool geometry(long long N, long long H, long long W, long long C, long long sh, long long sw, long long ph,
                     long long pw, Geo& g) {
  if (N < 1 || H < 1 || W < 1 || C < GC || C % GC != 0 || C > (1 << 20)) return false;
  if (sh < 1 || sh > 2 || sw < 1 || sw > 2 || ph < 0 || ph > (1 << 20) || pw < 0 || pw > (1 << 20)) return false;
  if (H + 2 * ph < 3 || W + 2 * pw < 3) return false;
  const long long P = (H + 2 * ph - 3) / sh + 1, Q = (W + 2 * pw - 3) / sw + 1;
  const long long lim = 1LL << 30;
  if (N * H * W >= lim || N * P * Q >= lim) return false;
  g.N = (int)N; g.H = (int)H; g.W = (int)W; g.C = (int)C; g.P = (int)P; g.Q = (int)Q;
  g.sh = (int)sh; g.sw = (int)sw; g.ph = (int)ph; g.pw = (int)pw;
  return true;
}

// one axis of the tiling.  Forward: n output pixels, source pixel t * stride - pad + k.  Data
// gradient: the cells i = (h + pad) / stride of the n_in pixels h, source pixel i - t for the
// ceil(3 / stride) tap offsets t.
inline Axis axis(int n_in, int n_out, int stride, int pad, bool dgrad) {
  Axis a;
  a.stride = stride; a.pad = pad;
  if (dgrad) {
    const int tm = stride == 1 ? 3 : 2;
    a.first = pad / stride;
    a.n = (n_in - 1 + pad) / stride - a.first + 1;
    a.src_n = n_out; a.dst_n = n_in;
    a.mul = 1; a.add = -(tm - 1);
    a.ext = TR + tm - 1;
  } else {
    a.first = 0;
    a.n = n_out;
    a.src_n = n_in; a.dst_n = n_out;
    a.mul = stride; a.add = -pad;
    a.ext = (TR - 1) * stride + 3;
  }
  a.tiles = (a.n + TR - 1) / TR;
  return a;
}

inline Tiling tiling(const Geo& g, bool dgrad) {
  Tiling t;
  t.r = axis(g.H, g.P, g.sh, g.ph, dgrad);
  t.c = axis(g.W, g.Q, g.sw, g.pw, dgrad);
  t.C = g.C;
  t.ntiles = (uint32_t)((long long)g.N * t.r.tiles * t.c.tiles);
  t.fimg = make_fdiv((uint32_t)(t.r.tiles * t.c.tiles));
  t.ftc = make_fdiv((uint32_t)t.c.tiles);
  t.fext = make_fdiv((uint32_t)t.c.ext);
  return t;
}

inline unsigned channel_blocks(long long C) { return (unsigned)((C / GC + BW - 1) / BW); }

// blocks of BW groups on y; on x the tiles, evenly over at most about 4096 blocks in all
inline dim3 io_grid(const Tiling& t) {
  const unsigned gy = channel_blocks(t.C);
  unsigned cap = 4096 / gy;
  if (cap < 1) cap = 1;
  const unsigned per = (t.ntiles + cap - 1) / cap;
  return dim3((t.ntiles + per - 1) / per, gy);
}

inline size_t patch_lds(const Tiling& t) { return (size_t)t.r.ext * t.c.ext * PIXB; }

// Weight-gradient slabs of `per` consecutive tiles: about g_wg_blocks blocks in all.  A slab's
// partial is C x 9 x 32 floats, as many bytes as 2.25 tiles of x at stride 1, so the rule aims
// lower than conv_grouped.hip's 512.
inline int wgrad_slabs(long long ntiles, long long C, int& per) {
  long long want = g_wg_blocks / channel_blocks(C);
  if (want < 1) want = 1;
  const long long p = (ntiles + want - 1) / want;
  per = (int)p;
  return (int)((ntiles + p - 1) / p);
}

inline long long out_tiles(long long N, long long P, long long Q) {
  return N * ((P + TR - 1) / TR) * ((Q + TC - 1) / TC);
}

// Dynamic LDS above the default 64 KB needs the limit raised: once per device, a failure is not kept.
template <typename K>
inline bool lds_ok(K kernel, size_t lds, bool* raised) {
  if (lds <= 64 * 1024) return true;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (dev >= 0 && dev < 64 && raised[dev]) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          160 * 1024) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (dev >= 0 && dev < 64) raised[dev] = true;
  return true;
}

template <int SH, int SW>
int launch_dgrad(const bf16_t* dy, const bf16_t* w, const bf16_t* gate, bf16_t* dx, const Tiling& t, hipStream_t st) {
  hipLaunchKernelGGL((conv_wgroup_io_k<true, SH, SW>), io_grid(t), dim3(NT), patch_lds(t), st, dy, w,
                     (const float*)nullptr, gate, dx, t, 0);
  return SN_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

// Weight-gradient blocks aimed at (scripts/wgroup_probe.py sweeps it); blocks < 1 restores the default.
void sn_conv_wgroup_tune(long long blocks) { g_wg_blocks = blocks < 1 ? DEFAULT_WG_BLOCKS : (int)blocks; }

// Floats the weight-gradient workspace needs for N x P x Q outputs of C channels in groups of 32.
long long sn_conv_wgroup_part_floats(long long N, long long P, long long Q, long long C) {
  if (N < 1 || P < 1 || Q < 1 || C < GC || C % GC != 0 || C > (1 << 20) || N * P * Q >= (1LL << 30)) return 0;
  int per;
  return (long long)wgrad_slabs(out_tiles(N, P, Q), C, per) * C * 9 * GC;
}

// y[N][P][Q][C] = relu?(3x3 conv of x[N][H][W][C] in groups of 32 with w[C][3][3][32] + bias); bias may be null.
int sn_conv_wgroup_fwd(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, long long N, long long H,
                       long long W, long long C, long long sh, long long sw, long long ph, long long pw,
                       long long relu, hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, sh, sw, ph, pw, g)) return 3;
  if (!al16(x) || !al16(w) || !al16(y)) return 2;
  const Tiling t = tiling(g, false);
  static bool raised[64] = {};
  if (!lds_ok(conv_wgroup_io_k<false, 1, 1>, patch_lds(t), raised)) return 1;
  hipLaunchKernelGGL((conv_wgroup_io_k<false, 1, 1>), io_grid(t), dim3(NT), patch_lds(t), st, x, w, bias,
                     (const bf16_t*)nullptr, y, t, (int)relu);
  return SN_CHECK_LAUNCH();
}

// dx[N][H][W][C] = the data gradient of dy[N][P][Q][C], zeroed where gate <= 0 (gate shaped like
// dx; may be null).
int sn_conv_wgroup_dgrad(const bf16_t* dy, const bf16_t* w, const bf16_t* gate, bf16_t* dx, long long N, long long H,
                         long long W, long long C, long long sh, long long sw, long long ph, long long pw,
                         hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, sh, sw, ph, pw, g)) return 3;
  if (!al16(dy) || !al16(w) || !al16(gate) || !al16(dx)) return 2;
  const Tiling t = tiling(g, true);  // patches of at most 10 x 10 pixels: 27 KB
  if (sh == 1) return sw == 1 ? launch_dgrad<1, 1>(dy, w, gate, dx, t, st) : launch_dgrad<1, 2>(dy, w, gate, dx, t, st);
  return sw == 1 ? launch_dgrad<2, 1>(dy, w, gate, dx, t, st) : launch_dgrad<2, 2>(dy, w, gate, dx, t, st);
}

// dw[C][3][3][32] (fp32) from dy and x, stored (acc == 0) or accumulated.  part: workspace of
// part_floats >= sn_conv_wgroup_part_floats(N, P, Q, C) floats.
int sn_conv_wgroup_wgrad(const bf16_t* dy, const bf16_t* x, float* part, long long part_floats, float* dw,
                         long long acc, long long N, long long H, long long W, long long C, long long sh,
                         long long sw, long long ph, long long pw, hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, sh, sw, ph, pw, g)) return 3;
  if (!al16(dy) || !al16(x) || !al16(part) || !dw) return 2;
  const Tiling t = tiling(g, false);
  int per;
  const int slabs = wgrad_slabs(t.ntiles, C, per);
  const long long total = C * 9 * GC;
  if (slabs * total > part_floats) return 3;
  const size_t lds = patch_lds(t) + TR * TC * PIXB;
  static bool raised[64] = {};
  if (!lds_ok(conv_wgroup_wgrad_k, lds, raised)) return 1;
  hipLaunchKernelGGL(conv_wgroup_wgrad_k, dim3((unsigned)slabs, channel_blocks(C)), dim3(NT), lds, st, dy, x, part, t,
                     per);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(conv_wgroup_wgrad_finalize_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part,
                     slabs, total, dw, (int)acc);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
