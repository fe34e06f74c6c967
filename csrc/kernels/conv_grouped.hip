// Narrow-group 3x3 convolution (gfx950): Cg == Kg in {4, 8, 16} channels per group, NHWC bf16.
//
// Caffe runs a grouped layer as `group` independent im2col + GEMM products (base_conv_layer.cpp).
// With 4 to 16 channels per group each of those GEMMs is a sliver, and the layer as a whole is
// bandwidth-bound, so these kernels make one pass over the activations instead.  They work on
// "bundles" of 16 consecutive channels = 16 / Cg whole groups: with Cg == Kg a bundle's 16 outputs
// read exactly its 16 inputs, i.e. a bundle is a dense 16 -> 16 convolution whose weight operand
// is block-diagonal.  The zero blocks waste 16 / Cg of the MFMA work, which is accepted.
//
// A block of four waves owns 64 channels, a bundle per wave, and walks 8 x 8 pixel tiles of the
// tensor its product runs over.  Per tile it stages the source pixels every tap of the tile
// reads, 64 channels each and zero outside the image, in LDS with whole-line 16-byte loads: every
// source byte is fetched once per block instead of once per tap.  A staged pixel is padded to
// 144 bytes, so that the 16 pixels of one operand read fall on 16 different bank quads.
//
//   forward   v_mfma_f32_16x16x32_bf16, K = 32 = (2 taps) x (16 channels), five steps for the
//             nine taps (the second half of the fifth is zero).  The weight operand (rows = output
//             channel) is built once per wave from the weights in place [K][3][3][Cg], zero where
//             input and output channel lie in different groups: 20 VGPRs kept across the wave's
//             tiles.  The activation operand of a step is one 16-byte LDS read per lane: lane l
//             reads pixel l & 15, tap 2 step + (l >> 5), channels 8 ((l >> 4) & 1) .. + 7.  A lane
//             ends with 4 consecutive channels of one pixel: fp32 bias, ReLU, one 8-byte store.
//   dgrad     the same kernel in gather form over dy: input pixel (h, w) takes tap (r, s) from
//             dy[(h + ph - r) / sh][(w + pw - s) / sw] where both quotients are exact (an inexact
//             one is zeroed in the operand, one outside dy is a staged zero); the weight operand
//             has the roles of the channels swapped (rows = input channel).  Weights are read in
//             place, nothing is flipped.  dx = 0 where gate <= 0.
//   wgrad     the reduction runs over pixels: per bundle and tap a 16 x 16 fp32 accumulator
//             dy^T . x_shifted, of which the diagonal Cg x Cg blocks are kept.  The block stages
//             the dy tile (zero past the edge) next to the x patch; both operands have the pixels
//             along k and are read transposed straight from the staged pixels
//             (ds_read_b64_tr_b16), two steps of 32 pixels per tile.  A block sums a slab of
//             consecutive tiles in tile order and writes its partial; a finalize launch sums the
//             slabs in slab order and stores or accumulates onto dw [K][3][3][Cg] fp32.  No float
//             atomics; the result is bitwise reproducible.  The bias gradient stays on the
//             column-sum launch.
//
// The off-group entries of the weight operand are zeros that the MFMA multiplies: an Inf or NaN
// activation in one group therefore turns all 16 outputs of its bundle into NaN in forward and
// data gradient (0 x Inf), where the per-group paths confine it to the Cg outputs of its group.
// Finite inputs are not affected.
//
// Geometry: strides 1 or 2 per axis, any pad, no dilation, C % 16 == 0, every tensor dense and
// 16-byte aligned.  Pixel counts stay below 2^30 (checked), element offsets are 64-bit.
#include "common.h"

namespace {

constexpr int BW = 4;          // bundles (waves) of a block
constexpr int TR = 8, TC = 8;  // pixels of a tile: four MFMA tiles of 16, two reduction steps of 32
constexpr int PIXB = 144;      // LDS bytes of a staged pixel: 64 channels and 16 bytes of padding
constexpr int MAX_WG = 512;    // weight-gradient blocks aimed at: two per CU measured best (docs/PERF_NOTES.md)

struct Geo {
  int N, H, W, C, P, Q, sh, sw, ph, pw;
};

struct Axis {
  int n, tiles, ext;     // extent of the tensor the tiles walk, its tiles, extent of the staged source
  int src_n;             // extent of the source tensor
  int mul, shift, add;   // source origin of the tile at t0: ((t0 * mul) >> shift) + add
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

// tile t -> image, first row and column, origin of its source patch
SN_DEV void tile_of(const Tiling& g, uint32_t t, int& n, int& r0, int& c0, int& sr0, int& sc0) {
  const uint32_t img = udiv(t, g.fimg), ti = t - img * g.fimg.d, tr = udiv(ti, g.ftc);
  n = (int)img;
  r0 = (int)tr * TR;
  c0 = (int)(ti - tr * g.ftc.d) * TC;
  sr0 = ((r0 * g.r.mul) >> g.r.shift) + g.r.add;
  sc0 = ((c0 * g.c.mul) >> g.c.shift) + g.c.add;
}

// Stage rows x cols pixels from (r0, c0) of image n of src [.][src_r][src_c][C], channels
// cb0 .. cb0 + 63, at sm; zero outside the image and past C.  8 lanes load the 128 bytes of a pixel.
SN_DEV void stage(const bf16_t* __restrict__ src, int n, int r0, int c0, int rows, int cols, const FDiv& fcols,
                  int src_r, int src_c, int C, int cb0, unsigned char* sm) {
  const int chunk = threadIdx.x & 7;
  const bool cok = cb0 + chunk * 8 < C;
  for (int i = threadIdx.x >> 3; i < rows * cols; i += 8 * BW) {
    const int pr = (int)udiv((uint32_t)i, fcols), pc = i - pr * cols;
    const int r = r0 + pr, c = c0 + pc;
    const bool ok = cok && r >= 0 && r < src_r && c >= 0 && c < src_c;
    *reinterpret_cast<uint4*>(sm + i * PIXB + chunk * 16) =
        ld8(src, (((long long)n * src_r + r) * src_c + c) * C + cb0 + chunk * 8, ok);
  }
}

// The weight operand of the five steps for the bundle at channel ch0: lane l holds row l & 15,
// k = 8 (l >> 4) + j = tap 2 step + (l >> 5), channel 8 ((l >> 4) & 1) + j.  Forward: rows are
// output channels and k runs over input channels; DGRAD: the other way round.
template <int CG, bool DGRAD>
SN_DEV void load_wfrag(const bf16_t* __restrict__ w, int ch0, int lane, bf16x8_t* wf) {
  const int row = lane & 15, k0 = 8 * ((lane >> 4) & 1), th = lane >> 5;
#pragma unroll
  for (int step = 0; step < 5; ++step) {
    const int tap = 2 * step + th;
    s16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int kout = DGRAD ? k0 + j : row, cin = DGRAD ? row : k0 + j;
      const bool ok = tap < 9 && kout / CG == cin / CG;
      v[j] = ok ? (short)w[((ch0 + kout) * 9 + tap) * CG + cin % CG] : (short)0;
    }
    wf[step] = __builtin_bit_cast(bf16x8_t, v);
  }
}

// ---------------------------------------------------------------------------------------
// Forward (src = x, dst = y) and data gradient (src = dy, dst = dx): the tiles walk dst
// ---------------------------------------------------------------------------------------
template <int CG, bool DGRAD>
__global__ void __launch_bounds__(64 * BW) conv_grouped_io_k(const bf16_t* __restrict__ src,
                                                             const bf16_t* __restrict__ w,
                                                             const float* __restrict__ bias,
                                                             const bf16_t* __restrict__ gate,
                                                             bf16_t* __restrict__ dst, const Tiling g, int relu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cb0 = blockIdx.y * (16 * BW), ch0 = cb0 + wave * 16;
  const bool live = ch0 < g.C;  // C % 16 == 0: a live wave's 16 channels are all inside
  bf16x8_t wf[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) wf[i] = bf16x8_t{};
  if (live) load_wfrag<CG, DGRAD>(w, ch0, lane, wf);
  const int th = lane >> 5, co = ch0 + 4 * (lane >> 4);      // the lane's 4 output channels
  const int lane_off = wave * 32 + 16 * ((lane >> 4) & 1);  // its 8 operand channels in a staged pixel
  float bv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) bv[i] = (live && bias) ? bias[co + i] : 0.f;
  for (uint32_t t = blockIdx.x; t < g.ntiles; t += gridDim.x) {
    int n, r0, c0, sr0, sc0;
    tile_of(g, t, n, r0, c0, sr0, sc0);
    __syncthreads();  // the previous tile's reads are done
    stage(src, n, sr0, sc0, g.r.ext, g.c.ext, g.fext, g.r.src_n, g.c.src_n, g.C, cb0, sm);
    __syncthreads();
    if (!live) continue;
#pragma unroll
    for (int mt = 0; mt < TR * TC / 16; ++mt) {
      const int idx = mt * 16 + (lane & 15), lr = idx / TC, lc = idx % TC;
      const int r = r0 + lr, c = c0 + lc;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int step = 0; step < 5; ++step) {
        const int tap = 2 * step + th, kr = tap / 3, kc = tap - 3 * kr;
        int pr, pc;
        bool ok = tap < 9;
        if (DGRAD) {  // strides are 1 or 2; an exact quotient lies inside the patch
          const int ur = r + g.r.pad - kr, uc = c + g.c.pad - kc;
          ok = ok && (ur & (g.r.stride - 1)) == 0 && (uc & (g.c.stride - 1)) == 0;
          pr = (ur >> (g.r.stride - 1)) - sr0;
          pc = (uc >> (g.c.stride - 1)) - sc0;
        } else {
          pr = lr * g.r.stride + kr;
          pc = lc * g.c.stride + kc;
        }
        const uint4 a = ok ? *reinterpret_cast<const uint4*>(sm + (pr * g.c.ext + pc) * PIXB + lane_off)
                           : make_uint4(0u, 0u, 0u, 0u);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[step], __builtin_bit_cast(bf16x8_t, a), acc, 0, 0, 0);
      }
      if (r < g.r.n && c < g.c.n) {
        const long long e = (((long long)n * g.r.n + r) * g.c.n + c) * g.C + co;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = acc[i] + bv[i];
          if (relu) v[i] = fmaxf(v[i], 0.f);
        }
        if (gate) {
          const uint2 gv = *reinterpret_cast<const uint2*>(gate + e);
          const uint32_t gw[2] = {gv.x, gv.y};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float gf = __uint_as_float(i & 1 ? gw[i >> 1] & 0xffff0000u : gw[i >> 1] << 16);
            v[i] = gf > 0.f ? v[i] : 0.f;
          }
        }
        *reinterpret_cast<uint2*>(dst + e) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Weight gradient pass 1: part[slab][K][3][3][Cg], the sum over the slab's tiles of output pixels
// ---------------------------------------------------------------------------------------

// 8 staged pixels as an MFMA operand with the pixels along k: a0 addresses 4 channels of pixel
// q of the lane's 8, a0 + second the same of pixel q + 4.  ds_read_b64_tr_b16: lane 4q + p of a
// 16-lane group addresses row q, columns 4p .. 4p + 3 of a 4 x 16 block and receives column
// (lane & 15) of its 4 rows, so the lane ends with channel lane & 15 of the 8 pixels.
SN_DEV bf16x8_t tr_frag(const unsigned char* a0, int second) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + second));
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, r);
}

// g: the forward tiling (the tiles walk the output pixels, the patch is x's)
template <int CG>
__global__ void __launch_bounds__(64 * BW) conv_grouped_wgrad_k(const bf16_t* __restrict__ dy,
                                                                const bf16_t* __restrict__ x,
                                                                float* __restrict__ part, const Tiling g, int per) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];  // the x patch, then the dy tile
  unsigned char* smd = sm + g.r.ext * g.c.ext * PIXB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cb0 = blockIdx.y * (16 * BW), ch0 = cb0 + wave * 16;
  const bool live = ch0 < g.C;
  f32x4 acc[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const FDiv ftile = {TC, 0u, 3};  // udiv by TC = 8: a shift
  // the lane's address in a transposed read: pixel q (then q + 4) of the 8 of its 16-lane group,
  // channels 4p .. 4p + 3 of the wave's bundle
  const int q = (lane & 15) >> 2, lane_off = wave * 32 + 8 * (lane & 3);
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
      const int lr = ck * 4 + (lane >> 4);  // the group's 8 pixels are row lr of the tile
      const bf16x8_t a = tr_frag(smd + (lr * TC + q) * PIXB + lane_off, 4 * PIXB);
      const unsigned char* b0 = sm + ((lr * g.r.stride) * g.c.ext + q * g.c.stride) * PIXB + lane_off;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
        acc[tap] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a, tr_frag(b0 + ((tap / 3) * g.c.ext + tap % 3) * PIXB, 4 * g.c.stride * PIXB), acc[tap], 0, 0, 0);
    }
  }
  if (!live) return;
  // acc[tap][i]: output channel 4 (lane >> 4) + i (the row), input channel lane & 15 (the column)
  const int cin = lane & 15;
  const long long total = (long long)g.C * 9 * CG;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int kout = 4 * (lane >> 4) + i;
    if (kout / CG != cin / CG) continue;
    float* dst = part + blockIdx.x * total + ((long long)(ch0 + kout) * 9) * CG + cin % CG;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) dst[tap * CG] = acc[tap][i];
  }
}

// The slabs in slab order, stored or accumulated onto dw.
__global__ void __launch_bounds__(256) conv_grouped_wgrad_finalize_k(const float* __restrict__ part, int slabs,
                                                                     long long total, float* __restrict__ dw,
                                                                     int acc) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  float a = 0.f;
#pragma unroll 4
  for (int s = 0; s < slabs; ++s) a += part[(long long)s * total + o];
  dw[o] = acc ? dw[o] + a : a;
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Output size and the limits of the index arithmetic; false for a geometry the kernels do not take.
inline bool geometry(long long N, long long H, long long W, long long C, long long Cg, long long sh, long long sw,
                     long long ph, long long pw, Geo& g) {
  if (N < 1 || H < 1 || W < 1 || C < 16 || C % 16 != 0 || C > (1 << 20)) return false;
  if (Cg != 4 && Cg != 8 && Cg != 16) return false;
  if (sh < 1 || sh > 2 || sw < 1 || sw > 2 || ph < 0 || ph > (1 << 20) || pw < 0 || pw > (1 << 20)) return false;
  if (H + 2 * ph < 3 || W + 2 * pw < 3) return false;
  const long long P = (H + 2 * ph - 3) / sh + 1, Q = (W + 2 * pw - 3) / sw + 1;
  const long long lim = 1LL << 30;
  if (N * H * W >= lim || N * P * Q >= lim) return false;
  g.N = (int)N; g.H = (int)H; g.W = (int)W; g.C = (int)C; g.P = (int)P; g.Q = (int)Q;
  g.sh = (int)sh; g.sw = (int)sw; g.ph = (int)ph; g.pw = (int)pw;
  return true;
}

inline int ceil_div(int a, int b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

// one axis of the tiling: n walked pixels in tiles of `tile`, read from src_n source pixels
inline Axis axis(int n, int src_n, int tile, int stride, int pad, bool dgrad) {
  Axis a;
  a.n = n; a.src_n = src_n; a.stride = stride; a.pad = pad;
  a.tiles = (n + tile - 1) / tile;
  if (dgrad) {  // source pixel (t + pad - k) / stride for k = 0..2; t0 is a multiple of the stride
    a.mul = 1; a.shift = stride - 1; a.add = ceil_div(pad - 2, stride);
    a.ext = (tile - 1 + pad) / stride - a.add + 1;
  } else {      // source pixel t * stride - pad + k
    a.mul = stride; a.shift = 0; a.add = -pad;
    a.ext = (tile - 1) * stride + 3;
  }
  return a;
}

inline Tiling tiling(const Geo& g, bool dgrad) {
  Tiling t;
  t.r = dgrad ? axis(g.H, g.P, TR, g.sh, g.ph, true) : axis(g.P, g.H, TR, g.sh, g.ph, false);
  t.c = dgrad ? axis(g.W, g.Q, TC, g.sw, g.pw, true) : axis(g.Q, g.W, TC, g.sw, g.pw, false);
  t.C = g.C;
  t.ntiles = (uint32_t)((long long)g.N * t.r.tiles * t.c.tiles);
  t.fimg = make_fdiv((uint32_t)(t.r.tiles * t.c.tiles));
  t.ftc = make_fdiv((uint32_t)t.c.tiles);
  t.fext = make_fdiv((uint32_t)t.c.ext);
  return t;
}

inline unsigned channel_blocks(long long C) { return (unsigned)((C / 16 + BW - 1) / BW); }

// blocks of BW bundles on y; on x the tiles, evenly over at most about 4096 blocks in all
inline dim3 io_grid(const Tiling& t) {
  const unsigned gy = channel_blocks(t.C);
  unsigned cap = 4096 / gy;
  if (cap < 1) cap = 1;
  const unsigned per = (t.ntiles + cap - 1) / cap;
  return dim3((t.ntiles + per - 1) / per, gy);
}

inline size_t patch_lds(const Tiling& t) { return (size_t)t.r.ext * t.c.ext * PIXB; }

// Weight-gradient slabs of `per` consecutive tiles: about MAX_WG blocks, at least 4 tiles each
// (a slab's partial is C x 9 x Cg floats; with fewer tiles it outweighs the activations summed).
inline int wgrad_slabs(long long ntiles, long long C, int& per) {
  long long want = MAX_WG / channel_blocks(C);
  if (want < 1) want = 1;
  long long p = (ntiles + want - 1) / want;
  if (p < 4) p = 4;
  per = (int)p;
  return (int)((ntiles + p - 1) / p);
}

inline long long out_tiles(long long N, long long P, long long Q) {
  return N * ((P + TR - 1) / TR) * ((Q + TC - 1) / TC);
}

}  // namespace

#define SN_GROUPED_LAUNCH(KERNEL, GRID, LDS, ...)                                            \
  do {                                                                                       \
    if (Cg == 4)                                                                             \
      hipLaunchKernelGGL((KERNEL(4)), GRID, dim3(64 * BW), LDS, st, __VA_ARGS__);            \
    else if (Cg == 8)                                                                        \
      hipLaunchKernelGGL((KERNEL(8)), GRID, dim3(64 * BW), LDS, st, __VA_ARGS__);            \
    else                                                                                     \
      hipLaunchKernelGGL((KERNEL(16)), GRID, dim3(64 * BW), LDS, st, __VA_ARGS__);           \
  } while (0)
#define SN_FWD_K(CG) conv_grouped_io_k<CG, false>
#define SN_DGRAD_K(CG) conv_grouped_io_k<CG, true>
#define SN_WGRAD_K(CG) conv_grouped_wgrad_k<CG>

extern "C" {

// Floats the weight-gradient workspace needs for N x P x Q outputs of C channels in groups of Cg.
long long sn_conv_grouped_part_floats(long long N, long long P, long long Q, long long C, long long Cg) {
  if (N < 1 || P < 1 || Q < 1 || C < 16 || C % 16 != 0 || C > (1 << 20) || N * P * Q >= (1LL << 30)) return 0;
  if (Cg != 4 && Cg != 8 && Cg != 16) return 0;
  int per;
  return (long long)wgrad_slabs(out_tiles(N, P, Q), C, per) * C * 9 * Cg;
}

// y[N][P][Q][C] = relu?(3x3 conv of x[N][H][W][C] in groups of Cg with w[C][3][3][Cg] + bias); bias may be null.
int sn_conv_grouped_fwd(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, long long N, long long H,
                        long long W, long long C, long long Cg, long long sh, long long sw, long long ph,
                        long long pw, long long relu, hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, Cg, sh, sw, ph, pw, g)) return 3;
  if (!al16(x) || !al16(w) || !al16(y)) return 2;
  const Tiling t = tiling(g, false);
  SN_GROUPED_LAUNCH(SN_FWD_K, io_grid(t), patch_lds(t), x, w, bias, (const bf16_t*)nullptr, y, t, (int)relu);
  return SN_CHECK_LAUNCH();
}

// dx[N][H][W][C] = the data gradient of dy[N][P][Q][C], zeroed where gate <= 0 (gate shaped like
// dx; may be null).
int sn_conv_grouped_dgrad(const bf16_t* dy, const bf16_t* w, const bf16_t* gate, bf16_t* dx, long long N,
                          long long H, long long W, long long C, long long Cg, long long sh, long long sw,
                          long long ph, long long pw, hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, Cg, sh, sw, ph, pw, g)) return 3;
  if (!al16(dy) || !al16(w) || !al16(gate) || !al16(dx)) return 2;
  const Tiling t = tiling(g, true);
  SN_GROUPED_LAUNCH(SN_DGRAD_K, io_grid(t), patch_lds(t), dy, w, (const float*)nullptr, gate, dx, t, 0);
  return SN_CHECK_LAUNCH();
}

// dw[C][3][3][Cg] (fp32) from dy and x, stored (acc == 0) or accumulated.  part: workspace of
// part_floats >= sn_conv_grouped_part_floats(N, P, Q, C, Cg) floats.
int sn_conv_grouped_wgrad(const bf16_t* dy, const bf16_t* x, float* part, long long part_floats, float* dw,
                          long long acc, long long N, long long H, long long W, long long C, long long Cg,
                          long long sh, long long sw, long long ph, long long pw, hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, Cg, sh, sw, ph, pw, g)) return 3;
  if (!al16(dy) || !al16(x) || !al16(part) || !dw) return 2;
  const Tiling t = tiling(g, false);
  int per;
  const int slabs = wgrad_slabs(t.ntiles, C, per);
  const long long total = C * 9 * Cg;
  if (slabs * total > part_floats) return 3;
  SN_GROUPED_LAUNCH(SN_WGRAD_K, dim3((unsigned)slabs, channel_blocks(C)), patch_lds(t) + TR * TC * PIXB, dy, x, part,
                    t, per);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(conv_grouped_wgrad_finalize_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part,
                     slabs, total, dw, (int)acc);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
