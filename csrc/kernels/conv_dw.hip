// Depthwise 3x3 convolution (gfx950): groups == C == K, one filter per channel, NHWC bf16.
//
// Caffe runs a depthwise layer as C one-channel groups of im2col + GEMM (base_conv_layer.cpp);
// with 9 MACs per element the operator is purely bandwidth-bound and MFMA is the wrong tool, so
// these are plain per-channel kernels in the manner of bn_scale.hip:
//   forward   y = relu?(sum_rs x w + bias)                                  (1 read of x, 1 write)
//   dgrad     dx = sum over the taps that reach the input pixel, gathered   (1 read of dy, 1 write)
//             — nothing is scattered; dx = 0 where gate <= 0 (the ReLU that produced x)
//   wgrad     pass 1: per-(slab, channel) 9 tap sums and the dy sum (1 read of dy, 1 of x)
//             finalize: the slabs in a fixed order -> fp32 dw[C][3][3], db[C]
//
// Geometry: any stride and pad, no dilation, C % 8 == 0, every tensor 16-byte aligned.  The
// weights are read in place in the layer's layout [K][R][S][Cg = 1] = [C][3][3] bf16.  A lane
// owns 8 consecutive channels (16-byte accesses) and keeps their 72 weights and 8 bias values in
// registers as fp32; it computes a strip of QS = 4 neighbouring pixels of one row at a time.  At
// column stride 1 the QS + 2 columns of an input row a strip touches are loaded once and shared
// by its taps and outputs; at other strides every tap loads its own column.  A block is TX
// channel groups x TY strip lanes (TX * TY = 256, TX <= 64 a power of two); grid = (channel-group
// tiles, strip slabs); a lane strides over the strips of its slab.  Element offsets are 64-bit;
// strip indices stay below 2^31 (checked) and are decoded by multiply-shift division.
//
// Accumulation is fp32.  Every reduction is deterministic: the strip lanes of a wave are combined
// by a fixed butterfly, the four waves of a block in wave order, the slabs by the finalize launch
// in a fixed order (FL lanes, each over a contiguous run of slabs, then the lanes in lane order).
// No float atomics.
#include "common.h"

namespace {

enum { GRAD_SKIP = 0, GRAD_STORE = 1, GRAD_ACC = 2 };
constexpr int QS = 4;    // pixels of a strip
constexpr int NQ = 10;   // partials per channel: 9 tap sums, then the dy sum
constexpr int FO = 8;    // finalize block: FO outputs x FL slab lanes
constexpr int FL = 32;

struct Geo {
  int N, H, W, C, P, Q, sh, sw, ph, pw;
  int txlog;
  int nqs, rows;    // strips per row, rows per image of the tensor the strips walk
  long long strips, sps;  // strips in all, strips per slab
  FDiv fqs, frows, fsh, fsw;
};

struct Plan {
  int txlog, gx, slabs;
  long long sps;
};

// A slab holds at least `min_lane` strips per lane and `min_slab` strips; at most `cap` blocks.
inline Plan make_plan(long long strips, long long CG, int min_lane, int min_slab, int cap) {
  Plan p;
  p.txlog = 0;
  while ((1 << p.txlog) < 64 && (1LL << p.txlog) < CG) ++p.txlog;
  const int TX = 1 << p.txlog, TY = 256 >> p.txlog;
  p.gx = (int)((CG + TX - 1) / TX);
  long long capy = cap / p.gx;
  if (capy < 1) capy = 1;
  long long least = (long long)TY * min_lane;
  if (least < min_slab) least = min_slab;
  long long want = (strips + least - 1) / least;
  if (want > capy) want = capy;
  if (want < 1) want = 1;
  p.sps = (strips + want - 1) / want;
  p.slabs = (int)((strips + p.sps - 1) / p.sps);
  return p;
}

inline Plan io_plan(long long strips, long long C) { return make_plan(strips, C / 8, 2, 0, 4096); }
inline Plan red_plan(long long strips, long long C) { return make_plan(strips, C / 8, 2, 32, 1024); }

struct Lane {
  int cl, rl, TX, TY, c0;
  bool act;
  long long t0, t1;
};

SN_DEV Lane lane_of(const Geo& g) {
  Lane l;
  l.TX = 1 << g.txlog;
  l.TY = 256 >> g.txlog;
  l.cl = threadIdx.x & (l.TX - 1);
  l.rl = threadIdx.x >> g.txlog;
  l.c0 = (blockIdx.x * l.TX + l.cl) * 8;
  l.act = l.c0 < g.C;  // C % 8 == 0: an active lane's 8 channels are all inside
  l.t0 = blockIdx.y * g.sps;
  l.t1 = min(g.strips, l.t0 + g.sps);
  return l;
}

// strip t -> image n, row (of g.rows), first pixel of the strip in that row
SN_DEV void strip_of(const Geo& g, long long t, int& n, int& row, int& p0) {
  const uint32_t u = (uint32_t)t;
  const uint32_t line = udiv(u, g.fqs);
  p0 = (int)(u - line * (uint32_t)g.nqs) * QS;
  n = (int)udiv(line, g.frows);
  row = (int)(line - (uint32_t)n * (uint32_t)g.rows);
}

// the lane's 8 x 9 weights: wv[j * 9 + tap], channel c0 + j
SN_DEV void load_w(const bf16_t* __restrict__ w, int c0, float* wv) {
  const uint4* p = reinterpret_cast<const uint4*>(w + (long long)c0 * 9);
#pragma unroll
  for (int i = 0; i < 9; ++i) unpack8(p[i], wv + 8 * i);
}

SN_DEV uint4 ld8(const bf16_t* __restrict__ p, long long e, bool ok) {
  return ok ? *reinterpret_cast<const uint4*>(p + e) : make_uint4(0u, 0u, 0u, 0u);
}

template <bool S1>
struct Cols {
  static constexpr int N = S1 ? QS + 2 : QS * 3;
  static SN_DEV constexpr int at(int j, int s) { return S1 ? j + s : j * 3 + s; }
};

// The columns of row `line` (pixel index of its column 0; read only when ok) of a [.][W][C]
// tensor that the taps s = 0..2 of the strip's QS outputs read: column w0 + j * sw + s for
// (j, s), zero outside [0, W).  S1 (sw == 1): the QS + 2 distinct columns, once.
template <bool S1>
SN_DEV void load_cols(const bf16_t* __restrict__ x, long long line, bool ok, int w0, int sw, int W, int C, int c0,
                      uint4* raw) {
#pragma unroll
  for (int i = 0; i < Cols<S1>::N; ++i) {
    const int wc = S1 ? w0 + i : w0 + (i / 3) * sw + i % 3;
    raw[i] = ld8(x, (line + wc) * C + c0, ok && wc >= 0 && wc < W);
  }
}

// ---------------------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------------------
template <bool S1>
__global__ void __launch_bounds__(256) conv_dw_fwd_k(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                     const float* __restrict__ bias, bf16_t* __restrict__ y,
                                                     const Geo g, int relu) {
  const Lane l = lane_of(g);
  if (!l.act) return;
  float wv[72], bv[8];
  load_w(w, l.c0, wv);
#pragma unroll
  for (int c = 0; c < 8; ++c) bv[c] = bias ? bias[l.c0 + c] : 0.f;
  for (long long t = l.t0 + l.rl; t < l.t1; t += l.TY) {
    int n, p, q0;
    strip_of(g, t, n, p, q0);
    float acc[QS][8];
#pragma unroll
    for (int j = 0; j < QS; ++j)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[j][c] = bv[c];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int h = p * g.sh - g.ph + r;
      uint4 raw[Cols<S1>::N];
      load_cols<S1>(x, ((long long)n * g.H + h) * g.W, h >= 0 && h < g.H, q0 * g.sw - g.pw, g.sw, g.W, g.C, l.c0, raw);
#pragma unroll
      for (int j = 0; j < QS; ++j)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          float f[8];
          unpack8(raw[Cols<S1>::at(j, s)], f);
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[j][c] = fmaf(f[c], wv[c * 9 + r * 3 + s], acc[j][c]);
        }
    }
    const long long o = (((long long)n * g.P + p) * g.Q + q0) * g.C + l.c0;
#pragma unroll
    for (int j = 0; j < QS; ++j) {
      if (q0 + j >= g.Q) break;  // the strip tail
      if (relu) {
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[j][c] = fmaxf(acc[j][c], 0.f);
      }
      *reinterpret_cast<uint4*>(y + o + (long long)j * g.C) = pack8(acc[j]);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Data gradient, gather form: input pixel (h, w) receives dy[(h + ph - r) / sh][(w + pw - s) / sw]
// w[r][s] from every tap whose two quotients are exact and inside the output.
// ---------------------------------------------------------------------------------------
template <bool S1>
__global__ void __launch_bounds__(256) conv_dw_dgrad_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ w,
                                                       const bf16_t* __restrict__ gate, bf16_t* __restrict__ dx,
                                                       const Geo g) {
  const Lane l = lane_of(g);
  if (!l.act) return;
  float wv[72];
  load_w(w, l.c0, wv);
  for (long long t = l.t0 + l.rl; t < l.t1; t += l.TY) {
    int n, h, w0;
    strip_of(g, t, n, h, w0);
    float acc[QS][8];
#pragma unroll
    for (int j = 0; j < QS; ++j)
#pragma unroll
      for (int c = 0; c < 8; ++c) acc[j][c] = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int th = h + g.ph - r;
      const int p = (int)udiv((uint32_t)max(th, 0), g.fsh);
      const bool ok = th >= 0 && p * g.sh == th && p < g.P;
      const long long line = ((long long)n * g.P + p) * g.Q;
      uint4 raw[Cols<S1>::N];
      if constexpr (S1) {
        // output column of (j, s) is w0 + j + pw - s = (w0 + pw - 2) + (j + 2 - s)
        load_cols<true>(dy, line, ok, w0 + g.pw - 2, 1, g.Q, g.C, l.c0, raw);
      } else {
#pragma unroll
        for (int j = 0; j < QS; ++j)
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            const int tw = w0 + j + g.pw - s;
            const int q = (int)udiv((uint32_t)max(tw, 0), g.fsw);
            raw[j * 3 + s] = ld8(dy, (line + q) * g.C + l.c0, ok && tw >= 0 && q * g.sw == tw && q < g.Q);
          }
      }
#pragma unroll
      for (int j = 0; j < QS; ++j)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
          float f[8];
          unpack8(raw[S1 ? j + 2 - s : j * 3 + s], f);
#pragma unroll
          for (int c = 0; c < 8; ++c) acc[j][c] = fmaf(f[c], wv[c * 9 + r * 3 + s], acc[j][c]);
        }
    }
    const long long o = (((long long)n * g.H + h) * g.W + w0) * g.C + l.c0;
#pragma unroll
    for (int j = 0; j < QS; ++j) {
      if (w0 + j >= g.W) break;
      const long long e = o + (long long)j * g.C;
      if (gate) {
        float gv[8];
        unpack8(*reinterpret_cast<const uint4*>(gate + e), gv);
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[j][c] = gv[c] > 0.f ? acc[j][c] : 0.f;
      }
      *reinterpret_cast<uint4*>(dx + e) = pack8(acc[j]);
    }
  }
}

// ---------------------------------------------------------------------------------------
// Weight / bias gradient pass 1: part[slab][k][C], k = r * 3 + s: sum dy x(tap), k = 9: sum dy
// ---------------------------------------------------------------------------------------
template <bool S1>
__global__ void __launch_bounds__(256) conv_dw_wgrad_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                       float* __restrict__ part, const Geo g) {
  __shared__ float sm[4 * 8 * 64];
  const Lane l = lane_of(g);
  float acc[NQ][8];
#pragma unroll
  for (int k = 0; k < NQ; ++k)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[k][c] = 0.f;
  if (l.act) {
    for (long long t = l.t0 + l.rl; t < l.t1; t += l.TY) {
      int n, p, q0;
      strip_of(g, t, n, p, q0);
      const long long o = (((long long)n * g.P + p) * g.Q + q0) * g.C + l.c0;
      float d[QS][8];
#pragma unroll
      for (int j = 0; j < QS; ++j) {
        unpack8(ld8(dy, o + (long long)j * g.C, q0 + j < g.Q), d[j]);
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[9][c] += d[j][c];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const int h = p * g.sh - g.ph + r;
        uint4 raw[Cols<S1>::N];
        load_cols<S1>(x, ((long long)n * g.H + h) * g.W, h >= 0 && h < g.H, q0 * g.sw - g.pw, g.sw, g.W, g.C, l.c0,
                      raw);
#pragma unroll
        for (int j = 0; j < QS; ++j)
#pragma unroll
          for (int s = 0; s < 3; ++s) {
            float f[8];
            unpack8(raw[Cols<S1>::at(j, s)], f);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[r * 3 + s][c] = fmaf(d[j][c], f[c], acc[r * 3 + s][c]);
          }
      }
    }
  }
  // strip lanes of a wave by a fixed butterfly (lanes TX apart share their channels), then the
  // four waves in wave order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NQ; ++k) {
    float v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = acc[k][c];
    for (int o = l.TX; o < 64; o <<= 1) {
#pragma unroll
      for (int c = 0; c < 8; ++c) v[c] += __shfl_xor(v[c], o, 64);
    }
    if (lane < l.TX) {
#pragma unroll
      for (int c = 0; c < 8; ++c) sm[(wave * 8 + c) * 64 + lane] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < l.TX && l.act) {
      // TX == 64: a wave is one strip lane and the four waves are the block's four;
      // TX < 64: every wave holds its own strip lanes' sum
      float a[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        a[c] = sm[c * 64 + lane];
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) a[c] += sm[(wv * 8 + c) * 64 + lane];
      }
      float* dst = part + ((long long)blockIdx.y * NQ + k) * g.C + l.c0;
      *reinterpret_cast<float4*>(dst) = make_float4(a[0], a[1], a[2], a[3]);
      *reinterpret_cast<float4*>(dst + 4) = make_float4(a[4], a[5], a[6], a[7]);
    }
    __syncthreads();
  }
}

// Slab sums in a fixed order; output o = k * C + c of the NQ * C per-slab partials goes to
// dw[c][k] (k < 9) or db[c] (k == 9), stored, accumulated or skipped.
__global__ void __launch_bounds__(FO * FL) conv_dw_wgrad_finalize_k(const float* __restrict__ part, int slabs, int C,
                                                                    float* __restrict__ dw, int wflag,
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
  if (tap < 9) {
    if (wflag != GRAD_SKIP) {
      float* d = dw + (long long)c * 9 + tap;
      *d = wflag == GRAD_ACC ? *d + a : a;
    }
  } else if (bflag != GRAD_SKIP) {
    db[c] = bflag == GRAD_ACC ? db[c] + a : a;
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Output size and the limits of the index arithmetic; false for a geometry the kernels do not take.
inline bool geometry(long long N, long long H, long long W, long long C, long long sh, long long sw, long long ph,
                     long long pw, Geo& g) {
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 != 0 || sh < 1 || sw < 1 || ph < 0 || pw < 0) return false;
  if (H + 2 * ph < 3 || W + 2 * pw < 3) return false;
  const long long P = (H + 2 * ph - 3) / sh + 1, Q = (W + 2 * pw - 3) / sw + 1;
  const long long lim = 1LL << 30;
  if (C > lim / 16 || sh > lim || sw > lim || ph > lim || pw > lim) return false;
  if (N * H * W >= lim || N * P * Q >= lim) return false;
  g.N = (int)N; g.H = (int)H; g.W = (int)W; g.C = (int)C; g.P = (int)P; g.Q = (int)Q;
  g.sh = (int)sh; g.sw = (int)sw; g.ph = (int)ph; g.pw = (int)pw;
  g.fsh = make_fdiv((uint32_t)sh);
  g.fsw = make_fdiv((uint32_t)sw);
  return true;
}

// the strips walk rows of `width` pixels, `rows` of them per image
inline Plan strips_over(Geo& g, int rows, int width, bool reduce) {
  g.rows = rows;
  g.nqs = (width + QS - 1) / QS;
  g.strips = (long long)g.N * rows * g.nqs;
  g.frows = make_fdiv((uint32_t)rows);
  g.fqs = make_fdiv((uint32_t)g.nqs);
  const Plan p = reduce ? red_plan(g.strips, g.C) : io_plan(g.strips, g.C);
  g.txlog = p.txlog;
  g.sps = p.sps;
  return p;
}

}  // namespace

#define SN_DW_LAUNCH(KERNEL, ...)                                                            \
  do {                                                                                       \
    const dim3 grid((unsigned)pl.gx, (unsigned)pl.slabs);                                    \
    if (g.sw == 1)                                                                           \
      hipLaunchKernelGGL((KERNEL<true>), grid, dim3(256), 0, st, __VA_ARGS__);               \
    else                                                                                     \
      hipLaunchKernelGGL((KERNEL<false>), grid, dim3(256), 0, st, __VA_ARGS__);              \
  } while (0)

extern "C" {

// Floats the weight-gradient workspace needs for N x P x Q outputs of C channels.
long long sn_conv_dw_part_floats(long long N, long long P, long long Q, long long C) {
  if (N < 1 || P < 1 || Q < 1 || C < 8 || C % 8 != 0 || N * P * Q >= (1LL << 30)) return 0;
  const long long strips = N * P * ((Q + QS - 1) / QS);
  return (long long)red_plan(strips, C).slabs * NQ * C;
}

// y[N][P][Q][C] = relu?(depthwise 3x3 of x[N][H][W][C] with w[C][3][3] + bias); bias may be null.
int sn_conv_dw_fwd(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, long long N, long long H,
                   long long W, long long C, long long sh, long long sw, long long ph, long long pw, long long relu,
                   hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, sh, sw, ph, pw, g)) return 3;
  if (!al16(x) || !al16(w) || !al16(y)) return 2;
  const Plan pl = strips_over(g, g.P, g.Q, false);
  SN_DW_LAUNCH(conv_dw_fwd_k, x, w, bias, y, g, (int)relu);
  return SN_CHECK_LAUNCH();
}

// dx[N][H][W][C] = the data gradient of dy[N][P][Q][C], zeroed where gate <= 0 (gate shaped like
// dx; may be null).
int sn_conv_dw_dgrad(const bf16_t* dy, const bf16_t* w, const bf16_t* gate, bf16_t* dx, long long N, long long H,
                     long long W, long long C, long long sh, long long sw, long long ph, long long pw, hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, sh, sw, ph, pw, g)) return 3;
  if (!al16(dy) || !al16(w) || !al16(gate) || !al16(dx)) return 2;
  const Plan pl = strips_over(g, g.H, g.W, false);
  SN_DW_LAUNCH(conv_dw_dgrad_k, dy, w, gate, dx, g);
  return SN_CHECK_LAUNCH();
}

// dw[C][3][3] and db[C] (fp32) from dy and x.  dw_flag / db_flag: 0 skip, 1 store, 2 accumulate.
// part: workspace of part_floats >= sn_conv_dw_part_floats(N, P, Q, C) floats.
int sn_conv_dw_wgrad(const bf16_t* dy, const bf16_t* x, float* part, long long part_floats, float* dw,
                     long long dw_flag, float* db, long long db_flag, long long N, long long H, long long W,
                     long long C, long long sh, long long sw, long long ph, long long pw, hipStream_t st) {
  Geo g;
  if (!geometry(N, H, W, C, sh, sw, ph, pw, g)) return 3;
  if (!al16(dy) || !al16(x) || !al16(part)) return 2;
  if ((dw_flag != GRAD_SKIP && !dw) || (db_flag != GRAD_SKIP && !db)) return 2;
  const Plan pl = strips_over(g, g.P, g.Q, true);
  if ((long long)pl.slabs * NQ * C > part_floats) return 3;
  SN_DW_LAUNCH(conv_dw_wgrad_k, dy, x, part, g);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(conv_dw_wgrad_finalize_k, dim3((unsigned)((NQ * C + FO - 1) / FO)), dim3(FO * FL), 0, st, part,
                     pl.slabs, (int)C, dw, (int)dw_flag, db, (int)db_flag);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
