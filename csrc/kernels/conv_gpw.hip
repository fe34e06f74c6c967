// Grouped pointwise (1x1) convolution and channel shuffle (gfx950): ShuffleNet's arithmetic.
//
// With a 1x1 window, stride 1 and no pad the image structure vanishes: x is [M][C], y is [M][K] with
// M = N H W flat rows, and group g is the product [M][Cg] x [Cg][Kg] on columns g Cg .. of x and
// g Kg .. of y.  Cg and Kg are multiples of 4 and free to differ (ShuffleNet 1x g=3: 20, 60, 72, 80,
// 160, 320 per group; g=8: 12 .. 192), so neither the 8-channel lanes of the implicit grouped GEMM
// nor the Cg == Kg bundles of conv_grouped.hip fit.  Everything is NHWC bf16, weights [K][1][1][Cg]
// read in place, v_mfma_f32_16x16x32_bf16 throughout.
//
//   forward   one kernel for forward and data gradient ("io"): dst[M][G No] = src[M][G Nr] x W_g with
//   dgrad     Nr reduced and No output channels per group (forward Nr = Cg, No = Kg; data gradient
//             the other way round, src = dy).  A persistent block of four waves runs over a
//             contiguous range of (group, 64-row tile) items, group-major, and keeps the group's
//             weight matrix in LDS as [16 OF][32 RS] bf16 (OF = ceil(No / 16) output fragments, RS =
//             ceil(Nr / 32) reduction steps), staged when the group changes: in place for the
//             forward, transposed on the way in for the data gradient (the [Kg][Cg] matrix is reduced
//             over its rows there; no flip pass, no second copy in global memory).  Per item the
//             block stages the 64 x Nr source tile; a wave owns 16 rows and walks the output
//             fragments four at a time (one 16-byte LDS read per operand and step).  BOTH operands'
//             padding is zeroed in LDS: weight rows past No and columns past Nr, and source columns
//             past Nr, which in global memory are the neighbouring group's channels; an Inf or NaN
//             there would otherwise reach this group as Inf x 0.  Rows past M are zero too.  The
//             output tile goes through LDS (fp32 bias, ReLU, one rounding to bf16) and leaves in
//             16-byte stores when No % 8 == 0 and 8-byte ones otherwise; the data gradient's ReLU
//             gate (gate <= 0 zeroes dx) is applied in that store.
//   wgrad     dw[g] = dy_g^T x_g, reduced over the rows.  A block owns a group and a slab of
//             consecutive 64-row tiles, stages the dy and x tiles side by side and reads both operands
//             transposed from them (ds_read_b64_tr_b16: the rows are the k of the MFMA).  The group's
//             ceil(Kg / 16) x ceil(Cg / 16) output fragments are cut into bands of whole fragment
//             rows of at most 48 fragments (16 where that still leaves few blocks), a band per block
//             (grid z), which stages only its band's dy columns; a band's fragments are dealt
//             round-robin to the four waves, at most 12 each, all in registers (Cg <= 768: a wider
//             group does not pass the data gradient's LDS check either).
//             The first version gave a block the whole group (25 accumulators a wave at 80 x 320)
//             and lost to the implicit GEMM at 7 x 7 images, where 21 blocks were all it launched.
//             Each block writes its part of the slab's fp32 partial [K][Cg];
//             conv_gpw_wgrad_finalize_k sums the slabs in slab order and stores or accumulates onto
//             dw.  No atomics: bitwise reproducible.  The bias gradient stays on the column-sum launch.
//   shuffle   y[m][j G + i] = x[m][i (C / G) + j]: a block stages a run of whole rows (they are
//             contiguous) in LDS and writes the permuted rows, eight channels per 16-byte store when
//             C % 8 == 0 and one channel per lane otherwise.  The backward pass is the same kernel
//             with C / G in place of G.  Element offsets are 64-bit.
//
// The io kernels are not double-buffered: a block's LDS is at most a third of a CU's for the
// ShuffleNet shapes, so two or three blocks of a CU overlap each other's loads (said in the README
// under "Not done").
//
// Limits (checked in the C entries; hip.gpw_ok mirrors them): groups >= 2, Cg % 4 == 0, Kg % 4 == 0,
// both at most 1024, the three LDS regions of either io product within 160 KB, M < 2^30 rows,
// groups x tiles < 2^31, tensors dense and 8-byte aligned (16-byte when the 16-byte paths are taken:
// the Python side routes 16-byte aligned tensors only).
#include "common.h"

namespace {

constexpr int NT = 256;             // threads of a block: four waves
constexpr int TM = 64;              // rows of a tile: 16 per wave
constexpr int PADB = 16;            // bytes added to every LDS row: consecutive rows start 4 banks apart
constexpr int MAX_WIDTH = 1024;     // channels per group on either side
constexpr int BAND_FRAGS = 48;      // weight-gradient fragments of a block: 12 per wave
constexpr int BAND_FRAGS_SMALL = 16;  // the same where the launch would otherwise have fewer than WG_BLOCKS / 2 blocks
constexpr int LDS_LIMIT = 160 * 1024;
constexpr int WG_MIN_TILES = 4;     // tiles per weight-gradient slab at least: a slab's partial is Kg Cg floats
constexpr int WG_BLOCKS = 512;      // weight-gradient blocks aimed at: two per CU
enum { GRAD_SKIP = 0, GRAD_STORE = 1, GRAD_ACC = 2 };

struct Io {
  int M, G, Nr, No;       // rows, groups, reduced and output channels per group
  int RS, OF;             // reduction steps of 32, output fragments of 16
  int rsb, osb;           // LDS bytes of a weight / source row and of an output row
  uint32_t tiles, items;  // 64-row tiles, groups x tiles
  int per;                // consecutive items of a block
  FDiv ftiles, frc, foc, fo4;  // / tiles, / 8-byte chunks of a staged row, / store chunks and / 8-byte chunks of an output row
};

struct Wg {
  int M, G, Cg, Kg, KF, CF;  // fragments of 16 output (dy) and input (x) channels
  int KB, nz;                // fragment rows of a band, bands
  int dsb, xsb;              // LDS bytes of a staged dy / x row
  uint32_t tiles;
  int per;                   // tiles of a slab
  FDiv fdc, fxc;             // / 8-byte chunks of a staged dy / x row
};

SN_DEV uint2 ld4(const bf16_t* __restrict__ p, long long e, bool ok) {
  return ok ? *reinterpret_cast<const uint2*>(p + e) : make_uint2(0u, 0u);
}

// rows m0 .. m0 + TM - 1 of src [M][ld], columns c0 .. c0 + n - 1, at sm as rows of `rowb` bytes
// holding `chunks` 8-byte chunks; zero past M and past n (the neighbouring group's channels).
SN_DEV void stage_rows(const bf16_t* __restrict__ src, int M, long long ld, int m0, int c0, int n, int chunks,
                       const FDiv& fchunks, int rowb, unsigned char* sm) {
  for (int i = threadIdx.x; i < TM * chunks; i += NT) {
    const int r = (int)udiv((uint32_t)i, fchunks), c4 = i - r * chunks;
    const bool ok = m0 + r < M && 4 * c4 < n;
    *reinterpret_cast<uint2*>(sm + r * rowb + c4 * 8) = ld4(src, (long long)(m0 + r) * ld + c0 + 4 * c4, ok);
  }
}

// ---------------------------------------------------------------------------------------
// Forward (src = x, Nr = Cg, No = Kg) and data gradient (src = dy, Nr = Kg, No = Cg)
// ---------------------------------------------------------------------------------------
template <bool DGRAD>
__global__ void __launch_bounds__(NT) conv_gpw_io_k(const bf16_t* __restrict__ src, const bf16_t* __restrict__ w,
                                                    const float* __restrict__ bias,
                                                    const bf16_t* __restrict__ gate, bf16_t* __restrict__ dst,
                                                    const Io p, int relu) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  unsigned char* wm = sm;                        // [16 OF][rsb]: output channel x reduced channel
  unsigned char* xs = wm + 16 * p.OF * p.rsb;    // [TM][rsb]
  unsigned char* ot = xs + TM * p.rsb;           // [TM][osb]
  float* bs = reinterpret_cast<float*>(ot + TM * p.osb);  // [16 OF]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int chunks = 8 * p.RS;  // 8-byte chunks of a weight / source row
  const long long lds_ = (long long)p.G * p.Nr, ldd = (long long)p.G * p.No;
  const uint32_t i0 = blockIdx.x * (uint32_t)p.per, i1 = min(p.items, i0 + (uint32_t)p.per);
  int cur = -1;
  for (uint32_t it = i0; it < i1; ++it) {
    const int g = (int)udiv(it, p.ftiles), m0 = (int)(it - (uint32_t)g * p.tiles) * TM;
    __syncthreads();  // the previous item's reads of xs and ot are done
    if (g != cur) {   // uniform over the block
      cur = g;
      for (int i = threadIdx.x; i < 16 * p.OF; i += NT) bs[i] = (bias && i < p.No) ? bias[g * p.No + i] : 0.f;
      if (!DGRAD) {  // w rows g No + o are the matrix's rows
        for (int i = threadIdx.x; i < 16 * p.OF * chunks; i += NT) {
          const int o = (int)udiv((uint32_t)i, p.frc), c4 = i - o * chunks;
          *reinterpret_cast<uint2*>(wm + o * p.rsb + c4 * 8) =
              ld4(w, ((long long)g * p.No + o) * p.Nr + 4 * c4, o < p.No && 4 * c4 < p.Nr);
        }
      } else {  // w rows g Nr + k hold the matrix's columns: w[g Nr + k][o] -> wm[o][k]
        for (int i = threadIdx.x; i < 16 * p.OF * chunks; i += NT) {
          const int o = (int)udiv((uint32_t)i, p.frc), c4 = i - o * chunks;
          *reinterpret_cast<uint2*>(wm + o * p.rsb + c4 * 8) = make_uint2(0u, 0u);
        }
        __syncthreads();
        const int oc = p.No >> 2;  // 8-byte chunks of a w row
        for (int i = threadIdx.x; i < p.Nr * oc; i += NT) {
          const int k = (int)udiv((uint32_t)i, p.fo4), o4 = i - k * oc;
          const uint2 v = *reinterpret_cast<const uint2*>(w + ((long long)g * p.Nr + k) * p.No + 4 * o4);
          bf16_t* d = reinterpret_cast<bf16_t*>(wm + (4 * o4) * p.rsb) + k;
          const int rs2 = p.rsb >> 1;
          d[0] = (bf16_t)(v.x & 0xffffu);
          d[rs2] = (bf16_t)(v.x >> 16);
          d[2 * rs2] = (bf16_t)(v.y & 0xffffu);
          d[3 * rs2] = (bf16_t)(v.y >> 16);
        }
      }
    }
    stage_rows(src, p.M, lds_, m0, g * p.Nr, p.Nr, chunks, p.frc, p.rsb, xs);
    __syncthreads();
    // the wave's 16 rows x four output fragments at a time
    const unsigned char* brow = xs + (wave * 16 + (lane & 15)) * p.rsb + (lane >> 4) * 16;
    const unsigned char* arow = wm + (lane & 15) * p.rsb + (lane >> 4) * 16;
    for (int f0 = 0; f0 < p.OF; f0 += 4) {
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int ks = 0; ks < p.RS; ++ks) {
        const bf16x8_t b = *reinterpret_cast<const bf16x8_t*>(brow + ks * 64);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (f0 + j < p.OF)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                *reinterpret_cast<const bf16x8_t*>(arow + (f0 + j) * 16 * p.rsb + ks * 64), b, acc[j], 0, 0, 0);
      }
      // acc[j][i]: output channel 16 (f0 + j) + 4 (lane >> 4) + i of row lane & 15
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (f0 + j >= p.OF) continue;
        const int ch = 16 * (f0 + j) + 4 * (lane >> 4);
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = acc[j][i] + bs[ch + i];
          if (relu) v[i] = fmaxf(v[i], 0.f);
        }
        *reinterpret_cast<uint2*>(ot + (wave * 16 + (lane & 15)) * p.osb + ch * 2) =
            make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
      }
    }
    __syncthreads();
    // the tile's No columns of rows below M, gated
    if ((p.No & 7) == 0) {
      const int oc = p.No >> 3;
      for (int i = threadIdx.x; i < TM * oc; i += NT) {
        const int r = (int)udiv((uint32_t)i, p.foc), c8 = i - r * oc;
        if (m0 + r >= p.M) continue;
        uint4 v = *reinterpret_cast<const uint4*>(ot + r * p.osb + c8 * 16);
        const long long e = (long long)(m0 + r) * ldd + g * p.No + 8 * c8;
        if (gate) {
          const uint4 gv = *reinterpret_cast<const uint4*>(gate + e);
          float f[8], gf[8];
          unpack8(v, f);
          unpack8(gv, gf);
#pragma unroll
          for (int k = 0; k < 8; ++k) f[k] = gf[k] > 0.f ? f[k] : 0.f;
          v = pack8(f);
        }
        *reinterpret_cast<uint4*>(dst + e) = v;
      }
    } else {
      const int oc = p.No >> 2;
      for (int i = threadIdx.x; i < TM * oc; i += NT) {
        const int r = (int)udiv((uint32_t)i, p.foc), c4 = i - r * oc;
        if (m0 + r >= p.M) continue;
        uint2 v = *reinterpret_cast<const uint2*>(ot + r * p.osb + c4 * 8);
        const long long e = (long long)(m0 + r) * ldd + g * p.No + 4 * c4;
        if (gate) {
          const uint2 gv = *reinterpret_cast<const uint2*>(gate + e);
          if (!(__uint_as_float(gv.x << 16) > 0.f)) v.x &= 0xffff0000u;
          if (!(__uint_as_float(gv.x & 0xffff0000u) > 0.f)) v.x &= 0x0000ffffu;
          if (!(__uint_as_float(gv.y << 16) > 0.f)) v.y &= 0xffff0000u;
          if (!(__uint_as_float(gv.y & 0xffff0000u) > 0.f)) v.y &= 0x0000ffffu;
        }
        *reinterpret_cast<uint2*>(dst + e) = v;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------
// Weight gradient pass 1: part[slab][K][Cg], the slab's rows of dy_g^T x_g
// ---------------------------------------------------------------------------------------

// 8 staged rows as an MFMA operand with the rows along k: a0 addresses 4 channels of row q of the
// lane's 8, a0 + second the same of row q + 4 (ds_read_b64_tr_b16; see conv_grouped.hip).
SN_DEV bf16x8_t tr_frag(const unsigned char* a0, int second) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + second));
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, r);
}

// NA: accumulators of a wave; fragment f = kf CF + cf of the block's band belongs to wave f % 4 as its (f / 4)-th
template <int NA>
__global__ void __launch_bounds__(NT) conv_gpw_wgrad_k(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ x,
                                                       float* __restrict__ part, const Wg p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  unsigned char* ds = sm;                // [TM][dsb]
  unsigned char* xs = sm + TM * p.dsb;   // [TM][xsb]
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = blockIdx.y;
  const int kf0 = blockIdx.z * p.KB, kfn = min(p.KB, p.KF - kf0);  // the band's fragment rows
  const long long K = (long long)p.G * p.Kg, C = (long long)p.G * p.Cg;
  f32x4 acc[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // the lane's address in a transposed read: row 8 (lane >> 4) + q, then + 4; channels 4 pq .. + 3
  const int row = 8 * (lane >> 4) + ((lane & 15) >> 2), coff = 8 * (lane & 3);
  const unsigned char* a0 = ds + row * p.dsb + coff;
  const unsigned char* b0 = xs + row * p.xsb + coff;
  const uint32_t t0 = blockIdx.x * (uint32_t)p.per, t1 = min(p.tiles, t0 + (uint32_t)p.per);
  for (uint32_t t = t0; t < t1; ++t) {
    const int m0 = (int)t * TM;
    __syncthreads();  // the previous tile's reads are done
    stage_rows(dy, p.M, K, m0, g * p.Kg + 16 * kf0, min(p.Kg - 16 * kf0, 16 * p.KB), 4 * p.KB, p.fdc, p.dsb, ds);
    stage_rows(x, p.M, C, m0, g * p.Cg, p.Cg, 4 * p.CF, p.fxc, p.xsb, xs);
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < TM / 32; ++ks) {
      int kf = 0, cf = wave;
      while (cf >= p.CF) { cf -= p.CF; ++kf; }
#pragma unroll
      for (int j = 0; j < NA; ++j) {
        if (kf < kfn)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_frag(a0 + ks * 32 * p.dsb + kf * 32, 4 * p.dsb),
                                                           tr_frag(b0 + ks * 32 * p.xsb + cf * 32, 4 * p.xsb), acc[j],
                                                           0, 0, 0);
        cf += 4;
        while (cf >= p.CF) { cf -= p.CF; ++kf; }
      }
    }
  }
  // acc[j][i]: output channel 16 kf + 4 (lane >> 4) + i (the row), input channel 16 cf + (lane & 15)
  float* dst = part + ((long long)blockIdx.x * K + (long long)g * p.Kg) * p.Cg;
  int kf = 0, cf = wave;
  while (cf >= p.CF) { cf -= p.CF; ++kf; }
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const int c = 16 * cf + (lane & 15);
    if (kf < kfn && c < p.Cg) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 16 * (kf0 + kf) + 4 * (lane >> 4) + i;
        if (k < p.Kg) dst[(long long)k * p.Cg + c] = acc[j][i];
      }
    }
    cf += 4;
    while (cf >= p.CF) { cf -= p.CF; ++kf; }
  }
}

// The slabs in slab order, stored or accumulated onto dw.
__global__ void __launch_bounds__(256) conv_gpw_wgrad_finalize_k(const float* __restrict__ part, int slabs,
                                                                 long long total, float* __restrict__ dw, int flag) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  float a = 0.f;
#pragma unroll 4
  for (int s = 0; s < slabs; ++s) a += part[(long long)s * total + o];
  dw[o] = flag == GRAD_ACC ? dw[o] + a : a;
}

// ---------------------------------------------------------------------------------------
// Channel shuffle: V channels of an output row per lane
// ---------------------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(NT) shuffle_channel_k(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                        long long M, int C, int G, int rows, FDiv fcv, FDiv fg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(sm);  // [rows][C]
  const int cv = C / V, per = C / G;            // lanes of a row; channels of a group
  const long long runs = (M + rows - 1) / rows;
  for (long long run = blockIdx.x; run < runs; run += gridDim.x) {
    const long long m0 = run * rows, e0 = m0 * C;
    const int n = (int)min((long long)rows, M - m0) * cv;  // lanes of the run: its rows are contiguous
    __syncthreads();  // the previous run's reads are done
    for (int i = threadIdx.x; i < n; i += NT) {
      if (V == 8)
        reinterpret_cast<uint4*>(xs)[i] = reinterpret_cast<const uint4*>(x + e0)[i];
      else
        xs[i] = x[e0 + i];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += NT) {
      const int r = (int)udiv((uint32_t)i, fcv), co = (i - r * cv) * V;
      int j = (int)udiv((uint32_t)co, fg), g = co - j * G;  // output channel co = j G + g reads g per + j
      const bf16_t* s = xs + r * C;
      if (V == 8) {
        uint32_t u[4];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const uint32_t v = s[g * per + j];
          u[k >> 1] = (k & 1) ? (u[k >> 1] | (v << 16)) : v;
          if (++g == G) { g = 0; ++j; }
        }
        *reinterpret_cast<uint4*>(y + e0 + (long long)r * C + co) = make_uint4(u[0], u[1], u[2], u[3]);
      } else {
        y[e0 + (long long)r * C + co] = s[g * per + j];
      }
    }
  }
}

inline bool al(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
inline int cdiv(long long a, int b) { return (int)((a + b - 1) / b); }

inline bool widths_ok(long long M, long long G, long long Cg, long long Kg) {
  return M >= 1 && M < (1LL << 30) && G >= 2 && G <= (1 << 20) && Cg >= 4 && Kg >= 4 && Cg % 4 == 0 && Kg % 4 == 0 &&
         Cg <= MAX_WIDTH && Kg <= MAX_WIDTH && G * ((M + TM - 1) / TM) < (1LL << 31);
}

inline size_t io_lds(const Io& p) {
  return (size_t)(16 * p.OF + TM) * p.rsb + (size_t)TM * p.osb + (size_t)16 * p.OF * sizeof(float);
}

// false for a geometry the io kernels do not take, the LDS budget included
inline bool io_plan(long long M, long long G, long long Nr, long long No, Io& p) {
  if (!widths_ok(M, G, Nr, No)) return false;
  p.M = (int)M; p.G = (int)G; p.Nr = (int)Nr; p.No = (int)No;
  p.RS = cdiv(Nr, 32);
  p.OF = cdiv(No, 16);
  p.rsb = 64 * p.RS + PADB;
  p.osb = 32 * p.OF + PADB;
  if (io_lds(p) > (size_t)LDS_LIMIT) return false;
  p.tiles = (uint32_t)cdiv(M, TM);
  p.items = (uint32_t)(G * p.tiles);
  // as many blocks as stay resident (by LDS, at most 4 per CU), each a contiguous range of items
  long long fit = LDS_LIMIT / (long long)io_lds(p);
  if (fit > 4) fit = 4;
  const long long want = fit * sn_cu_count();
  p.per = (int)((p.items + want - 1) / want);
  p.ftiles = make_fdiv(p.tiles);
  p.frc = make_fdiv((uint32_t)(8 * p.RS));
  p.foc = make_fdiv((uint32_t)((No & 7) == 0 ? No >> 3 : No >> 2));
  p.fo4 = make_fdiv((uint32_t)(No >> 2));
  return true;
}

inline bool wg_plan(long long M, long long G, long long Cg, long long Kg, Wg& p, int& slabs) {
  if (!widths_ok(M, G, Cg, Kg) || G > 65535) return false;
  p.M = (int)M; p.G = (int)G; p.Cg = (int)Cg; p.Kg = (int)Kg;
  p.KF = cdiv(Kg, 16);
  p.CF = cdiv(Cg, 16);
  if (p.CF > BAND_FRAGS) return false;  // a fragment row is a band at least
  p.tiles = (uint32_t)cdiv(M, TM);
  for (int band = BAND_FRAGS;; band = BAND_FRAGS_SMALL) {
    // bands of whole fragment rows, evened out; then slabs of tiles towards WG_BLOCKS blocks in all
    p.KB = band / p.CF < 1 ? 1 : band / p.CF;
    p.nz = cdiv(p.KF, p.KB);
    p.KB = cdiv(p.KF, p.nz);
    long long want = WG_BLOCKS / (G * p.nz);
    if (want < 1) want = 1;
    long long per = (p.tiles + want - 1) / want;
    if (per < WG_MIN_TILES) per = WG_MIN_TILES;
    p.per = (int)per;
    slabs = (int)((p.tiles + per - 1) / per);
    if (band == BAND_FRAGS_SMALL || p.CF > BAND_FRAGS_SMALL || (long long)slabs * G * p.nz >= WG_BLOCKS / 2) break;
  }
  p.dsb = 32 * p.KB + PADB;
  p.xsb = 32 * p.CF + PADB;
  if ((size_t)TM * (p.dsb + p.xsb) > (size_t)LDS_LIMIT) return false;
  p.fdc = make_fdiv((uint32_t)(4 * p.KB));
  p.fxc = make_fdiv((uint32_t)(4 * p.CF));
  return true;
}

// Dynamic LDS above the default 64 KB needs the limit raised: once per device, a failure is not kept.
template <typename K>
inline bool lds_ok(K kernel, size_t lds, bool* raised) {
  if (lds <= 64 * 1024) return true;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (dev >= 0 && dev < 64 && raised[dev]) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          LDS_LIMIT) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (dev >= 0 && dev < 64) raised[dev] = true;
  return true;
}

template <bool DGRAD>
int launch_io(const bf16_t* src, const bf16_t* w, const float* bias, const bf16_t* gate, bf16_t* dst, const Io& p,
              int relu, hipStream_t st) {
  static bool raised[64] = {};
  const size_t lds = io_lds(p);
  if (!lds_ok(conv_gpw_io_k<DGRAD>, lds, raised)) return 1;
  hipLaunchKernelGGL((conv_gpw_io_k<DGRAD>), dim3((p.items + p.per - 1) / p.per), dim3(NT), lds, st, src, w, bias,
                     gate, dst, p, relu);
  return SN_CHECK_LAUNCH();
}

template <int NA>
int launch_wgrad(const bf16_t* dy, const bf16_t* x, float* part, const Wg& p, int slabs, hipStream_t st) {
  static bool raised[64] = {};
  const size_t lds = (size_t)TM * (p.dsb + p.xsb);
  if (!lds_ok(conv_gpw_wgrad_k<NA>, lds, raised)) return 1;
  hipLaunchKernelGGL((conv_gpw_wgrad_k<NA>), dim3((unsigned)slabs, (unsigned)p.G, (unsigned)p.nz), dim3(NT), lds, st, dy, x, part,
                     p);
  return SN_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

// Floats the weight-gradient workspace needs for M rows of `groups` groups of Cg -> Kg channels; 0 for
// a geometry the kernels do not take.
long long sn_conv_gpw_part_floats(long long M, long long groups, long long Cg, long long Kg) {
  Wg p;
  int slabs;
  if (!wg_plan(M, groups, Cg, Kg, p, slabs)) return 0;
  return (long long)slabs * groups * Kg * Cg;
}

// y[M][groups Kg] = relu?(x[M][groups Cg] x w[groups Kg][Cg] per group + bias); bias may be null.
int sn_conv_gpw_fwd(const bf16_t* x, const bf16_t* w, const float* bias, bf16_t* y, long long M, long long groups,
                    long long Cg, long long Kg, long long relu, hipStream_t st) {
  Io p;
  if (!io_plan(M, groups, Cg, Kg, p)) return 3;
  if (!al(x, 8) || !al(w, 8) || !al(y, Kg % 8 == 0 ? 16 : 8) || !al(bias, 4)) return 2;
  return launch_io<false>(x, w, bias, nullptr, y, p, (int)relu, st);
}

// dx[M][groups Cg] = dy[M][groups Kg] x w per group, zeroed where gate <= 0 (gate shaped like dx; may
// be null).
int sn_conv_gpw_dgrad(const bf16_t* dy, const bf16_t* w, const bf16_t* gate, bf16_t* dx, long long M,
                      long long groups, long long Cg, long long Kg, hipStream_t st) {
  Io p;
  if (!io_plan(M, groups, Kg, Cg, p)) return 3;
  const uintptr_t a = Cg % 8 == 0 ? 16 : 8;
  if (!al(dy, 8) || !al(w, 8) || !al(dx, a) || !al(gate, a)) return 2;
  return launch_io<true>(dy, w, nullptr, gate, dx, p, 0, st);
}

// part[slab][groups Kg][Cg] (fp32) from dy and x; part_floats >= sn_conv_gpw_part_floats(...).
int sn_conv_gpw_wgrad(const bf16_t* dy, const bf16_t* x, float* part, long long part_floats, long long M,
                      long long groups, long long Cg, long long Kg, hipStream_t st) {
  Wg p;
  int slabs;
  if (!wg_plan(M, groups, Cg, Kg, p, slabs)) return 3;
  if (!al(dy, 8) || !al(x, 8) || !part || !al(part, 4)) return 2;
  if ((long long)slabs * groups * Kg * Cg > part_floats) return 3;
  if (p.KB * p.CF <= BAND_FRAGS_SMALL) return launch_wgrad<BAND_FRAGS_SMALL / 4>(dy, x, part, p, slabs, st);
  return launch_wgrad<BAND_FRAGS / 4>(dy, x, part, p, slabs, st);
}

// dw[groups Kg][Cg] (fp32) = (flag == 2: dw +) the slabs of part in slab order; flag 1 stores.
int sn_conv_gpw_wgrad_finalize(const float* part, long long part_floats, float* dw, long long flag, long long M,
                               long long groups, long long Cg, long long Kg, hipStream_t st) {
  Wg p;
  int slabs;
  if (!wg_plan(M, groups, Cg, Kg, p, slabs)) return 3;
  if (!part || !dw || (flag != GRAD_STORE && flag != GRAD_ACC)) return 2;
  const long long total = groups * Kg * Cg;
  if (slabs * total > part_floats) return 3;
  hipLaunchKernelGGL(conv_gpw_wgrad_finalize_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, slabs,
                     total, dw, (int)flag);
  return SN_CHECK_LAUNCH();
}

// y[m][j groups + i] = x[m][i (C / groups) + j] for M rows of C bf16 channels.
int sn_shuffle_channel(const bf16_t* x, bf16_t* y, long long M, long long C, long long groups, hipStream_t st) {
  if (M < 1 || C < 1 || groups < 1 || C % groups != 0 || C > 16384 || M > (1LL << 40)) return 3;
  if (!x || !y || x == y) return 2;
  const int rows = (int)(32768 / (2 * C)) > 64 ? 64 : (int)(32768 / (2 * C));  // whole rows in 32 KB
  const size_t lds = (size_t)rows * C * 2;
  const int blocks = sn_blocks((M + rows - 1) / rows, 1, 8 * sn_cu_count());
  if (C % 8 == 0 && al(x, 16) && al(y, 16))
    hipLaunchKernelGGL((shuffle_channel_k<8>), dim3(blocks), dim3(NT), lds, st, x, y, M, (int)C, (int)groups, rows,
                       make_fdiv((uint32_t)(C / 8)), make_fdiv((uint32_t)groups));
  else
    hipLaunchKernelGGL((shuffle_channel_k<1>), dim3(blocks), dim3(NT), lds, st, x, y, M, (int)C, (int)groups, rows,
                       make_fdiv((uint32_t)C), make_fdiv((uint32_t)groups));
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
