// Data gradient of a dense stride-2 convolution (= a stride-2 transposed convolution), gfx950:
// ungrouped, undilated, window R x S with 1 <= R, S <= 4, any pad, NHWC bf16, fp32 accumulation.
// One launch, dx written exactly once, no scratch buffer and no gather pass.
//
// Phase decomposition.  Write h + ph = 2 i + a and w + pw = 2 j + b: (i, j) is a cell, (a, b) its
// phase.  Only taps r = a + 2 t, s = b + 2 u reach phase (a, b), and they read dy at (i - t, j - u):
//
//   dx[n, 2i+a-ph, 2j+b-pw, c] = sum_{t, u, k} dy[n, i-t, j-u, k] * w[k, a+2t, b+2u, c]
//
// so each phase is a dense stride-1 correlation of dy with a sub-sampled window, the four phases
// together do exactly 2 N P Q R S K C flops, and a phase without a tap (three of four at 1x1) is
// identically zero.  dx pixels that no dy pixel reaches come out as zeros the same way: their
// patch entries lie outside dy.
//
// Work split.  A block of four waves owns 8 x 16 cells of one image times 64 channels c, all four
// phases.  Per 32-deep chunk of K it stages in LDS
//   * the dy patch of (8 + ceil(R/2) - 1) x (16 + ceil(S/2) - 1) pixels, 64 bytes of k each, zero
//     outside dy and past K; a pixel is padded to 80 bytes, so that the 16 consecutive pixels one
//     operand read touches start on 16 different bank quads;
//   * all R S taps of w[k][r][s][c-tile] in place, k outermost: a k row is R S x 128 bytes plus 64
//     bytes of padding, which puts the four rows one 16-lane group reads transposed on four
//     different 64-byte bank groups.
// Wave v takes cell rows 2v and 2v + 1 (two 16-cell MFMA tiles) times the 64 channels (four
// 16-channel tiles) times every phase that has taps: v_mfma_f32_16x16x32_bf16 with the weights as
// the row operand and the cells as the column operand.  The cell operand of tap offset (t, u) is
// one 16-byte LDS read per lane at a constant offset into the patch and is shared by the phases;
// the weight operand needs k along the lane's 8 values while LDS has c contiguous, so it is read
// with ds_read_b64_tr_b16 (two reads of 4 k rows).  The transposed read lets each lane name its
// own 4 columns: lane p of a group names channels 8 p + 4 h .. + 3 for half h of a channel pair
// of tiles, so the accumulator rows 4 g + i of the pair are channels 8 g + 4 h + i and a lane ends
// with 8 consecutive channels of one cell: one 16-byte store per (phase, cell row, 32 channels).
// Accumulators exist only for phases with taps (R and S are template parameters); the others
// store zeros through the same epilogue.
//
// The K loop is two-stage: the next chunk's global loads are issued into registers before the
// current chunk's MFMAs and written to LDS after them.
//
// Epilogue: dx = gate > 0 ? v : 0 where a gate (laid out as dx) is given, bf16, 16 bytes per lane.
// Addressing: 64-bit image bases, 32-bit offsets inside an image (checked on the host).
#include "common.h"

namespace {

constexpr int TI = 8, TJ = 16;  // cells of a block
constexpr int CT = 64;          // channels of a block
constexpr int KC = 32;          // reduction chunk
constexpr int PIXB = 80;        // LDS bytes of a staged dy pixel: 32 k and 16 bytes of padding
constexpr int NT = 256;

struct Geo {
  int N, H, W, C, K, P, Q, ph, pw;
  int i0, j0;          // first cell row / column that holds a dx pixel
  FDiv fimg, ftj;      // cell tiles per image, per row of tiles
};

template <int R, int S>
struct Win {
  static constexpr int TR = (R + 1) / 2, TS = (S + 1) / 2;     // tap offsets per axis
  static constexpr int PR = TI + TR - 1, PS = TJ + TS - 1;     // the patch
  static constexpr int NPIX = PR * PS, TAPS = R * S;
  static constexpr int WROW = TAPS * CT * 2 + 64;              // LDS bytes of a k row of the weights
  static constexpr int PATCH_BYTES = NPIX * PIXB;
  static constexpr int LDS = PATCH_BYTES + KC * WROW;
  static constexpr int PU = (NPIX * 4 + NT - 1) / NT;          // 16-byte patch loads of a thread
};

SN_DEV bf16x8_t tr_frag(const unsigned char* a0, int second) {
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)a0);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a0 + second));
  const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, r);
}

template <int R, int S>
__global__ void __launch_bounds__(NT) conv_tstride_dgrad_k(const bf16_t* __restrict__ dy,
                                                           const bf16_t* __restrict__ w,
                                                           const bf16_t* __restrict__ gate,
                                                           bf16_t* __restrict__ dx, const Geo g) {
  using Wn = Win<R, S>;
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  unsigned char* const smw = sm + Wn::PATCH_BYTES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lg = lane >> 4, ln = lane & 15;

  // the block's cells and channels
  const uint32_t tile = blockIdx.x, img = udiv(tile, g.fimg), tin = tile - img * g.fimg.d;
  const uint32_t trow = udiv(tin, g.ftj);
  const int ib = g.i0 + (int)trow * TI, jb = g.j0 + (int)(tin - trow * g.ftj.d) * TJ;
  const int c0 = blockIdx.y * CT;
  const bf16_t* const dyn = dy + (long long)img * g.P * g.Q * g.K;
  const long long xbase = (long long)img * g.H * g.W * g.C;

  // what this thread stages per chunk: PU patch loads (pixel, 8 k) and TAPS weight loads (k, tap, 8 c)
  int p_off[Wn::PU];   // element offset inside the image at k = 0, -1: a zero
  int p_kq[Wn::PU];
#pragma unroll
  for (int x = 0; x < Wn::PU; ++x) {
    const int u = tid + x * NT, pix = u >> 2, kq = u & 3;
    const int pr = pix / Wn::PS, pc = pix - pr * Wn::PS;
    const int p = ib - (Wn::TR - 1) + pr, q = jb - (Wn::TS - 1) + pc;
    const bool ok = u < Wn::NPIX * 4 && p >= 0 && p < g.P && q >= 0 && q < g.Q;
    p_off[x] = ok ? (p * g.Q + q) * g.K + kq * 8 : -1;
    p_kq[x] = kq * 8;
  }
  const int w_cu = tid & 7;
  const bool w_cok = c0 + w_cu * 8 < g.C;

  uint4 pre_p[Wn::PU], pre_w[Wn::TAPS];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int x = 0; x < Wn::PU; ++x) {
      const bool ok = p_off[x] >= 0 && k0 + p_kq[x] < g.K;
      pre_p[x] = ok ? *reinterpret_cast<const uint4*>(dyn + p_off[x] + k0) : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int x = 0; x < Wn::TAPS; ++x) {
      const int rest = (tid >> 3) + x * (NT / 8), kk = rest / Wn::TAPS, tap = rest - kk * Wn::TAPS;
      const bool ok = w_cok && k0 + kk < g.K;
      pre_w[x] = ok ? *reinterpret_cast<const uint4*>(w + ((long long)(k0 + kk) * Wn::TAPS + tap) * g.C + c0 + w_cu * 8)
                    : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int x = 0; x < Wn::PU; ++x) {
      const int u = tid + x * NT;
      if (u < Wn::NPIX * 4) *reinterpret_cast<uint4*>(sm + (u >> 2) * PIXB + (u & 3) * 16) = pre_p[x];
    }
#pragma unroll
    for (int x = 0; x < Wn::TAPS; ++x) {
      const int rest = (tid >> 3) + x * (NT / 8), kk = rest / Wn::TAPS, tap = rest - kk * Wn::TAPS;
      *reinterpret_cast<uint4*>(smw + kk * Wn::WROW + tap * (CT * 2) + w_cu * 16) = pre_w[x];
    }
  };

  // acc[a][b][cell row][channel tile]; only the phases with taps are ever touched
  f32x4 acc[2][2][2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int rr = 0; rr < 2; ++rr)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) acc[a][b][rr][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  // operand addresses of the lane: the cell operand reads cell ln of a row, k 8 lg .. + 7; the
  // transposed weight read names k row 8 lg + (ln >> 2) (then + 4), channels 8 (ln & 3) + 4 half
  const unsigned char* const pa = sm + ((2 * wave + Wn::TR - 1) * Wn::PS + ln + Wn::TS - 1) * PIXB + lg * 16;
  const unsigned char* const wa = smw + (8 * lg + (ln >> 2)) * Wn::WROW + (ln & 3) * 16;

  fetch(0);
  for (int k0 = 0; k0 < g.K; k0 += KC) {
    __syncthreads();  // the previous chunk's operand reads are done
    commit();
    __syncthreads();
    if (k0 + KC < g.K) fetch(k0 + KC);  // in flight while the MFMAs below run
#pragma unroll
    for (int t = 0; t < Wn::TR; ++t)
#pragma unroll
      for (int u = 0; u < Wn::TS; ++u) {
        bf16x8_t cell[2];
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
          cell[rr] = __builtin_bit_cast(
              bf16x8_t, *reinterpret_cast<const uint4*>(pa + ((rr - t) * Wn::PS - u) * PIXB));
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            if (a + 2 * t >= R || b + 2 * u >= S) continue;
            const int tap = (a + 2 * t) * S + b + 2 * u;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
              const bf16x8_t wf = tr_frag(wa + tap * (CT * 2) + (ct >> 1) * 64 + (ct & 1) * 8, 4 * Wn::WROW);
#pragma unroll
              for (int rr = 0; rr < 2; ++rr)
                acc[a][b][rr][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, cell[rr], acc[a][b][rr][ct], 0, 0, 0);
            }
          }
      }
  }

  // the lane's cell (2 wave + rr, ln) and channels c0 + 32 cp + 8 lg .. + 7
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const bool taps = a < R && b < S;
      const int wx = 2 * (jb + ln) + b - g.pw;
#pragma unroll
      for (int rr = 0; rr < 2; ++rr) {
        const int h = 2 * (ib + 2 * wave + rr) + a - g.ph;
        if (h < 0 || h >= g.H || wx < 0 || wx >= g.W) continue;
#pragma unroll
        for (int cp = 0; cp < 2; ++cp) {
          const int c = c0 + cp * 32 + lg * 8;
          if (c >= g.C) continue;
          const long long e = xbase + (h * g.W + wx) * g.C + c;
          uint4 out = make_uint4(0u, 0u, 0u, 0u);
          if (taps) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              v[i] = acc[a][b][rr][2 * cp][i];
              v[4 + i] = acc[a][b][rr][2 * cp + 1][i];
            }
            if (gate) {
              float gf[8];
              unpack8(*reinterpret_cast<const uint4*>(gate + e), gf);
#pragma unroll
              for (int i = 0; i < 8; ++i) v[i] = gf[i] > 0.f ? v[i] : 0.f;
            }
            out = pack8(v);
          }
          *reinterpret_cast<uint4*>(dx + e) = out;
        }
      }
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int R, int S>
int launch(const bf16_t* dy, const bf16_t* w, const bf16_t* gate, bf16_t* dx, const Geo& g, dim3 grid, hipStream_t st) {
  constexpr int lds = Win<R, S>::LDS;
  if (lds > 64 * 1024) {  // above the default limit of dynamic LDS: raised once per device, a failure is not kept
    static bool raised[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1;
    if (dev < 0 || dev >= 64 || !raised[dev]) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(conv_tstride_dgrad_k<R, S>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return 1;
      if (dev >= 0 && dev < 64) raised[dev] = true;
    }
  }
  hipLaunchKernelGGL((conv_tstride_dgrad_k<R, S>), grid, dim3(NT), lds, st, dy, w, gate, dx, g);
  return SN_CHECK_LAUNCH();
}

}  // namespace

extern "C" {

// dx[N][H][W][C] = the data gradient of the stride-2 convolution x[N][H][W][C] -> y[N][P][Q][K] with
// w[K][R][S][C] and pads (ph, pw), from dy[N][P][Q][K]; zeroed where gate <= 0 (gate shaped like dx;
// may be null).  P = (H + 2 ph - R) / 2 + 1, Q likewise.  Returns 3 for a geometry outside the
// kernel's (1 <= R, S <= 4, K % 8 == 0, C % 8 == 0, an image below 2^31 elements), 2 for a
// misaligned pointer.
int sn_conv_tstride_dgrad(const bf16_t* dy, const bf16_t* w, const bf16_t* gate, bf16_t* dx, long long N,
                          long long H, long long W, long long C, long long K, long long R, long long S,
                          long long ph, long long pw, hipStream_t st) {
  const long long lim = 1LL << 31;
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || K < 8 || K % 8 || R < 1 || R > 4 || S < 1 || S > 4) return 3;
  if (ph < 0 || pw < 0 || ph > (1 << 20) || pw > (1 << 20) || H + 2 * ph < R || W + 2 * pw < S) return 3;
  const long long P = (H + 2 * ph - R) / 2 + 1, Q = (W + 2 * pw - S) / 2 + 1;
  if (H * W * C >= lim || (P + 4) * (Q + 4) * K >= lim || K * R * S * C >= (1LL << 40)) return 3;
  if (!al16(dy) || !al16(w) || !al16(gate) || !al16(dx)) return 2;
  Geo g;
  g.N = (int)N; g.H = (int)H; g.W = (int)W; g.C = (int)C; g.K = (int)K; g.P = (int)P; g.Q = (int)Q;
  g.ph = (int)ph; g.pw = (int)pw;
  g.i0 = (int)(ph >> 1); g.j0 = (int)(pw >> 1);
  const long long ci = ((H - 1 + ph) >> 1) - g.i0 + 1, cj = ((W - 1 + pw) >> 1) - g.j0 + 1;
  const long long ti = (ci + TI - 1) / TI, tj = (cj + TJ - 1) / TJ;
  if (N * ti * tj >= lim || (C + CT - 1) / CT > 65535) return 3;
  g.fimg = make_fdiv((uint32_t)(ti * tj));
  g.ftj = make_fdiv((uint32_t)tj);
  const dim3 grid((unsigned)(N * ti * tj), (unsigned)((C + CT - 1) / CT));
#define SN_TSTRIDE_CASE(r, s) \
  case (r) * 4 + (s): return launch<r, s>(dy, w, gate, dx, g, grid, st);
  switch ((int)R * 4 + (int)S) {
    SN_TSTRIDE_CASE(1, 1) SN_TSTRIDE_CASE(1, 2) SN_TSTRIDE_CASE(1, 3) SN_TSTRIDE_CASE(1, 4)
    SN_TSTRIDE_CASE(2, 1) SN_TSTRIDE_CASE(2, 2) SN_TSTRIDE_CASE(2, 3) SN_TSTRIDE_CASE(2, 4)
    SN_TSTRIDE_CASE(3, 1) SN_TSTRIDE_CASE(3, 2) SN_TSTRIDE_CASE(3, 3) SN_TSTRIDE_CASE(3, 4)
    SN_TSTRIDE_CASE(4, 1) SN_TSTRIDE_CASE(4, 2) SN_TSTRIDE_CASE(4, 3) SN_TSTRIDE_CASE(4, 4)
  }
#undef SN_TSTRIDE_CASE
  return 3;
}

}  // extern "C"
