// Fused LSTM step kernels (gfx950): one launch per timestep and direction, the gate math in the epilogue.
// Upstream LSTMLayer semantics, gate order i, f, o, g along the 4H axis:
//
//   pre  = xg_t + b_c (+ xs) + W_hc (cont_t h_{t-1})        xg [N][4H] fp32: the input projection of step t
//   i, f, o = sigmoid(pre[0:3H]),  g = tanh(pre[3H:4H])      xs [N][4H] fp32: the static projection (optional)
//   c_t  = cont_t f c_{t-1} + i g                            W_hc [4H][H] bf16, h [N][H] bf16, c [N][H] fp32
//   h_t  = o tanh(c_t)                                        cont [N] fp32, one value per stream
//
// Ownership, the same in both kernels: a block of four waves owns 16 hidden units (u0 ..) with all four of
// their gates, and 16 batch rows (n0 ..); the grid is ceil(H / 16) x ceil(N / 16).  The dependency between
// timesteps is the launch order and nothing else: no atomics, no scratch, no host read, no grid barrier, so
// the launches sit in a captured graph like any other.
//
// lstm_step_fwd_k.  The four 16 x 16 pre-activation tiles come from v_mfma_f32_16x16x32_bf16 with the weight
// rows as the A operand and the rows of h_{t-1} as the B operand.  Both are contiguous along the reduction, so
// a fragment is one 16-byte global load per lane (row lane & 15, reduction elements 8 (lane >> 4) ..) and
// nothing is staged in LDS.  H % 8 == 0 makes every 8-element chunk whole: a chunk at or past H, a unit at or
// past H and a row at or past N load zeros on BOTH sides, so nothing outside the matrices reaches a sum.  The
// K-steps of 32 are dealt round-robin to the four waves (the step is latency-bound: four waves put four
// times the loads in flight); the partial tiles meet in 17 KB of LDS and are summed in wave order, a fixed
// order, so a step is reproducible bit for bit.  The sum is read back with the threads along (row, unit):
// 16 consecutive lanes hold 16 consecutive units of a row, so every store below is a 32- or 64-byte run.
// Accumulator element r of lane l is unit 4 (l >> 4) + r of row l & 15 in all four tiles, so one thread ends
// up with the four gates of its (row, unit) in registers and the rest never leaves them: cont_t scales the
// recurrent sum (cont_t is one value per row, so this is W_hc (cont_t h) with the scaling done in fp32), the
// fp32 input projection, the bias and the static projection are added, the gates are activated, the cell is
// updated.  Written: h_t as bf16 (straight into slice t of the top blob), c_t as fp32 and, when training,
// the four activated gates as bf16 and cont_t h_{t-1} as bf16 (the weight gradient's operand).
//
// lstm_step_bwd_k.  Step t first forms the recurrent gradient of ITS h_t, cont_{t+1} (dgates_{t+1} . W_hc),
// for its own (row, unit) tile on the same MFMA: the reduction runs over the 4H gate rows, so the kernel reads a
// [H][4H] transposed bf16 copy of W_hc (lstm_transpose_k, once per backward pass) and both operands are again
// contiguous 16-byte loads; 4H is a multiple of 32, so there is no K tail.  The waves split the K-steps and
// reduce through LDS as above.  The epilogue is the pointwise LSTM-unit backward of step t on the saved bf16
// gates and the fp32 cells; it writes the four pre-activation gradients as bf16 into dgates[t] and
// dc_{t-1} = dc_t cont_t f_t as fp32 in place (an entry is read and written by the one thread that owns it).
// The recurrent dh and the carried dc never pass through bf16.  At t = T - 1 there is no step t + 1: the
// product is skipped and the carried dc is taken as zero, so the buffer needs no clearing.
//
// Limits (checked in the C entries; hip.lstm_ok mirrors them): H % 8 == 0, 8 <= H, N 4H < 2^31,
// ceil(N / 16) <= 65535, the bf16 matrices 16-byte aligned.  Element offsets are 64-bit.
#include "common.h"

namespace {

constexpr int NT = 256;  // four waves
constexpr int NW = 4;
constexpr int TILE = 16;  // units and rows of a block
// floats of one accumulator element's row in LDS: 64 lanes + 4, so that the read-back below, whose 64 threads take
// element un & 3 of lane 16 (un >> 2) + row for four consecutive rows, lands on 64 different banks (4 r + 16 q + row)
constexpr int PL = 68;

SN_DEV bf16x8_t ldfrag(const bf16_t* __restrict__ p, long long e, bool ok) {
  const uint4 v = ok ? *reinterpret_cast<const uint4*>(p + e) : make_uint4(0u, 0u, 0u, 0u);
  return __builtin_bit_cast(bf16x8_t, v);
}

SN_DEV float sigm(float x) { return 1.f / (1.f + __expf(-x)); }

// where in a wave's accumulators the (row, unit) of this thread sits: lane 16 (unit / 4) + row, element unit % 4
SN_DEV int acc_lane(int row, int un) { return (un >> 2) * 16 + row; }

__global__ void __launch_bounds__(NT) lstm_step_fwd_k(const bf16_t* __restrict__ hprev, const bf16_t* __restrict__ whc,
                                                      const float* __restrict__ xg, const float* __restrict__ bias,
                                                      const float* __restrict__ xs, const float* __restrict__ cont,
                                                      const float* __restrict__ cprev, bf16_t* __restrict__ hout,
                                                      float* __restrict__ cout, bf16_t* __restrict__ gates,
                                                      bf16_t* __restrict__ hc, int N, int H) {
  __shared__ float part[NW][4][4][PL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u0 = blockIdx.x * TILE, n0 = blockIdx.y * TILE;
  const int fr = lane & 15, kq = (lane >> 4) * 8;
  const bool uok = u0 + fr < H, nok = n0 + fr < N;
  f32x4 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int ksteps = (H + 31) >> 5;
  for (int ks = wave; ks < ksteps; ks += NW) {
    const int k = ks * 32 + kq;
    const bool kok = k < H;  // H % 8 == 0: a chunk is inside or outside as a whole
    const bf16x8_t b = ldfrag(hprev, (long long)(n0 + fr) * H + k, nok && kok);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ldfrag(whc, ((long long)g * H + u0 + fr) * H + k, uok && kok), b,
                                                       acc[g], 0, 0, 0);
  }
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][g][r][lane] = acc[g][r];
  __syncthreads();
  const int row = threadIdx.x >> 4, un = threadIdx.x & 15;
  const int n = n0 + row, u = u0 + un;
  if (n >= N || u >= H) return;
  const int al = acc_lane(row, un), r = un & 3;
  const float ct = cont[n];
  const long long e = (long long)n * H + u, e4 = (long long)n * 4 * H + u;
  float a[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float rec = ((part[0][g][r][al] + part[1][g][r][al]) + part[2][g][r][al]) + part[3][g][r][al];
    float in = xg[e4 + (long long)g * H] + bias[g * H + u];
    if (xs) in += xs[e4 + (long long)g * H];
    const float pre = ct * rec + in;
    a[g] = g < 3 ? sigm(pre) : tanhf(pre);
  }
  const float c = ct * a[1] * cprev[e] + a[0] * a[3];
  hout[e] = f2bf(a[2] * tanhf(c));
  cout[e] = c;
  if (gates) {
#pragma unroll
    for (int g = 0; g < 4; ++g) gates[e4 + (long long)g * H] = f2bf(a[g]);
  }
  if (hc) hc[e] = f2bf(ct * bf2f(hprev[e]));
}

__global__ void __launch_bounds__(NT) lstm_step_bwd_k(const bf16_t* __restrict__ dgn, const bf16_t* __restrict__ whct,
                                                      const float* __restrict__ contn, const bf16_t* __restrict__ dh,
                                                      const float* __restrict__ cont, const bf16_t* __restrict__ gates,
                                                      const float* __restrict__ c, const float* __restrict__ cprev,
                                                      float* __restrict__ dc, bf16_t* __restrict__ dg, int N, int H) {
  __shared__ float part[NW][4][PL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u0 = blockIdx.x * TILE, n0 = blockIdx.y * TILE;
  const int fr = lane & 15, kq = (lane >> 4) * 8;
  const bool uok = u0 + fr < H, nok = n0 + fr < N;
  const long long K = 4ll * H;  // a multiple of 32
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  if (dgn) {  // uniform: a step t + 1 exists
    const int ksteps = (int)(K >> 5);
    for (int ks = wave; ks < ksteps; ks += NW) {
      const int k = ks * 32 + kq;
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ldfrag(whct, (long long)(u0 + fr) * K + k, uok),
                                                    ldfrag(dgn, (long long)(n0 + fr) * K + k, nok), acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][r][lane] = acc[r];
  __syncthreads();
  const int row = threadIdx.x >> 4, un = threadIdx.x & 15;
  const int n = n0 + row, u = u0 + un;
  if (n >= N || u >= H) return;
  const int al = acc_lane(row, un), r = un & 3;
  const long long e = (long long)n * H + u, e4 = (long long)n * K + u;
  float d = bf2f(dh[e]), dct = 0.f;
  if (dgn) {
    d += contn[n] * (((part[0][r][al] + part[1][r][al]) + part[2][r][al]) + part[3][r][al]);
    dct = dc[e];
  }
  const float gi = bf2f(gates[e4]), gf = bf2f(gates[e4 + H]), go = bf2f(gates[e4 + 2ll * H]), gg = bf2f(gates[e4 + 3ll * H]);
  const float ct = cont[n], tc = tanhf(c[e]);
  dct += d * go * (1.f - tc * tc);
  dg[e4] = f2bf(dct * gg * gi * (1.f - gi));
  dg[e4 + H] = f2bf(dct * ct * cprev[e] * gf * (1.f - gf));
  dg[e4 + 2ll * H] = f2bf(d * tc * go * (1.f - go));
  dg[e4 + 3ll * H] = f2bf(dct * gi * (1.f - gg * gg));
  dc[e] = dct * ct * gf;
}

// dst [C][R] = src [R][C]^T, bf16: a 32 x 32 tile through LDS, rows of both sides read and written along the lanes.
__global__ void __launch_bounds__(256) lstm_transpose_k(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst, int R, int C) {
  __shared__ bf16_t tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int j = ty; j < 32; j += 8)
    if (r0 + j < R && c0 + tx < C) tile[j][tx] = src[(long long)(r0 + j) * C + c0 + tx];
  __syncthreads();
  for (int j = ty; j < 32; j += 8)
    if (c0 + j < C && r0 + tx < R) dst[(long long)(c0 + j) * R + r0 + tx] = tile[tx][j];
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool geometry_ok(long long N, long long H) {
  return N >= 1 && H >= 8 && H % 8 == 0 && N * 4 * H < (1ll << 31) && 4 * H * H < (1ll << 40) && (N + TILE - 1) / TILE <= 65535;
}

}  // namespace

extern "C" {

// One forward step: hout [N][H], cout [N][H] and (training: non-null) gates [N][4H], hc [N][H] from hprev, cprev,
// the step's xg [N][4H] and cont [N]; xs [N][4H] may be null.
int sn_lstm_step_fwd(const bf16_t* hprev, const bf16_t* whc, const float* xg, const float* bias, const float* xs,
                     const float* cont, const float* cprev, bf16_t* hout, float* cout, bf16_t* gates, bf16_t* hc,
                     long long N, long long H, hipStream_t st) {
  if (!hprev || !whc || !xg || !bias || !cont || !cprev || !hout || !cout) return 2;
  if (!geometry_ok(N, H) || !al16(hprev) || !al16(whc)) return 3;
  if (hout == hprev || cout == cprev) return 3;  // other blocks still read the previous state
  const dim3 grid((unsigned)((H + TILE - 1) / TILE), (unsigned)((N + TILE - 1) / TILE));
  hipLaunchKernelGGL(lstm_step_fwd_k, grid, dim3(NT), 0, st, hprev, whc, xg, bias, xs, cont, cprev, hout, cout, gates, hc,
                     (int)N, (int)H);
  return SN_CHECK_LAUNCH();
}

// One backward step t: dg = dgates[t] [N][4H] and dc [N][H] (in: dc_t, out: dc_{t-1}) from the top gradient dh [N][H],
// the saved gates and cells of t and, unless t is the last step (dgn and contn null), dgates[t + 1] and cont[t + 1].
int sn_lstm_step_bwd(const bf16_t* dgn, const bf16_t* whct, const float* contn, const bf16_t* dh, const float* cont,
                     const bf16_t* gates, const float* c, const float* cprev, float* dc, bf16_t* dg, long long N,
                     long long H, hipStream_t st) {
  if (!whct || !dh || !cont || !gates || !c || !cprev || !dc || !dg || (dgn != nullptr) != (contn != nullptr)) return 2;
  if (!geometry_ok(N, H) || !al16(dgn) || !al16(whct) || dgn == dg) return 3;
  const dim3 grid((unsigned)((H + TILE - 1) / TILE), (unsigned)((N + TILE - 1) / TILE));
  hipLaunchKernelGGL(lstm_step_bwd_k, grid, dim3(NT), 0, st, dgn, whct, contn, dh, cont, gates, c, cprev, dc, dg, (int)N,
                     (int)H);
  return SN_CHECK_LAUNCH();
}

// dst [C][R] = src [R][C]^T (bf16): the [H][4H] copy of W_hc that the backward steps read.
int sn_lstm_transpose(const bf16_t* src, bf16_t* dst, long long R, long long C, hipStream_t st) {
  if (!src || !dst || src == dst) return 2;
  if (R < 1 || C < 1 || R > (1 << 20) || C > (1 << 20)) return 3;
  const dim3 grid((unsigned)((C + 31) / 32), (unsigned)((R + 31) / 32));
  if (grid.y > 65535) return 3;
  hipLaunchKernelGGL(lstm_transpose_k, grid, dim3(256), 0, st, src, dst, (int)R, (int)C);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
