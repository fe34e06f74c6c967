// Patch-resident data gradient of a 5x5, stride-1, pad-2 grouped convolution with 128 output
// and 48 input channels per group (CaffeNet conv2), NHWC bf16 (gfx950).
//
// Per group the product is dx[M][48] = im2col(dy)[M][25 * 128] . wt[25 * 128][48] with
// M = N H W pixels.  The GEMM engine streams the im2col operand from L2 into LDS once per tap:
// 25 fetches of every dy byte with only 48 output columns of reuse each, and that L2 -> LDS
// stream, not the MFMA pipe, sets its speed.  Here the work is cut into items, one (image,
// group, band of whole dx rows) each.  An item's dy patch is staged in LDS once (band rows + 4
// halo rows, W + 4 columns, zeros outside the image, whole 256-B pixel lines in 16-byte loads)
// and the A fragments of all 25 taps are read out of that patch: a lane computes its pixel's
// patch offset once per M fragment, a tap adds one constant.  Only the weights stream, from the
// flip-transposed copy [G][48][5][5][128] the step already builds for the GEMM (one tap = 48
// rows of 256 contiguous bytes; reading the weights in place would be 2-byte gathers), through
// a ring of three taps in LDS, written one tap ahead of its first read.
//
// A block is eight waves and persistent (one per CU, walking the items in steps of the grid):
// four MFMA waves, one per SIMD, and four loader waves.  The patch takes nearly all of the LDS,
// so the next item's patch cannot be staged beside it; the loader waves fetch it into registers
// instead (27 x 16 bytes a thread) while the MFMA waves work, and write it to LDS when those have
// left the current one.  The MFMA waves cannot do that fetch themselves: a wave that also streams
// weights cannot keep a long fetch in flight, because the wait for a weight load (the load
// counter retires in order) drains everything issued before it, and fetching between two items
// measured 13 % slower (docs/PERF_NOTES.md), presumably because every CU then waits for memory
// in the same phase and leaves it idle in the next.
//
// LDS images.  A pixel's (or weight row's) 256 bytes are sixteen 16-byte chunks; chunk kc is
// what lanes 16 q .. 16 q + 15 read in k-step s = kc / 4, q = kc % 4.  A ds_read_b128 is served
// in four groups of 16 lanes, each made of 8 lanes of an even q and 8 lanes of the q + 1 above
// it, so the even and the odd chunks go to two half images a whole number of 256-B bank rows
// apart, and inside a half a pixel takes 8 chunks + 16 bytes of padding = 144 bytes = 9 bank
// quads: 16 consecutive pixels then fall on 16 different quads, whichever q they read (a band
// row's end inside the 16 pixels costs a few two-way conflicts).
//
// LDS budget (27 x 27, the CaffeNet shape): bands of 9 rows -> patch 13 x 31 pixels x 288 B =
// 116,224 B (two halves of 58,112), ring 3 x 13,824 = 41,472 B, together 157,696 B <= 160 KiB:
// one block per CU.  Two blocks per CU would need bands of 3 rows, whose halo more than doubles
// the staged bytes.
//
// LDS reads per MFMA.  A wave's tile is 64 pixels x 48 channels: per 32-deep k-step 4 A and 3 B
// fragment reads (ds_read_b128) feed 12 v_mfma_f32_16x16x32_bf16, 7 reads per 12 MFMAs.  Four
// SIMDs issue 4 MFMAs per 16 cycles while the LDS serves 4 such reads in that time, so the read
// rate is 58 % of what the LDS can give and the MFMA pipe stays the limit.  A 32 x 48 tile
// (eight MFMA waves) would be 5 reads per 6 MFMAs, at the LDS limit.  With one MFMA wave per SIMD
// nothing else hides the read latency, so the k-loop is software-pipelined: the fragments of step s + 1
// (at a tap's last step: of the next tap's first) are read while the MFMAs of step s run.
//
// Summation order: one fp32 accumulator per output, taps in the flipped weights' order, the
// channels of a tap ascending in 32-deep steps, the k of a step on the lanes as in the GEMM
// engine (lane l holds k = 8 (l >> 4) + j), weights as the MFMA's first operand: the GEMM
// path's own order, so the result is bitwise the GEMM's.  Epilogue as the GEMM's: optional
// ReLU-backward gate (dx = gate > 0 ? dx * gate_scale : 0), bf16 store of 4 channels per lane.
#include "common.h"
#include "conv_patch_plan.h"

namespace {

using namespace sn_patch;

struct Args {
  Plan p;
  FDiv fw, fpw;  // division by W (a block pixel -> row, column) and by the patch width
  uint32_t items;
  float gate_scale;
};


SN_DEV bf16x8_t lds_frag(const unsigned char* a) {
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4*>(a));
}

struct Item {
  int n, g, h0, rows;  // image, group, first dx row of the band, its rows
};

SN_DEV Item item_of(const Plan& p, uint32_t it) {
  const uint32_t b1 = it / (uint32_t)p.G, n = b1 / (uint32_t)p.nb;
  Item r;
  r.g = (int)(it - b1 * p.G);
  r.n = (int)n;
  r.h0 = (int)(b1 - n * p.nb) * p.bh;
  r.rows = min(p.bh, p.H - r.h0);
  return r;
}

// What a thread stages for an item, into registers: chunk kc = tid & 15 of the patch pixels
// (tid >> 4) + 16 u (pixel i = row i / pw, column i % pw of the patch, whose origin is dy row
// h0 - 2, column -2; every load is made from a clamped address, and bit u of the mask returned
// says whether pixel u lies inside the image: the store to LDS writes zeros where it does not, so
// that nothing here waits for a load) and of rows (tid >> 4) + 16 j of the weights of taps 0 and 1.
SN_DEV uint32_t fetch(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ wt, const Args& a, const Item& it,
                      int tid, u32x4* pv, u32x4* w0, u32x4* w1) {
  const Plan& p = a.p;
  const int kc = tid & 15, npix = (it.rows + HALO) * p.pw;
  const bf16_t* src = dy + (long long)it.n * p.H * p.W * p.ldd + (long long)it.g * KG;  // uniform; 32-bit offsets inside an image
  uint32_t inside = 0;
  int pr = (int)udiv((uint32_t)(tid >> 4), a.fpw), pc = (tid >> 4) - pr * p.pw;
#pragma unroll
  for (int u = 0; u < PPT; ++u) {
    const int r = it.h0 - 2 + pr, c = pc - 2;
    const bool ok = ((tid >> 4) + 16 * u < npix) & (r >= 0) & (r < p.H) & (c >= 0) & (c < p.W);
    const int rc = min(max(r, 0), p.H - 1), cc = min(max(c, 0), p.W - 1);
    pv[u] = *reinterpret_cast<const u32x4*>(src + (uint32_t)((rc * p.W + cc) * (int)p.ldd + kc * 8));
    inside |= (uint32_t)ok << u;
    pc += 16;  // 16 pixels on: at most two patch rows down, the patch being at least 12 wide
    if (pc >= p.pw) { pc -= p.pw; ++pr; }
    if (pc >= p.pw) { pc -= p.pw; ++pr; }
  }
  const bf16_t* wsrc = wt + (long long)it.g * CG * (TAPS * KG);
  const uint32_t woff = (uint32_t)((tid >> 4) * (TAPS * KG) + kc * 8);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    w0[j] = *reinterpret_cast<const u32x4*>(wsrc + woff + j * 16 * (TAPS * KG));
    w1[j] = *reinterpret_cast<const u32x4*>(wsrc + woff + j * 16 * (TAPS * KG) + KG);
  }
  return inside;
}

__global__ void __launch_bounds__(128 * NWAVE) conv_patch_dgrad_k(const bf16_t* __restrict__ dy,
                                                                  const bf16_t* __restrict__ wt,
                                                                  const bf16_t* __restrict__ gate,
                                                                  bf16_t* __restrict__ dx, const Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];  // the weight ring, then the patch
  unsigned char* const patch = sm + RING * WSLOT;
  const Plan& p = a.p;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tid = threadIdx.x & (64 * NWAVE - 1);  // the thread among the 256 of its role
  const int q = lane >> 4, kc = tid & 15;
  unsigned char* const wdst = sm + (kc & 1) * WHALF + (tid >> 4) * HPIX + (kc >> 1) * 16;
  uint32_t item = blockIdx.x;  // the grid is at most the items
  Item cur = item_of(p, item);

  if (wave >= NWAVE) {
    // The loader waves: the item's patch and first two taps go from registers to LDS once the
    // MFMA waves have left the previous item's (the tap loop's last barrier), then the next
    // item's loads are issued and stay in flight while the MFMA waves work; these waves only
    // keep the barrier count until then.  Their load counter sees no other load, so nothing
    // waits for the fetch before its data is needed.
    unsigned char* const pdst = patch + (kc & 1) * p.half + (tid >> 4) * HPIX + (kc >> 1) * 16;
    u32x4 pv[PPT], w0[3], w1[3];
    uint32_t inside = fetch(dy, wt, a, cur, tid, pv, w0, w1);
    for (;;) {
      const int npix = (cur.rows + HALO) * p.pw;
#pragma unroll
      for (int u = 0; u < PPT; ++u)
        if ((tid >> 4) + 16 * u < npix)
          *reinterpret_cast<u32x4*>(pdst + u * 16 * HPIX) = (inside >> u) & 1 ? pv[u] : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        *reinterpret_cast<u32x4*>(wdst + j * 16 * HPIX) = w0[j];
        *reinterpret_cast<u32x4*>(wdst + WSLOT + j * 16 * HPIX) = w1[j];
      }
      const uint32_t next = item + gridDim.x;
      const bool has_next = next < a.items;
      if (has_next) cur = item_of(p, next);
      __syncthreads();  // the patch and taps 0 and 1 are in LDS
      if (has_next) inside = fetch(dy, wt, a, cur, tid, pv, w0, w1);
      for (int t = 0; t < TAPS; ++t) __syncthreads();
      if (!has_next) return;
      item = next;
    }
  }

  // The MFMA waves.
  const unsigned char* const bbase = sm + (q & 1) * WHALF + (lane & 15) * HPIX + (q >> 1) * 16;
  u32x4 wv[3];
  for (;;) {
    // the lane's pixel of each of the wave's four M fragments: its patch offset (a pixel past the
    // band reads pixel 0 and stores nothing) and its dx pixel
    const unsigned char* abase[4];
    int opix[4];
    const int mlim = cur.rows * p.W;
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int m = wave * MWAVE + f * 16 + (lane & 15);
      const int mm = m < mlim ? m : 0;
      const int lr = (int)udiv((uint32_t)mm, a.fw), w = mm - lr * p.W;
      abase[f] = patch + (q & 1) * p.half + (lr * p.pw + w) * HPIX + (q >> 1) * 16;
      opix[f] = m < mlim ? (cur.h0 + lr) * p.W + w : -1;
    }
    const bf16_t* wsrc = wt + ((long long)cur.g * CG + (tid >> 4)) * (TAPS * KG) + kc * 8;

    f32x4 acc[4][3];
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
      for (int i = 0; i < 3; ++i) acc[f][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    __syncthreads();  // the patch and taps 0 and 1 are in LDS

    bf16x8_t fa[4], fb[3];
#pragma unroll
    for (int f = 0; f < 4; ++f) fa[f] = lds_frag(abase[f]);
#pragma unroll
    for (int i = 0; i < 3; ++i) fb[i] = lds_frag(bbase + i * 16 * HPIX);

    // tap t = (tr, ts): patch offset toff, ring slot `slot`; (nr, ns), noff, nslot: tap t + 1
    int tr = 0, ts = 0, toff = 0, slot = 0;
    for (int t = 0; t < TAPS; ++t) {
      const bool more = t + 2 < TAPS;
      if (more) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
          wv[j] = *reinterpret_cast<const u32x4*>(wsrc + (long long)j * 16 * (TAPS * KG) + (t + 2) * KG);
      }
      int nr = tr, ns = ts + 1;
      if (ns == RS) {
        ns = 0;
        ++nr;
      }
      if (nr == RS) {  // past the last tap: read the last tap again, the fragments are not used
        nr = tr;
        ns = ts;
      }
      const int noff = (nr * p.pw + ns) * HPIX;
      const int nslot = slot + 1 == RING ? 0 : slot + 1;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        bf16x8_t na[4], nb[3];
        const int ao = s < 3 ? toff + 32 * (s + 1) : noff;
        const int bo = s < 3 ? slot * WSLOT + 32 * (s + 1) : nslot * WSLOT;
#pragma unroll
        for (int f = 0; f < 4; ++f) na[f] = lds_frag(abase[f] + ao);
#pragma unroll
        for (int i = 0; i < 3; ++i) nb[i] = lds_frag(bbase + bo + i * 16 * HPIX);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int f = 0; f < 4; ++f)
            acc[f][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[i], fa[f], acc[f][i], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int f = 0; f < 4; ++f) fa[f] = na[f];
#pragma unroll
        for (int i = 0; i < 3; ++i) fb[i] = nb[i];
      }
      // tap t + 2 goes where tap t - 1 was: every wave has left that slot at the last barrier
      if (more) {
        const int wslot = nslot + 1 == RING ? 0 : nslot + 1;
#pragma unroll
        for (int j = 0; j < 3; ++j) *reinterpret_cast<u32x4*>(wdst + wslot * WSLOT + j * 16 * HPIX) = wv[j];
      }
      __syncthreads();
      tr = nr;
      ts = ns;
      toff = noff;
      slot = nslot;
    }

    // acc[f][i][r]: pixel f, dx channel 16 i + 4 q + r of the group
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      if (opix[f] < 0) continue;
      const long long e0 = ((long long)cur.n * p.H * p.W + opix[f]) * p.ldo + (long long)cur.g * CG + 4 * q;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const long long e = e0 + 16 * i;
        float o[4] = {acc[f][i][0], acc[f][i][1], acc[f][i][2], acc[f][i][3]};
        if (gate) {
          const uint2 u = *reinterpret_cast<const uint2*>(gate + e);
          const float gv[4] = {__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                               __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u)};
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = gv[r] > 0.f ? o[r] * a.gate_scale : 0.f;
        }
        *reinterpret_cast<uint2*>(dx + e) = make_uint2(pack2(o[0], o[1]), pack2(o[2], o[3]));
      }
    }
    item += gridDim.x;
    if (item >= a.items) return;
    cur = item_of(p, item);
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

// Bands per image and rows per band the kernel would use (0, 0 for a geometry it does not take).
int sn_conv_patch_plan(long long N, long long H, long long W, long long G, long long ldd, long long ldo,
                       long long* bands, long long* band_rows, long long* lds_bytes) {
  Plan p;
  const bool ok = make_plan(N, H, W, G, ldd, ldo, p);
  if (bands) *bands = ok ? p.nb : 0;
  if (band_rows) *band_rows = ok ? p.bh : 0;
  if (lds_bytes) *lds_bytes = ok ? (long long)p.lds : 0;
  return ok ? 0 : 3;
}

// dx[N][H][W][ldo] (channels 48 g .. of group g) = the data gradient of dy[N][H][W][ldd] (channels
// 128 g ..) for the 5x5 / stride 1 / pad 2 convolution whose flip-transposed weights are
// wt[G][48][5][5][128]; dx = gate > 0 ? dx * gate_scale : 0 where gate (laid out like dx) is given.
// max_blocks: the grid is min(items, max_blocks), or min(items, CUs) where it is 0; a block walks
// its items (image, group, band) in steps of the grid.
int sn_conv_patch_dgrad(const bf16_t* dy, const bf16_t* wt, const bf16_t* gate, bf16_t* dx, long long N, long long H,
                        long long W, long long G, long long ldd, long long ldo, float gate_scale, long long max_blocks,
                        hipStream_t st) {
  Args a;
  if (!make_plan(N, H, W, G, ldd, ldo, a.p)) return 3;
  if (!dy || !wt || !dx || !al16(dy) || !al16(wt) || !al16(gate) || !al16(dx)) return 2;
  a.fw = make_fdiv((uint32_t)a.p.W);
  a.fpw = make_fdiv((uint32_t)a.p.pw);
  a.gate_scale = gate_scale;
  a.items = a.p.items;
  if (max_blocks < 0) return 3;
  const long long cap = max_blocks ? max_blocks : sn_cu_count();
  const unsigned grid = (unsigned)(a.items < cap ? a.items : cap);
  hipLaunchKernelGGL(conv_patch_dgrad_k, dim3(grid), dim3(128 * NWAVE), a.p.lds, st, dy, wt, gate, dx, a);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
