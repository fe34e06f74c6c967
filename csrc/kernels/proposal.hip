// Proposal kernels of Faster R-CNN's region-proposal network (gfx950): decode, top-k select, bitmask NMS and
// the greedy scan, on the NHWC storage.  Four launches per forward, no host read, no float atomics, no scratch:
// deterministic bit for bit and capturable.
//
//   scores [N][H][W][2A] bf16 (foreground: channels A .. 2A-1)     im_info [N][3] fp32 (height, width, scale)
//   deltas [N][H][W][4A] bf16 (anchor a: 4a .. 4a+3 = dx dy dw dh)  anchors [A][4] fp32, the base anchors
//   boxes  [N][B][4] fp32, B = A H W, box i = (h W + w) A + a       keys [N][B] uint32
//   sorted boxes [N][K][4] fp32 / scores [N][K] fp32, K = pre_nms_topn (0: B); cnt [N] int32 = M_n <= K
//   mask   [N][64 nbk][nbk] uint64, nbk = ceil(K / 64): bit c of word (row, cb) = row suppresses box 64 cb + c
//   rois   [N post][5] fp32 (image, x1, y1, x2, y2), scores [N post] fp32, count [N] int32
//
// The file is built with -ffp-contract=off and without packed fp32: a box is DEFINED by the fp32 order of
// operations of the public bbox_transform_inv / clip_boxes / _filter_boxes / nms, so no product may fuse into a
// following sum.  All offsets are 64-bit; box indices stay below 2^16.
//
// proposal_decode_k.  Lanes along (pixel, anchor) of an image, so a pixel's A scores and 4A deltas are read where
// they are contiguous (one 8-byte load of an anchor's four deltas when the pointer allows); the base anchors sit
// in LDS.  A box is one 16-byte store; its key holds a monotone 16-bit code of the bf16 score (never zero for a
// kept box, -0 counted as +0) above 0xFFFF - i, and is 0 for a dropped box: a NaN score, a non-finite decoded
// coordinate, a clipped extent below min_size * scale, or an im_info row that is NaN or not positive.  Keys of
// kept boxes are unique and their descending order is the ranking rule: score first, then the lower index.
//
// proposal_select_k.  One block of 1024 lanes per image.  A radix select (11 + 11 + 10 bits; a 2048-bin LDS
// histogram with integer adds, then a suffix scan from the top bin down: wave shuffles and one pass over the 16
// wave totals) finds the key of rank K, or 1 when fewer boxes were kept.  The keys at or above it are compacted
// into LDS (wave ballot + prefix on a per-wave base taken by one integer LDS add; their order is arbitrary and
// the sort fixes it), padded with zeros to a power of two and sorted descending by a bitonic network in LDS.
// Each key's box is then gathered with one 16-byte load and written with its score in rank order.
//
// proposal_mask_k.  One wave per (row block, column block) of 64 x 64 boxes on or above the diagonal; the column
// block's boxes are staged in LDS, a lane owns a row and forms its 64-bit word.  Blocks beyond M_n return at
// once; inside the last block, rows and columns beyond M_n give zero bits.
//
// proposal_scan_k.  One wave per image: the greedy pass.  The removed set (256 words at the most) lives in LDS.
// Per row block, lane r loads its row's diagonal word and the block's words right of the diagonal are brought
// into LDS with the lanes along the words: none of these loads depends on a decision.  The 64 decisions of the
// block are uniform: bit r of the removed word is tested and, when row r is kept, lane r's diagonal word is ORed
// in by a cross-lane read.  The kept rows' staged words are then ORed into the removed set, lanes along the
// words, and the kept rows are written at the running count through a prefix over the kept bits.  The wave
// stops at post_nms_topn and writes the padding rows (-1, 0, 0, 0, 0) / 0.
#include <float.h>

#include "common.h"

namespace {

constexpr int MAX_A = 1024;     // base anchors in LDS
constexpr int MAX_BOXES = 65535;  // boxes of an image: the index is a key's low half
constexpr int MAX_PRE = 16384;  // keys sorted in LDS: 64 KB
constexpr int SEL_NT = 1024;
constexpr int BINS = 2048;

typedef unsigned long long u64;

struct DGeo {
  int N, H, W, A, B, stride;  // B: boxes of an image
  float min_size;
  FDiv fa, fw;
};

SN_DEV bool finite(float v) { return fabsf(v) <= FLT_MAX; }  // false for NaN

// center form of an anchor's axis, then the public decode: lo' = pc - 0.5 pe, hi' = pc + 0.5 pe
SN_DEV void decode_axis(float lo, float hi, float d, float dl, float& plo, float& phi) {
  const float e = hi - lo + 1.f;
  const float c = lo + 0.5f * e;
  const float pc = d * e + c;
  const float pe = expf(dl) * e;
  plo = pc - 0.5f * pe;
  phi = pc + 0.5f * pe;
}

SN_DEV float clip(float v, float hi) { return fmaxf(fminf(v, hi), 0.f); }

template <bool V8>
__global__ void __launch_bounds__(256) proposal_decode_k(const bf16_t* __restrict__ scores,
                                                         const bf16_t* __restrict__ deltas,
                                                         const float* __restrict__ im_info,
                                                         const float* __restrict__ anchors, float4* __restrict__ boxes,
                                                         uint32_t* __restrict__ keys, const DGeo g) {
  __shared__ float s_anc[MAX_A * 4];
  for (int t = threadIdx.x; t < g.A * 4; t += 256) s_anc[t] = anchors[t];
  __syncthreads();
  const int n = blockIdx.y, i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= g.B) return;
  const int pix = (int)udiv((uint32_t)i, g.fa), a = i - pix * g.A;
  const int h = (int)udiv((uint32_t)pix, g.fw), w = pix - h * g.W;
  const long long p = (long long)n * g.H * g.W + pix;
  uint32_t sb = scores[p * (2 * g.A) + g.A + a];
  float d[4];
  const long long doff = p * (4 * g.A) + 4 * a;
  if constexpr (V8) {
    const uint2 v = *reinterpret_cast<const uint2*>(deltas + doff);
    d[0] = __uint_as_float(v.x << 16); d[1] = __uint_as_float(v.x & 0xffff0000u);
    d[2] = __uint_as_float(v.y << 16); d[3] = __uint_as_float(v.y & 0xffff0000u);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k] = bf2f(deltas[doff + k]);
  }
  const float ih = im_info[n * 3], iw = im_info[n * 3 + 1], is = im_info[n * 3 + 2];
  bool keep = ih > 0.f && iw > 0.f && is > 0.f && finite(ih) && finite(iw) && finite(is);
  const float sx = (float)(w * g.stride), sy = (float)(h * g.stride);
  float x1, y1, x2, y2;
  decode_axis(s_anc[4 * a] + sx, s_anc[4 * a + 2] + sx, d[0], d[2], x1, x2);
  decode_axis(s_anc[4 * a + 1] + sy, s_anc[4 * a + 3] + sy, d[1], d[3], y1, y2);
  keep = keep && finite(x1) && finite(y1) && finite(x2) && finite(y2);
  float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
  if (keep) {
    box = make_float4(clip(x1, iw - 1.f), clip(y1, ih - 1.f), clip(x2, iw - 1.f), clip(y2, ih - 1.f));
    const float lim = g.min_size * is;
    keep = box.z - box.x + 1.f >= lim && box.w - box.y + 1.f >= lim;
  }
  if (sb == 0x8000u) sb = 0;                      // -0 ranks as +0
  keep = keep && (sb & 0x7fffu) <= 0x7f80u;       // not NaN
  const uint32_t code = (sb & 0x8000u) ? (~sb & 0xffffu) : (sb | 0x8000u);  // >= 0x7f for every non-NaN
  const long long o = (long long)n * g.B + i;
  boxes[o] = box;
  keys[o] = keep ? (code << 16) | (uint32_t)(0xffff - i) : 0u;
}

// ---------------------------------------------------------------------------------------
// select
// ---------------------------------------------------------------------------------------
struct SGeo {
  int N, B, K, P2;  // K: keys to take at the most (1 .. MAX_PRE), P2: the power of two at or above K
};

// Sum of v over the lanes at and above this one in the block of 1024; swave: 16 ints.  Two barriers.
SN_DEV int suffix_sum(int v, int* swave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_down(v, o, 64);
    if (lane + o < 64) v += u;
  }
  __syncthreads();  // the previous call's readers
  if (lane == 0) swave[wave] = v;
  __syncthreads();
  for (int q = wave + 1; q < SEL_NT / 64; ++q) v += swave[q];
  return v;
}

__global__ void __launch_bounds__(SEL_NT) proposal_select_k(const uint32_t* __restrict__ keys,
                                                            const float4* __restrict__ boxes,
                                                            float4* __restrict__ sboxes, float* __restrict__ sscores,
                                                            int* __restrict__ cnt, const SGeo g) {
  extern __shared__ uint32_t s_keys[];  // P2 keys
  __shared__ int s_hist[BINS], s_wave[SEL_NT / 64], s_total, s_bin, s_want, s_fill;
  const int n = blockIdx.x, tid = threadIdx.x;
  const uint32_t* kn = keys + (long long)n * g.B;
  // The key of rank `want` among the non-zero keys: pass by pass, `prefix` fixes its leading bits.
  uint32_t prefix = 0;
  int want = g.K, M = g.K;  // keys are unique: exactly K lie at or above the key of rank K
  bool all = false;         // fewer than K boxes were kept: take every non-zero key
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
    const uint32_t dmask = pass == 2 ? 1023u : 2047u;
    for (int b = tid; b < BINS; b += SEL_NT) s_hist[b] = 0;
    __syncthreads();
    for (int i = tid; i < g.B; i += SEL_NT) {
      const uint32_t k = kn[i];
      const bool cand = pass == 0 ? k != 0 : (k >> (pass == 1 ? 21 : 10)) == prefix;  // prefix is never 0
      if (cand) atomicAdd(&s_hist[(k >> shift) & dmask], 1);
    }
    __syncthreads();
    const int hi = s_hist[2 * tid + 1], lo = s_hist[2 * tid];
    const int incl = suffix_sum(hi + lo, s_wave);
    const int above = incl - hi - lo;  // candidates in the bins above this lane's two
    if (tid == 0) s_total = incl;
    if (above < want && want <= above + hi) {
      s_bin = 2 * tid + 1;
      s_want = want - above;
    } else if (above + hi < want && want <= above + hi + lo) {
      s_bin = 2 * tid;
      s_want = want - above - hi;
    }
    __syncthreads();
    if (s_total < want) {  // the first pass only: later passes count a bin that holds the rank
      all = true;
      M = s_total;
      break;
    }
    prefix = (prefix << (pass == 2 ? 10 : 11)) | (uint32_t)s_bin;
    want = s_want;
  }
  const uint32_t cut = all ? 1u : prefix;
  if (tid == 0) s_fill = 0;
  __syncthreads();
  const int lane = tid & 63;
  for (int i0 = 0; i0 < g.B; i0 += SEL_NT) {
    const int i = i0 + tid;
    const uint32_t k = i < g.B ? kn[i] : 0u;
    const bool take = k != 0 && k >= cut;
    const u64 ball = __ballot(take);
    int base = 0;
    if (lane == 0 && ball) base = atomicAdd(&s_fill, __popcll(ball));
    base = __shfl(base, 0, 64);
    if (take) {
      const int slot = base + __popcll(ball & ((1ull << lane) - 1ull));
      if (slot < g.P2) s_keys[slot] = k;  // always true: M <= K <= P2
    }
  }
  int p2 = 2;
  while (p2 < M) p2 <<= 1;
  __syncthreads();
  for (int i = M + tid; i < p2; i += SEL_NT) s_keys[i] = 0;
  __syncthreads();
  for (int k = 2; k <= p2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < (p2 >> 1); t += SEL_NT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint32_t a = s_keys[i], b = s_keys[l];
        if (((i & k) == 0) ? a < b : a > b) {
          s_keys[i] = b;
          s_keys[l] = a;
        }
      }
      __syncthreads();
    }
  }
  for (int j = tid; j < M; j += SEL_NT) {
    const uint32_t k = s_keys[j], code = k >> 16;
    const int i = min(0xffff - (int)(k & 0xffffu), g.B - 1);  // a key written by proposal_decode_k is inside
    const uint32_t sb = (code & 0x8000u) ? (code & 0x7fffu) : (~code & 0xffffu);
    const long long o = (long long)n * g.K + j;
    sboxes[o] = boxes[(long long)n * g.B + i];
    sscores[o] = __uint_as_float(sb << 16);
  }
  if (tid == 0) cnt[n] = M;
}

// ---------------------------------------------------------------------------------------
// mask and scan
// ---------------------------------------------------------------------------------------
struct NGeo {
  int N, K, nbk, post;  // nbk: 64-box blocks of K
  float thresh;
};

SN_DEV float box_area(const float4& b) { return (b.z - b.x + 1.f) * (b.w - b.y + 1.f); }

SN_DEV float iou(const float4& a, float aa, const float4& b) {
  const float w = fmaxf(0.f, fminf(a.z, b.z) - fmaxf(a.x, b.x) + 1.f);
  const float h = fmaxf(0.f, fminf(a.w, b.w) - fmaxf(a.y, b.y) + 1.f);
  const float inter = w * h;
  return inter / (aa + box_area(b) - inter);
}

__global__ void __launch_bounds__(64) proposal_mask_k(const float4* __restrict__ sboxes, const int* __restrict__ cnt,
                                                      u64* __restrict__ mask, const NGeo g) {
  __shared__ float4 s_col[64];
  const int cb = blockIdx.x, rb = blockIdx.y, n = blockIdx.z, lane = threadIdx.x;
  const int M = min(max(cnt[n], 0), g.K), nb = (M + 63) >> 6;
  if (cb < rb || cb >= nb) return;
  const float4* bn = sboxes + (long long)n * g.K;
  const int row = rb * 64 + lane, col = cb * 64 + lane;
  s_col[lane] = col < M ? bn[col] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 me = row < M ? bn[row] : make_float4(0.f, 0.f, 0.f, 0.f);
  const float area = box_area(me);
  __syncthreads();
  u64 word = 0;
  if (row < M) {
    const int c1 = min(64, M - cb * 64);
    for (int c = 0; c < c1; ++c)
      if (cb * 64 + c > row && iou(me, area, s_col[c]) > g.thresh) word |= 1ull << c;
  }
  mask[((long long)n * g.nbk * 64 + row) * g.nbk + cb] = word;
}

SN_DEV u64 uniform64(u64 v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((u64)hi << 32) | lo;
}

__global__ void __launch_bounds__(64) proposal_scan_k(const float4* __restrict__ sboxes, const float* __restrict__ sscores,
                                                      const int* __restrict__ cnt, const u64* __restrict__ mask,
                                                      float* __restrict__ rois, float* __restrict__ scores,
                                                      int* __restrict__ count, const NGeo g) {
  extern __shared__ u64 s_stage[];  // [64 rows][nbk words]: the block's words right of the diagonal
  __shared__ u64 s_removed[MAX_PRE / 64];
  const int n = blockIdx.x, lane = threadIdx.x;
  const int M = min(max(cnt[n], 0), g.K), nb = (M + 63) >> 6;
  const u64* mn = mask + (long long)n * g.nbk * 64 * g.nbk;
  float* rn = rois + (long long)n * g.post * 5;
  float* sn = scores + (long long)n * g.post;
  for (int w = lane; w < MAX_PRE / 64; w += 64) s_removed[w] = 0;
  __syncthreads();
  int total = 0;
  for (int rb = 0; rb < nb && total < g.post; ++rb) {
    const int row = rb * 64 + lane, nw = nb - rb - 1;
    const u64 diag = mn[(long long)row * g.nbk + rb];
    for (int r = 0; r < 64; ++r) {
      const u64* src = mn + (long long)(rb * 64 + r) * g.nbk + rb + 1;
      for (int w = lane; w < nw; w += 64) s_stage[r * g.nbk + w] = src[w];
    }
    __syncthreads();
    u64 rem = uniform64(s_removed[rb]);
    const int valid = M - rb * 64;  // rows of the block that hold a box
    if (valid < 64) rem |= ~0ull << valid;
    u64 kept = 0;
    const uint32_t dlo = (uint32_t)diag, dhi = (uint32_t)(diag >> 32);
#pragma unroll
    for (int r = 0; r < 64; ++r) {
      const uint32_t lo = __builtin_amdgcn_readlane(dlo, r), hi = __builtin_amdgcn_readlane(dhi, r);  // unsigned:
      const u64 d = ((u64)hi << 32) | lo;  // the builtin returns int, whose bit 31 would spread over the high word
      if (!((rem >> r) & 1)) {
        kept |= 1ull << r;
        rem |= d;
      }
    }
    for (int w = lane; w < nw; w += 64) {
      u64 acc = s_removed[rb + 1 + w];
      for (u64 k = kept; k; k &= k - 1) acc |= s_stage[(__ffsll((long long)k) - 1) * g.nbk + w];
      s_removed[rb + 1 + w] = acc;
    }
    const int at = total + __popcll(kept & ((1ull << lane) - 1ull));
    if (((kept >> lane) & 1) && at < g.post) {
      const float4 b = sboxes[(long long)n * g.K + row];
      float* o = rn + (long long)at * 5;
      o[0] = (float)n; o[1] = b.x; o[2] = b.y; o[3] = b.z; o[4] = b.w;
      sn[at] = sscores[(long long)n * g.K + row];
    }
    total = min(g.post, total + __popcll(kept));
    __syncthreads();  // the stage is overwritten and the removed set read by the next block
  }
  for (int j = total + lane; j < g.post; j += 64) {
    float* o = rn + (long long)j * 5;
    o[0] = -1.f; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f; o[4] = 0.f;
    sn[j] = 0.f;
  }
  if (lane == 0) count[n] = total;
}

inline bool al8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// LDS (dynamic plus static) above the default 64 KB needs the kernel's dynamic limit raised to `most`: once per
// device, a failure is not kept.
template <typename K>
inline bool lds_ok(K kernel, size_t lds, int most, bool* raised) {
  if (lds > 160 * 1024) return false;
  if (lds <= 64 * 1024) return true;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  if (dev >= 0 && dev < 64 && raised[dev]) return true;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          most) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (dev >= 0 && dev < 64) raised[dev] = true;
  return true;
}

// K and the mask's blocks for `pre` (0: every box) of B boxes; false outside the kernels' limits.
inline bool nms_geometry(long long N, long long B, long long pre, long long post, float thresh, NGeo& g) {
  if (N < 1 || N > 65535 || B < 1 || B > MAX_BOXES || pre < 0 || pre > MAX_PRE) return false;
  const long long K = pre == 0 || pre > B ? B : pre;
  if (K > MAX_PRE || post < 1 || post > (pre == 0 ? B : pre) || !(thresh >= 0.f && thresh <= 1.f)) return false;
  g.N = (int)N; g.K = (int)K; g.nbk = (int)((K + 63) / 64); g.post = (int)post; g.thresh = thresh;
  return true;
}

}  // namespace

extern "C" {

// boxes[N][A H W][4] and keys[N][A H W] from scores[N][H][W][2A], deltas[N][H][W][4A], im_info[N][3], anchors[A][4].
int sn_proposal_decode(const bf16_t* scores, const bf16_t* deltas, const float* im_info, const float* anchors,
                       float* boxes, uint32_t* keys, long long N, long long H, long long W, long long A,
                       long long feat_stride, float min_size, hipStream_t st) {
  if (!scores || !deltas || !im_info || !anchors || !boxes || !keys) return 2;
  if (N < 1 || N > 65535 || H < 1 || W < 1 || A < 1 || A > MAX_A || A * H * W > MAX_BOXES) return 3;
  if (feat_stride < 1 || feat_stride > 65535 || !(min_size >= 0.f) || !al16(boxes)) return 3;
  DGeo g;
  g.N = (int)N; g.H = (int)H; g.W = (int)W; g.A = (int)A; g.B = (int)(A * H * W); g.stride = (int)feat_stride;
  g.min_size = min_size;
  g.fa = make_fdiv((uint32_t)A); g.fw = make_fdiv((uint32_t)W);
  const dim3 grid((unsigned)((g.B + 255) / 256), (unsigned)N);
  float4* b4 = reinterpret_cast<float4*>(boxes);
  if (al8(deltas)) hipLaunchKernelGGL((proposal_decode_k<true>), grid, dim3(256), 0, st, scores, deltas, im_info, anchors, b4, keys, g);
  else hipLaunchKernelGGL((proposal_decode_k<false>), grid, dim3(256), 0, st, scores, deltas, im_info, anchors, b4, keys, g);
  return SN_CHECK_LAUNCH();
}

// The `pre` (0: all) largest keys of each image, sorted: sboxes[N][K][4], sscores[N][K], cnt[N].
int sn_proposal_select(const uint32_t* keys, const float* boxes, float* sboxes, float* sscores, int* cnt, long long N,
                       long long B, long long pre, hipStream_t st) {
  static bool raised[64];
  if (!keys || !boxes || !sboxes || !sscores || !cnt) return 2;
  NGeo ng;
  if (!nms_geometry(N, B, pre, 1, 0.f, ng) || !al16(boxes) || !al16(sboxes)) return 3;
  SGeo g;
  g.N = (int)N; g.B = (int)B; g.K = ng.K;
  g.P2 = 2;
  while (g.P2 < g.K) g.P2 <<= 1;
  const size_t lds = (size_t)g.P2 * 4;
  if (!lds_ok(proposal_select_k, lds + BINS * 4 + 256, MAX_PRE * 4, raised)) return 4;
  hipLaunchKernelGGL(proposal_select_k, dim3((unsigned)N), dim3(SEL_NT), lds, st, keys,
                     reinterpret_cast<const float4*>(boxes), reinterpret_cast<float4*>(sboxes), sscores, cnt, g);
  return SN_CHECK_LAUNCH();
}

// mask[N][64 nbk][nbk]: the words on and above the diagonal of the blocks that hold boxes.
int sn_proposal_mask(const float* sboxes, const int* cnt, unsigned long long* mask, long long N, long long B,
                     long long pre, float thresh, hipStream_t st) {
  if (!sboxes || !cnt || !mask) return 2;
  NGeo g;
  if (!nms_geometry(N, B, pre, 1, thresh, g) || !al16(sboxes)) return 3;
  hipLaunchKernelGGL(proposal_mask_k, dim3((unsigned)g.nbk, (unsigned)g.nbk, (unsigned)N), dim3(64), 0, st,
                     reinterpret_cast<const float4*>(sboxes), cnt, mask, g);
  return SN_CHECK_LAUNCH();
}

// rois[N post][5], scores[N post], count[N]: the greedy pass over the mask.
int sn_proposal_scan(const float* sboxes, const float* sscores, const int* cnt, const unsigned long long* mask,
                     float* rois, float* scores, int* count, long long N, long long B, long long pre, long long post,
                     float thresh, hipStream_t st) {
  static bool raised[64];
  if (!sboxes || !sscores || !cnt || !mask || !rois || !scores || !count) return 2;
  NGeo g;
  if (!nms_geometry(N, B, pre, post, thresh, g) || !al16(sboxes)) return 3;
  const size_t lds = (size_t)64 * g.nbk * 8;
  if (!lds_ok(proposal_scan_k, lds + MAX_PRE / 8 + 256, MAX_PRE * 8, raised)) return 4;
  hipLaunchKernelGGL(proposal_scan_k, dim3((unsigned)N), dim3(64), lds, st, reinterpret_cast<const float4*>(sboxes),
                     sscores, cnt, mask, rois, scores, count, g);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
