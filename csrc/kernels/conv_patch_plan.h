// Host-side band and LDS arithmetic of the patch-resident 5x5 data gradient (conv_patch.hip).
// Plain C++ with no HIP in it, so that a stand-alone program can check it under a sanitizer.
#pragma once
#include <stddef.h>

namespace sn_patch {

constexpr int KG = 128;            // dy channels per group (the reduction, per tap)
constexpr int CG = 48;             // dx channels per group (the output columns)
constexpr int RS = 5, TAPS = 25;   // the window; stride 1, pad 2
constexpr int HALO = RS - 1;       // extra patch rows and columns
constexpr int NWAVE = 4, MWAVE = 64, MBLK = NWAVE * MWAVE;  // dx pixels of a block
constexpr int HPIX = 144;          // LDS bytes of a pixel (or weight row) in one half image: 8 chunks + 16 B of padding
constexpr int WHALF = CG * HPIX;   // one half image of a tap's weights: 6912 B = 27 bank rows
constexpr int WSLOT = 2 * WHALF;   // a tap's weights
constexpr int RING = 3;            // taps in the weight ring
constexpr int LDS_MAX = 160 * 1024;
constexpr int PPT = 27;           // patch pixels a thread stages at most, 16 threads a pixel: 432 pixels

struct Plan {
  int N, H, W, G;      // dx is [N][H][W][ldo], dy [N][H][W][ldd]; G groups
  int bh, nb;          // dx rows of a band, bands per image (the last may be shorter)
  int pw;              // patch columns = W + HALO
  int half;            // bytes of one half image of the patch (a multiple of the 256-B bank row)
  long long ldd, ldo;  // pixel strides in elements
  unsigned items;      // (image, group, band) triples = blocks' worth of work
  size_t lds;
};

inline int patch_half(int bh, int pw) { return ((bh + HALO) * pw * HPIX + 255) & ~255; }

// The plan for a geometry, false where the kernel does not take it.  A band is as many whole
// dx rows as fit the block's MBLK pixels, the LDS left beside the weight ring and the registers
// a block stages a patch through (16 * PPT pixels), then evened
// out over the image so that the last band is at most one row short.
inline bool make_plan(long long N, long long H, long long W, long long G, long long ldd, long long ldo, Plan& p) {
  if (N < 1 || H < 1 || W < 8 || G < 1 || W > MBLK || H > (1 << 20) || G > (1 << 12)) return false;
  if (ldd < G * KG || ldo < G * CG || ldd > (1 << 20) || ldo > (1 << 20) || ldd % 8 != 0 || ldo % 4 != 0) return false;
  if (N * H * W >= (1LL << 30) || H * W * ldd >= (1LL << 30)) return false;  // 32-bit offsets inside an image
  const int pw = (int)W + HALO;
  int bh = MBLK / (int)W;
  if (bh > H) bh = (int)H;
  while (bh >= 1 && (RING * WSLOT + 2 * patch_half(bh, pw) > LDS_MAX || (bh + HALO) * pw > 16 * PPT)) --bh;
  if (bh < 1) return false;
  const int nb = ((int)H + bh - 1) / bh;
  bh = ((int)H + nb - 1) / nb;
  if (N * G * nb >= (1LL << 31)) return false;
  p.N = (int)N; p.H = (int)H; p.W = (int)W; p.G = (int)G;
  p.bh = bh; p.nb = nb; p.pw = pw; p.half = patch_half(bh, pw);
  p.ldd = ldd; p.ldo = ldo;
  p.items = (unsigned)(N * G * nb);
  p.lds = (size_t)RING * WSLOT + 2 * (size_t)p.half;
  return true;
}

}  // namespace sn_patch
