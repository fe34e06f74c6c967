// Squeeze-and-excitation kernels (gfx950): the global average pool ("squeeze") and the
// per-image, per-channel affine ("excitation", Axpy, Scale / Bias with an (N, C) coefficient).
//
//   sn_gap_fwd         y[n, c]    = (1 / HW) sum_p x[n, p, c]                      (1 read of x)
//   sn_nc_affine_fwd   y[n, p, c] = x[n, p, c] s[n, c] + b[n, c] + r[n, p, c]      (1 read of x and r, 1 write)
//   sn_nc_affine_bwd   dx = dy s,  ds[n, c] = sum_p dy x,  db[n, c] = sum_p dy     (1 read of dy and x, 1 write)
//
// s, b, r and every backward output are optional.  On the NHWC storage the coefficient of image
// n is one contiguous C-vector that applies to every pixel row of the image, so nothing is
// transposed: Caffe's spelling (Scale with axis 0 on NCHW) walks H W-strided planes instead.
//
// Geometry: [N][HW][C], rows of C contiguous channels, 64-bit element offsets.  A block is TX
// channel groups x TY row lanes (TX * TY = 256, TX <= 64 a power of two), as in bn_scale.hip; a
// lane owns V consecutive channels — V = 8 bf16 or 4 fp32 per 16-byte access when C % 8 == 0,
// else V = 1 — keeps its image's coefficients in registers and strides over the rows of its
// slab.  grid = (channel-group tiles, HW slabs, N).
//
// Every reduction is deterministic: a block combines its row lanes in lane order; when one slab
// covers HW it writes the result itself (one launch), otherwise one fp32 partial per
// (slab, n, c) and a finalize launch combines the slabs in a fixed order (FL lanes, each over a
// contiguous run of slabs in slab order, then the lanes in lane order).  No float atomics.
#include "common.h"
#include "row_io.h"  // ldx / stx

namespace {

enum { GRAD_SKIP = 0, GRAD_STORE = 1, GRAD_ACC = 2 };
constexpr int U = 4;    // rows a lane loads before it consumes them
constexpr int FC = 8;   // finalize block: FC outputs x FL slab lanes
constexpr int FL = 32;
constexpr long long MAX_BLOCKS = 1024;  // per launch: 4 per CU
constexpr long long MIN_ROWS = 64;      // per slab

struct Plan {
  int txlog, gx, slabs;
  long long rps;  // rows per slab
};

// bn_scale.hip's make_plan with HW in place of R and the images as grid.z: a slab is >= 8 rows
// per lane and >= MIN_ROWS rows, so the two fp32 partials per (slab, n, c) cost <= 1/16 of the
// bf16 activation traffic; gx * slabs * N <= MAX_BLOCKS unless one slab per image already exceeds it.
inline Plan make_plan(long long N, long long HW, long long C, int V) {
  const long long CG = C / V;
  Plan p;
  p.txlog = 0;
  while ((1 << p.txlog) < 64 && (1LL << p.txlog) < CG) ++p.txlog;
  const int TX = 1 << p.txlog, TY = 256 >> p.txlog;
  p.gx = (int)((CG + TX - 1) / TX);
  long long cap = MAX_BLOCKS / (p.gx * N);
  if (cap < 1) cap = 1;
  const long long min_rows = TY * 8LL > MIN_ROWS ? TY * 8LL : MIN_ROWS;
  long long want = (HW + min_rows - 1) / min_rows;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  p.rps = (HW + want - 1) / want;
  p.slabs = (int)((HW + p.rps - 1) / p.rps);
  return p;
}

struct Lane {
  int cl, rl, TX, TY, c0;
  bool act;
  long long r0, r1;  // rows of the whole [N HW] tensor: image blockIdx.z, slab blockIdx.y
  long long nc;      // offset of the image's coefficients in an [N][C] vector
};

template <int V>
SN_DEV Lane lane_of(long long HW, int C, int txlog, long long rps) {
  Lane l;
  l.TX = 1 << txlog;
  l.TY = 256 >> txlog;
  l.cl = threadIdx.x & (l.TX - 1);
  l.rl = threadIdx.x >> txlog;
  l.c0 = (blockIdx.x * l.TX + l.cl) * V;
  l.act = l.c0 < C;  // C % V == 0: an active lane's V channels are all inside
  const long long p0 = blockIdx.y * rps;
  const long long base = (long long)blockIdx.z * HW;
  l.r0 = base + p0;
  l.r1 = base + min(HW, p0 + rps);
  l.nc = (long long)blockIdx.z * C;
  return l;
}

// Row lanes of a block in lane order -> the sum of channel j of column lane cl.
template <int V>
SN_DEV float lane_sum(const float* sm, const Lane& l, int j) {
  float a = 0.f;
  for (int k = 0; k < l.TY; ++k) a += sm[j * 256 + k * l.TX + l.cl];
  return a;
}

SN_DEV void emit(float* out, long long o, float v, int flag) {
  if (flag != GRAD_SKIP) out[o] = flag == GRAD_ACC ? out[o] + v : v;
}

// ---------------------------------------------------------------------------------------
// Global average pool.  part == null: one slab, y is written here.
// ---------------------------------------------------------------------------------------
template <int V, int DT>
__global__ void __launch_bounds__(256) gap_k(const void* __restrict__ x, long long HW, int C, int txlog, long long rps,
                                             float inv_hw, void* __restrict__ y, float* __restrict__ part) {
  __shared__ float sm[V * 256];
  const Lane l = lane_of<V>(HW, C, txlog, rps);
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  if (l.act) {
    long long r = l.r0 + l.rl;
    for (; r + (U - 1) * l.TY < l.r1; r += U * l.TY) {  // U independent row loads, then the adds
      float f[U][V];
#pragma unroll
      for (int u = 0; u < U; ++u) ldx<V, DT>(x, (r + u * l.TY) * C + l.c0, f[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += f[u][j];
      }
    }
    for (; r < l.r1; r += l.TY) {
      float f[V];
      ldx<V, DT>(x, r * C + l.c0, f);
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] += f[j];
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) sm[j * 256 + threadIdx.x] = acc[j];
  __syncthreads();
  if (l.rl != 0 || !l.act) return;
  float out[V];
#pragma unroll
  for (int j = 0; j < V; ++j) out[j] = lane_sum<V>(sm, l, j);
  if (part) {
    const long long NC = (long long)gridDim.z * C;
#pragma unroll
    for (int j = 0; j < V; ++j) part[blockIdx.y * NC + l.nc + l.c0 + j] = out[j];
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) out[j] *= inv_hw;
    stx<V, DT>(y, l.nc + l.c0, out);
  }
}

// Slab sums in a fixed order -> y = sum / HW.  One output per (n, c): NC = N C.
template <int DT>
__global__ void __launch_bounds__(FC * FL) gap_finalize_k(const float* __restrict__ part, int slabs, long long NC,
                                                          float inv_hw, void* __restrict__ y) {
  __shared__ float sa[FL][FC];
  const int cj = threadIdx.x % FC, k = threadIdx.x / FC;
  const long long j = (long long)blockIdx.x * FC + cj;
  const int chunk = (slabs + FL - 1) / FL, s0 = k * chunk, s1 = min(slabs, s0 + chunk);
  float a = 0.f;
  if (j < NC) {
#pragma unroll 4
    for (int s = s0; s < s1; ++s) a += part[s * NC + j];
  }
  sa[k][cj] = a;
  __syncthreads();
  if (k != 0 || j >= NC) return;
  for (int q = 1; q < FL; ++q) a += sa[q][cj];
  a *= inv_hw;
  stx<1, DT>(y, j, &a);
}

// ---------------------------------------------------------------------------------------
// Forward: y = x s[n] + b[n] + r   (s, b, r may be null)
// ---------------------------------------------------------------------------------------
template <int V, int DT>
__global__ void __launch_bounds__(256) nc_affine_fwd_k(const void* __restrict__ x, const void* __restrict__ r_,
                                                       void* __restrict__ y, long long HW, int C, int txlog,
                                                       long long rps, const float* __restrict__ s,
                                                       const float* __restrict__ b) {
  const Lane l = lane_of<V>(HW, C, txlog, rps);
  if (!l.act) return;
  float sv[V], bv[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sv[j] = s ? s[l.nc + l.c0 + j] : 1.f;
    bv[j] = b ? b[l.nc + l.c0 + j] : 0.f;
  }
  const bool res = r_ != nullptr;
  long long r = l.r0 + l.rl;
  for (; r + (U - 1) * l.TY < l.r1; r += U * l.TY) {
    float f[U][V], g[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long e = (r + u * l.TY) * C + l.c0;
      ldx<V, DT>(x, e, f[u]);
      if (res) ldx<V, DT>(r_, e, g[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        f[u][j] = fmaf(f[u][j], sv[j], bv[j]);
        if (res) f[u][j] += g[u][j];
      }
      stx<V, DT>(y, (r + u * l.TY) * C + l.c0, f[u]);
    }
  }
  for (; r < l.r1; r += l.TY) {
    float f[V], g[V];
    const long long e = r * C + l.c0;
    ldx<V, DT>(x, e, f);
    if (res) ldx<V, DT>(r_, e, g);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      f[j] = fmaf(f[j], sv[j], bv[j]);
      if (res) f[j] += g[j];
    }
    stx<V, DT>(y, e, f);
  }
}

// ---------------------------------------------------------------------------------------
// Backward: one pass over dy (and x when ds is wanted).  dx = dy s (dx may be null),
// sum_p dy x and sum_p dy per (n, c).  part == null: one slab, ds / db are written here;
// else part[slab][0][NC] = sum dy x, part[slab][1][NC] = sum dy.
// ---------------------------------------------------------------------------------------
template <int V, int DT>
__global__ void __launch_bounds__(256) nc_affine_bwd_k(const void* __restrict__ dy, const void* __restrict__ x,
                                                       void* __restrict__ dx, long long HW, int C, int txlog,
                                                       long long rps, const float* __restrict__ s, int need_s,
                                                       int need_b, float* __restrict__ part, float* __restrict__ ds,
                                                       int sflag, float* __restrict__ db, int bflag) {
  __shared__ float sm[2][V * 256];
  const Lane l = lane_of<V>(HW, C, txlog, rps);
  const bool want_dx = dx != nullptr;
  float sg[V], sgx[V];
#pragma unroll
  for (int j = 0; j < V; ++j) sg[j] = sgx[j] = 0.f;
  if (l.act) {
    float sv[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sv[j] = s ? s[l.nc + l.c0 + j] : 1.f;
    auto load = [&](long long r, float* g, float* xv) {
      const long long e = r * C + l.c0;
      ldx<V, DT>(dy, e, g);
      if (need_s) ldx<V, DT>(x, e, xv);
    };
    auto finish = [&](long long r, float* g, const float* xv) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sg[j] += g[j];
        if (need_s) sgx[j] = fmaf(g[j], xv[j], sgx[j]);
        g[j] *= sv[j];
      }
      if (want_dx) stx<V, DT>(dx, r * C + l.c0, g);
    };
    long long r = l.r0 + l.rl;
    for (; r + l.TY < l.r1; r += 2 * l.TY) {  // two rows (up to four loads) in flight per lane
      float g[2][V], xv[2][V];
      load(r, g[0], xv[0]);
      load(r + l.TY, g[1], xv[1]);
      finish(r, g[0], xv[0]);
      finish(r + l.TY, g[1], xv[1]);
    }
    if (r < l.r1) {
      float g[V], xv[V];
      load(r, g, xv);
      finish(r, g, xv);
    }
  }
  if (!need_s && !need_b) return;  // uniform: dx alone needs no reduction
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sm[0][j * 256 + threadIdx.x] = sgx[j];
    sm[1][j * 256 + threadIdx.x] = sg[j];
  }
  __syncthreads();
  if (l.rl != 0 || !l.act) return;
  const long long NC = (long long)gridDim.z * C;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const long long o = l.nc + l.c0 + j;
    const float a = need_s ? lane_sum<V>(sm[0], l, j) : 0.f;
    const float b = need_b ? lane_sum<V>(sm[1], l, j) : 0.f;
    if (part) {
      if (need_s) part[((long long)blockIdx.y * 2) * NC + o] = a;
      if (need_b) part[((long long)blockIdx.y * 2 + 1) * NC + o] = b;
    } else {
      if (need_s) emit(ds, o, a, sflag);
      if (need_b) emit(db, o, b, bflag);
    }
  }
}

__global__ void __launch_bounds__(FC * FL) nc_affine_bwd_finalize_k(const float* __restrict__ part, int slabs,
                                                                    long long NC, int need_s, int need_b,
                                                                    float* __restrict__ ds, int sflag,
                                                                    float* __restrict__ db, int bflag) {
  __shared__ float sa[FL][FC], sb[FL][FC];
  const int cj = threadIdx.x % FC, k = threadIdx.x / FC;
  const long long j = (long long)blockIdx.x * FC + cj;
  const int chunk = (slabs + FL - 1) / FL, s0 = k * chunk, s1 = min(slabs, s0 + chunk);
  float a = 0.f, b = 0.f;
  if (j < NC) {
#pragma unroll 4
    for (int s = s0; s < s1; ++s) {
      if (need_s) a += part[((long long)s * 2) * NC + j];
      if (need_b) b += part[((long long)s * 2 + 1) * NC + j];
    }
  }
  sa[k][cj] = a;
  sb[k][cj] = b;
  __syncthreads();
  if (k != 0 || j >= NC) return;
  for (int q = 1; q < FL; ++q) {
    a += sa[q][cj];
    b += sb[q][cj];
  }
  if (need_s) emit(ds, j, a, sflag);
  if (need_b) emit(db, j, b, bflag);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// lane width: 16-byte accesses need C % 8 == 0 and aligned tensors (null pointers are aligned)
inline int pick_v(long long dt, long long C, const void* a, const void* b, const void* c) {
  if (C % 8 != 0 || !al16(a) || !al16(b) || !al16(c)) return 1;
  return dt ? 4 : 8;
}

// grid.z = N; the [N][C] outputs are indexed below 2^31
inline bool bad_geom(long long N, long long HW, long long C) {
  return N < 1 || HW < 1 || C < 1 || N > 65535 || C > 2147483647LL / 8 || N * C > 2147483647LL / 8;
}

}  // namespace

#define SN_SE_DISPATCH(KERNEL, V, DT, ...)                                                              \
  do {                                                                                                  \
    const dim3 grid((unsigned)pl.gx, (unsigned)pl.slabs, (unsigned)N);                                  \
    if (V == 8)                                                                                         \
      hipLaunchKernelGGL((KERNEL<8, 0>), grid, dim3(256), 0, st, __VA_ARGS__);                          \
    else if (V == 4)                                                                                    \
      hipLaunchKernelGGL((KERNEL<4, 1>), grid, dim3(256), 0, st, __VA_ARGS__);                          \
    else if (DT)                                                                                        \
      hipLaunchKernelGGL((KERNEL<1, 1>), grid, dim3(256), 0, st, __VA_ARGS__);                          \
    else                                                                                                \
      hipLaunchKernelGGL((KERNEL<1, 0>), grid, dim3(256), 0, st, __VA_ARGS__);                          \
  } while (0)

extern "C" {

// Floats the partial workspace of sn_gap_fwd / sn_nc_affine_bwd needs (the larger of the two
// lane widths); 0 when one slab covers HW and no finalize launch is made.
long long sn_nc_part_floats(long long N, long long HW, long long C, long long dt) {
  if (bad_geom(N, HW, C)) return -1;
  long long s = make_plan(N, HW, C, 1).slabs;
  if (C % 8 == 0) {
    const long long sv = make_plan(N, HW, C, dt ? 4 : 8).slabs;
    if (sv > s) s = sv;
  }
  return s > 1 ? s * 2 * N * C : 0;
}

int sn_gap_fwd(const void* x, void* y, long long dt, long long N, long long HW, long long C, float* part,
               long long part_floats, hipStream_t st) {
  if (bad_geom(N, HW, C)) return 3;
  const int V = pick_v(dt, C, x, y, nullptr);
  const Plan pl = make_plan(N, HW, C, V);
  const long long NC = N * C;
  const float inv_hw = 1.f / (float)HW;
  if (pl.slabs == 1) {
    SN_SE_DISPATCH(gap_k, V, dt, x, HW, (int)C, pl.txlog, pl.rps, inv_hw, y, (float*)nullptr);
    return SN_CHECK_LAUNCH();
  }
  if (!part || (long long)pl.slabs * NC > part_floats) return 3;
  SN_SE_DISPATCH(gap_k, V, dt, x, HW, (int)C, pl.txlog, pl.rps, inv_hw, y, part);
  if (hipGetLastError() != hipSuccess) return 1;
  const dim3 fgrid((unsigned)((NC + FC - 1) / FC));
  if (dt)
    hipLaunchKernelGGL(gap_finalize_k<1>, fgrid, dim3(FC * FL), 0, st, part, pl.slabs, NC, inv_hw, y);
  else
    hipLaunchKernelGGL(gap_finalize_k<0>, fgrid, dim3(FC * FL), 0, st, part, pl.slabs, NC, inv_hw, y);
  return SN_CHECK_LAUNCH();
}

int sn_nc_affine_fwd(const void* x, const void* r, void* y, long long dt, long long N, long long HW, long long C,
                     const float* s, const float* b, hipStream_t st) {
  if (bad_geom(N, HW, C)) return 3;
  const int V = pick_v(dt, C, x, r, y);
  const Plan pl = make_plan(N, HW, C, V);
  SN_SE_DISPATCH(nc_affine_fwd_k, V, dt, x, r, y, HW, (int)C, pl.txlog, pl.rps, s, b);
  return SN_CHECK_LAUNCH();
}

// sflag / bflag: 0 skip, 1 store, 2 accumulate (ds needs x; dx needs s).
int sn_nc_affine_bwd(const void* dy, const void* x, void* dx, long long dt, long long N, long long HW, long long C,
                     const float* s, float* part, long long part_floats, float* ds, long long sflag, float* db,
                     long long bflag, hipStream_t st) {
  if (bad_geom(N, HW, C)) return 3;
  const int need_s = sflag != GRAD_SKIP, need_b = bflag != GRAD_SKIP;
  if ((need_s && (!x || !ds)) || (need_b && !db) || (dx && !s)) return 2;
  if (!dx && !need_s && !need_b) return 0;
  const int V = pick_v(dt, C, dy, need_s ? x : nullptr, dx);
  const Plan pl = make_plan(N, HW, C, V);
  const long long NC = N * C;
  const bool split = pl.slabs > 1 && (need_s || need_b);
  if (split && (!part || (long long)pl.slabs * 2 * NC > part_floats)) return 3;
  SN_SE_DISPATCH(nc_affine_bwd_k, V, dt, dy, x, dx, HW, (int)C, pl.txlog, pl.rps, s, need_s, need_b,
                 split ? part : (float*)nullptr, ds, (int)sflag, db, (int)bflag);
  if (!split) return SN_CHECK_LAUNCH();
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(nc_affine_bwd_finalize_k, dim3((unsigned)((NC + FC - 1) / FC)), dim3(FC * FL), 0, st, part,
                     pl.slabs, NC, need_s, need_b, ds, (int)sflag, db, (int)bflag);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
