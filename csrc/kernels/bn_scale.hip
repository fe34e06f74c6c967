// Fused BatchNorm -> Scale -> ReLU kernels (gfx950) and the per-channel Scale / Bias layers.
//
// Caffe runs the chain as three layers (batch_norm_layer.cu, scale_layer.cu, relu_layer.cu):
// about 8 passes over the activation forward and 14 backward.  Here the chain is
//   forward   stats (1 read of x)  ->  y = relu?(gamma (x - mean) inv_std + beta)  (1 read, 1 write)
//   backward  pass 1: sum g, sum g xhat per channel (reads dy, y, x)
//             pass 2: dx = gamma inv_std (g - sum g / M - xhat sum g xhat / M)  (reads dy, y, x; writes dx)
// with g = dy [y > 0] and xhat = (x - mean) inv_std recomputed from the saved input, so neither
// xhat nor the Scale input is ever stored.  With global statistics the coefficients come from
// the running blobs inside the same kernels (one launch forward).  A "no normalisation"
// instance (mean 0, inv_std 1) is the standalone per-channel Scale / Bias layer.
//
// Geometry: R rows of C contiguous channels (NHWC blobs: R = N H W; 2-D blobs: R = N); element
// offsets are 64-bit.  A block is TX channel groups x TY row lanes (TX * TY = 256, TX <= 64 a
// power of two); a lane owns V consecutive channels — V = 8 bf16 or 4 fp32 per 16-byte access
// when C % 8 == 0, else V = 1 (the scalar tail path) — keeps their coefficients in registers and
// strides over the rows of its slab.  grid = (channel-group tiles, row slabs).
//
// Every reduction is deterministic: a block combines its row lanes in lane order and writes one
// partial per (slab, channel); a finalize launch combines the slabs in a fixed order (32 lanes,
// each over a contiguous run of slabs in slab order, then the lanes in lane order: a serial
// walk over ~1000 slabs cost more than the reduction itself).  No float atomics.  The statistics are Welford (count, mean, M2) triples merged with the parallel-
// variance formula (Chan et al.), never E[x^2] - E[x]^2; the count of a partial follows from
// the geometry and is not stored.
#include "common.h"
#include "row_io.h"  // ldx / stx

namespace {

enum { ST_NONE = 0, ST_BATCH = 1, ST_GLOBAL = 2 };  // where mean / inv_std come from
enum { GRAD_SKIP = 0, GRAD_STORE = 1, GRAD_ACC = 2 };
constexpr int U = 4;    // rows a lane loads before it consumes them
constexpr int FC = 8;   // finalize block: FC channels x FL slab lanes
constexpr int FL = 32;

struct Plan {
  int txlog, gx, slabs;
  long long rps;  // rows per slab
};

// A slab is >= 8 rows per lane and >= 64 rows (partials then cost <= 1/16 of the activation
// traffic); at most 1024 blocks per launch (4 per CU, each lane with U row loads in flight).
inline Plan make_plan(long long R, long long C, int V) {
  const long long CG = C / V;
  Plan p;
  p.txlog = 0;
  while ((1 << p.txlog) < 64 && (1LL << p.txlog) < CG) ++p.txlog;
  const int TX = 1 << p.txlog, TY = 256 >> p.txlog;
  p.gx = (int)((CG + TX - 1) / TX);
  long long cap = 1024 / p.gx;
  if (cap < 1) cap = 1;
  const long long min_rows = TY * 8LL > 64 ? TY * 8LL : 64;
  long long want = (R + min_rows - 1) / min_rows;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  p.rps = (R + want - 1) / want;
  p.slabs = (int)((R + p.rps - 1) / p.rps);
  return p;
}

// mean and inv_std of channels c0 .. c0 + V - 1.  ST_BATCH: sa = mean, sb = inv_std.
// ST_GLOBAL: sa / sb = running mean / variance sums, scaled by 1 / factor (0 when factor == 0).
template <int V>
SN_DEV void load_stats(int mode, const float* __restrict__ sa, const float* __restrict__ sb,
                       const float* __restrict__ factor, float eps, int c0, float* mu, float* inv) {
  float s = 0.f;
  if (mode == ST_GLOBAL) {
    const float f = factor[0];
    s = f == 0.f ? 0.f : 1.f / f;
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (mode == ST_BATCH) {
      mu[j] = sa[c0 + j];
      inv[j] = sb[c0 + j];
    } else if (mode == ST_GLOBAL) {
      mu[j] = sa[c0 + j] * s;
      inv[j] = rsqrtf(sb[c0 + j] * s + eps);
    } else {
      mu[j] = 0.f;
      inv[j] = 1.f;
    }
  }
}

struct Lane {
  int cl, rl, TX, TY, c0;
  bool act;
  long long r0, r1;
};

template <int V>
SN_DEV Lane lane_of(long long R, int C, int txlog, long long rps) {
  Lane l;
  l.TX = 1 << txlog;
  l.TY = 256 >> txlog;
  l.cl = threadIdx.x & (l.TX - 1);
  l.rl = threadIdx.x >> txlog;
  l.c0 = (blockIdx.x * l.TX + l.cl) * V;
  l.act = l.c0 < C;  // C % V == 0: an active lane's V channels are all inside
  l.r0 = blockIdx.y * rps;
  l.r1 = min(R, l.r0 + rps);
  return l;
}

// ---------------------------------------------------------------------------------------
// Statistics: one read of x -> per-(slab, channel) Welford partials (mean, M2)
// ---------------------------------------------------------------------------------------
SN_DEV void chan_merge(float& na, float& ma, float& m2a, float nb, float mb, float m2b) {
  if (nb == 0.f) return;
  const float n = na + nb, d = mb - ma, w = nb / n;
  ma += d * w;
  m2a += m2b + d * d * na * w;
  na = n;
}

template <int V>
SN_DEV void welford(const float* f, float& n, float* mean, float* m2) {
  n += 1.f;
  const float rn = __builtin_amdgcn_rcpf(n);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float d = f[j] - mean[j];
    mean[j] += d * rn;
    m2[j] += d * (f[j] - mean[j]);
  }
}

template <int V, int DT>
__global__ void __launch_bounds__(256) bn_stats_k(const void* __restrict__ x, long long R, int C, int txlog,
                                                  long long rps, float* __restrict__ pmean,
                                                  float* __restrict__ pm2) {
  __shared__ float sm[2][V * 256];
  const Lane l = lane_of<V>(R, C, txlog, rps);
  float mean[V], m2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) mean[j] = m2[j] = 0.f;
  if (l.act) {
    float n = 0.f;
    long long r = l.r0 + l.rl;
    for (; r + (U - 1) * l.TY < l.r1; r += U * l.TY) {  // U independent row loads, then the updates
      float f[U][V];
#pragma unroll
      for (int u = 0; u < U; ++u) ldx<V, DT>(x, (r + u * l.TY) * C + l.c0, f[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) welford<V>(f[u], n, mean, m2);
    }
    for (; r < l.r1; r += l.TY) {
      float f[V];
      ldx<V, DT>(x, r * C + l.c0, f);
      welford<V>(f, n, mean, m2);
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sm[0][j * 256 + threadIdx.x] = mean[j];
    sm[1][j * 256 + threadIdx.x] = m2[j];
  }
  __syncthreads();
  if (l.rl != 0 || !l.act) return;
  const long long rows = l.r1 - l.r0;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float na = 0.f, ma = 0.f, m2a = 0.f;
    for (int k = 0; k < l.TY; ++k) {
      const float nb = rows > k ? (float)((rows - k + l.TY - 1) / l.TY) : 0.f;  // rows of lane k
      chan_merge(na, ma, m2a, nb, sm[0][j * 256 + k * l.TX + l.cl], sm[1][j * 256 + k * l.TX + l.cl]);
    }
    pmean[(long long)blockIdx.y * C + l.c0 + j] = ma;
    pm2[(long long)blockIdx.y * C + l.c0 + j] = m2a;
  }
}

// Slab merge in a fixed order (FL lanes, each over a contiguous run of slabs); mean, biased variance, inv_std = rsqrt(var + eps), and Caffe's
// running-statistics update (batch_norm_layer.cpp): factor = frac factor + 1,
// running mean = frac mean + batch mean, running var = frac var + m / (m - 1) batch var.
__global__ void __launch_bounds__(FC * FL) bn_stats_finalize_k(
    const float* __restrict__ pmean, const float* __restrict__ pm2, int slabs, long long R, long long rps, int C,
    float eps, float* __restrict__ mean, float* __restrict__ var, float* __restrict__ inv, float* __restrict__ rmean,
    float* __restrict__ rvar, float* __restrict__ factor, float frac, float unbias) {
  __shared__ float sn[FL][FC], sm[FL][FC], s2[FL][FC];
  const int cj = threadIdx.x % FC, k = threadIdx.x / FC;
  const int j = blockIdx.x * FC + cj;
  if (rmean && blockIdx.x == 0 && threadIdx.x == 0) factor[0] = frac * factor[0] + 1.f;
  // lane k merges its contiguous run of slabs in order, then the lanes are merged in order
  const int chunk = (slabs + FL - 1) / FL, s0 = k * chunk, s1 = min(slabs, s0 + chunk);
  float na = 0.f, ma = 0.f, m2a = 0.f;
  if (j < C) {
#pragma unroll 4
    for (int s = s0; s < s1; ++s) {
      const long long nb = min(rps, R - s * rps);
      chan_merge(na, ma, m2a, (float)nb, pmean[(long long)s * C + j], pm2[(long long)s * C + j]);
    }
  }
  sn[k][cj] = na;
  sm[k][cj] = ma;
  s2[k][cj] = m2a;
  __syncthreads();
  if (k != 0 || j >= C) return;
  for (int q = 1; q < FL; ++q) chan_merge(na, ma, m2a, sn[q][cj], sm[q][cj], s2[q][cj]);
  const float v = m2a / (float)R;
  mean[j] = ma;
  if (var) var[j] = v;
  inv[j] = rsqrtf(v + eps);
  if (rmean) {
    rmean[j] = frac * rmean[j] + ma;
    rvar[j] = frac * rvar[j] + unbias * v;
  }
}

// ---------------------------------------------------------------------------------------
// Forward: y = relu?(gamma (x - mean) inv_std + beta)
// ---------------------------------------------------------------------------------------
template <int V, int DT>
__global__ void __launch_bounds__(256) bn_fwd_k(const void* __restrict__ x, void* __restrict__ y, long long R, int C,
                                                int txlog, long long rps, const float* __restrict__ sa,
                                                const float* __restrict__ sb, const float* __restrict__ factor,
                                                float eps, int mode, const float* __restrict__ gamma,
                                                const float* __restrict__ beta, int relu) {
  const Lane l = lane_of<V>(R, C, txlog, rps);
  if (!l.act) return;
  float mu[V], gi[V], b[V];
  load_stats<V>(mode, sa, sb, factor, eps, l.c0, mu, gi);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    if (gamma) gi[j] *= gamma[l.c0 + j];
    b[j] = beta ? beta[l.c0 + j] : 0.f;
  }
  auto apply = [&](float* f) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      f[j] = fmaf(f[j] - mu[j], gi[j], b[j]);
      if (relu) f[j] = fmaxf(f[j], 0.f);
    }
  };
  long long r = l.r0 + l.rl;
  for (; r + (U - 1) * l.TY < l.r1; r += U * l.TY) {
    float f[U][V];
#pragma unroll
    for (int u = 0; u < U; ++u) ldx<V, DT>(x, (r + u * l.TY) * C + l.c0, f[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      apply(f[u]);
      stx<V, DT>(y, (r + u * l.TY) * C + l.c0, f[u]);
    }
  }
  for (; r < l.r1; r += l.TY) {
    float f[V];
    ldx<V, DT>(x, r * C + l.c0, f);
    apply(f);
    stx<V, DT>(y, r * C + l.c0, f);
  }
}

// ---------------------------------------------------------------------------------------
// Backward pass 1: per-(slab, channel) sum g and sum g xhat, g = dy [y > 0]
// part[slab][0][C] = sum g, part[slab][1][C] = sum g xhat (left unwritten when !need_x)
// ---------------------------------------------------------------------------------------
template <int V, int DT>
__global__ void __launch_bounds__(256) bn_bwd_red_k(const void* __restrict__ dy, const void* __restrict__ x,
                                                    const void* __restrict__ y, long long R, int C, int txlog,
                                                    long long rps, const float* __restrict__ sa,
                                                    const float* __restrict__ sb, const float* __restrict__ factor,
                                                    float eps, int mode, int relu, int need_x,
                                                    float* __restrict__ part) {
  __shared__ float sm[2][V * 256];
  const Lane l = lane_of<V>(R, C, txlog, rps);
  float sg[V], sgx[V];
#pragma unroll
  for (int j = 0; j < V; ++j) sg[j] = sgx[j] = 0.f;
  if (l.act) {
    float mu[V], inv[V];
    load_stats<V>(mode, sa, sb, factor, eps, l.c0, mu, inv);
    auto load = [&](long long r, float* g, float* yv, float* xv) {
      const long long e = r * C + l.c0;
      ldx<V, DT>(dy, e, g);
      if (relu) ldx<V, DT>(y, e, yv);
      if (need_x) ldx<V, DT>(x, e, xv);
    };
    auto accum = [&](float* g, const float* yv, const float* xv) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (relu) g[j] = yv[j] > 0.f ? g[j] : 0.f;
        sg[j] += g[j];
        if (need_x) sgx[j] = fmaf(g[j], (xv[j] - mu[j]) * inv[j], sgx[j]);
      }
    };
    long long r = l.r0 + l.rl;
    for (; r + l.TY < l.r1; r += 2 * l.TY) {  // two rows (up to six loads) in flight per lane
      float g[2][V], yv[2][V], xv[2][V];
      load(r, g[0], yv[0], xv[0]);
      load(r + l.TY, g[1], yv[1], xv[1]);
      accum(g[0], yv[0], xv[0]);
      accum(g[1], yv[1], xv[1]);
    }
    if (r < l.r1) {
      float g[V], yv[V], xv[V];
      load(r, g, yv, xv);
      accum(g, yv, xv);
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) {
    sm[0][j * 256 + threadIdx.x] = sg[j];
    sm[1][j * 256 + threadIdx.x] = sgx[j];
  }
  __syncthreads();
  if (l.rl != 0 || !l.act) return;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < l.TY; ++k) {
      a += sm[0][j * 256 + k * l.TX + l.cl];
      b += sm[1][j * 256 + k * l.TX + l.cl];
    }
    part[((long long)blockIdx.y * 2) * C + l.c0 + j] = a;
    part[((long long)blockIdx.y * 2 + 1) * C + l.c0 + j] = b;
  }
}

// Slab sums in the same fixed order -> dbeta = sum g, dgamma = sum g xhat (stored, accumulated or
// skipped), and the two per-channel coefficients of pass 2: coef[0][c] = sum g / M,
// coef[1][c] = sum g xhat / M (both 0 unless the statistics are the batch's).
__global__ void __launch_bounds__(FC * FL) bn_bwd_finalize_k(const float* __restrict__ part, int slabs, int C,
                                                             float inv_m, int mode, int need_x,
                                                             float* __restrict__ dgamma, int gflag,
                                                             float* __restrict__ dbeta, int bflag,
                                                             float* __restrict__ coef) {
  __shared__ float sa[FL][FC], sb[FL][FC];
  const int cj = threadIdx.x % FC, k = threadIdx.x / FC;
  const int j = blockIdx.x * FC + cj;
  const int chunk = (slabs + FL - 1) / FL, s0 = k * chunk, s1 = min(slabs, s0 + chunk);
  float a = 0.f, b = 0.f;
  if (j < C) {
#pragma unroll 4
    for (int s = s0; s < s1; ++s) {
      a += part[((long long)s * 2) * C + j];
      if (need_x) b += part[((long long)s * 2 + 1) * C + j];
    }
  }
  sa[k][cj] = a;
  sb[k][cj] = b;
  __syncthreads();
  if (k != 0 || j >= C) return;
  for (int q = 1; q < FL; ++q) {
    a += sa[q][cj];
    b += sb[q][cj];
  }
  if (gflag != GRAD_SKIP) dgamma[j] = gflag == GRAD_ACC ? dgamma[j] + b : b;
  if (bflag != GRAD_SKIP) dbeta[j] = bflag == GRAD_ACC ? dbeta[j] + a : a;
  if (coef) {
    coef[j] = mode == ST_BATCH ? a * inv_m : 0.f;
    coef[C + j] = mode == ST_BATCH ? b * inv_m : 0.f;
  }
}

// ---------------------------------------------------------------------------------------
// Backward pass 2: dx = gamma inv_std (g - c1 - xhat c2); without batch statistics
// (global stats, plain Scale) c1 = c2 = 0 and x is not read.
// ---------------------------------------------------------------------------------------
template <int V, int DT>
__global__ void __launch_bounds__(256) bn_bwd_dx_k(const void* __restrict__ dy, const void* __restrict__ x,
                                                   const void* __restrict__ y, void* __restrict__ dx, long long R,
                                                   int C, int txlog, long long rps, const float* __restrict__ sa,
                                                   const float* __restrict__ sb, const float* __restrict__ factor,
                                                   float eps, int mode, int relu, const float* __restrict__ gamma,
                                                   const float* __restrict__ coef) {
  const Lane l = lane_of<V>(R, C, txlog, rps);
  if (!l.act) return;
  float mu[V], inv[V], gi[V], c1[V], c2[V];
  load_stats<V>(mode, sa, sb, factor, eps, l.c0, mu, inv);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    gi[j] = gamma ? gamma[l.c0 + j] * inv[j] : inv[j];
    c1[j] = mode == ST_BATCH ? coef[l.c0 + j] : 0.f;
    c2[j] = mode == ST_BATCH ? coef[C + l.c0 + j] : 0.f;
  }
  const bool batch = mode == ST_BATCH;
  auto load = [&](long long r, float* g, float* yv, float* xv) {
    const long long e = r * C + l.c0;
    ldx<V, DT>(dy, e, g);
    if (relu) ldx<V, DT>(y, e, yv);
    if (batch) ldx<V, DT>(x, e, xv);
  };
  auto finish = [&](long long r, float* g, const float* yv, const float* xv) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (relu) g[j] = yv[j] > 0.f ? g[j] : 0.f;
      g[j] = batch ? gi[j] * (g[j] - c1[j] - (xv[j] - mu[j]) * inv[j] * c2[j]) : g[j] * gi[j];
    }
    stx<V, DT>(dx, r * C + l.c0, g);
  };
  long long r = l.r0 + l.rl;
  for (; r + l.TY < l.r1; r += 2 * l.TY) {  // two rows (up to six loads) in flight per lane
    float g[2][V], yv[2][V], xv[2][V];
    load(r, g[0], yv[0], xv[0]);
    load(r + l.TY, g[1], yv[1], xv[1]);
    finish(r, g[0], yv[0], xv[0]);
    finish(r + l.TY, g[1], yv[1], xv[1]);
  }
  if (r < l.r1) {
    float g[V], yv[V], xv[V];
    load(r, g, yv, xv);
    finish(r, g, yv, xv);
  }
}

// General Scale / Bias over [outer][A][inner] with inner > 1 (not on the hot path):
// y = x s[a] + b[a], a = (e / inner) % A; s / b may be null.
template <int DT>
__global__ void __launch_bounds__(256) axis_scale_bias_k(const void* __restrict__ x, void* __restrict__ y,
                                                         long long n, long long A, long long inner,
                                                         const float* __restrict__ s, const float* __restrict__ b) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n; e += stride) {
    const long long a = (e / inner) % A;
    float f[1];
    ldx<1, DT>(x, e, f);
    f[0] = fmaf(f[0], s ? s[a] : 1.f, b ? b[a] : 0.f);
    stx<1, DT>(y, e, f);
  }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// lane width: 16-byte accesses need C % 8 == 0 and aligned tensors (views into a wider
// buffer may not be)
inline int pick_v(long long dt, long long C, const void* a, const void* b, const void* c, const void* d) {
  if (C % 8 != 0 || !al16(a) || !al16(b) || !al16(c) || !al16(d)) return 1;
  return dt ? 4 : 8;
}

inline bool bad_geom(long long R, long long C) { return R < 1 || C < 1 || C > 2147483647LL / 8; }

}  // namespace

#define SN_BN_DISPATCH(KERNEL, V, DT, ...)                                                              \
  do {                                                                                                  \
    const Plan p = make_plan(R, C, V);                                                                  \
    const dim3 grid((unsigned)p.gx, (unsigned)p.slabs);                                                 \
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

// Floats a partial workspace needs for R rows of C channels (the larger of the two lane widths).
long long sn_bn_part_floats(long long R, long long C, long long dt) {
  if (bad_geom(R, C)) return 0;
  long long s = make_plan(R, C, 1).slabs;
  if (C % 8 == 0) {
    const long long sv = make_plan(R, C, dt ? 4 : 8).slabs;
    if (sv > s) s = sv;
  }
  return s * 2 * C;
}

// mean / var / inv_std of x over the rows (var may be null); rmean != null also updates the
// running blobs.  part: workspace of part_floats floats.
int sn_bn_stats(const void* x, long long dt, long long R, long long C, float* part, long long part_floats, float eps,
                float* mean, float* var, float* inv, float* rmean, float* rvar, float* factor, float frac,
                float unbias, hipStream_t st) {
  if (bad_geom(R, C)) return 3;
  const int V = pick_v(dt, C, x, nullptr, nullptr, nullptr);
  const Plan pl = make_plan(R, C, V);
  if ((long long)pl.slabs * 2 * C > part_floats) return 3;
  float* pmean = part;
  float* pm2 = part + (long long)pl.slabs * C;
  SN_BN_DISPATCH(bn_stats_k, V, dt, x, R, (int)C, p.txlog, p.rps, pmean, pm2);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(bn_stats_finalize_k, dim3((unsigned)((C + FC - 1) / FC)), dim3(FC * FL), 0, st, pmean, pm2, pl.slabs,
                     R, pl.rps, (int)C, eps, mean, var, inv, rmean, rvar, factor, frac, unbias);
  return SN_CHECK_LAUNCH();
}

int sn_bn_fwd(const void* x, void* y, long long dt, long long R, long long C, const float* sa, const float* sb,
              const float* factor, float eps, long long mode, const float* gamma, const float* beta, long long relu,
              hipStream_t st) {
  if (bad_geom(R, C)) return 3;
  const int V = pick_v(dt, C, x, y, nullptr, nullptr);
  SN_BN_DISPATCH(bn_fwd_k, V, dt, x, y, R, (int)C, p.txlog, p.rps, sa, sb, factor, eps, (int)mode, gamma, beta,
                 (int)relu);
  return SN_CHECK_LAUNCH();
}

// Pass 1 and its finalize.  gflag / bflag: 0 skip, 1 store, 2 accumulate.  need_x = 0 skips
// the sum g xhat (x is not read; dgamma must be skipped and the statistics not the batch's).
int sn_bn_bwd_reduce(const void* dy, const void* x, const void* y, long long dt, long long R, long long C,
                     const float* sa, const float* sb, const float* factor, float eps, long long mode, long long relu,
                     long long need_x, float* part, long long part_floats, float* dgamma, long long gflag,
                     float* dbeta, long long bflag, float* coef, hipStream_t st) {
  if (bad_geom(R, C)) return 3;
  if (!need_x && (gflag != GRAD_SKIP || mode == ST_BATCH)) return 2;
  const int V = pick_v(dt, C, dy, need_x ? x : nullptr, relu ? y : nullptr, nullptr);
  const Plan pl = make_plan(R, C, V);
  if ((long long)pl.slabs * 2 * C > part_floats) return 3;
  SN_BN_DISPATCH(bn_bwd_red_k, V, dt, dy, x, y, R, (int)C, p.txlog, p.rps, sa, sb, factor, eps, (int)mode, (int)relu,
                 (int)need_x, part);
  if (hipGetLastError() != hipSuccess) return 1;
  hipLaunchKernelGGL(bn_bwd_finalize_k, dim3((unsigned)((C + FC - 1) / FC)), dim3(FC * FL), 0, st, part, pl.slabs, (int)C,
                     1.f / (float)R, (int)mode, (int)need_x, dgamma, (int)gflag, dbeta, (int)bflag, coef);
  return SN_CHECK_LAUNCH();
}

int sn_bn_bwd_dx(const void* dy, const void* x, const void* y, void* dx, long long dt, long long R, long long C,
                 const float* sa, const float* sb, const float* factor, float eps, long long mode, long long relu,
                 const float* gamma, const float* coef, hipStream_t st) {
  if (bad_geom(R, C)) return 3;
  if (mode == ST_BATCH && !coef) return 2;
  const int V = pick_v(dt, C, dy, dx, mode == ST_BATCH ? x : nullptr, relu ? y : nullptr);
  SN_BN_DISPATCH(bn_bwd_dx_k, V, dt, dy, x, y, dx, R, (int)C, p.txlog, p.rps, sa, sb, factor, eps, (int)mode,
                 (int)relu, gamma, coef);
  return SN_CHECK_LAUNCH();
}

int sn_axis_scale_bias(const void* x, void* y, long long n, long long A, long long inner, const float* s,
                       const float* b, long long dt, hipStream_t st) {
  if (n < 1 || A < 1 || inner < 1) return 3;
  const dim3 grid((unsigned)sn_blocks(n, 256, 4096));
  if (dt)
    hipLaunchKernelGGL(axis_scale_bias_k<1>, grid, dim3(256), 0, st, x, y, n, A, inner, s, b);
  else
    hipLaunchKernelGGL(axis_scale_bias_k<0>, grid, dim3(256), 0, st, x, y, n, A, inner, s, b);
  return SN_CHECK_LAUNCH();
}

}  // extern "C"
