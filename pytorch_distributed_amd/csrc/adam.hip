// Adaptive optimizer kernels for gfx950: AdamW and LAMB over the flat buffers, per segment.
//
// The geometry is optim.hip's: one SegRow per parameter tensor, one BlkRow (at most FLAT_CHUNK
// elements of one segment) per workgroup of 256 threads. The hyper-parameters live in a plain device
// float table, ADAM_HYPER floats per segment (the H_* slots below); the bias corrections in a second
// one, two floats per segment, written by adam_tick. Per segment, with inv the device scalar (AMP's
// 1/scale, the clip launch's out[1], or 1) and t = applied steps + 1:
//
//   g' = g inv;  m += (1 - b1) (g' - m);  v += (1 - b2) (g'^2 - v)     (= b m + (1 - b) x)
//   c1 = 1 / (1 - b1^t);  c2 = 1 / sqrt(1 - b2^t);  a = (m c1) / (sqrt(v) c2 + eps)
//   AdamW: p = p (1 - lr wd) - lr a
//   LAMB : u = a + wd p;  r = |p| / |u| if |p| > 0 and |u| > 0 else 1;  p = p - lr r u
//
//   adam_tick    : one block. Every thread reads the step counter t0; after a barrier thread 0 stores
//                  t0 + 1; the threads stride over the segments and write (c1, c2), evaluated in
//                  double from the betas (kept as float hi + lo pairs: 0.999f alone is 1.3e-5 off in
//                  1 - b2) and rounded to float once. The counter advances only on applied steps.
//   adamw_seg    : the whole AdamW step in one launch: 16 B per lane on p, g, m, v, all of a chunk's
//                  loads issued before the first use, the 16-bit shadow written beside p.
//   lamb_moments : phase A. m and v are updated and stored, u is formed in f32, and the chunk's
//                  sum p^2 and sum u^2 go, in double through block_sum_f64, into a slab of two doubles
//                  per block (no float atomics, no arrival counter).
//   lamb_apply   : phase B. Thread 0 sums its segment's slab entries in ascending block order (every
//                  block of a segment gets the same bits), forms r in double and rounds it once; u
//                  is recomputed from the stored m, v and the not yet updated p with lamb_dir(), the
//                  function phase A used, so both phases see one u; p and the shadow are written.
//                  Segments with the lamb slot 0 run both phases with r = 1 and add nothing to the slab.
//
// Every kernel returns at once when found_inf[0] != 0: a skipped step leaves p, m, v, the shadow,
// the bias table and the counter bit for bit. Elements outside every segment are neither read nor
// written. The launchers validate the tables on the host (pda_seg_check, pda_adam_check) before
// anything is launched; the kernels then trust them. The file is compiled without FMA contraction:
// the fused operations are the ones written as fmaf.
#include "common.h"
#include "pda_api.h"

#include <cmath>

namespace {

constexpr int NT = 256;
constexpr int U = FLAT_CHUNK / (4 * NT);   // 16-byte pieces per lane of a full chunk
static_assert(U * 4 * NT == FLAT_CHUNK, "a chunk is a whole number of 16-byte pieces per lane");

// slots of one segment's row of the hyper-parameter table
enum { H_LR, H_B1, H_B2, H_EPS, H_WD, H_LAMB, H_OMB1, H_OMB2, H_B1LO, H_B2LO, ADAM_HYPER = 12 };

struct Hyper {
  float lr, eps, wd, omb1, omb2, c1, c2;
  bool lamb;
};

__device__ __forceinline__ Hyper load_hyper(const float* __restrict__ hyper,
                                            const float* __restrict__ bias, int seg) {
  const float* h = hyper + (size_t)ADAM_HYPER * seg;
  return {h[H_LR], h[H_EPS], h[H_WD], h[H_OMB1], h[H_OMB2], bias[2 * (size_t)seg],
          bias[2 * (size_t)seg + 1], h[H_LAMB] != 0.f};
}

// both moments of one element, in place (the lerp form: the rounded 1 - b weighs only the change)
__device__ __forceinline__ void adam_moments(float g, float inv, float& m, float& v, const Hyper& h) {
  const float gs = g * inv;
  m = fmaf(h.omb1, gs - m, m);
  v = fmaf(h.omb2, gs * gs - v, v);
}

// a = (m c1) / (sqrt(v) c2 + eps)
__device__ __forceinline__ float adam_dir(float m, float v, const Hyper& h) {
  return (m * h.c1) / fmaf(sqrtf(v), h.c2, h.eps);
}

// u = a + wd p: phase A sums its square, phase B applies it -- one function, one u
__device__ __forceinline__ float lamb_dir(float p, float m, float v, const Hyper& h) {
  return fmaf(h.wd, p, adam_dir(m, v, h));
}

// p (1 - lr wd) - lr a, with the decay folded into an FMA on p (1 - lr wd is never rounded)
__device__ __forceinline__ float adamw_p(float p, float m, float v, const Hyper& h) {
  return fmaf(-h.lr, adam_dir(m, v, h), fmaf(-(h.lr * h.wd), p, p));
}

__device__ __forceinline__ void store_shadow4(u16* shadow, long long first, int i, const f32x4& pv,
                                              int dt) {
  u16 s[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) s[e] = cvt16_rt(pv[e], dt);
  reinterpret_cast<uint2*>(shadow + first)[i] = *reinterpret_cast<uint2*>(s);
}

#define Z4 (f32x4{0.f, 0.f, 0.f, 0.f})

__global__ __launch_bounds__(NT) void adam_tick_kernel(const float* __restrict__ hyper, int nseg,
                                                       int* step, float* __restrict__ bias,
                                                       const float* __restrict__ found_inf) {
  if (found_inf && found_inf[0] != 0.f) return;
  const int t = step[0] + 1;
  __syncthreads();   // every thread holds t0 before thread 0 overwrites it
  if (threadIdx.x == 0) step[0] = t;
  for (int s = threadIdx.x; s < nseg; s += NT) {
    const float* h = hyper + (size_t)ADAM_HYPER * s;
    const double b1 = (double)h[H_B1] + (double)h[H_B1LO], b2 = (double)h[H_B2] + (double)h[H_B2LO];
    bias[2 * (size_t)s] = (float)(1.0 / (1.0 - pow(b1, (double)t)));
    bias[2 * (size_t)s + 1] = (float)(1.0 / sqrt(1.0 - pow(b2, (double)t)));
  }
}

// flags: bit1 = write shadow (as sgd_seg)
__global__ __launch_bounds__(NT) void adamw_seg_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                       float* __restrict__ m, float* __restrict__ v,
                                                       u16* __restrict__ shadow,
                                                       const BlkRow* __restrict__ blks,
                                                       const float* __restrict__ hyper,
                                                       const float* __restrict__ bias,
                                                       const float* __restrict__ inv_src,
                                                       const float* __restrict__ found_inf, int flags,
                                                       int dt) {
  if (found_inf && found_inf[0] != 0.f) return;
  const float inv = inv_src ? inv_src[0] : 1.f;
  const BlkRow b = blks[blockIdx.x];
  const Hyper h = load_hyper(hyper, bias, b.seg);
  const int nv = b.count >> 2;
  f32x4* p4 = reinterpret_cast<f32x4*>(p + b.first);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g + b.first);
  f32x4* m4 = reinterpret_cast<f32x4*>(m + b.first);
  f32x4* v4 = reinterpret_cast<f32x4*>(v + b.first);
  // 4 U loads per lane, all in flight before the first use: one dependent round per block
  f32x4 pv[U], gv[U], mv[U], vv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = threadIdx.x + u * NT;
    const bool in = i < nv;
    pv[u] = in ? p4[i] : Z4;
    gv[u] = in ? g4[i] : Z4;
    mv[u] = in ? m4[i] : Z4;
    vv[u] = in ? v4[i] : Z4;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = threadIdx.x + u * NT;
    if (i >= nv) break;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float me = mv[u][e], ve = vv[u][e];
      adam_moments(gv[u][e], inv, me, ve, h);
      mv[u][e] = me;
      vv[u][e] = ve;
      pv[u][e] = adamw_p(pv[u][e], me, ve, h);
    }
    p4[i] = pv[u];
    m4[i] = mv[u];
    v4[i] = vv[u];
    if (flags & 2) store_shadow4(shadow, b.first, i, pv[u], dt);
  }
  if ((int)threadIdx.x < (b.count & 3)) {   // ragged tail of the segment's last chunk
    const long long i = b.first + (nv << 2) + threadIdx.x;
    float me = m[i], ve = v[i];
    adam_moments(g[i], inv, me, ve, h);
    const float pn = adamw_p(p[i], me, ve, h);
    p[i] = pn;
    m[i] = me;
    v[i] = ve;
    if (flags & 2) shadow[i] = cvt16_rt(pn, dt);
  }
}

__global__ __launch_bounds__(NT) void lamb_moments_kernel(const float* __restrict__ p,
                                                          const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          const BlkRow* __restrict__ blks,
                                                          const float* __restrict__ hyper,
                                                          const float* __restrict__ bias,
                                                          double* __restrict__ slab,
                                                          const float* __restrict__ inv_src,
                                                          const float* __restrict__ found_inf) {
  if (found_inf && found_inf[0] != 0.f) return;
  const float inv = inv_src ? inv_src[0] : 1.f;
  const BlkRow b = blks[blockIdx.x];
  const Hyper h = load_hyper(hyper, bias, b.seg);
  const int nv = b.count >> 2;
  const f32x4* p4 = reinterpret_cast<const f32x4*>(p + b.first);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g + b.first);
  f32x4* m4 = reinterpret_cast<f32x4*>(m + b.first);
  f32x4* v4 = reinterpret_cast<f32x4*>(v + b.first);
  f32x4 pv[U], gv[U], mv[U], vv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = threadIdx.x + u * NT;
    const bool in = i < nv;
    pv[u] = in ? p4[i] : Z4;
    gv[u] = in ? g4[i] : Z4;
    mv[u] = in ? m4[i] : Z4;
    vv[u] = in ? v4[i] : Z4;
  }
  double sp = 0.0, su = 0.0;   // ascending per lane; a segment without LAMB sums nothing
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = threadIdx.x + u * NT;
    if (i >= nv) break;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float me = mv[u][e], ve = vv[u][e];
      adam_moments(gv[u][e], inv, me, ve, h);
      mv[u][e] = me;
      vv[u][e] = ve;
      if (h.lamb) {
        const float pe = pv[u][e], ue = lamb_dir(pe, me, ve, h);
        sp += (double)pe * (double)pe;
        su += (double)ue * (double)ue;
      }
    }
    m4[i] = mv[u];
    v4[i] = vv[u];
  }
  if ((int)threadIdx.x < (b.count & 3)) {   // ragged tail of the segment's last chunk
    const long long i = b.first + (nv << 2) + threadIdx.x;
    float me = m[i], ve = v[i];
    adam_moments(g[i], inv, me, ve, h);
    m[i] = me;
    v[i] = ve;
    if (h.lamb) {
      const float pe = p[i], ue = lamb_dir(pe, me, ve, h);
      sp += (double)pe * (double)pe;
      su += (double)ue * (double)ue;
    }
  }
  if (!h.lamb) return;   // (block-uniform: one segment per block)
  __shared__ double red[2][NT / 64];
  const double tp = block_sum_f64<NT>(sp, red[0]), tu = block_sum_f64<NT>(su, red[1]);
  if (threadIdx.x == 0) {
    slab[2 * (size_t)blockIdx.x] = tp;
    slab[2 * (size_t)blockIdx.x + 1] = tu;
  }
}

__global__ __launch_bounds__(NT) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                        const float* __restrict__ v,
                                                        u16* __restrict__ shadow,
                                                        const SegRow* __restrict__ segs,
                                                        const BlkRow* __restrict__ blks,
                                                        const float* __restrict__ hyper,
                                                        const float* __restrict__ bias,
                                                        const double* __restrict__ slab,
                                                        const float* __restrict__ found_inf, int flags,
                                                        int dt) {
  if (found_inf && found_inf[0] != 0.f) return;
  const BlkRow b = blks[blockIdx.x];
  const Hyper h = load_hyper(hyper, bias, b.seg);
  const int nv = b.count >> 2;
  f32x4* p4 = reinterpret_cast<f32x4*>(p + b.first);
  const f32x4* m4 = reinterpret_cast<const f32x4*>(m + b.first);
  const f32x4* v4 = reinterpret_cast<const f32x4*>(v + b.first);
  f32x4 pv[U], mv[U], vv[U];   // in flight while thread 0 walks the slab
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = threadIdx.x + u * NT;
    const bool in = i < nv;
    pv[u] = in ? p4[i] : Z4;
    mv[u] = in ? m4[i] : Z4;
    vv[u] = in ? v4[i] : Z4;
  }
  float r = 1.f;
  if (h.lamb) {
    __shared__ float s_r;
    if (threadIdx.x == 0) {
      const SegRow s = segs[b.seg];
      double sp = 0.0, su = 0.0;
      for (int k = 0; k < s.nblk; ++k) {   // ascending block order: every block gets the same bits
        sp += slab[2 * (size_t)(s.blk0 + k)];
        su += slab[2 * (size_t)(s.blk0 + k) + 1];
      }
      s_r = (sp > 0.0 && su > 0.0) ? (float)(sqrt(sp) / sqrt(su)) : 1.f;
    }
    __syncthreads();
    r = s_r;
  }
  const float nlr = -(h.lr * r);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = threadIdx.x + u * NT;
    if (i >= nv) break;
#pragma unroll
    for (int e = 0; e < 4; ++e)
      pv[u][e] = fmaf(nlr, lamb_dir(pv[u][e], mv[u][e], vv[u][e], h), pv[u][e]);
    p4[i] = pv[u];
    if (flags & 2) store_shadow4(shadow, b.first, i, pv[u], dt);
  }
  if ((int)threadIdx.x < (b.count & 3)) {   // ragged tail of the segment's last chunk
    const long long i = b.first + (nv << 2) + threadIdx.x;
    const float pe = p[i], pn = fmaf(nlr, lamb_dir(pe, m[i], v[i], h), pe);
    p[i] = pn;
    if (flags & 2) shadow[i] = cvt16_rt(pn, dt);
  }
}

inline bool finite_nonneg(float x) { return x >= 0.f && x <= 3.4028235e38f; }

// tables first (pda_seg_check), then the hyper-parameters; lamb: 0 = no segment may have LAMB on,
// 1 = a segment with LAMB on needs the slab
int adam_check(const void* seg_host, const void* blk_host, int nseg, int nblk, long long n,
               const float* hyper_host, const void* slab, int lamb) {
  int rc = pda_seg_check((const SegRow*)seg_host, nseg, (const BlkRow*)blk_host, nblk, n);
  if (rc) return rc;
  if ((rc = pda_adam_check(hyper_host, nseg))) return rc;
  for (int i = 0; i < nseg; ++i)
    if (hyper_host[(size_t)ADAM_HYPER * i + H_LAMB] != 0.f) {
      if (!lamb) return -11;
      if (!slab) return -12;
    }
  return 0;
}

}  // namespace

extern "C" {

int pda_adam_floats() { return ADAM_HYPER; }

int pda_adam_check(const float* hyper, int nseg) {
  if (nseg < 0 || (nseg && !hyper)) return -1;
  for (int i = 0; i < nseg; ++i) {
    const float* h = hyper + (size_t)ADAM_HYPER * i;
    if (!finite_nonneg(h[H_LR])) return -7;
    for (int k = 0; k < 2; ++k) {
      // the beta as the tick sees it (hi + lo), and the rounded 1 - beta the moments use
      const double b = (double)h[H_B1 + k] + (double)h[H_B1LO + k];
      if (!(b >= 0.0) || !(b < 1.0) || !(h[H_B1 + k] < 1.f)) return -8;
      if (!(h[H_OMB1 + k] > 0.f) || !(h[H_OMB1 + k] <= 1.f)) return -8;
    }
    if (!finite_nonneg(h[H_EPS])) return -9;
    if (!finite_nonneg(h[H_WD])) return -10;
  }
  return 0;
}

int pda_adam_tick(const float* hyper_dev, const float* hyper_host, int nseg, int* step, float* bias,
                  const float* found_inf, hipStream_t st) {
  const int rc = pda_adam_check(hyper_host, nseg);
  if (rc) return rc;
  if (!hyper_dev || !step || !bias) return -1;
  TRACKED_LAUNCH(adam_tick_kernel, dim3(1), dim3(NT), 0, st, hyper_dev, nseg, step, bias, found_inf);
  return (int)hipGetLastError();
}

int pda_adamw_seg(float* p, const float* g, float* m, float* v, void* shadow, long long n,
                  const void* seg_dev, const void* blk_dev, const void* seg_host, const void* blk_host,
                  int nseg, int nblk, const float* hyper_dev, const float* hyper_host,
                  const float* bias, const float* scale, const float* found_inf, int flags, int dt,
                  hipStream_t st) {
  const int rc = adam_check(seg_host, blk_host, nseg, nblk, n, hyper_host, nullptr, 0);
  if (rc) return rc;
  if (nblk == 0) return 0;
  if (!p || !g || !m || !v || !seg_dev || !blk_dev || !hyper_dev || !bias ||
      ((flags & 2) && !shadow))
    return -1;
  TRACKED_LAUNCH(adamw_seg_kernel, dim3(nblk), dim3(NT), 0, st, p, g, m, v, (u16*)shadow,
                 (const BlkRow*)blk_dev, hyper_dev, bias, scale, found_inf, flags, dt);
  return (int)hipGetLastError();
}

int pda_lamb_moments(const float* p, const float* g, float* m, float* v, long long n,
                     const void* seg_dev, const void* blk_dev, const void* seg_host,
                     const void* blk_host, int nseg, int nblk, const float* hyper_dev,
                     const float* hyper_host, const float* bias, double* slab, const float* scale,
                     const float* found_inf, hipStream_t st) {
  const int rc = adam_check(seg_host, blk_host, nseg, nblk, n, hyper_host, slab, 1);
  if (rc) return rc;
  if (nblk == 0) return 0;
  if (!p || !g || !m || !v || !seg_dev || !blk_dev || !hyper_dev || !bias) return -1;
  TRACKED_LAUNCH(lamb_moments_kernel, dim3(nblk), dim3(NT), 0, st, p, g, m, v, (const BlkRow*)blk_dev,
                 hyper_dev, bias, slab, scale, found_inf);
  return (int)hipGetLastError();
}

int pda_lamb_apply(float* p, const float* m, const float* v, void* shadow, long long n,
                   const void* seg_dev, const void* blk_dev, const void* seg_host,
                   const void* blk_host, int nseg, int nblk, const float* hyper_dev,
                   const float* hyper_host, const float* bias, const double* slab,
                   const float* found_inf, int flags, int dt, hipStream_t st) {
  const int rc = adam_check(seg_host, blk_host, nseg, nblk, n, hyper_host, slab, 1);
  if (rc) return rc;
  if (nblk == 0) return 0;
  if (!p || !m || !v || !seg_dev || !blk_dev || !hyper_dev || !bias || ((flags & 2) && !shadow))
    return -1;
  TRACKED_LAUNCH(lamb_apply_kernel, dim3(nblk), dim3(NT), 0, st, p, m, v, (u16*)shadow,
                 (const SegRow*)seg_dev, (const BlkRow*)blk_dev, hyper_dev, bias, slab, found_inf,
                 flags, dt);
  return (int)hipGetLastError();
}

}  // extern "C"
