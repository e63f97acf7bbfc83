// Segmented optimizer kernels for gfx950: SGD with per-tensor hyper-parameters over the flat buffers.
//
// A *segment* is one parameter tensor's element range [off, off + numel) of the flat parameter
// buffer; its learning rate, momentum, weight decay, Nesterov bit and LARS trust coefficient live in
// one row of a device table (SegRow), so parameter groups, frozen tensors (no row) and schedulers
// (a re-uploaded table) need no kernel arguments. A host-built block table (BlkRow) gives every
// workgroup one chunk of at most FLAT_CHUNK (common.h) elements of one segment.
//
//   seg_norms : per chunk, sum p^2 and sum g^2 in double, block_sum_f64 (common.h), two doubles
//               per block into a slab (launched only when some segment has a trust coefficient)
//   sgd_seg   : q = LARS trust ratio from the segment's slab entries summed in ascending block
//               order (1 without LARS); d = q (g inv + wd p); b = mom b + d; p -= lr (b | d + mom b);
//               16-bit shadow write; the whole launch is skipped on found_inf (as sgd_flat)
//
// Elements of p, g, buf and the shadow outside every segment are neither read nor written. The
// launchers validate both tables on the host (pda_seg_check); the kernels then trust them.
#include "common.h"
#include "pda_api.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void seg_norms_kernel(const float* __restrict__ p,
                                                       const float* __restrict__ g,
                                                       const SegRow* __restrict__ segs,
                                                       const BlkRow* __restrict__ blks,
                                                       double* __restrict__ slab) {
  const BlkRow b = blks[blockIdx.x];
  if (!(segs[b.seg].trust > 0.f)) return;
  double sp = 0.0, sg = 0.0;
  const int nv = b.count >> 2;
  const f32x4* p4 = reinterpret_cast<const f32x4*>(p + b.first);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g + b.first);
  for (int i = threadIdx.x; i < nv; i += NT) {
    const f32x4 pv = p4[i], gv = g4[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sp += (double)pv[e] * (double)pv[e];
      sg += (double)gv[e] * (double)gv[e];
    }
  }
  if ((int)threadIdx.x < (b.count & 3)) {   // ragged tail of the segment's last chunk
    const long long i = b.first + (nv << 2) + threadIdx.x;
    sp += (double)p[i] * (double)p[i];
    sg += (double)g[i] * (double)g[i];
  }
  __shared__ double red[2][NT / 64];
  const double tp = block_sum_f64<NT>(sp, red[0]), tg = block_sum_f64<NT>(sg, red[1]);
  if (threadIdx.x == 0) {
    slab[2 * (size_t)blockIdx.x] = tp;
    slab[2 * (size_t)blockIdx.x + 1] = tg;
  }
}

// one element of the update; returns the new p, updates b in place
__device__ __forceinline__ float sgd_elem(float pv, float gv, float& bv, float inv, float q, float lr,
                                          float momentum, float wd, bool init, bool nesterov) {
  const float d = q * (gv * inv + wd * pv);
  const float b = init ? momentum * bv + d : d;
  bv = b;
  const float step = nesterov ? d + momentum * b : b;
  return pv - lr * step;
}

// flags: bit0 = momentum buffer initialised (else buf = d), bit1 = write shadow
__global__ __launch_bounds__(NT) void sgd_seg_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ buf, u16* __restrict__ shadow,
                                                     const SegRow* __restrict__ segs,
                                                     const BlkRow* __restrict__ blks,
                                                     const double* __restrict__ slab,
                                                     const float* __restrict__ inv_scale_src,
                                                     const float* __restrict__ found_inf, int flags,
                                                     int dt) {
  if (found_inf && found_inf[0] != 0.f) return;
  const float inv = inv_scale_src ? inv_scale_src[0] : 1.f;   // published by amp_scan_kernel
  const BlkRow b = blks[blockIdx.x];
  const SegRow s = segs[b.seg];
  float q = 1.f;
  if (s.trust > 0.f) {
    __shared__ float s_q;
    if (threadIdx.x == 0) {
      double sp = 0.0, sg = 0.0;
      for (int k = 0; k < s.nblk; ++k) {   // ascending block order: every block gets the same bits
        sp += slab[2 * (size_t)(s.blk0 + k)];
        sg += slab[2 * (size_t)(s.blk0 + k) + 1];
      }
      const double wn = sqrt(sp), gn = (double)inv * sqrt(sg);
      s_q = (wn > 0.0 && gn > 0.0)
                ? (float)((double)s.trust * wn / (gn + (double)s.wd * wn + (double)s.eps))
                : 1.f;
    }
    __syncthreads();
    q = s_q;
  }
  const bool init = flags & 1, nesterov = s.flags & 1;
  const int nv = b.count >> 2;
  f32x4* p4 = reinterpret_cast<f32x4*>(p + b.first);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g + b.first);
  f32x4* b4 = reinterpret_cast<f32x4*>(buf + b.first);
  for (int i = threadIdx.x; i < nv; i += NT) {
    f32x4 pv = p4[i];
    const f32x4 gv = g4[i];
    f32x4 bv;
    if (init) bv = b4[i];   // (a first step never reads the stale buffer)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float be = init ? bv[e] : 0.f;
      pv[e] = sgd_elem(pv[e], gv[e], be, inv, q, s.lr, s.momentum, s.wd, init, nesterov);
      bv[e] = be;
    }
    p4[i] = pv;
    b4[i] = bv;
    if (flags & 2) {
      u16 h[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) h[e] = cvt16_rt(pv[e], dt);
      reinterpret_cast<uint2*>(shadow + b.first)[i] = *reinterpret_cast<uint2*>(h);
    }
  }
  if ((int)threadIdx.x < (b.count & 3)) {   // ragged tail of the segment's last chunk
    const long long i = b.first + (nv << 2) + threadIdx.x;
    float be = init ? buf[i] : 0.f;
    const float pn = sgd_elem(p[i], g[i], be, inv, q, s.lr, s.momentum, s.wd, init, nesterov);
    p[i] = pn;
    buf[i] = be;
    if (flags & 2) shadow[i] = cvt16_rt(pn, dt);
  }
}

}  // namespace

extern "C" {

int pda_seg_check(const SegRow* segs, int nseg, const BlkRow* blks, int nblk, long long n) {
  if (nseg < 0 || nblk < 0 || n < 0 || (nseg && !segs) || (nblk && !blks)) return -1;
  std::vector<std::pair<long long, long long>> span;
  span.reserve(nseg);
  long long next_blk = 0;
  for (int i = 0; i < nseg; ++i) {
    const SegRow& s = segs[i];
    if (s.off < 0 || (s.off & 3)) return -2;
    if (s.numel <= 0 || s.off > n || s.numel > n - s.off) return -3;
    const float h[5] = {s.lr, s.momentum, s.wd, s.trust, s.eps};
    for (float v : h)
      if (!(v >= 0.f) || !(v <= 3.4028235e38f)) return -5;
    span.emplace_back(s.off, s.numel);
    // the segment's blocks follow those of the segment before it, ascending and gap-free
    if (s.blk0 != next_blk || s.nblk <= 0 || s.nblk > nblk - s.blk0) return -6;
    long long at = s.off;
    for (int k = 0; k < s.nblk; ++k) {
      const BlkRow& b = blks[s.blk0 + k];
      if (b.seg != i || b.first != at || b.count <= 0 || b.count > FLAT_CHUNK) return -6;
      if (k + 1 < s.nblk && (b.count & 3)) return -6;   // only a segment's last chunk is ragged
      at += b.count;
    }
    if (at != s.off + s.numel) return -6;
    next_blk += s.nblk;
  }
  if (next_blk != nblk) return -6;
  std::sort(span.begin(), span.end());
  for (size_t i = 1; i < span.size(); ++i)
    if (span[i - 1].first + span[i - 1].second > span[i].first) return -4;
  return 0;
}

int pda_seg_chunk() { return FLAT_CHUNK; }

int pda_seg_norms(const float* p, const float* g, long long n, const void* seg_dev, const void* blk_dev,
                  const void* seg_host, const void* blk_host, int nseg, int nblk, double* slab,
                  hipStream_t st) {
  const int rc = pda_seg_check((const SegRow*)seg_host, nseg, (const BlkRow*)blk_host, nblk, n);
  if (rc) return rc;
  if (nblk == 0) return 0;
  if (!p || !g || !seg_dev || !blk_dev || !slab) return -1;
  TRACKED_LAUNCH(seg_norms_kernel, dim3(nblk), dim3(NT), 0, st, p, g, (const SegRow*)seg_dev,
                 (const BlkRow*)blk_dev, slab);
  return (int)hipGetLastError();
}

int pda_sgd_seg(float* p, const float* g, float* buf, void* shadow, long long n, const void* seg_dev,
                const void* blk_dev, const void* seg_host, const void* blk_host, int nseg, int nblk,
                const double* slab, const float* scale, const float* found_inf, int flags, int dt,
                hipStream_t st) {
  const int rc = pda_seg_check((const SegRow*)seg_host, nseg, (const BlkRow*)blk_host, nblk, n);
  if (rc) return rc;
  if (nblk == 0) return 0;
  if (!p || !g || !buf || !seg_dev || !blk_dev || ((flags & 2) && !shadow)) return -1;
  if (!slab)   // a trust coefficient needs the norms of seg_norms
    for (int i = 0; i < nseg; ++i)
      if (((const SegRow*)seg_host)[i].trust > 0.f) return -1;
  TRACKED_LAUNCH(sgd_seg_kernel, dim3(nblk), dim3(NT), 0, st, p, g, buf, (u16*)shadow,
                 (const SegRow*)seg_dev, (const BlkRow*)blk_dev, slab, scale, found_inf, flags, dt);
  return (int)hipGetLastError();
}

}  // extern "C"
