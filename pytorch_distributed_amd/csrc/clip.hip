// Global-norm gradient clipping for gfx950: the clip coefficient of torch.nn.utils.clip_grad_norm_
// produced on the device in ONE launch, for the fused SGD to multiply into its gradient scale.
//
//   grad_clip : one workgroup per row of a block table (BlkRow, as seg_norms): sum g^2 of the chunk
//               in double, fixed-order block reduction, one double per block into a slab. The last
//               block to arrive (agent-scope counter) sums the slab -- each of its 256 threads a
//               fixed strided share in ascending order, then a fixed tree: the bits depend on the
//               block count alone, not on which block came last -- and publishes
//                 out[0] = (float)(inv * sqrt(sum))          the unscaled norm before clipping
//                 out[1] = inv * min(1, max_norm / (out[0] + 1e-6f))   in IEEE single precision
//               with inv = inv_in[0] (1/loss-scale of amp_scan) or 1. A NaN norm gives a NaN
//               coefficient (torch's clamp propagates it), an infinite one 0; with found_inf set
//               out[1] = inv (the SGD skips that step anyway).
//
// Elements of g outside every row are never read. The hand-off is bn_stats_kernel's (bn.hip): the
// slab entry is stored write-through (relaxed agent-scope store), drained by the storing lane
// (vmcnt(0)), then that lane arrives on the counter; the last arriver runs an agent-scope acquire
// before any lane of its block loads the slab, and resets the counter, so the launch needs no
// memset and replays inside a HIP graph. No float atomics: runs repeat bit for bit.
#include "common.h"
#include "pda_api.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void grad_clip_kernel(const float* __restrict__ g,
                                                       const BlkRow* __restrict__ blks, double* slab,
                                                       int* cnt, float max_norm,
                                                       const float* __restrict__ inv_in,
                                                       const float* __restrict__ found_inf,
                                                       float* __restrict__ out) {
  __shared__ double red[NT / 64];
  __shared__ int s_last;
  const BlkRow b = blks[blockIdx.x];
  double s = 0.0;
  const int nv = b.count >> 2;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g + b.first);
  // a full chunk is U 16-byte loads per lane: all issued before the first use (one dependent
  // round per block instead of U), accumulated in ascending order; a lane past the end adds +0
  constexpr int U = FLAT_CHUNK / (4 * NT);
  f32x4 gv[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int i = threadIdx.x + u * NT;
    gv[u] = i < nv ? g4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (double)gv[u][e] * (double)gv[u][e];
  if ((int)threadIdx.x < (b.count & 3)) {   // ragged tail of a tensor's last chunk
    const float gv = g[b.first + (nv << 2) + threadIdx.x];
    s += (double)gv * (double)gv;
  }
  const double tot = block_sum_f64<NT>(s, red);
  if (threadIdx.x == 0) {
    // publish: write-through store, drained by this lane before its arrival (bn.hip, the hand-off)
    __hip_atomic_store(slab + blockIdx.x, tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = old == (int)gridDim.x - 1;
    if (s_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // reset
    }
  }
  __syncthreads();   // (also: every wave has read red[] before the second block_sum_f64 writes it)
  if (!s_last) return;
  double a = 0.0;
  for (int k = threadIdx.x; k < (int)gridDim.x; k += NT) a += slab[k];   // ascending, fixed share
  const double sum = block_sum_f64<NT>(a, red);
  if (threadIdx.x == 0) {
    const float inv = inv_in ? inv_in[0] : 1.f;
    const float norm = (float)((double)inv * sqrt(sum));
    float coef = max_norm / (norm + 1e-6f);
    if (coef > 1.f) coef = 1.f;   // a NaN compares false and stays (torch.clamp), unlike fminf
    out[0] = norm;
    out[1] = (found_inf && found_inf[0] != 0.f) ? inv : inv * coef;
  }
}

}  // namespace

extern "C" {

int pda_clip_check(const BlkRow* blks, int nblk, long long n, float max_norm) {
  if (nblk < 1 || n < 0 || !blks) return -1;
  if (!(max_norm > 0.f) || !(max_norm <= 3.4028235e38f)) return -5;
  bool ascending = true;
  long long prev_end = 0;
  for (int i = 0; i < nblk; ++i) {
    const BlkRow& b = blks[i];
    if (b.first < 0 || (b.first & 3)) return -2;
    if (b.count <= 0 || b.count > FLAT_CHUNK) return -6;
    if (b.first > n || b.count > n - b.first) return -3;
    ascending &= b.first >= prev_end;
    prev_end = b.first + b.count;
  }
  if (!ascending) {   // rows in group order: no element may count twice
    std::vector<std::pair<long long, int>> span(nblk);
    for (int i = 0; i < nblk; ++i) span[i] = {blks[i].first, blks[i].count};
    std::sort(span.begin(), span.end());
    for (int i = 1; i < nblk; ++i)
      if (span[i - 1].first + span[i - 1].second > span[i].first) return -4;
  }
  return 0;
}

int pda_grad_clip(const float* g, long long n, const void* blk_dev, const void* blk_host, int nblk,
                  double* slab, int* cnt, float max_norm, const float* inv_in,
                  const float* found_inf, float* out, hipStream_t st) {
  const int rc = pda_clip_check((const BlkRow*)blk_host, nblk, n, max_norm);
  if (rc) return rc;
  if (!g || !blk_dev || !slab || !cnt || !out) return -1;
  TRACKED_LAUNCH(grad_clip_kernel, dim3(nblk), dim3(NT), 0, st, g, (const BlkRow*)blk_dev, slab, cnt,
                 max_norm, inv_in, found_inf, out);
  return (int)hipGetLastError();
}

}  // extern "C"
