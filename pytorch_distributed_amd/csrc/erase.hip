// Random erasing for gfx950: torchvision's RandomErasing(p, scale, ratio, value=0) on a finished,
// normalised batch, just before the batch mixing (mix.hip).
//
//   erase_draw  : one thread per sample writes the sample's box (y1, y2, x1, x2), half-open, into an
//                 int32 table [B][4]; all zeros when the sample is left alone. The arithmetic is
//                 double, as the crop draw of augment.hip, and this file is compiled without FMA
//                 contraction for the same reason: the integers must be those of a float64 Python
//                 evaluation of the same expressions (erase.py draw_erase, tests/erase_refs.py).
//                 The uniforms are counter-based (batch_image.h) on a stream of their own:
//                   bkey = hash32(hash32(hash32(hash32(seed*97 + 0x455241) ^ rank) ^ epoch) ^ step)  (host)
//                   skey = counter_subkey(bkey, b),  b = position in the batch
//                   u(k) = counter_u01(skey, k)
//                 u(0) is the gate (erase if u(0) < p); attempt a = 0..9 draws area 1+4a, log-ratio
//                 2+4a, row 3+4a, column 4+4a and is accepted when h < S and w < S (strict, as
//                 torchvision). Ten refusals leave the image alone.
//   batch_erase : in place, pixels inside a sample's box become +0.0 in all three channels. The
//                 table is device-produced, so each box is clamped to [0, S] here and an empty one
//                 skipped. Layouts as batch_mix: the stem's 2x2 space-to-depth [B, S/2, S/2, 16]
//                 (f32 / bf16 / f16; batch_image.h) and NCHW f32. Only the boxes are visited: a lane owns one 16-B chunk that touches
//                 the box, stores it whole when every element of it lies inside, and otherwise
//                 stores the inside elements one by one. Nothing is loaded, so nothing outside the
//                 box (pixels, padding slots, the memory around the tensor) can change a bit; no LDS,
//                 no atomics.
#include <cmath>

#include "batch_image.h"
#include "pda_api.h"

namespace {

constexpr int NT = 256;

struct EraseDraw {
  uint32_t bkey;
  int S;
  double p, s0, s1, l0, l1;
};

__global__ __launch_bounds__(NT) void erase_draw_kernel(int B, EraseDraw d, int* __restrict__ boxes) {
  const int b = blockIdx.x * NT + threadIdx.x;
  if (b >= B) return;
  const uint32_t skey = counter_subkey(d.bkey, (uint32_t)b);
  int y1 = 0, y2 = 0, x1 = 0, x2 = 0;
  if (counter_u01(skey, 0) < d.p) {
    const double S = (double)d.S, full = S * S;
    for (uint32_t a = 0; a < 10; ++a) {
      const double area = full * (d.s0 + (d.s1 - d.s0) * counter_u01(skey, 1 + 4 * a));
      const double ar = exp(d.l0 + (d.l1 - d.l0) * counter_u01(skey, 2 + 4 * a));
      const double fh = rint(sqrt(area * ar)), fw = rint(sqrt(area / ar));
      // compared as doubles: a NaN or a side beyond int range is a refusal, never a conversion
      if (fh < S && fw < S) {
        const int h = (int)fh, w = (int)fw;
        const int i = (int)(counter_u01(skey, 3 + 4 * a) * (double)(d.S - h + 1));
        const int j = (int)(counter_u01(skey, 4 + 4 * a) * (double)(d.S - w + 1));
        y1 = i;
        y2 = i + h;
        x1 = j;
        x2 = j + w;
        break;
      }
    }
  }
  boxes[b * 4 + 0] = y1;
  boxes[b * 4 + 1] = y2;
  boxes[b * 4 + 2] = x1;
  boxes[b * 4 + 3] = x2;
}

// row b of the table, clamped to [0, S]; false: nothing to erase
__device__ __forceinline__ bool erase_box(const int* __restrict__ boxes, int b, int S, PixBox& bx) {
  const int* r = boxes + (size_t)b * 4;
  bx.y1 = r[0] < 0 ? 0 : r[0];
  bx.y2 = r[1] > S ? S : r[1];
  bx.x1 = r[2] < 0 ? 0 : r[2];
  bx.x2 = r[3] > S ? S : r[3];
  return bx.y1 < bx.y2 && bx.x1 < bx.x2;
}

// s2d [B, S2, S2, 16]: grid.y walks the samples, grid.x strides over the 16-B chunks of the 2x2
// pixel groups the sample's box touches (CPG chunks per group)
// EPC: elements per chunk, 4 (f32) or 8 (bf16 / f16: zero has the same bits in both)
template <int EPC>
__global__ __launch_bounds__(NT) void erase_s2d_kernel(i32x4* __restrict__ x,
                                                       const int* __restrict__ boxes, int B, int S2) {
  constexpr int CPG = S2D_CPG<EPC>;
  constexpr uint32_t FULL = S2D_FULL<EPC>;
  const size_t cpi = (size_t)S2 * S2 * CPG;     // chunks per sample
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    PixBox bx;
    if (!erase_box(boxes, b, 2 * S2, bx)) continue;
    const int i0 = bx.y1 >> 1, j0 = bx.x1 >> 1;
    const uint32_t ni = (uint32_t)(((bx.y2 - 1) >> 1) - i0 + 1), nj = (uint32_t)(((bx.x2 - 1) >> 1) - j0 + 1);
    const uint32_t items = ni * nj * CPG;       // S2D_MAX_SIDE: <= 2^30
    i32x4* xs = x + (size_t)b * cpi;
    for (uint32_t t = blockIdx.x * NT + threadIdx.x; t < items; t += gridDim.x * NT) {
      const uint32_t g = t / CPG, ci = t % CPG;
      const uint32_t r = g / nj;
      const int oi = i0 + (int)r, oj = j0 + (int)(g - r * nj);
      const uint32_t em = s2d_box_mask<EPC>(oi, oj, ci, bx);
      if (em == 0) continue;                    // (the f32 padding chunk among them)
      i32x4* c = xs + ((size_t)oi * S2 + oj) * CPG + ci;
      if (em == FULL) {
        *c = i32x4{0, 0, 0, 0};
      } else if constexpr (EPC == 4) {
        int* e = reinterpret_cast<int*>(c);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if ((em >> k) & 1) e[k] = 0;
      } else if (em == 0x0Fu) {                 // slots 8..11 of a group inside the box: 8 B, not the padding
        *reinterpret_cast<unsigned long long*>(c) = 0ull;
      } else {
        short* e = reinterpret_cast<short*>(c);
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if ((em >> k) & 1) e[k] = 0;
      }
    }
  }
}

// NCHW f32 [B, 3, S, S], any S: per (channel, row) of the box, the 16-B chunks (aligned in memory,
// not in the row) that touch the row's span. A chunk wholly inside one span belongs to that lane
// alone; a chunk that two spans share (rows of S % 4 != 0 floats) is never stored whole.
__global__ __launch_bounds__(NT) void erase_nchw_kernel(float* __restrict__ x,
                                                        const int* __restrict__ boxes, int B, int S) {
  const size_t epi = (size_t)3 * S * S;         // elements per sample
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    PixBox bx;
    if (!erase_box(boxes, b, S, bx)) continue;
    const uint32_t h = (uint32_t)(bx.y2 - bx.y1), w = (uint32_t)(bx.x2 - bx.x1);
    const uint32_t ncm = (w + 3) / 4 + 1;       // most chunks a span of w floats can touch
    const uint32_t items = 3u * h * ncm;        // NCHW_MAX_SIDE: < 2^32
    for (uint32_t t = blockIdx.x * NT + threadIdx.x; t < items; t += gridDim.x * NT) {
      const uint32_t r = t / ncm, k = t - r * ncm;
      const uint32_t c = r / h;
      const uint32_t y = (uint32_t)bx.y1 + (r - c * h);
      const size_t e0 = (size_t)b * epi + ((size_t)c * S + y) * S + bx.x1, e1 = e0 + w;
      const size_t base = ((e0 >> 2) + k) << 2;
      if (base >= e1) continue;
      if (base >= e0 && base + 4 <= e1) {
        *reinterpret_cast<i32x4*>(x + base) = i32x4{0, 0, 0, 0};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (base + e >= e0 && base + e < e1) x[base + e] = 0.0f;
      }
    }
  }
}

}  // namespace

extern "C" {

int pda_erase_draw(int B, int S, unsigned bkey, double p, double s0, double s1, double l0, double l1,
                   int* boxes, hipStream_t st) {
  if (B <= 0 || S <= 0 || S > S2D_MAX_SIDE || boxes == nullptr) return -2;
  if (!(p >= 0.0 && p <= 1.0)) return -2;                     // (NaN fails both)
  if (!std::isfinite(s0) || !std::isfinite(s1) || !std::isfinite(l0) || !std::isfinite(l1)) return -2;
  if (s0 < 0.0 || s0 > s1 || l0 > l1) return -2;
  if ((uintptr_t)boxes % 4) return -2;
  EraseDraw d;
  d.bkey = bkey;
  d.S = S;
  d.p = p;
  d.s0 = s0;
  d.s1 = s1;
  d.l0 = l0;
  d.l1 = l1;
  TRACKED_LAUNCH(erase_draw_kernel, dim3((unsigned)((B + NT - 1) / NT)), dim3(NT), 0, st, B, d, boxes);
  return (int)hipGetLastError();
}

int pda_batch_erase(void* x, const int* boxes, int B, int S, int dt, int layout, int grid_cap,
                    hipStream_t st) {
  if (!batch_args_ok(B, S, dt, layout, {x}) || grid_cap < 0) return -2;
  if (boxes == nullptr || (uintptr_t)boxes % 4) return -2;
  // the host does not know the boxes: grid.y walks the samples, grid.x is sized for a box of a
  // third of the image (RandomErasing's largest scale), at least ~4096 blocks in all when the
  // images are that large; larger boxes take more trips of the stride loop
  auto grid = [&](long long items) { return batch_grid(B, items / 3, grid_cap, NT, 4096); };
  if (layout == 0) {
    const int S2 = S / 2;
    const long long cpi = (long long)S2 * S2 * (dt == DT_F32 ? 4 : 2);
    i32x4* xi = (i32x4*)x;
    if (dt == DT_F32)
      TRACKED_LAUNCH(erase_s2d_kernel<4>, grid(cpi), dim3(NT), 0, st, xi, boxes, B, S2);
    else
      TRACKED_LAUNCH(erase_s2d_kernel<8>, grid(cpi), dim3(NT), 0, st, xi, boxes, B, S2);
  } else {
    TRACKED_LAUNCH(erase_nchw_kernel, grid(3LL * S * ((S + 3) / 4)), dim3(NT), 0, st, (float*)x, boxes,
                   B, S);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
