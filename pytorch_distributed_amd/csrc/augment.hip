// Folder-image augmentation for gfx950: resample (PIL's bilinear / triangle filter on a real-valued
// box), horizontal flip, normalise and store model-ready, in one launch over a packed batch of raw
// uint8 HWC images of different sizes (data/folder.py raw mode; K12).
//
//   R[oy][ox][c] = sum_y kv(oy,y) * sum_x kh(ox,x) * I[y][x][c]          (levels 0..255, no rounding)
//   out = (R[oy][flip ? S-1-ox : ox][c] / 255 - mean[c]) / std[c]
//
// Per axis (PIL precompute_coeffs, all in double; this file is built with -ffp-contract=off so the
// integer tap bounds are those of a float64 numpy evaluation of the same expressions):
//   scale = (x1-x0)/S, fs = max(scale,1), center(o) = x0 + (o+0.5)*scale,
//   xmin = max(int(center-fs+0.5),0), xmax = min(int(center+fs+0.5),W),
//   w(x) = max(0, 1-|(x-center+0.5)/fs|), k(x) = w(x)/sum(w).
//
// One block per (image, strip of AUG_TR output rows, tile of <= AUG_TW output columns). The strip's
// band of source rows [ymin(first row), ymax(last row)) is walked in chunks of AUG_NR rows: each
// chunk row is filtered horizontally ONCE into an LDS row buffer (f32 [row][column][3]), then every
// thread adds the chunk's rows, in source order, into the register accumulators of the output
// values it owns (3 interleaved columns x AUG_TR rows). LDS and registers are therefore independent
// of the scale: a strong downscale walks more chunks, an upscale has a band of 2-3 rows that feeds
// all rows of the strip. Tap weights are evaluated where they are used (no per-tap table, so no
// limit on the tap count); sums are sequential f32 fmas in a fixed order: deterministic, no atomics.
// Source bytes are read one at a time, so image offsets and row pitches (3*W) need no alignment.
#include "common.h"

namespace {

constexpr int AUG_NT = 256;
constexpr int AUG_TR = 8;     // output rows per block (even: s2d pairs rows)
constexpr int AUG_TW = 256;   // output columns per block (even)
constexpr int AUG_NR = 8;     // source rows per chunk
constexpr int AUG_CPT = AUG_TW * 3 / AUG_NT;   // interleaved (column, channel) values per thread

struct AugNorm {
  float a[3], b[3];   // out = R * a[c] + b[c]: a = 1/(255 std), b = -mean/std
};

struct AugAxis {
  double scale, fs, inv_fs, lo;
  int n;   // source extent
};

__device__ __forceinline__ double aug_center(const AugAxis& ax, int o) {
  return ax.lo + ((double)o + 0.5) * ax.scale;
}
__device__ __forceinline__ int aug_min(const AugAxis& ax, double center) {
  const int v = (int)(center - ax.fs + 0.5);
  return v < 0 ? 0 : v;
}
__device__ __forceinline__ int aug_max(const AugAxis& ax, double center) {
  const int v = (int)(center + ax.fs + 0.5);
  return v > ax.n ? ax.n : v;
}
__device__ __forceinline__ double aug_w(const AugAxis& ax, double center, int x) {
  const double w = 1.0 - fabs(((double)x - center + 0.5) * ax.inv_fs);
  return w < 0.0 ? 0.0 : w;
}
// 1 / sum of the taps' weights
__device__ __forceinline__ double aug_inv_sum(const AugAxis& ax, double center, int lo, int hi) {
  double s = 0.0;
  for (int x = lo; x < hi; ++x) s += aug_w(ax, center, x);
  return 1.0 / s;
}

// LAYOUT 0: s2d [B][S/2][S/2][16] of DT; 1: NCHW f32 [B][3][S][S]
template <int DT, int LAYOUT>
__global__ __launch_bounds__(AUG_NT) void aug_resize_kernel(const uint8_t* __restrict__ packed,
                                                            const long long* __restrict__ ti,
                                                            const double* __restrict__ tf, int S,
                                                            int nstrips, int ntx,
                                                            void* __restrict__ out, AugNorm nm) {
  __shared__ float s_row[AUG_NR * AUG_TW * 3];   // chunk rows; reused as the finished tile
  __shared__ double s_xc[AUG_TW], s_xinv[AUG_TW];
  __shared__ int s_xmin[AUG_TW], s_xmax[AUG_TW];
  __shared__ double s_yc[AUG_TR], s_yinv[AUG_TR];
  __shared__ int s_ymin[AUG_TR], s_ymax[AUG_TR];
  __shared__ float s_kv[AUG_NR][AUG_TR];

  const int tid = threadIdx.x;
  uint32_t bid = blockIdx.x;
  const int tx = (int)(bid % (uint32_t)ntx);
  bid /= (uint32_t)ntx;
  const int strip = (int)(bid % (uint32_t)nstrips);
  const int b = (int)(bid / (uint32_t)nstrips);

  const long long off = ti[b * 4 + 0];
  const int H = (int)ti[b * 4 + 1], W = (int)ti[b * 4 + 2];
  const bool flip = ti[b * 4 + 3] != 0;
  const double bx0 = tf[b * 4 + 0], by0 = tf[b * 4 + 1], bx1 = tf[b * 4 + 2], by1 = tf[b * 4 + 3];
  AugAxis ax, ay;
  ax.scale = (bx1 - bx0) / (double)S;
  ax.fs = ax.scale < 1.0 ? 1.0 : ax.scale;
  ax.inv_fs = 1.0 / ax.fs;
  ax.lo = bx0;
  ax.n = W;
  ay.scale = (by1 - by0) / (double)S;
  ay.fs = ay.scale < 1.0 ? 1.0 : ay.scale;
  ay.inv_fs = 1.0 / ay.fs;
  ay.lo = by0;
  ay.n = H;

  const int ox0 = tx * AUG_TW, tw = min(AUG_TW, S - ox0);      // even: S and AUG_TW are
  const int oy0 = strip * AUG_TR, tr = min(AUG_TR, S - oy0);   // even likewise
  const uint8_t* img = packed + off;

  for (int i = tid; i < tw; i += AUG_NT) {
    const double c = aug_center(ax, ox0 + i);
    const int lo = aug_min(ax, c), hi = aug_max(ax, c);
    s_xc[i] = c;
    s_xmin[i] = lo;
    s_xmax[i] = hi;
    s_xinv[i] = aug_inv_sum(ax, c, lo, hi);
  }
  if (tid < AUG_TR) {
    // rows past the strip's end (tid >= tr) get an empty tap range
    const double c = aug_center(ay, oy0 + tid);
    const int lo = tid < tr ? aug_min(ay, c) : 0, hi = tid < tr ? aug_max(ay, c) : 0;
    s_yc[tid] = c;
    s_ymin[tid] = lo;
    s_ymax[tid] = hi;
    s_yinv[tid] = tid < tr ? aug_inv_sum(ay, c, lo, hi) : 0.0;
  }
  __syncthreads();

  float acc[AUG_CPT][AUG_TR];
#pragma unroll
  for (int m = 0; m < AUG_CPT; ++m)
#pragma unroll
    for (int r = 0; r < AUG_TR; ++r) acc[m][r] = 0.f;

  const int tw3 = tw * 3;
  const int ylo = s_ymin[0], yhi = s_ymax[tr - 1];   // tap bounds are monotone in the output row
  for (int yc = ylo; yc < yhi; yc += AUG_NR) {
    const int nr = min(AUG_NR, yhi - yc);
    // vertical weights of this chunk's rows (0 outside an output row's taps)
    if (tid < AUG_NR * AUG_TR) {
      const int yy = tid / AUG_TR, r = tid % AUG_TR, y = yc + yy;
      float k = 0.f;
      if (yy < nr && y >= s_ymin[r] && y < s_ymax[r])
        k = (float)(aug_w(ay, s_yc[r], y) * s_yinv[r]);
      s_kv[yy][r] = k;
    }
    // horizontal pass: (row, column) items, 3 channels each
    for (int i = tid; i < nr * tw; i += AUG_NT) {
      const int yy = i / tw, ox = i - yy * tw;
      const int xa = s_xmin[ox], xb = s_xmax[ox];
      const double c = s_xc[ox], inv = s_xinv[ox];
      const uint8_t* p = img + ((size_t)(yc + yy) * W + xa) * 3;
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      for (int x = xa; x < xb; ++x, p += 3) {
        const float k = (float)(aug_w(ax, c, x) * inv);
        a0 = __builtin_fmaf(k, (float)p[0], a0);
        a1 = __builtin_fmaf(k, (float)p[1], a1);
        a2 = __builtin_fmaf(k, (float)p[2], a2);
      }
      float* d = s_row + yy * tw3 + ox * 3;
      d[0] = a0;
      d[1] = a1;
      d[2] = a2;
    }
    __syncthreads();
    // vertical pass: rows in source order into the accumulators
    for (int yy = 0; yy < nr; ++yy) {
#pragma unroll
      for (int r = 0; r < AUG_TR; ++r) {
        const float k = s_kv[yy][r];
        if (k != 0.f) {
#pragma unroll
          for (int m = 0; m < AUG_CPT; ++m) {
            const int q = tid + m * AUG_NT;
            if (q < tw3) acc[m][r] = __builtin_fmaf(k, s_row[yy * tw3 + q], acc[m][r]);
          }
        }
      }
    }
    __syncthreads();
  }

  // normalise into the tile image [row][column][3] (unflipped)
#pragma unroll
  for (int m = 0; m < AUG_CPT; ++m) {
    const int q = tid + m * AUG_NT;
    if (q < tw3) {
      const int c = q % 3;
#pragma unroll
      for (int r = 0; r < AUG_TR; ++r)
        if (r < tr) s_row[r * tw3 + q] = __builtin_fmaf(acc[m][r], nm.a[c], nm.b[c]);
    }
  }
  __syncthreads();

  // stored column j of the tile (from oxs) is tile column (flip ? tw-1-j : j)
  const int oxs = flip ? S - ox0 - tw : ox0;
  if constexpr (LAYOUT == 0) {
    const int S2 = S / 2, tw2 = tw / 2;
    for (int i = tid; i < (tr / 2) * tw2; i += AUG_NT) {
      const int ri = i / tw2, j = i - ri * tw2;
      float h[16];
#pragma unroll
      for (int pq = 0; pq < 4; ++pq) {
        const int col = 2 * j + (pq & 1);
        const float* s = s_row + (2 * ri + (pq >> 1)) * tw3 + (flip ? tw - 1 - col : col) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) h[pq * 3 + c] = s[c];
      }
#pragma unroll
      for (int c = 12; c < 16; ++c) h[c] = 0.f;
      const size_t o = (((size_t)b * S2 + (oy0 / 2 + ri)) * S2 + (oxs / 2 + j)) * 16;
      store8<DT>(out, o, h);
      store8<DT>(out, o + 8, h + 8);
    }
  } else {
    float* o = reinterpret_cast<float*>(out);
    for (int i = tid; i < 3 * tr * tw; i += AUG_NT) {
      const int c = i / (tr * tw), rem = i - c * (tr * tw);
      const int r = rem / tw, j = rem - r * tw;
      o[(((size_t)b * 3 + c) * S + (oy0 + r)) * S + oxs + j] =
          s_row[r * tw3 + (flip ? tw - 1 - j : j) * 3 + c];
    }
  }
}

}  // namespace

extern "C" {

// packed: device bytes; ti: device int64 [B][4] = byte offset, H, W, flip; tf: device f64 [B][4] =
// x0, y0, x1, y1; mean / std: HOST float[3]. layout 0: s2d [B][S/2][S/2][16] of dtype dt (16-B
// aligned), 1: NCHW f32. The tables must have been validated by the caller (ops/native_ops.py
// aug_check): the kernel trusts offsets, sizes and boxes.
int pda_aug_resize(const void* packed, const long long* ti, const double* tf, int B, int S, void* out,
                   int dt, int layout, const float* mean, const float* std, hipStream_t st) {
  if (B < 1 || S < 2 || (S & 1) || (layout != 0 && layout != 1)) return -2;
  if (layout == 1 && dt != DT_F32) return -2;
  if (layout == 0 && ((uintptr_t)out & 15)) return -2;
  AugNorm nm;
  for (int c = 0; c < 3; ++c) {
    nm.a[c] = (float)(1.0 / (255.0 * (double)std[c]));
    nm.b[c] = (float)(-(double)mean[c] / (double)std[c]);
  }
  const int nstrips = (S + AUG_TR - 1) / AUG_TR, ntx = (S + AUG_TW - 1) / AUG_TW;
  const long long nblk = (long long)B * nstrips * ntx;
  if (nblk > 0x7fffffffLL) return -2;
  const dim3 grid((unsigned)nblk), block(AUG_NT);
  const uint8_t* src = reinterpret_cast<const uint8_t*>(packed);
#define AUG_K(D, L) \
  TRACKED_LAUNCH((aug_resize_kernel<D, L>), grid, block, 0, st, src, ti, tf, S, nstrips, ntx, out, nm)
  if (layout == 1) AUG_K(DT_F32, 1);
  else if (dt == DT_BF16) AUG_K(DT_BF16, 0);
  else if (dt == DT_F16) AUG_K(DT_F16, 0);
  else if (dt == DT_F32) AUG_K(DT_F32, 0);
  else return -2;
#undef AUG_K
  return (int)hipGetLastError();
}

}  // extern "C"
