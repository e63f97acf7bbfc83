// Folder-image augmentation for gfx950: resample (PIL's bilinear / triangle filter on a real-valued
// box), horizontal flip, normalise and store model-ready, in one launch over a packed batch of raw
// uint8 HWC images of different sizes (data/folder.py raw mode; K12). A second, small kernel
// (aug_draw_kernel, below) draws the crop boxes and flips on the device for the packed data path
// (data/packed.py), whose decoded images stay resident and need no per-step host pipeline.
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
//
// Source format 1 (FMT, version-2 packed files of data/packed.py) is YCbCr 4:2:0: a record is the Y
// plane [H][W], then the interleaved CbCr plane [Hc][Wc][2] at half resolution (Hc = (H+1)/2,
// Wc = (W+1)/2). The stored image is I = (Y[y][x], Cb[y>>1][x>>1] - 128, Cr[y>>1][x>>1] - 128)
// (nearest chroma; the subtraction is exact in f32). The colour transform is linear, so the same
// tap loops filter these three planes and the store stage converts once per output pixel:
//   R = Y + 1.402 cr, G = Y - 0.344136 cb - 0.714136 cr, B = Y + 1.772 cb, clamped to [0, 255],
// then normalised as above. A grey image has filtered chroma of exactly 0 and R = G = B = Y.
#include "batch_image.h"
#include "pda_api.h"

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

// filtered (Y, Cb-128, Cr-128) levels -> channel c of the clamped RGB levels (format 1)
__device__ __forceinline__ float aug_rgb(float y, float cb, float cr, int c) {
  const float v = c == 0   ? __builtin_fmaf(1.402f, cr, y)
                  : c == 1 ? __builtin_fmaf(-0.714136f, cr, __builtin_fmaf(-0.344136f, cb, y))
                           : __builtin_fmaf(1.772f, cb, y);
  return fminf(fmaxf(v, 0.f), 255.f);
}

// LAYOUT 0: s2d [B][S/2][S/2][16] of DT; 1: NCHW f32 [B][3][S][S]. FMT 0: HWC RGB; 1: YCbCr 4:2:0
template <int DT, int LAYOUT, int FMT>
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
      float a0 = 0.f, a1 = 0.f, a2 = 0.f;
      if constexpr (FMT == 0) {
        const uint8_t* p = img + ((size_t)(yc + yy) * W + xa) * 3;
        for (int x = xa; x < xb; ++x, p += 3) {
          const float k = (float)(aug_w(ax, c, x) * inv);
          a0 = __builtin_fmaf(k, (float)p[0], a0);
          a1 = __builtin_fmaf(k, (float)p[1], a1);
          a2 = __builtin_fmaf(k, (float)p[2], a2);
        }
      } else {
        // y < H and x < W, so (y>>1, x>>1) lies inside the [Hc][Wc] chroma plane
        const int y = yc + yy, Wc = (W + 1) >> 1;
        const uint8_t* py = img + (size_t)y * W;
        const uint8_t* pc = img + (size_t)H * W + (size_t)(y >> 1) * Wc * 2;
        for (int x = xa; x < xb; ++x) {
          const float k = (float)(aug_w(ax, c, x) * inv);
          const uint8_t* q = pc + (x >> 1) * 2;
          a0 = __builtin_fmaf(k, (float)py[x], a0);
          a1 = __builtin_fmaf(k, (float)q[0] - 128.f, a1);
          a2 = __builtin_fmaf(k, (float)q[1] - 128.f, a2);
        }
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

  // normalise into the tile image [row][column][3] (unflipped); format 1 leaves the filtered
  // YCbCr levels there: a thread holds no whole pixel, the store stage converts and normalises
#pragma unroll
  for (int m = 0; m < AUG_CPT; ++m) {
    const int q = tid + m * AUG_NT;
    if (q < tw3) {
      const int c = q % 3;
#pragma unroll
      for (int r = 0; r < AUG_TR; ++r) {
        if constexpr (FMT == 0) {
          if (r < tr) s_row[r * tw3 + q] = __builtin_fmaf(acc[m][r], nm.a[c], nm.b[c]);
        } else {
          if (r < tr) s_row[r * tw3 + q] = acc[m][r];
        }
      }
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
        for (int c = 0; c < 3; ++c) {
          if constexpr (FMT == 0) h[pq * 3 + c] = s[c];
          else h[pq * 3 + c] = __builtin_fmaf(aug_rgb(s[0], s[1], s[2], c), nm.a[c], nm.b[c]);
        }
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
      if constexpr (FMT == 0) {
        o[(((size_t)b * 3 + c) * S + (oy0 + r)) * S + oxs + j] =
            s_row[r * tw3 + (flip ? tw - 1 - j : j) * 3 + c];
      } else {
        const float* s = s_row + r * tw3 + (flip ? tw - 1 - j : j) * 3;
        o[(((size_t)b * 3 + c) * S + (oy0 + r)) * S + oxs + j] =
            __builtin_fmaf(aug_rgb(s[0], s[1], s[2], c), nm.a[c], nm.b[c]);
      }
    }
  }
}

// ---- crop draw (packed data path, data/packed.py) ---------------------------------------------
// One thread per sample: looks the sample's record up in the dataset index [N][4] = (byte offset, H,
// W, label) and writes the rows of the tables aug_resize_kernel reads, plus the label. Train mode is
// data/folder.py train_crop_params (RandomResizedCrop + flip) in double; val mode is val_crop_params.
// The uniforms are counter-based (batch_image.h): u(k) = counter_u01(ekey, k) with
//   key = hash32(id*2654435761 + salt), salt = (seed*97 + split_id)*0x632BE5AB   (as the synthetic data)
//   ekey = counter_subkey(key, epoch)
// and fixed counters: attempt a draws area 4a, ratio 4a+1, row 4a+2, column 4a+3; the flip is 40. A
// sample's crop therefore depends on (seed, split, epoch, id) alone, not on where in which batch of
// which rank it is drawn. tests/packed_refs.py evaluates the same expressions in Python float64.
struct AugDraw {
  long long N;
  uint32_t salt, epoch;
  int mode, S, resize;
  double s0, s1, l0, l1, r0, r1;   // scale bounds, log ratio bounds, ratio bounds
};

__global__ __launch_bounds__(AUG_NT) void aug_draw_kernel(const long long* __restrict__ ids,
                                                          const long long* __restrict__ index,
                                                          const long long* __restrict__ batch_off,
                                                          int B, AugDraw d, long long* __restrict__ ti,
                                                          double* __restrict__ tf,
                                                          long long* __restrict__ labels) {
  const int b = blockIdx.x * AUG_NT + threadIdx.x;
  if (b >= B) return;
  long long id = ids[b];
  // the wrapper checked the ids on the host; a stray one must still not read outside the index
  if ((unsigned long long)id >= (unsigned long long)d.N) id = 0;
  const long long* rec = index + id * 4;
  const long long off = batch_off != nullptr ? batch_off[b] : rec[0];
  const int H = (int)rec[1], W = (int)rec[2];
  double x0, y0, x1, y1;
  int flip = 0;
  if (d.mode == 0) {
    const uint32_t key = hash32((uint32_t)id * 2654435761u + d.salt);
    const uint32_t ekey = counter_subkey(key, d.epoch);
    const double area = (double)(W * H);
    int w = 0, h = 0, i = 0, j = 0;
    bool ok = false;
    for (uint32_t a = 0; a < 10 && !ok; ++a) {
      const double target = area * (d.s0 + (d.s1 - d.s0) * counter_u01(ekey, 4 * a));
      const double ar = exp(d.l0 + (d.l1 - d.l0) * counter_u01(ekey, 4 * a + 1));
      w = (int)rint(sqrt(target * ar));
      h = (int)rint(sqrt(target / ar));
      if (0 < w && w <= W && 0 < h && h <= H) {
        i = (int)(counter_u01(ekey, 4 * a + 2) * (double)(H - h + 1));
        j = (int)(counter_u01(ekey, 4 * a + 3) * (double)(W - w + 1));
        ok = true;
      }
    }
    if (!ok) {   // centre crop at the clamped ratio
      const double in_ratio = (double)W / (double)H;
      if (in_ratio < d.r0) {
        w = W;
        h = (int)rint((double)W / d.r0);
      } else if (in_ratio > d.r1) {
        h = H;
        w = (int)rint((double)H * d.r1);
      } else {
        w = W;
        h = H;
      }
      w = w < 1 ? 1 : (w > W ? W : w);   // no-ops for r0 <= r1; the box must stay inside the image
      h = h < 1 ? 1 : (h > H ? H : h);
      i = (H - h) / 2;
      j = (W - w) / 2;
    }
    x0 = (double)j;
    y0 = (double)i;
    x1 = (double)(j + w);
    y1 = (double)(i + h);
    flip = counter_u01(ekey, 40) < 0.5 ? 1 : 0;
  } else {
    int nw, nh;
    if (W <= H) {
      nw = d.resize;
      nh = (int)((double)((long long)d.resize * H) / (double)W);
    } else {
      nh = d.resize;
      nw = (int)((double)((long long)d.resize * W) / (double)H);
    }
    const int top = (int)rint((double)(nh - d.S) / 2.0), left = (int)rint((double)(nw - d.S) / 2.0);
    x0 = (double)((long long)left * W) / (double)nw;
    y0 = (double)((long long)top * H) / (double)nh;
    x1 = (double)((long long)(left + d.S) * W) / (double)nw;
    y1 = (double)((long long)(top + d.S) * H) / (double)nh;
  }
  ti[b * 4 + 0] = off;
  ti[b * 4 + 1] = H;
  ti[b * 4 + 2] = W;
  ti[b * 4 + 3] = flip;
  tf[b * 4 + 0] = x0;
  tf[b * 4 + 1] = y0;
  tf[b * 4 + 2] = x1;
  tf[b * 4 + 3] = y1;
  labels[b] = rec[3];
}

}  // namespace

extern "C" {

int pda_aug_resize_fmt(const void* packed, const long long* ti, const double* tf, int B, int S,
                       void* out, int dt, int layout, int fmt, const float* mean, const float* std,
                       hipStream_t st) {
  if (B < 1 || S < 2 || (S & 1) || (layout != 0 && layout != 1) || (fmt != 0 && fmt != 1)) return -2;
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
#define AUG_K1(D, L, F) \
  TRACKED_LAUNCH((aug_resize_kernel<D, L, F>), grid, block, 0, st, src, ti, tf, S, nstrips, ntx, out, nm)
#define AUG_K(D, L)                \
  do {                             \
    if (fmt == 0) AUG_K1(D, L, 0); \
    else AUG_K1(D, L, 1);          \
  } while (0)
  if (layout == 1) AUG_K(DT_F32, 1);
  else if (dt == DT_BF16) AUG_K(DT_BF16, 0);
  else if (dt == DT_F16) AUG_K(DT_F16, 0);
  else if (dt == DT_F32) AUG_K(DT_F32, 0);
  else return -2;
#undef AUG_K
#undef AUG_K1
  return (int)hipGetLastError();
}

int pda_aug_draw(const long long* ids, const long long* index, const long long* batch_off, int B,
                 long long N, unsigned seed, int split_id, unsigned epoch, int mode, int S, int resize,
                 double s0, double s1, double r0, double r1, long long* ti, double* tf,
                 long long* labels, hipStream_t st) {
  if (B < 1 || N < 1 || S < 2 || (mode != 0 && mode != 1)) return -2;
  if (mode == 0 && !(0.0 < s0 && s0 <= s1 && s1 <= 1.0 && 1e-3 <= r0 && r0 <= r1 && r1 <= 1e3)) return -2;
  if (mode == 1 && (resize < S || resize > 65536)) return -2;
  AugDraw d;
  d.N = N;
  d.salt = (seed * 97u + (unsigned)split_id) * 0x632BE5ABu;
  d.epoch = epoch;
  d.mode = mode;
  d.S = S;
  d.resize = resize;
  d.s0 = s0;
  d.s1 = s1;
  d.l0 = log(r0);
  d.l1 = log(r1);
  d.r0 = r0;
  d.r1 = r1;
  const dim3 grid((unsigned)((B + AUG_NT - 1) / AUG_NT)), block(AUG_NT);
  TRACKED_LAUNCH(aug_draw_kernel, grid, block, 0, st, ids, index, batch_off, B, d, ti, tf, labels);
  return (int)hipGetLastError();
}

}  // extern "C"
