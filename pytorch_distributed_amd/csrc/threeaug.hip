// 3-Augment for gfx950 (DeiT-III; timm's three_augment): per sample ONE of Grayscale(3),
// RandomSolarize(p=1) and GaussianBlur(kernel_size=2R+1, sigma in [0.1, 2]) on a finished,
// normalised batch, after RandAugment and before the colour jitter (jitter.hip), whose conventions
// hold: un-normalise with the clamp, the op, re-normalise ((y - mean) * (1 / std)), one rounding to
// the batch dtype. Built without FMA contraction: every fma below is written as fmaf.
//
//   three_aug_draw : one thread per sample writes its row of the int32 table [B][16]:
//                    (op, bits(sigma), R, 0, bits(w[0]) .. bits(w[11])). Counter-based uniforms as
//                    erase_draw (batch_image.h), in double: skey = counter_subkey(bkey, b),
//                    op = int(u(0) * 3), sigma = float(0.1 + 1.9 * u(1)); from the float32 sigma
//                    widened to double e[d] = exp(-0.5 (d / sigma)^2), sum = e[0] + sum_{d=1..R}
//                    2 e[d] in ascending d, w[d] = float(e[d] / sum); 0 beyond R.
//   three_aug      : out of place, one launch, one uniform branch per sample.
//
// The grid: grid.y walks the samples, grid.x the TH x TW = 32 x 32 pixel tiles of one sample (both
// strided when grid_cap holds the grid below B x tiles). A blur sample's block takes tiles
// blockIdx.x, blockIdx.x + gridDim.x, ... . A point-wise sample (grayscale, solarize) has no tiles:
// its gridDim.x blocks stride over the sample's 16-B items instead, block blockIdx.x taking items
// blockIdx.x * 256 + lane, + gridDim.x * 256, ...; a 32 x 32 tile is 256 s2d groups, so on the
// natural grid every block of a point-wise sample moves exactly one tile's worth of chunks and none
// sits idle. A lane's item is a 2x2 s2d group (two 16-B chunks in bf16 / f16, four in f32: the
// padding chunk of dst gets src's bits) or four pixels of each NCHW plane (one pixel when
// S % 4 != 0), as in jitter.hip.
//
// A blur tile (all 256 lanes of the block, four barriers):
//   1. stage-in : the in-image part of the (th + 22) x (tw + 22) source region around the tile
//                 (th, tw <= 32: the tile clipped to the image; the halo is always RMAX = 11 wide,
//                 the weights beyond the row's R are 0 and add +0 to a non-negative sum, so the
//                 result is that of 2R + 1 taps bit for bit) comes in through 16-B loads of the
//                 layout's chunks, is un-normalised and clamped once per element and written to
//                 LDS as planar f32 st[c][row][col], row stride 55 floats.
//   2. border   : region elements outside the image are copied from their reflection
//                 (-k -> k, S-1+k -> S-1-k), which lies inside the image part of the same region
//                 (proof at fill_border); LDS to LDS, no global access. Tiles whose region lies
//                 inside the image skip it.
//   3. horizontal: item (c, region row, 8 output columns), lanes along the ROWS: 30 LDS reads at
//                 lane stride 55 (odd: no bank conflict) feed 8 accumulators of 23 sequential fmaf
//                 in ascending tap order; results to hm[c][row][col], row stride 33 (odd again).
//   4. vertical : a lane owns what it stores: a 2x2 s2d group (6 columns (c, x) of 2 rows) or
//                 2 rows x 4 pixels of one NCHW plane; per column 24 LDS reads (lanes along x)
//                 feed 2 accumulators of 23 sequential fmaf; re-normalise, round once, 16-B
//                 stores (element-wise in NCHW when S % 4 != 0).
//   The 12 weights are read once per sample from the table row, uniformly: they live in SGPRs.
//   The layout is a template parameter that changes stage-in and store-out only.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -Rpass-analysis=kernel-resource-usage):
//
//   kernel                         VGPRs  SGPRs  scratch B/lane  LDS B/block  waves/SIMD
//   three_aug_kernel<S2d<f32>>     205    106    0               57032        2
//   three_aug_kernel<S2d<bf16>>    205    106    0               57032        2
//   three_aug_kernel<S2d<f16>>     205    106    0               57032        2
//   three_aug_kernel<Nchw<4>>      132    106    0               57032        2
//   three_aug_kernel<Nchw<1>>      131    106    16              57032        2
//   three_aug_draw_kernel           38     14    0                   0        8
//
// LDS: st 3 x 54 x 55 x 4 = 35640 B, hm 3 x 54 x 33 x 4 = 21384 B: two blocks (8 waves, 2 per SIMD,
// 2 x 205 VGPRs of 512) fit a CU's 160 KiB; LDS, not registers, sets the occupancy.
// No atomics, fixed summation order: two launches give identical bits.
#include <cmath>

#include "batch_image.h"
#include "pda_api.h"

namespace {

constexpr int NT = 256;
constexpr int ROW = 16;             // int32 per table row
constexpr int RMAX = 11;            // largest radius: 23 taps per axis
constexpr int TH = 32, TW = 32;     // output tile, pixels
constexpr int RH = TH + 2 * RMAX, RW = TW + 2 * RMAX;   // source region of a tile
constexpr int SS = RW + 1, SP = RH * SS;                // st: row and plane stride, floats
constexpr int HS = TW + 1, HP = RH * HS;                // hm: row and plane stride, floats
static_assert((3 * SP + 3 * HP) * 4 <= 65536, "a block's LDS");
static_assert(2 * (3 * SP + 3 * HP) * 4 <= 160 * 1024, "two blocks per CU");
static_assert(TH % 2 == 0 && TW % 8 == 0 && (TH / 2) * (TW / 2) == NT, "tile / lane mapping");

__global__ __launch_bounds__(NT) void three_aug_draw_kernel(int B, int R, uint32_t bkey,
                                                            int* __restrict__ table) {
  const int n = blockIdx.x * NT + threadIdx.x;
  if (n >= B) return;
  const uint32_t skey = counter_subkey(bkey, (uint32_t)n);
  const int op = (int)(counter_u01(skey, 0u) * 3.0);
  const float sigma = (float)(0.1 + 1.9 * counter_u01(skey, 1u));
  const double s = (double)sigma;
  double e[RMAX + 1], sum = 0.0;
#pragma unroll
  for (int d = 0; d <= RMAX; ++d) {
    const double q = (double)d / s;
    e[d] = d <= R ? exp(-0.5 * (q * q)) : 0.0;
    sum += d == 0 ? e[d] : 2.0 * e[d];
  }
  int* row = table + (size_t)n * ROW;
  row[0] = op;
  row[1] = __float_as_int(sigma);
  row[2] = R;
  row[3] = 0;
#pragma unroll
  for (int d = 0; d <= RMAX; ++d) row[4 + d] = __float_as_int((float)(e[d] / sum));
}

struct Norm3 {
  float mean[3], std[3], istd[3];
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float pick3(const float (&a)[3], int c) { return c == 0 ? a[0] : (c == 1 ? a[1] : a[2]); }

// ---- the layouts: the point-wise item of a lane, and a blur tile's stage-in and store-out -------
// s2d [B, S/2, S/2, 16]: group g = (gi, gj) row-major is CPG 16-B chunks; slot (2p+q)*3 + c
template <int DT_> struct S2d {
  static constexpr int DT = DT_, PIX = 4;
  static constexpr int CPG = DT == DT_F32 ? 4 : 2;
  i32x4 pad;                        // the chunk that holds only (f32) or also (16-bit) padding slots
  __host__ __device__ static uint32_t items(int S) { return (uint32_t)(S / 2) * (uint32_t)(S / 2); }
  __host__ __device__ static size_t sample_bytes(int S) { return (size_t)items(S) * CPG * 16; }

  __device__ __forceinline__ void load(const char* xs, uint32_t g, int, float* v) {
    const i32x4* c = reinterpret_cast<const i32x4*>(xs) + (size_t)g * CPG;
    if constexpr (DT == DT_F32) {
      const i32x4 a0 = c[0], a1 = c[1], a2 = c[2];
      pad = c[3];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[e] = __int_as_float(a0[e]);
        v[4 + e] = __int_as_float(a1[e]);
        v[8 + e] = __int_as_float(a2[e]);
      }
    } else {
      const i32x4 c0 = c[0];
      pad = c[1];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const f32x2 f = unpack2<DT>((uint32_t)(k < 4 ? c0[k] : pad[k - 4]));
        v[2 * k] = f.x;
        v[2 * k + 1] = f.y;
      }
    }
  }
  __device__ __forceinline__ void load_pad(const char* xs, uint32_t g) {
    pad = reinterpret_cast<const i32x4*>(xs)[(size_t)g * CPG + CPG - 1];
  }
  // after load or load_pad of the same group of src
  __device__ __forceinline__ void store(char* xd, uint32_t g, int, const float* v) const {
    i32x4* c = reinterpret_cast<i32x4*>(xd) + (size_t)g * CPG;
    if constexpr (DT == DT_F32) {
      c[0] = i32x4{__float_as_int(v[0]), __float_as_int(v[1]), __float_as_int(v[2]), __float_as_int(v[3])};
      c[1] = i32x4{__float_as_int(v[4]), __float_as_int(v[5]), __float_as_int(v[6]), __float_as_int(v[7])};
      c[2] = i32x4{__float_as_int(v[8]), __float_as_int(v[9]), __float_as_int(v[10]), __float_as_int(v[11])};
      c[3] = pad;
    } else {
      i32x4 c0, c1 = pad;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int w = (int)pack2<DT>(f32x2{v[2 * k], v[2 * k + 1]});
        if (k < 4) c0[k] = w; else c1[k - 4] = w;
      }
      c[0] = c0;
      c[1] = c1;
    }
  }
};

// NCHW f32 [B, 3, S, S]; VEC 4 (S % 4 == 0: every row of every plane starts on 16 bytes): item t =
// pixels 4t .. 4t+3 of each plane; VEC 1: pixel t, element-wise
template <int VEC> struct Nchw {
  static constexpr int DT = DT_F32, PIX = VEC;
  __host__ __device__ static uint32_t items(int S) { return (uint32_t)S * (uint32_t)S / VEC; }
  __host__ __device__ static size_t sample_bytes(int S) { return (size_t)3 * S * S * 4; }
  __device__ __forceinline__ void load(const char* xs, uint32_t t, int S, float* v) {
    const float* x = reinterpret_cast<const float*>(xs);
    const size_t plane = (size_t)S * S;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (VEC == 4) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(x + c * plane + (size_t)t * 4);
#pragma unroll
        for (int p = 0; p < 4; ++p) v[3 * p + c] = a[p];
      } else {
        v[c] = x[c * plane + t];
      }
    }
  }
  __device__ __forceinline__ void store(char* xd, uint32_t t, int S, const float* v) const {
    float* x = reinterpret_cast<float*>(xd);
    const size_t plane = (size_t)S * S;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (VEC == 4)
        *reinterpret_cast<f32x4*>(x + c * plane + (size_t)t * 4) = f32x4{v[c], v[3 + c], v[6 + c], v[9 + c]};
      else
        x[c * plane + t] = v[c];
    }
  }
};

// ---- the point-wise ops: block `blk` of `nblk` strides over the sample's items -------------------
template <class L>
__device__ __forceinline__ void pointwise(const char* xs, char* xd, int S, int op, const Norm3& nm,
                                          uint32_t blk, uint32_t nblk) {
  constexpr int PIX = L::PIX;
  const uint32_t items = L::items(S);
  const float thr = 128.0f / 255.0f;
  for (uint32_t t = blk * NT + threadIdx.x; t < items; t += nblk * NT) {
    L it;
    float v[3 * PIX];
    it.load(xs, t, S, v);
#pragma unroll
    for (int e = 0; e < 3 * PIX; ++e) v[e] = clamp01(v[e] * nm.std[e % 3] + nm.mean[e % 3]);
    if (op == 0) {
#pragma unroll
      for (int p = 0; p < PIX; ++p) {
        const float g = 0.2989f * v[3 * p] + 0.587f * v[3 * p + 1] + 0.114f * v[3 * p + 2];
        v[3 * p] = v[3 * p + 1] = v[3 * p + 2] = g;
      }
    } else if (op == 1) {
#pragma unroll
      for (int e = 0; e < 3 * PIX; ++e) v[e] = v[e] >= thr ? 1.0f - v[e] : v[e];
    }
#pragma unroll
    for (int e = 0; e < 3 * PIX; ++e) v[e] = (v[e] - nm.mean[e % 3]) * nm.istd[e % 3];
    it.store(xd, t, S, v);
  }
}

// ---- a blur tile --------------------------------------------------------------------------------
// the tile's geometry: output pixels [y0, y0 + th) x [x0, x0 + tw); region row r / column q is image
// row by + r / column bx + q, r < th + 22, q < tw + 22; [ya, yb) x [xa, xb) its part inside the image
struct Tile {
  int y0, x0, th, tw, by, bx, ya, yb, xa, xb;
};
__device__ __forceinline__ Tile tile_of(int t, int tiles_x, int S) {
  Tile g;
  g.y0 = (t / tiles_x) * TH;
  g.x0 = (t % tiles_x) * TW;
  g.th = min(TH, S - g.y0);
  g.tw = min(TW, S - g.x0);
  g.by = g.y0 - RMAX;
  g.bx = g.x0 - RMAX;
  g.ya = max(g.by, 0);
  g.xa = max(g.bx, 0);
  g.yb = min(g.y0 + g.th + RMAX, S);
  g.xb = min(g.x0 + g.tw + RMAX, S);
  return g;
}

template <int DT>
__device__ __forceinline__ void stage_in(S2d<DT>, const char* xs, int S, const Tile& g, const Norm3& nm,
                                         float* st) {
  const int ga = g.ya >> 1, gb = (g.yb + 1) >> 1, ha = g.xa >> 1, hb = (g.xb + 1) >> 1;   // S even: <= S/2
  const int gw = hb - ha, n = (gb - ga) * gw, half = S >> 1;
  for (int i = threadIdx.x; i < n; i += NT) {
    const int gi = ga + i / gw, gj = ha + i % gw;
    S2d<DT> it;
    float v[12];
    it.load(xs, (uint32_t)gi * (uint32_t)half + (uint32_t)gj, S, v);
#pragma unroll
    for (int pq = 0; pq < 4; ++pq) {
      const int y = 2 * gi + (pq >> 1), x = 2 * gj + (pq & 1);
      if (y >= g.ya && y < g.yb && x >= g.xa && x < g.xb) {
        float* p = st + (y - g.by) * SS + (x - g.bx);
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c * SP] = clamp01(v[3 * pq + c] * nm.std[c] + nm.mean[c]);
      }
    }
  }
}

template <int VEC>
__device__ __forceinline__ void stage_in(Nchw<VEC>, const char* xs, int S, const Tile& g, const Norm3& nm,
                                         float* st) {
  const float* x = reinterpret_cast<const float*>(xs);
  const int ca = g.xa / VEC, cb = (g.xb + VEC - 1) / VEC;        // VEC 4: S % 4 == 0, so cb <= S / 4
  const int cw = cb - ca, rows = g.yb - g.ya, n = 3 * rows * cw;
  const size_t plane = (size_t)S * S;
  for (int i = threadIdx.x; i < n; i += NT) {
    const int cc = ca + i % cw, t = i / cw, y = g.ya + t % rows, c = t / rows;
    const float sd = pick3(nm.std, c), mn = pick3(nm.mean, c);
    const float* src = x + c * plane + (size_t)y * S + (size_t)cc * VEC;
    float a[VEC];
    if constexpr (VEC == 4) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = q[e];
    } else {
      a[0] = src[0];
    }
    float* p = st + c * SP + (y - g.by) * SS;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const int xx = cc * VEC + e;
      if (xx >= g.xa && xx < g.xb) p[xx - g.bx] = clamp01(a[e] * sd + mn);
    }
  }
}

// Region elements outside the image, from their reflection. Along one axis, with the region
// [b, b + n) of a tile [o, o + t), b = o - 11, n = t + 22, 0 <= o, o + t <= S: an element at -k < 0
// has k <= 11 - o, and k lies in [b, b + n) because b <= 0 < k and k <= 11 <= o + t + 10; an element
// at S - 1 + k, k >= 1, has k <= o + t + 11 - S <= 11 and S - 1 - k >= o - 11 = b because o <= S - 1.
// So the reflection is a region element, and an in-image one (staged, never written here) when
// k <= S - 1; every element within R < S of the image is. Farther ones (only met by weights that are
// 0) become 0.
__device__ __forceinline__ void fill_border(int S, const Tile& g, float* st) {
  const int rows = g.th + 2 * RMAX, cols = g.tw + 2 * RMAX;
  if (g.by >= 0 && g.bx >= 0 && g.by + rows <= S && g.bx + cols <= S) return;      // (uniform)
  for (int i = threadIdx.x; i < rows * cols; i += NT) {
    const int r = i / cols, q = i % cols, y = g.by + r, x = g.bx + q;
    if (y >= 0 && y < S && x >= 0 && x < S) continue;
    const int yy = y < 0 ? -y : (y >= S ? 2 * (S - 1) - y : y);
    const int xx = x < 0 ? -x : (x >= S ? 2 * (S - 1) - x : x);
    const int rr = yy - g.by, qq = xx - g.bx;
    const bool ok = yy >= 0 && yy < S && xx >= 0 && xx < S && rr >= 0 && rr < rows && qq >= 0 && qq < cols;
#pragma unroll
    for (int c = 0; c < 3; ++c) st[c * SP + r * SS + q] = ok ? st[c * SP + rr * SS + qq] : 0.0f;
  }
}

// hm[c][r][x] = sum_k w[|k|] st[c][r][x + 11 + k], k = -11 .. 11 ascending, for the region's rows and
// the tile's columns (rounded up to 8: the surplus is never read)
__device__ __forceinline__ void horizontal(const Tile& g, const float (&w)[RMAX + 1], const float* st,
                                           float* hm) {
  const int rows = g.th + 2 * RMAX, noct = (g.tw + 7) >> 3, n = 3 * rows * noct;
  for (int i = threadIdx.x; i < n; i += NT) {
    const int r = i % rows, t = i / rows, xo = (t % noct) * 8, c = t / noct;
    const float* s = st + c * SP + r * SS + xo;               // reads s[0 .. 29]: xo + 29 <= 53 < SS
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = 0.0f;
#pragma unroll
    for (int j = 0; j < 8 + 2 * RMAX; ++j) {
      const float v = s[j];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int tap = j - k;                                // 0 .. 22: offset tap - 11
        if (tap >= 0 && tap <= 2 * RMAX) a[k] = fmaf(w[tap < RMAX ? RMAX - tap : tap - RMAX], v, a[k]);
      }
    }
    float* h = hm + c * HP + r * HS + xo;
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = a[k];
  }
}

// output rows r0 and r0 + 1 (tile-relative) of the column that starts at hc (= hm + c * HP + x):
// hm rows r0 .. r0 + 23 (r0 + 23 <= 53; row r0 + 23 feeds o1 only)
__device__ __forceinline__ void vertical2(const float* hc, int r0, const float (&w)[RMAX + 1], float& o0,
                                          float& o1) {
  float a0 = 0.0f, a1 = 0.0f;
  const float* p = hc + r0 * HS;
#pragma unroll
  for (int j = 0; j < 2 * RMAX + 2; ++j) {
    const float v = p[j * HS];
    if (j <= 2 * RMAX) a0 = fmaf(w[j < RMAX ? RMAX - j : j - RMAX], v, a0);
    if (j >= 1) a1 = fmaf(w[j - 1 < RMAX ? RMAX - (j - 1) : j - 1 - RMAX], v, a1);
  }
  o0 = a0;
  o1 = a1;
}

template <int DT>
__device__ __forceinline__ void store_out(S2d<DT>, const char* xs, char* xd, int S, const Tile& g,
                                          const Norm3& nm, const float (&w)[RMAX + 1], const float* hm) {
  const int lgi = threadIdx.x / (TW / 2), lgj = threadIdx.x % (TW / 2);     // one group per lane
  if (2 * lgi >= g.th || 2 * lgj >= g.tw) return;                           // (th, tw are even)
  float v[12];
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      vertical2(hm + c * HP + 2 * lgj + q, 2 * lgi, w, v[3 * q + c], v[3 * (2 + q) + c]);
#pragma unroll
  for (int e = 0; e < 12; ++e) v[e] = (v[e] - nm.mean[e % 3]) * nm.istd[e % 3];
  const uint32_t grp = (uint32_t)(g.y0 / 2 + lgi) * (uint32_t)(S >> 1) + (uint32_t)(g.x0 / 2 + lgj);
  S2d<DT> it;
  it.load_pad(xs, grp);
  it.store(xd, grp, S, v);
}

template <int VEC>
__device__ __forceinline__ void store_out(Nchw<VEC>, const char*, char* xd, int S, const Tile& g,
                                          const Norm3& nm, const float (&w)[RMAX + 1], const float* hm) {
  float* x = reinterpret_cast<float*>(xd);
  const size_t plane = (size_t)S * S;
  for (int i = threadIdx.x; i < 3 * (TH / 2) * (TW / 4); i += NT) {         // (c, row pair, 4 pixels)
    const int xq = (i % (TW / 4)) * 4, r0 = ((i / (TW / 4)) % (TH / 2)) * 2, c = i / ((TW / 4) * (TH / 2));
    if (r0 >= g.th || xq >= g.tw) continue;
    float o[2][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) vertical2(hm + c * HP + xq + e, r0, w, o[0][e], o[1][e]);
    const float mn = pick3(nm.mean, c), is = pick3(nm.istd, c);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      float* d = x + c * plane + (size_t)(g.y0 + r0 + p) * S + (g.x0 + xq);
      if constexpr (VEC == 4) {                               // S % 4 == 0: the four pixels are inside
        if (r0 + p < g.th)
          *reinterpret_cast<f32x4*>(d) = f32x4{(o[p][0] - mn) * is, (o[p][1] - mn) * is, (o[p][2] - mn) * is,
                                               (o[p][3] - mn) * is};
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (r0 + p < g.th && xq + e < g.tw) d[e] = (o[p][e] - mn) * is;
      }
    }
  }
}

template <class L>
__global__ __launch_bounds__(NT) void three_aug_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                       const int* __restrict__ table, int B, int S,
                                                       int tiles_x, Norm3 nm) {
  __shared__ float st[3 * SP];
  __shared__ float hm[3 * HP];
  const size_t sbytes = L::sample_bytes(S);
  const int tiles = tiles_x * tiles_x;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int* row = table + (size_t)b * ROW;
    const int op = row[0], R = row[2];
    const char* xs = src + (size_t)b * sbytes;
    char* xd = dst + (size_t)b * sbytes;
    if (op != 2) {
      pointwise<L>(xs, xd, S, op, nm, blockIdx.x, gridDim.x);
      continue;
    }
    float w[RMAX + 1];
#pragma unroll
    for (int d = 0; d <= RMAX; ++d) w[d] = d <= R ? __int_as_float(row[4 + d]) : 0.0f;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
      const Tile g = tile_of(t, tiles_x, S);
      stage_in(L{}, xs, S, g, nm, st);
      __syncthreads();
      fill_border(S, g, st);
      __syncthreads();
      horizontal(g, w, st, hm);
      __syncthreads();
      store_out(L{}, xs, xd, S, g, nm, w, hm);
      __syncthreads();                                        // hm and st are free for the next tile
    }
  }
}

bool norm3(const float* mean, const float* stdev, Norm3& nm) {
  if (mean == nullptr || stdev == nullptr) return false;
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(mean[c]) || !std::isfinite(stdev[c]) || !(stdev[c] > 0.0f)) return false;
    nm.mean[c] = mean[c];
    nm.std[c] = stdev[c];
    nm.istd[c] = 1.0f / stdev[c];
  }
  return true;
}

}  // namespace

extern "C" {

int pda_three_aug_draw(int B, int R, unsigned bkey, int* table, hipStream_t st) {
  if (B <= 0 || R < 1 || R > RMAX || table == nullptr || (uintptr_t)table % 4) return -2;
  TRACKED_LAUNCH(three_aug_draw_kernel, dim3((unsigned)((B + NT - 1) / NT)), dim3(NT), 0, st, B, R,
                 (uint32_t)bkey, table);
  return (int)hipGetLastError();
}

int pda_three_aug(const void* src, void* dst, const int* table, int B, int S, int dt, int layout,
                  const float* mean, const float* stdev, int grid_cap, hipStream_t st) {
  Norm3 nm;
  if (!batch_args_ok(B, S, dt, layout, {src, dst}) || grid_cap < 0 || !norm3(mean, stdev, nm)) return -2;
  if (table == nullptr || (uintptr_t)table % 4) return -2;
  const size_t sbytes = layout == 1 ? Nchw<1>::sample_bytes(S)
                                    : (dt == DT_F32 ? S2d<DT_F32>::sample_bytes(S) : S2d<DT_BF16>::sample_bytes(S));
  const uintptr_t a = (uintptr_t)src, d = (uintptr_t)dst, n = (uintptr_t)B * sbytes;
  if (a < d + n && d < a + n) return -2;                      // the blur reads a neighbourhood
  const int tiles_x = (S + TW - 1) / TW;
  const dim3 grid = batch_grid(B, (long long)tiles_x * tiles_x * NT, grid_cap, NT);
#define THREE_GO(L)                                                                               \
  TRACKED_LAUNCH(three_aug_kernel<L>, grid, dim3(NT), 0, st, (const char*)src, (char*)dst, table, B, S, \
                 tiles_x, nm)
  if (layout == 0 && dt == DT_F32) THREE_GO(S2d<DT_F32>);
  else if (layout == 0 && dt == DT_BF16) THREE_GO(S2d<DT_BF16>);
  else if (layout == 0) THREE_GO(S2d<DT_F16>);
  else if (S % 4 == 0) THREE_GO(Nchw<4>);
  else THREE_GO(Nchw<1>);
#undef THREE_GO
  return (int)hipGetLastError();
}

}  // extern "C"
