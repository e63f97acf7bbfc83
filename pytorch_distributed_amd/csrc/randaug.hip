// RandAugment for gfx950: torchvision's RandAugment(num_ops = n, magnitude = m, num_magnitude_bins = 31,
// interpolation = NEAREST) on a finished, normalised batch, per sample, before the colour jitter
// (jitter.hip), the random erasing (erase.hip) and the mixing (mix.hip). Built without FMA
// contraction: the order of operations is the source's.
//
// A slot is one of a sample's n successive ops. It reads the whole sample from a source buffer and
// writes it, rounded once to the batch dtype, to ANOTHER buffer (the geometric ops gather, Sharpness
// reads a neighbourhood: neither can run in place); the chain ping-pongs between the loader's batch
// and a persistent second buffer. A step is 2n + 1 launches:
//
//   randaug_draw  : one thread per sample writes its n rows of the int32 table [B][n][8]: word 0 the
//                   op id, word 1 the bits of the float32 factor / threshold or the posterize mask,
//                   words 2..7 the bits of the six float32 affine coefficients (geometric ops; else
//                   0). Counter-based uniforms as erase_draw, slot j takes u(2j) (op = int(u * 14))
//                   and u(2j + 1) (< 0.5: the magnitude is negated), all arithmetic in double and
//                   one rounding to float32. sin / cos of the one angle a run can draw come from the
//                   host. It also zeroes the statistics rows the sample's slots will accumulate into.
//   randaug_stats : once per slot; blocks of a sample whose op is not Contrast, AutoContrast or
//                   Equalize return at once. Equalize: a per-channel histogram of
//                   q = floor(255 x + 0.5) in LDS (3 x 256 uint32, integer LDS atomics), then one
//                   device-scope integer atomic per non-empty bin into the sample's zeroed row.
//                   AutoContrast: per-channel min / max, lane, wave shuffles, then device-scope
//                   integer max on the bits of the non-negative floats (the min as 1.0f's bits minus
//                   the value's, so the zeroed row is its neutral element). Integer counts and float
//                   min / max give the same bits in any order. Contrast: gray summed in DOUBLE,
//                   lane, wave shuffles, LDS, one partial per block into the slab [B][bps]; no
//                   float atomics.
//   randaug_apply : once per slot, source != destination. The sample's row is decoded once into
//                   scalar registers, one uniform branch per op. Contrast: every block sums its
//                   sample's slab row in index order. Equalize: every block rebuilds the three
//                   256-entry LUTs in LDS from the combined histogram (waves 0..2 take a channel
//                   each, four bins per lane, the prefix sum a wave scan). Geometric ops copy stored
//                   values: every element written is a source element's bits or 0.
//
// Work split as batch_jitter: a lane owns whole pixels. s2d [B, S/2, S/2, 16]: one 2x2 pixel group
// per lane, two 16-B chunks (bf16 / f16) or four (f32; the fourth is padding only); NCHW f32: four
// consecutive pixels of each plane when S*S % 4 == 0, else one pixel. Point-wise ops load the owned
// chunks with 16-B loads; the geometric ops and Sharpness fetch source pixels element by element
// through the tile's fetch(): a sample's pixels sit in L2. Stores are 16 B per lane; the s2d padding
// slots of the destination get the source's bits. grid.y walks the samples, grid.x strides over a
// sample's items.
#include <cmath>

#include "batch_image.h"
#include "pda_api.h"

namespace {

constexpr int NT = 256;
constexpr int ROW = 8;               // int32 per table row
constexpr int STAT_ROW = 776;        // 3 x 256 counts, 3 min codes, 3 max bits, 2 unused: 16-B rows
constexpr int ST_MIN = 768, ST_MAX = 771;
constexpr int BPS_MAX = 64;          // most partials per sample: every apply block sums the row
constexpr uint32_t ONE_BITS = 0x3F800000u;

enum RandOp : int {
  IDENTITY = 0, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST,
  SHARPNESS, POSTERIZE, SOLARIZE, AUTOCONTRAST, EQUALIZE, NUM_OPS
};

struct RandDraw {
  uint32_t bkey;
  int n, m, S;
  double ca, sa;                     // cos, sin of the rotation's positive angle
};

__global__ __launch_bounds__(NT) void randaug_draw_kernel(int B, RandDraw d, int* __restrict__ table,
                                                          int* __restrict__ stats) {
  const int b = blockIdx.x * NT + threadIdx.x;
  if (b >= B) return;
  const uint32_t skey = counter_subkey(d.bkey, (uint32_t)b);
  const double k = (double)d.m, S = (double)d.S;
  for (int j = 0; j < d.n; ++j) {
    const int op = (int)(counter_u01(skey, 2u * j) * (double)NUM_OPS);
    const double sgn = counter_u01(skey, 2u * j + 1u) < 0.5 ? -1.0 : 1.0;
    double a[6] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    int w1 = 0;
    if (op == SHEAR_X) a[1] = sgn * (0.3 * k / 30.0);
    else if (op == SHEAR_Y) a[3] = sgn * (0.3 * k / 30.0);
    else if (op == TRANSLATE_X) a[2] = -(sgn * trunc(150.0 / 331.0 * S * k / 30.0));
    else if (op == TRANSLATE_Y) a[5] = -(sgn * trunc(150.0 / 331.0 * S * k / 30.0));
    else if (op == ROTATE) {
      const double c = d.ca, s = sgn * d.sa, h = 0.5 * S;
      a[0] = c;
      a[1] = -s;
      a[2] = h - c * h + s * h;
      a[3] = s;
      a[4] = c;
      a[5] = h - s * h - c * h;
    } else if (op >= BRIGHTNESS && op <= SHARPNESS) w1 = __float_as_int((float)(1.0 + sgn * (0.9 * k / 30.0)));
    else if (op == POSTERIZE) w1 = 0xFF & ~((1 << (int)rint(k / 7.5)) - 1);
    else if (op == SOLARIZE) w1 = __float_as_int((float)((255.0 - 255.0 * k / 30.0) / 255.0));
    int* row = table + ((size_t)b * d.n + j) * ROW;
    const bool geo = op >= SHEAR_X && op <= ROTATE;
    row[0] = op;
    row[1] = w1;
#pragma unroll
    for (int i = 0; i < 6; ++i) row[2 + i] = geo ? __float_as_int((float)a[i]) : 0;
    if (op == AUTOCONTRAST || op == EQUALIZE) {
      i32x4* st = reinterpret_cast<i32x4*>(stats + ((size_t)j * B + b) * STAT_ROW);
      for (int i = 0; i < STAT_ROW / 4; ++i) st[i] = i32x4{0, 0, 0, 0};
    }
  }
}

struct RandNorm {
  float mean[3], std[3], istd[3];
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) {
  return 0.2989f * r + 0.587f * g + 0.114f * b;
}
__device__ __forceinline__ int level_of(float v) { return (int)floorf(255.0f * v + 0.5f); }   // v in [0, 1]

// one stored element as raw bits (a 16-bit one zero-extended) <-> its value
template <int DT> __device__ __forceinline__ float raw_val(uint32_t r) {
  if constexpr (DT == DT_F32) return __uint_as_float(r);
  else return ld16<DT>((u16)r);
}
template <int DT> __device__ __forceinline__ uint32_t raw_of(float f) {
  if constexpr (DT == DT_F32) return __float_as_uint(f);
  else return st16<DT>(f);
}

// ---- what a lane owns: PIX whole pixels as raw elements r[3*p + c], item t of a sample; the s2d
// padding the source held goes to the destination with them. pixel(): where owned pixel p lies;
// fetch(): the raw element (y, x, c) of the sample, in this layout
template <int DT_> struct S2dTile {          // 16-bit: group t = chunks 2t, 2t+1; slots 12..15 in `pad`
  static constexpr int PIX = 4, DT = DT_;
  i32x4 pad;
  __host__ __device__ static uint32_t items(int S) { return (uint32_t)(S / 2) * (uint32_t)(S / 2); }
  __host__ __device__ static size_t sample_bytes(int S) { return (size_t)items(S) * 32; }
  __device__ __forceinline__ void load(const char* xs, uint32_t t, int, uint32_t* r) {
    const i32x4* c = reinterpret_cast<const i32x4*>(xs) + (size_t)t * 2;
    const i32x4 c0 = c[0];
    pad = c[1];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const uint32_t w = (uint32_t)(k < 4 ? c0[k] : pad[k - 4]);
      r[2 * k] = w & 0xFFFFu;
      r[2 * k + 1] = w >> 16;
    }
  }
  __device__ __forceinline__ void store(char* xd, uint32_t t, int, const uint32_t* r) {
    i32x4 c0, c1 = pad;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int w = (int)((r[2 * k] & 0xFFFFu) | (r[2 * k + 1] << 16));
      if (k < 4) c0[k] = w; else c1[k - 4] = w;
    }
    i32x4* c = reinterpret_cast<i32x4*>(xd) + (size_t)t * 2;
    c[0] = c0;
    c[1] = c1;
  }
  __device__ __forceinline__ static void pixel(uint32_t t, int p, int S, int& y, int& x) {
    const uint32_t hs = (uint32_t)S / 2;
    y = 2 * (int)(t / hs) + (p >> 1);
    x = 2 * (int)(t % hs) + (p & 1);
  }
  __device__ __forceinline__ static size_t slot(int S, int y, int x, int c) {
    return ((size_t)(y >> 1) * (size_t)(S >> 1) + (size_t)(x >> 1)) * 16 + (size_t)(((y & 1) * 2 + (x & 1)) * 3 + c);
  }
  __device__ __forceinline__ static uint32_t fetch(const char* xs, int S, int y, int x, int c) {
    return reinterpret_cast<const u16*>(xs)[slot(S, y, x, c)];
  }
};
template <> struct S2dTile<DT_F32> {         // f32: group t = chunks 4t .. 4t+3, the last all padding
  static constexpr int PIX = 4, DT = DT_F32;
  i32x4 pad;
  __host__ __device__ static uint32_t items(int S) { return (uint32_t)(S / 2) * (uint32_t)(S / 2); }
  __host__ __device__ static size_t sample_bytes(int S) { return (size_t)items(S) * 64; }
  __device__ __forceinline__ void load(const char* xs, uint32_t t, int, uint32_t* r) {
    const i32x4* c = reinterpret_cast<const i32x4*>(xs) + (size_t)t * 4;
    const i32x4 a0 = c[0], a1 = c[1], a2 = c[2];
    pad = c[3];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[e] = (uint32_t)a0[e];
      r[4 + e] = (uint32_t)a1[e];
      r[8 + e] = (uint32_t)a2[e];
    }
  }
  __device__ __forceinline__ void store(char* xd, uint32_t t, int, const uint32_t* r) {
    i32x4* c = reinterpret_cast<i32x4*>(xd) + (size_t)t * 4;
    c[0] = i32x4{(int)r[0], (int)r[1], (int)r[2], (int)r[3]};
    c[1] = i32x4{(int)r[4], (int)r[5], (int)r[6], (int)r[7]};
    c[2] = i32x4{(int)r[8], (int)r[9], (int)r[10], (int)r[11]};
    c[3] = pad;
  }
  __device__ __forceinline__ static void pixel(uint32_t t, int p, int S, int& y, int& x) {
    S2dTile<DT_BF16>::pixel(t, p, S, y, x);
  }
  __device__ __forceinline__ static uint32_t fetch(const char* xs, int S, int y, int x, int c) {
    return reinterpret_cast<const uint32_t*>(xs)[S2dTile<DT_BF16>::slot(S, y, x, c)];
  }
};
// NCHW f32, VEC 4 (S*S % 4 == 0: every plane of every sample starts on 16 bytes): pixels 4t .. 4t+3
// of each plane; VEC 1: pixel t, element-wise
template <int VEC> struct NchwTile {
  static constexpr int PIX = VEC, DT = DT_F32;
  __host__ __device__ static uint32_t items(int S) { return (uint32_t)S * (uint32_t)S / VEC; }
  __host__ __device__ static size_t sample_bytes(int S) { return (size_t)3 * S * S * 4; }
  __device__ __forceinline__ void load(const char* xs, uint32_t t, int S, uint32_t* r) {
    const uint32_t* x = reinterpret_cast<const uint32_t*>(xs);
    const size_t plane = (size_t)S * S;
    if constexpr (VEC == 4) {
      i32x4 a[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c] = *reinterpret_cast<const i32x4*>(x + c * plane + (size_t)t * 4);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) r[3 * p + c] = (uint32_t)a[c][p];
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c] = x[c * plane + t];
    }
  }
  __device__ __forceinline__ void store(char* xd, uint32_t t, int S, const uint32_t* r) {
    uint32_t* x = reinterpret_cast<uint32_t*>(xd);
    const size_t plane = (size_t)S * S;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (VEC == 4)
        *reinterpret_cast<i32x4*>(x + c * plane + (size_t)t * 4) =
            i32x4{(int)r[c], (int)r[3 + c], (int)r[6 + c], (int)r[9 + c]};
      else
        x[c * plane + t] = r[c];
    }
  }
  __device__ __forceinline__ static void pixel(uint32_t t, int p, int S, int& y, int& x) {
    const uint32_t i = t * VEC + (uint32_t)p;
    y = (int)(i / (uint32_t)S);
    x = (int)(i % (uint32_t)S);
  }
  __device__ __forceinline__ static uint32_t fetch(const char* xs, int S, int y, int x, int c) {
    return reinterpret_cast<const uint32_t*>(xs)[((size_t)c * S + (size_t)y) * S + (size_t)x];
  }
};

template <class T> __device__ __forceinline__ float unnorm(uint32_t raw, int c, const RandNorm& nm) {
  return clamp01(raw_val<T::DT>(raw) * nm.std[c] + nm.mean[c]);
}

// a lane's items of one sample: for (t ...) over the block's share
#define RANDAUG_ITEMS(t, items) \
  for (uint32_t t = blockIdx.x * NT + threadIdx.x; t < (items); t += gridDim.x * NT)

template <class T>
__global__ __launch_bounds__(NT) void randaug_stats_kernel(const char* __restrict__ x,
                                                           const int* __restrict__ table, int n, int slot,
                                                           uint32_t* __restrict__ stats,
                                                           double* __restrict__ slab, int B, int S,
                                                           RandNorm nm) {
  __shared__ double red[NT / 64];
  __shared__ uint32_t hist[3 * 256];
  constexpr int PIX = T::PIX;
  const uint32_t items = T::items(S);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int op = table[((size_t)b * n + slot) * ROW];
    if (op != CONTRAST && op != AUTOCONTRAST && op != EQUALIZE) continue;
    const char* xs = x + (size_t)b * T::sample_bytes(S);
    uint32_t* st = stats + (size_t)b * STAT_ROW;
    if (op == CONTRAST) {
      double acc = 0.0;
      RANDAUG_ITEMS(t, items) {
        T tile;
        uint32_t r[3 * PIX];
        tile.load(xs, t, S, r);
#pragma unroll
        for (int p = 0; p < PIX; ++p)
          acc += (double)gray_of(unnorm<T>(r[3 * p], 0, nm), unnorm<T>(r[3 * p + 1], 1, nm),
                                 unnorm<T>(r[3 * p + 2], 2, nm));
      }
      const double sum = block_sum_f64<NT>(acc, red);
      if (threadIdx.x == 0) slab[(size_t)b * gridDim.x + blockIdx.x] = sum;
      __syncthreads();                          // red is read by all before the next sample writes it
    } else if (op == AUTOCONTRAST) {
      float lo[3] = {1.0f, 1.0f, 1.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
      RANDAUG_ITEMS(t, items) {
        T tile;
        uint32_t r[3 * PIX];
        tile.load(xs, t, S, r);
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e) {
          const float v = unnorm<T>(r[e], e % 3, nm);
          lo[e % 3] = fminf(lo[e % 3], v);
          hi[e % 3] = fmaxf(hi[e % 3], v);
        }
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          lo[c] = fminf(lo[c], __shfl_xor(lo[c], o, 64));
          hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], o, 64));
        }
        if ((threadIdx.x & 63) == 0) {
          atomicMax(&st[ST_MIN + c], ONE_BITS - __float_as_uint(lo[c]));
          atomicMax(&st[ST_MAX + c], __float_as_uint(hi[c]));
        }
      }
    } else {
      for (int i = threadIdx.x; i < 3 * 256; i += NT) hist[i] = 0;
      __syncthreads();
      RANDAUG_ITEMS(t, items) {
        T tile;
        uint32_t r[3 * PIX];
        tile.load(xs, t, S, r);
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e) atomicAdd(&hist[(e % 3) * 256 + level_of(unnorm<T>(r[e], e % 3, nm))], 1u);
      }
      __syncthreads();
      for (int i = threadIdx.x; i < 3 * 256; i += NT)
        if (hist[i]) atomicAdd(&st[i], hist[i]);
      __syncthreads();                          // hist is read by all before the next sample zeroes it
    }
  }
}

// the point-wise frame of a slot: un-normalise the lane's pixels, op(v, t), re-normalise, one
// rounding. A channel in `keep` (bit c) is left unchanged: an element the clamp leaves alone keeps
// its bits (jitter's rule), a clamped one is re-normalised
template <class T, class F>
__device__ __forceinline__ void randaug_pointwise(const char* xs, char* xd, int S, const RandNorm& nm,
                                                  uint32_t keep, F op) {
  constexpr int E = 3 * T::PIX;
  RANDAUG_ITEMS(t, T::items(S)) {
    T tile;
    uint32_t r[E];
    float v[E];
    tile.load(xs, t, S, r);
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = unnorm<T>(r[e], e % 3, nm);
    op(v, t);
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int c = e % 3;
      if ((keep >> c) & 1u) {
        const float u = raw_val<T::DT>(r[e]) * nm.std[c] + nm.mean[c], cl = clamp01(u);
        if (!(cl == u)) r[e] = raw_of<T::DT>((cl - nm.mean[c]) * nm.istd[c]);
      } else {
        r[e] = raw_of<T::DT>((v[e] - nm.mean[c]) * nm.istd[c]);
      }
    }
    tile.store(xd, t, S, r);
  }
}

// bps: partials per sample in the slab (the stats launch's grid.x)
template <class T>
__global__ __launch_bounds__(NT) void randaug_apply_kernel(const char* __restrict__ src, char* __restrict__ dst,
                                                           const int* __restrict__ table, int n, int slot,
                                                           const uint32_t* __restrict__ stats,
                                                           const double* __restrict__ slab, int bps, int B,
                                                           int S, RandNorm nm) {
  __shared__ float lut[3 * 256];
  __shared__ uint32_t lut_keep[3];
  constexpr int PIX = T::PIX;
  const size_t sbytes = T::sample_bytes(S);
  const uint32_t npix = (uint32_t)S * (uint32_t)S;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int* row = table + ((size_t)b * n + slot) * ROW;
    int op = row[0];
    const float f = __int_as_float(row[1]), omf = 1.0f - f;
    const char* xs = src + (size_t)b * sbytes;
    char* xd = dst + (size_t)b * sbytes;
    const uint32_t* st = stats + (size_t)b * STAT_ROW;
    if (op == SHARPNESS && S <= 2) op = IDENTITY;
    if (op >= SHEAR_X && op <= ROTATE) {
      const float a0 = __int_as_float(row[2]), a1 = __int_as_float(row[3]), a2 = __int_as_float(row[4]);
      const float a3 = __int_as_float(row[5]), a4 = __int_as_float(row[6]), a5 = __int_as_float(row[7]);
      const float fs = (float)S;
      RANDAUG_ITEMS(t, T::items(S)) {
        T tile;
        uint32_t r[3 * PIX];
        tile.load(xs, t, S, r);                 // (for the padding the tile carries)
#pragma unroll
        for (int p = 0; p < PIX; ++p) {
          int y, x;
          T::pixel(t, p, S, y, x);
          const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
          const float u = floorf((a0 * cx + a1 * cy) + a2), v = floorf((a3 * cx + a4 * cy) + a5);
          const bool in = u >= 0.0f && u < fs && v >= 0.0f && v < fs;     // (false for a NaN)
#pragma unroll
          for (int c = 0; c < 3; ++c) r[3 * p + c] = in ? T::fetch(xs, S, (int)v, (int)u, c) : 0u;
        }
        tile.store(xd, t, S, r);
      }
    } else if (op == BRIGHTNESS) {
      randaug_pointwise<T>(xs, xd, S, nm, 0u, [=](float* v, uint32_t) {
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e) v[e] = clamp01(f * v[e]);
      });
    } else if (op == COLOR) {
      randaug_pointwise<T>(xs, xd, S, nm, 0u, [=](float* v, uint32_t) {
#pragma unroll
        for (int p = 0; p < PIX; ++p) {
          const float og = omf * gray_of(v[3 * p], v[3 * p + 1], v[3 * p + 2]);
#pragma unroll
          for (int c = 0; c < 3; ++c) v[3 * p + c] = clamp01(f * v[3 * p + c] + og);
        }
      });
    } else if (op == CONTRAST) {
      double sum = 0.0;
      for (int i = 0; i < bps; ++i) sum += slab[(size_t)b * bps + i];
      const float cm = omf * (float)(sum / (double)npix);
      randaug_pointwise<T>(xs, xd, S, nm, 0u, [=](float* v, uint32_t) {
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e) v[e] = clamp01(f * v[e] + cm);
      });
    } else if (op == SHARPNESS) {
      randaug_pointwise<T>(xs, xd, S, nm, 0u, [=](float* v, uint32_t t) {
#pragma unroll
        for (int p = 0; p < PIX; ++p) {
          int y, x;
          T::pixel(t, p, S, y, x);
          const bool inner = y >= 1 && y < S - 1 && x >= 1 && x < S - 1;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            float blur = v[3 * p + c];
            if (inner) {
              float acc = 0.0f;
#pragma unroll
              for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                  const float w = unnorm<T>(T::fetch(xs, S, y + dy, x + dx, c), c, nm);
                  acc += dy == 0 && dx == 0 ? 5.0f * w : w;
                }
              blur = acc / 13.0f;
            }
            v[3 * p + c] = clamp01(f * v[3 * p + c] + omf * blur);
          }
        }
      });
    } else if (op == POSTERIZE) {
      const int mask = row[1];
      randaug_pointwise<T>(xs, xd, S, nm, 0u, [=](float* v, uint32_t) {
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e) v[e] = (float)(level_of(v[e]) & mask) / 255.0f;
      });
    } else if (op == SOLARIZE) {
      randaug_pointwise<T>(xs, xd, S, nm, 0u, [=](float* v, uint32_t) {
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e) v[e] = v[e] >= f ? 1.0f - v[e] : v[e];
      });
    } else if (op == AUTOCONTRAST) {
      float lo[3], sc[3];
      uint32_t keep = 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lo[c] = __uint_as_float(ONE_BITS - st[ST_MIN + c]);
        const float hi = __uint_as_float(st[ST_MAX + c]);
        if (hi == lo[c]) keep |= 1u << c;
        sc[c] = 1.0f / (hi == lo[c] ? 1.0f : hi - lo[c]);
      }
      randaug_pointwise<T>(xs, xd, S, nm, keep, [=](float* v, uint32_t) {
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e) v[e] = clamp01((v[e] - lo[e % 3]) * sc[e % 3]);
      });
    } else if (op == EQUALIZE) {
      __syncthreads();                          // the previous sample's pixels are done with the LUT
      const int lane = threadIdx.x & 63, ch = threadIdx.x >> 6;
      if (ch < 3) {
        const i32x4 h4 = *reinterpret_cast<const i32x4*>(st + ch * 256 + lane * 4);
        const uint32_t h[4] = {(uint32_t)h4[0], (uint32_t)h4[1], (uint32_t)h4[2], (uint32_t)h4[3]};
        int last = h[3] ? lane * 4 + 3 : h[2] ? lane * 4 + 2 : h[1] ? lane * 4 + 1 : h[0] ? lane * 4 : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
        last = max(last, 0);
        const int li = last & 3;
        const uint32_t at_last = __shfl(li == 0 ? h[0] : li == 1 ? h[1] : li == 2 ? h[2] : h[3], last >> 2, 64);
        const uint32_t step = (npix - min(at_last, npix)) / 255u;
        const uint32_t tot = h[0] + h[1] + h[2] + h[3];
        uint32_t incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const uint32_t up = __shfl_up(incl, o, 64);
          if (lane >= o) incl += up;
        }
        uint32_t before = incl - tot;           // counts in the bins below this lane's first
        if (lane == 0) lut_keep[ch] = step == 0u;
        if (step != 0u) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            lut[ch * 256 + lane * 4 + i] = (float)min(255u, (before + step / 2u) / step) / 255.0f;
            before += h[i];
          }
        }
      }
      __syncthreads();
      const uint32_t keep = lut_keep[0] | lut_keep[1] << 1 | lut_keep[2] << 2;
      const float* lp = lut;
      randaug_pointwise<T>(xs, xd, S, nm, keep, [=](float* v, uint32_t) {
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e)
          if (!((keep >> (e % 3)) & 1u)) v[e] = lp[(e % 3) * 256 + level_of(v[e])];
      });
    } else {                                    // Identity, and any id that names no op
      randaug_pointwise<T>(xs, xd, S, nm, 7u, [](float*, uint32_t) {});
    }
  }
}

uint32_t randaug_items(int S, int layout) {
  if (layout == 0) return S2dTile<DT_F32>::items(S);
  return ((long long)S * S) % 4 == 0 ? NchwTile<4>::items(S) : NchwTile<1>::items(S);
}

size_t batch_bytes(int B, int S, int dt, int layout) {
  if (layout == 0) return (size_t)B * (size_t)(S / 2) * (size_t)(S / 2) * (dt == DT_F32 ? 64 : 32);
  return (size_t)B * 3 * S * S * 4;
}

dim3 stats_grid(int B, int S, int layout, int grid_cap) {
  dim3 g = batch_grid(B, randaug_items(S, layout), grid_cap, NT);
  if (g.x > BPS_MAX) g.x = BPS_MAX;
  return g;
}

bool randaug_norm(const float* mean, const float* stdev, RandNorm& nm) {
  if (mean == nullptr || stdev == nullptr) return false;
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(mean[c]) || !std::isfinite(stdev[c]) || !(stdev[c] > 0.0f)) return false;
    nm.mean[c] = mean[c];
    nm.std[c] = stdev[c];
    nm.istd[c] = 1.0f / stdev[c];
  }
  return true;
}

// what the stats and the apply launchers both refuse; on success nm and the slot's statistics rows
bool randaug_args_ok(int B, int S, int dt, int layout, const int* table, int n, int slot, const int* stats,
                     long long stats_len, const double* slab, long long slab_len, int grid_cap,
                     const float* mean, const float* stdev, RandNorm& nm) {
  if (grid_cap < 0 || n < 1 || n > 4 || slot < 0 || slot >= n || !randaug_norm(mean, stdev, nm)) return false;
  if (table == nullptr || (uintptr_t)table % 4 || stats == nullptr || (uintptr_t)stats % 16) return false;
  if (slab == nullptr || (uintptr_t)slab % 8) return false;
  return stats_len >= (long long)n * B * STAT_ROW &&
         slab_len >= (long long)B * stats_grid(B, S, layout, grid_cap).x;
}

template <bool STATS, class... A>
void randaug_launch(int S, int dt, int layout, dim3 grid, hipStream_t st, A... a) {
#define RANDAUG_GO(T)                                                                             \
  do {                                                                                            \
    if constexpr (STATS) TRACKED_LAUNCH(randaug_stats_kernel<T>, grid, dim3(NT), 0, st, a...);    \
    else TRACKED_LAUNCH(randaug_apply_kernel<T>, grid, dim3(NT), 0, st, a...);                    \
  } while (0)
  if (layout == 0 && dt == DT_F32) RANDAUG_GO(S2dTile<DT_F32>);
  else if (layout == 0 && dt == DT_BF16) RANDAUG_GO(S2dTile<DT_BF16>);
  else if (layout == 0) RANDAUG_GO(S2dTile<DT_F16>);
  else if (((long long)S * S) % 4 == 0) RANDAUG_GO(NchwTile<4>);
  else RANDAUG_GO(NchwTile<1>);
#undef RANDAUG_GO
}

}  // namespace

extern "C" {

int pda_randaug_stat_row() { return STAT_ROW; }

int pda_randaug_draw(int B, int n, int m, int S, unsigned bkey, int* table, int* stats,
                     long long stats_len, hipStream_t st) {
  if (B <= 0 || n < 1 || n > 4 || m < 0 || m > 30 || S < 1 || S > S2D_MAX_SIDE) return -2;
  if (table == nullptr || (uintptr_t)table % 4 || stats == nullptr || (uintptr_t)stats % 16) return -2;
  if (stats_len < (long long)n * B * STAT_ROW) return -2;
  RandDraw d;
  d.bkey = bkey;
  d.n = n;
  d.m = m;
  d.S = S;
  const double a = (30.0 * (double)m / 30.0) * (3.14159265358979323846 / 180.0);
  d.ca = std::cos(a);
  d.sa = std::sin(a);
  TRACKED_LAUNCH(randaug_draw_kernel, dim3((unsigned)((B + NT - 1) / NT)), dim3(NT), 0, st, B, d, table, stats);
  return (int)hipGetLastError();
}

int pda_randaug_bps(int B, int S, int dt, int layout, int grid_cap) {
  const void* aligned = (const void*)16;
  if (!batch_args_ok(B, S, dt, layout, {aligned}) || grid_cap < 0) return -2;
  return (int)stats_grid(B, S, layout, grid_cap).x;
}

int pda_randaug_stats(const void* x, const int* table, int n, int slot, int* stats, long long stats_len,
                      double* slab, long long slab_len, int B, int S, int dt, int layout,
                      const float* mean, const float* stdev, int grid_cap, hipStream_t st) {
  RandNorm nm;
  if (!batch_args_ok(B, S, dt, layout, {x})) return -2;
  if (!randaug_args_ok(B, S, dt, layout, table, n, slot, stats, stats_len, slab, slab_len, grid_cap, mean,
                       stdev, nm))
    return -2;
  randaug_launch<true>(S, dt, layout, stats_grid(B, S, layout, grid_cap), st, (const char*)x, table, n, slot,
                       (uint32_t*)stats + (size_t)slot * B * STAT_ROW, slab, B, S, nm);
  return (int)hipGetLastError();
}

int pda_randaug_apply(const void* src, void* dst, const int* table, int n, int slot, const int* stats,
                      long long stats_len, const double* slab, long long slab_len, int B, int S, int dt,
                      int layout, const float* mean, const float* stdev, int grid_cap, hipStream_t st) {
  RandNorm nm;
  if (!batch_args_ok(B, S, dt, layout, {src, dst})) return -2;
  if (!randaug_args_ok(B, S, dt, layout, table, n, slot, stats, stats_len, slab, slab_len, grid_cap, mean,
                       stdev, nm))
    return -2;
  const uintptr_t s = (uintptr_t)src, d = (uintptr_t)dst, nb = batch_bytes(B, S, dt, layout);
  if (s < d + nb && d < s + nb) return -2;      // the slot gathers: it cannot run in place
  const int bps = (int)stats_grid(B, S, layout, grid_cap).x;
  randaug_launch<false>(S, dt, layout, batch_grid(B, randaug_items(S, layout), grid_cap, NT), st,
                        (const char*)src, (char*)dst, table, n, slot,
                        (const uint32_t*)stats + (size_t)slot * B * STAT_ROW, slab, bps, B, S, nm);
  return (int)hipGetLastError();
}

}  // extern "C"
