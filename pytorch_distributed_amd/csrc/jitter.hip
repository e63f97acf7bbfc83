// Colour jitter for gfx950: torchvision's ColorJitter(brightness, contrast, saturation, hue) on a
// finished, normalised batch, per sample, before the random erasing (erase.hip) and the mixing
// (mix.hip). Built without FMA contraction: the order of operations is the source's.
//
//   jitter_draw  : one thread per sample writes the sample's row of the int32 table [B][5]: the bits
//                  of four float32 factors (brightness, contrast, saturation, hue) and the op order
//                  packed in nibbles, nibble k = the op at position k (0 brightness, 1 contrast,
//                  2 saturation, 3 hue, 15 = skipped: its strength is 0). Counter-based uniforms
//                  as erase_draw (batch_image.h), in double, on a stream of their own:
//                    skey = counter_subkey(bkey, b),  u(k) = counter_u01(skey, k)
//                  order: Fisher-Yates on (0, 1, 2, 3), for i = 3, 2, 1: j = int(u(3 - i) * (i + 1));
//                  fb = lo + (hi - lo) * u(3), [lo, hi] = [max(0, 1 - b), 1 + b]; fc from u(4), fs
//                  from u(5) alike; fh = -h + 2h * u(6); each rounded once to float32.
//   jitter_mean  : the contrast mean. Per pixel: un-normalise (clamp(x * std + mean, 0, 1)), the ops
//                  ordered before contrast, gray = 0.2989 r + 0.587 g + 0.114 b in f32; the sum in
//                  DOUBLE: lane, wave shuffles, block through LDS, one partial per block into the
//                  slab [B][bps] (bps = grid.x). Fixed order, no atomics.
//   batch_jitter : in place. Every block sums its sample's slab row in index order and forms
//                  m = float(sum / (S*S)): all blocks of a sample hold the same m and runs repeat
//                  bit for bit. Then un-normalise, the ops in the sample's order, re-normalise
//                  ((y - mean) * (1 / std)), one rounding to the batch dtype. A sample with every op
//                  skipped keeps the stored value of each element the clamp leaves alone.
//
// Work split: a lane owns whole pixels, all three channels in registers. s2d [B, S/2, S/2, 16]: one
// 2x2 pixel group per lane (a pixel's channels straddle the 16-B chunks, so the group is the
// smallest unit of whole pixels): two 16-B loads (bf16 / f16) or three (f32: the fourth chunk is
// all padding and is neither loaded nor stored), all issued before the first use; the 16-bit
// padding slots 12..15 go back as they were read. NCHW f32: four consecutive pixels of each plane
// as three 16-B loads when S*S % 4 == 0, else one pixel per lane. grid.y walks the samples, grid.x
// strides over a sample's items. The op order is decoded once per sample into scalar registers; the
// pixel loop reads no table. Ops run op-major (one uniform branch per op, its body unrolled over
// the lane's pixels).
#include <cmath>

#include "batch_image.h"
#include "pda_api.h"

namespace {

constexpr int NT = 256;
constexpr int ROW = 5;              // int32 per table row
constexpr int MEAN_BPS_MAX = 64;    // most partials per sample: every apply block sums the row

struct JitterDraw {
  uint32_t bkey;
  int skip;                         // bit op: the op's strength is 0
  double b, c, s, h;
};

__global__ __launch_bounds__(NT) void jitter_draw_kernel(int B, JitterDraw d, int* __restrict__ table) {
  const int n = blockIdx.x * NT + threadIdx.x;
  if (n >= B) return;
  const uint32_t skey = counter_subkey(d.bkey, (uint32_t)n);
  uint32_t ord = 0x3210u;
  for (int i = 3; i > 0; --i) {
    const int j = (int)(counter_u01(skey, (uint32_t)(3 - i)) * (double)(i + 1));
    const uint32_t ni = (ord >> (4 * i)) & 15u, nj = (ord >> (4 * j)) & 15u;
    ord = (ord & ~(15u << (4 * i)) & ~(15u << (4 * j))) | (ni << (4 * j)) | (nj << (4 * i));
  }
  for (int k = 0; k < 4; ++k)
    if ((d.skip >> ((ord >> (4 * k)) & 15u)) & 1) ord |= 15u << (4 * k);
  const double str[3] = {d.b, d.c, d.s};
  int* row = table + (size_t)n * ROW;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lo = fmax(0.0, 1.0 - str[k]), hi = 1.0 + str[k];
    row[k] = __float_as_int((float)(lo + (hi - lo) * counter_u01(skey, 3u + k)));
  }
  row[3] = __float_as_int((float)(-d.h + 2.0 * d.h * counter_u01(skey, 6u)));
  row[4] = (int)ord;
}

struct JitterNorm {
  float mean[3], std[3], istd[3];
};

// one sample's row, in scalar registers: nibbles above 3 (and contrast, when no mean was taken)
// become 15, so ord == 0xFFFF is "nothing to do"
struct JitterRow {
  float fb, fc, fs, fh;
  uint32_t ord;
  bool contrast;
};
__device__ __forceinline__ JitterRow jitter_row(const int* __restrict__ table, int b, bool with_mean) {
  const int* r = table + (size_t)b * ROW;
  JitterRow j;
  j.fb = __int_as_float(r[0]);
  j.fc = __int_as_float(r[1]);
  j.fs = __int_as_float(r[2]);
  j.fh = __int_as_float(r[3]);
  const uint32_t raw = (uint32_t)r[4];
  j.ord = 0;
  j.contrast = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t op = (raw >> (4 * k)) & 15u;
    if (op > 3u || (op == 1u && !with_mean)) op = 15u;
    j.contrast = j.contrast || op == 1u;
    j.ord |= op << (4 * k);
  }
  return j;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) {
  return 0.2989f * r + 0.587f * g + 0.114f * b;
}

// torchvision's _rgb2hsv, h = (h + fh) mod 1, _hsv2rgb on one pixel of [0, 1] values. Both mods act
// on numbers above -1 with a result in [0, 1]: x - floor(x), exact. The sector selects are
// branch-free; the three divisions by cr share one reciprocal.
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float fh) {
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const float cr = maxc - minc;
  const bool eq = cr == 0.0f;
  const float s = cr / (eq ? 1.0f : maxc);
  const float icr = 1.0f / (eq ? 1.0f : cr);
  const float rc = (maxc - r) * icr, gc = (maxc - g) * icr, bc = (maxc - b) * icr;
  const float h6 = maxc == r ? bc - gc : (maxc == g ? 2.0f + rc - bc : 4.0f + gc - rc);
  float h = h6 / 6.0f + 1.0f;
  h = h - floorf(h);
  h = h + fh;
  h = h - floorf(h);
  const float v = maxc, hs = h * 6.0f, fi = floorf(hs), f = hs - fi;
  const int i = fi >= 6.0f ? 0 : (int)fi;
  const float p = clamp01(v * (1.0f - s));
  const float q = clamp01(v * (1.0f - f * s));
  const float t = clamp01(v * (1.0f - (1.0f - f) * s));
  r = i == 0 ? v : i == 1 ? q : i <= 3 ? p : i == 4 ? t : v;
  g = i == 0 ? t : i <= 2 ? v : i == 3 ? q : p;
  b = i <= 1 ? p : i == 2 ? t : i <= 4 ? v : q;
}

// the sample's ops on PIX un-normalised pixels v[3*p + c], op-major; UNTIL_CONTRAST: the ops ordered
// before contrast only (the mean pass). cm = (1 - fc) * m
template <int PIX, bool UNTIL_CONTRAST>
__device__ __forceinline__ void jitter_ops(float* v, const JitterRow& j, float cm) {
#pragma unroll 1
  for (int k = 0; k < 4; ++k) {
    const uint32_t op = (j.ord >> (4 * k)) & 15u;
    if (op == 0u) {
#pragma unroll
      for (int e = 0; e < 3 * PIX; ++e) v[e] = clamp01(j.fb * v[e]);
    } else if (op == 1u) {
      if constexpr (UNTIL_CONTRAST) return;
#pragma unroll
      for (int e = 0; e < 3 * PIX; ++e) v[e] = clamp01(j.fc * v[e] + cm);
    } else if (op == 2u) {
      const float omf = 1.0f - j.fs;
#pragma unroll
      for (int p = 0; p < PIX; ++p) {
        const float og = omf * gray_of(v[3 * p], v[3 * p + 1], v[3 * p + 2]);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[3 * p + c] = clamp01(j.fs * v[3 * p + c] + og);
      }
    } else if (op == 3u) {
#pragma unroll
      for (int p = 0; p < PIX; ++p) hue_shift(v[3 * p], v[3 * p + 1], v[3 * p + 2], j.fh);
    }
  }
}

// ---- what a lane owns: PIX whole pixels as v[3*p + c], item t of a sample ----------------------
// s2d, 16-bit: group t = chunks 2t, 2t+1; slot 3*p + c = v[3*p + c], slots 12..15 kept in `pad`
template <int DT> struct S2dTile {
  static constexpr int PIX = 4;
  i32x4 pad;
  __host__ __device__ static uint32_t items(int S) { return (uint32_t)(S / 2) * (uint32_t)(S / 2); }
  __host__ __device__ static size_t sample_bytes(int S) { return (size_t)items(S) * 32; }
  __device__ __forceinline__ void load(const char* xs, uint32_t t, int, float* v) {
    const i32x4* c = reinterpret_cast<const i32x4*>(xs) + (size_t)t * 2;
    const i32x4 c0 = c[0];
    pad = c[1];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const f32x2 f = unpack2<DT>((uint32_t)(k < 4 ? c0[k] : pad[k - 4]));
      v[2 * k] = f.x;
      v[2 * k + 1] = f.y;
    }
  }
  __device__ __forceinline__ void store(char* xs, uint32_t t, int, const float* v) {
    i32x4 c0, c1 = pad;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int w = (int)pack2<DT>(f32x2{v[2 * k], v[2 * k + 1]});
      if (k < 4) c0[k] = w; else c1[k - 4] = w;
    }
    i32x4* c = reinterpret_cast<i32x4*>(xs) + (size_t)t * 2;
    c[0] = c0;
    c[1] = c1;
  }
};
// s2d, f32: group t = chunks 4t .. 4t+2; chunk 4t+3 is padding only and stays where it is
template <> struct S2dTile<DT_F32> {
  static constexpr int PIX = 4;
  __host__ __device__ static uint32_t items(int S) { return (uint32_t)(S / 2) * (uint32_t)(S / 2); }
  __host__ __device__ static size_t sample_bytes(int S) { return (size_t)items(S) * 64; }
  __device__ __forceinline__ void load(const char* xs, uint32_t t, int, float* v) {
    const f32x4* c = reinterpret_cast<const f32x4*>(xs) + (size_t)t * 4;
    const f32x4 a0 = c[0], a1 = c[1], a2 = c[2];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = a0[e];
      v[4 + e] = a1[e];
      v[8 + e] = a2[e];
    }
  }
  __device__ __forceinline__ void store(char* xs, uint32_t t, int, const float* v) {
    f32x4* c = reinterpret_cast<f32x4*>(xs) + (size_t)t * 4;
    c[0] = f32x4{v[0], v[1], v[2], v[3]};
    c[1] = f32x4{v[4], v[5], v[6], v[7]};
    c[2] = f32x4{v[8], v[9], v[10], v[11]};
  }
};
// NCHW f32, VEC 4 (S*S % 4 == 0: every plane of every sample starts on 16 bytes): pixels 4t .. 4t+3
// of each plane; VEC 1: pixel t, element-wise
template <int VEC> struct NchwTile {
  static constexpr int PIX = VEC;
  __host__ __device__ static uint32_t items(int S) { return (uint32_t)S * (uint32_t)S / VEC; }
  __host__ __device__ static size_t sample_bytes(int S) { return (size_t)3 * S * S * 4; }
  __device__ __forceinline__ void load(const char* xs, uint32_t t, int S, float* v) {
    const float* x = reinterpret_cast<const float*>(xs);
    const size_t plane = (size_t)S * S;
    if constexpr (VEC == 4) {
      f32x4 a[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) a[c] = *reinterpret_cast<const f32x4*>(x + c * plane + (size_t)t * 4);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int p = 0; p < 4; ++p) v[3 * p + c] = a[c][p];
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = x[c * plane + t];
    }
  }
  __device__ __forceinline__ void store(char* xs, uint32_t t, int S, const float* v) {
    float* x = reinterpret_cast<float*>(xs);
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

template <int PIX> __device__ __forceinline__ void unnormalise(float* v, const JitterNorm& nm) {
#pragma unroll
  for (int e = 0; e < 3 * PIX; ++e) v[e] = clamp01(v[e] * nm.std[e % 3] + nm.mean[e % 3]);
}

template <class T>
__global__ __launch_bounds__(NT) void jitter_mean_kernel(const char* __restrict__ x,
                                                         const int* __restrict__ table,
                                                         double* __restrict__ slab, int B, int S,
                                                         JitterNorm nm) {
  __shared__ double red[NT / 64];
  constexpr int PIX = T::PIX;
  const uint32_t items = T::items(S);
  const size_t sbytes = T::sample_bytes(S);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const JitterRow j = jitter_row(table, b, true);
    double acc = 0.0;
    if (j.contrast) {
      const char* xs = x + (size_t)b * sbytes;
      for (uint32_t t = blockIdx.x * NT + threadIdx.x; t < items; t += gridDim.x * NT) {
        T tile;
        float v[3 * PIX];
        tile.load(xs, t, S, v);
        unnormalise<PIX>(v, nm);
        jitter_ops<PIX, true>(v, j, 0.0f);
#pragma unroll
        for (int p = 0; p < PIX; ++p) acc += (double)gray_of(v[3 * p], v[3 * p + 1], v[3 * p + 2]);
      }
    }
    const double sum = block_sum_f64<NT>(acc, red);
    if (threadIdx.x == 0) slab[(size_t)b * gridDim.x + blockIdx.x] = sum;
    __syncthreads();                            // red is read by all before the next sample writes it
  }
}

// bps: partials per sample in the slab (the mean launch's grid.x); 0: no mean was taken
template <class T>
__global__ __launch_bounds__(NT) void jitter_apply_kernel(char* __restrict__ x,
                                                          const int* __restrict__ table,
                                                          const double* __restrict__ slab, int bps,
                                                          int B, int S, JitterNorm nm) {
  constexpr int PIX = T::PIX;
  const uint32_t items = T::items(S);
  const size_t sbytes = T::sample_bytes(S);
  const double npix = (double)S * (double)S;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const JitterRow j = jitter_row(table, b, bps > 0);
    float cm = 0.0f;
    if (j.contrast) {
      double sum = 0.0;
      for (int i = 0; i < bps; ++i) sum += slab[(size_t)b * bps + i];
      cm = (1.0f - j.fc) * (float)(sum / npix);
    }
    const bool ident = j.ord == 0xFFFFu;
    char* xs = x + (size_t)b * sbytes;
    for (uint32_t t = blockIdx.x * NT + threadIdx.x; t < items; t += gridDim.x * NT) {
      T tile;
      float v[3 * PIX];
      tile.load(xs, t, S, v);
      if (ident) {
        // nothing between the two normalisations: an element the clamp leaves alone keeps its bits
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e) {
          const float u = v[e] * nm.std[e % 3] + nm.mean[e % 3], c = clamp01(u);
          v[e] = c == u ? v[e] : (c - nm.mean[e % 3]) * nm.istd[e % 3];
        }
      } else {
        unnormalise<PIX>(v, nm);
        jitter_ops<PIX, false>(v, j, cm);
#pragma unroll
        for (int e = 0; e < 3 * PIX; ++e) v[e] = (v[e] - nm.mean[e % 3]) * nm.istd[e % 3];
      }
      tile.store(xs, t, S, v);
    }
  }
}

uint32_t jitter_items(int S, int layout) {
  if (layout == 0) return S2dTile<DT_F32>::items(S);
  return ((long long)S * S) % 4 == 0 ? NchwTile<4>::items(S) : NchwTile<1>::items(S);
}

dim3 mean_grid(int B, int S, int layout, int grid_cap) {
  dim3 g = batch_grid(B, jitter_items(S, layout), grid_cap, NT);
  if (g.x > MEAN_BPS_MAX) g.x = MEAN_BPS_MAX;
  return g;
}

bool jitter_norm(const float* mean, const float* stdev, JitterNorm& nm) {
  if (mean == nullptr || stdev == nullptr) return false;
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(mean[c]) || !std::isfinite(stdev[c]) || !(stdev[c] > 0.0f)) return false;
    nm.mean[c] = mean[c];
    nm.std[c] = stdev[c];
    nm.istd[c] = 1.0f / stdev[c];
  }
  return true;
}

// the kernel of the batch's layout and dtype, MEAN or apply, launched with the same arguments
template <bool MEAN, class... A>
void jitter_launch(int S, int dt, int layout, dim3 grid, hipStream_t st, A... a) {
#define JITTER_GO(T)                                                                              \
  do {                                                                                            \
    if constexpr (MEAN) TRACKED_LAUNCH(jitter_mean_kernel<T>, grid, dim3(NT), 0, st, a...);       \
    else TRACKED_LAUNCH(jitter_apply_kernel<T>, grid, dim3(NT), 0, st, a...);                     \
  } while (0)
  if (layout == 0 && dt == DT_F32) JITTER_GO(S2dTile<DT_F32>);
  else if (layout == 0 && dt == DT_BF16) JITTER_GO(S2dTile<DT_BF16>);
  else if (layout == 0) JITTER_GO(S2dTile<DT_F16>);
  else if (((long long)S * S) % 4 == 0) JITTER_GO(NchwTile<4>);
  else JITTER_GO(NchwTile<1>);
#undef JITTER_GO
}

}  // namespace

extern "C" {

int pda_jitter_draw(int B, unsigned bkey, double b, double c, double s, double h, int* table,
                    hipStream_t st) {
  if (B <= 0 || table == nullptr || (uintptr_t)table % 4) return -2;
  if (!std::isfinite(b) || !std::isfinite(c) || !std::isfinite(s) || !std::isfinite(h)) return -2;
  if (b < 0.0 || c < 0.0 || s < 0.0 || h < 0.0 || h > 0.5) return -2;
  JitterDraw d;
  d.bkey = bkey;
  d.skip = (b == 0.0 ? 1 : 0) | (c == 0.0 ? 2 : 0) | (s == 0.0 ? 4 : 0) | (h == 0.0 ? 8 : 0);
  d.b = b;
  d.c = c;
  d.s = s;
  d.h = h;
  TRACKED_LAUNCH(jitter_draw_kernel, dim3((unsigned)((B + NT - 1) / NT)), dim3(NT), 0, st, B, d, table);
  return (int)hipGetLastError();
}

int pda_jitter_bps(int B, int S, int dt, int layout, int grid_cap) {
  const void* aligned = (const void*)16;
  if (!batch_args_ok(B, S, dt, layout, {aligned}) || grid_cap < 0) return -2;
  return (int)mean_grid(B, S, layout, grid_cap).x;
}

int pda_jitter_mean(const void* x, const int* table, double* slab, long long slab_len, int B, int S,
                    int dt, int layout, const float* mean, const float* stdev, int grid_cap,
                    hipStream_t st) {
  JitterNorm nm;
  if (!batch_args_ok(B, S, dt, layout, {x}) || grid_cap < 0 || !jitter_norm(mean, stdev, nm)) return -2;
  if (table == nullptr || (uintptr_t)table % 4 || slab == nullptr || (uintptr_t)slab % 8) return -2;
  const dim3 grid = mean_grid(B, S, layout, grid_cap);
  if (slab_len < (long long)B * grid.x) return -2;
  jitter_launch<true>(S, dt, layout, grid, st, (const char*)x, table, slab, B, S, nm);
  return (int)hipGetLastError();
}

int pda_batch_jitter(void* x, const int* table, const double* slab, long long slab_len, int with_mean,
                     int B, int S, int dt, int layout, const float* mean, const float* stdev,
                     int grid_cap, hipStream_t st) {
  JitterNorm nm;
  if (!batch_args_ok(B, S, dt, layout, {x}) || grid_cap < 0 || !jitter_norm(mean, stdev, nm)) return -2;
  if (table == nullptr || (uintptr_t)table % 4) return -2;
  int bps = 0;
  if (with_mean) {
    if (slab == nullptr || (uintptr_t)slab % 8) return -2;
    bps = (int)mean_grid(B, S, layout, grid_cap).x;
    if (slab_len < (long long)B * bps) return -2;
  }
  const dim3 grid = batch_grid(B, jitter_items(S, layout), grid_cap, NT);
  jitter_launch<false>(S, dt, layout, grid, st, (char*)x, table, slab, bps, B, S, nm);
  return (int)hipGetLastError();
}

}  // extern "C"
