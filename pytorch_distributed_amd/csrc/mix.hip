// Soft-target loss and batch mixing for gfx950: label smoothing, mixup and CutMix.
//
//   xent_soft  : the soft-target sibling of xent_kernel (misc.hip): one wave per row of the
//                [B, classes] f32 logits, forward loss AND gradient against the target distribution
//                q_k = eps/K + (1-eps) * (lam*[k==a] + (1-lam)*[k==b]) of two labels per row
//   batch_mix  : out[b] = mix(x[b], x[(b-1) mod B]) of a finished batch, out of place (sample b's
//                partner is the row above it, torchvision's roll(1, 0): in place it would read rows
//                already overwritten). mode 0 = mixup (lam*x + (1-lam)*partner in f32, one
//                rounding), mode 1 = CutMix (pixels inside the box take the partner's bits: a
//                select, no arithmetic). Layouts: the stem's 2x2 space-to-depth [B, S/2, S/2, 16]
//                (f32 / bf16 / f16, misc.hip) and NCHW f32 [B, 3, S, S]. 16 B per lane, no LDS,
//                no atomics; a lane whose chunk lies wholly on one side of the box loads only
//                that side.
#include "batch_image.h"
#include "pda_api.h"

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void xent_soft_kernel(
    const float* __restrict__ logits, int B, int K, int ld_in, const long long* __restrict__ labels,
    const long long* __restrict__ labels_b, float lam, float eps, float* __restrict__ loss_rows,
    void* __restrict__ dlog, int ld_out, float gscale, const float* __restrict__ gdev, int dt,
    int want_grad) {
  const int wave = (blockIdx.x * NT + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= B) return;
  const float* x = logits + (size_t)wave * ld_in;
  float m = -INFINITY;
  for (int k = lane; k < K; k += 64) m = fmaxf(m, x[k]);
  m = wave_max(m);
  // s = sum exp(x - m); c = sum (x - m): shifted, so its rounding does not grow with a common
  // offset of the logits (sum x = c + K*m)
  float s = 0.f, c = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float d = x[k] - m;
    s += __expf(d);
    c += d;
  }
  s = wave_sum(s);
  c = wave_sum(c);
  const float lse = m + __logf(s);
  const int la = (int)labels[wave];
  const int lb = labels_b ? (int)labels_b[wave] : la;
  const float u = eps / (float)K;
  const float wa = (1.f - eps) * lam, wb = (1.f - eps) * (1.f - lam);
  // sum_k q_k x_k; (eps/K) * sum x = u*c + eps*m. With eps = 0, lam = 1 this is x[la] exactly.
  if (lane == 0) loss_rows[wave] = lse - (wa * x[la] + wb * x[lb] + (u * c + eps * m));
  if (!want_grad) return;
  const float inv = 1.f / s;
  if (gdev) gscale *= gdev[0];
  const size_t drow = (size_t)wave * ld_out;
  for (int k = lane; k < ld_out; k += 64) {
    float g = 0.f;
    if (k < K) {
      const float q = u + (k == la ? wa : 0.f) + (k == lb ? wb : 0.f);
      g = (__expf(x[k] - m) * inv - q) * gscale;
    }
    st_any(dlog, drow + k, g, dt);
  }
}

// ------------------------------------------------------------------ batch mixing
// 16 B of any dtype as f32 (4 or 8 elements), mixed, rounded once
template <int DT> __device__ __forceinline__ i32x4 mix16(i32x4 a, i32x4 b, float lam, float oml) {
  if constexpr (DT == DT_F32) {
    const f32x4 fa = __builtin_bit_cast(f32x4, a), fb = __builtin_bit_cast(f32x4, b);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = lam * fa[e] + oml * fb[e];
    return __builtin_bit_cast(i32x4, o);
  } else {
    Raw8<DT> ra, rb;
    ra.v = a;
    rb.v = b;
    float fa[8], fb[8], o[8];
    cvt8<DT>(ra, fa);
    cvt8<DT>(rb, fb);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = lam * fa[e] + oml * fb[e];
    return pk8<DT>(o).v;
  }
}

// element e of the chunk takes b's bits where bit e of ``em`` is set
template <int DT> __device__ __forceinline__ i32x4 select16(i32x4 a, i32x4 b, uint32_t em) {
  if constexpr (DT == DT_F32) {
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = (em >> e) & 1 ? b[e] : a[e];
    return a;
  } else {
    s16x8 ha = __builtin_bit_cast(s16x8, a);
    const s16x8 hb = __builtin_bit_cast(s16x8, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) ha[e] = (em >> e) & 1 ? hb[e] : ha[e];
    return __builtin_bit_cast(i32x4, ha);
  }
}

// one 16-B chunk: mixup, or the select with only the needed side(s) loaded. ``em``: the chunk's
// elements inside the box; ``full``: every element of a chunk
template <int DT>
__device__ __forceinline__ i32x4 mix_chunk(const i32x4* pa, const i32x4* pb, int mode, float lam,
                                           float oml, uint32_t em, uint32_t full) {
  if (mode == 0) return mix16<DT>(*pa, *pb, lam, oml);
  if (em == 0) return *pa;
  if (em == full) return *pb;
  return select16<DT>(*pa, *pb, em);
}

// s2d [B, S2, S2, 16] (batch_image.h): grid.y walks the samples, grid.x strides over one sample's
// 16-B chunks. The padding slots follow the chunk's source like any other slot.
template <int DT>
__global__ __launch_bounds__(NT) void mix_s2d_kernel(const i32x4* __restrict__ x,
                                                     i32x4* __restrict__ out, int B, int S2, int mode,
                                                     float lam, float oml, PixBox bx) {
  constexpr int EPC = DT == DT_F32 ? 4 : 8;     // elements per chunk
  constexpr int CPG = S2D_CPG<EPC>;
  constexpr uint32_t FULL = S2D_FULL<EPC>;
  const uint32_t cpi = (uint32_t)S2 * S2 * CPG;   // chunks per sample (S2D_MAX_SIDE: < 2^31)
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int pb = b == 0 ? B - 1 : b - 1;
    const i32x4* xa = x + (size_t)b * cpi;
    const i32x4* xb = x + (size_t)pb * cpi;
    i32x4* o = out + (size_t)b * cpi;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < cpi; i += gridDim.x * NT) {
      uint32_t em = 0;
      if (mode == 1) {
        const uint32_t g = i / CPG, ci = i % CPG;
        const int oi = (int)(g / (uint32_t)S2), oj = (int)(g - (uint32_t)oi * S2);
        em = s2d_box_mask<EPC>(oi, oj, ci, bx);
        // a chunk whose pixels all lie in the box comes whole from the partner, padding included
        if (em == ((0x0FFFu >> (ci * EPC)) & FULL) && em != 0) em = FULL;
      }
      o[i] = mix_chunk<DT>(xa + i, xb + i, mode, lam, oml, em, FULL);
    }
  }
}

// NCHW f32 [B, 3, S, S] with S % 4 == 0: a chunk = 4 pixels of one row
__global__ __launch_bounds__(NT) void mix_nchw_vec_kernel(const i32x4* __restrict__ x,
                                                          i32x4* __restrict__ out, int B, int S,
                                                          int mode, float lam, float oml, PixBox bx) {
  const uint32_t cpr = (uint32_t)S / 4;            // chunks per row
  const uint32_t cpi = 3u * S * cpr;               // chunks per sample
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int pb = b == 0 ? B - 1 : b - 1;
    const i32x4* xa = x + (size_t)b * cpi;
    const i32x4* xb = x + (size_t)pb * cpi;
    i32x4* o = out + (size_t)b * cpi;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < cpi; i += gridDim.x * NT) {
      uint32_t em = 0;
      if (mode == 1) {
        const uint32_t row = i / cpr;              // c*S + y
        const int x0 = (int)(i - row * cpr) * 4;
        const int yy = (int)(row % (uint32_t)S);
        if (yy >= bx.y1 && yy < bx.y2) {
#pragma unroll
          for (int e = 0; e < 4; ++e) em |= (x0 + e >= bx.x1 && x0 + e < bx.x2) ? 1u << e : 0u;
        }
      }
      o[i] = mix_chunk<DT_F32>(xa + i, xb + i, mode, lam, oml, em, 15u);
    }
  }
}

// NCHW f32, any S: one element per lane (rows of S % 4 != 0 floats are not 16-B aligned)
__global__ __launch_bounds__(NT) void mix_nchw_scalar_kernel(const float* __restrict__ x,
                                                             float* __restrict__ out, int B, int S,
                                                             int mode, float lam, float oml,
                                                             PixBox bx) {
  const uint32_t epi = 3u * S * S;                 // elements per sample (launcher: < 2^31)
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int pb = b == 0 ? B - 1 : b - 1;
    const float* xa = x + (size_t)b * epi;
    const float* xb = x + (size_t)pb * epi;
    float* o = out + (size_t)b * epi;
    for (uint32_t i = blockIdx.x * NT + threadIdx.x; i < epi; i += gridDim.x * NT) {
      if (mode == 0) {
        o[i] = lam * xa[i] + oml * xb[i];
      } else {
        const uint32_t row = i / (uint32_t)S;
        const int xx = (int)(i - row * S), yy = (int)(row % (uint32_t)S);
        const bool in = yy >= bx.y1 && yy < bx.y2 && xx >= bx.x1 && xx < bx.x2;
        o[i] = in ? xb[i] : xa[i];
      }
    }
  }
}

}  // namespace

extern "C" {

int pda_xent_soft(const float* logits, int B, int K, int ld_in, const long long* labels,
                  const long long* labels_b, float lam, float eps, float* loss_rows, float* loss,
                  void* dlog, int ld_out, float gscale, const float* gdev, int dt, int want_grad,
                  hipStream_t st) {
  TRACKED_LAUNCH(xent_soft_kernel, dim3((B + 3) / 4), dim3(NT), 0, st, logits, B, K, ld_in, labels,
                 labels_b, lam, eps, loss_rows, dlog, ld_out, gscale, gdev, dt, want_grad);
  if (loss) return pda_mean_rows(loss_rows, B, loss, st);
  return (int)hipGetLastError();
}

int pda_batch_mix(const void* x, void* out, int B, int S, int dt, int layout, int mode, float lam,
                  float oml, int y1, int y2, int x1, int x2, int grid_cap, hipStream_t st) {
  if (!batch_args_ok(B, S, dt, layout, {x, out}) || x == out || grid_cap < 0) return -2;
  if (mode != 0 && mode != 1) return -2;
  if (mode == 1 && !(0 <= y1 && y1 <= y2 && y2 <= S && 0 <= x1 && x1 <= x2 && x2 <= S)) return -2;
  const PixBox bx{y1, y2, x1, x2};
  auto grid = [&](long long items) { return batch_grid(B, items, grid_cap, NT); };
  if (layout == 0) {
    const int S2 = S / 2;
    const long long cpi = (long long)S2 * S2 * (dt == DT_F32 ? 4 : 2);
    const i32x4* xi = (const i32x4*)x;
    i32x4* oi = (i32x4*)out;
    if (dt == DT_F32)
      TRACKED_LAUNCH(mix_s2d_kernel<DT_F32>, grid(cpi), dim3(NT), 0, st, xi, oi, B, S2, mode, lam, oml, bx);
    else if (dt == DT_BF16)
      TRACKED_LAUNCH(mix_s2d_kernel<DT_BF16>, grid(cpi), dim3(NT), 0, st, xi, oi, B, S2, mode, lam, oml, bx);
    else
      TRACKED_LAUNCH(mix_s2d_kernel<DT_F16>, grid(cpi), dim3(NT), 0, st, xi, oi, B, S2, mode, lam, oml, bx);
  } else {
    if (S % 4 == 0)
      TRACKED_LAUNCH(mix_nchw_vec_kernel, grid(3LL * S * (S / 4)), dim3(NT), 0, st, (const i32x4*)x,
                     (i32x4*)out, B, S, mode, lam, oml, bx);
    else
      TRACKED_LAUNCH(mix_nchw_scalar_kernel, grid(3LL * S * S), dim3(NT), 0, st, (const float*)x,
                     (float*)out, B, S, mode, lam, oml, bx);
  }
  return (int)hipGetLastError();
}

}  // extern "C"
