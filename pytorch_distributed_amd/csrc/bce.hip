// Sigmoid (binary) cross-entropy on soft targets for gfx950: the loss of the LAMB ResNet recipe
// (timm's BinaryCrossEntropy), the sigmoid sibling of xent_soft (mix.hip).
//
//   bce_soft : one wave per row of the [B, K] f32 logits, forward loss AND gradient against
//              t_k = q_k, or [q_k > thresh] with a threshold, of the project's soft target
//              q_k = eps/K + (1-eps) * (lam*[k==a] + (1-lam)*[k==b]) of two labels per row:
//                l_k  = max(z,0) - z*t_k + log1p(exp(-|z|))
//                dl_k = sigmoid(z) - t_k,  sigmoid from the same e = exp(-|z|)
//              A sigmoid needs no row maximum and no row sum, so loss and gradient come from ONE
//              read of the row. A row holds at most four distinct targets (neither label, a, b,
//              both): they and their thresholded versions are formed once per row on scalars.
//              Aligned rows move 32 B of logits per lane and unit (two 16-B loads, every load of a
//              pass issued before the first is used) and leave as one 16-B store of eight 16-bit
//              gradients, or two of f32. A lane adds its elements in ascending k and one shuffle
//              tree follows: a row's sum has one order, runs repeat bit for bit. No LDS, no atomics.
// Built without FMA contraction: q is the sums and products written here, in this order, and the
// only fused operation is the fmaf spelled out in bce_elem.
#include "common.h"
#include "pda_api.h"

namespace {

constexpr int NT = 256;
constexpr int UPL = 2;     // units (8 logits) per lane and pass: 64 * 2 * 8 = 1024 logits a pass

// the row's targets, in registers: neither label, label a alone, label b alone, a == b
struct RowT {
  float t0, ta, tb, tab;
  int la, lb;
};
__device__ __forceinline__ float target_at(int k, RowT r) {
  const float on_a = k == r.lb ? r.tab : r.ta, off_a = k == r.lb ? r.tb : r.t0;
  return k == r.la ? on_a : off_a;
}

// one element: adds its loss to ``acc``, returns d(loss)/dz unscaled
__device__ __forceinline__ float bce_elem(float z, float t, float& acc) {
  const float e = expf(-fabsf(z));
  acc += fmaf(-z, t, fmaxf(z, 0.f)) + log1pf(e);     // max(z,0) - z*t in one rounding
  return (z >= 0.f ? 1.f : e) / (1.f + e) - t;
}

// four logits at columns k0..k0+3 -> four scaled gradients
__device__ __forceinline__ void bce_chunk(f32x4 z, int k0, RowT r, float sc, float& acc, float* g) {
#pragma unroll
  for (int e = 0; e < 4; ++e) g[e] = bce_elem(z[e], target_at(k0 + e, r), acc) * sc;
}

// VEC: logits rows 16-B aligned (base and ld_in % 4 == 0) and dlog rows 16-B aligned with whole
// 16-B pieces (ld_out % 4 == 0 for f32, % 8 for 16-bit). The launcher decides, never a lane.
template <int DT, bool VEC>
__global__ __launch_bounds__(NT) void bce_soft_kernel(
    const float* __restrict__ logits, int B, int K, int ld_in, const long long* __restrict__ labels,
    const long long* __restrict__ labels_b, float lam, float eps, float thresh, int mode,
    float* __restrict__ loss_rows, void* __restrict__ dlog, int ld_out, float gscale,
    const float* __restrict__ gdev, int want_grad) {
  const int wave = (blockIdx.x * NT + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= B) return;
  const float* x = logits + (size_t)wave * ld_in;
  const int la = (int)labels[wave];
  const float u = eps / (float)K;
  const float wa = (1.f - eps) * lam, wb = (1.f - eps) * (1.f - lam);
  float t0 = u, ta = u + wa, tb = u + wb, tab = u + wa + wb;
  if (thresh >= 0.f) {    // strict, as timm's target.gt(thresh)
    t0 = t0 > thresh ? 1.f : 0.f, ta = ta > thresh ? 1.f : 0.f;
    tb = tb > thresh ? 1.f : 0.f, tab = tab > thresh ? 1.f : 0.f;
  }
  const RowT r{t0, ta, tb, tab, la, labels_b ? (int)labels_b[wave] : la};
  float sc = gscale;
  if (want_grad && gdev) sc *= gdev[0];
  const size_t drow = (size_t)wave * ld_out;
  float acc = 0.f;
  int done = 0;             // columns the vector part has finished
  if constexpr (VEC) {
    const int K4 = K >> 2;              // whole 16-B chunks of the row
    const int NU = (K4 + 1) >> 1;       // units of two chunks; the last may hold one
    const f32x4* xv = reinterpret_cast<const f32x4*>(x);
    for (int u0 = 0; u0 < NU; u0 += 64 * UPL) {
      f32x4 v[UPL][2];
#pragma unroll
      for (int j = 0; j < UPL; ++j) {
        const int c = 2 * (u0 + j * 64 + lane);
        v[j][0] = c < K4 ? xv[c] : f32x4{0.f, 0.f, 0.f, 0.f};
        v[j][1] = c + 1 < K4 ? xv[c + 1] : f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int j = 0; j < UPL; ++j) {
        const int un = u0 + j * 64 + lane;
        const int c = 2 * un;
        if (c >= K4) continue;
        const bool two = c + 1 < K4;
        float g[8];
        bce_chunk(v[j][0], 4 * c, r, sc, acc, g);
        if (two) bce_chunk(v[j][1], 4 * c + 4, r, sc, acc, g + 4);
        if (!want_grad) continue;
        if constexpr (DT == DT_F32) {
          f32x4* o = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(dlog) + drow) + c;
          o[0] = f32x4{g[0], g[1], g[2], g[3]};
          if (two) o[1] = f32x4{g[4], g[5], g[6], g[7]};
        } else {
          u16* o = reinterpret_cast<u16*>(dlog) + drow + 8 * (size_t)un;
          if (two) {
            *reinterpret_cast<i32x4*>(o) = pk8<DT>(g).v;
          } else {
            *reinterpret_cast<uint2*>(o) =
                uint2{pack2<DT>(f32x2{g[0], g[1]}), pack2<DT>(f32x2{g[2], g[3]})};
          }
        }
      }
    }
    done = K4 << 2;
  }
  // the K % 4 tail of an aligned row, or the whole of an unaligned one: one element per lane and
  // step, after the lane's chunks (ascending k)
  for (int k = done + lane; k < K; k += 64) {
    const float g = bce_elem(x[k], target_at(k, r), acc) * sc;
    if (want_grad) st_any(dlog, drow + k, g, DT);
  }
  acc = wave_sum(acc);
  if (lane == 0) loss_rows[wave] = mode == 0 ? acc / (float)K : acc;
  if (!want_grad) return;
  // the engine's fc tile reads the padded rows
  for (int k = K + lane; k < ld_out; k += 64) st_any(dlog, drow + k, 0.f, DT);
}

template <int DT>
void launch(bool vec, int B, hipStream_t st, const float* logits, int K, int ld_in,
            const long long* labels, const long long* labels_b, float lam, float eps, float thresh,
            int mode, float* loss_rows, void* dlog, int ld_out, float gscale, const float* gdev,
            int want_grad) {
  const dim3 grid((B + 3) / 4);
  if (vec)
    TRACKED_LAUNCH((bce_soft_kernel<DT, true>), grid, dim3(NT), 0, st, logits, B, K, ld_in, labels,
                   labels_b, lam, eps, thresh, mode, loss_rows, dlog, ld_out, gscale, gdev, want_grad);
  else
    TRACKED_LAUNCH((bce_soft_kernel<DT, false>), grid, dim3(NT), 0, st, logits, B, K, ld_in, labels,
                   labels_b, lam, eps, thresh, mode, loss_rows, dlog, ld_out, gscale, gdev, want_grad);
}

}  // namespace

extern "C" {

int pda_bce_soft(const float* logits, int B, int K, int ld_in, const long long* labels,
                 const long long* labels_b, float lam, float eps, float thresh, int mode,
                 float* loss_rows, float* loss, void* dlog, int ld_out, float gscale,
                 const float* gdev, int dt, int want_grad, hipStream_t st) {
  if (B < 1 || K < 1 || ld_in < K || !logits || !labels || !loss_rows) return -2;
  if (mode != 0 && mode != 1) return -2;
  if (!(lam >= 0.f && lam <= 1.f) || !(eps >= 0.f && eps < 1.f) || !(thresh < 1.f)) return -2;
  if (dt != DT_F32 && dt != DT_BF16 && dt != DT_F16) return -2;
  if ((want_grad && !dlog) || (dlog && ld_out < K)) return -2;
  // d(mean of loss_rows)/dz: mode 0 the mean over B*K elements, mode 1 over the B rows
  gscale = (float)((double)gscale / (mode == 0 ? (double)B * (double)K : (double)B));
  bool vec = ld_in % 4 == 0 && (uintptr_t)logits % 16 == 0;
  if (want_grad) vec = vec && ld_out % (dt == DT_F32 ? 4 : 8) == 0 && (uintptr_t)dlog % 16 == 0;
  if (dt == DT_F32)
    launch<DT_F32>(vec, B, st, logits, K, ld_in, labels, labels_b, lam, eps, thresh, mode, loss_rows,
                   dlog, ld_out, gscale, gdev, want_grad);
  else if (dt == DT_BF16)
    launch<DT_BF16>(vec, B, st, logits, K, ld_in, labels, labels_b, lam, eps, thresh, mode,
                    loss_rows, dlog, ld_out, gscale, gdev, want_grad);
  else
    launch<DT_F16>(vec, B, st, logits, K, ld_in, labels, labels_b, lam, eps, thresh, mode, loss_rows,
                   dlog, ld_out, gscale, gdev, want_grad);
  if (loss) return pda_mean_rows(loss_rows, B, loss, st);
  return (int)hipGetLastError();
}

}  // extern "C"
