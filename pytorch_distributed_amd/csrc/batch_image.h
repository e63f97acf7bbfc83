// Shared by the kernels on a finished, model-ready batch of images (mix.hip, erase.hip) and the
// counter-based draws (augment.hip, erase.hip). augment.hip and erase.hip are built without FMA
// contraction and mix.hip with it: nothing here may hold a floating-point a*b+c.
#pragma once
#include "common.h"

#include <initializer_list>

struct PixBox {   // pixels with y1 <= y < y2 and x1 <= x < x2
  int y1, y2, x1, x2;
};

// The s2d layout [B, S/2, S/2, 16] (the stem's 2x2 space-to-depth, misc.hip): pixel group (oi, oj)
// holds 16 slots, slot (2p+q)*3 + c = pixel (2*oi+p, 2*oj+q), channel c; slots 12..15 are padding
// (0 by the layout's contract). A lane moves one 16-B chunk of EPC elements, 4 (f32) or 8 (bf16 /
// f16): a group is S2D_CPG chunks and chunk ci holds slots [ci*EPC, (ci+1)*EPC).
template <int EPC> constexpr int S2D_CPG = 16 / EPC;                   // chunks per pixel group
template <int EPC> constexpr uint32_t S2D_FULL = (1u << EPC) - 1;      // every element of a chunk

// bit e: element e of chunk ci of group (oi, oj) is a pixel inside the box (never a padding slot)
template <int EPC>
__device__ __forceinline__ uint32_t s2d_box_mask(int oi, int oj, uint32_t ci, const PixBox& bx) {
  uint32_t slots = 0;                           // 12 bits: slot k inside the box
#pragma unroll
  for (int pq = 0; pq < 4; ++pq) {
    const int yy = 2 * oi + (pq >> 1), xx = 2 * oj + (pq & 1);
    if (yy >= bx.y1 && yy < bx.y2 && xx >= bx.x1 && xx < bx.x2) slots |= 7u << (3 * pq);
  }
  return (slots >> (ci * EPC)) & S2D_FULL<EPC>;
}

// Counter-based uniforms (host mirrors: erase.py, tests/erase_refs.py, tests/packed_refs.py): the
// key of stream n under ``key``, and uniform number k of a key: an integer times 2^-32, exact
__device__ __forceinline__ uint32_t counter_subkey(uint32_t key, uint32_t n) {
  return hash32(key ^ (n * 0x9E3779B9u + 0x85EBCA6Bu));
}
__device__ __forceinline__ double counter_u01(uint32_t key, uint32_t k) {
  return (double)hash32(key ^ ((k + 1u) * 0x27D4EB2Fu)) * (1.0 / 4294967296.0);
}

constexpr int S2D_MAX_SIDE = 32768;    // a sample's 16-B chunks (and a box's) stay below 2^31
constexpr int NCHW_MAX_SIDE = 26000;   // 3*S*S < 2^31

// what every batch launcher refuses: an empty batch, a side out of range or odd in s2d, a dtype the
// layout does not take (0: s2d f32 / bf16 / f16; 1: NCHW f32), a null or misaligned tensor
inline bool batch_args_ok(int B, int S, int dt, int layout, std::initializer_list<const void*> tensors) {
  if (B < 1 || S < 1 || S > S2D_MAX_SIDE) return false;
  for (const void* t : tensors)
    if (t == nullptr || (uintptr_t)t % 16) return false;
  if (layout == 0) return S % 2 == 0 && (dt == DT_F32 || dt == DT_BF16 || dt == DT_F16);
  return layout == 1 && dt == DT_F32 && S <= NCHW_MAX_SIDE;
}

// grid.y walks the samples, grid.x strides over the ``items`` of one sample, ``nt`` per block, at
// most ``grid_cap`` blocks in all (0: 65536). ``total_want`` > 0 also holds grid.x to
// max(total_want / grid.y, 8): for a launcher that cannot know how many of the items are live.
inline dim3 batch_grid(int B, long long items, int grid_cap, int nt, long long total_want = 0) {
  const int blocks = grid_cap > 0 && grid_cap < 65536 ? grid_cap : 65536;
  const int gy = B < blocks ? (B < 65535 ? B : 65535) : (blocks < 65535 ? blocks : 65535);
  long long gx = (items + nt - 1) / nt, cap = blocks / gy;
  const long long want = total_want / gy < 8 ? 8 : total_want / gy;
  if (total_want > 0 && cap > want) cap = want;
  if (cap < 1) cap = 1;
  return dim3((unsigned)(gx < 1 ? 1 : (gx > cap ? cap : gx)), (unsigned)gy);
}
