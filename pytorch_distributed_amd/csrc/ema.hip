// Weight-EMA kernel for gfx950: one streaming pass over a few (e, p) range pairs of f32 buffers.
//
// A *range* (EmaRange) is an averaged buffer e, the live buffer p it follows, an optional 16-bit
// shadow of p and an element count; the parameters and the BatchNorm statistics are two ranges of
// one launch. The launcher validates the ranges on the host (pda_ema_check), cuts each into chunks
// of at most FLAT_CHUNK (common.h) elements, one workgroup per chunk, and passes the table by value:
// there is no device table to upload, so a launch allocates nothing and copies nothing.
//
//   EMA_LERP : e = fmaf(w, p - e, e) in f32; p is only read. Where p == e the difference is +0 and
//              e keeps its bits (an e of -0 excepted: -0 + +0 = +0); w = 0 keeps e, w = 1 gives
//              e + (p - e), which is p up to the rounding of the difference
//   EMA_COPY : e = p, bit for bit
//   EMA_SWAP : e and p exchange their bits; with a shadow pointer the 16-bit value of what lands in
//              p is written too (the conversions of cast_flat / sgd_flat: torch's cast of p)
//
// COPY and SWAP move 32-bit words, so a range may hold any 4-byte-granular data (the int64
// num_batches_tracked counters ride along as pairs of words). Elements outside every range are
// neither read nor written. No atomics; every element is owned by one lane, so runs repeat bit for bit.
#include "common.h"
#include "pda_api.h"

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace {

constexpr int NT = 256;
constexpr int EMA_MAX_ROWS = 8;    // ranges per launch (the launcher splits longer tables)
enum EmaMode : int { EMA_LERP = 0, EMA_COPY = 1, EMA_SWAP = 2 };

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct EmaRow {
  uint32_t* e;
  uint32_t* p;
  u16* shadow;
  long long count;
  long long blk0;        // the row's blocks: [blk0, blk0 of the next row)
};
struct EmaTable {
  EmaRow rows[EMA_MAX_ROWS];
  int nrows;
};

__device__ __forceinline__ uint32_t ema_lerp(uint32_t e, uint32_t p, float w) {
  const float ef = __uint_as_float(e);
  return __float_as_uint(__builtin_fmaf(w, __uint_as_float(p) - ef, ef));
}

template <int MODE>
__global__ __launch_bounds__(NT) void ema_kernel(const EmaTable t, float w, int dt) {
  // the block's row: the last one whose first block is not past this block (wave-uniform selects
  // over constant indices; the table stays in the kernel arguments)
  EmaRow r = t.rows[0];
#pragma unroll
  for (int k = 1; k < EMA_MAX_ROWS; ++k)
    if (k < t.nrows && (long long)blockIdx.x >= t.rows[k].blk0) r = t.rows[k];
  const long long first = ((long long)blockIdx.x - r.blk0) * FLAT_CHUNK;
  const long long left = r.count - first;
  if (left <= 0) return;   // (the launcher sizes the grid exactly: not reached)
  const int count = left < FLAT_CHUNK ? (int)left : FLAT_CHUNK;
  uint32_t* e = r.e + first;
  uint32_t* p = r.p + first;
  u16* shadow = (MODE == EMA_SWAP && r.shadow) ? r.shadow + first : nullptr;
  const int nv = count >> 2;
  u32x4* e4 = reinterpret_cast<u32x4*>(e);
  u32x4* p4 = reinterpret_cast<u32x4*>(p);
  for (int i = threadIdx.x; i < nv; i += NT) {
    const u32x4 pv = p4[i];
    if constexpr (MODE == EMA_COPY) {
      e4[i] = pv;
    } else if constexpr (MODE == EMA_LERP) {
      u32x4 ev = e4[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) ev[k] = ema_lerp(ev[k], pv[k], w);
      e4[i] = ev;
    } else {
      const u32x4 ev = e4[i];
      e4[i] = pv;
      p4[i] = ev;
      if (shadow) {
        u16 h[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) h[k] = cvt16_rt(__uint_as_float(ev[k]), dt);
        reinterpret_cast<uint2*>(shadow)[i] = *reinterpret_cast<uint2*>(h);
      }
    }
  }
  if ((int)threadIdx.x < (count & 3)) {   // ragged tail of the range's last chunk
    const int i = (nv << 2) + threadIdx.x;
    const uint32_t pv = p[i];
    if constexpr (MODE == EMA_COPY) {
      e[i] = pv;
    } else if constexpr (MODE == EMA_LERP) {
      e[i] = ema_lerp(e[i], pv, w);
    } else {
      const uint32_t ev = e[i];
      e[i] = pv;
      p[i] = ev;
      if (shadow) shadow[i] = cvt16_rt(__uint_as_float(ev), dt);
    }
  }
}

}  // namespace

extern "C" {

int pda_ema_check(const EmaRange* rows, int nrows, int mode, float w, int dt) {
  if (nrows < 0 || (nrows && !rows) || mode < EMA_LERP || mode > EMA_SWAP) return -1;
  if (!std::isfinite(w) || w < 0.f || w > 1.f) return -5;
  std::vector<std::pair<uintptr_t, uintptr_t>> span;   // [begin, end) bytes
  span.reserve(3 * (size_t)nrows);
  long long blocks = 0;
  for (int i = 0; i < nrows; ++i) {
    const EmaRange& r = rows[i];
    if (r.count < 0) return -3;
    if (r.count == 0) continue;   // an empty range is skipped whole (its pointers may be null)
    if (!r.e || !r.p) return -1;
    const bool sh = mode == EMA_SWAP && r.shadow;
    if (sh && dt != DT_BF16 && dt != DT_F16) return -1;
    if (((uintptr_t)r.e & 15) || ((uintptr_t)r.p & 15) || (sh && ((uintptr_t)r.shadow & 7))) return -2;
    blocks += (r.count + FLAT_CHUNK - 1) / FLAT_CHUNK;
    if (blocks > 0x7fffffffLL) return -3;
    span.emplace_back((uintptr_t)r.e, (uintptr_t)r.e + 4 * (uintptr_t)r.count);
    span.emplace_back((uintptr_t)r.p, (uintptr_t)r.p + 4 * (uintptr_t)r.count);
    if (sh) span.emplace_back((uintptr_t)r.shadow, (uintptr_t)r.shadow + 2 * (uintptr_t)r.count);
  }
  std::sort(span.begin(), span.end());
  for (size_t i = 1; i < span.size(); ++i)
    if (span[i - 1].second > span[i].first) return -4;
  return 0;
}

int pda_ema_chunk() { return FLAT_CHUNK; }

int pda_ema(const EmaRange* rows, int nrows, int mode, float w, int dt, hipStream_t st) {
  const int rc = pda_ema_check(rows, nrows, mode, w, dt);
  if (rc) return rc;
  EmaTable t;
  t.nrows = 0;
  long long blocks = 0;
  auto flush = [&]() -> int {
    if (t.nrows == 0) return 0;
    for (int k = t.nrows; k < EMA_MAX_ROWS; ++k) t.rows[k] = EmaRow{nullptr, nullptr, nullptr, 0, blocks};
    const dim3 grid((unsigned)blocks), block(NT);
    if (mode == EMA_LERP) TRACKED_LAUNCH(ema_kernel<EMA_LERP>, grid, block, 0, st, t, w, dt);
    else if (mode == EMA_COPY) TRACKED_LAUNCH(ema_kernel<EMA_COPY>, grid, block, 0, st, t, w, dt);
    else TRACKED_LAUNCH(ema_kernel<EMA_SWAP>, grid, block, 0, st, t, w, dt);
    t.nrows = 0;
    blocks = 0;
    return (int)hipGetLastError();
  };
  for (int i = 0; i < nrows; ++i) {
    const EmaRange& r = rows[i];
    if (r.count == 0) continue;
    t.rows[t.nrows++] = EmaRow{(uint32_t*)r.e, (uint32_t*)r.p, (u16*)r.shadow, r.count, blocks};
    blocks += (r.count + FLAT_CHUNK - 1) / FLAT_CHUNK;
    if (t.nrows == EMA_MAX_ROWS) {
      const int e = flush();
      if (e) return e;
    }
  }
  return flush();
}

}  // extern "C"
