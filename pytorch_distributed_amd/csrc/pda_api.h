// The C ABI of libpda_kernels.so, declared once: the structs Python fills and one prototype per
// exported pda_* function. Every csrc/*.hip includes this header, so a definition that disagrees
// with its prototype does not compile (conflicting types for a C-linkage function), and
// ops/ext.py binds ctypes from this text, so there is no second signature table to keep in step.
//
// ops/ext.py reads this file with a few regular expressions, not a C parser. Keep to this style:
//   * one prototype per ';', return type and name at the start of a line, no macros inside it;
//   * every parameter is named, and its type is one of int, unsigned, float, double, long long,
//     unsigned long long, hipStream_t, hipEvent_t, a pointer to one of those, a pointer to void,
//     or a pointer to one of the structs below;
//   * every struct has a ctypes.Structure of the same name in ops/ext.py (BwdArgsC: ext.BwdArgs)
//     and the two static_asserts below it (size, offset of the last field), which
//     tests/test_abi_cpu.py compares with the ctypes layout.
// The structs are used inside kernels: nothing here but plain host-and-device C.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

// ------------------------------------------------------------------ structs
struct ConvDesc {
  int Nb, H, W, Cin, Cout, R, S, stride, pad, Ho, Wo;
};
static_assert(sizeof(ConvDesc) == 44, "ConvDesc");
static_assert(offsetof(ConvDesc, Wo) == 40, "ConvDesc");

// dgrad epilogue = BatchNorm-backward reduction (conv_gemm.hip ConvParams e*)
struct BnEpi {
  int mode, nq;
  const void* y; const float* sc; const float* sh;
  const void* y2; const float* sc2; const float* sh2;
  const void* g2; float* part;
  const void* mask;
};
static_assert(sizeof(BnEpi) == 80, "BnEpi");
static_assert(offsetof(BnEpi, mask) == 72, "BnEpi");

// one queued split-K reduction of pda_wgrad_reduce_batch (host side)
struct RedDescC {
  const float* slab; float* grad; const float* ck; const float* cB; const float* cs;
  int splits, M, N, cin_log2, cin_real, pitch, accumulate;
  float scale;
};
static_assert(sizeof(RedDescC) == 72, "RedDescC");
static_assert(offsetof(RedDescC, scale) == 68, "RedDescC");

// outputs of the one-launch BatchNorm forward statistics (bn.hip bn_stats_kernel<0>)
struct BnFwdOut {
  const float* gamma; const float* beta;
  float eps, momentum;
  float* mean; float* invstd; float* scale; float* shift;
  float* rmean; float* rvar; long long* nbt;
  int update;
  double* tot;   // non-null: f64 totals [2][C] instead of the finalize (bn_finalize_tot after)
};
static_assert(sizeof(BnFwdOut) == 96, "BnFwdOut");
static_assert(offsetof(BnFwdOut, tot) == 88, "BnFwdOut");

// outputs of the one-launch BatchNorm backward finalize (bn.hip bn_stats_kernel<1>);
// branch b = 0: BN of y, 1: shortcut BN of y2
struct BnBwdOut {
  float count, gscale;
  int accumulate;
  const float* gamma[2]; const float* mean[2]; const float* invstd[2];
  float* dgamma[2]; float* dbeta[2];
  float* k;      // [NQ-1][3][C]: dy_b = k0*dz + k1*y_b + k2
};
static_assert(sizeof(BnBwdOut) == 104, "BnBwdOut");
static_assert(offsetof(BnBwdOut, k) == 96, "BnBwdOut");

// arguments of pda_bn_bwd_reduce / pda_bn_bwd_apply (bn.hip BwdArgs without rows_per_block)
struct BwdArgsC {
  const void* g1; const void* g2; const void* gp; int HW;
  const void* y; const float* sc; const float* sh;
  const void* y2; const float* sc2; const float* sh2;
  int mode; void* dz_out;
  float* part; int nq; long long rows; int C;
};
static_assert(sizeof(BwdArgsC) == 128, "BwdArgsC");
static_assert(offsetof(BwdArgsC, C) == 120, "BwdArgsC");

// one parameter tensor's range of the flat buffers and its hyper-parameters (optim.hip)
struct SegRow {
  long long off, numel;
  float lr, momentum, wd, trust, eps;
  int flags;             // bit0 = Nesterov
  int blk0, nblk;        // the segment's blocks: [blk0, blk0 + nblk) of the block table
};
static_assert(sizeof(SegRow) == 48, "SegRow");
static_assert(offsetof(SegRow, nblk) == 44, "SegRow");

// one block's chunk of a segment (optim.hip)
struct BlkRow {
  long long first;       // flat index of the chunk's first element (a multiple of 4)
  int seg, count;
};
static_assert(sizeof(BlkRow) == 16, "BlkRow");
static_assert(offsetof(BlkRow, count) == 12, "BlkRow");

// one (e, p[, shadow]) range of the weight EMA (ema.hip)
struct EmaRange {
  void* e;
  void* p;
  void* shadow;          // 16-bit shadow of p (EMA_SWAP), or null
  long long count;       // elements (4 bytes each)
};
static_assert(sizeof(EmaRange) == 32, "EmaRange");
static_assert(offsetof(EmaRange, count) == 24, "EmaRange");

extern "C" {

// ------------------------------------------------------------------ conv_gemm.hip
// Y[M=Nb*Ho*Wo][Cout] = conv(X, W). W: [Cout][Kpad] 16-bit. stats: [ceil(M/bm)][3][Cout] shifted
// partials or null.
int pda_conv_fwd(const ConvDesc* d, const void* x, const void* w, int Kpad, void* y, int out_f32,
                 int out_pitch, const float* bias, float* stats, int relu, const float* pro_sc,
                 const float* pro_sh, int dt, int bm, int bn, hipStream_t st);
// FWD_TAIL (see the Pass enum): Y = conv(a, W) of a 1x1 stride-1 conv whose input
// a = relu(y3 * sc + sh + r) (mode 1, r = res) or relu(y3 * sc + sh + res * sc2 + sh2) (mode 2) is
// formed while staging; a is written to a_out (and its ReLU bitmask to mask, mode 1, nullable) by
// the first N-tile's blocks. Register-staged single-stage tiles (-128, 64) / (-128, 128).
int pda_conv_fwd_tail(const ConvDesc* d, const void* y3, const void* w, int Kpad, void* y,
                      float* stats, const float* sc, const float* sh, const void* res,
                      const float* sc2, const float* sh2, void* a_out, void* mask, int mode, int dt,
                      int bm, int bn, hipStream_t st);
// dX[Nb,H,W,Cin] = conv_transpose(dY, W). Every dX element is written (zeros where no tap lands).
int pda_conv_dgrad(const ConvDesc* d, const void* dy, const void* w, void* dx, const BnEpi* epi,
                   int dt, int bm, int bn, hipStream_t st);
// DGRAD of a 1x1 conv whose dY = k1*dz + k2*y + k3 is folded (see DGRAD_BNF): dz [Nb,Ho,Wo,Cout];
// wf = [k1 o W ; G] ([Cout + Cin][Cin], pda_bn_fold); xa [Nb,H,W,Cin] the Gram operand (the conv's
// forward input; xa_sc / xa_sh: its BN+ReLU prologue, or null); dbias [Cin] f32. Register-staged
// tiles (-128, 64), (-128, 128), (64, 64), (64, 128); -1 otherwise.
int pda_conv_dgrad_bnf(const ConvDesc* d, const void* dz, const void* wf, void* dx, const BnEpi* epi,
                       const void* xa, const float* xa_sc, const float* xa_sh, const float* dbias,
                       int dt, int bm, int bn, hipStream_t st);
// Wf = [k1 o W ; W^T diag(k2) W] and b = W^T k3 of a 1x1 conv (W [Cout][Cin] 16-bit, k = [k1;k2;k3]
// 3 x Cout f32): the operands of pda_conv_dgrad_bnf. Cout, Cin multiples of 64.
int pda_bn_fold(const void* w, const float* k, int Cout, int Cin, void* wf, float* bias, int dt,
                hipStream_t st);
// As pda_conv_wgrad with dY formed while staging from the BatchNorm backward: dY = k1*dz + k2*y + k3
// (per output channel; the stem: Cout 64). 16-bit, 64x128 tiles only (wider ones spill); -1 otherwise.
int pda_conv_wgrad_bna(const ConvDesc* d, const void* dz, const void* y, const float* k1,
                       const float* k2, const float* k3, const void* x, float* slab, int splits,
                       int k_chunk, const float* pro_sc, const float* pro_sh, int dt, int bm, int bn,
                       hipStream_t st);
// Gram = a^T a and s = sum_p a_p of a = relu(sc*y + sh) (y [Nb,H,W,C] 16-bit; WGRAD_GRAM): slab
// [splits][C + 1][C] -- per split the partial Gram, then the partial column sums as row C (one
// split-K reduce gives both). Tiles (64, 64) two-stage, (-128, 128), (-128, 64); -1 otherwise.
int pda_conv_wgrad_gram(const ConvDesc* d, const void* y, const float* sc, const float* sh,
                        float* slab, int splits, int k_chunk, int dt, int bm, int bn, hipStream_t st);
// B = W Gram (f32 [Cout][C]); W 16-bit [Cout][C], Gram f32 [C][C]. C a multiple of 4.
int pda_fold_bgemm(const void* w, const float* gram, int Cout, int C, float* b, int dt, hipStream_t st);
// slab[splits][Cout][R*S*Cin] partial weight gradients (f32). k_chunk must be a multiple of 64.
int pda_conv_wgrad(const ConvDesc* d, const void* dy, const void* x, float* slab, int splits,
                   int k_chunk, const float* pro_sc, const float* pro_sh, int dt, int bm, int bn,
                   hipStream_t st);
// n (<= 24) split-K reductions of pda_wgrad_reduce's kind, N % 4 == 0 each, in one launch.
int pda_wgrad_reduce_batch(const RedDescC* ds, int n, hipStream_t st);
int pda_wgrad_reduce(const float* slab, float* grad, int splits, int M, int N, int cin_pad_log2,
                     int cin_real, int dst_pitch, float scale, int accumulate, const float* ck,
                     const float* cB, const float* cs, hipStream_t st);

// ------------------------------------------------------------------ bn.hip
// Streaming apply kernels (see StreamCfg): unroll < 0 = auto with -unroll chunks (-1: 4) for
// tensors >= min_mb MiB, 0 = the one-chunk kernels, 1/2/4 = that many chunks for every shape;
// ntm / cap apply to the multi-chunk launches. Returns the previous unroll.
int pda_set_stream_cfg(int unroll, int ntm, int cap, int min_mb);
int pda_slab_reduce(const float* in, int G, int QC, int S, float* out, hipStream_t st);
int pda_bn_finalize_tot(const double* tot, int C, double count, const float* gamma,
                        const float* beta, float eps, float momentum, float* mean, float* invstd,
                        float* scale, float* shift, float* rmean, float* rvar, long long* nbt,
                        int update_running, hipStream_t st);
// Partial statistics -> BatchNorm coefficients in one launch (bn_stats_kernel). slabs: f64 >=
// S * nq * C; cnt: int32 >= ceil(C / 256), zero (and left zero). Returns -2 on a bad shape.
// cg: channels per block group (a power of two in [4, 256]; 0 = 256). Fewer channels per group
// give each channel quad more lanes (SL = 1024 / cg): shorter serial chains in both levels.
int pda_bn_fwd_stats(const float* part, int T, int C, int bm, int M, int S, double* slabs, int* cnt,
                     const BnFwdOut* o, int cg, hipStream_t st);
int pda_bn_bwd_stats(const float* part, int T, int nq, int C, int S, double* slabs, int* cnt,
                     const BnBwdOut* o, int cg, hipStream_t st);
int pda_bn_eval_coeffs(const float* gamma, const float* beta, const float* rm, const float* rv,
                       float eps, int C, float* scale, float* shift, hipStream_t st);
// mask (nullable): one byte per 8 elements, bit e = (output element e > 0) -- lets the backward of an
// identity-shortcut tail skip re-reading the residual to rebuild its ReLU mask.
// pda_bn_apply / pda_bn_bwd_apply / pda_bn_bwd_apply2 work on 8-channel chunks of whole rows: -2
// (nothing launched) for C < 8, C % 8 != 0 or an element count that is no multiple of C.
int pda_bn_apply(const void* y, const float* sc, const float* sh, const void* r2, const float* sc2,
                 const float* sh2, void* out, long long numel, int C, int mode, int relu,
                 void* mask, int dt, hipStream_t st);
int pda_stem_pool(const void* y, const float* sc, const float* sh, void* out, void* arg, int N,
                  int H, int W, int C, int Ho, int Wo, int dt, hipStream_t st);
int pda_maxpool_bwd(const void* dout, const void* dout2, const void* arg, void* din, int N, int H,
                    int W, int C, int Ho, int Wo, int dt, hipStream_t st);
int pda_tail_pool(const void* y, const float* sc, const float* sh, const void* r2, const float* sc2,
                  const float* sh2, void* out, int N, int HW, int C, int mode, int dt,
                  hipStream_t st);
// G = number of partial slabs to write; part must hold G*nq*C floats. -2 (nothing launched) for
// C < 8, C % 8 != 0, C > 2048 that is no multiple of 2048 (the kernel's row passes of 256 chunks
// have no tail check), G <= 0 or rows <= 0.
int pda_bn_bwd_reduce(const BwdArgsC* c, int G, int dt, hipStream_t st);
// stem backward reduce (maxpool gather + ReLU mask + dz store + partials [G][2][C])
int pda_stem_bwd_reduce(const void* dout, const void* dout2, const void* arg, const void* y,
                        const float* sc, const float* sh, void* dz_out, float* part, int G, int N,
                        int H, int W, int C, int Ho, int Wo, int dt, hipStream_t st);
int pda_bn_bwd_finalize(const float* part, int G, int nq, int qy, int C, float count,
                        const float* gamma, const float* mean, const float* invstd, float* dgamma,
                        float* dbeta, float* k1, float* k2, float* k3, float gscale, int accumulate,
                        hipStream_t st);
// Both branches of a downsample tail in one pass (16-bit; -1 for other dtypes): k = [2][3][C].
int pda_bn_bwd_apply2(const void* dz, const void* y, const void* y2, const float* k, void* dy,
                      void* dy2, long long rows, int C, int dt, hipStream_t st);
int pda_bn_bwd_apply(const BwdArgsC* c, const void* dz_in, const void* ysel, const float* k1,
                     const float* k2, const float* k3, void* dy, int dt, hipStream_t st);

// ------------------------------------------------------------------ misc.hip
// Arm (ev != null) / disarm fork tracking of this host thread's launches on stream st (common.h).
int pda_track(hipStream_t st, hipEvent_t ev);
unsigned long long pda_track_count();
// flags: hipEventDisableTiming | optionally hipEventDisableSystemFence (the fork events are only
// waited on by a stream of the same device: an agent-scope release is enough)
int pda_event_create_flags(hipEvent_t* ev, unsigned flags);
int pda_event_record(hipEvent_t ev, hipStream_t st);
int pda_event_destroy(hipEvent_t ev);
int pda_stream_wait_event(hipStream_t st, hipEvent_t ev);
int pda_fork_probe(float* dst, const float* src, int n, hipEvent_t stop, hipStream_t st);
int pda_xent(const float* logits, int B, int K, int ld_in, const long long* labels, float* loss_rows,
             float* loss, void* dlog, int ld_out, float gscale, const float* gdev, int dt,
             int want_grad, hipStream_t st);
// loss = mean(loss_rows) alone: the second launch of pda_xent, for the soft-target loss (mix.hip)
int pda_mean_rows(const float* v, int n, float* out, hipStream_t st);
int pda_topk(const float* logits, int B, int K, int ld, const long long* labels, float* hits,
             hipStream_t st);
int pda_col_sum(const void* x, int rows, int C, int ld, float scale, float* out, int dt,
                int accumulate, hipStream_t st);
int pda_sgd_flat(float* p, float* g, float* buf, void* shadow, long long n, float lr, float momentum,
                 float wd, const float* scale, const float* found_inf, int flags, int dt,
                 hipStream_t st);
int pda_cast_flat(const float* p, void* s, long long n, int dt, hipStream_t st);
int pda_amp_scan(const float* g, long long n, float* found_inf, float* inv, float* scale,
                 int* tracker, int* ws, float growth, float backoff, int interval, hipStream_t st);
int pda_pack_stem(const float* src, void* dst, int Cout, int RS, int Cin, int Cpad, int Kpad, int dt,
                  hipStream_t st);
int pda_synth(const long long* ids, int B, unsigned salt, int num_classes, unsigned* keys,
              long long* labels, int S, void* out, int dt, hipStream_t st);
int pda_synth_s2d(const long long* ids, int B, unsigned salt, int num_classes, unsigned* keys,
                  long long* labels, int S, void* out, int dt, hipStream_t st);
int pda_nchw_to_s2d(const float* x, int B, int C, int S, void* out, int dt, hipStream_t st);
int pda_pack_stem_s2d(const float* src, void* dst, int Cout, int dt, hipStream_t st);
int pda_stem_s2d_grad(const float* gp, float* g, int Cout, int accumulate, hipStream_t st);

// ------------------------------------------------------------------ stem.hip
// y [Nb][H][W][64] = conv4x4/1 (pad 2 top/left) of x [Nb][H][W][16] with w [64][256] (K order
// tap-major, channel-minor), 16-bit; stats (nullable) [Nb*H][3][64] shifted partials per output
// row (W rows of M). Requires H % 4 == 0, W % 16 == 0, W <= 128; returns -1 otherwise.
int pda_stem_fwd(const void* x, const void* w, void* y, float* stats, int Nb, int H, int W,
                 int dt, int grid_cap, hipStream_t st);

// ------------------------------------------------------------------ wgrad_tap.hip
// Split-K weight-gradient slabs of a 3x3 / stride-1 / pad-1 convolution, tap-reuse form:
// slab [splits][Cout][9 Cin] (f32) -- pda_wgrad_reduce sums them like the generic kernel's.
// dy [Nb,H,W,Cout], x [Nb,H,W,Cin] 16-bit; pro_sc / pro_sh: BN+ReLU of a PRE-BatchNorm x (or null).
// kb: padded rows per split (multiple of 64); splits = ceil(Nb (H+2)(W+2) / kb). Cin, Cout multiples
// of 64; W <= 59 (the X ring holds 4 steps + the two halos). Returns -2 on a shape it does not take.
int pda_wgrad_tap(const void* dy, const void* x, float* slab, const float* pro_sc,
                  const float* pro_sh, int Nb, int H, int W, int Cin, int Cout, int kb, int splits,
                  int dt, hipStream_t st);
// The stem's weight-gradient slabs in the tap-reuse form (wgrad_stem_tap_kernel): slab
// [splits][64][16 taps x 16] (f32), summed by pda_wgrad_reduce as the generic kernel's. dz, y
// [Nb,H,W,64], x [Nb,H,W,16] 16-bit, k [3][64]. kb: padded rows per split (multiple of 64);
// splits = ceil(Nb (H+3)(W+3) / kb). W + 3 <= 122 (the X ring holds 4 steps + the forward halo).
int pda_wgrad_stem_tap(const void* dz, const void* y, const float* k, const void* x, float* slab,
                       int Nb, int H, int W, int kb, int splits, int dt, hipStream_t st);

// ------------------------------------------------------------------ augment.hip
// packed: device bytes; ti: device int64 [B][4] = byte offset, H, W, flip; tf: device f64 [B][4] =
// x0, y0, x1, y1; mean / std: HOST float[3]. layout 0: s2d [B][S/2][S/2][16] of dtype dt (16-B
// aligned), 1: NCHW f32. fmt 0: records are HWC RGB (3*H*W bytes); 1: YCbCr 4:2:0 (Y plane, then
// the interleaved half-resolution CbCr plane: H*W + 2*((H+1)/2)*((W+1)/2) bytes). The tables must
// have been validated by the caller (ops/native_ops.py aug_check): the kernel trusts offsets, sizes
// and boxes.
int pda_aug_resize_fmt(const void* packed, const long long* ti, const double* tf, int B, int S,
                       void* out, int dt, int layout, int fmt, const float* mean, const float* std,
                       hipStream_t st);
// ids: device int64 [B], every one in [0, N); index: device int64 [N][4] = byte offset, H, W, label,
// validated on the host when the file was opened (data/packed.py); batch_off: device int64 [B] byte
// offsets that replace the index's (host residency), or null. mode 0: train draw with scale bounds
// s0 <= s1 and ratio bounds r0 <= r1; 1: val box of Resize(resize) -> CenterCrop(S), resize >= S.
// Writes ti [B][4], tf [B][4] (pda_aug_resize_fmt's tables) and labels [B].
int pda_aug_draw(const long long* ids, const long long* index, const long long* batch_off, int B,
                 long long N, unsigned seed, int split_id, unsigned epoch, int mode, int S, int resize,
                 double s0, double s1, double r0, double r1, long long* ti, double* tf,
                 long long* labels, hipStream_t st);

// ------------------------------------------------------------------ optim.hip
// Host-side validation of a segment table and its block table against a flat buffer of n elements.
// 0 = good; otherwise the negative code that ops/native_ops.py turns into a ValueError:
//  -1 counts / pointers, -2 offset not a multiple of 4 or negative, -3 segment empty or past n,
//  -4 overlapping segments, -5 hyper-parameter not finite or negative, -6 block table does not cover
//  every segment exactly once in chunks of at most SEG_CHUNK elements
int pda_seg_check(const SegRow* segs, int nseg, const BlkRow* blks, int nblk, long long n);
int pda_seg_chunk();
// slab: 2 * nblk doubles. *_host tables (SegRow / BlkRow rows) are validated, *_dev tables (the same
// bytes) are read by the kernel.
int pda_seg_norms(const float* p, const float* g, long long n, const void* seg_dev, const void* blk_dev,
                  const void* seg_host, const void* blk_host, int nseg, int nblk, double* slab,
                  hipStream_t st);
int pda_sgd_seg(float* p, const float* g, float* buf, void* shadow, long long n, const void* seg_dev,
                const void* blk_dev, const void* seg_host, const void* blk_host, int nseg, int nblk,
                const double* slab, const float* scale, const float* found_inf, int flags, int dt,
                hipStream_t st);

// ------------------------------------------------------------------ clip.hip
// Host-side validation of a clip launch: blks (nblk BlkRow rows, `seg` unused) against a flat
// gradient of n elements. 0 = good; otherwise the negative code that ops/native_ops.py turns into a
// ValueError: -1 no rows or a missing buffer, -2 a row start negative or no multiple of 4, -3 a row
// ends past n, -4 rows overlap, -5 max_norm not finite or not > 0, -6 a row's count outside
// [1, SEG_CHUNK]
int pda_clip_check(const BlkRow* blks, int nblk, long long n, float max_norm);
// Global L2 norm of the rows' elements of g and torch's clip coefficient, one launch on stream st:
// out[0] = inv * sqrt(sum g^2) (evaluated in double), out[1] = inv * min(1, max_norm / (out[0] +
// 1e-6f)) in single precision, inv = inv_in[0] or 1 (inv_in null); found_inf (nullable) set:
// out[1] = inv. slab: nblk doubles; cnt: one int32, zero (and left zero). The host rows are
// validated first (pda_clip_check); nothing is launched on a bad table.
int pda_grad_clip(const float* g, long long n, const void* blk_dev, const void* blk_host, int nblk,
                  double* slab, int* cnt, float max_norm, const float* inv_in,
                  const float* found_inf, float* out, hipStream_t st);

// ------------------------------------------------------------------ mix.hip
int pda_xent_soft(const float* logits, int B, int K, int ld_in, const long long* labels,
                  const long long* labels_b, float lam, float eps, float* loss_rows, float* loss,
                  void* dlog, int ld_out, float gscale, const float* gdev, int dt, int want_grad,
                  hipStream_t st);
// layout 0 = s2d (dt f32 / bf16 / f16, S even), 1 = NCHW f32. Returns -2 for arguments the kernels
// must never see (the Python wrapper refuses them first, with a message), pointers that are not
// 16-byte aligned among them, in either layout. ``grid_cap``: the most blocks to launch (0: 65536;
// the kernels stride over what a smaller grid leaves) -- the wrapper always passes 0, the tests
// call this entry point with a small cap to make both grid-stride loops iterate at small shapes.
int pda_batch_mix(const void* x, void* out, int B, int S, int dt, int layout, int mode, float lam,
                  float oml, int y1, int y2, int x1, int x2, int grid_cap, hipStream_t st);

// ------------------------------------------------------------------ erase.hip
// Random-erasing boxes of a batch of B SxS images, one launch on stream st: boxes (device int32
// [B][4], 4-byte aligned) row b = (y1, y2, x1, x2), half-open, all zeros when sample b is left alone.
// bkey: the batch's key (erase.py batch_key); p: the probability; s0 <= s1: the scale bounds (>= 0);
// l0 <= l1: the LOGARITHMS of the ratio bounds. Returns -2 and launches nothing for B <= 0, S <= 0,
// S > 32768, p outside [0, 1] or NaN, descending or non-finite bounds, a negative scale bound, or a
// null or misaligned table.
int pda_erase_draw(int B, int S, unsigned bkey, double p, double s0, double s1, double l0, double l1,
                   int* boxes, hipStream_t st);
// x (in place): layout 0 = s2d [B][S/2][S/2][16] (dt f32 / bf16 / f16, S even), 1 = NCHW f32; pixels
// with y1 <= y < y2 and x1 <= x < x2 of sample b's row of boxes (device int32 [B][4], as
// pda_erase_draw writes it; clamped to [0, S] by the kernel, an empty box skipped) become +0.0 in
// all three channels, every other bit stays. Returns -2 for arguments the kernels must never see: x
// not 16-byte or boxes not 4-byte aligned, odd S in layout 0, a dtype other than f32 in layout 1.
// ``grid_cap`` as in pda_batch_mix: the most blocks to launch (0: the natural grid).
int pda_batch_erase(void* x, const int* boxes, int B, int S, int dt, int layout, int grid_cap,
                    hipStream_t st);

// ------------------------------------------------------------------ ema.hip
// Host-side validation of a range table. 0 = good; otherwise the negative code that
// ops/native_ops.py turns into a ValueError:
//  -1 bad row count / mode / shadow dtype, or a null e or p, -2 a range start that is not 16-byte
//  aligned (8-byte for the shadow), -3 a negative count (or more than 2^31 - 1 blocks), -4 two of
//  the e, p and shadow ranges overlap, -5 w not finite or outside [0, 1]
int pda_ema_check(const EmaRange* rows, int nrows, int mode, float w, int dt);
int pda_ema_chunk();
// One pass of `mode` over the ranges, on stream st: the whole table is validated first, then every
// EMA_MAX_ROWS non-empty ranges go out as one launch (the model's two ranges: one launch).
int pda_ema(const EmaRange* rows, int nrows, int mode, float w, int dt, hipStream_t st);

}  // extern "C"
