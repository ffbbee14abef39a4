// conv_common.h -- helpers shared by the convolution translation units (conv.hip: forward API + tile kernels, conv_v3.hip: halo
// kernel, conv_sk.hip: streaming kernel, conv_wgrad.hip: weight gradient). One translation unit per kernel family keeps
// `make -j` at the longest single family (~1.5 min) instead of their sum.
#pragma once
#include <stdlib.h>
#include <type_traits>
#include "gemm_core.h"
#include "../../include/sgamd.h"

static inline int ilog2_exact(int v) {
  if (v <= 0 || (v & (v - 1))) return -1;
  int s = 0;
  while ((1 << s) < v) s++;
  return s;
}
static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

template <typename T>
static void fill_geom(PixGeom<T>& g, const void* x, int N, int Hs, int Ws, int C, int ldx, int Ho, int Wo, int R, int S,
                      int stride, int pad_h, int pad_w, int flags) {
  g.x = (const T*)x; g.N = N; g.Hs = Hs; g.Ws = Ws;
  const int up = (flags & SG_PIX_UPSAMPLE) ? 2 : 1;
  g.Hin = Hs * up; g.Win = Ws * up; g.C = C; g.ldx = ldx; g.Ho = Ho; g.Wo = Wo;
  g.R = R; g.S = S; g.stride = stride; g.pad_h = pad_h; g.pad_w = pad_w; g.flags = flags;
  g.vec_ok = (C % ET<T>::VEC == 0) && (ldx % ET<T>::VEC == 0) && aligned16(x);
  g.wshift = ilog2_exact(Wo); g.hshift = ilog2_exact(Ho);
}

// ---- what the engine dispatchers (conv.hip, conv_<family>.hip, conv_q.hip, conv_wgrad.hip) ask of a problem -------------------------
// first character of an environment switch, 0 when unset (read per call: the tests flip these inside one process)
static inline char env_mode(const char* name) { const char* m = getenv(name); return m ? m[0] : 0; }

// bytes a buffer descriptor must span for npix bf16 pixel rows of C channels at row stride ld (offsets with bit 31 set read as "out of range")
static inline long long bf16_extent(long long npix, int ld, int C) { return ((npix - 1) * ld + C) * 2; }

template <typename D> static inline bool is_3x3_s1_p1(const D* d) { return d->R == 3 && d->S == 3 && d->stride == 1 && d->pad_h == 1 && d->pad_w == 1; }

// 32-cout accumulator blocks per workgroup of the small-workgroup kernels (conv_v4.h, conv_q.h, wgrad_v3.h, wgrad_q.h): 3, 2, or 0 = not served
static inline int cout_blocks(int Cout) { return Cout % 96 == 0 ? 3 : Cout % 64 == 0 ? 2 : 0; }

// cout tile of the 256-pixel tile kernels (conv_v2.h, conv_v3.h): the candidate that divides I and gives the most tiles, the first one with >= 512
// tiles outright. 0 = none divides I. (A 256-wide cout tile puts part of its 128 accumulator registers in scratch with hipcc 7.2: left out)
static const int kCoutTiles[3] = {192, 128, 96};
static inline int cout_tile_search(int I, int tj, int& best_tiles) {
  int best = 0;
  best_tiles = 0;
  for (int c = 0; c < 3; c++) {
    if (I % kCoutTiles[c]) continue;
    const int tiles = (I / kCoutTiles[c]) * tj;
    if (tiles >= 512) { best = kCoutTiles[c]; best_tiles = tiles; break; }
    if (tiles > best_tiles) { best = kCoutTiles[c]; best_tiles = tiles; }
  }
  return best;
}

// tile table of the generic engine's forward / data-gradient launches (conv.hip, modconv.hip): I = couts, J = output pixels
template <typename T, class LP, class LQ, int SPLIT, class EPI = Epilogue<T>>
static void conv_fwd_tiles(const LP& lp, const LQ& lq, const EPI& e, int I, int J, int K, hipStream_t st) {
  if (I <= 32) sg_launch_gemm<T, LP, LQ, 32, 256, 1, 4, true, SPLIT, EPI>(lp, lq, e, I, J, K, 1, 1, st);
  else if (I % 128 != 0 && (I % 96 == 0 || (I < 128 && I > 64))) sg_launch_gemm<T, LP, LQ, 96, 256, 1, 4, true, SPLIT, EPI>(lp, lq, e, I, J, K, 1, 1, st);
  else sg_launch_gemm<T, LP, LQ, 128, 128, 2, 2, true, SPLIT, EPI>(lp, lq, e, I, J, K, 1, 1, st);
}

// D: sg_conv_fwd_desc or sg_convq_desc
template <typename T, typename D> static Epilogue<T> make_epilogue(const D* d, int I, int J) {
  Epilogue<T> e;
  e.out = d->out; e.out_bstride = 0; e.ldo = d->ldo; e.bias = d->bias;
  e.res = d->res; e.res_bstride = 0; e.ldr = d->ldr; e.beta = d->beta;
  e.mask = (const T*)d->mask; e.mask_bstride = 0; e.ldm = d->ldm; e.split_stride = 0;
  e.alpha = d->alpha; e.alpha_ptr = d->alpha_ptr; e.flags = d->epi_flags & ~SG_EPI_PLANES; e.I = I; e.J = J;
  // sign planes: the trailing descriptor fields are read only behind SG_EPI_PLANES (a caller built against the shorter descriptor never sets it).
  // A plane the kernels cannot address (bf16 only; dword rows; fewer words than channels) is dropped here: the launch then runs as if it had not been given.
  const bool planes = std::is_same_v<T, bf16_t> && (d->epi_flags & SG_EPI_PLANES);
  const int nw = (I + 31) >> 5;
  const bool mb = planes && d->mask && d->mask_bits && d->ldmb >= nw && !((uintptr_t)d->mask_bits & 3);
  const bool so = planes && d->sign_out && d->lds >= nw && !((uintptr_t)d->sign_out & 3);
  e.mask_bits = mb ? (const uint32_t*)d->mask_bits : nullptr; e.ldmb = mb ? d->ldmb : 0;
  e.sign_out = so ? (uint32_t*)d->sign_out : nullptr; e.lds = so ? d->lds : 0;
  return e;
}
// sign-plane bookkeeping of a forward / data-gradient launch (sg_sign_plane_launches): epilogue_planes = the engine that took the problem ends in
// sg_conv_epilogue (conv_v2 / v3 / v4 / v4 skip / quad), which reads and writes planes; the streaming kernel (conv_sk.h) writes them but reads the activation
extern long long g_sg_sign_plane_launches[3];
static inline void sg_sign_plane_count(const Epilogue<bf16_t>& e, bool epilogue_planes, bool writes_only = false) {      // writes_only: conv_sk (a producer, not a consumer)
  if (e.sign_out && (epilogue_planes || writes_only)) __atomic_fetch_add(&g_sg_sign_plane_launches[0], 1, __ATOMIC_RELAXED);
  if (e.mask) __atomic_fetch_add(&g_sg_sign_plane_launches[(e.mask_bits && epilogue_planes) ? 1 : 2], 1, __ATOMIC_RELAXED);
}
// the only epilogue of the tile / halo / streaming / quad kernels (sg_conv_epilogue): bf16 rows, 16-byte stores; the ReLU-mask and the residual tile (bf16)
// are pre-staged with 16-byte loads (both together: the mask tile is condensed to register bits, then the residual tile is staged)
static inline bool epi_bf16_rows_ok(const Epilogue<bf16_t>& e) {
  if ((e.flags & (SG_EPI_ATOMIC | SG_EPI_OUT_F32)) || (e.ldo & 7) || !aligned16(e.out)) return false;
  if (e.mask && ((e.ldm & 7) || !aligned16(e.mask))) return false;
  if (e.res && ((e.flags & SG_EPI_RES_F32) || (e.ldr & 7) || !aligned16(e.res))) return false;
  return true;
}

// one bf16 forward / data-gradient problem as every fast path sees it; built once per call (conv.hip), so a `*_try` holds only what ITS kernel adds
struct ConvFwdProblem {
  const sg_conv_fwd_desc* d;
  Epilogue<bf16_t> e;
  int I, J, K, pflags;             // couts, output pixels, R * S * C; pix_flags with SG_PIX_QUAD following SG_EPI_POOL
  bool up, quad;
  int wshift, hshift;              // log2 of Wo / Ho, -1 when not a power of two
  long long xbytes, wbytes;        // descriptor extents of the activation and the filter image
  bool out_is_in_times_up() const { return d->Ho == d->Hs * (up ? 2 : 1) && d->Wo == d->Ws * (up ? 2 : 1); }
};
static inline ConvFwdProblem conv_fwd_problem(const sg_conv_fwd_desc* d, const Epilogue<bf16_t>& e, int I, int J, int K, int pflags) {
  ConvFwdProblem pb;
  pb.d = d; pb.e = e; pb.I = I; pb.J = J; pb.K = K; pb.pflags = pflags;
  pb.up = (pflags & SG_PIX_UPSAMPLE) != 0; pb.quad = (pflags & SG_PIX_QUAD) != 0;
  pb.wshift = ilog2_exact(d->Wo); pb.hshift = ilog2_exact(d->Ho);
  pb.xbytes = bf16_extent((long long)d->N * d->Hs * d->Ws, d->ldx, d->C); pb.wbytes = (long long)I * K * 2;
  return pb;
}

// the bf16 fast paths living in their own translation units; false = not eligible (the caller falls through to the next engine)
bool sg_conv_fwd_sk_try(const ConvFwdProblem& pb, hipStream_t st);   // conv_sk.hip
bool sg_conv_fwd_rs_try(const ConvFwdProblem& pb, hipStream_t st);   // conv_rs.hip
bool sg_conv_fwd_v4_try(const ConvFwdProblem& pb, hipStream_t st);   // conv_v4.hip
bool sg_conv_fwd_v3_try(const ConvFwdProblem& pb, hipStream_t st);   // conv_v3.hip
// sk != nullptr: the fused 1x1 skip (conv_v4.h SKIP); dry: eligibility only, nothing is launched
bool sg_conv_fwd_v4_skip_try(const ConvFwdProblem& pb, const sg_conv_skip_desc* sk, hipStream_t st, bool dry);
