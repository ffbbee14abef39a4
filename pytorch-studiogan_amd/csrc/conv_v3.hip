// conv_v3.hip -- dispatcher of the halo kernel (conv_v3.h): 3x3 / stride 1 / pad 1 forward and data gradient, bf16.
#include "conv_common.h"
#include "conv_v3.h"
extern template int sg_conv_v3_dispatch<2>(int, int, const ConvV3Params&, const Epilogue<bf16_t>&, hipStream_t);   // conv_v3b.hip

// halo kernel (conv_v3.h) for 3x3 / stride 1 / pad 1 with >= 64 input channels; returns false when the problem is not eligible.
// SG_CONV_V3=0 disables it, =force skips the tile-count heuristic (tests).
bool sg_conv_fwd_v3_try(const ConvFwdProblem& pb, hipStream_t st) {
  const sg_conv_fwd_desc* d = pb.d;
  const int I = pb.I, J = pb.J, K = pb.K;
  const char mode = env_mode("SG_CONV_V3");
  if (mode == '0') return false;
  const bool force = mode == 'f';
  if (!is_3x3_s1_p1(d) || (pb.pflags & SG_PIX_TRANSPOSED)) return false;
  if (d->C < 64 || d->C % 32 || d->ldx % 8 || !aligned16(d->x) || !aligned16(d->w)) return false;   // slices of 64 channels, the last one whole or half
  if (!pb.out_is_in_times_up()) return false;
  if (pb.wshift < 0 || pb.hshift < 0 || d->Ws < 4 || d->Hs < 2) return false;
  if (pb.xbytes >= (1ll << 31) || pb.wbytes >= (1ll << 30)) return false;      // (weights: a row offset plus a k offset, each marking "out of range" with 2^30)
  if (!epi_bf16_rows_ok(pb.e)) return false;
  int best_tiles = 0;
  int best = cout_tile_search(I, (J + 255) / 256, best_tiles);
  if (I <= 32 && I % 8 == 0 && (J >= 512 * 256 || force)) { best = 32; best_tiles = (J + 511) / 512; }   // narrow outputs (G's RGB layer, 8 padded couts): HBM-bound, one cout tile
  // fewer tiles than CUs: still taken for long reductions (K >= 1152, >= 16 tiles) -- the alternative is the generic engine, whose 128 x 128
  // tiles fill the chip no better and run 3-4x slower per tile (the 1024-channel 8^2 / 4^2 layers of a batch-64 ResNet: 246 us per
  // launch = 78 TFLOP/s in the session-O trace of the WGAN-GP workload)
  if (!best || (best_tiles < 160 && !force && !(K >= 1152 && best_tiles >= 16))) return false;
  // force (tests): take the tile the batch-256 problem gets, so the benchmarked instantiation is the one under test at small batch
  const int BJ = (best == 32 || (best == 96 && (J >= 512 * 256 || (force && J % 512 == 0)))) ? 512 : 256;
  if ((pb.quad || pb.up) && (BJ % (2 * d->Wo))) return false;     // the tile must cover whole (pairs of) image rows
  if (J % d->Wo) return false;
  ConvV3Params p;
  p.x = (const bf16_t*)d->x; p.w = (const bf16_t*)d->w;
  p.W = d->Ws; p.wlog = ilog2_exact(d->Ws); p.C = d->C; p.ldx = d->ldx;
  p.Ho = d->Ho; p.Wo = d->Wo; p.wshift = pb.wshift; p.hshift = pb.hshift; p.flags = pb.pflags;
  p.I = I; p.J = J; p.K = K; p.nslice = (d->C + 63) / 64;
  p.npix_src = d->N * d->Hs * d->Ws;
  p.npx = (pb.up ? BJ / 4 : BJ) + 2 * d->Ws + 16;
  p.xbytes = (unsigned)pb.xbytes; p.wbytes = (unsigned)pb.wbytes;
  p.zero_off = 0; p.bias_off = 0; p.dump_off = 0;
  const bool par = pb.quad && p.wlog >= 4;      // image-row parity in the chunk swizzle: quad row order with W >= 16 (conv_v4.h has the derivation)
  p.pm4 = par ? 4 : 0;
  p.psh = par ? p.wlog - 2 : 0;
  if (((p.npx >> 3) + 7) / 8 >= 19) return false;           // would need more than 2 patch pieces per tap and wave (never with <= 160 KB of LDS)
  const int rc = (d->C % 64 == 0) ? sg_conv_v3_dispatch<4>(best, BJ, p, pb.e, st) : sg_conv_v3_dispatch<2>(best, BJ, p, pb.e, st);
  return rc == 0;
}
template int sg_conv_v3_dispatch<4>(int, int, const ConvV3Params&, const Epilogue<bf16_t>&, hipStream_t);
