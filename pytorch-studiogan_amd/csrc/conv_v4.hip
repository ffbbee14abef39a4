// conv_v4.hip -- dispatcher of the small-workgroup halo kernel (conv_v4.h): 3x3 / stride 1 / pad 1 forward and data gradient, bf16.
#include "conv_common.h"
#include "conv_v4.h"

// SG_CONV_V4=0 disables it; =force: no minimum tile count (tests: the kernel a batch-256 problem gets, at small batch); =all: in addition
// no channel rule (every eligible shape); default: the short-K layers (C <= 384), which conv_v3.h's one-workgroup-per-CU tiles serve worst.
bool sg_conv_fwd_v4_try(const ConvFwdProblem& pb, hipStream_t st) { return sg_conv_fwd_v4_skip_try(pb, nullptr, st, false); }
bool sg_conv_fwd_v4_skip_try(const ConvFwdProblem& pb, const sg_conv_skip_desc* sk, hipStream_t st, bool dry) {
  const sg_conv_fwd_desc* d = pb.d;
  const int I = pb.I, J = pb.J;
  const bool up = pb.up, quad = pb.quad;
  const char mode = env_mode("SG_CONV_V4");
  if (mode == '0') return false;
  const bool all = mode == 'a', force = all || mode == 'f' || sk != nullptr;   // a fused skip has no other engine to fall to
  if (!is_3x3_s1_p1(d) || (pb.pflags & SG_PIX_TRANSPOSED)) return false;
  if (d->C < 32 || d->C % 32 || d->ldx % 8 || !aligned16(d->x) || !aligned16(d->w)) return false;
  if (!all && !sk && d->C > 384) return false;
  long long x2bytes = 0, w2bytes = 0;
  if (sk) {
    if (up || !sk->x2 || !sk->w2 || sk->C2 < 32 || sk->C2 % 32 || sk->ldx2 % 8 || !aligned16(sk->x2) || !aligned16(sk->w2)) return false;
    if (sk->bias2 && !d->bias) return false;
    if (sk->x2_up && ((d->Ho & 1) || (d->Wo & 1) || quad)) return false;
    const long long npix2 = (long long)d->N * (sk->x2_up ? (d->Ho / 2) * (d->Wo / 2) : d->Ho * d->Wo);
    x2bytes = bf16_extent(npix2, sk->ldx2, sk->C2); w2bytes = (long long)I * sk->C2 * 2;
    if (x2bytes >= (1ll << 31) || w2bytes >= (1ll << 31)) return false;
  }
  if (!pb.out_is_in_times_up()) return false;
  if (pb.wshift < 0 || pb.hshift < 0 || d->Ws < 4 || d->Hs < 2) return false;
  if (pb.xbytes >= (1ll << 31) || pb.wbytes >= (1ll << 31)) return false;      // (weights: one offset per row, bit 31 = "out of range"; conv_v3.h adds two offsets and stops at 2^30)
  if (!epi_bf16_rows_ok(pb.e)) return false;
  const int NB = cout_blocks(I);
  if (!NB) return false;
  // (a 512-pixel tile -- 12 accumulator blocks per wave, two workgroups per CU -- ran no faster than this one in round 2, profiles/r02_conv_layer_table_v4_bj512_q.txt,
  // and again on conv_q.h in round 5: removed)
  const int BJ = 256;
  const int tiles = (I / (32 * NB)) * ((J + BJ - 1) / BJ);
  if (!force && tiles < 768) return false;   // one full wave of workgroups (three per CU)
  if ((quad || up || (sk && sk->x2_up)) && (BJ % (2 * d->Wo))) return false;         // the tile must cover whole pairs of image rows
  if (J % d->Wo) return false;
  const int npx = (((up ? BJ / 4 : BJ) + 2 * d->Ws + 16) + 15) & ~15;
  // the launcher's own limit, asked here so that a dry run is authoritative (the caller no longer swallows a launch failure): operand area + staged epilogue
  // of one workgroup within 80 KiB
  if (sg_conv_v4_lds(NB, npx, nullptr, nullptr, nullptr, sk ? (sk->x2_up ? 3 * 64 * 64 : 2 * 256 * 64) : 0) > 80 * 1024) return false;
  if (dry) return true;
  ConvV4Params p;
  p.x = (const bf16_t*)d->x; p.w = (const bf16_t*)d->w;
  p.W = d->Ws; p.wlog = ilog2_exact(d->Ws); p.C = d->C; p.ldx = d->ldx;
  p.Ho = d->Ho; p.Wo = d->Wo; p.wshift = pb.wshift; p.hshift = pb.hshift; p.flags = pb.pflags;
  p.I = I; p.J = J; p.K = pb.K; p.nslice = d->C / 32;
  p.npix_src = d->N * d->Hs * d->Ws;
  p.npx = npx;
  p.xbytes = (unsigned)pb.xbytes; p.wbytes = (unsigned)pb.wbytes;
  p.wgt_off = p.zero_off = p.bias_off = 0;
  const bool par = quad && p.wlog >= 4;      // image-row parity in the chunk swizzle (conv_v4.h): quad row order with W >= 16
  p.pm2 = par ? 2 : 0;
  p.psh = par ? p.wlog - 1 : 0;
  p.x2 = nullptr; p.w2 = nullptr; p.bias2 = nullptr; p.C2 = p.ldx2 = p.up2 = p.nslice2 = p.npix2 = 0; p.x2bytes = p.w2bytes = 0;
  p.stats = nullptr;
  if (sk) {
    p.stats = (pb.e.flags & SG_EPI_POOL) ? nullptr : sk->stats;     // (tile rows = output rows; the pooled tail of a D block feeds no batch norm)
    p.x2 = (const bf16_t*)sk->x2; p.w2 = (const bf16_t*)sk->w2; p.bias2 = sk->bias2;
    p.C2 = sk->C2; p.ldx2 = sk->ldx2; p.up2 = sk->x2_up ? 1 : 0; p.nslice2 = sk->C2 / 32;
    p.npix2 = d->N * (sk->x2_up ? (d->Ho / 2) * (d->Wo / 2) : d->Ho * d->Wo);
    p.x2bytes = (unsigned)x2bytes; p.w2bytes = (unsigned)w2bytes;
    return (NB == 3 ? sg_launch_conv_v4_skip<3>(p, pb.e, st) : sg_launch_conv_v4_skip<2>(p, pb.e, st)) == 0;
  }
  return (NB == 3 ? sg_launch_conv_v4<3, 2>(p, pb.e, st) : sg_launch_conv_v4<2, 2>(p, pb.e, st)) == 0;
}
