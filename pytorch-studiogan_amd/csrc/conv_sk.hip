// conv_sk.hip -- dispatcher of the small-K streaming kernel (conv_sk.h): 1x1 convolutions with <= 192 channels and the RGB stem, bf16.
#include "conv_common.h"
#include "conv_sk.h"

// small-K streaming kernel (conv_sk.h): 1x1 convolutions with <= 192 input channels and the 3x3 stem over 8 padded channels.
// SG_CONV_SK=0 disables it, =force skips the problem-size heuristic (tests).
bool sg_conv_fwd_sk_try(const ConvFwdProblem& pb, hipStream_t st) {
  const sg_conv_fwd_desc* d = pb.d;
  const Epilogue<bf16_t>& e = pb.e;
  const int I = pb.I, J = pb.J;
  const char mode = env_mode("SG_CONV_SK");
  if (mode == '0') return false;
  const bool force = mode == 'f';
  if (d->stride != 1 || (pb.pflags & SG_PIX_TRANSPOSED)) return false;
  const bool one = d->R == 1 && d->S == 1 && d->pad_h == 0 && d->pad_w == 0 && d->C <= 192;
  const bool stem = is_3x3_s1_p1(d) && d->C == 8 && !pb.up;
  if (!one && !stem) return false;
  if (d->C % 8 || d->ldx % 8 || I % 8 || I > 384 || !aligned16(d->x) || !aligned16(d->w)) return false;
  if (!pb.out_is_in_times_up()) return false;
  if (pb.wshift < 1 || pb.hshift < 1) return false;
  if (pb.xbytes >= (1ll << 31) || J >= (1 << 30)) return false;
  if (!epi_bf16_rows_ok(e) || (e.mask && e.res)) return false;      // (one staged operand tile: mask OR residual)
  if (J < 16384 && !force) return false;
  // output / mask / residual go through buffer descriptors too (32-bit offsets, bit 31 = "no access")
  const long long jout = (e.flags & SG_EPI_POOL) ? (J >> 2) : J;
  const long long obytes = bf16_extent(jout, e.ldo, I);
  const long long sbytes = e.mask ? bf16_extent(jout, e.ldm, I) : (e.res ? bf16_extent(jout, e.ldr, I) : 16);
  const long long pbytes = e.sign_out ? ((jout - 1) * e.lds + ((I + 31) >> 5)) * 4 : 0;      // the result's sign plane: dword rows of pitch lds
  if (obytes >= (1ll << 31) || sbytes >= (1ll << 31) || pbytes >= (1ll << 31)) return false;
  ConvSkParams p;
  p.obytes = (unsigned)obytes; p.sbytes = (unsigned)sbytes; p.pbytes = (unsigned)pbytes;
  p.x = (const bf16_t*)d->x; p.w = (const bf16_t*)d->w;
  p.C = d->C; p.ldx = d->ldx; p.Hs = d->Hs; p.Ws = d->Ws;
  p.Ho = d->Ho; p.Wo = d->Wo; p.wshift = pb.wshift; p.hshift = pb.hshift;
  p.mode3 = stem ? 1 : 0; p.flags = pb.pflags;
  p.I = I; p.J = J; p.K = pb.K; p.xbytes = (unsigned)pb.xbytes; p.nrb = 0;
  return sg_launch_conv_sk(p, e, st) == 0;
}
