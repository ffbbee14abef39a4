// attn_proj.hip -- the projection front end of the self-attention block (reference src/utils/ops.py:83-91) as ONE launch per direction, bf16.
//
// The block reads its input x four times (theta, phi, g, residual). As separate launches the three 1x1 projections each stream x from HBM,
// phi and g go out at full resolution only to be read back by the 2x2 max-pools, and on the way back three chained data-gradient launches each
// read and re-write an x-sized running sum after two un-pool launches have written full-resolution, three-quarters-zero gradients. Here
//   * k_attn_proj_fwd reads x ONCE and writes theta [B,HW,Dp], pooled phi [B,HW/4,Dp], pooled g [B,HW/4,Cg] and the two argmax planes;
//     full-resolution phi and g exist only in a wave-private LDS tile
//   * k_attn_proj_bwd reads the incoming residual gradient once and writes dx = res + W_theta^T dtheta + W_phi^T unpool(dphi) + W_g^T unpool(dg)
//     ONCE; the un-pooling is a select on load from the pooled gradient and the argmax plane
// Both are conv_sk.h's streaming structure: the (concatenated) weight image sits in LDS for the life of the workgroup, a wave owns row blocks of
// 32 pixels in QUAD order (row = window << 2 | dy << 1 | dx, so a row block is 8 whole pooling windows and the pooled index of a window is
// row >> 2), a lane fetches its own MFMA B fragments (pixel lane & 31, k-half lane >> 5) with 16-byte buffer loads that return zeros out of range,
// the loads of the next row block are issued before the MFMAs of this one, and the epilogue runs on a wave-private staging tile.
// Numerics of the forward: the contraction over C is the same v_mfma_f32_32x32x16_bf16 sequence in ascending k from a zero accumulator as
// sg_conv_sk_kernel's, and each projection is rounded to bf16 BEFORE the maximum is taken by the code of k_maxpool2_fwd<bf16_t, true> (elementwise.hip) (first maximum in
// (dy, dx) row-major order wins), so theta, the pooled values and the argmax planes are bit-identical to the three-launch path's.
// The data gradient rounds once (fp32 sum of the residual and all three products) where the chained launches rounded three times.
#include <stdlib.h>
#include "common.h"
#include "../../include/sgamd.h"

namespace {

constexpr unsigned OOR = 0x80000000u;      // buffer offset past every extent: loads return zeros, stores are dropped

typedef short s16x2_t __attribute__((ext_vector_type(2)));

// pixel of quad-ordered row `row`: linear NHWC pixel index
__device__ __forceinline__ unsigned quad_pixel(int row, int H, int W, int wshift, int hshift) {
  const int qd = row >> 2, dy = (row >> 1) & 1, dx = row & 1;
  const int wq = qd & ((W >> 1) - 1);
  const int t = qd >> (wshift - 1);
  const int hq = t & ((H >> 1) - 1);
  const int n = t >> (hshift - 1);
  return (unsigned)(n * H + 2 * hq + dy) * (unsigned)W + (unsigned)(2 * wq + dx);
}

struct ApFwdParams {
  const bf16_t* x; const bf16_t* wt; const bf16_t* wp; const bf16_t* wg;      // x [B,H,W,ldx]; forward images [Dp][C], [Dp][C], [Cg][C]
  bf16_t* theta; bf16_t* phi; bf16_t* g; uint8_t* iphi; uint8_t* ig;
  int C, ldx, H, W, wshift, hshift, J, relu, nrb;
  unsigned xbytes, tbytes, pbytes, gbytes;
};

// DP8 / CG8: 16-byte chunks of a theta (= phi) / g row; KS: 16-wide k-steps (C <= 16 KS)
template <int DP8, int CG8, int KS, int NW>
__global__ __launch_bounds__(64 * NW) void k_attn_proj_fwd(ApFwdParams p) {
  constexpr int I = (2 * DP8 + CG8) * 8;      // concatenated output rows: theta | phi | g
  constexpr int NT = (I + 31) / 32;
  constexpr int WP = KS * 32 + 16;            // weight row pitch in LDS (odd multiple of 16 bytes)
  constexpr int SP = NT * 64 + 16;            // staging row pitch
  constexpr int PCH = DP8 + CG8;              // pooled 16-byte chunks per window
  constexpr int NITT = (32 * DP8 + 63) / 64, NITP = (8 * PCH + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wsm = smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* const stg = smem + NT * 32 * WP + wave * (32 * SP);

  // ---- the three weight images, one under the other -> LDS (once) ---------------------------------------------------------------
  for (int idx = tid; idx < NT * 32 * 2 * KS; idx += 64 * NW) {
    const int row = idx / (2 * KS), c = idx - row * (2 * KS);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < I && c * 8 < p.C) {
      const bf16_t* src = row < DP8 * 8 ? p.wt + (long long)row * p.C : row < DP8 * 16 ? p.wp + (long long)(row - DP8 * 8) * p.C : p.wg + (long long)(row - DP8 * 16) * p.C;
      v = *(const u32x4*)(src + c * 8);
    }
    *(u32x4*)(wsm + row * WP + c * 16) = v;
  }
  __syncthreads();

  const auto rsx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.xbytes, 0x00020000);
  const auto rst = __builtin_amdgcn_make_buffer_rsrc((void*)p.theta, 0, (int)p.tbytes, 0x00020000);
  const auto rsp = __builtin_amdgcn_make_buffer_rsrc((void*)p.phi, 0, (int)p.pbytes, 0x00020000);
  const auto rsg = __builtin_amdgcn_make_buffer_rsrc((void*)p.g, 0, (int)p.gbytes, 0x00020000);
  const int frow = lane & 31, fhi = lane >> 5;
  const unsigned ldx2 = 2u * (unsigned)p.ldx;
  const short fl = p.relu ? (short)0 : (short)-32768;
  const s16x2_t floor2 = {fl, fl};
  const int JQ = p.J >> 2;

  auto fetch = [&](int rb, u32x4 (&q)[KS]) {
    const int row = rb * 32 + frow;
    const unsigned base = row < p.J ? quad_pixel(row, p.H, p.W, p.wshift, p.hshift) * ldx2 + (unsigned)fhi * 16u : OOR;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      const unsigned off = ((2 * ks + fhi) * 8 < p.C) ? base + (unsigned)ks * 32u : OOR;
      q[ks] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsx, (int)off, 0, 0));
    }
  };

  auto compute_store = [&](int rb, u32x4 (&q)[KS]) {
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
      for (int e = 0; e < 4; e++) {      // ReLU on load: one v_pk_max_i16 per dword against 0 or -32768
        const uint32_t xw = q[ks][e];
        s16x2_t t = __builtin_bit_cast(s16x2_t, xw);
        t = __builtin_elementwise_max(t, floor2);
        q[ks][e] = __builtin_bit_cast(uint32_t, t);
      }
    f32x16 acc[NT];
#pragma unroll
    for (int a = 0; a < NT; a++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
      const bf16x8_t qf = __builtin_bit_cast(bf16x8_t, q[ks]);
#pragma unroll
      for (int a = 0; a < NT; a++) {
        const u32x4 v = *(const u32x4*)(wsm + (a * 32 + frow) * WP + (2 * ks + fhi) * 16);
        acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, v), qf, acc[a], 0, 0, 0);
      }
    }
    // ---- wave-private epilogue: the 32 x I tile, rounded to bf16, through LDS ------------------------------------------------------
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the previous row block's staging reads are done (LDS is in order per wave)
#pragma unroll
    for (int a = 0; a < NT; a++)
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        const int il = a * 32 + 8 * g4 + 4 * fhi;
        u32x2 t;
        t[0] = pack2bf(acc[a][4 * g4 + 0], acc[a][4 * g4 + 1]);
        t[1] = pack2bf(acc[a][4 * g4 + 2], acc[a][4 * g4 + 3]);
        *(u32x2*)(stg + frow * SP + il * 2) = t;
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    // theta: every pixel of the row block, DP8 chunks each (a compile-time number of buffer stores; lanes with nothing to do are out of range)
#pragma unroll
    for (int it = 0; it < NITT; it++) {
      const int idx = lane + 64 * it;
      const int r = idx / DP8, c = idx - r * DP8;
      const int row = rb * 32 + r;
      const bool ok = idx < 32 * DP8 && row < p.J;
      const unsigned off = ok ? (quad_pixel(row, p.H, p.W, p.wshift, p.hshift) * DP8 + (unsigned)c) * 16u : OOR;
      const u32x4 v = *(const u32x4*)(stg + (r & 31) * SP + c * 16);
      __builtin_amdgcn_raw_buffer_store_b128(v, rst, (int)off, 0, 0);
    }
    // phi and g: a lane owns 8 channels of one window -- the four rows of the window, maximum and argmax as k_maxpool2_fwd takes them
#pragma unroll
    for (int it = 0; it < NITP; it++) {
      const int idx = lane + 64 * it;
      const int qw = (idx / PCH) & 7, cv = idx - (idx / PCH) * PCH;
      const int Q = rb * 8 + qw;
      const bool ok = idx < 8 * PCH && Q < JQ;
      const char* src = stg + (4 * qw) * SP + (DP8 + cv) * 16;
      const u32x4 r0 = *(const u32x4*)src, r1 = *(const u32x4*)(src + SP), r2 = *(const u32x4*)(src + 2 * SP), r3 = *(const u32x4*)(src + 3 * SP);
      float v0[8], v1[8], v2[8], v3[8], m[8];
      unpack16<bf16_t>(r0, v0); unpack16<bf16_t>(r1, v1); unpack16<bf16_t>(r2, v2); unpack16<bf16_t>(r3, v3);
      uint32_t a_lo = 0, a_hi = 0;
#pragma unroll
      for (int e = 0; e < 8; e++) {
        float mm = v0[e]; uint32_t a = 0;
        if (v1[e] > mm) { mm = v1[e]; a = 1; }
        if (v2[e] > mm) { mm = v2[e]; a = 2; }
        if (v3[e] > mm) { mm = v3[e]; a = 3; }
        m[e] = mm;
        if (e < 4) a_lo |= a << (8 * e); else a_hi |= a << (8 * (e - 4));
      }
      u32x4 o;      // (the values are bf16 already: repacking is a shift, not a rounding)
#pragma unroll
      for (int d = 0; d < 4; d++) o[d] = (__float_as_uint(m[2 * d]) >> 16) | (__float_as_uint(m[2 * d + 1]) & 0xffff0000u);
      const bool isphi = cv < DP8;
      const unsigned offp = (ok && isphi) ? ((unsigned)Q * DP8 + (unsigned)cv) * 16u : OOR;
      const unsigned offg = (ok && !isphi) ? ((unsigned)Q * CG8 + (unsigned)(cv - DP8)) * 16u : OOR;
      __builtin_amdgcn_raw_buffer_store_b128(o, rsp, (int)offp, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(o, rsg, (int)offg, 0, 0);
      if (ok) {
        uint8_t* ip = isphi ? p.iphi + ((long long)Q * DP8 + cv) * 8 : p.ig + ((long long)Q * CG8 + (cv - DP8)) * 8;
        const u32x2 av = {a_lo, a_hi};
        *(u32x2*)ip = av;
      }
    }
  };

  const int stride = gridDim.x * NW;
  int rb = blockIdx.x * NW + wave;
  u32x4 qa[KS], qb[KS];
  if (rb >= p.nrb) return;
  fetch(rb, qa);
  while (true) {
    fetch(rb + stride, qb);
    compute_store(rb, qa);
    rb += stride;
    if (rb >= p.nrb) break;
    fetch(rb + stride, qa);
    compute_store(rb, qb);
    rb += stride;
    if (rb >= p.nrb) break;
  }
}

struct ApBwdParams {
  const bf16_t* dtheta; const bf16_t* dphi; const bf16_t* dg; const uint8_t* iphi; const uint8_t* ig;
  const bf16_t* wt; const bf16_t* wp; const bf16_t* wg;      // data-gradient images [C][Dp], [C][Dp], [C][Cg]
  const bf16_t* res; bf16_t* dx;                             // [B,H,W,C] both (res may be null)
  int C, H, W, wshift, hshift, J, nrb;
  unsigned tbytes, pbytes, gbytes, obytes;
};

// k is laid out [theta | phi | g] with theta and phi each padded to whole 16-wide k-steps, so that a k-step has ONE source for all lanes.
// Output channels: NP passes of TI x 32 over the same fragments.
template <int DP8, int CG8, int TI, int NP, int NW>
__global__ __launch_bounds__(64 * NW) void k_attn_proj_bwd(ApBwdParams p) {
  constexpr int DS = (DP8 + 1) / 2, GS = CG8 / 2;      // k-steps of theta (= phi) and of g
  constexpr int KS = 2 * DS + GS;
  constexpr int BI = TI * NP * 32;
  constexpr int WP = KS * 32 + 16;
  constexpr int CP = TI * 64 + 16;
  constexpr int CPR = TI * 4;
  constexpr int NIT = (32 * CPR + 63) / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const wsm = smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* const stg = smem + BI * WP + wave * (32 * CP);

  for (int idx = tid; idx < BI * 2 * KS; idx += 64 * NW) {
    const int row = idx / (2 * KS), c = idx - row * (2 * KS);
    u32x4 v = {0u, 0u, 0u, 0u};
    if (row < p.C) {
      if (c < 2 * DS) { if (c < DP8) v = *(const u32x4*)(p.wt + (long long)row * (DP8 * 8) + c * 8); }
      else if (c < 4 * DS) { if (c - 2 * DS < DP8) v = *(const u32x4*)(p.wp + (long long)row * (DP8 * 8) + (c - 2 * DS) * 8); }
      else v = *(const u32x4*)(p.wg + (long long)row * (CG8 * 8) + (c - 4 * DS) * 8);
    }
    *(u32x4*)(wsm + row * WP + c * 16) = v;
  }
  __syncthreads();

  const auto rst = __builtin_amdgcn_make_buffer_rsrc((void*)p.dtheta, 0, (int)p.tbytes, 0x00020000);
  const auto rsp = __builtin_amdgcn_make_buffer_rsrc((void*)p.dphi, 0, (int)p.pbytes, 0x00020000);
  const auto rsg = __builtin_amdgcn_make_buffer_rsrc((void*)p.dg, 0, (int)p.gbytes, 0x00020000);
  const auto rso = __builtin_amdgcn_make_buffer_rsrc((void*)p.dx, 0, (int)p.obytes, 0x00020000);
  const auto rsr = __builtin_amdgcn_make_buffer_rsrc((void*)(p.res ? p.res : p.dx), 0, (int)p.obytes, 0x00020000);
  const int frow = lane & 31, fhi = lane >> 5;
  const bool pre_res = p.res != nullptr;
  const unsigned C2 = 2u * (unsigned)p.C;
  const int ncr = (p.C + 7) >> 3;

  struct Frag { u32x4 t[DS]; u32x4 ph[DS]; u32x2 pi[DS]; u32x4 g[GS]; u32x2 gi[GS]; };

  auto fetch = [&](int rb, Frag& f) {
    const int row = rb * 32 + frow;
    const bool rok = row < p.J;
    const unsigned pix = quad_pixel(rok ? row : 0, p.H, p.W, p.wshift, p.hshift);
    const unsigned Q = (unsigned)(rok ? row : 0) >> 2;
#pragma unroll
    for (int s = 0; s < DS; s++) {
      const int lc = 2 * s + fhi;
      const bool ok = rok && lc < DP8;
      f.t[s] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rst, (int)(ok ? (pix * DP8 + (unsigned)lc) * 16u : OOR), 0, 0));
      f.ph[s] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsp, (int)(ok ? (Q * DP8 + (unsigned)lc) * 16u : OOR), 0, 0));
      f.pi[s] = *(const u32x2*)(p.iphi + (ok ? ((long long)Q * DP8 + lc) * 8 : 0));      // (not ok: any valid address; the gradient chunk is zero)
    }
#pragma unroll
    for (int s = 0; s < GS; s++) {
      const int lc = 2 * s + fhi;
      f.g[s] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsg, (int)(rok ? (Q * CG8 + (unsigned)lc) * 16u : OOR), 0, 0));
      f.gi[s] = *(const u32x2*)(p.ig + (rok ? ((long long)Q * CG8 + lc) * 8 : 0));
    }
  };

  // un-pool on load: the pooled gradient where the window's argmax is this pixel's position, zero elsewhere (k_maxpool2_bwd's select)
  auto unpool = [](u32x4 g, u32x2 av, uint32_t pos) {
    u32x4 o;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const uint32_t w = d < 2 ? av[0] : av[1];
      const uint32_t a0 = (w >> (16 * (d & 1))) & 0xffu, a1 = (w >> (16 * (d & 1) + 8)) & 0xffu;
      o[d] = (a0 == pos ? (g[d] & 0xffffu) : 0u) | (a1 == pos ? (g[d] & 0xffff0000u) : 0u);
    }
    return o;
  };

  auto compute_store = [&](int rb, Frag& f) {
    const uint32_t pos = (uint32_t)(frow & 3);      // (rb * 32 + frow) & 3 = (dy << 1) | dx
    u32x4 q[KS];
#pragma unroll
    for (int s = 0; s < DS; s++) { q[s] = f.t[s]; q[DS + s] = unpool(f.ph[s], f.pi[s], pos); }
#pragma unroll
    for (int s = 0; s < GS; s++) q[2 * DS + s] = unpool(f.g[s], f.gi[s], pos);
#pragma unroll
    for (int ps = 0; ps < NP; ps++) {
      f32x16 acc[TI];
#pragma unroll
      for (int a = 0; a < TI; a++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[a][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        const bf16x8_t qf = __builtin_bit_cast(bf16x8_t, q[ks]);
#pragma unroll
        for (int a = 0; a < TI; a++) {
          const u32x4 v = *(const u32x4*)(wsm + ((ps * TI + a) * 32 + frow) * WP + (2 * ks + fhi) * 16);
          acc[a] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, v), qf, acc[a], 0, 0, 0);
        }
      }
      const int ic0 = ps * TI * 32;
      const int ncp = ncr - ps * CPR;      // 16-byte chunks of this pass that exist
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (pre_res) {
        u32x4 pre[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
          const int idx = lane + 64 * it;
          const int r = idx / CPR, c = idx - r * CPR;
          const int row = rb * 32 + r;
          const bool ok = idx < 32 * CPR && row < p.J && c < ncp;
          const unsigned off = ok ? quad_pixel(row, p.H, p.W, p.wshift, p.hshift) * C2 + (unsigned)(ic0 + c * 8) * 2u : OOR;
          pre[it] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsr, (int)off, 0, 0));
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
          const int idx = lane + 64 * it;
          const int r = idx / CPR, c = idx - r * CPR;
          if (idx < 32 * CPR) *(u32x4*)(stg + r * CP + c * 16) = pre[it];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
#pragma unroll
      for (int a = 0; a < TI; a++)
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) {
          const int il = a * 32 + 8 * g4 + 4 * fhi;
          char* loc = stg + frow * CP + il * 2;
          float v[4] = {acc[a][4 * g4 + 0], acc[a][4 * g4 + 1], acc[a][4 * g4 + 2], acc[a][4 * g4 + 3]};
          if (pre_res) {
            const u32x2 r = *(const u32x2*)loc;
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] += bf2f((bf16_t)((r[e >> 1] >> (16 * (e & 1))) & 0xffffu));
          }
          u32x2 t;
          t[0] = pack2bf(v[0], v[1]);
          t[1] = pack2bf(v[2], v[3]);
          *(u32x2*)loc = t;
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int it = 0; it < NIT; it++) {
        const int idx = lane + 64 * it;
        const int r = idx / CPR, c = idx - r * CPR;
        const int row = rb * 32 + r;
        const bool ok = idx < 32 * CPR && row < p.J && c < ncp;
        const unsigned off = ok ? quad_pixel(row, p.H, p.W, p.wshift, p.hshift) * C2 + (unsigned)(ic0 + c * 8) * 2u : OOR;
        const u32x4 v = *(const u32x4*)(stg + (r & 31) * CP + c * 16);
        __builtin_amdgcn_raw_buffer_store_b128(v, rso, (int)off, 0, 0);
      }
    }
  };

  const int stride = gridDim.x * NW;
  int rb = blockIdx.x * NW + wave;
  if (rb >= p.nrb) return;
  Frag fa, fb;
  fetch(rb, fa);
  while (true) {
    fetch(rb + stride, fb);
    compute_store(rb, fa);
    rb += stride;
    if (rb >= p.nrb) break;
    fetch(rb + stride, fa);
    compute_store(rb, fb);
    rb += stride;
    if (rb >= p.nrb) break;
  }
}

int ilog2_pow2(int v) {
  if (v <= 0 || (v & (v - 1))) return -1;
  int s = 0;
  while ((1 << s) < v) s++;
  return s;
}
bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// the two instantiated families: 0 = (Dp 16, Cg 48, C <= 96) -- BigGAN-128's discriminator at ch 96; 1 = (Dp 24, Cg 96, C <= 192) -- its generator
int family(int C, int Dp, int Cg) {
  if (Dp == 16 && Cg == 48 && C <= 96) return 0;
  if (Dp == 24 && Cg == 96 && C <= 192) return 1;
  return -1;
}

template <typename K> int set_lds(K kern, int lds) {
  return hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess ? 0 : -1;
}

}  // namespace

extern "C" int sg_attn_proj_ok(int B, int H, int W, int C, int ldx, int Dp, int Cg) {
  if (B <= 0 || ilog2_pow2(H) < 1 || ilog2_pow2(W) < 1 || C <= 0 || C % 8 || ldx % 8 || ldx < C) return 0;
  if (family(C, Dp, Cg) < 0) return 0;
  const long long J = (long long)B * H * W;
  if (J >= (1ll << 30) || J * ldx * 2 >= (1ll << 31) || J * C * 2 >= (1ll << 31)) return 0;      // 32-bit buffer offsets, bit 31 = "no access"
  return 1;
}

extern "C" int sg_attn_proj_fwd(const void* x, int ldx, const void* w_theta, const void* w_phi, const void* w_g, void* theta, void* phi, void* g,
                                uint8_t* idx_phi, uint8_t* idx_g, int B, int H, int W, int C, int Dp, int Cg, int relu, sg_stream_t s) {
  SG_CHECK(x && w_theta && w_phi && w_g && theta && phi && g && idx_phi && idx_g, "sg_attn_proj_fwd: null");
  SG_CHECK(sg_attn_proj_ok(B, H, W, C, ldx, Dp, Cg) == 1, "sg_attn_proj_fwd: unsupported shape (ask sg_attn_proj_ok)");
  SG_CHECK(al16(x) && al16(w_theta) && al16(w_phi) && al16(w_g) && al16(theta) && al16(phi) && al16(g) && !(((uintptr_t)idx_phi | (uintptr_t)idx_g) & 7),
           "sg_attn_proj_fwd: misaligned pointer");
  hipStream_t st = (hipStream_t)s;
  ApFwdParams p;
  p.x = (const bf16_t*)x; p.wt = (const bf16_t*)w_theta; p.wp = (const bf16_t*)w_phi; p.wg = (const bf16_t*)w_g;
  p.theta = (bf16_t*)theta; p.phi = (bf16_t*)phi; p.g = (bf16_t*)g; p.iphi = idx_phi; p.ig = idx_g;
  p.C = C; p.ldx = ldx; p.H = H; p.W = W; p.wshift = ilog2_pow2(W); p.hshift = ilog2_pow2(H);
  const long long J = (long long)B * H * W;
  p.J = (int)J; p.relu = relu ? 1 : 0; p.nrb = (int)((J + 31) / 32);
  p.xbytes = (unsigned)(((J - 1) * ldx + C) * 2); p.tbytes = (unsigned)(J * Dp * 2); p.pbytes = (unsigned)(J / 4 * Dp * 2); p.gbytes = (unsigned)(J / 4 * Cg * 2);
  const double I = 2.0 * Dp + Cg;
  const int prof = sg_prof_begin(st, 2.0 * I * (double)J * (double)C, 0);
  // algorithmic HBM bytes: x and the three images once, theta, the pooled phi / g and their one-byte argmax planes
  sg_prof_tag(prof, SG_ENG_CONV_SK, 2.0 * ((double)J * C + I * C + (double)J * Dp) + 0.25 * (double)J * (Dp + Cg) * 3.0);
#define AP_FWD(DP8, CG8, KS, NW)                                                                                     \
  {                                                                                                                  \
    constexpr int NT = ((2 * DP8 + CG8) * 8 + 31) / 32;                                                              \
    constexpr int lds = NT * 32 * (KS * 32 + 16) + NW * 32 * (NT * 64 + 16);                                         \
    static_assert(lds <= 160 * 1024, "LDS");                                                                         \
    static bool done = false;                                                                                        \
    if (!done) { SG_CHECK(set_lds(k_attn_proj_fwd<DP8, CG8, KS, NW>, lds) == 0, "sg_attn_proj_fwd: LDS attribute"); done = true; } \
    int gx = (p.nrb + NW - 1) / NW;                                                                                  \
    const int cap = 256 * (8 / NW);                                                                                  \
    if (gx > cap) gx = cap;                                                                                          \
    hipLaunchKernelGGL((k_attn_proj_fwd<DP8, CG8, KS, NW>), dim3(gx), dim3(64 * NW), lds, st, p);                    \
  }
  if (family(C, Dp, Cg) == 0) AP_FWD(2, 6, 6, 4) else AP_FWD(3, 12, 12, 8)
#undef AP_FWD
  sg_prof_end(st, prof);
  SG_LAUNCH_CHECK();
  return 0;
}

extern "C" int sg_attn_proj_bwd_data(const void* dtheta, const void* dphi, const void* dg, const uint8_t* idx_phi, const uint8_t* idx_g, const void* wd_theta,
                                     const void* wd_phi, const void* wd_g, const void* res, void* dx, int B, int H, int W, int C, int Dp, int Cg, sg_stream_t s) {
  SG_CHECK(dtheta && dphi && dg && idx_phi && idx_g && wd_theta && wd_phi && wd_g && dx, "sg_attn_proj_bwd_data: null");
  SG_CHECK(sg_attn_proj_ok(B, H, W, C, C, Dp, Cg) == 1, "sg_attn_proj_bwd_data: unsupported shape (ask sg_attn_proj_ok)");
  SG_CHECK(al16(dtheta) && al16(dphi) && al16(dg) && al16(wd_theta) && al16(wd_phi) && al16(wd_g) && al16(res) && al16(dx) &&
           !(((uintptr_t)idx_phi | (uintptr_t)idx_g) & 7), "sg_attn_proj_bwd_data: misaligned pointer");
  hipStream_t st = (hipStream_t)s;
  ApBwdParams p;
  p.dtheta = (const bf16_t*)dtheta; p.dphi = (const bf16_t*)dphi; p.dg = (const bf16_t*)dg; p.iphi = idx_phi; p.ig = idx_g;
  p.wt = (const bf16_t*)wd_theta; p.wp = (const bf16_t*)wd_phi; p.wg = (const bf16_t*)wd_g;
  p.res = (const bf16_t*)res; p.dx = (bf16_t*)dx;
  p.C = C; p.H = H; p.W = W; p.wshift = ilog2_pow2(W); p.hshift = ilog2_pow2(H);
  const long long J = (long long)B * H * W;
  p.J = (int)J; p.nrb = (int)((J + 31) / 32);
  p.tbytes = (unsigned)(J * Dp * 2); p.pbytes = (unsigned)(J / 4 * Dp * 2); p.gbytes = (unsigned)(J / 4 * Cg * 2); p.obytes = (unsigned)(J * C * 2);
  const double I = 2.0 * Dp + Cg;
  const int prof = sg_prof_begin(st, 2.0 * I * (double)J * (double)C, 0);
  sg_prof_tag(prof, SG_ENG_CONV_SK, 2.0 * ((double)J * C * (res ? 2.0 : 1.0) + I * C + (double)J * Dp) + 0.25 * (double)J * (Dp + Cg) * 3.0);
#define AP_BWD(DP8, CG8, TI, NP, NW)                                                                                 \
  {                                                                                                                  \
    constexpr int KS = 2 * ((DP8 + 1) / 2) + CG8 / 2;                                                                \
    constexpr int lds = TI * NP * 32 * (KS * 32 + 16) + NW * 32 * (TI * 64 + 16);                                    \
    static_assert(lds <= 160 * 1024, "LDS");                                                                         \
    static bool done = false;                                                                                        \
    if (!done) { SG_CHECK(set_lds(k_attn_proj_bwd<DP8, CG8, TI, NP, NW>, lds) == 0, "sg_attn_proj_bwd_data: LDS attribute"); done = true; } \
    int gx = (p.nrb + NW - 1) / NW;                                                                                  \
    const int cap = 256 * (8 / NW);                                                                                  \
    if (gx > cap) gx = cap;                                                                                          \
    hipLaunchKernelGGL((k_attn_proj_bwd<DP8, CG8, TI, NP, NW>), dim3(gx), dim3(64 * NW), lds, st, p);                \
  }
  if (family(C, Dp, Cg) == 0) AP_BWD(2, 6, 3, 1, 4) else AP_BWD(3, 12, 3, 2, 8)
#undef AP_BWD
  sg_prof_end(st, prof);
  SG_LAUNCH_CHECK();
  return 0;
}
