// attn.hip -- the self-attention core (reference src/utils/ops.py:83-103) on the bf16 path, without a score matrix in HBM.
//
// The generic chain materialises the fp32 scores S = theta . phi^T ([B, HW, HW/4]: 4.3 GB at BigGAN-128's 64x64 attention, batch 256), re-reads them for
// the softmax and writes the bf16 probabilities: ~13 GB of HBM traffic per forward for 0.26 TFLOP. Here scores, probabilities and their gradients live in
// registers only; what crosses HBM besides the operands is one fp32 row statistic per query each way (lse forward, delta backward):
//
//   sg_attn_fwd_fused : O = softmax_k(theta_q . phi_k) g, the row log-sum-exp and (on request) an unrounded fp32 copy of O   -- k_attn_fwd_flash
//   sg_attn_bwd_fused : dtheta, dphi, dg with P and dS = P * (dP - delta) recomputed per tile from theta / phi / lse          -- k_attn_bwd_q, k_attn_bwd_k
//
// Layout: one workgroup = 4 waves = 128 queries (key side of the backward: 128 keys) of one image; MFMA 32x32x16 with A = keys (rows), B = queries (rows),
// so a lane owns ONE query (l & 31) and 16 of the 32 keys of a block: the softmax statistics are in-lane plus one cross-half exchange. Key-side operands
// ([rows][32 channels] bf16) are streamed in 256-row chunks through the LDS tile image of lds_tile.h: (1 + NCG) * 16 KiB whatever the number of keys.
// The chunk barriers here are plain __syncthreads(): they rely on the s_waitcnt vmcnt(0) the compiler puts in front of s_barrier, not on lt_drain_barrier.
#include "common.h"
#include "lds_tile.h"
#include "../../include/sgamd.h"

// Inner-loop unrolling of the streaming kernels (k_attn_fwd_flash, k_attn_bwd_q, k_attn_bwd_k): left to the compiler these loops were unrolled
// eight times and their fragment loads hoisted -- 276 registers for k_attn_fwd_flash<3>, 324 / 432 for k_attn_bwd_k<2> / <3>: ONE wave per SIMD under kernels whose
// MFMA -> exp -> pack -> MFMA chains have nothing but other waves to hide behind (round 5, tools/isa_mix.py).
#ifndef AT_UNROLL
#define AT_UNROLL 1
#endif
// workgroups per CU the staging areas allow ((1 + NCG) * 16 KiB each): the register budget is set to match
#ifndef AT_WAVES
#define AT_WAVES(NCG) ((NCG) <= 2 ? 3 : 2)
#endif

// B fragment straight from global memory: row `row` of a [.][ld] matrix, 8 channels at c (zero beyond C)
__device__ __forceinline__ u32x4 at_gfrag(const bf16_t* base, long long row, int ld, int c, int C) {
  u32x4 z = {0u, 0u, 0u, 0u};
  return (c < C) ? *(const u32x4*)(base + row * ld + c) : z;
}

// ---- forward: ONE pass over the keys, running maximum with a deferred rescale -----------------------------------------------------------------------------
// Per 32-key block: scores on the MFMA, p = exp2(s log2e - m log2e), row sum, and O^T[c][q] += V^T[c][k] P[k][q] on the MFMA with the unnormalised bf16 p as
// the B operand; O = O' / l at the end. The probabilities go from the score accumulators straight into that B operand: a lane owns keys
// {0-3, 8-11, 16-19, 24-27} + 4h of a block for its query; the contraction index of the second product is simply taken in THAT order (slot (h, e) <-> key
// 4h + e, 8 + 4h + e - 4, ...: pa / pb below), and the V^T fragments are gathered in the same order by ds_read_b64_tr_b16 from the [key][32 channels] chunk
// image (lt_vfrag) -- no cross-lane exchange.
// History. The first fused forward (whole key image in LDS, two exp passes; removed since, with the variant of it that stored the bf16 probabilities for a
// GEMM backward): 811 us on D's attention (B 256, 4096 queries x 1024 keys, 48 channels). Round 2: keys and values streamed in 256-key chunks, pass 1 =
// running row maximum only (scores + 16 v_max per block), pass 2 = the block loop above. Round 5: the maximum pass is gone. The running maximum m of a
// query is only RAISED when a block's maximum exceeds it by more than AT_THR (then l and the O' accumulators of that query are rescaled by exp(m_old - m_new), as in
// online softmax); below the threshold the stale m is kept and p = exp(s - m) <= e^AT_THR simply carries a common factor that cancels in O' / l and in
// lse = m + log l. bf16 p has fp32's exponent range, l and O' accumulate in fp32: nothing is lost to the factor. With a threshold the rescale runs once per query
// (at the first block) instead of on almost every block for some query of the wave; what is saved per 32-key block is the first pass's two score MFMAs, its two
// fragment reads and its 16 v_max, and per chunk one key staging and two barriers.
// m is kept equal in the two lane halves of a query (they hold disjoint keys of the block, and the second product contracts over both halves' probabilities).
// grid (HW / 128, B), 256 threads, LDS (1 + NCG) * 16 KiB.
#ifndef AT_THR
#define AT_THR 8.0f
#endif
template <int NCG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(AT_WAVES(NCG), AT_WAVES(NCG)))) void k_attn_fwd_flash(const bf16_t* theta, const bf16_t* phi, const bf16_t* g, float* lse, bf16_t* O, float* O32,
                                                        int HW, int HW4, int Dp, int Cg) {
  constexpr int KC = 256;
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) char at_smem[];
  char* kimg = at_smem;
  char* vimg = at_smem + KC * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y;
  const int q = blockIdx.x * 128 + wave * 32 + (lane & 31);
  const int h = lane >> 5;
  const long long qrow = (long long)b * HW + q;
  const bf16x8_t qf0 = __builtin_bit_cast(bf16x8_t, at_gfrag(theta, qrow, Dp, 8 * h, Dp));
  const bf16x8_t qf1 = __builtin_bit_cast(bf16x8_t, at_gfrag(theta, qrow, Dp, 16 + 8 * h, Dp));
  float m = -3.0e38f;          // running reference maximum of this query (natural-log units), equal in both lane halves
  float m2 = m * LOG2E;
  float l = 0.f;
  f32x16 o[NCG];
#pragma unroll
  for (int cg = 0; cg < NCG; cg++)
#pragma unroll
    for (int r = 0; r < 16; r++) o[cg][r] = 0.f;
  for (int k0 = 0; k0 < HW4; k0 += KC) {
    __syncthreads();
    lt_stage_cols<4>(kimg, phi + ((long long)b * HW4 + k0) * Dp, KC, Dp, 0, Dp, wave, lane);
#pragma unroll
    for (int cg = 0; cg < NCG; cg++) lt_stage_cols<4>(vimg + cg * KC * 64, g + ((long long)b * HW4 + k0) * Cg, KC, Cg, cg * 32, Cg, wave, lane);
    __syncthreads();
#pragma unroll AT_UNROLL
    for (int kc = 0; kc < KC / 32; kc++) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; r++) s[r] = 0.f;
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(kimg, kc, 0, lane), qf0, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(kimg, kc, 1, lane), qf1, s, 0, 0, 0);
      float bm = s[0];
#pragma unroll
      for (int r = 1; r < 16; r++) bm = fmaxf(bm, s[r]);
      bm = lt_half_max(bm);
      if (bm > m + AT_THR) {                                      // (the first block always: m starts at -3e38)
        const float alpha = __builtin_amdgcn_exp2f((m - bm) * LOG2E);
        l *= alpha;
#pragma unroll
        for (int cg = 0; cg < NCG; cg++)
#pragma unroll
          for (int r = 0; r < 16; r++) o[cg][r] *= alpha;
        m = bm;
        m2 = m * LOG2E;
      }
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; r++) { p[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], LOG2E, -m2)); l += p[r]; }
      u32x4 pa, pb;                                               // regs 0-7 / 8-15 = contraction slots of the two k-steps
#pragma unroll
      for (int i = 0; i < 4; i++) { pa[i] = pack2bf(p[2 * i], p[2 * i + 1]); pb[i] = pack2bf(p[8 + 2 * i], p[8 + 2 * i + 1]); }
      const bf16x8_t pfa = __builtin_bit_cast(bf16x8_t, pa), pfb = __builtin_bit_cast(bf16x8_t, pb);
#pragma unroll
      for (int cg = 0; cg < NCG; cg++) {
        const char* vi = vimg + cg * KC * 64;
        o[cg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(vi, kc * 32 + 4 * h, lane), pfa, o[cg], 0, 0, 0);
        o[cg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(vi, kc * 32 + 16 + 4 * h, lane), pfb, o[cg], 0, 0, 0);
      }
    }
  }
  l = lt_half_sum(l);
  // (the MFMA contracts over the key slots of BOTH lane halves, so o[] is already complete for the channels this lane holds; only the
  // row sum is per half and needs the exchange -- the reference maximum is common to both halves by construction)
  const float inv = 1.f / l;
  if (h == 0) lse[qrow] = m + __logf(l);
  bf16_t* orow = O + qrow * Cg;
#pragma unroll
  for (int cg = 0; cg < NCG; cg++)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
      const int c0 = cg * 32 + 8 * g4 + 4 * h;
      if (c0 < Cg) {
        const f32x4 f = {o[cg][4 * g4 + 0] * inv, o[cg][4 * g4 + 1] * inv, o[cg][4 * g4 + 2] * inv, o[cg][4 * g4 + 3] * inv};
        u32x2 v = {pack2bf(f[0], f[1]), pack2bf(f[2], f[3])};
        *(u32x2*)(orow + c0) = v;
        if (O32) *(f32x4*)(O32 + qrow * Cg + c0) = f;             // unrounded copy for the backward's delta_q = dO_q . O_q
      }
    }
}

// ---- fused backward, query side: delta, dS (registers only) and dtheta = dS phi ------------------------------------------------------------
// Per 32-key block the scores and dP = dO . V^T come off the MFMA, P is recomputed from lse, and dS = P * (dP - delta) goes from the accumulators into the
// B operand of dtheta^T[d][q] += phi^T[d][k] dS[k][q] (same key order trick as the forward); delta_q is also written out for the key side.
// With the forward output O at hand, delta_q = sum_k P_qk dP_qk = sum_c dO_qc O_qc (the row identity flash attention uses) is a dot product of
// two rows the lane pair already touches, and the first of the two key passes (16 v_exp + 6 MFMAs per block just for delta) disappears.
// O comes as the UNROUNDED fp32 copy the forward keeps for this purpose: with the bf16 output the error of dtheta against fp64 grew from
// ~2e-2 to 4.4e-2 on the near-uniform softmax of tests/test_kernels_gpu.py::test_attention_core (session F), because dS = P (dP - delta)
// subtracts nearly equal numbers there.
template <int NCG> __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(AT_WAVES(NCG), AT_WAVES(NCG)))) void k_attn_bwd_q(const bf16_t* theta, const bf16_t* phi, const bf16_t* g, const bf16_t* dO, const float* Oin,
                                                                        const float* lse, float* delta_out, bf16_t* dtheta, int HW, int HW4, int Dp, int Cg) {
  constexpr int KC = 256;
  extern __shared__ __attribute__((aligned(16))) char at_smem[];
  char* kimg = at_smem;
  char* vimg = at_smem + KC * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y;
  const int q = blockIdx.x * 128 + wave * 32 + (lane & 31);
  const int h = lane >> 5;
  const long long qrow = (long long)b * HW + q;
  const bf16x8_t qf0 = __builtin_bit_cast(bf16x8_t, at_gfrag(theta, qrow, Dp, 8 * h, Dp));
  const bf16x8_t qf1 = __builtin_bit_cast(bf16x8_t, at_gfrag(theta, qrow, Dp, 16 + 8 * h, Dp));
  bf16x8_t df[NCG][2];
#pragma unroll
  for (int cg = 0; cg < NCG; cg++)
#pragma unroll
    for (int t = 0; t < 2; t++) df[cg][t] = __builtin_bit_cast(bf16x8_t, at_gfrag(dO, qrow, Cg, cg * 32 + 16 * t + 8 * h, Cg));
  float delta = 0.f;
  const float ls2 = lse[qrow] * 1.4426950408889634f;
  if (Oin) {
#pragma unroll
    for (int cg = 0; cg < NCG; cg++)
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const int c0 = cg * 32 + 16 * t + 8 * h;
        if (c0 < Cg) {                                               // Cg % 8 == 0: groups of 8 channels are whole
          const f32x4 oa = *(const f32x4*)(Oin + qrow * Cg + c0), ob = *(const f32x4*)(Oin + qrow * Cg + c0 + 4);
          const u32x4 dv = __builtin_bit_cast(u32x4, df[cg][t]);
          delta += oa[0] * __uint_as_float(dv[0] << 16) + oa[1] * __uint_as_float(dv[0] & 0xffff0000u) + oa[2] * __uint_as_float(dv[1] << 16) + oa[3] * __uint_as_float(dv[1] & 0xffff0000u)
                 + ob[0] * __uint_as_float(dv[2] << 16) + ob[1] * __uint_as_float(dv[2] & 0xffff0000u) + ob[2] * __uint_as_float(dv[3] << 16) + ob[3] * __uint_as_float(dv[3] & 0xffff0000u);
        }
      }
    delta = lt_half_sum(delta);
  }
  f32x16 dth;
#pragma unroll
  for (int r = 0; r < 16; r++) dth[r] = 0.f;
  for (int pass = Oin ? 1 : 0; pass < 2; pass++) {
    for (int k0 = 0; k0 < HW4; k0 += KC) {
      __syncthreads();
      lt_stage_cols<4>(kimg, phi + ((long long)b * HW4 + k0) * Dp, KC, Dp, 0, Dp, wave, lane);
#pragma unroll
      for (int cg = 0; cg < NCG; cg++) lt_stage_cols<4>(vimg + cg * KC * 64, g + ((long long)b * HW4 + k0) * Cg, KC, Cg, cg * 32, Cg, wave, lane);
      __syncthreads();
#pragma unroll AT_UNROLL
      for (int kb = 0; kb < KC / 32; kb++) {
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(kimg, kb, 0, lane), qf0, s, 0, 0, 0);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(kimg, kb, 1, lane), qf1, s, 0, 0, 0);
#pragma unroll
        for (int cg = 0; cg < NCG; cg++)
#pragma unroll
          for (int t = 0; t < 2; t++)
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(vimg + cg * KC * 64, kb, t, lane), df[cg][t], dp, 0, 0, 0);
        if (pass == 0) {
#pragma unroll
          for (int r = 0; r < 16; r++) delta += __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], 1.4426950408889634f, -ls2)) * dp[r];
        } else {
          float o[16];
#pragma unroll
          for (int r = 0; r < 16; r++) o[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], 1.4426950408889634f, -ls2)) * (dp[r] - delta);
          u32x4 da, db;
#pragma unroll
          for (int i = 0; i < 4; i++) { da[i] = pack2bf(o[2 * i], o[2 * i + 1]); db[i] = pack2bf(o[8 + 2 * i], o[8 + 2 * i + 1]); }
          dth = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(kimg, kb * 32 + 4 * h, lane), __builtin_bit_cast(bf16x8_t, da), dth, 0, 0, 0);
          dth = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(kimg, kb * 32 + 16 + 4 * h, lane), __builtin_bit_cast(bf16x8_t, db), dth, 0, 0, 0);
        }
      }
    }
    if (pass == 0) delta = lt_half_sum(delta);
  }
  if (h == 0) delta_out[qrow] = delta;
  bf16_t* trow = dtheta + qrow * Dp;
#pragma unroll
  for (int g4 = 0; g4 < 4; g4++) {
    const int c0 = 8 * g4 + 4 * h;
    if (c0 < Dp) {
      u32x2 v = {pack2bf(dth[4 * g4 + 0], dth[4 * g4 + 1]), pack2bf(dth[4 * g4 + 2], dth[4 * g4 + 3])};
      *(u32x2*)(trow + c0) = v;
    }
  }
}

// ---- fused backward, key side: dphi = dS^T theta, dg = P^T dO with P and dS recomputed per (32 queries x 32 keys) block ----------------------
// One workgroup = 4 waves = 128 keys of one image; a lane owns ONE key (l & 31) and 16 of the 32 queries of a block (the transposed
// orientation of the query-side kernels: scores = theta (rows) x phi (columns)). Query-side operands (theta, dO; lse, delta) are staged by
// LDS-DMA in chunks of 256 queries; they feed the score / dP products as k-contiguous fragments and the two accumulating products as
// transposed fragments of the same images. No P and no dS ever exist in HBM.
template <int NCG> __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(AT_WAVES(NCG), AT_WAVES(NCG)))) void k_attn_bwd_k(const bf16_t* theta, const bf16_t* phi, const bf16_t* g, const bf16_t* dO, const float* lse,
                                                                        const float* delta, bf16_t* dphi, bf16_t* dg, int HW, int HW4, int Dp, int Cg) {
  constexpr int QC = 256;
  extern __shared__ __attribute__((aligned(16))) char at_smem[];
  char* timg = at_smem;
  char* oimg = at_smem + QC * 64;
  float* st = (float*)(at_smem + (1 + NCG) * QC * 64);
  float* dl = st + QC;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y;
  const int key = blockIdx.x * 128 + wave * 32 + (lane & 31);
  const int h = lane >> 5;
  const long long krow = (long long)b * HW4 + key;
  const bf16x8_t kf0 = __builtin_bit_cast(bf16x8_t, at_gfrag(phi, krow, Dp, 8 * h, Dp));
  const bf16x8_t kf1 = __builtin_bit_cast(bf16x8_t, at_gfrag(phi, krow, Dp, 16 + 8 * h, Dp));
  bf16x8_t gf[NCG][2];
#pragma unroll
  for (int cg = 0; cg < NCG; cg++)
#pragma unroll
    for (int t = 0; t < 2; t++) gf[cg][t] = __builtin_bit_cast(bf16x8_t, at_gfrag(g, krow, Cg, cg * 32 + 16 * t + 8 * h, Cg));
  f32x16 dph, dgt[NCG];
#pragma unroll
  for (int r = 0; r < 16; r++) dph[r] = 0.f;
#pragma unroll
  for (int cg = 0; cg < NCG; cg++)
#pragma unroll
    for (int r = 0; r < 16; r++) dgt[cg][r] = 0.f;
  for (int q0 = 0; q0 < HW; q0 += QC) {
    __syncthreads();
    lt_stage_cols<4>(timg, theta + ((long long)b * HW + q0) * Dp, QC, Dp, 0, Dp, wave, lane);
#pragma unroll
    for (int cg = 0; cg < NCG; cg++) lt_stage_cols<4>(oimg + cg * QC * 64, dO + ((long long)b * HW + q0) * Cg, QC, Cg, cg * 32, Cg, wave, lane);
    if (tid < QC) { st[tid] = lse[(long long)b * HW + q0 + tid] * 1.4426950408889634f; dl[tid] = delta[(long long)b * HW + q0 + tid]; }
    __syncthreads();
#pragma unroll AT_UNROLL
    for (int qb = 0; qb < QC / 32; qb++) {
      f32x16 s, dp;
#pragma unroll
      for (int r = 0; r < 16; r++) { s[r] = 0.f; dp[r] = 0.f; }
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(timg, qb, 0, lane), kf0, s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(timg, qb, 1, lane), kf1, s, 0, 0, 0);
#pragma unroll
      for (int cg = 0; cg < NCG; cg++)
#pragma unroll
        for (int t = 0; t < 2; t++)
          dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(oimg + cg * QC * 64, qb, t, lane), gf[cg][t], dp, 0, 0, 0);
      float pr[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; r++) {
        const int qi = qb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;       // the query of accumulator register r
        pr[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], 1.4426950408889634f, -st[qi]));
        ds[r] = pr[r] * (dp[r] - dl[qi]);
      }
      u32x4 pa, pb, da, db;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        pa[i] = pack2bf(pr[2 * i], pr[2 * i + 1]); pb[i] = pack2bf(pr[8 + 2 * i], pr[8 + 2 * i + 1]);
        da[i] = pack2bf(ds[2 * i], ds[2 * i + 1]); db[i] = pack2bf(ds[8 + 2 * i], ds[8 + 2 * i + 1]);
      }
#pragma unroll
      for (int cg = 0; cg < NCG; cg++) {
        const char* oi = oimg + cg * QC * 64;
        dgt[cg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(oi, qb * 32 + 4 * h, lane), __builtin_bit_cast(bf16x8_t, pa), dgt[cg], 0, 0, 0);
        dgt[cg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(oi, qb * 32 + 16 + 4 * h, lane), __builtin_bit_cast(bf16x8_t, pb), dgt[cg], 0, 0, 0);
      }
      dph = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(timg, qb * 32 + 4 * h, lane), __builtin_bit_cast(bf16x8_t, da), dph, 0, 0, 0);
      dph = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(timg, qb * 32 + 16 + 4 * h, lane), __builtin_bit_cast(bf16x8_t, db), dph, 0, 0, 0);
    }
  }
  bf16_t* prow = dphi + krow * Dp;
  bf16_t* grow = dg + krow * Cg;
#pragma unroll
  for (int g4 = 0; g4 < 4; g4++) {
    const int c0 = 8 * g4 + 4 * h;
    if (c0 < Dp) {
      u32x2 v = {pack2bf(dph[4 * g4 + 0], dph[4 * g4 + 1]), pack2bf(dph[4 * g4 + 2], dph[4 * g4 + 3])};
      *(u32x2*)(prow + c0) = v;
    }
  }
#pragma unroll
  for (int cg = 0; cg < NCG; cg++)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
      const int c0 = cg * 32 + 8 * g4 + 4 * h;
      if (c0 < Cg) {
        u32x2 v = {pack2bf(dgt[cg][4 * g4 + 0], dgt[cg][4 * g4 + 1]), pack2bf(dgt[cg][4 * g4 + 2], dgt[cg][4 * g4 + 3])};
        *(u32x2*)(grow + c0) = v;
      }
    }
}

static bool at_ok(int B, int HW, int HW4, int Dp) {
  return B > 0 && B <= 65535 && HW % 128 == 0 && HW4 % 256 == 0 && Dp % 8 == 0 && Dp >= 8 && Dp <= 32;
}
// keys AND values stream in 256-key chunks: (1 + ncg) * 16 KiB of LDS whatever HW4 is (BigGAN-deep-256's discriminator attends over 128 x 128 = 16384
// queries x 4096 keys: reference src/models/big_resnet_deep_legacy.py:80-95)
extern "C" int sg_attn_fwd_flash_ok(int B, int HW, int HW4, int Dp, int Cg) {
  return (at_ok(B, HW, HW4, Dp) && Cg % 8 == 0 && Cg >= 8 && Cg <= 128) ? 1 : 0;
}
// O = softmax(theta phi^T) g in one launch; O32 (may be NULL): unrounded fp32 copy of O for sg_attn_bwd_fused
extern "C" int sg_attn_fwd_fused(const void* theta, const void* phi, const void* g, float* lse, void* O, float* O32, int B, int HW, int HW4, int Dp, int Cg, sg_stream_t s) {
  SG_CHECK(theta && phi && g && lse && O, "sg_attn_fwd_fused: null");
  SG_CHECK(sg_attn_fwd_flash_ok(B, HW, HW4, Dp, Cg) == 1, "sg_attn_fwd_fused: unsupported shape");
  const int ncg = (Cg + 31) / 32;
  SgProfScope prof((hipStream_t)s, (double)B * HW * ((Dp + Cg) * 2.0 + 4.0) + (double)B * HW4 * (Dp + Cg) * 2.0, 5);
  const dim3 grid(HW / 128, B), blk(256);
  hipStream_t st = (hipStream_t)s;
#define ATL_LAUNCH(N)                                                                                                                     \
  {                                                                                                                                        \
    static const bool ok = lt_allow_lds(k_attn_fwd_flash<N>, (1 + N) * 16384);                                                             \
    SG_CHECK(ok, "sg_attn_fwd_fused: LDS attribute");                                                                                      \
    hipLaunchKernelGGL((k_attn_fwd_flash<N>), grid, blk, (1 + N) * 16384, st, (const bf16_t*)theta, (const bf16_t*)phi, (const bf16_t*)g, lse, (bf16_t*)O, O32, HW, HW4, Dp, Cg); \
  }
  if (ncg == 1) ATL_LAUNCH(1) else if (ncg == 2) ATL_LAUNCH(2) else if (ncg == 3) ATL_LAUNCH(3) else ATL_LAUNCH(4)
#undef ATL_LAUNCH
  SG_LAUNCH_CHECK();
  return 0;
}
// fused backward (no P, no dS in HBM): dtheta [B][HW][Dp], dphi [B][HW4][Dp], dg [B][HW4][Cg] (pooled keys / values), delta = fp32 scratch [B][HW]
extern "C" int sg_attn_bwd_fused_ok(int B, int HW, int HW4, int Dp, int Cg) {
  return (at_ok(B, HW, HW4, Dp) && HW % 256 == 0 && HW4 % 128 == 0 && Cg % 8 == 0 && Cg >= 8 && Cg <= 128) ? 1 : 0;
}
extern "C" int sg_attn_bwd_fused(const void* theta, const void* phi, const void* g, const void* dO, const float* O32, const float* lse, float* delta, void* dtheta, void* dphi,
                                 void* dg, int B, int HW, int HW4, int Dp, int Cg, sg_stream_t s) {
  SG_CHECK(theta && phi && g && dO && lse && delta && dtheta && dphi && dg, "sg_attn_bwd_fused: null");
  SG_CHECK(sg_attn_bwd_fused_ok(B, HW, HW4, Dp, Cg) == 1, "sg_attn_bwd_fused: unsupported shape");
  const int ncg = (Cg + 31) / 32;
  const int lds_q = (1 + ncg) * 256 * 64, lds_k = (1 + ncg) * 256 * 64 + 2 * 256 * 4;
  SgProfScope prof((hipStream_t)s, 2.0 * ((double)B * HW * ((Dp + Cg) * 2.0 + 8.0) + (double)B * HW4 * (Dp + Cg) * 2.0) + (double)B * (HW + HW4) * (Dp * 2.0) + (double)B * HW4 * Cg * 2.0, 5);
  hipStream_t st = (hipStream_t)s;
#define ATB_LAUNCH(N)                                                                                                                     \
  {                                                                                                                                        \
    static const bool ok = lt_allow_lds(k_attn_bwd_q<N>, lds_q) && lt_allow_lds(k_attn_bwd_k<N>, lds_k);                                   \
    SG_CHECK(ok, "sg_attn_bwd_fused: LDS attribute");                                                                                      \
    hipLaunchKernelGGL(k_attn_bwd_q<N>, dim3(HW / 128, B), dim3(256), lds_q, st, (const bf16_t*)theta, (const bf16_t*)phi, (const bf16_t*)g, (const bf16_t*)dO, O32, lse, delta, (bf16_t*)dtheta, HW, HW4, Dp, Cg); \
    hipLaunchKernelGGL(k_attn_bwd_k<N>, dim3(HW4 / 128, B), dim3(256), lds_k, st, (const bf16_t*)theta, (const bf16_t*)phi, (const bf16_t*)g, (const bf16_t*)dO, lse, (const float*)delta, (bf16_t*)dphi, (bf16_t*)dg, HW, HW4, Dp, Cg); \
  }
  if (ncg == 1) ATB_LAUNCH(1) else if (ncg == 2) ATB_LAUNCH(2) else if (ncg == 3) ATB_LAUNCH(3) else ATB_LAUNCH(4)
#undef ATB_LAUNCH
  SG_LAUNCH_CHECK();
  return 0;
}
