// mha.hip -- multi-head attention forward of the ViT evaluation backbone (reference src/metrics/vit.py:68-80): O = softmax(scale * Q K^T) V per (image, head),
// reading the packed activation [B][N][3][H][64] exactly as the qkv GEMM wrote it and writing [B][N][H * 64] bf16: no permute, no split, scores and
// probabilities never in HBM.
//
// The structure is k_attn_fwd_flash's (attn.hip): one workgroup = 4 waves = 128 queries of one (image, head); MFMA 32x32x16 with A = keys, B = queries, so a lane
// owns ONE query and 16 of the 32 keys of a block (max / sum in-lane plus one v_permlane32_swap); the bf16 probabilities go from the score accumulators
// straight into the B operand of O^T += V^T P with the V^T fragments gathered by ds_read_b64_tr_b16; one pass with a running maximum that is only raised when a
// block exceeds it by MH_THR. New here:
//   - head dimension 64: K and V are each two [keys][32 channels] images of 64-byte rows (the tile image of lds_tile.h), four score MFMAs per block;
//   - `scale` lives in the exponent's multiplier: p = exp2(s * scale * log2 e - m * log2 e);
//   - K + V of a head at N = 785 is 200 KB: keys stream in 128-key chunks through a 2-deep ring (2 x 32 KiB: two workgroups per CU), one barrier per
//     chunk. The LDS-DMA of chunk c + 1 is ISSUED in front of chunk c's arithmetic, but the code object does not let it fly under that arithmetic: hipcc
//     (ROCm 7.2) puts an `s_waitcnt vmcnt(0)` in front of the first transposing LDS read of the block loop, so a wave waits for its own share of chunk
//     c + 1 before its first P V product of chunk c. What the ring buys is overlap ACROSS waves and across the two workgroups of a CU;
//   - every wave -- the ones that skip the arithmetic included -- drains its own DMA in front of the chunk barrier (lt_drain_barrier: the ordering rule of
//     LDS-DMA is written there);
//   - ragged tail: rows >= N of a chunk are fetched from a zero line, never from beyond the tensor; their scores are set to -inf before the running maximum;
//     32-key blocks that start at or beyond N are not visited at all (a block therefore always holds a live key, and the running maximum starts at a
//     FINITE floor: no exp(-inf + inf)); queries >= N are computed on zero rows and not stored. A wave whose 32 queries all lie beyond N skips the block
//     loop as a whole wave -- it still stages and meets every barrier; partial waves run with every lane active (the transposing LDS read wants that).
#include "common.h"
#include "lds_tile.h"
#include "../../include/sgamd.h"

#ifndef MH_THR
#define MH_THR 8.0f
#endif
#define MH_KC 128
#define MH_IMG (MH_KC * 64)
#define MH_STAGE (4 * MH_IMG)            // K channels 0-31 / 32-63, V channels 0-31 / 32-63

static long long g_mha_launches = 0;

// grid (ceil(N / 128), H, B), 256 threads, 2 * MH_STAGE bytes of LDS. Two workgroups per CU (LDS), two waves per SIMD: the register budget is set to match.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_mha_fwd(const bf16_t* qkv, bf16_t* O, int N, int H, float scale) {
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) char mh_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int head = blockIdx.y, b = blockIdx.z;
  const int ld = 3 * H * 64;
  const int q = blockIdx.x * 128 + wave * 32 + (lane & 31);
  const int h = lane >> 5;
  const bool active = blockIdx.x * 128 + wave * 32 < N;            // wave-uniform
  const bf16_t* base = qkv + (long long)b * N * ld + head * 64;     // q of this head; k at + H * 64, v at + 2 * H * 64
  const bf16_t* kbase = base + H * 64;
  const bf16_t* vbase = base + 2 * H * 64;
  bf16x8_t qf[4];                                                  // channels 16 i + 8 h .. + 8 of this lane's query
  {
    const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const u32x4 v = (q < N) ? *(const u32x4*)(base + (long long)q * ld + 16 * i + 8 * h) : z;
      qf[i] = __builtin_bit_cast(bf16x8_t, v);
    }
  }
  const float c2 = scale * LOG2E;
  float m = -1.0e30f;          // running reference maximum (scaled scores, natural-log units), equal in both lane halves; finite on purpose
  float m2 = m * LOG2E;
  float l = 0.f;
  f32x16 o[2];
#pragma unroll
  for (int cg = 0; cg < 2; cg++)
#pragma unroll
    for (int r = 0; r < 16; r++) o[cg][r] = 0.f;
  auto stage = [&](int c) {
    char* st = mh_smem + (c & 1) * MH_STAGE;
    const int k0 = c * MH_KC;
    lt_stage_rows(st, kbase, k0, N, ld, 0, wave, lane);
    lt_stage_rows(st + MH_IMG, kbase, k0, N, ld, 32, wave, lane);
    lt_stage_rows(st + 2 * MH_IMG, vbase, k0, N, ld, 0, wave, lane);
    lt_stage_rows(st + 3 * MH_IMG, vbase, k0, N, ld, 32, wave, lane);
  };
  const int nch = (N + MH_KC - 1) / MH_KC;
  stage(0);
  for (int c = 0; c < nch; c++) {
    lt_drain_barrier();                                            // chunk c has landed (idle waves wait for their share nowhere else); every wave is done with the other stage
    if (c + 1 < nch) stage(c + 1);
    if (!active) continue;
    const char* kimg = mh_smem + (c & 1) * MH_STAGE;
    const char* vimg = kimg + 2 * MH_IMG;
    const int k0 = c * MH_KC;
    const int left = N - k0;                                       // live keys from the start of this chunk
    const int nb = left >= MH_KC ? MH_KC / 32 : (left + 31) / 32;
#pragma unroll 1
    for (int kc = 0; kc < nb; kc++) {
      f32x16 s;
#pragma unroll
      for (int r = 0; r < 16; r++) s[r] = 0.f;
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(kimg, kc, 0, lane), qf[0], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(kimg, kc, 1, lane), qf[1], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(kimg + MH_IMG, kc, 0, lane), qf[2], s, 0, 0, 0);
      s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_frag(kimg + MH_IMG, kc, 1, lane), qf[3], s, 0, 0, 0);
      if (kc * 32 + 32 > left) {                                   // the last, partial block: keys >= N leave before the maximum is taken
#pragma unroll
        for (int r = 0; r < 16; r++)
          if (kc * 32 + (r & 3) + 8 * (r >> 2) + 4 * h >= left) s[r] = -__builtin_inff();
      }
      float bm = s[0];
#pragma unroll
      for (int r = 1; r < 16; r++) bm = fmaxf(bm, s[r]);
      bm = lt_half_max(bm) * scale;                                // scale > 0: the maximum commutes with it
      if (bm > m + MH_THR) {                                       // (the first block always)
        const float alpha = __builtin_amdgcn_exp2f((m - bm) * LOG2E);
        l *= alpha;
#pragma unroll
        for (int cg = 0; cg < 2; cg++)
#pragma unroll
          for (int r = 0; r < 16; r++) o[cg][r] *= alpha;
        m = bm;
        m2 = m * LOG2E;
      }
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; r++) { p[r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[r], c2, -m2)); l += p[r]; }
      u32x4 pa, pb;                                                // regs 0-7 / 8-15 = contraction slots of the two k-steps
#pragma unroll
      for (int i = 0; i < 4; i++) { pa[i] = pack2bf(p[2 * i], p[2 * i + 1]); pb[i] = pack2bf(p[8 + 2 * i], p[8 + 2 * i + 1]); }
      const bf16x8_t pfa = __builtin_bit_cast(bf16x8_t, pa), pfb = __builtin_bit_cast(bf16x8_t, pb);
#pragma unroll
      for (int cg = 0; cg < 2; cg++) {
        const char* vi = vimg + cg * MH_IMG;
        o[cg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(vi, kc * 32 + 4 * h, lane), pfa, o[cg], 0, 0, 0);
        o[cg] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lt_vfrag(vi, kc * 32 + 16 + 4 * h, lane), pfb, o[cg], 0, 0, 0);
      }
    }
  }
  if (!active || q >= N) return;                                   // (no barrier behind this point)
  l = lt_half_sum(l);
  const float inv = 1.f / l;
  // O^T tile: lane = (query, h) holds channels cg * 32 + 8 * g4 + 4 h + (0..3)
  bf16_t* orow = O + ((long long)b * N + q) * (H * 64) + head * 64;
#pragma unroll
  for (int cg = 0; cg < 2; cg++)
#pragma unroll
    for (int g4 = 0; g4 < 4; g4++) {
      const u32x2 v = {pack2bf(o[cg][4 * g4 + 0] * inv, o[cg][4 * g4 + 1] * inv), pack2bf(o[cg][4 * g4 + 2] * inv, o[cg][4 * g4 + 3] * inv)};
      *(u32x2*)(orow + cg * 32 + 8 * g4 + 4 * h) = v;
    }
}

extern "C" int sg_mha_fwd_ok(int B, int N, int H, int D) {
  return (B >= 1 && B <= 65535 && N >= 1 && H >= 1 && H <= 65535 && D == 64) ? 1 : 0;
}
extern "C" int sg_mha_fwd(const void* qkv, void* out, int B, int N, int H, int D, float scale, sg_stream_t s) {
  SG_CHECK(qkv && out, "sg_mha_fwd: null pointer");
  SG_CHECK(sg_mha_fwd_ok(B, N, H, D), "sg_mha_fwd: head dimension must be 64 (ask sg_mha_fwd_ok first)");
  SG_CHECK(scale > 0.f, "sg_mha_fwd: scale must be positive");
  SG_CHECK((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "sg_mha_fwd: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  static const bool ok = lt_allow_lds(k_mha_fwd, 2 * MH_STAGE);
  SG_CHECK(ok, "sg_mha_fwd: LDS attribute");
  {
    SgProfScope prof(st, 4.0 * (double)B * H * (double)N * (double)N * 64.0, 2);
    hipLaunchKernelGGL(k_mha_fwd, dim3((N + 127) / 128, H, B), dim3(256), 2 * MH_STAGE, st, (const bf16_t*)qkv, (bf16_t*)out, N, H, scale);
  }
  SG_LAUNCH_CHECK();
  __atomic_fetch_add(&g_mha_launches, 1, __ATOMIC_RELAXED);
  return 0;
}
extern "C" long long sg_mha_launches(void) { return __atomic_load_n(&g_mha_launches, __ATOMIC_RELAXED); }
