// vit.hip -- token-side kernels of the DINO ViT evaluation backbone (reference src/metrics/vit.py, eval_backbone "DINO_torch"), inference only:
//
//   sg_layernorm_rows : y[r][:] = (x[r][:] - mean) * rsqrt(var + eps) * gamma + beta over fp32 rows with a row pitch (nn.LayerNorm, vit.py:92-96,237)
//   sg_vit_tokens     : class token + patch embeddings + position embedding -> fp32 residual stream (vit.py:185-196, identity branch of the interpolation)
//   sg_gelu_f32       : exact (erf) GELU, fp32 -- the composed fp32 path only; the bf16 path has it in the fc1 epilogue
//   sg_tok_gemm       : out[m][n] = epi(sum_k a[m][k] w[n][k] + bias[n]), bf16 operands, fp32 accumulation (nn.Linear over [B * N_tok] rows)
//
// sg_tok_gemm. One workgroup = 4 waves = a 128 (tokens) x 128 (features) tile, each wave 64 x 64 as 2 x 2 MFMA 32x32x16 tiles with A = WEIGHT rows and
// B = TOKEN rows: a lane then owns ONE token and, per register group, four consecutive output features -- bias / GELU / residual run on 8- or 16-byte
// pieces of an output row without any cross-lane movement. Both operands are k-contiguous ([row][k]), staged 64 channels per step as two [128][32 ch]
// images of 64-byte rows (the LDS tile image of lds_tile.h, which attn.hip established), two stages: the DMA of step t + 1 flies under the MFMAs of step t, one
// barrier per step, in front of which every wave retires its own DMA (lt_drain_barrier). Rows beyond M (B * 785 is a multiple of nothing) and beyond N are
// fetched from a zero line instead of memory and masked at the store.
#include "common.h"
#include "lds_tile.h"
#include "../../include/sgamd.h"

static long long g_tok_gemm_launches = 0;

static inline int vt_grid1d(long long total) { long long b = (total + 255) / 256; if (b > 256 * 32) b = 256 * 32; if (b < 1) b = 1; return (int)b; }

// ---- LayerNorm over rows: one wave per row, the row in registers (two 16-byte loads per 8-channel group), centred variance like torch ----------------------
template <typename TO, int MAXG>
__global__ __launch_bounds__(256) void k_layernorm_rows(const float* x, long long pitch, const float* gamma, const float* beta, TO* y, long long ldo, int rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                   // whole waves only; no barrier in this kernel
  const int groups = C >> 3;
  const float* xr = x + (long long)row * pitch;
  float v[MAXG][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < MAXG; i++) {
    const int g = lane + 64 * i;
    if (g < groups) {
      const f32x4 a = *(const f32x4*)(xr + 8 * g), b = *(const f32x4*)(xr + 8 * g + 4);
#pragma unroll
      for (int e = 0; e < 4; e++) { v[i][e] = a[e]; v[i][4 + e] = b[e]; sum += a[e] + b[e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; e++) v[i][e] = 0.f;
    }
  }
  const float mean = wave_sum(sum) / (float)C;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < MAXG; i++)
    if (lane + 64 * i < groups) {
#pragma unroll
      for (int e = 0; e < 8; e++) { v[i][e] -= mean; sq += v[i][e] * v[i][e]; }
    }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)C + eps);
  TO* yr = y + (long long)row * ldo;
#pragma unroll
  for (int i = 0; i < MAXG; i++) {
    const int g = lane + 64 * i;
    if (g < groups) {
      const f32x4 ga = *(const f32x4*)(gamma + 8 * g), gb = *(const f32x4*)(gamma + 8 * g + 4);
      const f32x4 ba = *(const f32x4*)(beta + 8 * g), bb = *(const f32x4*)(beta + 8 * g + 4);
      float o[8];
#pragma unroll
      for (int e = 0; e < 4; e++) { o[e] = v[i][e] * rstd * ga[e] + ba[e]; o[4 + e] = v[i][4 + e] * rstd * gb[e] + bb[e]; }
      if (sizeof(TO) == 2) {
        u32x4 p = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7])};
        *(u32x4*)(yr + 8 * g) = p;
      } else {
        const f32x4 p0 = {o[0], o[1], o[2], o[3]}, p1 = {o[4], o[5], o[6], o[7]};
        *(f32x4*)((float*)yr + 8 * g) = p0;
        *(f32x4*)((float*)yr + 8 * g + 4) = p1;
      }
    }
  }
}

template <typename TO> static void layernorm_launch(const float* x, long long pitch, const float* gamma, const float* beta, void* y, long long ldo, int rows, int C, float eps, hipStream_t st) {
  const dim3 grid((rows + 3) / 4), blk(256);
  if (C <= 512) hipLaunchKernelGGL((k_layernorm_rows<TO, 1>), grid, blk, 0, st, x, pitch, gamma, beta, (TO*)y, ldo, rows, C, eps);
  else if (C <= 1024) hipLaunchKernelGGL((k_layernorm_rows<TO, 2>), grid, blk, 0, st, x, pitch, gamma, beta, (TO*)y, ldo, rows, C, eps);
  else hipLaunchKernelGGL((k_layernorm_rows<TO, 4>), grid, blk, 0, st, x, pitch, gamma, beta, (TO*)y, ldo, rows, C, eps);
}

extern "C" int sg_layernorm_rows(int out_dtype, const float* x, long long pitch, const float* gamma, const float* beta, void* y, long long ldo, int rows, int C,
                                 float eps, sg_stream_t s) {
  SG_CHECK(x && gamma && beta && y && rows > 0, "sg_layernorm_rows: bad args");
  SG_CHECK(C >= 8 && C % 8 == 0 && C <= 2048, "sg_layernorm_rows: C must be a multiple of 8, at most 2048");
  SG_CHECK(pitch >= C && pitch % 4 == 0 && ldo >= C && ldo % 8 == 0, "sg_layernorm_rows: row pitches must cover C and keep 16-byte alignment");
  SG_CHECK((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15) == 0, "sg_layernorm_rows: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  if (out_dtype == SG_DTYPE_BF16) layernorm_launch<bf16_t>(x, pitch, gamma, beta, y, ldo, rows, C, eps, st);
  else if (out_dtype == SG_DTYPE_F32) layernorm_launch<float>(x, pitch, gamma, beta, y, ldo, rows, C, eps, st);
  else { sg_set_error("sg_layernorm_rows: bad dtype"); return -1; }
  SG_LAUNCH_CHECK();
  return 0;
}

// ---- token assembly: x[b][0] = cls + pos[0], x[b][1 + p] = patch[b][p] + pos[1 + p], four channels per thread, everything fp32 --------------------------------
__global__ __launch_bounds__(256) void k_vit_tokens(const float* patch, const float* cls, const float* pos, float* x, int B, int N, int C) {
  const int C4 = C >> 2;
  const long long total = (long long)B * N * C4;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C4) * 4;
    const long long t = i / C4;
    const int tok = (int)(t % N), b = (int)(t / N);
    const f32x4 p = *(const f32x4*)(pos + (long long)tok * C + c);
    const f32x4 v = (tok == 0) ? *(const f32x4*)(cls + c) : *(const f32x4*)(patch + ((long long)b * (N - 1) + (tok - 1)) * C + c);
    *(f32x4*)(x + t * C + c) = v + p;
  }
}
extern "C" int sg_vit_tokens(const float* patch, const float* cls, const float* pos, float* x, int B, int N, int C, sg_stream_t s) {
  SG_CHECK(patch && cls && pos && x && B > 0 && N > 1, "sg_vit_tokens: bad args");
  SG_CHECK(C % 8 == 0, "sg_vit_tokens: C must be a multiple of 8");
  SG_CHECK((((uintptr_t)patch | (uintptr_t)cls | (uintptr_t)pos | (uintptr_t)x) & 15) == 0, "sg_vit_tokens: pointers must be 16-byte aligned");
  hipLaunchKernelGGL(k_vit_tokens, dim3(vt_grid1d((long long)B * N * (C / 4))), dim3(256), 0, (hipStream_t)s, patch, cls, pos, x, B, N, C);
  SG_LAUNCH_CHECK();
  return 0;
}

// exact GELU (nn.GELU default, vit.py:25): 0.5 x (1 + erf(x / sqrt 2))
__device__ __forceinline__ float vt_gelu(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

__global__ __launch_bounds__(256) void k_gelu_f32(const float* x, float* y, long long n4) {
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 v = ((const f32x4*)x)[i];
#pragma unroll
    for (int e = 0; e < 4; e++) v[e] = vt_gelu(v[e]);
    ((f32x4*)y)[i] = v;
  }
}
extern "C" int sg_gelu_f32(const float* x, float* y, long long n, sg_stream_t s) {
  SG_CHECK(x && y && n > 0 && n % 4 == 0, "sg_gelu_f32: n must be a positive multiple of 4");
  hipLaunchKernelGGL(k_gelu_f32, dim3(vt_grid1d(n / 4)), dim3(256), 0, (hipStream_t)s, x, y, n / 4);
  SG_LAUNCH_CHECK();
  return 0;
}

// ---- token GEMM -----------------------------------------------------------------------------------------------------------------------------------------
#define TG_BM 128
#define TG_BN 128
#define TG_IMG (128 * 64)                 // one [128 rows][32 channels] bf16 image
#define TG_STAGE (4 * TG_IMG)             // tokens k-half 0 / 1, weights k-half 0 / 1

// EPI 0: bias -> bf16; 1: bias + GELU -> bf16; 2: out(fp32) += acc + bias (the residual stream, in place)
template <int EPI>
__global__ __launch_bounds__(256) void k_tok_gemm(const bf16_t* a, int lda, const bf16_t* w, const float* bias, void* out, int ldo, int M, int N, int K) {
  extern __shared__ __attribute__((aligned(16))) char tg_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * TG_BN, m0 = blockIdx.y * TG_BM;
  const int wm = (wave & 1) * 64, wn = (wave >> 1) * 64;
  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; mi++)
#pragma unroll
    for (int ni = 0; ni < 2; ni++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[mi][ni][r] = 0.f;
  const int nk = K / 64;
  auto stage = [&](int kt) {
    char* st = tg_smem + (kt & 1) * TG_STAGE;
#pragma unroll
    for (int kh = 0; kh < 2; kh++) {
      lt_stage_rows(st + kh * TG_IMG, a, m0, M, lda, kt * 64 + kh * 32, wave, lane);
      lt_stage_rows(st + (2 + kh) * TG_IMG, w, n0, N, K, kt * 64 + kh * 32, wave, lane);
    }
  };
  stage(0);
  for (int kt = 0; kt < nk; kt++) {
    lt_drain_barrier();                                      // step kt has landed; every wave is done with the other stage
    if (kt + 1 < nk) stage(kt + 1);
    const char* st = tg_smem + (kt & 1) * TG_STAGE;
#pragma unroll
    for (int kh = 0; kh < 2; kh++)
#pragma unroll
      for (int t = 0; t < 2; t++) {
        bf16x8_t xf[2], wf[2];
#pragma unroll
        for (int i = 0; i < 2; i++) { xf[i] = lt_frag_rows(st + kh * TG_IMG, wm + 32 * i, t, lane); wf[i] = lt_frag_rows(st + (2 + kh) * TG_IMG, wn + 32 * i, t, lane); }
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
          for (int ni = 0; ni < 2; ni++) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[ni], xf[mi], acc[mi][ni], 0, 0, 0);
      }
  }
  // D[row = feature][col = token]: lane = (token, h) holds features 8 g4 + 4 h + (0..3) of each 32-feature tile
  const int h = lane >> 5;
#pragma unroll
  for (int mi = 0; mi < 2; mi++) {
    const int m = m0 + wm + 32 * mi + (lane & 31);
    if (m >= M) continue;
#pragma unroll
    for (int ni = 0; ni < 2; ni++)
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        const int n = n0 + wn + 32 * ni + 8 * g4 + 4 * h;
        if (n >= N) continue;
        const f32x4 bv = *(const f32x4*)(bias + n);
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = acc[mi][ni][4 * g4 + e] + bv[e];
        if (EPI == 2) {
          float* o = (float*)out + (long long)m * ldo + n;
          *(f32x4*)o = *(const f32x4*)o + v;
        } else {
          if (EPI == 1) {
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = vt_gelu(v[e]);
          }
          const u32x2 p = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
          *(u32x2*)((bf16_t*)out + (long long)m * ldo + n) = p;
        }
      }
  }
}

extern "C" int sg_tok_gemm(int epi, const void* a, int lda, const void* w, const float* bias, void* out, int ldo, int M, int N, int K, sg_stream_t s) {
  SG_CHECK(a && w && bias && out && M > 0, "sg_tok_gemm: bad args");
  SG_CHECK(epi >= 0 && epi <= 2, "sg_tok_gemm: epilogue must be 0 (bias), 1 (bias + GELU) or 2 (bias + fp32 residual in place)");
  SG_CHECK(K >= 64 && K % 64 == 0 && N >= 64 && N % 64 == 0, "sg_tok_gemm: K and N must be multiples of 64");
  SG_CHECK(lda >= K && lda % 8 == 0 && ldo >= N && ldo % 4 == 0, "sg_tok_gemm: row pitches must cover K / N and keep the vector alignment");
  SG_CHECK((((uintptr_t)a | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)out) & 15) == 0, "sg_tok_gemm: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)s;
  const dim3 grid((N + TG_BN - 1) / TG_BN, (M + TG_BM - 1) / TG_BM), blk(256);
  const double flops = 2.0 * (double)M * (double)N * (double)K;
#define TG_LAUNCH(E)                                                                                                                                   \
  {                                                                                                                                                    \
    static const bool ok = lt_allow_lds(k_tok_gemm<E>, 2 * TG_STAGE);                                                                                  \
    SG_CHECK(ok, "sg_tok_gemm: LDS attribute");                                                                                                        \
    SgProfScope prof(st, flops, 2);                                                                                                                    \
    hipLaunchKernelGGL((k_tok_gemm<E>), grid, blk, 2 * TG_STAGE, st, (const bf16_t*)a, lda, (const bf16_t*)w, bias, out, ldo, M, N, K);                \
  }
  if (epi == 0) TG_LAUNCH(0) else if (epi == 1) TG_LAUNCH(1) else TG_LAUNCH(2)
#undef TG_LAUNCH
  SG_LAUNCH_CHECK();
  __atomic_fetch_add(&g_tok_gemm_launches, 1, __ATOMIC_RELAXED);
  return 0;
}
extern "C" long long sg_tok_gemm_launches(void) { return __atomic_load_n(&g_tok_gemm_launches, __ATOMIC_RELAXED); }
