// style_fir.hip -- sg_fir_bias_act_nhwc: a small 2-D FIR on an NHWC tensor with the tail of a StyleGAN2 synthesis layer in its epilogue.
//
// An up = 2 SynthesisLayer is  transposed 3x3 convolution -> [2H+1]^2 core -> 4x4 low-pass (pad 1/1, gain 4) -> + noise -> + bias -> lrelu -> gain -> clamp.
// The convolution kernel (modconv.hip) writes the core channels-last; as a chain of operators the rest is an NHWC->NCHW copy, sg_upfirdn2d, a torch add, an
// NCHW->NHWC copy and sg_bias_act: five passes over the full-resolution activation. Here it is one:
//
//   y[n][oy][ox][c] = clamp( gain * act( sum_{fy,fx} F[fy][fx] x[n][oy - pady0 + fy][ox - padx0 + fx][c]  + noise[n][oy][ox] + bias[c] ) )
//
// F = f * fgain, flipped in both axes unless flip_filter (sg_upfirdn2d's convention: without the flag a true convolution); pixels outside x are zero, a negative
// padding crops. Everything after the sum is optional and applied to the fp32 accumulator; the one rounding is the store. With no epilogue the kernel is a
// plain NHWC FIR (the operator's backward: flipped filter, adjoint padding).
//
// HBM-bound. One thread owns V channels (one 16-byte vector; V = 1 on the scalar path for C % VEC != 0 or unaligned tensors) of ONE output column and walks
// down a strip of TY output rows. Every input row it loads (fw vectors) is used for the fh output rows it touches at once: the fh pending rows live in fp32
// accumulators, so vertical reuse is in registers and each thread loads (TY + fh - 1) fw vectors for TY outputs. Horizontal reuse (neighbouring columns read
// the same fw - 1 vectors) is between adjacent lanes / waves of one workgroup, i.e. served by the vector L1 / L2, never HBM. Consecutive threads run along
// C then x, so every wave load is contiguous. No LDS tile: nothing is shared that the cache does not already hold, and no barrier sits in the row loop.
//
// Summation order = sg_upfirdn2d's: per tap row an FMA chain over fx ascending from zero, the rows added in ascending fy. The plain mode is therefore
// bit-identical in fp32 to sg_upfirdn2d on the NCHW copy (a tap outside the image adds a zero here and is skipped there).
#include "common.h"
#include "../../include/sgamd.h"

static long long g_fir_launches = 0;
extern "C" long long sg_fir_bias_act_launches() { return __atomic_load_n(&g_fir_launches, __ATOMIC_RELAXED); }

struct FirArgs {
  const void* x; const float* f; void* y; const float* noise; const float* bias;
  long long noise_stride;
  int N, Hi, Wi, C, Ho, Wo, fh, fw, padx0, pady0, flip, act, TY, strips;
  float fgain, alpha, gain, clamp;
};

// The filter sits in the bottom-right corner of a 4 x 4 tap table (rows / columns in front of it are zero and pady0 / padx0 grow by the same amount), so the
// row loop below has static register indices for every fh, fw <= 4.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_fir_bias_act_nhwc(FirArgs a) {
  __shared__ float sf[16];
  const int dy = 4 - a.fh, dx = 4 - a.fw;
  if (threadIdx.x < 16) {
    const int fy = (int)(threadIdx.x >> 2) - dy, fx = (int)(threadIdx.x & 3) - dx;
    float v = 0.f;
    if (fy >= 0 && fx >= 0) {
      const int sy = a.flip ? fy : a.fh - 1 - fy, sx = a.flip ? fx : a.fw - 1 - fx;
      v = a.f[sy * a.fw + sx] * a.fgain;
    }
    sf[threadIdx.x] = v;
  }
  __syncthreads();
  float F[4][4];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) F[i][j] = sf[i * 4 + j];
  const int py = a.pady0 + dy, px = a.padx0 + dx;
  const int CV = a.C / V;
  const long long total = (long long)a.N * a.strips * a.Wo * CV;
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int cv = (int)(t % CV);
    long long r = t / CV;
    const int ox = (int)(r % a.Wo); r /= a.Wo;
    const int strip = (int)(r % a.strips);
    const int n = (int)(r / a.strips);
    const int c0 = cv * V;
    const int oy0 = strip * a.TY, oy1 = oy0 + a.TY < a.Ho ? oy0 + a.TY : a.Ho;
    const T* xn = (const T*)a.x + (long long)n * a.Hi * a.Wi * a.C + c0;
    T* yn = (T*)a.y + (long long)n * a.Ho * a.Wo * a.C + c0;
    const float* nz = a.noise ? a.noise + (long long)n * a.noise_stride : nullptr;
    float bv[V];
#pragma unroll
    for (int e = 0; e < V; e++) bv[e] = a.bias ? a.bias[c0 + e] : 0.f;
    float acc[4][V];      // acc[j]: output row iy + py - 3 + j, which takes tap row 3 - j of the input row iy
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int e = 0; e < V; e++) acc[j][e] = 0.f;
    const int ix0 = ox - px;
    // (loading a row ahead of the one being summed was measured and lost: +16 / +32 VGPRs, 3187 against 4327 GB/s in fp32 at 128 x 256^2, no change in bf16)
    for (int iy = oy0 - py; iy <= oy1 + 2 - py; iy++) {
      float xv[4][V];
      const bool rowin = iy >= 0 && iy < a.Hi;
#pragma unroll
      for (int fx = 0; fx < 4; fx++) {
        const int ix = ix0 + fx;
        if (fx >= dx && rowin && ix >= 0 && ix < a.Wi) load_f<T, V>(xn + ((long long)iy * a.Wi + ix) * a.C, xv[fx]);
        else {
#pragma unroll
          for (int e = 0; e < V; e++) xv[fx][e] = 0.f;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; j++)
#pragma unroll
        for (int e = 0; e < V; e++) {
          float s = 0.f;
#pragma unroll
          for (int fx = 0; fx < 4; fx++) s += F[3 - j][fx] * xv[fx][e];      // (written as sg_upfirdn2d writes it: the compiler contracts both alike)
          acc[j][e] += s;
        }
      const int oy = iy + py - 3;
      if (oy >= oy0) {      // (oy < oy1 by the loop bound)
        float o[V];
        const float nv = nz ? nz[(long long)oy * a.Wo + ox] : 0.f;
#pragma unroll
        for (int e = 0; e < V; e++) {
          float v = acc[0][e];
          if (nz) v += nv;
          if (a.bias) v += bv[e];
          if (a.act == 3) v = v > 0.f ? v : v * a.alpha;
          v *= a.gain;
          if (a.clamp >= 0.f) v = (v > -a.clamp && v < a.clamp) ? v : (v >= 0.f ? a.clamp : -a.clamp);
          o[e] = v;
        }
        *(vec_t<T, V>*)(yn + ((long long)oy * a.Wo + ox) * a.C) = pack_f<T, V>(o);
      }
#pragma unroll
      for (int e = 0; e < V; e++) { acc[0][e] = acc[1][e]; acc[1][e] = acc[2][e]; acc[2][e] = acc[3][e]; acc[3][e] = 0.f; }
    }
  }
}

template <typename T> static void fir_launch(FirArgs& a, hipStream_t st) {
  constexpr int VEC = ET<T>::VEC;
  const bool vec = a.C % VEC == 0 && ((((uintptr_t)a.x) | ((uintptr_t)a.y)) & 15) == 0;
  const long long per_row = (long long)a.N * a.Wo * (vec ? a.C / VEC : a.C);
  // strip height: as tall as leaves the chip ~half a million threads (the rows a strip re-reads from its neighbour are (fh - 1) / TY of the input)
  int TY = 32;
  while (TY > 4 && per_row * ((a.Ho + TY - 1) / TY) < (1ll << 19)) TY >>= 1;
  a.TY = TY;
  a.strips = (a.Ho + TY - 1) / TY;
  const long long total = per_row * a.strips;
  long long blocks = (total + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  if (vec) hipLaunchKernelGGL((k_fir_bias_act_nhwc<T, VEC>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_fir_bias_act_nhwc<T, 1>), dim3((unsigned)blocks), dim3(256), 0, st, a);
}

extern "C" int sg_fir_bias_act_nhwc(int dtype, const void* x, const float* f, void* y, const float* noise, long long noise_stride, const float* bias,
                                    int N, int Hi, int Wi, int C, int fh, int fw, int padx0, int padx1, int pady0, int pady1, int flip_filter,
                                    float filter_gain, int act, float alpha, float gain, float clamp, sg_stream_t s) {
  SG_CHECK(x && f && y && N > 0 && Hi > 0 && Wi > 0 && C > 0, "sg_fir_bias_act_nhwc: bad tensor arguments");
  SG_CHECK(dtype == SG_DTYPE_F32 || dtype == SG_DTYPE_BF16, "sg_fir_bias_act_nhwc: fp32 / bf16 only");
  SG_CHECK(fh >= 1 && fh <= 4 && fw >= 1 && fw <= 4, "sg_fir_bias_act_nhwc: filters of 1..4 taps per axis only (sg_upfirdn2d takes the others)");
  SG_CHECK(act == 1 || act == 3, "sg_fir_bias_act_nhwc: activation linear (1) or lrelu (3) only (sg_bias_act takes the others)");
  const long long Ho = (long long)Hi + pady0 + pady1 - fh + 1, Wo = (long long)Wi + padx0 + padx1 - fw + 1;
  SG_CHECK(Ho >= 1 && Wo >= 1, "sg_fir_bias_act_nhwc: empty output (padded image smaller than the filter)");
  SG_CHECK(Ho < (1 << 24) && Wo < (1 << 24) && Hi < (1 << 24) && Wi < (1 << 24) && abs(padx0) < (1 << 24) && abs(pady0) < (1 << 24),
           "sg_fir_bias_act_nhwc: image extent or padding too large");
  SG_CHECK(!noise || noise_stride == 0 || noise_stride >= Ho * Wo, "sg_fir_bias_act_nhwc: noise_stride must be 0 (one shared plane) or >= Ho * Wo");
  FirArgs a;
  a.x = x; a.f = f; a.y = y; a.noise = noise; a.bias = bias; a.noise_stride = noise ? noise_stride : 0;
  a.N = N; a.Hi = Hi; a.Wi = Wi; a.C = C; a.Ho = (int)Ho; a.Wo = (int)Wo; a.fh = fh; a.fw = fw; a.padx0 = padx0; a.pady0 = pady0;
  a.flip = flip_filter ? 1 : 0; a.act = act; a.fgain = filter_gain; a.alpha = alpha; a.gain = gain; a.clamp = clamp;
  if (dtype == SG_DTYPE_F32) fir_launch<float>(a, (hipStream_t)s);
  else fir_launch<bf16_t>(a, (hipStream_t)s);
  SG_LAUNCH_CHECK();
  __atomic_fetch_add(&g_fir_launches, 1, __ATOMIC_RELAXED);
  return 0;
}
