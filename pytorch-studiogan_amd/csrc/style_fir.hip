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
// row loops below have static register indices for every fh, fw <= 4. Staged through LDS once per workgroup (f flipped as sg_upfirdn2d flips it, gain folded in).
__device__ __forceinline__ void fir_stage_taps(float (&F)[4][4], const float* f, int fh, int fw, int flip, float fgain) {
  __shared__ float sf[16];
  const int dy = 4 - fh, dx = 4 - fw;
  if (threadIdx.x < 16) {
    const int fy = (int)(threadIdx.x >> 2) - dy, fx = (int)(threadIdx.x & 3) - dx;
    float v = 0.f;
    if (fy >= 0 && fx >= 0) {
      const int sy = flip ? fy : fh - 1 - fy, sx = flip ? fx : fw - 1 - fx;
      v = f[sy * fw + sx] * fgain;
    }
    sf[threadIdx.x] = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) F[i][j] = sf[i * 4 + j];
}

// strip height of the row-walking kernels: as tall as leaves the chip ~half a million threads (the rows a strip re-reads from its neighbour are (fh - 1) / TY
// of the input); -> workgroups of 256 threads for per_row threads per strip
static unsigned fir_strip_grid(long long per_row, int Ho, int& TY, int& strips) {
  TY = 32;
  while (TY > 4 && per_row * ((Ho + TY - 1) / TY) < (1ll << 19)) TY >>= 1;
  strips = (Ho + TY - 1) / TY;
  long long blocks = (per_row * strips + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  return (unsigned)blocks;
}

template <typename T, int V>
__global__ __launch_bounds__(256) void k_fir_bias_act_nhwc(FirArgs a) {
  // (fir_stage_taps, spelled out: calling the helper here moved this kernel's instruction stream, and this kernel's code is to stay as it was measured)
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
  const unsigned blocks = fir_strip_grid(per_row, a.Ho, a.TY, a.strips);
  if (vec) hipLaunchKernelGGL((k_fir_bias_act_nhwc<T, VEC>), dim3(blocks), dim3(256), 0, st, a);
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

// ---- sg_act_fir_nhwc: the head of a down layer ------------------------------------------------------------------------------------------
//
// A DiscriminatorBlock's down = 2 layer is  bias_act of the convolution in front -> 4x4 low-pass on the full-resolution map -> stride-2 convolution. As a chain
// that is sg_bias_act, NHWC->NCHW, sg_upfirdn2d, NCHW->NHWC between the two convolutions. Here the activation moves to the LOAD side of the same FIR:
//
//   a[n][iy][ix][c] = clamp( gain * act( x[n][iy][ix][c] + bias[c] ) )   inside the image,  0 outside (the padding is zeros of the ACTIVATED map, not act(bias))
//   y[n][oy][ox][c] = sum_{fy,fx} F[fy][fx] a[n][oy * down - pady0 + fy][ox * down - padx0 + fx][c]
//
// a is evaluated in fp32 on the loaded value and never stored; the one rounding is the store of y. Same shape as k_fir_bias_act_nhwc (a kernel of its own, so
// that kernel's code does not move): one thread, one 16-byte channel vector of one output column, a strip of output rows; every input row is loaded once and
// feeds the 4 / down output rows it reaches, which wait in fp32 accumulators; no LDS tile. Output row oy takes tap row i from the (padded) input row
// oy * down + i, so the rows arrive in ascending tap order and the summation order is sg_upfirdn2d's: with no gate the result equals upfirdn2d(..., down) on
// the NCHW copy bit for bit.
//
// sg_act_fir_nhwc_bwd: dx = (adjoint FIR of dy) * da/dx in one launch. The adjoint is sg_upfirdn2d with up = down, the filter reversed and the padding the
// caller derives (upfirdn2d.py); da/dx is re-evaluated from the kept x and bias (gain or gain * alpha, 0 where the forward clamped). One thread per dx vector,
// the polyphase tap loops written as k_upfirdn2d writes them (bit-identical with no gate); dy is a quarter of dx at down = 2 and its 2 x 2 reads per output
// are shared between neighbouring threads through the cache.
static long long g_act_fir_launches = 0;
extern "C" long long sg_act_fir_launches() { return __atomic_load_n(&g_act_fir_launches, __ATOMIC_RELAXED); }

struct ActFirArgs {
  const void* x; const float* f; void* y; const float* bias; const void* dy;
  int N, Hi, Wi, C, Ho, Wo, fh, fw, padx0, pady0, flip, act, gate, TY, strips;
  float fgain, alpha, gain, clamp;
};

// One step of a tap chain, s + f * x. sg_upfirdn2d's `s += f * x` compiles to an FMA chain on the device; whether the compiler contracts the same expression
// here depends on what surrounds it (the scalar instantiation kept a multiply and an add next to the border selects, one ulp off), so the device build asks for
// the FMA by name. A host build of these sources (tests/hipemu, no contraction anywhere) keeps the plain expression, which is again what sg_upfirdn2d does there.
__device__ __forceinline__ float fir_mad(float f, float x, float s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fmaf(f, x, s);
#else
  return s + f * x;
#endif
}

__device__ __forceinline__ float act_fir_gate(float v, float b, const ActFirArgs& a) {
  v += b;
  if (a.act == 3) v = v > 0.f ? v : v * a.alpha;
  v *= a.gain;
  if (a.clamp >= 0.f) v = (v > -a.clamp && v < a.clamp) ? v : (v >= 0.f ? a.clamp : -a.clamp);
  return v;
}

template <typename T, int V, int DOWN>
__global__ __launch_bounds__(256) void k_act_fir_nhwc(ActFirArgs a) {
  constexpr int NACC = 4 / DOWN;      // output rows one input row reaches
  const int dy = 4 - a.fh, dx = 4 - a.fw;
  float F[4][4];
  fir_stage_taps(F, a.f, a.fh, a.fw, a.flip, a.fgain);
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
    float bv[V];
#pragma unroll
    for (int e = 0; e < V; e++) bv[e] = a.bias ? a.bias[c0 + e] : 0.f;
    float acc[NACC][V];   // acc[j]: output row p - (NACC - 1) + j, which takes tap row s + DOWN * (NACC - 1 - j) of the padded input row p * DOWN + s
#pragma unroll
    for (int j = 0; j < NACC; j++)
#pragma unroll
      for (int e = 0; e < V; e++) acc[j][e] = 0.f;
    const int ix0 = ox * DOWN - px;
    for (int p = oy0; p <= oy1 + NACC - 2; p++) {
#pragma unroll
      for (int s = 0; s < DOWN; s++) {
        const int iy = p * DOWN + s - py;
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
        if (a.gate && rowin) {      // (after all four loads are issued, so that they are in flight together; only pixels inside the image are activated)
#pragma unroll
          for (int fx = 0; fx < 4; fx++) {
            const int ix = ix0 + fx;
            if (fx >= dx && ix >= 0 && ix < a.Wi) {
#pragma unroll
              for (int e = 0; e < V; e++) xv[fx][e] = act_fir_gate(xv[fx][e], bv[e], a);
            }
          }
        }
#pragma unroll
        for (int j = 0; j < NACC; j++)
#pragma unroll
          for (int e = 0; e < V; e++) {
            float sum = 0.f;
#pragma unroll
            for (int fx = 0; fx < 4; fx++) sum = fir_mad(F[s + DOWN * (NACC - 1 - j)][fx], xv[fx][e], sum);      // (sg_upfirdn2d's chain)
            acc[j][e] += sum;
          }
      }
      const int oy = p - (NACC - 1);
      if (oy >= oy0) {      // (oy < oy1 by the loop bound)
        float o[V];
#pragma unroll
        for (int e = 0; e < V; e++) o[e] = acc[0][e];
        *(vec_t<T, V>*)(yn + ((long long)oy * a.Wo + ox) * a.C) = pack_f<T, V>(o);
      }
#pragma unroll
      for (int e = 0; e < V; e++) {
#pragma unroll
        for (int j = 0; j + 1 < NACC; j++) acc[j][e] = acc[j + 1][e];
        acc[NACC - 1][e] = 0.f;
      }
    }
  }
}

// dx [N][Hi][Wi][C] from dy [N][Ho][Wo][C] (a.y = dx; a.padx0 / a.pady0 / a.flip are the ADJOINT's, up = DOWN)
template <typename T, int V, int UP>
__global__ __launch_bounds__(256) void k_act_fir_nhwc_bwd(ActFirArgs a) {
  __shared__ float sf[16];
  if (threadIdx.x < a.fh * a.fw) {
    const int fy = threadIdx.x / a.fw, fx = threadIdx.x - fy * a.fw;
    const int sy = a.flip ? fy : a.fh - 1 - fy, sx = a.flip ? fx : a.fw - 1 - fx;
    sf[threadIdx.x] = a.f[sy * a.fw + sx] * a.fgain;
  }
  __syncthreads();
  const int CV = a.C / V;
  const long long total = (long long)a.N * a.Hi * a.Wi * CV;
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
    const int cv = (int)(t % CV);
    long long r = t / CV;
    const int ix = (int)(r % a.Wi); r /= a.Wi;
    const int iy = (int)(r % a.Hi);
    const int n = (int)(r / a.Hi);
    const int c0 = cv * V;
    const T* gn = (const T*)a.dy + (long long)n * a.Ho * a.Wo * a.C + c0;
    const int uy0 = iy - a.pady0, ux0 = ix - a.padx0;
    const int fy0 = ((-uy0) % UP + UP) % UP, fx0 = ((-ux0) % UP + UP) % UP;
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; e++) acc[e] = 0.f;
    for (int fy = fy0; fy < a.fh; fy += UP) {
      const int u = uy0 + fy;
      if (u < 0) continue;
      const int gy = u / UP;
      if (gy >= a.Ho) break;
      const float* frow = sf + fy * a.fw;
      float s[V];
#pragma unroll
      for (int e = 0; e < V; e++) s[e] = 0.f;
      for (int fx = fx0; fx < a.fw; fx += UP) {
        const int v = ux0 + fx;
        if (v < 0) continue;
        const int gx = v / UP;
        if (gx >= a.Wo) break;
        float g[V];
        load_f<T, V>(gn + ((long long)gy * a.Wo + gx) * a.C, g);
#pragma unroll
        for (int e = 0; e < V; e++) s[e] = fir_mad(frow[fx], g[e], s[e]);
      }
#pragma unroll
      for (int e = 0; e < V; e++) acc[e] += s[e];
    }
    const long long off = (((long long)n * a.Hi + iy) * a.Wi + ix) * a.C + c0;
    if (a.gate) {       // da/dx from the kept forward input: the side of the activation, and whether the forward clamped
      float xv[V];
      load_f<T, V>((const T*)a.x + off, xv);
#pragma unroll
      for (int e = 0; e < V; e++) {
        const float v = xv[e] + (a.bias ? a.bias[c0 + e] : 0.f);
        const bool pos = a.act != 3 || v > 0.f;
        const float yv = (pos ? v : v * a.alpha) * a.gain;
        float g = pos ? acc[e] : acc[e] * a.alpha;
        g *= a.gain;
        if (a.clamp >= 0.f && !(yv > -a.clamp && yv < a.clamp)) g = 0.f;
        acc[e] = g;
      }
    }
    *(vec_t<T, V>*)((T*)a.y + off) = pack_f<T, V>(acc);
  }
}

template <typename T, int DOWN> static void act_fir_launch(ActFirArgs& a, bool bwd, hipStream_t st) {
  constexpr int VEC = ET<T>::VEC;
  const bool vec = a.C % VEC == 0 && ((((uintptr_t)a.x) | ((uintptr_t)a.y) | ((uintptr_t)a.dy)) & 15) == 0;
  const int cvn = vec ? a.C / VEC : a.C;
  if (bwd) {
    const long long total = (long long)a.N * a.Hi * a.Wi * cvn;
    long long blocks = (total + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    if (vec) hipLaunchKernelGGL((k_act_fir_nhwc_bwd<T, VEC, DOWN>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_act_fir_nhwc_bwd<T, 1, DOWN>), dim3((unsigned)blocks), dim3(256), 0, st, a);
    return;
  }
  const long long per_row = (long long)a.N * a.Wo * cvn;
  const unsigned blocks = fir_strip_grid(per_row, a.Ho, a.TY, a.strips);
  if (vec) hipLaunchKernelGGL((k_act_fir_nhwc<T, VEC, DOWN>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_act_fir_nhwc<T, 1, DOWN>), dim3((unsigned)blocks), dim3(256), 0, st, a);
}

static int act_fir_run(const char* who, bool bwd, int dtype, const void* x, const void* dy, const float* f, void* out, const float* bias, int N, int Hi, int Wi,
                       int C, int fh, int fw, int down, int padx0, int padx1, int pady0, int pady1, int flip_filter, float filter_gain, int act, float alpha,
                       float gain, float clamp, hipStream_t st) {
  char msg[160];
#define AF_CHECK(cond, text) do { if (!(cond)) { snprintf(msg, sizeof msg, "%s: %s", who, text); sg_set_error(msg); return -1; } } while (0)
  AF_CHECK(f && out && N > 0 && Hi > 0 && Wi > 0 && C > 0, "bad tensor arguments");
  AF_CHECK(dtype == SG_DTYPE_F32 || dtype == SG_DTYPE_BF16, "fp32 / bf16 only");
  AF_CHECK(down == 1 || down == 2, "down must be 1 or 2");
  AF_CHECK(fh >= 1 && fh <= 4 && fw >= 1 && fw <= 4, "filters of 1..4 taps per axis only (sg_upfirdn2d takes the others)");
  AF_CHECK(act == 1 || act == 3, "activation linear (1) or lrelu (3) only (sg_bias_act takes the others)");
  AF_CHECK(Hi < (1 << 24) && Wi < (1 << 24) && abs(padx0) < (1 << 24) && abs(pady0) < (1 << 24) && abs(padx1) < (1 << 24) && abs(pady1) < (1 << 24),
           "image extent or padding too large");
  const long long Hp = (long long)Hi + pady0 + pady1 - fh, Wp = (long long)Wi + padx0 + padx1 - fw;
  AF_CHECK(Hp >= 0 && Wp >= 0, "empty output (padded image smaller than the filter)");
  const bool gate = bias || act != 1 || gain != 1.f || clamp >= 0.f;
  AF_CHECK(bwd ? (dy && (x || !gate)) : x != nullptr, "bad tensor arguments");
  ActFirArgs a;
  a.x = x; a.f = f; a.y = out; a.bias = bias; a.dy = dy;
  a.N = N; a.Hi = Hi; a.Wi = Wi; a.C = C; a.Ho = (int)(Hp / down + 1); a.Wo = (int)(Wp / down + 1); a.fh = fh; a.fw = fw;
  a.act = act; a.gate = gate ? 1 : 0; a.TY = 0; a.strips = 0; a.fgain = filter_gain; a.alpha = alpha; a.gain = gain; a.clamp = clamp;
  if (bwd) {      // the adjoint of upfirdn (upfirdn2d.py: up <-> down, the filter reversed); with up = down its far padding never enters the kernel
    a.padx0 = fw - padx0 - 1; a.pady0 = fh - pady0 - 1; a.flip = flip_filter ? 0 : 1;
  } else {
    a.padx0 = padx0; a.pady0 = pady0; a.flip = flip_filter ? 1 : 0;
  }
#undef AF_CHECK
  if (dtype == SG_DTYPE_F32) { if (down == 1) act_fir_launch<float, 1>(a, bwd, st); else act_fir_launch<float, 2>(a, bwd, st); }
  else { if (down == 1) act_fir_launch<bf16_t, 1>(a, bwd, st); else act_fir_launch<bf16_t, 2>(a, bwd, st); }
  SG_LAUNCH_CHECK();
  __atomic_fetch_add(&g_act_fir_launches, 1, __ATOMIC_RELAXED);
  return 0;
}

extern "C" int sg_act_fir_nhwc(int dtype, const void* x, const float* f, void* y, const float* bias, int N, int Hi, int Wi, int C, int fh, int fw, int down,
                               int padx0, int padx1, int pady0, int pady1, int flip_filter, float filter_gain, int act, float alpha, float gain, float clamp,
                               sg_stream_t s) {
  return act_fir_run("sg_act_fir_nhwc", false, dtype, x, nullptr, f, y, bias, N, Hi, Wi, C, fh, fw, down, padx0, padx1, pady0, pady1, flip_filter, filter_gain,
                     act, alpha, gain, clamp, (hipStream_t)s);
}

extern "C" int sg_act_fir_nhwc_bwd(int dtype, const void* x, const void* dy, const float* f, void* dx, const float* bias, int N, int Hi, int Wi, int C, int fh,
                                   int fw, int down, int padx0, int padx1, int pady0, int pady1, int flip_filter, float filter_gain, int act, float alpha,
                                   float gain, float clamp, sg_stream_t s) {
  return act_fir_run("sg_act_fir_nhwc_bwd", true, dtype, x, dy, f, dx, bias, N, Hi, Wi, C, fh, fw, down, padx0, padx1, pady0, pady1, flip_filter, filter_gain,
                     act, alpha, gain, clamp, (hipStream_t)s);
}
