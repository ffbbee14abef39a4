// style_fir.hip -- a small 2-D FIR on an NHWC tensor with a StyleGAN2 layer's epilogue on either side of it: one kernel, two entry points.
//
// sg_fir_bias_act_nhwc, the tail of an up = 2 SynthesisLayer:  transposed 3x3 convolution -> [2H+1]^2 core -> 4x4 low-pass (pad 1/1, gain 4) -> + noise ->
// + bias -> lrelu -> gain -> clamp. The convolution kernel (modconv.hip) writes the core channels-last; as a chain of operators the rest is an NHWC->NCHW copy,
// sg_upfirdn2d, a torch add, an NCHW->NHWC copy and sg_bias_act: five passes over the full-resolution activation. Here it is one, the epilogue at the STORE:
//
//   y[n][oy][ox][c] = clamp( gain * act( sum_{fy,fx} F[fy][fx] x[n][oy - pady0 + fy][ox - padx0 + fx][c]  + noise[n][oy][ox] + bias[c] ) )
//
// sg_act_fir_nhwc, the head of a DiscriminatorBlock's down = 2 layer:  bias_act of the convolution in front -> 4x4 low-pass on the full-resolution map ->
// stride-2 convolution. As a chain that is sg_bias_act, NHWC->NCHW, sg_upfirdn2d, NCHW->NHWC between the two convolutions. Here the epilogue is at the LOAD:
//
//   a[n][iy][ix][c] = clamp( gain * act( x[n][iy][ix][c] + bias[c] ) )   inside the image,  0 outside (the padding is zeros of the ACTIVATED map, not act(bias))
//   y[n][oy][ox][c] = sum_{fy,fx} F[fy][fx] a[n][oy * down - pady0 + fy][ox * down - padx0 + fx][c]
//
// F = f * fgain, flipped in both axes unless flip_filter (sg_upfirdn2d's convention: without the flag a true convolution); pixels outside x are zero, a negative
// padding crops. The epilogue is optional and evaluated in fp32 (on the accumulator, or on the loaded value: a is never stored); the one rounding is the store.
// With no epilogue either entry is a plain NHWC FIR (the tail's backward: flipped filter, adjoint padding).
//
// HBM-bound. One thread owns V channels (one 16-byte vector; V = 1 on the scalar path for C % VEC != 0 or unaligned tensors) of ONE output column and walks
// down a strip of TY output rows. Every input row it loads (fw vectors) is used for the 4 / down output rows it touches at once: the pending rows live in fp32
// accumulators, so vertical reuse is in registers and each thread loads (TY + fh - 1) fw vectors for TY outputs at down = 1. Horizontal reuse (neighbouring
// columns read the same fw - 1 vectors) is between adjacent lanes / waves of one workgroup, i.e. served by the vector L1 / L2, never HBM. Consecutive threads
// run along C then x, so every wave load is contiguous. No LDS tile: nothing is shared that the cache does not already hold, and no barrier sits in the row loop.
//
// Summation order = sg_upfirdn2d's: per tap row an FMA chain over fx ascending from zero, the rows added in ascending fy (output row oy takes tap row i from
// the padded input row oy * down + i, so the rows arrive in tap order). With no epilogue the result is therefore bit-identical to upfirdn2d(..., down) on the
// NCHW copy (a tap outside the image adds a zero here and is skipped there). Resources and timing against the two kernels this one replaced:
// profiles/style_fir_refactor.txt.
//
// sg_act_fir_nhwc_bwd: dx = (adjoint FIR of dy) * da/dx in one launch. The adjoint is sg_upfirdn2d with up = down, the filter reversed and the padding the
// caller derives (upfirdn2d.py); da/dx is re-evaluated from the kept x and bias (gain or gain * alpha, 0 where the forward clamped). One thread per dx vector,
// the polyphase tap loops written as k_upfirdn2d writes them (bit-identical with no gate); dy is a quarter of dx at down = 2 and its 2 x 2 reads per output
// are shared between neighbouring threads through the cache.
//
// sg_act_fir_nhwc_gate: the backward of THAT launch with respect to dy (second order, R1 through the discriminator). dx = FIR^T(dy) * m(x) is linear in dy, so
// a cotangent v on dx gives d_dy = FIR(v * m(x + bias)), decimated: the forward's strip walk with the epilogue on the load side replaced by a gate, m = da/dx
// evaluated from the kept raw x exactly as k_act_fir_nhwc_bwd evaluates it (the same expressions in the same order, so the two passes agree on every
// element). v takes the place of x; x travels through the dy slot of FirArgs and costs one more vector of loads per tap column, issued with v's before the
// first gate is evaluated. a is piecewise linear: d_x and d_bias are zero. With no gate x is never read and the launch is the plain FIR bit for bit.
//
// sg_fir_bias_act_nhwc_gate: the second-order pass of the TAIL (path-length regularisation through the generator). The tail's backward is
// dx = FIR^T(m * dy) with m the slope / gain / clamp gate evaluated from the kept y: linear in dy, piecewise constant in x. A cotangent (v_x, v_noise,
// v_bias) on (dx, dnoise, dbias) gives d_dy = m * (FIR(v_x) + v_noise + v_bias): the forward's strip walk on v_x, the fp32 v_noise / v_bias on the
// accumulator, and at the store the gate read from y -- sg_bias_act's gradient evaluator (style.hip bias_act_eval, MODE 1) restated for linear / lrelu, the
// same expressions in the same order, so the first-order backward (which runs that evaluator on (dy, y)) and this pass decide every element alike. y travels
// through the dy slot of FirArgs; its vector is requested before the row's taps are summed. With act linear, gain 1 and no clamp y is never read and the
// launch is the plain one bit for bit. A separate instantiation (EPI_STORE_GATE): the forward's registers do not change.
#include "common.h"
#include "../../include/sgamd.h"

static long long g_fir_launches = 0, g_act_fir_launches = 0;
extern "C" long long sg_fir_bias_act_launches() { return __atomic_load_n(&g_fir_launches, __ATOMIC_RELAXED); }
extern "C" long long sg_act_fir_launches() { return __atomic_load_n(&g_act_fir_launches, __ATOMIC_RELAXED); }

enum FirMode { FIR_TAIL, FIR_HEAD, FIR_HEAD_BWD, FIR_HEAD_GATE, FIR_TAIL_GATE };      // the five entry points
// the side of the forward kernel's epilogue; LOAD_GATE: the second-order pass of the head, STORE_GATE: the second-order pass of the tail (below)
enum { EPI_STORE, EPI_LOAD, EPI_LOAD_GATE, EPI_STORE_GATE };

struct FirArgs {
  const void* x; const float* f; void* y; const float* noise; const float* bias; const void* dy;
  long long noise_stride;
  int N, Hi, Wi, C, Ho, Wo, fh, fw, padx0, pady0, flip, act, gate, TY, strips;
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

// One step of a tap chain, s + f * x. sg_upfirdn2d's `s += f * x` compiles to an FMA chain on the device; whether the compiler contracts the same expression
// here depends on what surrounds it (a scalar instantiation kept a multiply and an add next to the border selects, one ulp off), so the device build asks for
// the FMA by name. A host build of these sources (tests/hipemu, no contraction anywhere) keeps the plain expression, which is again what sg_upfirdn2d does there.
__device__ __forceinline__ float fir_mad(float f, float x, float s) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fmaf(f, x, s);
#else
  return s + f * x;
#endif
}

// clamp( gain * act( v ) ) of a value that already carries its bias (and noise). A: how the caller hands the arguments over, `const FirArgs&` at the load
// side and `FirArgs` (a copy) at the store side. The arithmetic is the same; what follows the choice is whether the compiler keeps the tap chain of the fp32
// and bf16 vector instantiations in v_pk_fma_f32: by reference the store side loses 8 of its 32 (16 of 64 in bf16) and the fp32 tail measured 1.2 - 1.7 %
// slower than the kernel it replaced, by value the load side loses all of them (profiles/style_fir_refactor.txt).
template <typename A>
__device__ __forceinline__ float fir_act(float v, A a) {
  if (a.act == 3) v = v > 0.f ? v : v * a.alpha;
  v *= a.gain;
  if (a.clamp >= 0.f) v = (v > -a.clamp && v < a.clamp) ? v : (v >= 0.f ? a.clamp : -a.clamp);
  return v;
}

// g * da/dx at pre-activation v (bias included): the side of the leaky ReLU, the gain, and zero where the forward clamped. One statement for the first-order
// backward (g = the adjoint FIR of dy) and the second-order gate (g = the cotangent on dx), so that both passes take the same decision on every element.
__device__ __forceinline__ float fir_gate(float g, float v, const FirArgs& a) {
  const bool pos = a.act != 3 || v > 0.f;
  const float yv = (pos ? v : v * a.alpha) * a.gain;
  g = pos ? g : g * a.alpha;
  g *= a.gain;
  if (a.clamp >= 0.f && !(yv > -a.clamp && yv < a.clamp)) g = 0.f;
  return g;
}

// g * dy/dpre from the kept OUTPUT y of the tail: sg_bias_act's gradient rule (style.hip bias_act_eval<ACT, 1>: the side through y / gain, the gain, zero where
// the forward output sits at or beyond the clamp)
__device__ __forceinline__ float fir_gate_out(float g, float y, const FirArgs& a) {
  const float yy = a.gain != 0.f ? y / a.gain : 0.f;
  float r = a.act == 3 ? (yy > 0.f ? g : g * a.alpha) : g;
  r *= a.gain;
  if (a.clamp >= 0.f) r = (y > -a.clamp && y < a.clamp) ? r : 0.f;
  return r;
}

// strip height of the row-walking kernel: as tall as leaves the chip ~half a million threads (the rows a strip re-reads from its neighbour are (fh - 1) / TY
// of the input); -> workgroups of 256 threads for per_row threads per strip
static unsigned fir_strip_grid(long long per_row, int Ho, int& TY, int& strips) {
  TY = 32;
  while (TY > 4 && per_row * ((Ho + TY - 1) / TY) < (1ll << 19)) TY >>= 1;
  strips = (Ho + TY - 1) / TY;
  long long blocks = (per_row * strips + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  return (unsigned)blocks;
}

// SIDE = EPI_STORE: noise, bias, act, gain, clamp on the accumulator as it is stored (a.gate unused: every piece has its own test). SIDE = EPI_LOAD: bias, act,
// gain, clamp on each loaded value when a.gate (a.noise unused). SIDE = EPI_LOAD_GATE: each loaded value of a.x times da/dx at the same element of a.dy (the
// forward's raw input) when a.gate.
template <typename T, int V, int DOWN, int SIDE>
__global__ __launch_bounds__(256) void k_fir_nhwc(FirArgs a) {
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
    const float* nz = (SIDE == EPI_STORE || SIDE == EPI_STORE_GATE) && a.noise ? a.noise + (long long)n * a.noise_stride : nullptr;
    float bv[V];
#pragma unroll
    for (int e = 0; e < V; e++) bv[e] = a.bias ? a.bias[c0 + e] : 0.f;
    float acc[NACC][V];   // acc[j]: output row p - (NACC - 1) + j, which takes tap row s + DOWN * (NACC - 1 - j) of the padded input row p * DOWN + s
#pragma unroll
    for (int j = 0; j < NACC; j++)
#pragma unroll
      for (int e = 0; e < V; e++) acc[j][e] = 0.f;
    const int ix0 = ox * DOWN - px;
    // (loading a row ahead of the one being summed was measured and lost: +16 / +32 VGPRs, 3187 against 4327 GB/s in fp32 at 128 x 256^2, no change in bf16)
    for (int p = oy0; p <= oy1 + NACC - 2; p++) {
      float yk[V];      // EPI_STORE_GATE: the kept output at the element this iteration stores, in flight while the row's taps are summed
      if constexpr (SIDE == EPI_STORE_GATE) {
        const int oyk = p - (NACC - 1);
        if (a.gate && oyk >= oy0) load_f<T, V>((const T*)a.dy + (long long)n * a.Ho * a.Wo * a.C + c0 + ((long long)oyk * a.Wo + ox) * a.C, yk);
        else {
#pragma unroll
          for (int e = 0; e < V; e++) yk[e] = 0.f;
        }
      }
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
        if constexpr (SIDE == EPI_LOAD_GATE) {
          if (a.gate && rowin) {
            const T* rn = (const T*)a.dy + (long long)n * a.Hi * a.Wi * a.C + c0;
            float rv[4][V];
#pragma unroll
            for (int fx = 0; fx < 4; fx++) {      // (the raw row's loads join the cotangent's in flight; a tap outside the image keeps its zero)
              const int ix = ix0 + fx;
              if (fx >= dx && ix >= 0 && ix < a.Wi) load_f<T, V>(rn + ((long long)iy * a.Wi + ix) * a.C, rv[fx]);
              else {
#pragma unroll
                for (int e = 0; e < V; e++) rv[fx][e] = 1.f;
              }
            }
#pragma unroll
            for (int fx = 0; fx < 4; fx++) {
              const int ix = ix0 + fx;
              if (fx >= dx && ix >= 0 && ix < a.Wi) {
#pragma unroll
                for (int e = 0; e < V; e++) xv[fx][e] = fir_gate(xv[fx][e], rv[fx][e] + bv[e], a);
              }
            }
          }
        }
        if constexpr (SIDE == EPI_LOAD) {
          if (a.gate && rowin) {      // (after all four loads are issued, so that they are in flight together; only pixels inside the image are activated)
#pragma unroll
            for (int fx = 0; fx < 4; fx++) {
              const int ix = ix0 + fx;
              if (fx >= dx && ix >= 0 && ix < a.Wi) {
#pragma unroll
                for (int e = 0; e < V; e++) xv[fx][e] = fir_act<const FirArgs&>(xv[fx][e] + bv[e], a);
              }
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
        if constexpr (SIDE == EPI_STORE) {
          const float nv = nz ? nz[(long long)oy * a.Wo + ox] : 0.f;
#pragma unroll
          for (int e = 0; e < V; e++) {
            float v = o[e];
            if (nz) v += nv;
            if (a.bias) v += bv[e];
            o[e] = fir_act<FirArgs>(v, a);
          }
        }
        if constexpr (SIDE == EPI_STORE_GATE) {
          const float nv = nz ? nz[(long long)oy * a.Wo + ox] : 0.f;
#pragma unroll
          for (int e = 0; e < V; e++) {
            float v = o[e];
            if (nz) v += nv;
            if (a.bias) v += bv[e];
            o[e] = a.gate ? fir_gate_out(v, yk[e], a) : v;
          }
        }
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
__global__ __launch_bounds__(256) void k_act_fir_nhwc_bwd(FirArgs a) {
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
      for (int e = 0; e < V; e++) acc[e] = fir_gate(acc[e], xv[e] + (a.bias ? a.bias[c0 + e] : 0.f), a);
    }
    *(vec_t<T, V>*)((T*)a.y + off) = pack_f<T, V>(acc);
  }
}

template <typename T, int V, int DOWN> static void fir_launch_v(const FirArgs& a, FirMode mode, unsigned blocks, hipStream_t st) {
  if (mode == FIR_HEAD_BWD) hipLaunchKernelGGL((k_act_fir_nhwc_bwd<T, V, DOWN>), dim3(blocks), dim3(256), 0, st, a);
  else if (mode == FIR_HEAD_GATE) hipLaunchKernelGGL((k_fir_nhwc<T, V, DOWN, EPI_LOAD_GATE>), dim3(blocks), dim3(256), 0, st, a);
  else if (mode == FIR_HEAD) hipLaunchKernelGGL((k_fir_nhwc<T, V, DOWN, EPI_LOAD>), dim3(blocks), dim3(256), 0, st, a);
  else if constexpr (DOWN == 1) {      // (the tail has no down = 2)
    if (mode == FIR_TAIL_GATE) hipLaunchKernelGGL((k_fir_nhwc<T, V, 1, EPI_STORE_GATE>), dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_fir_nhwc<T, V, 1, EPI_STORE>), dim3(blocks), dim3(256), 0, st, a);
  }
}

// 16-byte vectors along C where the channels fill them and every tensor is aligned, one channel per thread otherwise; strips for the forward kernels
template <typename T, int DOWN> static void fir_launch(FirArgs& a, FirMode mode, hipStream_t st) {
  constexpr int VEC = ET<T>::VEC;
  const bool vec = a.C % VEC == 0 && ((((uintptr_t)a.x) | ((uintptr_t)a.y) | ((uintptr_t)a.dy)) & 15) == 0;
  const int cvn = vec ? a.C / VEC : a.C;
  unsigned blocks;
  if (mode == FIR_HEAD_BWD) {
    const long long b = ((long long)a.N * a.Hi * a.Wi * cvn + 255) / 256;
    blocks = (unsigned)(b > 256 * 32 ? 256 * 32 : b);
  } else {
    blocks = fir_strip_grid((long long)a.N * a.Wo * cvn, a.Ho, a.TY, a.strips);
  }
  if (vec) fir_launch_v<T, VEC, DOWN>(a, mode, blocks, st);
  else fir_launch_v<T, 1, DOWN>(a, mode, blocks, st);
}

// validation, argument set-up and launch of all four entry points (the tail: down = 1, dy = NULL; the head: noise = NULL; out = y, or dx of the backward; the
// gate: x = the cotangent, dy = the forward's raw input)
static int fir_run(const char* who, FirMode mode, int dtype, const void* x, const void* dy, const float* f, void* out, const float* noise, long long noise_stride,
                   const float* bias, int N, int Hi, int Wi, int C, int fh, int fw, int down, int padx0, int padx1, int pady0, int pady1, int flip_filter,
                   float filter_gain, int act, float alpha, float gain, float clamp, hipStream_t st) {
  char msg[160];
#define FIR_CHECK(cond, text) do { if (!(cond)) { snprintf(msg, sizeof msg, "%s: %s", who, text); sg_set_error(msg); return -1; } } while (0)
  FIR_CHECK(f && out && N > 0 && Hi > 0 && Wi > 0 && C > 0, "bad tensor arguments");
  FIR_CHECK(dtype == SG_DTYPE_F32 || dtype == SG_DTYPE_BF16, "fp32 / bf16 only");
  FIR_CHECK(down == 1 || down == 2, "down must be 1 or 2");
  FIR_CHECK(fh >= 1 && fh <= 4 && fw >= 1 && fw <= 4, "filters of 1..4 taps per axis only (sg_upfirdn2d takes the others)");
  FIR_CHECK(act == 1 || act == 3, "activation linear (1) or lrelu (3) only (sg_bias_act takes the others)");
  FIR_CHECK(Hi < (1 << 24) && Wi < (1 << 24) && abs(padx0) < (1 << 24) && abs(pady0) < (1 << 24) && abs(padx1) < (1 << 24) && abs(pady1) < (1 << 24),
            "image extent or padding too large");
  const long long Hp = (long long)Hi + pady0 + pady1 - fh, Wp = (long long)Wi + padx0 + padx1 - fw;
  FIR_CHECK(Hp >= 0 && Wp >= 0, "empty output (padded image smaller than the filter)");
  const long long Ho = Hp / down + 1, Wo = Wp / down + 1;
  FIR_CHECK(Ho < (1 << 24) && Wo < (1 << 24), "image extent or padding too large");
  FIR_CHECK(!noise || noise_stride == 0 || noise_stride >= Ho * Wo, "noise_stride must be 0 (one shared plane) or >= Ho * Wo");
  // (the tail's gate is read from y, which carries the bias already: v_bias is a cotangent there and opens no gate)
  const bool gate = (bias && mode != FIR_TAIL_GATE) || act != 1 || gain != 1.f || clamp >= 0.f;
  FIR_CHECK(mode == FIR_HEAD_BWD ? (dy && (x || !gate)) : (mode == FIR_HEAD_GATE || mode == FIR_TAIL_GATE) ? (x && (dy || !gate)) : x != nullptr,
            "bad tensor arguments");
#undef FIR_CHECK
  FirArgs a;
  a.x = x; a.f = f; a.y = out; a.noise = noise; a.bias = bias; a.dy = dy; a.noise_stride = noise ? noise_stride : 0;
  a.N = N; a.Hi = Hi; a.Wi = Wi; a.C = C; a.Ho = (int)Ho; a.Wo = (int)Wo; a.fh = fh; a.fw = fw;
  a.act = act; a.gate = gate ? 1 : 0; a.TY = 0; a.strips = 0; a.fgain = filter_gain; a.alpha = alpha; a.gain = gain; a.clamp = clamp;
  if (mode == FIR_HEAD_BWD) {      // the adjoint of upfirdn (upfirdn2d.py: up <-> down, the filter reversed); with up = down its far padding never enters the kernel
    a.padx0 = fw - padx0 - 1; a.pady0 = fh - pady0 - 1; a.flip = flip_filter ? 0 : 1;
  } else {
    a.padx0 = padx0; a.pady0 = pady0; a.flip = flip_filter ? 1 : 0;
  }
  if (dtype == SG_DTYPE_F32) { if (down == 1) fir_launch<float, 1>(a, mode, st); else fir_launch<float, 2>(a, mode, st); }
  else { if (down == 1) fir_launch<bf16_t, 1>(a, mode, st); else fir_launch<bf16_t, 2>(a, mode, st); }
  SG_LAUNCH_CHECK();
  __atomic_fetch_add((mode == FIR_TAIL || mode == FIR_TAIL_GATE) ? &g_fir_launches : &g_act_fir_launches, 1, __ATOMIC_RELAXED);
  return 0;
}

extern "C" int sg_fir_bias_act_nhwc(int dtype, const void* x, const float* f, void* y, const float* noise, long long noise_stride, const float* bias,
                                    int N, int Hi, int Wi, int C, int fh, int fw, int padx0, int padx1, int pady0, int pady1, int flip_filter,
                                    float filter_gain, int act, float alpha, float gain, float clamp, sg_stream_t s) {
  return fir_run("sg_fir_bias_act_nhwc", FIR_TAIL, dtype, x, nullptr, f, y, noise, noise_stride, bias, N, Hi, Wi, C, fh, fw, 1, padx0, padx1, pady0, pady1,
                 flip_filter, filter_gain, act, alpha, gain, clamp, (hipStream_t)s);
}

extern "C" int sg_act_fir_nhwc(int dtype, const void* x, const float* f, void* y, const float* bias, int N, int Hi, int Wi, int C, int fh, int fw, int down,
                               int padx0, int padx1, int pady0, int pady1, int flip_filter, float filter_gain, int act, float alpha, float gain, float clamp,
                               sg_stream_t s) {
  return fir_run("sg_act_fir_nhwc", FIR_HEAD, dtype, x, nullptr, f, y, nullptr, 0, bias, N, Hi, Wi, C, fh, fw, down, padx0, padx1, pady0, pady1, flip_filter,
                 filter_gain, act, alpha, gain, clamp, (hipStream_t)s);
}

extern "C" int sg_act_fir_nhwc_bwd(int dtype, const void* x, const void* dy, const float* f, void* dx, const float* bias, int N, int Hi, int Wi, int C, int fh,
                                   int fw, int down, int padx0, int padx1, int pady0, int pady1, int flip_filter, float filter_gain, int act, float alpha,
                                   float gain, float clamp, sg_stream_t s) {
  return fir_run("sg_act_fir_nhwc_bwd", FIR_HEAD_BWD, dtype, x, dy, f, dx, nullptr, 0, bias, N, Hi, Wi, C, fh, fw, down, padx0, padx1, pady0, pady1, flip_filter,
                 filter_gain, act, alpha, gain, clamp, (hipStream_t)s);
}

extern "C" int sg_act_fir_nhwc_gate(int dtype, const void* v, const void* x, const float* f, void* y, const float* bias, int N, int Hi, int Wi, int C, int fh,
                                    int fw, int down, int padx0, int padx1, int pady0, int pady1, int flip_filter, float filter_gain, int act, float alpha,
                                    float gain, float clamp, sg_stream_t s) {
  return fir_run("sg_act_fir_nhwc_gate", FIR_HEAD_GATE, dtype, v, x, f, y, nullptr, 0, bias, N, Hi, Wi, C, fh, fw, down, padx0, padx1, pady0, pady1, flip_filter,
                 filter_gain, act, alpha, gain, clamp, (hipStream_t)s);
}

extern "C" int sg_fir_bias_act_nhwc_gate(int dtype, const void* v, const void* y, const float* f, void* out, const float* v_noise, long long noise_stride,
                                         const float* v_bias, int N, int Hi, int Wi, int C, int fh, int fw, int padx0, int padx1, int pady0, int pady1,
                                         int flip_filter, float filter_gain, int act, float alpha, float gain, float clamp, sg_stream_t s) {
  return fir_run("sg_fir_bias_act_nhwc_gate", FIR_TAIL_GATE, dtype, v, y, f, out, v_noise, noise_stride, v_bias, N, Hi, Wi, C, fh, fw, 1, padx0, padx1, pady0,
                 pady1, flip_filter, filter_gain, act, alpha, gain, clamp, (hipStream_t)s);
}
