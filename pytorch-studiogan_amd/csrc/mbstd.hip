// mbstd.hip -- the minibatch standard deviation layer of the StyleGAN2 discriminator epilogue (Karras et al. 2018, section 3), forward and backward, one
// launch each.
//
// The batch is cut into M = N / G groups of G samples (sample n = g * M + m sits in group m) and the C channels into F slices of c = C / F:
//
//   s[m][f]        = mean_{j,h,w} sqrt( var_g( x[g M + m][h][w][f c + j] ) + 1e-8 )        biased variance over the G samples, two-pass
//   out[n][h][w][:C] = x[n][h][w][:],   out[n][h][w][C + f] = s[n mod M][f]
//
// As torch operators that is a reshape, mean, subtract, square, mean, add, sqrt, mean, reshape, repeat and cat: about ten launches over a small tensor, and more
// on the way back. Here the (m, f) pairs are the unit of work, each cut into S chunks of its c H W elements so that a large group (G = 32 of a batch of 64
// leaves M F = 2 pairs) still fills more than two compute units. A workgroup copies its chunk of its G samples into out and reduces sqrt(var + eps) over it.
// S = 1: it owns the pair and writes the statistic's plane. S > 1: it stores its partial sum, and the workgroup that takes the LAST ticket of the pair (one
// integer atomic on a zeroed counter, a device-scope fence on either side; nobody waits for anybody) adds the S partials IN CHUNK ORDER and writes the plane:
// the result does not depend on the order of arrival, and no float is ever added atomically. The backward needs no hand-over at all:
//
//   dS[m][f] = sum_{g,h,w} dout[g M + m][h][w][C + f]
//   dx       = dout[..., :C] + dS (x - mean_g) / (G c H W sqrt(var + 1e-8))
//
// dS is a sum over G H W values (a few hundred), so every chunk's workgroup adds it up itself, in the same fixed order; mean and variance are recomputed
// from x (G reads that hit the cache against a kept tensor of x's size). Sums: every thread adds its elements in ascending order, then one tree over the 256
// partials in LDS. Consecutive threads run along j, then the pixel: reads are contiguous within a slice. x is fp32 with a pixel pitch ldx >= C; out, dout and
// dx are dense.
//
// sg_mbstd_bwd2, the backward of that backward (R1: the one operator on the discriminator's path with a second derivative). With a cotangent v on dx,
// c_g = x_g - mean_g x, sigma = sqrt(var + 1e-8), P = c H W, and per element  dot = sum_g v_g c_g:
//
//   d_dout[..., :C]   = v
//   d_dout[n][..][C + f] = T[m][f] = sum_{j,h,w} dot / (G sigma P)                               one scalar per pair, broadcast like the statistic
//   d_x_k             = dS / (G P) * ( (v_k - mean_g v) / sigma - c_k dot / (G sigma^3) )          (the bracket's difference is taken in double: k_mbstd_bwd2)
//
// T is a sum over the whole pair, like the forward's statistic, and is handed over the same way: every chunk stores its partial sum and the one that takes
// the pair's last ticket adds them in chunk order. (Having every chunk re-add the whole pair, as the backward does for dS, would read x and v S times: dS is a
// sum over G H W stored values, T over c H W elements of 2 G reads each.) dS is re-added per chunk as in the backward.
#include "common.h"
#include "../../include/sgamd.h"

static long long g_mbstd_launches = 0;
extern "C" long long sg_mbstd_launches() { return __atomic_load_n(&g_mbstd_launches, __ATOMIC_RELAXED); }

struct MbstdArgs {
  const float* x; const float* dout; float* out; float* part; unsigned* tickets; const float* v; float* ddout;
  int N, HW, C, ldx, G, M, F, c, S;
  long long chunk;
};

// device-scope ordering around the ticket (a host build of this file runs its atomics sequentially consistent and needs nothing more)
__device__ __forceinline__ void mbstd_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
  __threadfence();
#endif
}
__device__ __forceinline__ float mbstd_load_shared(const float* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

__device__ __forceinline__ float mbstd_block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// mean and biased variance over the G samples of element (pixel p, channel ch) of group m
__device__ __forceinline__ void mbstd_moments(const MbstdArgs& a, int m, long long p, int ch, float& mean, float& var) {
  mean = 0.f;
  for (int g = 0; g < a.G; g++) mean += a.x[((long long)(g * a.M + m) * a.HW + p) * a.ldx + ch];
  mean /= (float)a.G;
  var = 0.f;
  for (int g = 0; g < a.G; g++) {
    const float d = a.x[((long long)(g * a.M + m) * a.HW + p) * a.ldx + ch] - mean;
    var += d * d;
  }
  var /= (float)a.G;
}

__global__ __launch_bounds__(256) void k_mbstd_fwd(MbstdArgs a) {
  __shared__ float red[256];
  __shared__ float stat;
  __shared__ int last;
  const int mf = blockIdx.x / a.S, sp = blockIdx.x - mf * a.S;
  const int m = mf / a.F, f = mf - m * a.F;
  const int CF = a.C + a.F;
  const long long per = (long long)a.c * a.HW;
  const long long e0 = sp * a.chunk, e1 = e0 + a.chunk < per ? e0 + a.chunk : per;
  float part = 0.f;
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
    const int j = (int)(e % a.c);
    const long long p = e / a.c;
    const int ch = f * a.c + j;
    for (int g = 0; g < a.G; g++) {
      const long long pix = (long long)(g * a.M + m) * a.HW + p;
      a.out[pix * CF + ch] = a.x[pix * a.ldx + ch];
    }
    float mean, var;
    mbstd_moments(a, m, p, ch, mean, var);
    part += sqrtf(var + 1e-8f);
  }
  float total = mbstd_block_sum(part, red);
  if (a.S > 1) {
    if (threadIdx.x == 0) {
      a.part[(long long)mf * a.S + sp] = total;
      mbstd_fence();
      last = atomicAdd(&a.tickets[mf], 1u) == (unsigned)(a.S - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0) {
      mbstd_fence();
      float t = 0.f;
      for (int i = 0; i < a.S; i++) t += mbstd_load_shared(&a.part[(long long)mf * a.S + i]);      // chunk order, whoever arrived when
      stat = t;
    }
    __syncthreads();
    total = stat;
  }
  const float s = total / (float)per;
  const long long planes = (long long)a.G * a.HW;
  for (long long e = threadIdx.x; e < planes; e += 256) {
    const int g = (int)(e / a.HW);
    const long long p = e - (long long)g * a.HW;
    a.out[((long long)(g * a.M + m) * a.HW + p) * CF + a.C + f] = s;
  }
}

// a.out = dx [N][HW][C] dense
__global__ __launch_bounds__(256) void k_mbstd_bwd(MbstdArgs a) {
  __shared__ float red[256];
  const int mf = blockIdx.x / a.S, sp = blockIdx.x - mf * a.S;
  const int m = mf / a.F, f = mf - m * a.F;
  const int CF = a.C + a.F;
  const long long per = (long long)a.c * a.HW, planes = (long long)a.G * a.HW;
  const long long e0 = sp * a.chunk, e1 = e0 + a.chunk < per ? e0 + a.chunk : per;
  float part = 0.f;
  for (long long e = threadIdx.x; e < planes; e += 256) {
    const int g = (int)(e / a.HW);
    const long long p = e - (long long)g * a.HW;
    part += a.dout[((long long)(g * a.M + m) * a.HW + p) * CF + a.C + f];
  }
  const float dS = mbstd_block_sum(part, red);
  const float k = dS / ((float)a.G * (float)per);
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
    const int j = (int)(e % a.c);
    const long long p = e / a.c;
    const int ch = f * a.c + j;
    float mean, var;
    mbstd_moments(a, m, p, ch, mean, var);
    const float w = k / sqrtf(var + 1e-8f);
    for (int g = 0; g < a.G; g++) {
      const long long pix = (long long)(g * a.M + m) * a.HW + p;
      a.out[pix * a.C + ch] = a.dout[pix * CF + ch] + w * (a.x[pix * a.ldx + ch] - mean);
    }
  }
}

// (1 / G) sum_g c_g (u_k c_g - c_k u_g) + 1e-8 u_k of sample k at element (p, ch), u = v - vbar, c = x - mean, from A = sum c^2 and B = sum c u: the difference
// u_k A - c_k B is taken in double (the products of two floats are exact there), so what cancels in it cancels without loss
__device__ __forceinline__ float mbstd_bracket(const MbstdArgs& a, int m, long long p, int ch, int k, float mean, float vbar, double A, double B) {
  const long long pk = (long long)(k * a.M + m) * a.HW + p;
  const float uk = a.v[pk * a.C + ch] - vbar, ck = a.x[pk * a.ldx + ch] - mean;
  return (float)(((double)uk * A - (double)ck * B) / (double)a.G) + 1e-8f * uk;
}

// a.out = d_x [N][HW][C] dense, a.v [N][HW][C] dense, a.ddout [N][HW][C + F] dense
__global__ __launch_bounds__(256) void k_mbstd_bwd2(MbstdArgs a) {
  __shared__ float red[256];
  __shared__ float stat;
  __shared__ int last;
  const int mf = blockIdx.x / a.S, sp = blockIdx.x - mf * a.S;
  const int m = mf / a.F, f = mf - m * a.F;
  const int CF = a.C + a.F;
  const long long per = (long long)a.c * a.HW, planes = (long long)a.G * a.HW;
  const long long e0 = sp * a.chunk, e1 = e0 + a.chunk < per ? e0 + a.chunk : per;
  float part = 0.f;
  for (long long e = threadIdx.x; e < planes; e += 256) {
    const int g = (int)(e / a.HW);
    const long long p = e - (long long)g * a.HW;
    part += a.dout[((long long)(g * a.M + m) * a.HW + p) * CF + a.C + f];
  }
  const float dS = mbstd_block_sum(part, red);
  const float k = dS / ((float)a.G * (float)per);
  part = 0.f;
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
    const int j = (int)(e % a.c);
    const long long p = e / a.c;
    const int ch = f * a.c + j;
    float mean, var;
    mbstd_moments(a, m, p, ch, mean, var);
    const float sigma = sqrtf(var + 1e-8f);
    float vbar = 0.f, dot = 0.f;
    for (int g = 0; g < a.G; g++) {
      const long long pix = (long long)(g * a.M + m) * a.HW + p;
      const float vg = a.v[pix * a.C + ch];
      vbar += vg;
      dot += vg * (a.x[pix * a.ldx + ch] - mean);
    }
    vbar /= (float)a.G;
    part += dot / sigma;
    // (u_k / sigma - c_k dot / (G sigma^3)) sigma^3 = (1 / G) sum_g c_g (u_k c_g - c_k u_g) + 1e-8 u_k,  u = v - mean_g v. Written as the difference of two
    // fp32 quotients it cancels to nothing where the group's deviation is one-dimensional (G = 2: sigma = |c|, whose second derivative is the 1e-8 term
    // alone); mbstd_bracket takes the difference in double, O(G) per sample.
    // The brackets sum to zero over the group (sum u = sum c = 0), and the gradient of a bias in front of the layer is such a sum: the mean over k is taken off
    // explicitly, as the backward of `x - mean_g x` does in a composition of operators, so that the rounding of mean and vbar does not survive in it.
    double A = 0., B = 0.;
    for (int g = 0; g < a.G; g++) {
      const long long pix = (long long)(g * a.M + m) * a.HW + p;
      const float cg = a.x[pix * a.ldx + ch] - mean, ug = a.v[pix * a.C + ch] - vbar;
      A += (double)cg * (double)cg;
      B += (double)cg * (double)ug;
    }
    const float k3 = k / (sigma * sigma * sigma);
    float tbar = 0.f;
    for (int kk = 0; kk < a.G; kk++) tbar += mbstd_bracket(a, m, p, ch, kk, mean, vbar, A, B);
    tbar /= (float)a.G;
    for (int kk = 0; kk < a.G; kk++) {
      const long long pix = (long long)(kk * a.M + m) * a.HW + p;
      a.out[pix * a.C + ch] = k3 * (mbstd_bracket(a, m, p, ch, kk, mean, vbar, A, B) - tbar);
      a.ddout[pix * CF + ch] = a.v[pix * a.C + ch];
    }
  }
  float total = mbstd_block_sum(part, red);
  if (a.S > 1) {
    if (threadIdx.x == 0) {
      a.part[(long long)mf * a.S + sp] = total;
      mbstd_fence();
      last = atomicAdd(&a.tickets[mf], 1u) == (unsigned)(a.S - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0) {
      mbstd_fence();
      float t = 0.f;
      for (int i = 0; i < a.S; i++) t += mbstd_load_shared(&a.part[(long long)mf * a.S + i]);      // chunk order, whoever arrived when
      stat = t;
    }
    __syncthreads();
    total = stat;
  }
  const float T = total / ((float)a.G * (float)per);
  for (long long e = threadIdx.x; e < planes; e += 256) {
    const int g = (int)(e / a.HW);
    const long long p = e - (long long)g * a.HW;
    a.ddout[((long long)(g * a.M + m) * a.HW + p) * CF + a.C + f] = T;
  }
}

// chunks per (m, f) pair: at least ~1024 elements each, at most 64, none when the pairs alone fill the chip
extern "C" int sg_mbstd_splits(int N, int H, int W, int C, int G, int F) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || G <= 0 || F <= 0 || N % G || C % F) return 1;
  const long long per = (long long)(C / F) * H * W, pairs = (long long)(N / G) * F;
  long long S = per / 1024;
  if (S > 64) S = 64;
  while (S > 1 && pairs * S > 1024) S >>= 1;
  return S < 1 ? 1 : (int)S;
}

static int mbstd_args(const char* who, MbstdArgs& a, const float* x, int ldx, int N, int H, int W, int C, int G, int F) {
  static const char* text[] = {"bad tensor arguments", "the group size must divide the batch (N % G != 0)", "num_channels must divide the channels (C % F != 0)",
                               "the pixel pitch is smaller than C", "the image is too large"};
  int bad = -1;
  if (!x || N <= 0 || H <= 0 || W <= 0 || C <= 0 || G <= 0 || F <= 0) bad = 0;
  else if (N % G) bad = 1;
  else if (C % F) bad = 2;
  else if (ldx < C) bad = 3;
  else if ((long long)H * W >= (1ll << 31) / G || (long long)(N / G) * F >= (1ll << 24)) bad = 4;
  if (bad >= 0) {
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, text[bad]);
    sg_set_error(msg);
    return -1;
  }
  a.x = x; a.N = N; a.HW = H * W; a.C = C; a.ldx = ldx; a.G = G; a.M = N / G; a.F = F; a.c = C / F;
  a.S = sg_mbstd_splits(N, H, W, C, G, F);
  const long long per = (long long)a.c * a.HW;
  a.chunk = (per + a.S - 1) / a.S;
  a.part = nullptr; a.tickets = nullptr; a.dout = nullptr; a.v = nullptr; a.ddout = nullptr;
  return 0;
}

extern "C" int sg_mbstd_fwd(const float* x, int ldx, float* out, float* part, unsigned* tickets, int N, int H, int W, int C, int G, int F, sg_stream_t s) {
  MbstdArgs a;
  if (mbstd_args("sg_mbstd_fwd", a, x, ldx, N, H, W, C, G, F)) return -1;
  SG_CHECK(out, "sg_mbstd_fwd: bad tensor arguments");
  SG_CHECK(a.S == 1 || (part && tickets), "sg_mbstd_fwd: sg_mbstd_splits() > 1 needs the partial sums [M F S] and the zeroed tickets [M F]");
  a.dout = nullptr; a.out = out; a.part = part; a.tickets = tickets;
  hipLaunchKernelGGL(k_mbstd_fwd, dim3((unsigned)(a.M * a.F * a.S)), dim3(256), 0, (hipStream_t)s, a);
  SG_LAUNCH_CHECK();
  __atomic_fetch_add(&g_mbstd_launches, 1, __ATOMIC_RELAXED);
  return 0;
}

extern "C" int sg_mbstd_bwd(const float* x, int ldx, const float* dout, float* dx, int N, int H, int W, int C, int G, int F, sg_stream_t s) {
  MbstdArgs a;
  if (mbstd_args("sg_mbstd_bwd", a, x, ldx, N, H, W, C, G, F)) return -1;
  SG_CHECK(dout && dx, "sg_mbstd_bwd: bad tensor arguments");
  a.dout = dout; a.out = dx;
  hipLaunchKernelGGL(k_mbstd_bwd, dim3((unsigned)(a.M * a.F * a.S)), dim3(256), 0, (hipStream_t)s, a);
  SG_LAUNCH_CHECK();
  __atomic_fetch_add(&g_mbstd_launches, 1, __ATOMIC_RELAXED);
  return 0;
}

extern "C" int sg_mbstd_bwd2(const float* x, int ldx, const float* dout, const float* v, float* d_dout, float* d_x, float* part, unsigned* tickets, int N, int H,
                             int W, int C, int G, int F, sg_stream_t s) {
  MbstdArgs a;
  if (mbstd_args("sg_mbstd_bwd2", a, x, ldx, N, H, W, C, G, F)) return -1;
  SG_CHECK(dout && v && d_dout && d_x, "sg_mbstd_bwd2: bad tensor arguments");
  SG_CHECK(a.S == 1 || (part && tickets), "sg_mbstd_bwd2: sg_mbstd_splits() > 1 needs the partial sums [M F S] and the zeroed tickets [M F]");
  a.dout = dout; a.v = v; a.ddout = d_dout; a.out = d_x; a.part = part; a.tickets = tickets;
  hipLaunchKernelGGL(k_mbstd_bwd2, dim3((unsigned)(a.M * a.F * a.S)), dim3(256), 0, (hipStream_t)s, a);
  SG_LAUNCH_CHECK();
  __atomic_fetch_add(&g_mbstd_launches, 1, __ATOMIC_RELAXED);
  return 0;
}
