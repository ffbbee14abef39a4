// norm.hip -- BatchNorm2d(eps=1e-4, momentum=0.1) and ConditionalBatchNorm2d forward/backward on NHWC tensors
// (reference src/utils/ops.py:14-28,227-228). Statistics are produced as fp64 partial sums {sum x, sum x^2}
// so that the cross-rank reduction of sync-BN is ONE small all-reduce between sg_bn_partial_stats and
// sg_bn_finalize (reference src/models/model.py:161-165 uses nn.SyncBatchNorm's all_gather instead).
// HBM-bound: every kernel streams 16-byte vectors along C.
#include "common.h"
#include "../../include/sgamd.h"

// which kernel an entry point launched (sgamd.h SG_BN_PATH_*): counted on the host next to the launch, read by tests that have to prove which one ran
static long long g_bn_path_launches[SG_BN_PATH_COUNT] = {};
static inline void bn_path_count(int path) { __atomic_fetch_add(&g_bn_path_launches[path], 1, __ATOMIC_RELAXED); }
extern "C" long long sg_bn_path_launches(int path) {
  if (path < 0 || path >= SG_BN_PATH_COUNT) return -1;
  return __atomic_load_n(&g_bn_path_launches[path], __ATOMIC_RELAXED);
}
static inline double elem_bytes(int dtype) { return dtype == SG_DTYPE_BF16 ? 2.0 : 4.0; }

// The arithmetic that the kernels of one entry point, and the forward and the backward of one layer, have to share BIT FOR BIT, written once with the fused
// multiply-adds spelled out and no contraction beyond them. Left to the compiler, a * b + c was fused in one instantiation and not in another (in the bf16
// k_bn_bwd_apply_stream even for six of a thread's eight channels and not for the other two), so that the streaming and the scalar kernel wrote different bytes and a
// ReLU input within an ulp of zero could pass the forward and be masked in the backward.
__device__ __forceinline__ float bn_xhat(float x, float mu, float is) {
#pragma clang fp contract(off)
  return (x - mu) * is;
}
// the ReLU's input, gain * xhat + bias, one rounding
__device__ __forceinline__ float bn_pre(float xh, float ga, float bi) { return __builtin_fmaf(xh, ga, bi); }
// dx = invstd (gain dy' - (k0 + xhat k1) / count) [+ res]
__device__ __forceinline__ float bn_dx(float g, float xh, float ga, float is, float k0, float k1, float invc, int use_batch) {
#pragma clang fp contract(off)
  float d = ga * g;
  if (use_batch) d = __builtin_fmaf(-__builtin_fmaf(xh, k1, k0), invc, d);
  return d * is;
}
__device__ __forceinline__ float bn_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
// The fused ReLU's gate: does the element pass. THE predicate of every backward's mask; the forward clamps with fmaxf(bn_pre, 0), which is 0 exactly where
// the gate is shut (a NaN pre-activation included)
__device__ __forceinline__ bool bn_gate(int relu, float xh, float ga, float bi) { return !(relu && !(bn_pre(xh, ga, bi) > 0.f)); }
// mean / invstd / gain / bias of the V channels from c0 on, for sample n: a null gain is 1, a null bias 0, rows of pitch gsn (0: one row for every sample);
// with k0 / k1, also the batch-statistics terms of bn_dx
template <int V> __device__ __forceinline__ void bn_coef(const float* mean, const float* invstd, const float* gain, const float* bias, int gsn, int n, int c0, float* mu, float* is, float* ga, float* bi,
                                                         const double* chan = nullptr, int use_batch = 0, float* k0 = nullptr, float* k1 = nullptr) {
#pragma unroll
  for (int e = 0; e < V; e++) {
    const int c = c0 + e;
    mu[e] = mean[c]; is[e] = invstd[c];
    ga[e] = gain ? gain[(long long)n * gsn + c] : 1.f;
    bi[e] = bias ? bias[(long long)n * gsn + c] : 0.f;
    if (k0) {
      k0[e] = use_batch ? (float)chan[2 * c] : 0.f;
      k1[e] = use_batch ? (float)chan[2 * c + 1] : 0.f;
    }
  }
}
// the per-element bodies, one per stage, on the V channels a thread holds. Forward: xv -> relu(gain xhat + bias)
template <int V> __device__ __forceinline__ void bn_apply_elems(float* xv, const float* mu, const float* is, const float* ga, const float* bi, int relu) {
#pragma unroll
  for (int e = 0; e < V; e++) {
    float v = bn_pre(bn_xhat(xv[e], mu[e], is[e]), ga[e], bi[e]);   // the same evaluation as the backward's recomputation
    if (relu) v = fmaxf(v, 0.f);
    xv[e] = v;
  }
}
// backward stage 1: s1 += dy', s2 += dy' xhat with dy' = dy behind the gate
template <int V> __device__ __forceinline__ void bn_bwd_sum_elems(const float* xv, const float* gv, const float* mu, const float* is, const float* ga, const float* bi, int relu, float* s1, float* s2) {
#pragma unroll
  for (int e = 0; e < V; e++) {
    const float xh = bn_xhat(xv[e], mu[e], is[e]);
    float g = gv[e];
    if (!bn_gate(relu, xh, ga[e], bi[e])) g = 0.f;
    s1[e] += g; s2[e] += g * xh;
  }
}
// backward stage 3: xv -> dx (bn_dx) [+ the V elements at res, the gradient the same input received through a residual block's skip path; null: none]
template <typename T, int V> __device__ __forceinline__ void bn_bwd_apply_elems(float* xv, const float* gv, const T* res, const float* mu, const float* is, const float* ga, const float* bi, const float* k0, const float* k1, float invc, int relu, int use_batch) {
#pragma unroll
  for (int e = 0; e < V; e++) {
    const float xh = bn_xhat(xv[e], mu[e], is[e]);
    float g = gv[e];
    if (!bn_gate(relu, xh, ga[e], bi[e])) g = 0.f;
    xv[e] = bn_dx(g, xh, ga[e], is[e], k0[e], k1[e], invc, use_batch);
  }
  if (res) {
    float rv[V];
    load_f<T, V>(res, rv);
#pragma unroll
    for (int e = 0; e < V; e++) xv[e] = bn_add(xv[e], rv[e]);
  }
}
// Column reduce of a (64 channels x 4 row phases) block: every thread stores its K accumulators into sm[K][4][64] (declared by the kernel), and after the
// barrier row phase 0 combines the four of a channel, left to right or PAIRWISE (a + b) + (c + d), whichever the kernel has always had.
template <int K, typename A> __device__ __forceinline__ void bn_col_store(A (&sm)[K][4][64], const A* s, int ry, int cx) {
#pragma unroll
  for (int k = 0; k < K; k++) sm[k][ry][cx] = s[k];
  __syncthreads();
}
template <bool PAIRWISE, typename A> __device__ __forceinline__ A bn_col_sum(const A (&p)[4][64], int cx) {
  return PAIRWISE ? (p[0][cx] + p[1][cx]) + (p[2][cx] + p[3][cx]) : p[0][cx] + p[1][cx] + p[2][cx] + p[3][cx];
}
__device__ __forceinline__ void bn_atomic_add(double* p, double v) { atomicAdd(p, v); }
__device__ __forceinline__ void bn_atomic_add(float* p, float v) { unsafeAtomicAdd(p, v); }

// Streaming ownership (grid (pixel chunks, N[, channel-vector tiles]); block = lanes_p pixel lanes x cvt channel vectors): thread -> its channel vector cv of
// sample n = blockIdx.y, its pixel lane pl, the pixels [p0, p1) of its block and the element offset `base` of (n, pixel 0, channel cv * V)
struct BnOwn { int cv, pl, lanes_p; long long p0, p1, base; };
__device__ __forceinline__ BnOwn bn_own(int cv0, int cvt, int lanes_p, int V, long long HW, int C, int ppb) {
  BnOwn w;
  w.lanes_p = lanes_p;
  w.cv = cv0 + threadIdx.x % cvt; w.pl = threadIdx.x / cvt;
  w.p0 = (long long)blockIdx.x * ppb;
  w.p1 = w.p0 + ppb; if (w.p1 > HW) w.p1 = HW;
  w.base = (long long)blockIdx.y * HW * C + w.cv * V;
  return w;
}
// The walk of a block's pixels by its lanes: UN pixels per trip, all UN x NIN 16-byte loads issued before the first use, then a one-pixel tail.
// load(k, pix, unrolled) -> input k's vector at pix; body(r, pix) consumes the NIN vectors of one pixel. With one 16-byte load in flight per lane the 32 resident
// waves of a CU hold 32 KB, which at ~2 us of HBM latency is 4.2 TB/s for the chip -- exactly what the r02 roofline_hbm leg measured for the batch-norm family
// (0.53 of peak). Same arithmetic per element and same pixel order as a one-pixel walk, so results are unchanged.
template <int UN, int NIN, typename Load, typename Body> __device__ __forceinline__ void bn_walk(const BnOwn& w, Load load, Body body) {
  long long pix = w.p0 + w.pl;
  for (; pix + (long long)(UN - 1) * w.lanes_p < w.p1; pix += (long long)UN * w.lanes_p) {
    u32x4 r[UN][NIN];
#pragma unroll
    for (int i = 0; i < UN; i++)
#pragma unroll
      for (int k = 0; k < NIN; k++) r[i][k] = load(k, pix + (long long)i * w.lanes_p, true);
#pragma unroll
    for (int i = 0; i < UN; i++) body(r[i], pix + (long long)i * w.lanes_p);
  }
  for (; pix < w.p1; pix += w.lanes_p) {
    u32x4 r[NIN];
#pragma unroll
    for (int k = 0; k < NIN; k++) r[k] = load(k, pix, false);
    body(r, pix);
  }
}
// The tail of a streaming reduce: the lanes' sums {s1, s2} of every channel meet in sm[lanes_p][C][2] (dynamic LDS), one atomic per channel, sum and block
template <int V, typename A> __device__ __forceinline__ void bn_lane_combine(A* sm, const A* s1, const A* s2, int pl, int cv, int lanes_p, int C, A* out) {
#pragma unroll
  for (int e = 0; e < V; e++) { sm[((long long)pl * C + cv * V + e) * 2] = s1[e]; sm[((long long)pl * C + cv * V + e) * 2 + 1] = s2[e]; }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
    A a = 0;
    for (int l = 0; l < lanes_p; l++) a += sm[(long long)l * C * 2 + i];
    bn_atomic_add(out + i, a);
  }
}

// ---- statistics ------------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(256) void k_bn_partial(const T* x, int ldx, long long rows, int C, double* partial, long long rpb) {
  __shared__ double sm[2][4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  long long r0 = blockIdx.y * rpb, r1 = r0 + rpb; if (r1 > rows) r1 = rows;
  double s[2] = {0.0, 0.0};
  if (c < C) {
    for (long long r = r0 + ry; r < r1; r += 4) {
      const double v = (double)to_f<T>(x[r * ldx + c]);
      s[0] += v; s[1] += v * v;
    }
  }
  bn_col_store(sm, s, ry, cx);
  if (ry == 0 && c < C) {
#pragma unroll
    for (int k = 0; k < 2; k++) bn_atomic_add(partial + 2 * c + k, bn_col_sum<false>(sm[k], cx));
  }
}
// Streaming variant: a thread owns one 16-byte channel vector and walks pixels (16-byte loads instead of 2-byte ones);
// fp32 partials are flushed into fp64 every 32 pixels, lanes of a block are combined through LDS, one fp64 atomic per
// channel and block.
template <typename T> __global__ __launch_bounds__(256) void k_bn_partial_stream(const T* x, int ldx, long long rows, int C, double* partial, long long rpb) {
  constexpr int V = ET<T>::VEC;
  extern __shared__ double smd[];                       // [lanes_p][C][2]
  const int CV = C / V;
  const int lanes_p = blockDim.x / CV;
  const int cv = threadIdx.x % CV, pl = threadIdx.x / CV;
  long long r0 = blockIdx.x * rpb, r1 = r0 + rpb; if (r1 > rows) r1 = rows;
  double d1[V], d2[V];
#pragma unroll
  for (int e = 0; e < V; e++) { d1[e] = 0.0; d2[e] = 0.0; }
  for (long long rb = r0 + pl; rb < r1; rb += 32ll * lanes_p) {
    float s1[V], s2[V];
#pragma unroll
    for (int e = 0; e < V; e++) { s1[e] = 0.f; s2[e] = 0.f; }
    for (int k = 0; k < 32; k += 4) {                        // four loads in flight per lane (see bn_walk); same summation order
      u32x4 raw[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const long long r = rb + (long long)(k + i) * lanes_p;
        raw[i] = r < r1 ? *(const u32x4*)(x + r * ldx + cv * V) : u32x4{0u, 0u, 0u, 0u};
      }
#pragma unroll
      for (int i = 0; i < 4; i++) {
        float xv[V];
        unpack16<T>(raw[i], xv);
#pragma unroll
        for (int e = 0; e < V; e++) { s1[e] += xv[e]; s2[e] += xv[e] * xv[e]; }
      }
      if (rb + (long long)(k + 4) * lanes_p >= r1) break;
    }
#pragma unroll
    for (int e = 0; e < V; e++) { d1[e] += (double)s1[e]; d2[e] += (double)s2[e]; }
  }
  bn_lane_combine<V>(smd, d1, d2, pl, cv, lanes_p, C, partial);
}
extern "C" int sg_bn_partial_stats(int dtype, const void* x, int ldx, long long rows, int C, double* partial, sg_stream_t s) {
  SgProfScope prof((hipStream_t)s, (double)rows * C * elem_bytes(dtype), 4);
  SG_CHECK(x && partial && rows > 0 && C > 0, "sg_bn_partial_stats: bad args");
  bool done = false;
  DISPATCH_T(dtype, {
    constexpr int V = ET<T>::VEC;
    const int CV = C / V;
    if (C % V == 0 && ldx % V == 0 && ((uintptr_t)x & 15) == 0 && CV <= 128 && rows >= 4096) {
      const int lanes_p = 256 / CV;
      long long rpb = (rows + 1023) / 1024; if (rpb < 32ll * lanes_p) rpb = 32ll * lanes_p;
      const int gx = (int)((rows + rpb - 1) / rpb);
      hipLaunchKernelGGL(k_bn_partial_stream<T>, dim3(gx), dim3(CV * lanes_p), (size_t)lanes_p * C * 2 * sizeof(double), (hipStream_t)s, (const T*)x, ldx, rows, C, partial, rpb);
      bn_path_count(SG_BN_PATH_PARTIAL_STREAM);
      done = true;
    }
  });
  if (done) { SG_LAUNCH_CHECK(); return 0; }
  int ct = (C + 63) / 64;
  long long want = 2048 / ct; if (want < 1) want = 1;
  long long rpb = (rows + want - 1) / want; if (rpb < 64) rpb = 64;
  int gy = (int)((rows + rpb - 1) / rpb);
  DISPATCH_T(dtype, hipLaunchKernelGGL(k_bn_partial<T>, dim3(ct, gy), dim3(256), 0, (hipStream_t)s, (const T*)x, ldx, rows, C, partial, rpb));
  bn_path_count(SG_BN_PATH_PARTIAL_GENERIC);
  SG_LAUNCH_CHECK();
  return 0;
}
// partial[2 c + {0, 1}] += sum over the tile rows of stats[row][c][{0, 1}] (the per-tile sums a convolution epilogue wrote: conv_v2.h
// sg_conv_epilogue `stats`). Block (64 channels x 4 row phases), fixed summation order per block, fp64; blocks of different row groups meet in
// fp64 atomics like k_bn_partial_stream's.
__global__ __launch_bounds__(256) void k_bn_stats_from_tiles(const float* stats, int nrows, int C, double* partial, int rpb) {
  __shared__ double sm[2][4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  int r0 = blockIdx.y * rpb, r1 = r0 + rpb;
  if (r1 > nrows) r1 = nrows;
  double s[2] = {0.0, 0.0};
  if (c < C) {
    for (int r = r0 + ry; r < r1; r += 4) {
      const float2 v = *(const float2*)(stats + ((long long)r * C + c) * 2);
      s[0] += (double)v.x; s[1] += (double)v.y;
    }
  }
  bn_col_store(sm, s, ry, cx);
  if (ry == 0 && c < C) {
#pragma unroll
    for (int k = 0; k < 2; k++) bn_atomic_add(partial + 2 * c + k, bn_col_sum<true>(sm[k], cx));
  }
}
extern "C" int sg_bn_stats_from_tiles(const float* stats, int nrows, int C, double* partial, sg_stream_t s) {
  SG_CHECK(stats && partial && nrows > 0 && C > 0, "sg_bn_stats_from_tiles: bad args");
  SgProfScope prof((hipStream_t)s, (double)nrows * C * 8.0, 4);
  int gy = (nrows + 255) / 256;
  if (gy > 64) gy = 64;
  const int rpb = (nrows + gy - 1) / gy;
  hipLaunchKernelGGL(k_bn_stats_from_tiles, dim3((C + 63) / 64, gy), dim3(256), 0, (hipStream_t)s, stats, nrows, C, partial, rpb);
  SG_LAUNCH_CHECK();
  return 0;
}
__global__ void k_bn_finalize(const double* partial, double count, int C, float eps, float momentum, float* mean, float* invstd, float* rm, float* rv) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double m = partial[2 * c] / count;
  double var = partial[2 * c + 1] / count - m * m;
  if (var < 0.0) var = 0.0;
  mean[c] = (float)m;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (rm) {
    const double unb = (count > 1.0) ? var * count / (count - 1.0) : var;
    rm[c] = (1.f - momentum) * rm[c] + momentum * (float)m;
    rv[c] = (1.f - momentum) * rv[c] + momentum * (float)unb;
  }
}
extern "C" int sg_bn_finalize(const double* partial, double count, int C, float eps, float momentum, float* mean, float* invstd, float* running_mean, float* running_var, sg_stream_t s) {
  SG_CHECK(partial && mean && invstd && count > 0, "sg_bn_finalize: bad args");
  SG_CHECK((running_mean == nullptr) == (running_var == nullptr), "sg_bn_finalize: running stats must come as a pair");
  hipLaunchKernelGGL(k_bn_finalize, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)s, partial, count, C, eps, momentum, mean, invstd, running_mean, running_var);
  SG_LAUNCH_CHECK();
  return 0;
}
__global__ void k_bn_from_running(const float* rm, const float* rv, int C, float eps, float* mean, float* invstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  mean[c] = rm[c];
  invstd[c] = 1.f / sqrtf(rv[c] + eps);
}
extern "C" int sg_bn_from_running(const float* running_mean, const float* running_var, int C, float eps, float* mean, float* invstd, sg_stream_t s) {
  SG_CHECK(running_mean && running_var && mean && invstd, "sg_bn_from_running: null");
  hipLaunchKernelGGL(k_bn_from_running, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)s, running_mean, running_var, C, eps, mean, invstd);
  SG_LAUNCH_CHECK();
  return 0;
}

// ---- apply -------------------------------------------------------------------------------------------------
// one thread = one 16-byte vector of channels; requires C % VEC == 0 (checked on the host; scalar kernel otherwise)
template <typename T, bool VECP> __global__ __launch_bounds__(256) void k_bn_apply(const T* x, T* y, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gsn, int relu) {
  constexpr int V = VECP ? ET<T>::VEC : 1;
  const int CV = C / V;
  const long long total = (long long)N * HW * CV;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int cv = (int)(i % CV); const long long pix = i / CV; const int n = (int)(pix / HW);
    const int c0 = cv * V;
    float xv[V], mu[V], is[V], ga[V], bi[V];
    load_f<T, V>(x + pix * C + c0, xv);
    bn_coef<V>(mean, invstd, gain, bias, gsn, n, c0, mu, is, ga, bi);
    bn_apply_elems<V>(xv, mu, is, ga, bi, relu);
    *(vec_t<T, V>*)(y + pix * C + c0) = pack_f<T, V>(xv);
  }
}
static inline int grid_for(long long total) { long long b = (total + 255) / 256; if (b > 256 * 32) b = 256 * 32; if (b < 1) b = 1; return (int)b; }
template <typename T> static bool vec_ok(const void* a, const void* b, int C) {
  return (C % ET<T>::VEC == 0) && ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0;
}
// a call takes its streaming kernel: 16-byte operands (`vec`), a sample's channel vectors within one block, the batch within grid.y, at least 16 pixels
// (HW 64 -> 16: the 4 x 4 maps of a generator's first block took the generic kernel at 0.56 TB/s, 45 us for 25 MB)
template <typename T> static bool bn_streams(bool vec, int N, long long HW, int C) { return vec && C / ET<T>::VEC <= 256 && N <= 65535 && HW >= 16; }
// streaming geometry: `want` workgroups over `slabs` (samples [x channel-vector tiles]) -> pixels per block, at least `floor_pix` per lane; returns grid.x
static inline int bn_stream_geom(long long HW, long long slabs, int lanes_p, long long want, int floor_pix, int* ppb) {
  long long chunks = want / slabs; if (chunks < 1) chunks = 1;
  long long p = (HW + chunks - 1) / chunks; if (p < floor_pix * lanes_p) p = floor_pix * lanes_p;
  *ppb = (int)p;
  return (int)((HW + p - 1) / p);
}
// grid (channel tiles, row groups, N) of the generic per-sample reduces (64 channels x 4 row phases per block): about 2048 blocks, at least 16 rows per block
static inline dim3 bn_col_grid(int N, long long HW, int C, long long* rpb) {
  const int ct = (C + 63) / 64;
  long long want = 2048 / ((long long)ct * N); if (want < 1) want = 1;
  *rpb = (HW + want - 1) / want; if (*rpb < 16) *rpb = 16;
  return dim3(ct, (int)((HW + *rpb - 1) / *rpb), N);
}
// Streaming variant: grid (pixel chunks, N). A thread owns ONE 16-byte channel vector of ONE sample, so its
// scale/shift (8 or 4 channels) are computed once and the loop body is load -> fma -> store (the generic kernel
// re-reads 4 parameters per channel per element, which made it VALU/L1-bound at ~40 % of HBM speed).
template <typename T, int UN, bool NT> __global__ __launch_bounds__(256) void k_bn_apply_stream(const T* x, T* y, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gsn, int relu, int ppb) {
  constexpr int V = ET<T>::VEC;
  const int CV = C / V;
  const BnOwn w = bn_own(0, CV, blockDim.x / CV, V, HW, C, ppb);      // blockDim.x == CV * lanes_p
  float mu[V], is[V], ga[V], bi[V];
  bn_coef<V>(mean, invstd, gain, bias, gsn, blockIdx.y, w.cv * V, mu, is, ga, bi);
  const T* xs = x + (long long)blockIdx.y * HW * C + w.cv * V;      // (= x + w.base with the sample's uniform part added first, as this kernel has always formed it:
  T* ys = y + (long long)blockIdx.y * HW * C + w.cv * V;            //  from w.base the fp32 instantiations take four more registers)
  bn_walk<UN, 1>(w,
    [&](int, long long pix, bool unrolled) { return NT && unrolled ? __builtin_nontemporal_load((const u32x4*)(xs + pix * C)) : *(const u32x4*)(xs + pix * C); },
    [&](const u32x4* r, long long pix) {
      float xv[V];
      unpack16<T>(r[0], xv);
      bn_apply_elems<V>(xv, mu, is, ga, bi, relu);
      const u32x4 o = pack16<T>(xv);
      if (NT) __builtin_nontemporal_store(o, (u32x4*)(ys + pix * C)); else *(u32x4*)(ys + pix * C) = o;
    });
}
// one instantiation launched and counted under the variant number its template arguments stand for (not the one that was asked for)
template <typename T, int UN, bool NT> static void bn_apply_stream_go(dim3 grid, dim3 blk, hipStream_t st, const T* x, T* y, long long HW, int C, const float* mean, const float* invstd, const float* gain,
                                                                     const float* bias, int gsn, int relu, int ppb) {
  hipLaunchKernelGGL((k_bn_apply_stream<T, UN, NT>), grid, blk, 0, st, x, y, HW, C, mean, invstd, gain, bias, gsn, relu, ppb);
  bn_path_count(SG_BN_PATH_APPLY_STREAM_V0 + (UN == 8 ? 1 : 0) + (NT ? 2 : 0));
}
template <typename T> static void bn_apply_stream_launch(int variant, dim3 grid, dim3 blk, hipStream_t st, const T* x, T* y, long long HW, int C, const float* mean, const float* invstd, const float* gain,
                                                         const float* bias, int gsn, int relu, int ppb) {
  if (variant == 0) bn_apply_stream_go<T, 4, false>(grid, blk, st, x, y, HW, C, mean, invstd, gain, bias, gsn, relu, ppb);
  else if (variant == 1) bn_apply_stream_go<T, 8, false>(grid, blk, st, x, y, HW, C, mean, invstd, gain, bias, gsn, relu, ppb);
  else if (variant == 2) bn_apply_stream_go<T, 4, true>(grid, blk, st, x, y, HW, C, mean, invstd, gain, bias, gsn, relu, ppb);
  else bn_apply_stream_go<T, 8, true>(grid, blk, st, x, y, HW, C, mean, invstd, gain, bias, gsn, relu, ppb);
}
// The streaming variant and workgroup target of sg_bn_apply: SG_BN_APPLY (read once) or the default, unless sg_bn_apply_variant has set them for this process
static int g_bn_apply_set_variant = -1, g_bn_apply_set_want = 0;
extern "C" int sg_bn_apply_variant(int variant, int workgroups) {
  SG_CHECK(variant <= 3, "sg_bn_apply_variant: variant 0-3, or < 0 for what SG_BN_APPLY or the default says");
  __atomic_store_n(&g_bn_apply_set_want, variant >= 0 && workgroups > 0 ? workgroups : 0, __ATOMIC_RELAXED);
  __atomic_store_n(&g_bn_apply_set_variant, variant < 0 ? -1 : variant, __ATOMIC_RELAXED);
  return 0;
}
static void bn_apply_config(int* variant, long long* want) {
  static const char* ev = getenv("SG_BN_APPLY");
  *variant = ev && ev[0] >= '0' && ev[0] <= '3' ? ev[0] - '0' : 0;
  *want = ev && ev[0] && ev[1] >= '1' && ev[1] <= '9' ? 1024ll * (ev[1] - '0') : 2048;
  const int sv = __atomic_load_n(&g_bn_apply_set_variant, __ATOMIC_RELAXED), sw = __atomic_load_n(&g_bn_apply_set_want, __ATOMIC_RELAXED);
  if (sv >= 0) { *variant = sv; if (sw > 0) *want = sw; }
}
extern "C" int sg_bn_apply(int dtype, const void* x, void* y, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gb_stride_n, int relu, sg_stream_t s) {
  SgProfScope prof((hipStream_t)s, 2.0 * N * (double)HW * C * elem_bytes(dtype), 4);
  SG_CHECK(x && y && mean && invstd, "sg_bn_apply: null");
  DISPATCH_T(dtype, {
    const int CV = C / ET<T>::VEC;
    if (bn_streams<T>(vec_ok<T>(x, y, C), N, HW, C)) {
      const int lanes_p = 256 / CV;
      // Variant 0 = four loads in flight, 1 = eight, 2 = four + non-temporal accesses, 3 = eight + non-temporal; `want` workgroups (SG_BN_APPLY="<variant><workgroups / 1024>", A/B).
      // Measured (tools/bn_bench.py, profiles/r06_bn_apply_variants_r7f.txt): ALONE, this pass streams tensors far beyond the 256 MB Infinity Cache 7-12 % faster with non-temporal
      // accesses, eight loads in flight and 4096 workgroups (4.64 -> 5.10 TB/s on BigGAN-128's 128^2 maps). IN THE STEP no gain could be shown: A, B, A, B
      // alternations read +1.0 ms for the non-temporal arm (profiles/r06_bn_apply_step_ab_r7l.txt), but an ABBA series showed every second PROCESS on such a box running 1.5 ms
      // faster whatever the variant (profiles/r06_bn_apply_reverse_walk_r7r.txt): corrected, the effect lies between -0.9 and +0.2 ms. Unresolved, so the default stays variant 0
      // (the pass's output is the next convolution's input; what it leaves in the Infinity Cache may matter as much as its own 0.1 ms).
      int variant, ppb; long long want;
      bn_apply_config(&variant, &want);
      const int gx = bn_stream_geom(HW, N, lanes_p, want, 4, &ppb);
      bn_apply_stream_launch<T>(variant, dim3(gx, N), dim3(CV * lanes_p), (hipStream_t)s, (const T*)x, (T*)y, HW, C, mean, invstd, gain, bias, gb_stride_n, relu, ppb);
      bn_path_count(SG_BN_PATH_APPLY_STREAM);
    } else if (vec_ok<T>(x, y, C)) {
      hipLaunchKernelGGL((k_bn_apply<T, true>), dim3(grid_for((long long)N * HW * C / ET<T>::VEC)), dim3(256), 0, (hipStream_t)s, (const T*)x, (T*)y, N, HW, C, mean, invstd, gain, bias, gb_stride_n, relu);
      bn_path_count(SG_BN_PATH_APPLY_VEC);
    } else {
      hipLaunchKernelGGL((k_bn_apply<T, false>), dim3(grid_for((long long)N * HW * C)), dim3(256), 0, (hipStream_t)s, (const T*)x, (T*)y, N, HW, C, mean, invstd, gain, bias, gb_stride_n, relu);
      bn_path_count(SG_BN_PATH_APPLY_SCALAR);
    }
  });
  SG_LAUNCH_CHECK();
  return 0;
}

// ---- backward ----------------------------------------------------------------------------------------------
// stage 1: sums[n][c] = {sum_hw dy', sum_hw dy' * xhat}; grid (channel tiles, hw chunks, N); caller zeroes sums
template <typename T> __global__ __launch_bounds__(256) void k_bn_bwd_reduce(const T* x, const T* dy, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gsn, int relu, float* sums, long long rpb) {
  __shared__ float sm[2][4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  const int n = blockIdx.z;
  long long r0 = blockIdx.y * rpb, r1 = r0 + rpb; if (r1 > HW) r1 = HW;
  float s[2] = {0.f, 0.f};
  if (c < C) {
    float mu, is, ga, bi;
    bn_coef<1>(mean, invstd, gain, bias, gsn, n, c, &mu, &is, &ga, &bi);
    const T* xp = x + (long long)n * HW * C + c;
    const T* gp = dy + (long long)n * HW * C + c;
    for (long long r = r0 + ry; r < r1; r += 4) {
      const float xv = to_f<T>(xp[r * C]), gv = to_f<T>(gp[r * C]);
      bn_bwd_sum_elems<1>(&xv, &gv, &mu, &is, &ga, &bi, relu, &s[0], &s[1]);
    }
  }
  bn_col_store(sm, s, ry, cx);
  if (ry == 0 && c < C) {
    float* o = sums + ((long long)n * C + c) * 2;
#pragma unroll
    for (int k = 0; k < 2; k++) bn_atomic_add(o + k, bn_col_sum<false>(sm[k], cx));
  }
}
// Streaming variant of stage 1 (16-byte loads; thread = one channel vector of one sample; LDS combine; float atomics)
template <typename T> __global__ __launch_bounds__(256) void k_bn_bwd_reduce_stream(const T* x, const T* dy, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gsn, int relu, float* sums, int ppb) {
  constexpr int V = ET<T>::VEC;
  extern __shared__ float smf[];                        // [lanes_p][C][2]
  const int CV = C / V;
  const BnOwn w = bn_own(0, CV, blockDim.x / CV, V, HW, C, ppb);
  float mu[V], is[V], ga[V], bi[V], s1[V], s2[V];
  bn_coef<V>(mean, invstd, gain, bias, gsn, blockIdx.y, w.cv * V, mu, is, ga, bi);
#pragma unroll
  for (int e = 0; e < V; e++) { s1[e] = 0.f; s2[e] = 0.f; }
  bn_walk<4, 2>(w,                                           // eight loads in flight
    [&](int k, long long pix, bool) { return *(const u32x4*)((k ? dy : x) + w.base + pix * C); },
    [&](const u32x4* r, long long) {
      float xv[V], gv[V];
      unpack16<T>(r[0], xv);
      unpack16<T>(r[1], gv);
      bn_bwd_sum_elems<V>(xv, gv, mu, is, ga, bi, relu, s1, s2);
    });
  bn_lane_combine<V>(smf, s1, s2, w.pl, w.cv, w.lanes_p, C, sums + (long long)blockIdx.y * C * 2);
}
extern "C" int sg_bn_bwd_reduce(int dtype, const void* x, const void* dy, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gb_stride_n, int relu, float* sums, sg_stream_t s) {
  SgProfScope prof((hipStream_t)s, 2.0 * N * (double)HW * C * elem_bytes(dtype), 4);
  SG_CHECK(x && dy && mean && invstd && sums, "sg_bn_bwd_reduce: null");
  SG_CHECK(N <= 65535, "sg_bn_bwd_reduce: batch too large for grid.z");
  bool done = false;
  DISPATCH_T(dtype, {
    const int CV = C / ET<T>::VEC;
    if (bn_streams<T>(vec_ok<T>(x, dy, C), N, HW, C)) {
      const int lanes_p = 256 / CV;
      int ppb;
      const int gx = bn_stream_geom(HW, N, lanes_p, 2048, 8, &ppb);
      hipLaunchKernelGGL(k_bn_bwd_reduce_stream<T>, dim3(gx, N), dim3(CV * lanes_p), (size_t)lanes_p * C * 2 * sizeof(float), (hipStream_t)s, (const T*)x, (const T*)dy, HW, C, mean, invstd, gain, bias, gb_stride_n, relu, sums, ppb);
      bn_path_count(SG_BN_PATH_BWD_REDUCE_STREAM);
      done = true;
    }
  });
  if (done) { SG_LAUNCH_CHECK(); return 0; }
  long long rpb;
  const dim3 grid = bn_col_grid(N, HW, C, &rpb);
  DISPATCH_T(dtype, hipLaunchKernelGGL(k_bn_bwd_reduce<T>, grid, dim3(256), 0, (hipStream_t)s, (const T*)x, (const T*)dy, HW, C, mean, invstd, gain, bias, gb_stride_n, relu, sums, rpb));
  bn_path_count(SG_BN_PATH_BWD_REDUCE_GENERIC);
  SG_LAUNCH_CHECK();
  return 0;
}
// grid (C / 64), block (64 channels x 16 sample groups): the per-sample partial sums of sg_bn_bwd_reduce -> per-channel fp64 terms of
// the batch-statistics gradient, plus the (conditional) gain / bias gradients. One thread per channel walking all N samples (the
// first version) was a 256-long dependent chain per launch: 226 us average in the r01 trace for a few KB of data.
__global__ __launch_bounds__(1024) void k_bn_bwd_finalize(const float* sums, int N, int C, const float* gain, int gsn, float* dgain, float* dbias, double* chan) {
  __shared__ double sa0[16][64], sa1[16][64];
  __shared__ float sg0[16][64], sg1[16][64];
  const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double a0 = 0.0, a1 = 0.0; float g0 = 0.f, g1 = 0.f;
  if (c < C) {
    for (int n = grp; n < N; n += 16) {
      const float s1 = sums[((long long)n * C + c) * 2], s2 = sums[((long long)n * C + c) * 2 + 1];
      const float ga = gain ? gain[(long long)n * gsn + c] : 1.f;
      a0 += (double)ga * s1; a1 += (double)ga * s2;
      if (gsn) {     // per-sample gain / bias gradients at the row pitch of gain / bias themselves (gsn == C, or 2 C for the packed [gain | bias] rows of a cBN)
        if (dgain) dgain[(long long)n * gsn + c] += s2;
        if (dbias) dbias[(long long)n * gsn + c] += s1;
      } else { g0 += s1; g1 += s2; }
    }
  }
  sa0[grp][cl] = a0; sa1[grp][cl] = a1; sg0[grp][cl] = g0; sg1[grp][cl] = g1;
  __syncthreads();
  if (grp == 0 && c < C) {
    a0 = 0.0; a1 = 0.0; g0 = 0.f; g1 = 0.f;
    for (int g = 0; g < 16; g++) { a0 += sa0[g][cl]; a1 += sa1[g][cl]; g0 += sg0[g][cl]; g1 += sg1[g][cl]; }   // fixed order: deterministic
    if (!gsn) { if (dgain) dgain[c] += g1; if (dbias) dbias[c] += g0; }
    chan[2 * c] = a0; chan[2 * c + 1] = a1;
  }
}
extern "C" int sg_bn_bwd_finalize(const float* sums, int N, int C, const float* gain, int gb_stride_n, float* dgain, float* dbias, double* chan, sg_stream_t s) {
  SG_CHECK(sums && chan, "sg_bn_bwd_finalize: null");
  hipLaunchKernelGGL(k_bn_bwd_finalize, dim3((C + 63) / 64), dim3(1024), 0, (hipStream_t)s, sums, N, C, gain, gb_stride_n, dgain, dbias, chan);
  SG_LAUNCH_CHECK();
  return 0;
}
// res (optional): a tensor of dx's shape ADDED to the result -- the gradient the same input received through another branch (a residual block's
// skip path), so that the sum autograd would run as its own elementwise launch rides in this one.
template <typename T, bool VECP> __global__ __launch_bounds__(256) void k_bn_bwd_apply(const T* x, const T* dy, T* dx, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gsn, int relu, const double* chan, double count, int use_batch, const T* res) {
  constexpr int V = VECP ? ET<T>::VEC : 1;
  const int CV = C / V;
  const long long total = (long long)N * HW * CV;
  const float invc = (float)(1.0 / count);
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int cv = (int)(i % CV); const long long pix = i / CV; const int n = (int)(pix / HW);
    const long long o = pix * C + cv * V;
    float xv[V], gv[V], mu[V], is[V], ga[V], bi[V], k0[V], k1[V];
    load_f<T, V>(x + o, xv);
    load_f<T, V>(dy + o, gv);
    bn_coef<V>(mean, invstd, gain, bias, gsn, n, cv * V, mu, is, ga, bi, chan, use_batch, k0, k1);
    bn_bwd_apply_elems<T, V>(xv, gv, res ? res + o : nullptr, mu, is, ga, bi, k0, k1, invc, relu, use_batch);
    *(vec_t<T, V>*)(dx + o) = pack_f<T, V>(xv);
  }
}
// Streaming variant (same ownership as k_bn_apply_stream): a thread keeps the 6 per-channel coefficients of its 16-byte
// channel vector in registers; the loop body is 2 loads -> ~6 flops per element -> 1 store.
template <typename T> __global__ __launch_bounds__(256) void k_bn_bwd_apply_stream(const T* x, const T* dy, T* dx, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gsn, int relu, const double* chan, double count, int use_batch, int ppb, const T* res) {
  constexpr int V = ET<T>::VEC;
  const int CV = C / V;
  const BnOwn w = bn_own(0, CV, blockDim.x / CV, V, HW, C, ppb);
  const float invc = (float)(1.0 / count);
  float mu[V], is[V], ga[V], bi[V], k0[V], k1[V];
  bn_coef<V>(mean, invstd, gain, bias, gsn, blockIdx.y, w.cv * V, mu, is, ga, bi, chan, use_batch, k0, k1);
  bn_walk<4, 2>(w,                                           // four pixels = eight loads in flight per lane
    [&](int k, long long pix, bool) { return *(const u32x4*)((k ? dy : x) + w.base + pix * C); },
    [&](const u32x4* r, long long pix) {
      float xv[V], gv[V];
      unpack16<T>(r[0], xv);
      unpack16<T>(r[1], gv);
      bn_bwd_apply_elems<T, V>(xv, gv, res ? res + w.base + pix * C : nullptr, mu, is, ga, bi, k0, k1, invc, relu, use_batch);
      *(u32x4*)(dx + w.base + pix * C) = pack16<T>(xv);
    });
}
extern "C" int sg_bn_bwd_apply(int dtype, const void* x, const void* dy, void* dx, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gb_stride_n, int relu, const double* chan, double count, int use_batch_stats, sg_stream_t s) {
  return sg_bn_bwd_apply_res(dtype, x, dy, dx, N, HW, C, mean, invstd, gain, bias, gb_stride_n, relu, chan, count, use_batch_stats, nullptr, s);
}
extern "C" int sg_bn_bwd_apply_res(int dtype, const void* x, const void* dy, void* dx, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gb_stride_n, int relu, const double* chan, double count, int use_batch_stats, const void* res, sg_stream_t s) {
  SgProfScope prof((hipStream_t)s, (res ? 4.0 : 3.0) * N * (double)HW * C * elem_bytes(dtype), 4);
  SG_CHECK(x && dy && dx && mean && invstd && chan && count > 0, "sg_bn_bwd_apply: bad args");
  SG_CHECK(!res || ((((uintptr_t)res) & 15) == 0), "sg_bn_bwd_apply_res: res must be 16-byte aligned");
  DISPATCH_T(dtype, {
    const int CV = C / ET<T>::VEC;
    const bool vec = vec_ok<T>(x, dy, C) && ((((uintptr_t)dx) & 15) == 0);
    if (bn_streams<T>(vec, N, HW, C)) {
      const int lanes_p = 256 / CV;
      int ppb;
      const int gx = bn_stream_geom(HW, N, lanes_p, 2048, 4, &ppb);
      hipLaunchKernelGGL(k_bn_bwd_apply_stream<T>, dim3(gx, N), dim3(CV * lanes_p), 0, (hipStream_t)s, (const T*)x, (const T*)dy, (T*)dx, HW, C, mean, invstd, gain, bias, gb_stride_n, relu, chan, count, use_batch_stats, ppb, (const T*)res);
      bn_path_count(SG_BN_PATH_BWD_APPLY_STREAM);
    } else if (vec) {
      hipLaunchKernelGGL((k_bn_bwd_apply<T, true>), dim3(grid_for((long long)N * HW * C / ET<T>::VEC)), dim3(256), 0, (hipStream_t)s, (const T*)x, (const T*)dy, (T*)dx, N, HW, C, mean, invstd, gain, bias, gb_stride_n, relu, chan, count, use_batch_stats, (const T*)res);
      bn_path_count(SG_BN_PATH_BWD_APPLY_VEC);
    } else {
      hipLaunchKernelGGL((k_bn_bwd_apply<T, false>), dim3(grid_for((long long)N * HW * C)), dim3(256), 0, (hipStream_t)s, (const T*)x, (const T*)dy, (T*)dx, N, HW, C, mean, invstd, gain, bias, gb_stride_n, relu, chan, count, use_batch_stats, (const T*)res);
      bn_path_count(SG_BN_PATH_BWD_APPLY_SCALAR);
    }
  });
  SG_LAUNCH_CHECK();
  return 0;
}

// ---- second-order backward (WGAN-GP: gradient of the gradient penalty through BN's data gradient) -------------------
// First order (per channel, gain g_c, r = invstd, N = count, g = dy' after the ReLU mask):
//     dx = g_c r ( g - mean(g) - xhat mean(g xhat) )
// Given u = dL/d(dx), with  ub = mean(u), a = mean(u xhat), gb = mean(g), c = mean(g xhat), m = mean(u g):
//     dL/d(dy) = mask * g_c r ( u - ub - xhat a )
//     dL/dx    = g_c r^2 ( -c (u - ub) - a (g - gb) + xhat (3 a c - m + ub gb) )
//     dL/dg_c  = r N ( m - ub gb - a c )                       (reference: torch autograd through F.batch_norm's backward,
//                                                               reached from utils/losses.py:268-275,301-316)
// stage 1: sums[n][c][5] = {sum u, sum u xhat, sum g, sum g xhat, sum u g}; caller zeroes sums. Only the mask reads gain / bias, as rows of pitch gsn: the
// per-channel pass (sg_bn_bwd2_reduce) is pitch 0, the per-sample pass below (sg_cbn_bwd2_reduce) the pitch of its rows
template <typename T> __global__ __launch_bounds__(256) void k_cbn_bwd2_reduce(const T* x, const T* dy, const T* u, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gsn, int relu, float* sums, long long rpb) {
  __shared__ float sm[5][4][64];
  const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cx;
  const int n = blockIdx.z;
  long long r0 = blockIdx.y * rpb, r1 = r0 + rpb; if (r1 > HW) r1 = HW;
  float s[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    float mu, is, ga, bi;
    bn_coef<1>(mean, invstd, gain, bias, gsn, n, c, &mu, &is, &ga, &bi);
    const long long base = (long long)n * HW * C + c;
    for (long long r = r0 + ry; r < r1; r += 4) {
      const float xh = bn_xhat(to_f<T>(x[base + r * C]), mu, is);
      float g = to_f<T>(dy[base + r * C]);
      if (!bn_gate(relu, xh, ga, bi)) g = 0.f;
      const float uu = to_f<T>(u[base + r * C]);
      s[0] += uu; s[1] += uu * xh; s[2] += g; s[3] += g * xh; s[4] += uu * g;
    }
  }
  bn_col_store(sm, s, ry, cx);
  if (ry == 0 && c < C) {
    float* o = sums + ((long long)n * C + c) * 5;
#pragma unroll
    for (int k = 0; k < 5; k++) bn_atomic_add(o + k, bn_col_sum<false>(sm[k], cx));
  }
}
static int bn_bwd2_reduce_launch(int dtype, const void* x, const void* dy, const void* u, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gsn, int relu, float* sums, sg_stream_t s) {
  long long rpb;
  const dim3 grid = bn_col_grid(N, HW, C, &rpb);
  DISPATCH_T(dtype, hipLaunchKernelGGL(k_cbn_bwd2_reduce<T>, grid, dim3(256), 0, (hipStream_t)s, (const T*)x, (const T*)dy, (const T*)u, HW, C, mean, invstd, gain, bias, gsn, relu, sums, rpb));
  SG_LAUNCH_CHECK();
  return 0;
}
extern "C" int sg_bn_bwd2_reduce(int dtype, const void* x, const void* dy, const void* u, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int relu, float* sums, sg_stream_t s) {
  SG_CHECK(x && dy && u && mean && invstd && sums, "sg_bn_bwd2_reduce: null");
  SG_CHECK(N <= 65535, "sg_bn_bwd2_reduce: batch too large for grid.z");
  return bn_bwd2_reduce_launch(dtype, x, dy, u, N, HW, C, mean, invstd, gain, bias, 0, relu, sums, s);
}
// stage 2: chan[c][5] (fp64) = sum over n
__global__ void k_bn_bwd2_finalize(const float* sums, int N, int C, double* chan) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double a[5] = {0, 0, 0, 0, 0};
  for (int n = 0; n < N; n++)
    for (int k = 0; k < 5; k++) a[k] += (double)sums[((long long)n * C + c) * 5 + k];
  for (int k = 0; k < 5; k++) chan[5 * c + k] = a[k];
}
extern "C" int sg_bn_bwd2_finalize(const float* sums, int N, int C, double* chan, sg_stream_t s) {
  SG_CHECK(sums && chan, "sg_bn_bwd2_finalize: null");
  hipLaunchKernelGGL(k_bn_bwd2_finalize, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)s, sums, N, C, chan);
  SG_LAUNCH_CHECK();
  return 0;
}
// gain gradient from this rank's own sums (chan_local) and the statistics of the whole (possibly cross-rank) batch (chan)
__global__ void k_bn_bwd2_dgain(const double* chan_local, const double* chan, double count, const float* invstd, int C, int use_batch, float* dgain) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double r = invstd[c];
  double v;
  if (use_batch) {
    const double gb = chan[5 * c + 2] / count, cc = chan[5 * c + 3] / count;
    v = r * (chan_local[5 * c + 4] - gb * chan_local[5 * c + 0] - cc * chan_local[5 * c + 1]);
  } else v = r * chan_local[5 * c + 4];
  dgain[c] += (float)v;
}
extern "C" int sg_bn_bwd2_dgain(const double* chan_local, const double* chan, double count, const float* invstd, int C, int use_batch_stats, float* dgain, sg_stream_t s) {
  SG_CHECK(chan_local && chan && invstd && dgain && count > 0, "sg_bn_bwd2_dgain: bad args");
  hipLaunchKernelGGL(k_bn_bwd2_dgain, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)s, chan_local, chan, count, invstd, C, use_batch_stats, dgain);
  SG_LAUNCH_CHECK();
  return 0;
}
// stage 3: elementwise; g_dy and/or g_x may be null
template <typename T> __global__ __launch_bounds__(256) void k_bn_bwd2_apply(const T* x, const T* dy, const T* u, T* g_dy, T* g_x, long long total, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int relu, const double* chan, double count, int use_batch) {
  const float invc = (float)(1.0 / count);
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int c = (int)(i % C);
    float mu, is, ga, bi;
    bn_coef<1>(mean, invstd, gain, bias, 0, 0, c, &mu, &is, &ga, &bi);
    const float xh = bn_xhat(to_f<T>(x[i]), mu, is);
    const bool on = bn_gate(relu, xh, ga, bi);
    const float g = on ? to_f<T>(dy[i]) : 0.f;
    const float uu = to_f<T>(u[i]);
    float ub = 0.f, a = 0.f, gb = 0.f, cc = 0.f, m = 0.f;
    if (use_batch) {
      ub = (float)chan[5 * c] * invc; a = (float)chan[5 * c + 1] * invc; gb = (float)chan[5 * c + 2] * invc;
      cc = (float)chan[5 * c + 3] * invc; m = (float)chan[5 * c + 4] * invc;
    }
    if (g_dy) g_dy[i] = from_f<T>(on ? ga * is * (uu - ub - xh * a) : 0.f);
    if (g_x) g_x[i] = from_f<T>(use_batch ? ga * is * is * (-cc * (uu - ub) - a * (g - gb) + xh * (3.f * a * cc - m + ub * gb)) : 0.f);
  }
}
extern "C" int sg_bn_bwd2_apply(int dtype, const void* x, const void* dy, const void* u, void* g_dy, void* g_x, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int relu, const double* chan, double count, int use_batch_stats, sg_stream_t s) {
  SG_CHECK(x && dy && u && mean && invstd && chan && count > 0 && (g_dy || g_x), "sg_bn_bwd2_apply: bad args");
  const long long total = (long long)N * HW * C;
  DISPATCH_T(dtype, hipLaunchKernelGGL(k_bn_bwd2_apply<T>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)s, (const T*)x, (const T*)dy, (const T*)u, (T*)g_dy, (T*)g_x, total, C, mean, invstd, gain, bias, relu, chan, count, use_batch_stats));
  SG_LAUNCH_CHECK();
  return 0;
}

// ---- second-order backward with per-sample affine rows (conditional batch norm: latent optimisation through a class-conditional generator) ----
// First order (per channel; sample n has the rows gam_n, bet_n; r = invstd, M = count, s = 1 with batch statistics else 0; g = dy' after the
// ReLU mask [gam_n xhat + bet_n > 0], h = gam_n g):
//     dx     = r ( h - s mean(h) - s xhat mean(h xhat) )        dgam_n = sum_p g xhat        dbet_n = sum_p g
// Given the cotangents u (of dx), A_n (of dgam_n), B_n (of dbet_n), with  ub = mean(u), a = mean(u xhat), hb = mean(h), ch = mean(h xhat),
// mh = mean(u h), w = A_n g, wb = mean(w), wx = mean(w xhat):
//     dL/d(dy)   = mask * ( gam_n r (u - s ub - s xhat a) + A_n xhat + B_n )
//     dL/dgam_n  = r ( sum_p g u - s ub sum_p g - s a sum_p g xhat )
//     dL/dx      = s r^2 ( -ch (u - ub) - a (h - hb) + xhat (3 a ch - mh + ub hb) ) + r ( w - s wb - s xhat wx )
//     dL/dbet_n  = 0                                              (the bias enters through the mask only)
// With gam_n = g_c for every n and A = B = 0 these are the per-channel formulas above. Same launch structure: reduce -> finalize -> apply (+ gain rows).
// stage 1: the per-channel pass's five sums per (n, c), by its kernel (k_cbn_bwd2_reduce above) at the pitch of the rows; caller zeroes sums
extern "C" int sg_cbn_bwd2_reduce(int dtype, const void* x, const void* dy, const void* u, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, int gb_stride_n, int relu, float* sums, sg_stream_t s) {
  SG_CHECK(x && dy && u && mean && invstd && sums && N > 0 && HW > 0 && C > 0, "sg_cbn_bwd2_reduce: bad args");
  SG_CHECK(N <= 65535, "sg_cbn_bwd2_reduce: batch too large for grid.z");
  SG_CHECK((!gain && !bias) || gb_stride_n >= C, "sg_cbn_bwd2_reduce: row pitch below C");
  return bn_bwd2_reduce_launch(dtype, x, dy, u, N, HW, C, mean, invstd, gain, bias, gb_stride_n, relu, sums, s);
}
// stage 2: chan[c][7] (fp64) = {sum_n S0, sum_n S1, sum_n gam_n S2, sum_n gam_n S3, sum_n gam_n S4, sum_n A_n S2, sum_n A_n S3}; block = 64 channels x 4 sample
// groups, combined in a fixed order (deterministic). A (cotangent of the gain rows, pitch gsn as the rows themselves) may be null
__global__ __launch_bounds__(256) void k_cbn_bwd2_finalize(const float* sums, int N, int C, const float* gain, const float* A, int gsn, double* chan) {
  __shared__ double sa[7][4][64];
  const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double a[7] = {0, 0, 0, 0, 0, 0, 0};
  if (c < C) {
    for (int n = grp; n < N; n += 4) {
      const float* sp = sums + ((long long)n * C + c) * 5;
      const double ga = gain ? (double)gain[(long long)n * gsn + c] : 1.0;
      const double an = A ? (double)A[(long long)n * gsn + c] : 0.0;
      a[0] += (double)sp[0]; a[1] += (double)sp[1];
      a[2] += ga * sp[2]; a[3] += ga * sp[3]; a[4] += ga * sp[4];
      a[5] += an * sp[2]; a[6] += an * sp[3];
    }
  }
  bn_col_store(sa, a, grp, cl);
  if (grp == 0 && c < C) {
#pragma unroll
    for (int k = 0; k < 7; k++) chan[7 * c + k] = bn_col_sum<true>(sa[k], cl);
  }
}
extern "C" int sg_cbn_bwd2_finalize(const float* sums, int N, int C, const float* gain, const float* A, int gb_stride_n, double* chan, sg_stream_t s) {
  SG_CHECK(sums && chan && N > 0 && C > 0, "sg_cbn_bwd2_finalize: bad args");
  SG_CHECK((!gain && !A) || gb_stride_n >= C, "sg_cbn_bwd2_finalize: row pitch below C");
  hipLaunchKernelGGL(k_cbn_bwd2_finalize, dim3((C + 63) / 64), dim3(256), 0, (hipStream_t)s, sums, N, C, gain, A, gb_stride_n, chan);
  SG_LAUNCH_CHECK();
  return 0;
}
// gradient of the gain rows: dgain[n][c] += r ( S4 - s ub S2 - s a S3 ), rows of pitch gsn
__global__ __launch_bounds__(256) void k_cbn_bwd2_dgain(const float* sums, const double* chan, double count, const float* invstd, int N, int C, int gsn, int use_batch, float* dgain) {
  const long long i = blockIdx.x * 256ll + threadIdx.x;
  if (i >= (long long)N * C) return;
  const int c = (int)(i % C); const long long n = i / C;
  const float* sp = sums + i * 5;
  double v = (double)sp[4];
  if (use_batch) v -= (chan[7 * c] / count) * (double)sp[2] + (chan[7 * c + 1] / count) * (double)sp[3];
  dgain[n * gsn + c] += (float)((double)invstd[c] * v);
}
extern "C" int sg_cbn_bwd2_dgain(const float* sums, const double* chan, double count, const float* invstd, int N, int C, int gb_stride_n, int use_batch_stats, float* dgain, sg_stream_t s) {
  SG_CHECK(sums && chan && invstd && dgain && count > 0 && N > 0 && C > 0 && gb_stride_n >= C, "sg_cbn_bwd2_dgain: bad args");
  hipLaunchKernelGGL(k_cbn_bwd2_dgain, dim3((unsigned)(((long long)N * C + 255) / 256)), dim3(256), 0, (hipStream_t)s, sums, chan, count, invstd, N, C, gb_stride_n, use_batch_stats, dgain);
  SG_LAUNCH_CHECK();
  return 0;
}
// stage 3: streaming pass over x, dy, u -> g_dy and / or g_x. Grid (pixel chunks, N, tiles of `cvt` channel vectors): a thread owns ONE channel vector (16 bytes
// with VECP, else one element) of ONE sample and folds the per-channel terms and its sample's rows into 7 coefficients per channel once, in fp64:
//     g_dy = mask (P u + Q xhat + R)                 P = gam r,  Q = A - s P a,  R = B - s P ub
//     g_x  = E1 u + E2 g + E3 xhat + E4              E1 = -s r^2 ch,  E2 = r A - s r^2 a gam,  E3 = s r^2 (3 a ch - mh + ub hb) - s r wx,  E4 = s r^2 (ch ub + a hb) - s r wb
// so that the loop body is 3 loads -> ~10 flops per element -> 2 stores.
template <typename T, bool VECP> __global__ __launch_bounds__(256) void k_cbn_bwd2_apply(const T* x, const T* dy, const T* u, T* g_dy, T* g_x, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, const float* A, const float* Bc, int gsn, int relu, const double* chan, double count, int use_batch, int ppb, int cvt) {
  constexpr int V = VECP ? ET<T>::VEC : 1;
  const int CV = C / V;
  const int n = blockIdx.y;
  const BnOwn w = bn_own(blockIdx.z * cvt, cvt, 256 / cvt, V, HW, C, ppb);
  if (w.pl >= w.lanes_p || w.cv >= CV) return;
  float mu[V], is[V], ga[V], bi[V], P[V], Q[V], R[V], E1[V], E2[V], E3[V], E4[V];
  bn_coef<V>(mean, invstd, gain, bias, gsn, n, w.cv * V, mu, is, ga, bi);
#pragma unroll
  for (int e = 0; e < V; e++) {
    const int c = w.cv * V + e;
    const double r = is[e], gm = ga[e];
    const double an = A ? (double)A[(long long)n * gsn + c] : 0.0, bn = Bc ? (double)Bc[(long long)n * gsn + c] : 0.0;
    double p = gm * r, q = an, rr = bn, e1 = 0.0, e2 = r * an, e3 = 0.0, e4 = 0.0;
    if (use_batch) {
      const double* ch = chan + 7 * c;
      const double ub = ch[0] / count, a = ch[1] / count, hb = ch[2] / count, chh = ch[3] / count, mh = ch[4] / count, wb = ch[5] / count, wx = ch[6] / count;
      q -= p * a; rr -= p * ub;
      e1 = -r * r * chh; e2 -= r * r * a * gm;
      e3 = r * r * (3.0 * a * chh - mh + ub * hb) - r * wx;
      e4 = r * r * (chh * ub + a * hb) - r * wb;
    }
    P[e] = (float)p; Q[e] = (float)q; R[e] = (float)rr; E1[e] = (float)e1; E2[e] = (float)e2; E3[e] = (float)e3; E4[e] = (float)e4;
  }
#pragma unroll 2
  for (long long pix = w.p0 + w.pl; pix < w.p1; pix += w.lanes_p) {
    const long long o = w.base + pix * C;
    float xv[V], gv[V], uv[V], o1[V], o2[V];
    load_f<T, V>(x + o, xv);
    load_f<T, V>(dy + o, gv);
    load_f<T, V>(u + o, uv);
#pragma unroll
    for (int e = 0; e < V; e++) {
      const float xh = bn_xhat(xv[e], mu[e], is[e]);
      const bool on = bn_gate(relu, xh, ga[e], bi[e]);
      const float g = on ? gv[e] : 0.f;
      o1[e] = on ? (P[e] * uv[e] + Q[e] * xh + R[e]) : 0.f;
      o2[e] = E1[e] * uv[e] + E2[e] * g + E3[e] * xh + E4[e];
    }
    if (g_dy) *(vec_t<T, V>*)(g_dy + o) = pack_f<T, V>(o1);
    if (g_x) *(vec_t<T, V>*)(g_x + o) = pack_f<T, V>(o2);
  }
}
extern "C" int sg_cbn_bwd2_apply(int dtype, const void* x, const void* dy, const void* u, void* g_dy, void* g_x, int N, long long HW, int C, const float* mean, const float* invstd, const float* gain, const float* bias, const float* A, const float* B, int gb_stride_n, int relu, const double* chan, double count, int use_batch_stats, sg_stream_t s) {
  SG_CHECK(x && dy && u && mean && invstd && chan && count > 0 && (g_dy || g_x) && N > 0 && HW > 0 && C > 0, "sg_cbn_bwd2_apply: bad args");
  SG_CHECK(N <= 65535, "sg_cbn_bwd2_apply: batch too large for grid.y");
  SG_CHECK((!gain && !bias && !A && !B) || gb_stride_n >= C, "sg_cbn_bwd2_apply: row pitch below C");
  DISPATCH_T(dtype, {
    const bool vec = vec_ok<T>(x, dy, C) && (((((uintptr_t)u) | ((uintptr_t)g_dy) | ((uintptr_t)g_x)) & 15) == 0);
    const int CV = vec ? C / ET<T>::VEC : C;
    const int cvt = CV < 256 ? CV : 256;
    const int gz = (CV + cvt - 1) / cvt;
    int ppb;
    const int gx = bn_stream_geom(HW, (long long)N * gz, 256 / cvt, 2048, 4, &ppb);
    if (vec) hipLaunchKernelGGL((k_cbn_bwd2_apply<T, true>), dim3(gx, N, gz), dim3(256), 0, (hipStream_t)s, (const T*)x, (const T*)dy, (const T*)u, (T*)g_dy, (T*)g_x, HW, C, mean, invstd, gain, bias, A, B, gb_stride_n, relu, chan, count, use_batch_stats, ppb, cvt);
    else hipLaunchKernelGGL((k_cbn_bwd2_apply<T, false>), dim3(gx, N, gz), dim3(256), 0, (hipStream_t)s, (const T*)x, (const T*)dy, (const T*)u, (T*)g_dy, (T*)g_x, HW, C, mean, invstd, gain, bias, A, B, gb_stride_n, relu, chan, count, use_batch_stats, ppb, cvt);
    bn_path_count(vec ? SG_BN_PATH_CBN_BWD2_APPLY_VEC : SG_BN_PATH_CBN_BWD2_APPLY_SCALAR);
  });
  SG_LAUNCH_CHECK();
  return 0;
}
