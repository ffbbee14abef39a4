// modconv.hip -- StyleGAN2's modulated, demodulated convolution (reference src/models/stylegan2.py:28-98) as ONE shared-weight implicit GEMM:
//
//   out[n,p,o] = post[n,o] * sum_{r,s,c} W[o][r][s][c] * ( pre[n,c] * x[n, tap(p,r,s), c] ) + noise[n,p] (+ bias[o])
//
// The reference builds per-sample weights [N,Cout,Cin,k,k] and runs a grouped convolution with groups = N. Here the weight image stays shared by all
// pixels of a tile: the per-(sample, input channel) factor rides on the activation chunk while it sits in registers between the global load and the
// LDS store of gemm_core.h's kernel (ModPixKC wraps ConvPixKC, which knows the sample of every row), the per-(sample, output channel) factor and
// the noise plane are applied to the fp32 accumulator (ModEpilogue wraps Epilogue; a 256-pixel tile of an 8 x 8 map holds four samples, so n is
// taken per row). Tiling, LDS images, fragment reads and the store are gemm_core.h's: nothing of the contraction is restated here.
// bf16: pre * x is formed in fp32 and rounded to bf16 once, for the MFMA; post and noise meet the fp32 accumulator before the single rounding on store.
// fp32: v_mfma_f32_32x32x2_f32 (the exact chain) whatever sg_set_f32_mode says -- the operator's fp32 is a parity path.
#include "conv_common.h"

static long long g_modconv_launches = 0, g_modconv_jvp_launches = 0;
extern "C" long long sg_modconv_launches() { return __atomic_load_n(&g_modconv_launches, __ATOMIC_RELAXED); }
extern "C" long long sg_modconv_jvp_launches() { return __atomic_load_n(&g_modconv_jvp_launches, __ATOMIC_RELAXED); }

// ---- the forward-mode tangent (second order: path-length regularisation), JVP = true below ------------------------------------------------------
//   out[n,p,o] = post[n,o] * sum_{r,s,c} W[o][r][s][c] * ( pre[n,c] * vx[n,tap,c] + vs[n,c] * x[n,tap,c] )  +  e[n,o] * ( y[n,p,o] - noise[n,p] )
// the tangent of the forward along (vx, vs): the operand of the contraction is the tangent of pre * x, the last term the tangent of the demodulation
// coefficient riding on the stored result. Same engine, same policies: what the tangent adds to each sits in an `if constexpr (JVP)` and in members that are
// empty for the plain instantiation. The kernels are the ones the two separate pairs of policies compiled to, instruction for instruction (20 of the 22; the
// two bf16 16-byte-path tangent kernels differ by one s_nop per table read): the members keep their places among the kernel arguments and the table reads
// their order, which is what the scheduler starts from -- both are written as they are for that reason (profiles/modconv_fold_resources.txt).

// VEC factors of each of NT [N][C] table rows for the chunk that starts at channel c0: ONE walk over the chunk's channels reads every table
template <int VEC, bool FAST, int NT> __device__ __forceinline__ void mod_factors(const float* const (&row)[NT], int c0, int C, float (&m)[NT][VEC]) {
  if constexpr (FAST) {        // C % VEC == 0: the chunk is VEC consecutive channels of one tap; the tables are 16-byte aligned (launcher)
#pragma unroll
    for (int q = 0; q < VEC / 4; q++) {
#pragma unroll
      for (int k = 0; k < NT; k++) {
        const f32x4 t = *(const f32x4*)(row[k] + c0 + 4 * q);
        m[k][4 * q] = t[0]; m[k][4 * q + 1] = t[1]; m[k][4 * q + 2] = t[2]; m[k][4 * q + 3] = t[3];
      }
    }
  } else {                     // the chunk may run over a tap boundary: the channel wraps (more than once when C < VEC)
    int c = c0;
#pragma unroll
    for (int e = 0; e < VEC; e++) {
#pragma unroll
      for (int k = 0; k < NT; k++) m[k][e] = row[k][c];
      c++; if (c == C) c = 0;
    }
  }
}

// a member only the tangent has: M with JVP, else an empty type of its own (ID) that [[no_unique_address]] gives no room, so that the plain instantiation's
// kernel arguments are those of a struct without it, and the tangent's stand in the order M is declared at
template <int ID> struct ModAbsent {};
template <bool JVP, typename M, int ID> using mod_tangent_t = std::conditional_t<JVP, M, ModAbsent<ID>>;

// pixel-side operand with the per-(sample, channel) factor folded in: pre * x, or its tangent vs * x + pre * vx; formed in fp32, rounded once to the MFMA operand
template <typename T, bool FAST, bool JVP = false> struct ModPixKC {
  static constexpr bool KC = true;
  static constexpr int VEC = ET<T>::VEC, BK = ET<T>::BK, NT = JVP ? 2 : 1;
  typedef ConvPixKC<T, FAST> Base;
  typedef typename Base::Chunk Chunk;
  Base b;                                                     // x
  [[no_unique_address]] mod_tangent_t<JVP, Base, 0> bv;          // vx: the geometry of b, another base pointer
  const float* pre;                                           // [N][C] fp32: the styles; the plain instantiation takes nullptr (the chunk passes as loaded)
  [[no_unique_address]] mod_tangent_t<JVP, const float*, 1> vs;  // [N][C] fp32: the tangent of the styles
  __device__ __forceinline__ void set_batch(int) {}
  __device__ __forceinline__ void init(Chunk& ch, int row, int k) const { b.init(ch, row, k); }
  __device__ __forceinline__ void advance(Chunk& ch) const { b.advance(ch); }
  __device__ __forceinline__ u32x4 load(const Chunk& ch) const {
    const u32x4 v = b.load(ch);
    u32x4 vv;                  // the chunk of vx at the same geometry: both global loads are issued before either is unpacked
    if constexpr (JVP) vv = bv.load(ch);
    else if (!pre) return v;
    // rows behind the problem hold zeros and have no sample (ch.n >= N): row 0 of the tables stands in. ch.c is always inside [0, C).
    const long long row = ch.valid ? (long long)ch.n * b.g.C : 0ll;
    const float* tab[NT];
    tab[0] = pre + row;
    if constexpr (JVP) tab[1] = vs + row;
    float f[VEC], m[NT][VEC];
    mod_factors<VEC, FAST, NT>(tab, ch.c, b.g.C, m);
    unpack16<T>(v, f);
    if constexpr (JVP) {
      float fv[VEC];
      unpack16<T>(vv, fv);
#pragma unroll
      for (int e = 0; e < VEC; e++) f[e] = m[1][e] * f[e] + m[0][e] * fv[e];
    } else {
#pragma unroll
      for (int e = 0; e < VEC; e++) f[e] *= m[0][e];
    }
    if constexpr (sizeof(T) == 4) return pack16<float>(f);
    else {
      u32x4 o;
#pragma unroll
      for (int e = 0; e < 4; e++) o[e] = pack2bf(f[2 * e], f[2 * e + 1]);
      return o;
    }
  }
};

// Epilogue + the per-(sample, cout) factor on the fp32 accumulator, then the noise plane or the tangent's e * (y - noise) from the stored forward result;
// one rounding, on store
template <typename T, bool JVP = false> struct ModEpilogue : Epilogue<T> {
  const float* post;                                          // [N][I] or nullptr
  [[no_unique_address]] mod_tangent_t<JVP, const float*, 2> e;   // [N][I] or nullptr (no demodulation: no second term, y is not read)
  [[no_unique_address]] mod_tangent_t<JVP, const T*, 3> y;       // [J][ldy]: the forward's result
  const float* noise;                                         // [.][HW] or nullptr; the tangent's: what the forward added to y
  long long noise_stride;                                     // floats between samples; 0 = one plane for all
  [[no_unique_address]] mod_tangent_t<JVP, int, 4> ldy;
  int HW;
  int tab_vec;             // I % 4 == 0 and 16-byte aligned tables: a lane's four factors of a table row in one f32x4 load
  static __device__ __forceinline__ void load4(const float* t, float d[4]) {
    const f32x4 q = *(const f32x4*)t;
    d[0] = q[0]; d[1] = q[1]; d[2] = q[2]; d[3] = q[3];
  }
  __device__ __forceinline__ void store(int j, int i0, float v[4], float a) const {
    if (j < this->J && i0 < this->I) {
      const int n = j / HW, p = j - n * HW;
      const int ne = (this->I - i0) < 4 ? (this->I - i0) : 4;
      float d[4] = {1.f, 1.f, 1.f, 1.f};
      // The two table fetches below do the same thing and are NOT written as one: the tangent branches on tab_vec first and on each table inside, the plain
      // one on post first, and either shape given to the other changes that kernel's instruction stream (tried both ways).
      if constexpr (JVP) {
        float c[4] = {0.f, 0.f, 0.f, 0.f}, u[4] = {0.f, 0.f, 0.f, 0.f};
        const long long row = (long long)n * this->I + i0;
        if (tab_vec) {
          if (post) load4(post + row, d);
          if (e) load4(e + row, c);
        } else {
#pragma unroll
          for (int q = 0; q < 4; q++) if (q < ne) { if (post) d[q] = post[row + q]; if (e) c[q] = e[row + q]; }
        }
        if (e) {               // (without e the launcher passes no noise either)
          const float z = noise ? noise[(long long)n * noise_stride + p] : 0.f;
          const T* yr = y + (long long)j * ldy + i0;
#pragma unroll
          for (int q = 0; q < 4; q++) if (q < ne) u[q] = to_f<T>(yr[q]) - z;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = v[q] * a * d[q] + c[q] * u[q];
      } else {
        const float z = noise ? noise[(long long)n * noise_stride + p] : 0.f;
        if (post) {
          const float* pr = post + (long long)n * this->I + i0;
          if (tab_vec) load4(pr, d);
          else {
#pragma unroll
            for (int e = 0; e < 4; e++) if (e < ne) d[e] = pr[e];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = v[e] * a * d[e] + z;
      }
    }
    Epilogue<T>::store(j, i0, v, 1.f);      // (rows / columns behind the problem: nothing is written)
  }
};

// ---- what the kernel takes --------------------------------------------------------------------------------------------------------------
static bool modconv_geom_ok(const sg_conv_fwd_desc* d) {
  if (d->R != d->S || (d->R != 1 && d->R != 3)) return false;
  if (d->pad_h != d->pad_w || d->pad_h < 0) return false;
  if (d->pix_flags & ~SG_PIX_TRANSPOSED) return false;
  const int k = d->R, p = d->pad_h;
  if (d->pix_flags & SG_PIX_TRANSPOSED) {       // gather form of the stride-2 transposed convolution (up = 2)
    if (d->stride != 2 || k != 3 || p > 2) return false;
    return d->Ho == (d->Hs - 1) * 2 + k - 2 * p && d->Wo == (d->Ws - 1) * 2 + k - 2 * p;
  }
  if (d->stride == 1) return p == k / 2 && d->Ho == d->Hs && d->Wo == d->Ws;
  if (d->stride == 2) {                         // its data gradient: a plain stride-2 convolution
    if (k != 3 || p > 1 || d->Hs + 2 * p < k || d->Ws + 2 * p < k) return false;
    return d->Ho == (d->Hs + 2 * p - k) / 2 + 1 && d->Wo == (d->Ws + 2 * p - k) / 2 + 1;
  }
  return false;
}
static bool modconv_ok(const sg_modconv_desc* m) {
  if (!m) return false;
  const sg_conv_fwd_desc* d = &m->conv;
  if (d->dtype != SG_DTYPE_F32 && d->dtype != SG_DTYPE_BF16) return false;
  if (d->N <= 0 || d->C <= 0 || d->Cout <= 0 || d->Hs <= 0 || d->Ws <= 0 || d->Ho <= 0 || d->Wo <= 0) return false;
  if (d->ldx < d->C || d->ldo < d->Cout) return false;
  if (d->epi_flags || d->mask || d->res) return false;
  if (!modconv_geom_ok(d)) return false;
  if ((long long)d->N * d->Ho * d->Wo >= (1ll << 31) || (long long)d->N * d->Hs * d->Ws * d->ldx >= (1ll << 31)) return false;
  if ((long long)d->R * d->S * d->C >= (1ll << 24)) return false;
  if (m->noise && m->noise_stride != 0 && m->noise_stride < (long long)d->Ho * d->Wo) return false;
  return true;
}
extern "C" int sg_modconv2d_ok(const sg_modconv_desc* m) { return modconv_ok(m) ? 1 : 0; }

static bool modconv_jvp_ok(const sg_modconv_jvp_desc* j) {
  if (!j || !modconv_ok(&j->m)) return false;
  const sg_conv_fwd_desc* d = &j->m.conv;
  if (!j->m.pre || !j->vs || !j->vx) return false;                    // both tables and both operands: the tangent of pre * x
  if (j->e && (!j->y || j->ldy < d->Cout)) return false;             // the demodulation term reads the stored result
  return true;
}
extern "C" int sg_modconv2d_jvp_ok(const sg_modconv_jvp_desc* j) { return modconv_jvp_ok(j) ? 1 : 0; }

// ---- one launcher for both entry points: p is the sg_modconv_desc, or with JVP the sg_modconv_jvp_desc that holds one ---------------------------------
template <bool JVP> using modconv_desc_t = std::conditional_t<JVP, sg_modconv_jvp_desc, sg_modconv_desc>;
static const sg_modconv_desc* forward_desc(const sg_modconv_desc* m) { return m; }
static const sg_modconv_desc* forward_desc(const sg_modconv_jvp_desc* j) { return &j->m; }

template <typename T, bool FAST, bool JVP>
static void modconv_launch(const modconv_desc_t<JVP>* p, int I, int J, int K, hipStream_t st) {
  const sg_modconv_desc* m = forward_desc(p);
  const sg_conv_fwd_desc* d = &m->conv;
  typedef StridedKC<T, FAST> LP;
  typedef ModPixKC<T, FAST, JVP> LQ;
  typedef ModEpilogue<T, JVP> EP;
  LP lp;
  lp.base = (const T*)d->w; lp.bstride = 0; lp.ld = K; lp.rows = I; lp.K = K;
  lp.vec_ok = (K % ET<T>::VEC == 0) && aligned16(d->w);
  LQ lq;
  fill_geom<T>(lq.b.g, d->x, d->N, d->Hs, d->Ws, d->C, d->ldx, d->Ho, d->Wo, d->R, d->S, d->stride, d->pad_h, d->pad_w, d->pix_flags);
  lq.b.rows = J; lq.b.K = K; lq.pre = m->pre;
  EP e;
  static_cast<Epilogue<T>&>(e) = make_epilogue<T>(d, I, J);
  e.post = m->post; e.noise = m->noise; e.noise_stride = m->noise_stride; e.HW = d->Ho * d->Wo;
  if constexpr (JVP) {
    fill_geom<T>(lq.bv.g, p->vx, d->N, d->Hs, d->Ws, d->C, d->ldx, d->Ho, d->Wo, d->R, d->S, d->stride, d->pad_h, d->pad_w, d->pix_flags);
    lq.bv.rows = J; lq.bv.K = K; lq.vs = p->vs;
    e.e = p->e; e.y = (const T*)p->y; e.ldy = p->ldy;
    if (!p->e) e.noise = nullptr;      // the noise enters through e * (y - noise) alone
    e.tab_vec = (I % 4 == 0) && (!m->post || aligned16(m->post)) && (!p->e || aligned16(p->e));
  } else {
    e.tab_vec = m->post && (I % 4 == 0) && aligned16(m->post);
  }
  // The generic engine's tile table, exact fp32 MFMA. The tangent in bf16: without its 96 x 256 tile -- with the second operand chunk and the second table in
  // flight that instantiation needs 280 VGPRs + 96 AGPRs and spills 448 bytes (profiles/modconv_jvp_resources.txt); a ragged cout tile of 128 x 128 costs idle
  // MFMA rows, not scratch traffic in the k-loop.
  if constexpr (!JVP || sizeof(T) == 4) conv_fwd_tiles<T, LP, LQ, 0, EP>(lp, lq, e, I, J, K, st);
  else if (I <= 32) sg_launch_gemm<T, LP, LQ, 32, 256, 1, 4, true, 0, EP>(lp, lq, e, I, J, K, 1, 1, st);
  else sg_launch_gemm<T, LP, LQ, 128, 128, 2, 2, true, 0, EP>(lp, lq, e, I, J, K, 1, 1, st);
}

template <typename T, bool JVP> static int modconv_t(const modconv_desc_t<JVP>* p, hipStream_t st) {
  const sg_modconv_desc* m = forward_desc(p);
  const sg_conv_fwd_desc* d = &m->conv;
  const int K = d->R * d->S * d->C, I = d->Cout, J = d->N * d->Ho * d->Wo;
  const bool w_vec = (K % ET<T>::VEC == 0) && aligned16(d->w);
  bool x_vec = (d->C % ET<T>::VEC == 0) && (d->ldx % ET<T>::VEC == 0) && aligned16(d->x) && (!m->pre || aligned16(m->pre));
  double x_reads = 1.0, out_passes = 1.0;      // what the tangent moves more: the second operand, and y wherever e is given
  if constexpr (JVP) {
    x_vec = x_vec && aligned16(p->vx) && aligned16(p->vs);
    x_reads = 2.0; out_passes = p->e ? 2.0 : 1.0;
  }
  const int prof = sg_prof_begin(st, 2.0 * (double)I * (double)J * (double)K, 0);
  if (w_vec && x_vec) modconv_launch<T, true, JVP>(p, I, J, K, st);
  else modconv_launch<T, false, JVP>(p, I, J, K, st);
  sg_prof_tag(prof, SG_ENG_CONV_GEMM, (double)sizeof(T) * (x_reads * (double)d->N * d->Hs * d->Ws * d->C + (double)I * K + out_passes * (double)J * I));
  sg_prof_end(st, prof);
  SG_LAUNCH_CHECK();
  __atomic_fetch_add(JVP ? &g_modconv_jvp_launches : &g_modconv_launches, 1, __ATOMIC_RELAXED);
  return 0;
}

extern "C" int sg_modconv2d_fwd(const sg_modconv_desc* m, sg_stream_t stream) {
  SG_CHECK(m && m->conv.x && m->conv.w && m->conv.out, "sg_modconv2d_fwd: null pointer");
  SG_CHECK(modconv_ok(m), "sg_modconv2d_fwd: problem not served (ask sg_modconv2d_ok first): fp32 / bf16; 1x1 or 3x3 at stride 1 and pad k/2, the 3x3 stride-2 "
                          "transposed gather, or the plain 3x3 stride-2 convolution; no mask / residual / epilogue flags");
  if (m->conv.dtype == SG_DTYPE_F32) return modconv_t<float, false>(m, (hipStream_t)stream);
  return modconv_t<bf16_t, false>(m, (hipStream_t)stream);
}
extern "C" int sg_modconv2d_jvp(const sg_modconv_jvp_desc* j, sg_stream_t stream) {
  SG_CHECK(j && j->m.conv.x && j->m.conv.w && j->m.conv.out && j->vx && j->vs && j->m.pre, "sg_modconv2d_jvp: null pointer");
  SG_CHECK(modconv_jvp_ok(j), "sg_modconv2d_jvp: problem not served (ask sg_modconv2d_jvp_ok first): sg_modconv2d_fwd's problems with both tables, both "
                              "operands, and the stored result wherever e is given");
  if (j->m.conv.dtype == SG_DTYPE_F32) return modconv_t<float, true>(j, (hipStream_t)stream);
  return modconv_t<bf16_t, true>(j, (hipStream_t)stream);
}

// ---- demodulation coefficients: Q[o][c] = sum_{r,s} W[o][c][r][s]^2,  d[n][o] = ( sum_c s[n][c]^2 Q[o][c] + 1e-8 )^(-1/2), all fp32 ------------
__global__ __launch_bounds__(256) void k_modconv_q(const float* __restrict__ w, float* __restrict__ Q, long long n, int RS) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float a = 0.f;
  for (int t = 0; t < RS; t++) { const float v = w[i * RS + t]; a += v * v; }
  Q[i] = a;
}
// one wave per (n, o); four per workgroup
__global__ __launch_bounds__(256) void k_modconv_d(const float* __restrict__ s, const float* __restrict__ Q, float* __restrict__ d, int N, int C, int Cout) {
  const int lane = threadIdx.x & 63;
  const long long idx = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (idx >= (long long)N * Cout) return;
  const int n = (int)(idx / Cout), o = (int)(idx - (long long)n * Cout);
  const float* sr = s + (long long)n * C;
  const float* qr = Q + (long long)o * C;
  float a = 0.f;
  for (int c = lane; c < C; c += 64) { const float v = sr[c]; a += v * v * qr[c]; }
  a = wave_sum(a);
  if (lane == 0) d[idx] = rsqrtf(a + 1e-8f);
}
extern "C" int sg_modconv_dcoef(const float* w, const float* s, float* Q, float* d, int N, int C, int Cout, int RS, sg_stream_t stream) {
  SG_CHECK(w && Q && C > 0 && Cout > 0 && RS > 0, "sg_modconv_dcoef: bad arguments");
  SG_CHECK((s == nullptr) == (d == nullptr) && (!s || N > 0), "sg_modconv_dcoef: styles and d come together");
  hipStream_t st = (hipStream_t)stream;
  const long long n = (long long)Cout * C;
  hipLaunchKernelGGL(k_modconv_q, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, w, Q, n, RS);
  if (s) {
    const long long rows = (long long)N * Cout;
    hipLaunchKernelGGL(k_modconv_d, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, s, Q, d, N, C, Cout);
  }
  SG_LAUNCH_CHECK();
  return 0;
}

// ---- backward reductions: one pass over a pair of [N][P][C] tensors ------------------------------------------------------------------------
//   out[n,p,c]     = scale[n,c] * a[n,p,c]                       (activation dtype; scale == nullptr: not written)
//   part[n,k,c]    = sum_{p in slab k} a[n,p,c] * ( b[n,p,c] - rowsub[n,p] )      (fp32; b == nullptr: not written)
//   rowsum[n,p]    = sum_c a[n,p,c]                              (fp32; nullptr: not written)
// With (a, b, rowsub, scale) = (gy, y, noise, d): gu, the slabs of sum_p gy * (y - noise) = d * gd, and gnoise.
// With (a, b, scale) = (gxs, x, styles): dx and the slabs of ds_direct. The caller sums part over its nslab slabs (a fixed order: no float atomics).
// A wave walks the pixels of its slab; a lane owns the channels lane, lane + 64, ... and their accumulators in LDS ([wave][C]: its own addresses).
template <typename T>
__global__ __launch_bounds__(256) void k_modconv_reduce(const T* __restrict__ a, const T* __restrict__ b, const float* __restrict__ rowsub, long long rowsub_stride,
                                                        const float* __restrict__ scale, T* __restrict__ out, float* __restrict__ part,
                                                        float* __restrict__ rowsum, int P, int C, int lda, int ldb, int slab) {
  extern __shared__ float sacc[];      // [4][C]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.y, k = blockIdx.x, nslab = gridDim.x;
  const int p0 = k * slab, p1 = (p0 + slab < P) ? p0 + slab : P;
  float* acc = sacc + wave * C;
  if (b) for (int c = lane; c < C; c += 64) acc[c] = 0.f;
  const float* sc = scale ? scale + (long long)n * C : nullptr;
  for (int p = p0 + wave; p < p1; p += 4) {
    const long long row = (long long)n * P + p;
    const T* ar = a + row * lda;
    const T* br = b ? b + row * ldb : nullptr;
    const float z = rowsub ? rowsub[(long long)n * rowsub_stride + p] : 0.f;
    float rs = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float g = to_f<T>(ar[c]);
      if (sc) out[row * C + c] = from_f<T>(sc[c] * g);
      if (br) acc[c] += g * (to_f<T>(br[c]) - z);
      rs += g;
    }
    if (rowsum) { rs = wave_sum(rs); if (lane == 0) rowsum[row] = rs; }
  }
  if (!b) return;
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256)
    part[((long long)n * nslab + k) * C + c] = (sacc[c] + sacc[C + c]) + (sacc[2 * C + c] + sacc[3 * C + c]);
}
// slabs the reduction cuts P pixels into (the caller sizes part[N][nslab][C] with it)
extern "C" int sg_modconv_reduce_slabs(int P) {
  if (P <= 0) return 0;
  const int slab = P > 64 * 64 ? (P + 63) / 64 : 64;
  return (P + slab - 1) / slab;
}
extern "C" int sg_modconv_reduce(int dtype, const void* a, const void* b, const float* rowsub, long long rowsub_stride, const float* scale, void* out, float* part,
                                 float* rowsum, int N, int P, int C, int lda, int ldb, sg_stream_t stream) {
  SG_CHECK(a && N > 0 && P > 0 && C > 0 && lda >= C && (!b || ldb >= C), "sg_modconv_reduce: bad arguments");
  SG_CHECK((scale == nullptr) == (out == nullptr) && (b == nullptr) == (part == nullptr), "sg_modconv_reduce: scale / out and b / part come in pairs");
  SG_CHECK(!rowsub || b, "sg_modconv_reduce: rowsub without b");
  SG_CHECK(C <= 4096 && N <= 65535, "sg_modconv_reduce: at most 4096 channels, 65535 samples");
  const int nslab = sg_modconv_reduce_slabs(P), slab = (P + nslab - 1) / nslab;
  const dim3 grid(nslab, N);
  const size_t lds = b ? (size_t)16 * C : 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SG_DTYPE_F32)
    hipLaunchKernelGGL(k_modconv_reduce<float>, grid, dim3(256), lds, st, (const float*)a, (const float*)b, rowsub, rowsub_stride, scale, (float*)out, part, rowsum, P, C, lda, ldb, slab);
  else if (dtype == SG_DTYPE_BF16)
    hipLaunchKernelGGL(k_modconv_reduce<bf16_t>, grid, dim3(256), lds, st, (const bf16_t*)a, (const bf16_t*)b, rowsub, rowsub_stride, scale, (bf16_t*)out, part, rowsum, P, C, lda, ldb, slab);
  else { sg_set_error("sg_modconv_reduce: bad dtype"); return -1; }
  SG_LAUNCH_CHECK();
  return 0;
}
