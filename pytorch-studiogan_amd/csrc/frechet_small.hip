// frechet_small.hip -- the Frechet distance of MANY small sample sets in one go (intra-class FID; a quick FID on 1-2 k samples), fp64 on fp32 features.
// linalg.hip needs symmetric positive definite covariances; a class of n < d samples has none, and the reference's route (scipy.linalg.sqrtm of a d x d
// product, src/metrics/fid.py:34-62) costs ~10 s of host time per class. With the centred rows A = (X1 - mu1) / sqrt(n1 - 1), B = (X2 - mu2) / sqrt(n2 - 1):
//     S1 = A^T A,  S2 = B^T B,  eig(S1 S2) \ {0} = sigma_i(A B^T)^2    =>    tr sqrtm(S1 S2) = |A B^T|_*  (nuclear norm of an n1 x n2 matrix),
//     tr S1 = |A|_F^2,  tr S2 = |B|_F^2,
// so no d x d matrix is ever formed. Segments are class-sorted row ranges of one feature matrix [rows][C]: segment k = rows seg[k] .. seg[k + 1].
//   sg_seg_moments       per segment the mean and tr S = sum |x - mu|^2 / (n - 1) (second, centred pass: no cancellation)
//   sg_seg_cross_gram    per class M_k = (A_k B_k^T), the SMALLER set along the rows (r <= c; ties: a), written at M + moff[k]: a ragged batched GEMM over
//                        k = C, one flat grid of exactly the 64 x 64 tiles that exist (host-built table, bisection in the kernel, as sn.hip). The rows are
//                        centred while they are staged into LDS: no fp64 copy of the features exists.
//                        Arithmetic: fp64 FMA tiles (the body of linalg.hip k_dgemm_tn), not v_mfma_f64_16x16x4_f64. The product is not the bottleneck
//                        of this path (1000 classes x 50 x 50 x 2048 is 10 GFLOP, the 10 x 1000 x 1000 x 2048 case 41 GFLOP, against Jacobi sweeps and a
//                        feature extractor in front of it), every tile spends as much on converting and centring fp32 rows as on the contraction, and
//                        the FMA form keeps k_dgemm_tn's fixed summation order and its parity record; the matrix pipe would buy nothing measurable.
//   sg_seg_nuclear_norm  one workgroup per matrix, the matrix resident in LDS, ALL one-sided Jacobi sweeps in the kernel (linalg.hip pays n - 1 launches
//                        and one host read-back per sweep: right for one 2048 x 2048 matrix, hopeless for 1000 matrices of 50 x 50). Tournament of
//                        k_jacobi_round; an odd row count gets a zero row in LDS. A row pair is rotated by one 32-lane half wave (8 pairs in flight per
//                        workgroup, disjoint within a round), one barrier per round.
//                        LDS banking: a half wave walks a row contiguously, 8 bytes per lane. ds_read_b64 resolves banks per 32-lane half over 64 dword
//                        banks, so 32 adjacent doubles are conflict-free at ANY row pitch and the two halves of a wave never meet: the rows need no
//                        padding, and the pitch is the column count. (Padding is what a column walk would need; nothing here walks a column.)
//   sg_seg_nuclear_fits  1 when rows x cols takes the LDS route. Budget: FS_LDS_BUDGET = 128 KiB of the CU's 160 KiB per workgroup, i.e.
//                        8 * (re * cols + re + 16) bytes with re = rows rounded up to even: everything up to 126 x 126 (64 x 64 takes 33 KiB, 50 x 50
//                        21 KiB: 7 matrices per CU). Larger matrices are the caller's: padded to an even square for sg_jacobi_sweep / sg_row_norm_sum.
// seg / moff / rows / cols are HOST arrays: small tables the host owns anyway (it sizes M from them); they reach the kernels by value, in chunks.
#include "common.h"
#include "lds_tile.h"
#include "../../include/sgamd.h"

#define FS_LDS_BUDGET (128 * 1024)
#define FS_SEGS 256       // segments per sg_seg_moments launch      (table 3 KiB of kernel arguments)
#define FS_GCLS 80        // classes per sg_seg_cross_gram launch    (table 2.9 KiB)
#define FS_NMAT 200       // matrices per sg_seg_nuclear_norm launch (table 3.1 KiB)

struct fs_seg_tab { int n, k0; long long r0[FS_SEGS]; int rows[FS_SEGS]; };
struct fs_gram_tab {
  int n, k0;                      // classes of this launch; index of the first one (rows of mu)
  int start[FS_GCLS + 1];         // first tile of each class in the flat grid
  int nr[FS_GCLS], nc[FS_GCLS];   // rows / columns of M_k
  long long r0[FS_GCLS], c0[FS_GCLS], moff[FS_GCLS];   // first feature row of the row set / the column set; offset of M_k in doubles
  unsigned char swap[FS_GCLS];    // 1: the row set is b
};
struct fs_nuc_tab { int n, k0; long long moff[FS_NMAT]; int rows[FS_NMAT], cols[FS_NMAT]; };

// one workgroup per segment; a thread owns columns t, t + 256, ...: sum, then the centred squares
__global__ __launch_bounds__(256) void k_seg_moments(const float* f, int C, double* mu, double* tr, const fs_seg_tab T) {
  __shared__ double sm[4];
  const int k = blockIdx.x, n = T.rows[k];
  const float* x = f + T.r0[k] * C;
  double* m = mu + (long long)(T.k0 + k) * C;
  double acc = 0.0;
  for (int c = threadIdx.x; c < C; c += 256) {
    double s = 0.0;
    for (int r = 0; r < n; r++) s += (double)x[(long long)r * C + c];
    const double mean = s / (double)n;
    double q = 0.0;
    for (int r = 0; r < n; r++) { const double d = (double)x[(long long)r * C + c] - mean; q += d * d; }
    m[c] = mean;
    acc += q;
  }
  acc = block_sum_256_d(acc, sm);
  if (threadIdx.x == 0) tr[T.k0 + k] = acc / (double)(n - 1);
}

extern "C" int sg_seg_moments(const float* f, const long long* seg, int K, int C, double* mu, double* tr, sg_stream_t s) {
  SG_CHECK(f && seg && mu && tr && K > 0 && C > 0, "sg_seg_moments: bad args");
  for (int k = 0; k < K; k++) SG_CHECK(seg[k] >= 0 && seg[k + 1] - seg[k] >= 2 && seg[k + 1] - seg[k] < (1ll << 31), "sg_seg_moments: a segment needs at least 2 rows");
  for (int k0 = 0; k0 < K; k0 += FS_SEGS) {
    fs_seg_tab T;
    T.n = K - k0 < FS_SEGS ? K - k0 : FS_SEGS;
    T.k0 = k0;
    for (int i = 0; i < T.n; i++) { T.r0[i] = seg[k0 + i]; T.rows[i] = (int)(seg[k0 + i + 1] - seg[k0 + i]); }
    hipLaunchKernelGGL(k_seg_moments, dim3(T.n), dim3(256), 0, (hipStream_t)s, f, C, mu, tr, T);
  }
  SG_LAUNCH_CHECK();
  return 0;
}

// M_k[i][j] = <row_i - mu_r, col_j - mu_c> / sqrt((nr - 1)(nc - 1)); 64 x 64 tile per block, 4 x 4 per thread, k-tiles of 16 (k_dgemm_tn's body).
// LDS rows of 68 doubles: the staging writes of a wave (16 k x 4 rows, transposed into [k][row]) spread over the banks instead of landing on one column of
// them, and the 4-double reads stay 16-byte aligned.
__global__ __launch_bounds__(256) void k_seg_cross_gram(const float* fa, const double* mua, const float* fb, const double* mub, int C, double* M, const fs_gram_tab T) {
  __shared__ __attribute__((aligned(16))) double sa[16][68], sb[16][68];
  int li = 0, hi = T.n;
  while (hi - li > 1) { const int mid = (li + hi) >> 1; if ((int)blockIdx.x >= T.start[mid]) li = mid; else hi = mid; }
  const int nr = T.nr[li], nc = T.nc[li];
  const int tiles_x = (nc + 63) >> 6, local = blockIdx.x - T.start[li];
  const int ty = local / tiles_x, tx = local - ty * tiles_x;
  const int i0 = ty * 64, j0 = tx * 64;
  const bool sw = T.swap[li] != 0;
  const float* R = (sw ? fb : fa) + T.r0[li] * C;
  const float* Q = (sw ? fa : fb) + T.c0[li] * C;
  const double* mr = (sw ? mub : mua) + (long long)(T.k0 + li) * C;
  const double* mc = (sw ? mua : mub) + (long long)(T.k0 + li) * C;
  const int ta = threadIdx.x >> 4, tb = threadIdx.x & 15;
  double acc[4][4] = {};
  for (int k0 = 0; k0 < C; k0 += 16) {
    for (int e = threadIdx.x; e < 16 * 64; e += 256) {
      const int kk = e & 15, r = e >> 4;
      const int k = k0 + kk;
      sa[kk][r] = (k < C && i0 + r < nr) ? (double)R[(long long)(i0 + r) * C + k] - mr[k] : 0.0;
      sb[kk][r] = (k < C && j0 + r < nc) ? (double)Q[(long long)(j0 + r) * C + k] - mc[k] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; kk++) {
      double av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; i++) { av[i] = sa[kk][ta * 4 + i]; bv[i] = sb[kk][tb * 4 + i]; }
#pragma unroll
      for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] += av[i] * bv[j];
    }
    __syncthreads();
  }
  const double scale = 1.0 / sqrt((double)(nr - 1) * (double)(nc - 1));
  double* out = M + T.moff[li];
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int a = i0 + ta * 4 + i, b = j0 + tb * 4 + j;
      if (a < nr && b < nc) out[(long long)a * nc + b] = acc[i][j] * scale;
    }
}

extern "C" int sg_seg_cross_gram(const float* fa, const long long* sega, const double* mua, const float* fb, const long long* segb, const double* mub, int K, int C,
                                 double* M, const long long* moff, sg_stream_t s) {
  SG_CHECK(fa && sega && mua && fb && segb && mub && M && moff && K > 0 && C > 0, "sg_seg_cross_gram: bad args");
  for (int k = 0; k < K; k++) {
    const long long na = sega[k + 1] - sega[k], nb = segb[k + 1] - segb[k];
    SG_CHECK(sega[k] >= 0 && segb[k] >= 0 && na >= 2 && nb >= 2 && na < (1ll << 31) && nb < (1ll << 31) && moff[k] >= 0, "sg_seg_cross_gram: a class needs at least 2 rows on both sides");
  }
  int k0 = 0;
  while (k0 < K) {
    fs_gram_tab T;
    T.k0 = k0;
    T.start[0] = 0;
    int i = 0;
    for (; i < FS_GCLS && k0 + i < K; i++) {
      const int k = k0 + i;
      const int na = (int)(sega[k + 1] - sega[k]), nb = (int)(segb[k + 1] - segb[k]);
      const bool sw = nb < na;
      T.swap[i] = sw ? 1 : 0;
      T.nr[i] = sw ? nb : na; T.nc[i] = sw ? na : nb;
      T.r0[i] = sw ? segb[k] : sega[k]; T.c0[i] = sw ? sega[k] : segb[k];
      T.moff[i] = moff[k];
      const long long tiles = (long long)((T.nr[i] + 63) >> 6) * ((T.nc[i] + 63) >> 6);
      if (T.start[i] + tiles > (1ll << 30)) break;       // (a launch of its own for what follows)
      T.start[i + 1] = T.start[i] + (int)tiles;
    }
    SG_CHECK(i > 0, "sg_seg_cross_gram: a class too large for one grid");
    T.n = i;
    hipLaunchKernelGGL(k_seg_cross_gram, dim3(T.start[i]), dim3(256), 0, (hipStream_t)s, fa, mua, fb, mub, C, M, T);
    k0 += i;
  }
  SG_LAUNCH_CHECK();
  return 0;
}

static inline long long fs_lds_bytes(int rows, int cols) {
  const long long re = rows + (rows & 1);
  return 8 * (re * cols + re + 16);
}
extern "C" int sg_seg_nuclear_fits(int rows, int cols) { return rows >= 1 && cols >= 1 && fs_lds_bytes(rows, cols) <= FS_LDS_BUDGET ? 1 : 0; }
extern "C" int sg_seg_nuclear_lds_budget(void) { return FS_LDS_BUDGET; }

__device__ __forceinline__ double half_sum_d(double v) {      // sum over the 32 lanes of a half wave, in every lane of it
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// LDS: A[re][c] | nrm[re] | smax[2][8]. Half wave g of 8 rotates the pairs of slots g, g + 8, ... of a round; the pairs of a round are disjoint.
__global__ __launch_bounds__(256) void k_seg_nuclear(const double* M, int max_sweeps, double tol, double* nuc, double* offd, int* sweeps, const fs_nuc_tab T) {
  extern __shared__ __attribute__((aligned(16))) double fs_lds[];
  const int b = blockIdx.x, r = T.rows[b], c = T.cols[b];
  const int re = r + (r & 1), m = re - 1, half = re >> 1;
  double* A = fs_lds;
  double* nrm = A + re * c;
  double* smax = nrm + re;
  const double* src = M + T.moff[b];
  for (int e = threadIdx.x; e < re * c; e += 256) A[e] = e < r * c ? src[e] : 0.0;
  __syncthreads();
  const int g = threadIdx.x >> 5, l = threadIdx.x & 31;
  int sw = 0;
  double meas = 0.0;
  while (sw < max_sweeps) {
    double mx = 0.0;
    for (int round = 0; round < m; round++) {
      for (int s0 = 0; s0 < half; s0 += 8) {        // (uniform trip count: both half waves of a wave reach the shuffles together; a half wave without a pair idles)
        const int slot = s0 + g;
        const bool live = slot < half;
        int p = 0, q = 0;
        if (live) {
          if (slot == 0) { p = re - 1; q = round % m; }
          else { p = (round + slot) % m; q = (round - slot + m) % m; }
        }
        double* rp = A + p * c;
        double* rq = A + q * c;
        double a = 0.0, bb = 0.0, gg = 0.0;
        if (live)
          for (int j = l; j < c; j += 32) { const double x = rp[j], y = rq[j]; a += x * x; bb += y * y; gg += x * y; }
        a = half_sum_d(a); bb = half_sum_d(bb); gg = half_sum_d(gg);
        const double den = sqrt(a * bb);
        // A row of zero norm: nothing to rotate, and no NaN in the measure. The same holds for a row at the rounding level of its partner (|y| <= 2^-50 |x|): that is
        // what a rotation leaves of a row that was a MULTIPLE of its partner (two samples per class: the centred rows are x, -x, and M = [[d, -d], [-d, d]] exactly).
        // The remainder is again an exact multiple, the scale-free measure stays 1 however small it gets, every rotation shrinks it by 2^-53 until zeta^2 overflows
        // and the rotation angle rounds to 0: the measure would sit at 1 for good. Such a row adds less than 2^-50 |x| to the sum of the norms either way.
        const bool noise = fmin(a, bb) <= 7.888609052210118e-31 * fmax(a, bb);      // (2^-50)^2
        const double off = (den > 0.0 && !noise) ? fabs(gg) / den : 0.0;
        mx = fmax(mx, off);
        if (live && off > 1e-15 && gg != 0.0) {
          const double zeta = (bb - a) / (2.0 * gg);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
          for (int j = l; j < c; j += 32) {
            const double x = rp[j], y = rq[j];
            rp[j] = cs * x - sn * y;
            rq[j] = sn * x + cs * y;
          }
        }
      }
      __syncthreads();
    }
    double* sx = smax + (sw & 1) * 8;       // (two buffers: the next write to this one is two sweeps and many barriers away)
    if (l == 0) sx[g] = mx;
    __syncthreads();
    meas = sx[0];
#pragma unroll
    for (int i = 1; i < 8; i++) meas = fmax(meas, sx[i]);
    sw++;
    if (meas < tol) break;                  // (the same 8 values in every thread: uniform)
  }
  for (int r0 = 0; r0 < re; r0 += 8) {
    const int row = r0 + g;
    double a = 0.0;
    if (row < re)
      for (int j = l; j < c; j += 32) { const double x = A[row * c + j]; a += x * x; }
    a = half_sum_d(a);
    if (l == 0 && row < re) nrm[row] = sqrt(a);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int i = 0; i < re; i++) total += nrm[i];      // fixed order
    nuc[T.k0 + b] = total;
    offd[T.k0 + b] = meas;
    sweeps[T.k0 + b] = sw;
  }
}

extern "C" int sg_seg_nuclear_norm(const double* M, const long long* moff, const int* rows, const int* cols, int K, int max_sweeps, double tol,
                                   double* nuc, double* offd, int* sweeps, sg_stream_t s) {
  SG_CHECK(M && moff && rows && cols && nuc && offd && sweeps && K > 0 && max_sweeps >= 1, "sg_seg_nuclear_norm: bad args");
  for (int k = 0; k < K; k++) SG_CHECK(moff[k] >= 0 && sg_seg_nuclear_fits(rows[k], cols[k]), "sg_seg_nuclear_norm: a matrix beyond the LDS budget (ask sg_seg_nuclear_fits first)");
  static const bool ok = lt_allow_lds(k_seg_nuclear, FS_LDS_BUDGET);
  SG_CHECK(ok, "sg_seg_nuclear_norm: LDS attribute");
  for (int k0 = 0; k0 < K; k0 += FS_NMAT) {
    fs_nuc_tab T;
    T.n = K - k0 < FS_NMAT ? K - k0 : FS_NMAT;
    T.k0 = k0;
    long long lds = 0;
    for (int i = 0; i < T.n; i++) {
      T.moff[i] = moff[k0 + i]; T.rows[i] = rows[k0 + i]; T.cols[i] = cols[k0 + i];
      const long long need = fs_lds_bytes(rows[k0 + i], cols[k0 + i]);
      if (need > lds) lds = need;
    }
    hipLaunchKernelGGL(k_seg_nuclear, dim3(T.n), dim3(256), (size_t)lds, (hipStream_t)s, M, max_sweeps, tol, nuc, offd, sweeps, T);
  }
  SG_LAUNCH_CHECK();
  return 0;
}
