// conv_v3.h -- "halo" forward / data-gradient kernel for 3x3 stride-1 pad-1 convolutions (bf16, >= 64 input channels).
//
// conv_v2.h stages one im2col k-tile per step: for a 3x3 filter every input pixel of the tile travels L2 -> LDS nine times
// (once per tap), and with two LDS buffers only ONE k-tile of DMA is ever in flight -- the k-loop runs at
// (bytes in flight) / (memory latency), ~40 KB/us per CU, far below what the MFMAs could consume on the <= 192-channel layers.
// Here the pixel operand is staged ONCE per 64-channel slice as a PATCH: the tile's pixels plus one image row (+1 pixel) of
// halo on either side, in raster order, [pixel][64 channels] = 128-byte rows with the same source-side XOR swizzle as conv_v2.
// The nine taps then read their MFMA fragments from the same patch at SHIFTED row indices (row + (tr-1)*W + (ts-1)); pixels
// outside the image are redirected to a zero line. Only the weight tile (BI x 64) is streamed per tap. L2 -> LDS bytes per
// (tile, slice): patch (BJ + 2W + 16) * 128 + 9 * BI * 128   instead of   9 * (BJ + BI) * 128   (1.9x fewer on 192 -> 192 @64^2,
// 3.3x fewer on 96 -> 96 @128^2), and the next slice's patch is in flight during all nine taps of the current one.
//
//   * raster row order: patch row of tile pixel p, tap (tr,ts) = (p - j0) + W + 8 + (tr-1)*W + (ts-1)
//   * quad row order (2x2 pooling epilogue): same patch (the tile still covers BJ/W whole image rows), per-lane row base
//   * nearest x2 upsample on load: the patch holds SOURCE pixels (4x fewer); row = base + ((ph+tr-1)>>1)*Ws + ((pw+ts-1)>>1)
//   * fragment addresses: (row << 7) | ((chunk ^ (row >> 1 & 7)) << 4): any 16 rows with distinct residues mod 16 are
//     conflict-free for ds_read_b128, so every shift is as good as the unshifted read
//   * epilogue: sg_conv_epilogue (conv_v2.h); pixel decode, border masks and the other pieces shared with conv_v4.h / conv_q.h: halo_tile.h
#pragma once
#include <type_traits>
#include "halo_tile.h"

struct ConvV3Params {
  const bf16_t* x; const bf16_t* w;
  int W;                  // source image width (Ws): power of two >= 4; patch halo = one source row + 8 pixels either side
  int wlog;               // log2(W)
  int C, ldx;
  int Ho, Wo, wshift, hshift;
  int flags;
  int I, J, K;
  int nslice;             // ceil(C / 64)
  int npix_src;           // N * Hs * Ws
  int npx;                // patch pixels = BJ(/4 with upsample) + 2 W + 16
  unsigned xbytes, wbytes;
  int zero_off, bias_off; // LDS byte offsets of the zero line / bias vector (behind the output staging area)
  int dump_off;           // 1 KiB of LDS that absorbs the DMA pieces a wave has no use for (see "branch-free DMA" below)
  int pm4, psh;           // image-row parity term of the chunk swizzle (quad row order, W >= 16; see conv_v4.h): chunk ^= ((pixel >> psh) & pm4), pm4 = 4 or 0
};

// W3: three weight buffers (PB2 only). The weights of tap t+1 are then complete and visible one barrier EARLIER than they are
// needed, so the first fragments of tap t+1 are requested before the barrier that ends tap t: the matrix pipe does not drain at
// every tap boundary while all eight waves sit behind the barrier and then queue for the LDS at once.
//
// NKL: 16-channel sub-steps of the LAST 64-channel slice -- 4 (C % 64 == 0), 2 (C % 64 == 32: the 96-channel layers) or 0 = decided at
// run time (any other C). Straight-line taps: with the sub-step count a run-time value and the DMA pieces behind wave-dependent
// branches, every tap was a chain of small basic blocks, and at each join the compiler's s_waitcnt insertion had to assume the
// shorter path: the MFMAs of sub-step k waited for the fragment loads of sub-step k + 1 that had just been issued in front of them
// (s_waitcnt lgkmcnt(1) / lgkmcnt(0) right before every group of MFMAs in the r02 disassembly) -- the register double buffer of the
// fragments bought nothing. Now the sub-step count is a compile-time constant per slice (the slice body is instantiated for 4 and
// for NKL) and the DMA is branch-free: every wave issues every piece of every tap; a piece it has no use for (cout rows beyond the
// tile, patch groups beyond the patch, the prefetch behind the last slice) goes, with an out-of-range source offset (zero fill,
// no memory traffic), to a 1 KiB dump area of LDS. A tap is one basic block and the compiler counts its own loads exactly.
template <int BI, int WJ, int WI, int BJ, bool RELU, bool UP, bool PB2, bool W3 = false, int NKL = 0>
__global__ __launch_bounds__(64 * WJ * WI) void sg_conv_v3_kernel(ConvV3Params p, Epilogue<bf16_t> epi, int tilesI, int tilesJ) {
  static_assert(!W3 || PB2, "W3 needs the double patch buffer");
  constexpr int NW = WJ * WI;
  constexpr int PB = BI * 128;                 // one weight tile (BI couts x 64 channels)
  constexpr int NPI = (BI / 8 + NW - 1) / NW;  // weight DMA pieces per wave per tap (upper bound)
  constexpr int TJ = BJ / WJ / 32, TI = BI / WI / 32;
  static_assert(NW == 8 || NW == 4, "8 waves (2 per SIMD) or 4 waves (1 per SIMD, 512 registers: 12-16 accumulator blocks per wave)");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bid = sg_xcd_tile(blockIdx.x, tilesI * tilesJ);
  const int tI = bid % tilesI, tJ = bid / tilesI;
  const int i0 = tI * BI, j0 = tJ * BJ;
  const int patch_bytes = p.npx * 128;
  char* const pbufs = smem + (PB2 ? 2 : 1) * patch_bytes;      // the weight buffers sit behind the patch buffer(s)
  float* sbias = (float*)(smem + p.bias_off);
  ht_stage_bias<BI, 64 * NW, false>(sbias, epi, nullptr, i0, tid);
  ht_zero_line(smem, p.zero_off, tid);

  const auto rsx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.xbytes, 0x00020000);
  const auto rsw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)p.wbytes, 0x00020000);
  const int sub = lane >> 3;
  const int lc = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);       // logical 16-byte chunk this lane fetches (DMA group g: key = 4g + sub/2)
  const unsigned ldx2 = 2u * (unsigned)p.ldx;

  // ---- patch DMA: groups of 8 consecutive source pixels, group g = wave + 8 i ----------------------------------------------
  const int P0 = (UP ? (j0 >> 2) : j0) - p.W - 8;                    // raster index of patch row 0
  const int ngroups = p.npx >> 3;
  const int npw = (ngroups - wave + NW - 1) / NW;                    // groups of this wave (wave-uniform)
  const int pix0 = P0 + 8 * wave + sub;                              // this lane's pixel in group i = 0
  const unsigned poff0 = (unsigned)pix0 * ldx2 + (unsigned)lc * 16u;
  const unsigned pstep = 8u * NW * ldx2;
  // slice s: channel chunk lc of the slice exists when s*64 + lc*8 < C
  char* const dump = smem + p.dump_off;
  auto patch_piece = [&](int buf, int s, int i, bool en) {           // en: wave-uniform; false = the piece goes to the dump area
    const int pix = pix0 + 8 * NW * i;
    unsigned off = poff0;
    asm volatile("" : "+v"(off));     // (same: one live address per piece in flight, not one per piece of the slice)
    off += (unsigned)i * pstep + (unsigned)s * 128u;
    const int lce = lc ^ ((pix >> p.psh) & p.pm4);                  // quad row order: the image-row parity joins the swizzle key
    off += (unsigned)((lce - lc) * 16);
    const bool ok = en && ((unsigned)pix < (unsigned)p.npix_src) && (s * 64 + lce * 8 < p.C);
    off = ok ? off : 0x80000000u;
    char* dst = en ? smem + buf * patch_bytes + (wave + NW * i) * 1024 : dump;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (sg_lptr_t)dst, 16, (int)off, 0, 0, 0);
  };

  // ---- weight DMA: BI rows x 64 channels of tap t, slice s ------------------------------------------------------------------
  unsigned woff[NPI];
#pragma unroll
  for (int i = 0; i < NPI; i++) {
    const int g = wave + NW * i;
    const int row = i0 + 8 * g + sub;
    woff[i] = ((g < BI / 8) && (row < p.I)) ? (unsigned)row * (unsigned)p.K * 2u : 0x40000000u;
  }
  auto weight_piece = [&](int buf, int s, int t, int j, bool en) {
    const unsigned kw = (en && s * 64 + lc * 8 < p.C) ? (unsigned)((t * p.C + s * 64 + lc * 8) * 2) : 0x40000000u;   // 2^30 (+ 2^30) >= wbytes: zero fill
    en = en && (NW * (j + 1) <= BI / 8 || wave + NW * j < BI / 8);
    char* dst = en ? pbufs + buf * PB + (wave + NW * j) * 1024 : dump;
    unsigned wo = woff[j];
    asm volatile("" : "+v"(wo));
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (sg_lptr_t)dst, 16, (int)(wo + kw), 0, 0, 0);
  };
  auto weight_tile = [&](int buf, int s, int t) {
#pragma unroll
    for (int j = 0; j < NPI; j++) weight_piece(buf, s, t, j, true);
  };

  // ---- fragment rows of this lane ---------------------------------------------------------------------------------------------
  const int wj = wave % WJ, wi = wave / WJ;
  const int wj0 = wj * (BJ / WJ), wi0 = wi * (BI / WI);
  const int frow = lane & 31, fhi = lane >> 5;
  int rb[TJ];             // patch row of the centre pixel
  unsigned qinv[TJ];      // bit t set = tap t reads outside the image (or the row is outside the problem)
  int rs0[TJ], rs2[TJ], cs0[TJ], cs2[TJ];   // row / column displacement of taps tr = 0, 2 and ts = 0, 2 (tr = ts = 1: none)
#pragma unroll
  for (int b = 0; b < TJ; b++) {
    const int row = j0 + wj0 + b * 32 + frow;
    int n, ho, wo;
    ht_decode_pixel(p, row, n, ho, wo);
    qinv[b] = ~ht_border_mask(ho, wo, p.Ho, p.Wo, row < p.J);
    rb[b] = ht_patch_row<UP>(p, n, ho, wo, P0);
    if (UP) {
      rs0[b] = (ho & 1) ? 0 : -p.W; rs2[b] = (ho & 1) ? p.W : 0;
      cs0[b] = (wo & 1) ? 0 : -1;  cs2[b] = (wo & 1) ? 1 : 0;
    } else {
      rs0[b] = -p.W; rs2[b] = p.W; cs0[b] = -1; cs2[b] = 1;
    }
  }

  f32x16 acc[TI][TJ];
  ht_zero_acc(acc);

  const int nslice = p.nslice;
  // sub-steps of the last slice when NKL == 0 (run-time): a 96-channel layer's second slice is half empty, and running its zero
  // half cost 25 % of the layer's MFMAs and fragment reads
  const int crem_last = p.C - (nslice - 1) * 64;
  const int nks_last_rt = crem_last >= 64 ? 4 : ((crem_last + 15) >> 4);

  // Two weight-buffer schemes share the tap below. What differs:
  //   two buffers (!W3):  buffer of step (9 s + t) = step & 1; the DMA runs ONE tap ahead; a tap loads its own sub-step 0 at its head;
  //   three buffers (W3): buffer of tap t = t % 3; the DMA runs TWO taps ahead; sub-step 0 of tap t + 1 is loaded in front of the barrier that ends tap t
  //                       (fragments one sub-step ahead ACROSS taps; its weights were complete at the PREVIOUS barrier, the next slice's patch at barrier 7).
  constexpr int LA = W3 ? 2 : 1;                   // taps of weight lookahead
  constexpr int NPT = W3 ? 8 : 9;                  // taps of a slice that carry a share of the next slice's patch
  struct Frags {
    bf16x8_t pf[2][TI], qf[2][TJ];                 // register double buffer of the fragments, one sub-step ahead
    unsigned qa[TJ];                               // pixel-fragment byte offsets (from smem) of the tap whose sub-step 0 is loaded next
  };
  auto tap_addresses = [&](Frags& f, int t, int poff) {      // t: compile-time tap; poff: byte offset of the slice's patch buffer
    const int tr = t / 3, ts = t % 3;
#pragma unroll
    for (int b = 0; b < TJ; b++) {
      int row = rb[b];
      asm volatile("" : "+v"(row));   // keeps the nine taps' address arithmetic inside their taps (hoisted out of the slice loop it spilled)
      if (tr == 0) row += rs0[b];
      if (tr == 2) row += rs2[b];
      if (ts == 0) row += cs0[b];
      if (ts == 2) row += cs2[b];
      const int ipar = ((row + P0) >> p.psh) & p.pm4;
      unsigned a = (unsigned)poff + (((unsigned)row << 7) | ((unsigned)((fhi ^ (row >> 1) ^ ipar) & 7) << 4));
      a = ((qinv[b] >> t) & 1u) ? (unsigned)p.zero_off : a;
      f.qa[b] = a;
    }
  };
  auto load = [&](Frags& f, int ks, int slot, const char* ps) {
#pragma unroll
    for (int a = 0; a < TI; a++) {
      const int row = wi0 + a * 32 + frow;
      const int ch = (ks * 2 + fhi) ^ ((row >> 1) & 7);
      u32x4 v = *(const u32x4*)(ps + row * 128 + ch * 16);
      f.pf[slot][a] = __builtin_bit_cast(bf16x8_t, v);
    }
#pragma unroll
    for (int b = 0; b < TJ; b++) {
      u32x4 v = *(const u32x4*)(smem + (f.qa[b] ^ (unsigned)(ks * 32)));
      if (RELU) v = relu16<bf16_t>(v);
      f.qf[slot][b] = __builtin_bit_cast(bf16x8_t, v);
    }
  };

  // ---- prologue: patch of slice 0 and the weights of the first LA taps -------------------------------------------------------------
  for (int i = 0; i < npw; i++) patch_piece(0, 0, i, true);
  weight_tile(0, 0, 0);
  if constexpr (W3) weight_tile(1, 0, 1);
  __syncthreads();
  Frags carried;                                   // W3: fragments live across the tap boundary
  if constexpr (W3) { tap_addresses(carried, 0, 0); load(carried, 0, 0, pbufs); }
  const int ppt = W3 ? (npw + 7) >> 3 : (npw + 8) / 9;   // patch pieces of the next slice issued per tap (PB2; <= 2: launcher)
  auto run_slice = [&](int s, auto nkc) __attribute__((always_inline)) {
    constexpr int NKC = decltype(nkc)::value;      // sub-steps of this slice; 0: run-time
    const int nks = NKC ? NKC : nks_last_rt;
    const bool next_slice = s + 1 < nslice;
    const int poff_cur = (PB2 ? (s & 1) : 0) * patch_bytes, poff_nxt = ((s + 1) & 1) * patch_bytes;
    const int step0 = 9 * s;
#pragma unroll
    for (int t = 0; t < 9; t++) {
      const int wb = W3 ? t % 3 : (step0 + t) & 1;                   // weight buffer of this tap
      const int wbn = W3 ? (t + LA) % 3 : (step0 + t + 1) & 1;       // ... and of the tap LA ahead (as wb ^ 1 the two-buffer kernels took 2-4 registers more)
      const char* ps = pbufs + wb * PB;
      // prefetch: DMA piece k of this tap: k < NPI = piece k of the weights LA taps ahead; k = NPI, NPI + 1 = a share (<= 2 pieces: launcher) of the
      // next slice's patch
      auto dma_piece = [&](int k) {
        if (k < NPI) {
          if (t + LA < 9) weight_piece(wbn, s, t + LA, k, true);
          else weight_piece(wbn, s + 1, t + LA - 9, k, next_slice);
        } else if (PB2 && t < NPT) {
          const int i = t * ppt + (k - NPI);
          patch_piece((s + 1) & 1, s + 1, i, next_slice && (k - NPI) < ppt && i < npw);
        }
      };
      Frags own;                                 // two buffers: a tap's fragments live inside the tap (declared outside it they cost 20 registers)
      Frags& f = W3 ? carried : own;
      if constexpr (!W3) { tap_addresses(f, t, poff_cur); load(f, 0, 0, ps); }
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        if (ks < 3 && ks + 1 < nks) load(f, ks + 1, (ks + 1) & 1, ps);
        if (ks < nks) {
#pragma unroll
          for (int a = 0; a < TI; a++)
#pragma unroll
            for (int b = 0; b < TJ; b++) {
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.pf[ks & 1][a], f.qf[ks & 1][b], acc[a][b], 0, 0, 0);
              // a piece costs 60-180 issue cycles: one behind each of the first sub-step's MFMAs, where the matrix pipe is busy anyway
              if (ks == 0 && a * TJ + b < NPI + 2) {
                __builtin_amdgcn_sched_barrier(0);
                dma_piece(a * TJ + b);
                __builtin_amdgcn_sched_barrier(0);
              }
            }
          if (ks == 0) {   // fewer MFMAs in a sub-step than pieces: the rest behind the sub-step
#pragma unroll
            for (int k = TI * TJ; k < NPI + 2; k++) dma_piece(k);
          }
        }
        __builtin_amdgcn_sched_barrier(0);       // the scheduler keeps the software pipeline as written: fragments of sub-step k + 1, then the MFMAs
                                                 // of sub-step k (left alone it pulls the loads of several sub-steps to the tap's head and spills)
      }
      if constexpr (W3) {                        // sub-step 0 of the next tap
        if (t < 8) { tap_addresses(f, t + 1, poff_cur); load(f, 0, 0, pbufs + ((t + 1) % 3) * PB); }
        else if (next_slice) { tap_addresses(f, 0, poff_nxt); load(f, 0, 0, pbufs); }
      }
      __syncthreads();
    }
    if (!PB2 && next_slice) {                      // single patch buffer: the next slice's patch cannot overlap the taps
      for (int i = 0; i < npw; i++) patch_piece(0, s + 1, i, true);
      __syncthreads();
    }
  };
  if constexpr (NKL == 4) {
    for (int s = 0; s < nslice; s++) run_slice(s, std::integral_constant<int, 4>{});
  } else {                                         // last slice peeled (an if / else of the two bodies inside one loop spilled registers)
    for (int s = 0; s + 1 < nslice; s++) run_slice(s, std::integral_constant<int, 4>{});
    run_slice(nslice - 1, std::integral_constant<int, NKL>{});
  }

  float al = epi.alpha;
  if (epi.alpha_ptr) al *= *epi.alpha_ptr;
  // (the 32-cout tile -- the generator's RGB layer -- sits at a register boundary and has no use for sign planes: compiled without them, counted so in conv.hip)
  sg_conv_epilogue<BI, BJ, NW, TI, TJ, false, false, BI != 32>(acc, smem, sbias, epi, i0, j0, wi0, wj0, al);
}

// LDS layout and need (bytes) of a configuration, or -1 when it does not fit: [patch(es) | weight buffers], overlaid by the staged output tile; behind it
// the zero line, the bias vector and the DMA dump area
static inline int sg_conv_v3_lds(int BI, int BJ, int npx, bool pb2, bool w3 = false, int* zero_off = nullptr, int* bias_off = nullptr, int* dump_off = nullptr) {
  int body = (pb2 ? 2 : 1) * npx * 128 + (w3 ? 3 : 2) * BI * 128;
  const int stage = BJ * (BI * 2 + 16);
  if (stage > body) body = stage;
  if (zero_off) *zero_off = body;
  if (bias_off) *bias_off = body + 128;
  if (dump_off) *dump_off = body + 128 + BI * 4;
  const int lds = body + 128 + BI * 4 + 1024;
  return lds <= 160 * 1024 ? lds : -1;
}
template <int BI, int WJ, int WI, int BJ, bool RELU, bool UP, bool PB2, bool W3, int NKL>
static inline int sg_launch_conv_v3r(ConvV3Params p, const Epilogue<bf16_t>& e, hipStream_t st) {
  const int lds = sg_conv_v3_lds(BI, BJ, p.npx, PB2, W3, &p.zero_off, &p.bias_off, &p.dump_off);
  if (lds < 0) return -1;
  static bool attr_done = false;
  if (!ht_allow_lds(attr_done, sg_conv_v3_kernel<BI, WJ, WI, BJ, RELU, UP, PB2, W3, NKL>, 160 * 1024)) return -1;
  const int tilesI = (p.I + BI - 1) / BI, tilesJ = (p.J + BJ - 1) / BJ;
  hipLaunchKernelGGL((sg_conv_v3_kernel<BI, WJ, WI, BJ, RELU, UP, PB2, W3, NKL>), dim3(tilesI * tilesJ), dim3(64 * WJ * WI), lds, st, p, e, tilesI, tilesJ);
  return 0;
}
template <int BI, int WJ, int WI, int BJ, int NKL>
static inline int sg_launch_conv_v3(const ConvV3Params& p, const Epilogue<bf16_t>& e, hipStream_t st) {
  const bool up = (p.flags & SG_PIX_UPSAMPLE) != 0, relu = (p.flags & SG_PIX_RELU) != 0;
  const bool pb2 = p.nslice > 1 && sg_conv_v3_lds(BI, BJ, p.npx, true) > 0;
  if (!pb2 && sg_conv_v3_lds(BI, BJ, p.npx, false) < 0) return -1;
  if constexpr (BJ == 256 && (BI == 192 || BI == 128)) {      // the deep-layer configurations: three weight buffers when they fit
    if (pb2 && sg_conv_v3_lds(BI, BJ, p.npx, true, true) > 0 && (((p.npx >> 3) + WJ * WI - 1) / (WJ * WI) + 7) / 8 <= 2) {
      if (relu) return up ? sg_launch_conv_v3r<BI, WJ, WI, BJ, true, true, true, true, NKL>(p, e, st) : sg_launch_conv_v3r<BI, WJ, WI, BJ, true, false, true, true, NKL>(p, e, st);
      return up ? sg_launch_conv_v3r<BI, WJ, WI, BJ, false, true, true, true, NKL>(p, e, st) : sg_launch_conv_v3r<BI, WJ, WI, BJ, false, false, true, true, NKL>(p, e, st);
    }
  }
#define SG_V3_CASE(R_, U_, P_) if (relu == R_ && up == U_ && pb2 == P_) return sg_launch_conv_v3r<BI, WJ, WI, BJ, R_, U_, P_, false, NKL>(p, e, st);
  SG_V3_CASE(false, false, false) SG_V3_CASE(false, false, true) SG_V3_CASE(false, true, false) SG_V3_CASE(false, true, true)
  SG_V3_CASE(true, false, false) SG_V3_CASE(true, false, true) SG_V3_CASE(true, true, false) SG_V3_CASE(true, true, true)
#undef SG_V3_CASE
  return -1;
}
// tile choice -> instantiation, for one value of NKL (explicitly instantiated in conv_v3.hip (4) and conv_v3b.hip (2): two translation units, built in parallel)
template <int NKL>
int sg_conv_v3_dispatch(int best, int BJ, const ConvV3Params& p, const Epilogue<bf16_t>& e, hipStream_t st) {
  if (best == 192) return sg_launch_conv_v3<192, 4, 2, 256, NKL>(p, e, st);
  if (best == 128) return sg_launch_conv_v3<128, 4, 2, 256, NKL>(p, e, st);
  if (best == 32) return sg_launch_conv_v3<32, 8, 1, 512, NKL>(p, e, st);
  if (BJ == 512) return sg_launch_conv_v3<96, 8, 1, 512, NKL>(p, e, st);
  return sg_launch_conv_v3<96, 8, 1, 256, NKL>(p, e, st);
}
