// conv_v4.h -- halo forward / data-gradient kernel for the SHORT-K 3x3 layers (bf16, stride 1, pad 1, C % 32 == 0): three small
// independent workgroups per CU instead of one large one.
//
// conv_v3.h runs ONE 125-150 KB workgroup of 8 waves per CU. On the deep layers (K = 9 C >= 3456) a tile is hundreds of taps long and
// its fixed costs vanish; on the 96-channel 128^2 layers a 512-pixel tile is 18 taps against a 100 KB patch prologue, a second patch
// load between its two channel slices and a 98 KB staged epilogue, and with one workgroup per CU nothing overlaps them: 680-840 TFLOP/s
// (profiles/r02_conv_layer_table_f.txt), 670 even with the loop's DMA removed (profiles/r01_conv_v3_ablation_dma.txt). wgrad_v3.h
// fixed the same problem for the weight gradient by making workgroups small enough that three share a CU; this is the same move:
//   * tile = 256 output pixels x 32 NB couts (NB = 3 or 2); 4 waves, wave w = pixels 64 w .. 64 w + 63 x all couts (2 x NB accumulators
//     of 32 x 32 = 96 registers for NB = 3): <= 168 registers per lane;
//   * the pixel operand is staged once per 32-CHANNEL slice as a raster patch ([tile + one image row + 8 pixels either side] x 64 B,
//     chunk swizzle c ^ (row >> 2 & 3): any 16 consecutive rows are conflict-free for ds_read_b128), 33 KB at W = 128; the nine taps
//     read it at shifted rows exactly like conv_v3.h; weights stream per tap: 32 NB x 64 B, three buffers, two taps ahead;
//     Quad row order (2 x 2 pooling epilogue / pooling-sum data gradient) puts pixels (h, w) and (h + 1, w) into the same 16-lane group of a
//     ds_read_b128; their patch rows differ by W, a multiple of 16, so the row-keyed swizzle gave them the same 16-byte slot: a 2-way
//     conflict on every B-fragment read of those layers (10-26 % of the LDS cycles in profiles/r02_conv_sq_counters_final.txt). The
//     swizzle therefore also carries the PARITY OF THE IMAGE ROW (bit 1 of the chunk index ^= parity), applied on the DMA source side and
//     in the fragment addresses; W = 8 / 4 patches are conflict-free as they are (rows r, r + 8 already differ in the key);
//   * operand LDS 52 KB, staged epilogue 53 KB -> three workgroups per CU (12 waves, 3 per SIMD, from different workgroups: one
//     computes while another loads its patch or stores its tile). One barrier (4 waves) per tap = per 4 NB MFMAs of a wave.
// Row bookkeeping (raster / quad order, nearest x2 upsample on load, image-border masks), the 64-byte-row LDS image and its DMA / fragment addressing:
// halo_tile.h; epilogue: sg_conv_epilogue.
#pragma once
#include <type_traits>
#include "halo_tile.h"

struct ConvV4Params {
  const bf16_t* x; const bf16_t* w;
  int W, wlog;            // source image width (power of two >= 4)
  int C, ldx;
  int Ho, Wo, wshift, hshift;
  int flags;
  int I, J, K;
  int nslice;             // C / 32
  int npix_src;           // N * Hs * Ws
  int npx;                // patch pixels (multiple of 16) >= BJ(/4 with upsample) + 2 W + 16
  unsigned xbytes, wbytes;
  int wgt_off, zero_off, bias_off;   // LDS byte offsets: weight buffers, zero line, bias vector
  int pm2, psh;           // image-row parity term of the chunk swizzle: chunk ^= ((pixel >> psh) & pm2), pm2 = 2 (quad row order, W >= 16) or 0
  // fused 1x1 skip convolution (SKIP instantiations): acc += conv1x1(up2?(x2); w2) as extra K-slices at the centre tap
  const bf16_t* x2; const bf16_t* w2; const float* bias2;
  int C2, ldx2, up2, nslice2, npix2;   // C2 % 32 == 0; up2: x2 is at half resolution (nearest x2 on load); npix2 = N * Hs2 * Ws2
  unsigned x2bytes, w2bytes;
  float* stats;           // optional [tilesJ][I][2]: per-tile batch-norm statistics of the result (sg_conv_epilogue), 256-pixel tiles only
};

// TJW = 32-pixel blocks per wave; 2 is the only value built (tile 256 pixels, 6 accumulator blocks per wave for NB = 3, three workgroups per CU)
//
// SKIP: the residual block's 1x1 skip convolution rides in the same launch (reference src/models/big_resnet.py:177-192,221-242:
// `x0 = conv2d0(x0); out = x + x0`). pool(conv3x3(h)) + pool(conv1x1(x)) = pool(conv3x3(h) + conv1x1(x)), and for a generator block
// conv3x3(h) + conv1x1(up(x)): the skip is C2 / 32 more K-slices of the same accumulators, each a single (centre) tap, fed from a second
// input tensor and a second weight matrix. After the main loop the patch area is free: slice by slice the skip input of the tile's own
// pixels (no halo) is staged there (one source pixel per 2 x 2 outputs with up2) next to its 32 NB x 32 weights. This removes the skip's
// launch, its read-modify-write of the block output and the 1x1 kernel's tile overheads.
//
// Measured and removed in round 5 (profiles/r05_variant_ab_layer_tables_b.txt): a fourth weight buffer with the tiles three taps ahead -- +1.0 % on the layer
// table: the counted wait in front of a tap's barrier is not the weight tile's latency.
// ABL (measurement aid, tools/sessions/r6u.sh; never launched by the product): compile-time ablation of one cost at a time -- bit 0: no epilogue (the accumulators
// are kept alive by a store that never happens), bit 1: no patch reload at the slice boundaries (one barrier instead of the full stop), bit 2: no weight DMA inside
// the loop (every tap re-reads the prologue's tiles), bit 3: no barrier at the end of a tap, bit 4: no fragment reads (the MFMAs run on the first tap's registers), bit 5: the epilogue without its global stores. Results are wrong by construction; what is read off is the time.
template <int NB, bool RELU, bool UP, int TJW, bool SKIP = false, int ABL = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void sg_conv_v4_kernel(ConvV4Params p, Epilogue<bf16_t> epi, int tilesI, int tilesJ) {
  static_assert(TJW == 2, "256-pixel tiles (the 512-pixel instantiation was measured no faster and removed in round 5)");
  static_assert(!SKIP || !UP, "the fused skip is built for the plain tile");
  constexpr int BI = 32 * NB, BJ = 128 * TJW, NW = 4, TI = NB, TJ = TJW;
  constexpr int PB = BI * 64;                  // one weight tile (BI couts x 32 channels)
  constexpr int NWP = BI / 16;                 // weight DMA pieces per tap (16 rows each): 6 or 4
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bid = sg_xcd_tile(blockIdx.x, tilesI * tilesJ);
  const int tI = bid % tilesI, tJ = bid / tilesI;
  const int i0 = tI * BI, j0 = tJ * BJ;
  char* const pbufs = smem + p.wgt_off;
  float* sbias = (float*)(smem + p.bias_off);
  // (= ht_stage_bias + ht_zero_line of halo_tile.h, written out: through the helpers the data gradients of the 96-channel 128^2 layers ran 0.8-3 % slower,
  // profiles/r11_halo_fold_ab.txt section 3)
  if (epi.bias) {
    for (int i = tid; i < BI; i += 64 * NW) {
      float b = (i0 + i < epi.I) ? epi.bias[i0 + i] : 0.f;
      if (SKIP && p.bias2 && i0 + i < epi.I) b += p.bias2[i0 + i];
      sbias[i] = b;
    }
  }
  if (tid < 32) ((unsigned*)(smem + p.zero_off))[tid] = 0u;

  const auto rsx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.xbytes, 0x00020000);
  const int sub = ht32_sub(lane), lc = ht32_chunk(lane);              // DMA lane geometry: row of the 16-row piece, logical chunk
  const unsigned ldx2 = 2u * (unsigned)p.ldx;

  // ---- patch DMA: groups of 16 consecutive source pixels, group g = wave + 4 i ----------------------------------------------------
  const int P0 = (UP ? (j0 >> 2) : j0) - p.W - 8;                    // raster index of patch row 0
  const int ngroups = p.npx >> 4;
  const int pix0 = P0 + 16 * wave + sub;
  // (round 5, as conv_q.h: what a lane's LDS-DMA pieces read differs from slice to slice by a wave-uniform channel offset only -- the per-lane byte offsets,
  // bounds decision included, are computed once per workgroup and the slice / tap offset rides in the instruction's scalar offset; the loop this replaces
  // re-derived ~8 vector instructions per piece, one of them a quarter-rate multiply, for each of the 6-11 pieces of a slice)
  constexpr int MAXPG = 7;                           // pieces per wave held in registers: (BJ + 2 W + 16) / 64 rounded up for W <= 64
  unsigned pvo[MAXPG];
  auto patch_offset = [&](int i) -> unsigned {
    const int pix = pix0 + 64 * i;
    const int lce = lc ^ ((pix >> p.psh) & p.pm2);
    return ((unsigned)pix < (unsigned)p.npix_src) ? (unsigned)pix * ldx2 + (unsigned)(lce * 16) : 0x80000000u;
  };
#pragma unroll
  for (int i = 0; i < MAXPG; i++) pvo[i] = patch_offset(i);
  auto patch_slice = [&](int s) {
#pragma unroll
    for (int i = 0; i < MAXPG; i++) {
      const int g = wave + NW * i;
      if (g < ngroups) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (sg_lptr_t)(smem + g * 1024), 16, (int)pvo[i], s * 64, 0, 0);
    }
    for (int g = wave + NW * MAXPG; g < ngroups; g += NW)            // (wider images only: offsets on the fly)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (sg_lptr_t)(smem + g * 1024), 16, (int)patch_offset((g - wave) / NW), s * 64, 0, 0);
  };
  // ---- weight DMA: BI rows x 32 channels of (slice s, tap t): per-lane row offsets once per workgroup ---------------------------------
  unsigned wvo[2];
  ht32_weight_offsets(wvo, i0, wave, sub, lc, p.I, p.K);
  auto weight_tile = [&](int buf, int s, int t) { ht32_weight_tile<NWP>(p.w, p.wbytes, pbufs + buf * PB, wvo, wave, (t * p.C + s * 32) * 2); };

  // ---- fragment rows of this lane --------------------------------------------------------------------------------------------------
  const int wj0 = wave * (32 * TJ);
  const int frow = lane & 31, fhi = lane >> 5;
  int rb[TJ];             // patch row of the centre pixel
  unsigned qinv[TJ];      // bit t set = tap t reads outside the image (or the row is outside the problem)
  unsigned par[TJ];       // upsample on load: bit 0 = output row is odd, bit 1 = output column is odd (decides which taps stay on the source pixel)
#pragma unroll
  for (int b = 0; b < TJ; b++) {
    const int row = j0 + wj0 + b * 32 + frow;
    int n, ho, wo;
    ht_decode_pixel(p, row, n, ho, wo);
    qinv[b] = ~ht_border_mask(ho, wo, p.Ho, p.Wo, row < p.J);
    rb[b] = ht_patch_row<UP>(p, n, ho, wo, P0);
    par[b] = UP ? (unsigned)(ho & 1) | ((unsigned)(wo & 1) << 1) : 0u;
  }
  unsigned wa[TI];        // weight fragment addresses inside a weight tile
  ht32_weight_frag_addr(wa, frow, fhi);

  f32x16 acc[TI][TJ];
  ht_zero_acc(acc);

  // Weights run TWO taps ahead through three buffers (buffer of tap t = t % 3, 9 taps per slice): a tap is only 4 NB MFMAs per wave,
  // shorter than the L2 latency of its successor's weights, so the wait in front of the barrier that ends tap t is COUNTED -- it lets
  // the pieces issued during tap t (for tap t + 2) stay in flight and only requires the older ones (tap t + 1). Waves 0 .. NWP - 5 issue
  // two pieces per tap, the others one.
  const int nslice = p.nslice;
  const bool two = wave + NW < NWP;                                  // this wave issues two weight pieces per tap
  constexpr int LA = 2;                                              // taps of lookahead (three weight buffers)
  patch_slice(0);
  weight_tile(0, 0, 0);
  weight_tile(1, 0, 1);
  __syncthreads();
  bf16x8_t pf0[2][TI], qf0[2][TJ];      // (ABL bit 4 only)
  for (int s = 0; s < nslice; s++) {
    const bool next_slice = s + 1 < nslice;
#pragma unroll
    for (int t = 0; t < 9; t++) {
      // weights LA taps ahead: buffer (t + LA) % 3 = (t - 1) % 3 was read during the previous tap, every wave is past its barrier (9 % 3 == 0: the ring restarts every slice)
      const bool issue = (t + LA < 9) || next_slice;
      const int ibuf = (t + LA) % 3;
      if constexpr (!(ABL & 4)) {
        if (t + LA < 9) weight_tile(ibuf, s, t + LA);
        else if (next_slice) weight_tile(ibuf, s + 1, t + LA - 9);
      }
      const char* ps = pbufs + ((ABL & 4) ? (t & 1) : (t % 3)) * PB;
      const int tr = t / 3, ts = t % 3;                          // compile-time after unrolling
      unsigned qa[TJ];
#pragma unroll
      for (int b = 0; b < TJ; b++) {
        int row = rb[b];
        asm volatile("" : "+v"(row));   // keeps a tap's address arithmetic inside the tap (hoisted out of the slice loop it spills: 36 addresses)
        if (UP) {           // source-pixel displacement of tap (tr, ts) under nearest x2: (ho + tr - 1) >> 1 and (wo + ts - 1) >> 1
          if (tr == 0) row += (par[b] & 1u) ? 0 : -p.W;
          if (tr == 2) row += (par[b] & 1u) ? p.W : 0;
          if (ts == 0) row += (par[b] & 2u) ? 0 : -1;
          if (ts == 2) row += (par[b] & 2u) ? 1 : 0;
        } else {
          if (tr == 0) row -= p.W;
          if (tr == 2) row += p.W;
          if (ts == 0) row -= 1;
          if (ts == 2) row += 1;
        }
        const int ipar = ((row + P0) >> p.psh) & p.pm2;          // image-row parity of the patch row (x 2)
        unsigned a = ((unsigned)row << 6) | ((unsigned)((fhi ^ (row >> 2) ^ ipar) & 3) << 4);
        a = ((qinv[b] >> t) & 1u) ? (unsigned)p.zero_off : a;
        qa[b] = a;
      }
      // Round 6: the fragments of BOTH k-steps of the tap are requested up front (10 ds_read_b128 in flight), then the 4 NB MFMAs run behind counted waits.
      // Left to the scheduler the loop kept ONE weight-fragment register: read, s_waitcnt lgkmcnt(0), two MFMAs, read the next into the same register, full wait, ...
      // -- six exposed LDS round trips per tap (profiles/r06_conv_v4_loop_isa_before.txt). The scheduling barriers pin the order as written.
      bf16x8_t pf[2][TI], qf[2][TJ];
      if ((ABL & 16) && (s | t)) {
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
#pragma unroll
          for (int a = 0; a < TI; a++) pf[ks][a] = pf0[ks][a];
#pragma unroll
          for (int b = 0; b < TJ; b++) qf[ks][b] = qf0[ks][b];
        }
      } else
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
#pragma unroll
        for (int a = 0; a < TI; a++) {
          u32x4 v = *(const u32x4*)(ps + (wa[a] ^ (unsigned)(ks * 32)));
          pf[ks][a] = __builtin_bit_cast(bf16x8_t, v);
        }
#pragma unroll
        for (int b = 0; b < TJ; b++) {
          u32x4 v = *(const u32x4*)(smem + (qa[b] ^ (unsigned)(ks * 32)));
          qf[ks][b] = __builtin_bit_cast(bf16x8_t, v);
        }
      }
      if ((ABL & 16) && !(s | t)) {
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
#pragma unroll
          for (int a = 0; a < TI; a++) pf0[ks][a] = pf[ks][a];
#pragma unroll
          for (int b = 0; b < TJ; b++) qf0[ks][b] = qf[ks][b];
        }
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < 2; ks++) {
        if (RELU) {
#pragma unroll
          for (int b = 0; b < TJ; b++) qf[ks][b] = __builtin_bit_cast(bf16x8_t, relu16<bf16_t>(__builtin_bit_cast(u32x4, qf[ks][b])));
        }
#pragma unroll
        for (int a = 0; a < TI; a++)
#pragma unroll
          for (int b = 0; b < TJ; b++)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[ks][a], qf[ks][b], acc[a][b], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (t == 8 && next_slice) {
        // slice boundary: the patch is single-buffered -- everyone must be done reading it, then it is reloaded (a full stop for this
        // workgroup; the other two workgroups of the CU keep the matrix pipe busy)
        __syncthreads();
        if constexpr (!(ABL & 2)) {
          patch_slice(s + 1);
          __syncthreads();
        }
      } else {
        if constexpr (!(ABL & 4)) {
          if (!issue) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          else if (two) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
        }
        if constexpr (!(ABL & 8)) __builtin_amdgcn_s_barrier();
      }
    }
  }

  if constexpr (SKIP) {
    // the main loop ended behind vmcnt(0) + barrier: patch area and weight buffers are free
    const auto rsx2 = __builtin_amdgcn_make_buffer_rsrc((void*)p.x2, 0, (int)p.x2bytes, 0x00020000);
    const unsigned ldx2b = 2u * (unsigned)p.ldx2;
    const int Q0 = p.up2 ? (j0 >> 2) : j0;                 // first skip-input pixel (raster) of this tile: the tile covers whole pairs of image rows
    const int ng2 = (p.up2 ? BJ / 4 : BJ) >> 4;            // groups of 16 pixels
    int rb2[TJ];
#pragma unroll
    for (int b = 0; b < TJ; b++) {
      const int r = rb[b] + P0;                            // raster index of the output pixel (the main conv is not UP: patch row + P0)
      if (p.up2) {
        const int wo = r & (p.Wo - 1), t = r >> p.wshift, ho = t & (p.Ho - 1), n = t >> p.hshift;
        rb2[b] = (((n * (p.Ho >> 1) + (ho >> 1)) << (p.wshift - 1)) + (wo >> 1)) - Q0;
      } else {
        rb2[b] = r - Q0;
      }
    }
    // Pipeline: RING staging slots (skip-input patch + weight tile each), slices RING - 1 ahead, ONE barrier per slice like the main loop:
    // the barrier at the top of slice s2 says "slice s2 has landed for every wave" and "every wave is done with slice s2 - 1", so the slot
    // of slice s2 - 1 takes slice s2 + RING - 1 right behind it. up2 (generator blocks): 4 KB patches, RING = 3; otherwise 16 KB, RING = 2.
    const int RING = p.up2 ? 3 : 2;
    const int P2B = (p.up2 ? BJ / 4 : BJ) * 64;
    auto issue2 = [&](int s2, int slot) {
      for (int g = wave; g < ng2; g += NW) {
        const int pix = Q0 + 16 * g + sub;
        const int lce = lc ^ ((pix >> p.psh) & p.pm2);
        unsigned off = (unsigned)pix * ldx2b + (unsigned)(s2 * 64 + lce * 16);
        off = ((unsigned)pix < (unsigned)p.npix2) ? off : 0x80000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx2, (sg_lptr_t)(smem + slot * P2B + g * 1024), 16, (int)off, 0, 0, 0);
      }
      ht32_skip_weight_tile<NWP>(pbufs + slot * PB, p, i0, wave, sub, lc, s2);
    };
    const int n2 = p.nslice2;
    for (int i = 0; i < RING - 1 && i < n2; i++) issue2(i, i);
    int slot = 0;
    for (int s2 = 0; s2 < n2; s2++) {
      // pieces this wave has in flight for ONE later slice (up2 only: 1 patch piece + 1 or 2 weight pieces); the wait leaves exactly those
      const bool later = p.up2 && (s2 + 1 < n2);
      if (!later) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (two) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      {
        const int nxt = s2 + RING - 1;
        int nslot = slot + RING - 1; if (nslot >= RING) nslot -= RING;
        if (nxt < n2) issue2(nxt, nslot);
      }
      const char* ps = pbufs + slot * PB;
      const unsigned pbase = (unsigned)(slot * P2B);
      unsigned qa[TJ];
#pragma unroll
      for (int b = 0; b < TJ; b++) {
        const int row = rb2[b];
        const int ipar = ((row + Q0) >> p.psh) & p.pm2;
        unsigned a = pbase + (((unsigned)row << 6) | ((unsigned)((fhi ^ (row >> 2) ^ ipar) & 3) << 4));
        a = ((qinv[b] >> 4) & 1u) ? (unsigned)p.zero_off : a;        // the centre tap is outside only for rows beyond the problem
        qa[b] = a;
      }
#pragma unroll
      for (int ks = 0; ks < 2; ks++) ht32_kstep<RELU>(acc, ps, wa, smem, qa, ks);
      slot = slot + 1 == RING ? 0 : slot + 1;
    }
  }

  float al = epi.alpha;
  if (epi.alpha_ptr) al *= *epi.alpha_ptr;
  if constexpr (ABL & 1) {
    float t = 0.f;
#pragma unroll
    for (int a = 0; a < TI; a++)
#pragma unroll
      for (int b = 0; b < TJ; b++)
#pragma unroll
        for (int r = 0; r < 16; r++) t += acc[a][b][r];
    if (t == 1234.5f) *(float*)epi.out = t;
  } else if constexpr ((ABL & 32) != 0) {
    sg_conv_epilogue<BI, BJ, NW, TI, TJ, false, true>(acc, smem, sbias, epi, i0, j0, 0, wj0, al, 0, 0, p.stats, p.I, tJ);
  } else {
    sg_conv_epilogue<BI, BJ, NW, TI, TJ>(acc, smem, sbias, epi, i0, j0, 0, wj0, al, 0, 0, p.stats, p.I, tJ);
  }
}

// LDS need (bytes) of a configuration
static inline int sg_conv_v4_lds(int NB, int npx, int* wgt_off, int* zero_off, int* bias_off, int skip_patch_bytes = 0) {
  // (a fused skip stages its own patches at the start of the operand area: the weight buffers must lie behind them too)
  const int woff = npx * 64 > skip_patch_bytes ? npx * 64 : skip_patch_bytes;
  return ht32_lds(32 * NB, 256, woff, 3, 0, wgt_off, zero_off, bias_off);
}
template <int NB, bool RELU, bool UP, int TJW, bool SKIP = false, int ABL = 0>
static inline int sg_launch_conv_v4r(ConvV4Params p, const Epilogue<bf16_t>& e, hipStream_t st) {
  const int lds = sg_conv_v4_lds(NB, p.npx, &p.wgt_off, &p.zero_off, &p.bias_off, SKIP ? (p.up2 ? 3 * 64 * 64 : 2 * 256 * 64) : 0);
  if (lds > 80 * 1024) return -1;
  static bool attr_done = false;
  if (!ht_allow_lds(attr_done, sg_conv_v4_kernel<NB, RELU, UP, TJW, SKIP, ABL>, 80 * 1024)) return -1;
  const int BI = 32 * NB, BJ = 128 * TJW;
  const int tilesI = (p.I + BI - 1) / BI, tilesJ = (p.J + BJ - 1) / BJ;
  hipLaunchKernelGGL((sg_conv_v4_kernel<NB, RELU, UP, TJW, SKIP, ABL>), dim3(tilesI * tilesJ), dim3(256), lds, st, p, e, tilesI, tilesJ);
  return 0;
}
template <int NB>
static inline int sg_launch_conv_v4_skip(const ConvV4Params& p, const Epilogue<bf16_t>& e, hipStream_t st) {
  if (p.flags & SG_PIX_RELU) return sg_launch_conv_v4r<NB, true, false, 2, true>(p, e, st);
  return sg_launch_conv_v4r<NB, false, false, 2, true>(p, e, st);
}
template <int NB, int TJW>
static inline int sg_launch_conv_v4(const ConvV4Params& p, const Epilogue<bf16_t>& e, hipStream_t st) {
  const bool up = (p.flags & SG_PIX_UPSAMPLE) != 0, relu = (p.flags & SG_PIX_RELU) != 0;
#ifdef SG_ABLATION   // measurement builds only: wrong results by construction, so the product library has neither these instantiations nor the switch
  if constexpr (NB == 3 && TJW == 2) {
    if (!up && !relu) {          // ablation instantiations (see the kernel): SG_V4_ABLATE = bit mask, plain 96-cout tiles only
      static int abl = -1;
      if (abl < 0) { const char* ev = getenv("SG_V4_ABLATE"); abl = ev ? atoi(ev) : 0; }
      switch (abl) {
        case 1: return sg_launch_conv_v4r<3, false, false, 2, false, 1>(p, e, st);
        case 2: return sg_launch_conv_v4r<3, false, false, 2, false, 2>(p, e, st);
        case 3: return sg_launch_conv_v4r<3, false, false, 2, false, 3>(p, e, st);
        case 4: return sg_launch_conv_v4r<3, false, false, 2, false, 4>(p, e, st);
        case 6: return sg_launch_conv_v4r<3, false, false, 2, false, 6>(p, e, st);
        case 7: return sg_launch_conv_v4r<3, false, false, 2, false, 7>(p, e, st);
        case 15: return sg_launch_conv_v4r<3, false, false, 2, false, 15>(p, e, st);
        case 32: return sg_launch_conv_v4r<3, false, false, 2, false, 32>(p, e, st);
        case 31: return sg_launch_conv_v4r<3, false, false, 2, false, 31>(p, e, st);
        default: break;
      }
    }
  }
#endif
  if (relu) return up ? sg_launch_conv_v4r<NB, true, true, TJW>(p, e, st) : sg_launch_conv_v4r<NB, true, false, TJW>(p, e, st);
  return up ? sg_launch_conv_v4r<NB, false, true, TJW>(p, e, st) : sg_launch_conv_v4r<NB, false, false, TJW>(p, e, st);
}
