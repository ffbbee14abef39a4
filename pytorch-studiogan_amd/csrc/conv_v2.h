// conv_v2.h -- second-generation forward / data-gradient convolution kernel for the hot bf16 shapes.
//
// Same contraction and the same epilogue as gemm_core.h (OUT[pixel j][cout i] = sum_k W(i,k) X(j,k)), restructured
// along cdna_hip_programming.md §5 ("256-wide tile, BK=64, LDS-DMA staging, two LDS buffers"):
//   * 512 threads = 8 waves (2 per SIMD), pixel tile BJ = 256, cout tile BI in {96,128,192,256}, BK = 64 (128-byte rows)
//   * global -> LDS by global_load_lds_dwordx4 (no VGPR staging, no ds_write): one instruction moves 8 rows x 128 B.
//     The LDS image is lane-linear, so the bank-conflict swizzle is applied to the SOURCE address: lane (row, slot)
//     fetches logical 16-byte chunk  slot ^ ((row >> 1) & 7); fragment reads apply the same involution
//     (guide §5.4 rule 21). Conflict-free for the 16-lane service groups of ds_read_b128.
//   * the DMA goes through buffer descriptors (buffer_load_dwordx4 ... offen lds): a 32-bit byte offset per lane, no 64-bit
//     address arithmetic; convolution halo / k-tail / row-tail lanes set bit 31 of their offset, which is out of range of the
//     descriptor, and the hardware writes zeros to LDS for them (tools/probes/oob_lds_probe.hip). A DMA piece is 3-5 VALU
//     instructions + s_add m0 + the load (the pointer-select form it replaces compiled to ~40 instructions and 4 branches per
//     piece: ~300 of the 400 instructions of a k-tile, all in front of the 24 MFMAs)
//   * the (tap, channel-chunk) position of a lane is advanced incrementally (no division in the k-loop); the
//     per-row halo test is a precomputed bit mask
//   * next k-tile's DMA is issued before the current tile's MFMAs; one barrier per k-tile.
#pragma once
#include "gemm_core.h"

struct ConvV2Params {
  const bf16_t* x; const bf16_t* w;
  int N, Hs, Ws, C, ldx;
  int Hin, Win, Ho, Wo;
  int R, S, pad_h, pad_w;
  int stride;             // 1, or 2 without upsample-on-load / quad row order (InceptionV3's reduction layers): output (ho, wo) is centred on input (ho * stride, wo * stride)
  int flags;
  int I, J, K;
  int cpt;    // 16-byte chunks per tap = C / 8
  int ntap;   // R * S (<= 25)
  unsigned xbytes, wbytes;   // extents of the two descriptors (< 2^31 / < 2^30: bits 31 / 30 of an offset mean "out of range")
  int wshift, hshift;   // log2(Wo), log2(Ho) or -1
};

typedef __attribute__((address_space(1))) const void* sg_gptr_t;
typedef __attribute__((address_space(3))) void* sg_lptr_t;

// ---- the epilogue shared by conv_v2 / conv_v3 -------------------------------------------------------------------------
// acc[TI][TJ]: 32x32 accumulator blocks of this wave (block (a,b) = couts wi0+32a.., pixels wj0+32b..); smem: the (dead) operand
// buffers, reused as the output staging area; sbias: BI floats in LDS (valid when epi.bias).
// VMAP (conv_q.h, UP form): the tile's rows are positions of a LOW-resolution grid and the output / mask / residual tensors are one parity
// view of the tensor at twice the resolution: global row of tile row jg = ((jg >> vlog) << (vlog + 2)) + ((jg & (2^vlog - 1)) << 1) + vadd.
// PLANES = false: compiled without the sign-plane code (Epilogue::mask_bits / sign_out are ignored: the mask is read from the activation, no plane is written).
template <int BI, int BJ, int NW, int TI, int TJ, bool VMAP = false, bool NOSTORE = false, bool PLANES = true>      // NOSTORE: ablation only (conv_v4.h ABL bit 5)
__device__ __forceinline__ void sg_conv_epilogue(f32x16 (&acc)[TI][TJ], char* smem, const float* sbias, const Epilogue<bf16_t>& epi,
                                                 int i0, int j0, int wi0, int wj0, float al, int vlog = 0, int vadd = 0,
                                                 float* stats = nullptr, int stats_C = 0, int stats_row = 0) {
  auto grow = [&](int jg) -> long long {
    if (VMAP) return (long long)(((jg >> vlog) << (vlog + 2)) + ((jg & ((1 << vlog) - 1)) << 1) + vadd);
    return (long long)jg;
  };
  const int tid = threadIdx.x, lane = tid & 63;
  // bf16 output tile: staged through LDS (the operand buffers are dead now) so that the global stores are 16 bytes per lane with
  // consecutive lanes on consecutive addresses of a row. The direct form (8 bytes per lane, 32 different rows per instruction)
  // ran at ~1.4 TB/s and cost 17 us per 256 x 192 tile -- 27 % of a 192->192 @64^2 convolution. The launcher only admits
  // problems this path can store (bf16 output, 16-byte aligned rows, whole cout tiles): there is no second epilogue in the kernel
  // (the generic one was 19 k of the kernel's 21 k instructions -- fetched by every workgroup of a short-K layer).
  const bool pool = (epi.flags & SG_EPI_POOL) != 0;
  constexpr int CP = BI * 2 + 16;              // LDS row pitch of the staged tile (bytes)
  // ReLU-mask / residual operand of the epilogue: its tile is fetched with the SAME coalesced 16-byte pattern as the output store,
  // into the output staging area; a lane then finds the four values it needs at the very LDS location it is going to overwrite
  // with its result (each (row, 4-channel group) location belongs to exactly one lane, so the update is in place).
  // The generic form reads 8 bytes per lane from 32 different rows per instruction, 24 dependent groups per lane.
  const int rows_out = pool ? BJ / 4 : BJ;
  const int jbase = pool ? (j0 >> 2) : j0, Jout = pool ? (epi.J >> 2) : epi.J;
  constexpr int CPR = BI / 8;                  // 16-byte chunks per output row
  const bool pre_mask = epi.mask != nullptr, pre_res = epi.res != nullptr;    // bf16, 16-byte aligned rows (launcher)
  const bool pre_both = pre_mask && pre_res;
  const int ncr = ((epi.I - i0 < BI ? epi.I - i0 : BI) + 7) >> 3;             // 16-byte chunks of an output row that exist (cout tail tile)
  auto stage_tile = [&](const bf16_t* src, int ld) {
    for (int idx = tid; idx < rows_out * CPR; idx += 64 * NW) {
      const int r = idx / CPR, c = idx - r * CPR;
      const int jg = jbase + r;
      u32x4 t = {0u, 0u, 0u, 0u};
      if (jg < Jout && c < ncr) t = *(const u32x4*)(src + grow(jg) * ld + i0 + c * 8);
      *(u32x4*)(smem + r * CP + c * 16) = t;
    }
  };
  // ReLU mask AND residual in one launch (the data gradient of a block's first convolution taking the skip path's gradient as its residual:
  // dx = mask(x) * F^T(dh) + dx_skip -- the sum autograd would otherwise run as its own elementwise launch): the staging area holds one tile,
  // so the mask tile goes first and is condensed to 16 bits per accumulator block in registers, then the residual tile takes its place.
  uint32_t mbits[TI * TJ];
#pragma unroll
  for (int q = 0; q < TI * TJ; q++) mbits[q] = 0u;
  // The mask as a sign plane (Epilogue::mask_bits: one bit per element, 1/16 of the activation's bytes): no staging and no barrier. Every lane loads, per
  // accumulator block, the ONE dword that holds the block's 32 channels of its pixel and keeps its own 16 bits in the layout the mask-and-residual path
  // condenses a staged tile to (bit 4 g4 + e = channel 8 g4 + 4 (lane >> 5) + e of the block). Requested in front of the barrier that frees the operand
  // buffers, so the round trip runs while the workgroup's other waves finish their last k-tile.
  const bool plane = PLANES && pre_mask && epi.mask_bits != nullptr;
  if (plane) {
#pragma unroll
    for (int ta = 0; ta < TI; ta++)
#pragma unroll
      for (int tb = 0; tb < TJ; tb++) {
        const int jl = wj0 + tb * 32 + (lane & 31);
        const int jg = jbase + (pool ? (jl >> 2) : jl);
        const int ib = i0 + wi0 + ta * 32;                 // first channel of the block: a multiple of 32 (cout tiles and wave blocks are)
        uint32_t w = 0u;
        if (jg < Jout && ib < epi.I) w = epi.mask_bits[grow(jg) * epi.ldmb + (ib >> 5)];
        w >>= 4 * (lane >> 5);
        mbits[ta * TJ + tb] = (w & 0xfu) | ((w >> 4) & 0xf0u) | ((w >> 8) & 0xf00u) | ((w >> 12) & 0xf000u);
      }
  }
  __syncthreads();                             // every wave is done reading the operand buffers
  if (pre_both && !plane) {
    stage_tile(epi.mask, epi.ldm);
    __syncthreads();
#pragma unroll
    for (int ta = 0; ta < TI; ta++)
#pragma unroll
      for (int tb = 0; tb < TJ; tb++) {
        const int jl = wj0 + tb * 32 + (lane & 31);
        const int jo = pool ? (jl >> 2) : jl;
        uint32_t bits = 0u;
#pragma unroll
        for (int g4 = 0; g4 < 4; g4++) {
          const int il = wi0 + ta * 32 + 8 * g4 + 4 * (lane >> 5);
          const u32x2 m = *(const u32x2*)(smem + jo * CP + il * 2);
#pragma unroll
          for (int e = 0; e < 4; e++) { const bf16_t h = (bf16_t)((m[e >> 1] >> (16 * (e & 1))) & 0xffffu); if (sg_relu_pos(h)) bits |= 1u << (4 * g4 + e); }
        }
        mbits[ta * TJ + tb] = bits;
      }
    __syncthreads();
    stage_tile((const bf16_t*)epi.res, epi.ldr);
    __syncthreads();
  } else if ((pre_mask && !plane) || pre_res) {      // one operand to stage: the residual, or the mask when it came without a plane
    const bool sm = pre_mask && !plane;
    stage_tile(sm ? epi.mask : (const bf16_t*)epi.res, sm ? epi.ldm : epi.ldr);
    __syncthreads();
  }
  const bool relu_out = (epi.flags & SG_EPI_RELU) != 0;
#pragma unroll
  for (int ta = 0; ta < TI; ta++)
#pragma unroll
    for (int tb = 0; tb < TJ; tb++) {
      const int jl = wj0 + tb * 32 + (lane & 31);
#pragma unroll
      for (int g4 = 0; g4 < 4; g4++) {
        const int il = wi0 + ta * 32 + 8 * g4 + 4 * (lane >> 5);
        float v[4] = {acc[ta][tb][4 * g4 + 0], acc[ta][tb][4 * g4 + 1], acc[ta][tb][4 * g4 + 2], acc[ta][tb][4 * g4 + 3]};
        // same operation order as Epilogue::prep (pool, scale, bias, mask, residual, ReLU), operands from LDS
        if (pool) {
#pragma unroll
          for (int e = 0; e < 4; e++) v[e] = quad_sum(v[e]);
        }
        const int jo = pool ? (jl >> 2) : jl;
        const bool act = (!pool || (lane & 3) == 0) && (jbase + jo < Jout);
        if (act) {
          char* loc = smem + jo * CP + il * 2;
#pragma unroll
          for (int e = 0; e < 4; e++) v[e] *= al;
          if (epi.bias) {
            const f32x4 b = *(const f32x4*)(sbias + il);
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] += b[e];
          }
          if (pre_both || plane) {
            const uint32_t bits = mbits[ta * TJ + tb] >> (4 * g4);
#pragma unroll
            for (int e = 0; e < 4; e++) if (!((bits >> e) & 1u)) v[e] = 0.f;
          } else if (pre_mask) {
            const u32x2 m = *(const u32x2*)loc;
#pragma unroll
            for (int e = 0; e < 4; e++) { const bf16_t h = (bf16_t)((m[e >> 1] >> (16 * (e & 1))) & 0xffffu); if (!sg_relu_pos(h)) v[e] = 0.f; }
          }
          if (pre_res) {
            const u32x2 r = *(const u32x2*)loc;
#pragma unroll
            for (int e = 0; e < 4; e++) { const bf16_t h = (bf16_t)((r[e >> 1] >> (16 * (e & 1))) & 0xffffu); v[e] += epi.beta * bf2f(h); }
          }
          if (relu_out) {
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = fmaxf(v[e], 0.f);
          }
          u32x2 t;
          t[0] = pack2bf(v[0], v[1]);
          t[1] = pack2bf(v[2], v[3]);
          *(u32x2*)loc = t;
        }
      }
    }
  __syncthreads();
  if (stats) {
    // Batch-norm statistics of the layer behind this convolution, taken from the staged tile (the bf16 values the BN kernels would read back
    // from HBM): per channel the sum and the sum of squares over this tile's rows, written to stats[stats_row][channel][2]; the fp64 reduction
    // over the tiles is sg_bn_stats_from_tiles. Replaces the separate statistics pass over the activation (csrc/norm.hip k_bn_partial_stream:
    // one full read of every generator activation, 5 ms per C3 step). A wave owns BI / 8 channel pairs, its lanes split the rows RG ways.
    constexpr int PWV = BI / 2 / NW, RG = 64 / PWV;
    const int wv = tid >> 6, pl = lane % PWV, rg = lane / PWV;
    int rows_valid = Jout - jbase;
    if (rows_valid > rows_out) rows_valid = rows_out;
    float s1a = 0.f, s2a = 0.f, s1b = 0.f, s2b = 0.f;
    const int c2 = wv * PWV + pl;
    if (rg < RG) {
      // (fixed trip count, eight reads in flight: with the data-dependent bound the loop ran one LDS round trip per row, ~1.6 us per tile)
      constexpr int NIT = (BJ + RG - 1) / RG;
      const char* base = smem + rg * CP + c2 * 4;
#pragma unroll 8
      for (int k = 0; k < NIT; k++) {
        const int r = rg + k * RG;
        uint32_t v = *(const uint32_t*)(base + (r < BJ ? k * (RG * CP) : 0));      // (the last iterations of the higher row groups fall behind the tile: masked)
        v = r < rows_valid ? v : 0u;
        const float a = __uint_as_float(v << 16), b = __uint_as_float(v & 0xffff0000u);
        s1a += a; s2a += a * a; s1b += b; s2b += b * b;
      }
    }
    float t1a = s1a, t2a = s2a, t1b = s1b, t2b = s2b;
#pragma unroll
    for (int k = 1; k < RG; k++) {
      t1a += __shfl(s1a, lane + k * PWV, 64); t2a += __shfl(s2a, lane + k * PWV, 64);
      t1b += __shfl(s1b, lane + k * PWV, 64); t2b += __shfl(s2b, lane + k * PWV, 64);
    }
    const int c = i0 + 2 * c2;
    if (rg == 0 && c < epi.I) {
      f32x4 o4 = {t1a, t2a, t1b, t2b};
      *(f32x4*)(stats + ((long long)stats_row * stats_C + c) * 2) = o4;
    }
  }
  {
    bf16_t* o = (bf16_t*)epi.out;
    for (int idx = tid; idx < rows_out * CPR; idx += 64 * NW) {
      const int r = idx / CPR, c = idx - r * CPR;
      const int jg = jbase + r;
      if (NOSTORE) {
        const u32x4 v = *(const u32x4*)(smem + r * CP + c * 16);
        if (v[0] == 0x12345678u && v[1] == 0x9abcdef0u) *(u32x4*)(o + grow(jg) * epi.ldo + i0 + c * 8) = v;      // (never: keeps the read alive)
      } else if (jg < Jout && c < ncr) *(u32x4*)(o + grow(jg) * epi.ldo + i0 + c * 8) = *(const u32x4*)(smem + r * CP + c * 16);
    }
  }
  if (PLANES && epi.sign_out) {
    // Sign plane of the result (Epilogue::sign_out): one more pass over the finished tile in LDS, behind the tile's own stores. A thread owns one word =
    // 32 channels of one output row (four 16-byte chunks); consecutive threads write consecutive words of a row, then the next row. Rows beyond the problem
    // and words whose first chunk does not exist (cout tail tile) are skipped; inside a word, chunks and channels beyond the problem give zero bits.
    constexpr int NWD = BI / 32;
    const int nch = epi.I - i0 < BI ? epi.I - i0 : BI;      // channels of this tile that exist
    for (int idx = tid; idx < rows_out * NWD; idx += 64 * NW) {
      const int r = idx / NWD, k = idx - r * NWD;
      const int jg = jbase + r;
      if (jg >= Jout || 4 * k >= ncr) continue;
      uint32_t w = 0u;
#pragma unroll 1      // (one 16-byte chunk in registers at a time: the pass must not raise the kernel's register count)
      for (int c = 0; c < 4; c++)
        if (4 * k + c < ncr) w |= sg_relu_pos8(*(const u32x4*)(smem + r * CP + (4 * k + c) * 16)) << (8 * c);
      const int left = nch - 32 * k;                         // (a last chunk that is only partly inside the problem)
      if (left < 32) w &= (1u << left) - 1u;
      epi.sign_out[grow(jg) * epi.lds + (i0 >> 5) + k] = w;
    }
  }
}

// SCHED 0: all DMA pieces of the next k-tile are issued in front of the current tile's MFMAs.
// SCHED 1: the pieces are spread over the four 16-deep MFMA sub-steps (a wave issues in order: a DMA piece costs ~100 issue
//          cycles that would otherwise sit in front of the matrix pipe for BOTH lock-stepped waves of a SIMD at once).
template <int BI, int WJ, int WI, int BJ, int SCHED, bool RELU, bool UP>
__global__ __launch_bounds__(64 * WJ * WI) void sg_conv_v2_kernel(ConvV2Params p, Epilogue<bf16_t> epi, int tilesI, int tilesJ) {
  constexpr int NW = WJ * WI;                  // waves per workgroup (8, or 4 for the two-workgroups-per-CU variant)
  constexpr int QB = BJ * 128, PB = BI * 128, BUF = QB + PB;
  constexpr int NQ = BJ / 8 / NW;             // Q DMA instructions per wave per k-tile (8 rows each)
  constexpr int NPI = (BI / 8 + NW - 1) / NW; // P DMA instructions per wave per k-tile (upper bound)
  constexpr int TJ = BJ / WJ / 32, TI = BI / WI / 32;
  static_assert(NW == 8 || NW == 4, "4 or 8 waves");
  static_assert(BJ % (8 * NW) == 0, "pixel tile / DMA groups");
  static_assert(BJ % (WJ * 32) == 0 && BI % (WI * 32) == 0, "tile/wave mismatch");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // provably uniform: LDS-DMA destinations (M0) stay in SGPRs
  const int bid = sg_xcd_tile(blockIdx.x, tilesI * tilesJ);
  const int tI = bid % tilesI, tJ = bid / tilesI;
  const int i0 = tI * BI, j0 = tJ * BJ;
  // bias of this cout tile: fetched once per workgroup into its own LDS region (behind the operand buffers), visible after the
  // first barrier. The per-fragment scalar loads of the generic epilogue cost ~1 ms on the 96 -> 96 @128^2 layer (24 dependent
  // load groups per lane, every one exposing an L2 round trip).
  float* sbias = (float*)(smem + 2 * BUF);
  if (epi.bias) {
    for (int i = tid; i < BI; i += 64 * NW) sbias[i] = (i0 + i < epi.I) ? epi.bias[i0 + i] : 0.f;
  }

  // ---- per-lane DMA state ------------------------------------------------------------------------------
  const auto rsx = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.xbytes, 0x00020000);
  const auto rsw = __builtin_amdgcn_make_buffer_rsrc((void*)p.w, 0, (int)p.wbytes, 0x00020000);
  const int sub = lane >> 3;                                        // row within the 8-row DMA group
  const int lc = (lane & 7) ^ ((4 * wave + (lane >> 4)) & 7);       // logical chunk this lane fetches (same for all its rows: NW is a multiple of 2)
  const unsigned ldx2 = 2u * (unsigned)p.ldx;                       // pixel pitch in bytes
  unsigned qoff[NQ];      // byte offset of the row's centre pixel (source resolution)
  unsigned qinv[NQ];      // bit t set = tap t of this row is outside the image (or the row is outside the problem); bits >= ntap set
  bool qph[NQ], qpw[NQ];  // upsample-on-load: parity of the output pixel
#pragma unroll
  for (int i = 0; i < NQ; i++) {
    const int row = j0 + 8 * (wave + NW * i) + sub;
    int n, ho, wo;
    if (p.flags & SG_PIX_QUAD) {
      const int q = row >> 2, dy = (row >> 1) & 1, dx = row & 1;
      const int Wq = p.Wo >> 1, Hq = p.Ho >> 1;
      int wq, hq;
      if (p.wshift >= 1 && p.hshift >= 1) { wq = q & (Wq - 1); const int t = q >> (p.wshift - 1); hq = t & (Hq - 1); n = t >> (p.hshift - 1); }
      else { wq = q % Wq; const int t = q / Wq; hq = t % Hq; n = t / Hq; }
      ho = 2 * hq + dy; wo = 2 * wq + dx;
    } else if (p.wshift >= 0 && p.hshift >= 0) {
      wo = row & (p.Wo - 1); const int t = row >> p.wshift; ho = t & (p.Ho - 1); n = t >> p.hshift;
    } else {
      wo = row % p.Wo; const int t = row / p.Wo; ho = t % p.Ho; n = t / p.Ho;
    }
    unsigned m = 0;
    if (row < p.J) {     // halo bit mask, one bit per tap (nested loops: no division by S per tap -- that cost 7 us per tile)
      int t = 0;
      for (int rr = 0; rr < p.R; rr++) {
        const bool hok = (unsigned)(ho * p.stride - p.pad_h + rr) < (unsigned)p.Hin;
        for (int ss = 0; ss < p.S; ss++, t++)
          if (hok && (unsigned)(wo * p.stride - p.pad_w + ss) < (unsigned)p.Win) m |= 1u << t;
      }
    }
    qinv[i] = ~m;
    qph[i] = UP && (ho & 1); qpw[i] = UP && (wo & 1);
    const int hs = UP ? (ho >> 1) : ho * p.stride, ws = UP ? (wo >> 1) : wo * p.stride;
    qoff[i] = ((unsigned)(n * p.Hs + hs) * (unsigned)p.Ws + (unsigned)ws) * ldx2;
  }
  unsigned poff[NPI];     // byte offset of the weight row; 0x40000000 = row outside the problem
#pragma unroll
  for (int i = 0; i < NPI; i++) {
    const int g = wave + NW * i;                // DMA group index inside the P tile
    const int row = i0 + 8 * g + sub;
    poff[i] = ((g < BI / 8) && (row < p.I)) ? (unsigned)row * (unsigned)p.K * 2u : 0x40000000u;
  }
  // position of this lane inside K: tap (r,s) and chunk-in-tap c8; q = global chunk index
  int q = lc, tap = lc / p.cpt, c8 = lc - tap * p.cpt, tr = tap / p.S, ts = tap - tr * p.S;

  // per k-tile, per lane: the byte displacement of the lane's (tap, chunk) from the centre pixel. With upsample-on-load the
  // displacement depends on the parity of the output pixel: two row terms and two column terms, selected per piece.
  unsigned kd0 = 0, kdh1 = 0, kdw1 = 0, kw = 0;
  auto position = [&]() {
    const int dr = tr - p.pad_h, ds = ts - p.pad_w;
    if (UP) {
      const unsigned rowb = (unsigned)p.Ws * ldx2;
      kd0 = (unsigned)(dr >> 1) * rowb + (unsigned)(ds >> 1) * ldx2 + (unsigned)c8 * 16u;                  // even row, even column
      kdh1 = ((unsigned)((dr + 1) >> 1) - (unsigned)(dr >> 1)) * rowb;                                     // extra for an odd output row
      kdw1 = ((unsigned)((ds + 1) >> 1) - (unsigned)(ds >> 1)) * ldx2;                                     // extra for an odd output column
    } else {
      kd0 = (unsigned)(dr * p.Ws + ds) * ldx2 + (unsigned)c8 * 16u;
    }
    kw = (tap < p.ntap) ? (unsigned)q * 16u : 0x40000000u;
  };
  position();

  // one k-tile's DMA = NQ + NPI pieces per wave; piece(buf, i) issues piece i, advance() steps the lane's K position
  auto piece = [&](int buf, int i) {
    char* qd = smem + buf * BUF;
    char* pd = qd + QB;
    if (i < NQ) {
      unsigned off = qoff[i] + kd0;
      if (UP) off += (qph[i] ? kdh1 : 0u) + (qpw[i] ? kdw1 : 0u);
      off |= ((qinv[i] >> tap) & 1u) << 31;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsx, (sg_lptr_t)(qd + (wave + NW * i) * 1024), 16, (int)off, 0, 0, 0);
    } else {
      const int j = i - NQ;
      if (NW * (j + 1) <= BI / 8 || wave + NW * j < BI / 8) {     // compile-time true for full groups, else wave-uniform
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (sg_lptr_t)(pd + (wave + NW * j) * 1024), 16, (int)(poff[j] + kw), 0, 0, 0);
      }
    }
  };
  // next k-tile: 8 chunks further. C >= 64: at most one tap boundary, done with selects (no branch in the k-loop);
  // thin / odd channel counts (any C % 8 == 0): the position is recomputed from the chunk index
  auto advance = [&]() {
    q += 8;
    if (p.cpt >= 8) {
      c8 += 8;
      const bool w = c8 >= p.cpt;
      c8 -= w ? p.cpt : 0;
      tap += w ? 1 : 0; ts += w ? 1 : 0;
      const bool w2 = ts == p.S;
      ts = w2 ? 0 : ts; tr += w2 ? 1 : 0;
    } else {
      tap = q / p.cpt; c8 = q - tap * p.cpt;
      tr = tap / p.S; ts = tap - tr * p.S;
    }
    position();
  };
  auto issue = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NQ + NPI; i++) piece(buf, i);
    advance();
  };

  f32x16 acc[TI][TJ];
#pragma unroll
  for (int a = 0; a < TI; a++)
#pragma unroll
    for (int b = 0; b < TJ; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;

  const int wj = wave % WJ, wi = wave / WJ;
  const int wj0 = wj * (BJ / WJ), wi0 = wi * (BI / WI);
  const int frow = lane & 31, fhi = lane >> 5;

  const int nk = (SCHED == 5 || SCHED == 6) ? 1 : (p.K / 8 + 7) / 8;   // k-tiles of 8 chunks (SCHED 5/6: ablation, one k-tile only)
  issue(0);
  __syncthreads();
  constexpr int NP = NQ + NPI, PPS = (NP + 3) / 4;     // pieces per MFMA sub-step when spread (SCHED 1)
  for (int kt = 0; kt < nk; kt++) {
    const bool more = (SCHED == 2 || SCHED == 4) ? false : (kt + 1 < nk);     // SCHED 2/4: ablation, no DMA in the loop (wrong results)
    if ((SCHED == 0 || SCHED == 3 || SCHED == 7) && more) issue((kt + 1) & 1);
    const char* qs = smem + (kt & 1) * BUF;
    const char* ps = qs + QB;
    // 16-deep sub-steps of this k-tile that hold data (wave-uniform; < 4 only in the last tile when K % 64 != 0)
    const int krem = p.K - kt * 64;
    const int nks = krem >= 64 ? 4 : ((krem + 15) >> 4);
    if (SCHED == 7) {
      // fragments of sub-step ks+1 are requested before the MFMAs of sub-step ks (register double buffering)
      bf16x8_t pf[2][TI], qf[2][TJ];
      auto load = [&](int ks, int slot) {
#pragma unroll
        for (int a = 0; a < TI; a++) {
          const int row = wi0 + a * 32 + frow;
          const int ch = (ks * 2 + fhi) ^ ((row >> 1) & 7);
          u32x4 v = *(const u32x4*)(ps + row * 128 + ch * 16);
          pf[slot][a] = __builtin_bit_cast(bf16x8_t, v);
        }
#pragma unroll
        for (int b = 0; b < TJ; b++) {
          const int row = wj0 + b * 32 + frow;
          const int ch = (ks * 2 + fhi) ^ ((row >> 1) & 7);
          u32x4 v = *(const u32x4*)(qs + row * 128 + ch * 16);
          if (RELU) v = relu16<bf16_t>(v);
          qf[slot][b] = __builtin_bit_cast(bf16x8_t, v);
        }
      };
      load(0, 0);
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        if (ks < 3 && __builtin_expect(ks + 1 < nks, 1)) load(ks + 1, (ks + 1) & 1);
        if (__builtin_expect(ks < nks, 1)) {
#pragma unroll
          for (int a = 0; a < TI; a++)
#pragma unroll
            for (int b = 0; b < TJ; b++)
              acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[ks & 1][a], qf[ks & 1][b], acc[a][b], 0, 0, 0);
        }
      }
    } else {
#pragma unroll
    for (int ks = 0; ks < 4; ks++) {
      bf16x8_t pf[TI], qf[TJ];
      if ((SCHED == 3 || SCHED == 4) && kt > 0) {       // ablation: no fragment reads after the first tile (wrong results)
#pragma unroll
        for (int a = 0; a < TI; a++) { u32x4 z = {(unsigned)kt, 1u, 2u, 3u}; asm volatile("" : "+v"(z)); pf[a] = __builtin_bit_cast(bf16x8_t, z); }
#pragma unroll
        for (int b = 0; b < TJ; b++) { u32x4 z = {(unsigned)ks, 5u, 6u, 7u}; asm volatile("" : "+v"(z)); qf[b] = __builtin_bit_cast(bf16x8_t, z); }
      } else {
#pragma unroll
      for (int a = 0; a < TI; a++) {
        const int row = wi0 + a * 32 + frow;
        const int ch = (ks * 2 + fhi) ^ ((row >> 1) & 7);
        u32x4 v = *(const u32x4*)(ps + row * 128 + ch * 16);
        pf[a] = __builtin_bit_cast(bf16x8_t, v);
      }
#pragma unroll
      for (int b = 0; b < TJ; b++) {
        const int row = wj0 + b * 32 + frow;
        const int ch = (ks * 2 + fhi) ^ ((row >> 1) & 7);
        u32x4 v = *(const u32x4*)(qs + row * 128 + ch * 16);
        if (RELU) v = relu16<bf16_t>(v);
        qf[b] = __builtin_bit_cast(bf16x8_t, v);
      }
      }
      if (SCHED == 1 && more) {
#pragma unroll
        for (int i = ks * PPS; i < (ks + 1) * PPS && i < NP; i++) piece((kt + 1) & 1, i);
      }
      if (__builtin_expect(ks < nks, 1)) {
#pragma unroll
        for (int a = 0; a < TI; a++)
#pragma unroll
          for (int b = 0; b < TJ; b++)
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[a], qf[b], acc[a][b], 0, 0, 0);
      }
    }
    }
    if (SCHED == 1 && more) advance();
    __syncthreads();
  }

  float al = epi.alpha;
  if (epi.alpha_ptr) al *= *epi.alpha_ptr;
  if (SCHED == 6) {       // ablation: no epilogue (keep the accumulators alive with one conditional store)
    float t = 0.f;
#pragma unroll
    for (int ta = 0; ta < TI; ta++)
#pragma unroll
      for (int tb = 0; tb < TJ; tb++) t += acc[ta][tb][0];
    if (t == 1234.5f) *(float*)epi.out = t;
    return;
  }
  sg_conv_epilogue<BI, BJ, NW, TI, TJ>(acc, smem, sbias, epi, i0, j0, wi0, wj0, al);
}

template <int BI, int WJ, int WI, int BJ, int SCHED, bool RELU, bool UP>
static inline int sg_launch_conv_v2r(const ConvV2Params& p, const Epilogue<bf16_t>& e, hipStream_t st) {
  constexpr int BUF = (BJ + BI) * 128;
  static bool attr_done = false;
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)sg_conv_v2_kernel<BI, WJ, WI, BJ, SCHED, RELU, UP>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * BUF + BI * 4) != hipSuccess) return -1;
    attr_done = true;
  }
  const int tilesI = (p.I + BI - 1) / BI, tilesJ = (p.J + BJ - 1) / BJ;
  hipLaunchKernelGGL((sg_conv_v2_kernel<BI, WJ, WI, BJ, SCHED, RELU, UP>), dim3(tilesI * tilesJ), dim3(64 * WJ * WI), 2 * BUF + BI * 4, st, p, e, tilesI, tilesJ);
  return 0;
}
template <int BI, int WJ, int WI, int BJ = 256, int SCHED = 0>
static inline int sg_launch_conv_v2(const ConvV2Params& p, const Epilogue<bf16_t>& e, hipStream_t st) {
  const bool up = (p.flags & SG_PIX_UPSAMPLE) != 0;
  if (p.flags & SG_PIX_RELU) return up ? sg_launch_conv_v2r<BI, WJ, WI, BJ, SCHED, true, true>(p, e, st) : sg_launch_conv_v2r<BI, WJ, WI, BJ, SCHED, true, false>(p, e, st);
  return up ? sg_launch_conv_v2r<BI, WJ, WI, BJ, SCHED, false, true>(p, e, st) : sg_launch_conv_v2r<BI, WJ, WI, BJ, SCHED, false, false>(p, e, st);
}
