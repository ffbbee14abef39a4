// halo_tile.h -- the pieces that the halo forward / data-gradient kernels (conv_v3.h, conv_v4.h, conv_q.h) have in common, written once.
//
// A halo kernel stages the pixel operand of a tile ONCE per channel slice as a raster PATCH in LDS (the tile's pixels plus one image row and 8 pixels
// of halo on either side) and reads the MFMA fragments of every filter tap from that patch at shifted rows; only the weight tile streams per tap.
// Everything arrives by LDS-DMA (buffer_load ... lds, 16 B per lane, 1 KiB per instruction, lane-linear in LDS), so the bank-conflict swizzle sits on
// the SOURCE side: the lane that fills physical 16-byte slot c of row r fetches logical chunk c ^ key(r), and a fragment read of logical chunk c of row r
// goes to slot c ^ key(r). Two images:
//   * 64-channel slices (conv_v3.h): 128-byte rows, 8 rows per DMA piece, key(r) = (r >> 1) & 7  -- conv_v2.h's image;
//   * 32-channel slices (conv_v4.h, conv_q.h; the ht32_ functions): 64-byte rows, 16 rows per DMA piece, key(r) = (r >> 2) & 3, the k-step (16 channels)
//     is bit 5 of the address: fragment of k-step ks = address ^ (ks * 32). 4 waves, tile = 32 NB couts x 128 TJW pixels.
// Quad row order with W >= 16 adds the parity of the IMAGE row to the key (conv_v4.h has the derivation); that term stays with the kernels.
// Out of range means "bit 31 of the byte offset" (bit 30 where conv_v3.h adds two offsets): beyond the buffer descriptor, the hardware writes zeros to LDS
// and moves no memory. A fragment whose pixel lies outside the image (or the problem) is read from a zero line of 128 bytes at zero_off instead.
#pragma once
#include "conv_v2.h"

// ---- every halo kernel -------------------------------------------------------------------------------------------------------------------------------
template <int TI, int TJ> __device__ __forceinline__ void ht_zero_acc(f32x16 (&acc)[TI][TJ]) {
#pragma unroll
  for (int a = 0; a < TI; a++)
#pragma unroll
    for (int b = 0; b < TJ; b++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;
}
// 3 x 3 neighbourhood of pixel (ho, wo) in an H x W image: bit rr * 3 + ss set = (ho - 1 + rr, wo - 1 + ss) is inside; 0 for a row beyond the problem
__device__ __forceinline__ unsigned ht_border_mask(int ho, int wo, int H, int W, bool in_problem) {
  unsigned m = 0;
  if (in_problem) {
#pragma unroll
    for (int rr = 0; rr < 3; rr++)
#pragma unroll
      for (int ss = 0; ss < 3; ss++)
        if ((unsigned)(ho - 1 + rr) < (unsigned)H && (unsigned)(wo - 1 + ss) < (unsigned)W) m |= 1u << (rr * 3 + ss);
  }
  return m;
}
// tile row -> (image, output row, output column): raster order, or quad order (SG_PIX_QUAD: the four pixels of a 2 x 2 pooling window are neighbours)
template <class P> __device__ __forceinline__ void ht_decode_pixel(const P& p, int row, int& n, int& ho, int& wo) {
  if (p.flags & SG_PIX_QUAD) {
    const int q = row >> 2, dy = (row >> 1) & 1, dx = row & 1;
    const int wq = q & ((p.Wo >> 1) - 1);
    const int t = q >> (p.wshift - 1);
    const int hq = t & ((p.Ho >> 1) - 1);
    n = t >> (p.hshift - 1);
    ho = 2 * hq + dy; wo = 2 * wq + dx;
  } else {
    wo = row & (p.Wo - 1); const int t = row >> p.wshift; ho = t & (p.Ho - 1); n = t >> p.hshift;
  }
}
// patch row of the centre tap of output pixel (n, ho, wo); P0 = raster index of patch row 0. UP (nearest x2 on load): the patch holds SOURCE pixels
template <bool UP, class P> __device__ __forceinline__ int ht_patch_row(const P& p, int n, int ho, int wo, int P0) {
  if (UP) {
    const int Hs = p.Ho >> 1;
    return ((n * Hs + (ho >> 1)) << p.wlog) + (wo >> 1) - P0;
  }
  return (((n << p.hshift) + ho) << p.wshift) + wo - P0;
}
// bias of this cout tile (+ the fused skip's bias2), once per workgroup into LDS; visible after the first barrier
template <int BI, int NT, bool SKIP> __device__ __forceinline__ void ht_stage_bias(float* sbias, const Epilogue<bf16_t>& epi, const float* bias2, int i0, int tid) {
  if (epi.bias) {
    for (int i = tid; i < BI; i += NT) {
      float b = (i0 + i < epi.I) ? epi.bias[i0 + i] : 0.f;
      if (SKIP && bias2 && i0 + i < epi.I) b += bias2[i0 + i];
      sbias[i] = b;
    }
  }
}
__device__ __forceinline__ void ht_zero_line(char* smem, int zero_off, int tid) {
  if (tid < 32) ((unsigned*)(smem + zero_off))[tid] = 0u;
}
// host: let `kernel` be launched with up to `bytes` of dynamic LDS. `done` is a static of the launcher: the attribute is set once per kernel, and a call
// that failed is made again at the next launch
template <typename K> static bool ht_allow_lds(bool& done, K kernel, int bytes) {
  if (!done) done = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
  return done;
}

// ---- the 32-channel family (conv_v4.h, conv_q.h): 4 waves, 64-byte LDS rows ---------------------------------------------------------------------------
// DMA piece = 1 KiB = 16 rows x 64 B, LDS linear in lane order: lane -> (row sub = lane >> 2, physical chunk lane & 3); the logical
// 16-byte chunk it fetches is the swizzle inverse: lc = (lane & 3) ^ (row >> 2 & 3), and row = 16 g + sub gives (sub >> 2) & 3.
__device__ __forceinline__ int ht32_sub(int lane) { return lane >> 2; }
__device__ __forceinline__ int ht32_chunk(int lane) { return (lane & 3) ^ ((lane >> 4) & 3); }
// weight DMA: per-lane byte offsets of the (at most two) 16-row pieces of a [I][K] weight matrix this wave fetches per tile, once per workgroup;
// the (tap, slice) position rides in the instruction's scalar offset `so`
__device__ __forceinline__ void ht32_weight_offsets(unsigned (&wvo)[2], int i0, int wave, int sub, int lc, int I, int K) {
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int row = i0 + 16 * (wave + 4 * i) + sub;
    wvo[i] = (row < I) ? ((unsigned)row * (unsigned)K + (unsigned)(lc * 8)) * 2u : 0x80000000u;
  }
}
// one weight tile = NWP pieces (32 NB / 16). (w, wbytes: the matrix and its extent, as the kernel's own descriptor has them -- a buffer descriptor cannot be a
// function parameter)
template <int NWP> __device__ __forceinline__ void ht32_weight_tile(const bf16_t* w, unsigned wbytes, char* dst, const unsigned (&wvo)[2], int wave, int so) {
  const auto rsw = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, (int)wbytes, 0x00020000);
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const int g = wave + 4 * i;
    if (g < NWP) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (sg_lptr_t)(dst + g * 1024), 16, (int)wvo[i], so, 0, 0);
  }
}
// the fused skip's weight tile: slice s2 (32 channels) of the [I][C2] 1 x 1 filter, offsets on the fly (one tile per slice)
template <int NWP, class P> __device__ __forceinline__ void ht32_skip_weight_tile(char* dst, const P& p, int i0, int wave, int sub, int lc, int s2) {
  const auto rsw2 = __builtin_amdgcn_make_buffer_rsrc((void*)p.w2, 0, (int)p.w2bytes, 0x00020000);
  for (int g = wave; g < NWP; g += 4) {
    const int row = i0 + 16 * g + sub;
    unsigned off = ((unsigned)row * (unsigned)p.C2 + (unsigned)(s2 * 32 + lc * 8)) * 2u;
    off = (row < p.I) ? off : 0x80000000u;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw2, (sg_lptr_t)(dst + g * 1024), 16, (int)off, 0, 0, 0);
  }
}
// weight fragment addresses inside a weight tile: row = cout a * 32 + frow, chunk (ks * 2 + fhi) ^ (row >> 2 & 3); ks = 1 is the address ^ 32
template <int TI> __device__ __forceinline__ void ht32_weight_frag_addr(unsigned (&wa)[TI], int frow, int fhi) {
#pragma unroll
  for (int a = 0; a < TI; a++) {
    const int row = a * 32 + frow;
    wa[a] = (unsigned)(row * 64 + ((fhi ^ ((row >> 2) & 3)) << 4));
  }
}
// k-step ks (16 of the slice's 32 channels): weight fragments from the tile at ps, pixel fragments from byte offsets qa of smem (patch or zero line),
// ReLU on load, TI x TJ MFMAs. pb (conv_q.h's double-buffered patch): added to the offsets below zlim, i.e. to all but the zero line's
template <bool RELU, int TI, int TJ>
__device__ __forceinline__ void ht32_kstep(f32x16 (&acc)[TI][TJ], const char* ps, const unsigned (&wa)[TI], const char* smem, const unsigned (&qa)[TJ], int ks, bool relu = true,
                                           unsigned pb = 0u, unsigned zlim = 0u) {
  bf16x8_t pf[TI], qf[TJ];
#pragma unroll
  for (int a = 0; a < TI; a++) {
    u32x4 v = *(const u32x4*)(ps + (wa[a] ^ (unsigned)(ks * 32)));
    pf[a] = __builtin_bit_cast(bf16x8_t, v);
  }
#pragma unroll
  for (int b = 0; b < TJ; b++) {
    unsigned qaddr = qa[b] ^ (unsigned)(ks * 32);
    qaddr += (qaddr < zlim) ? pb : 0u;
    u32x4 v = *(const u32x4*)(smem + qaddr);
    if (RELU && relu) v = relu16<bf16_t>(v);
    qf[b] = __builtin_bit_cast(bf16x8_t, v);
  }
#pragma unroll
  for (int a = 0; a < TI; a++)
#pragma unroll
    for (int b = 0; b < TJ; b++)
      acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pf[a], qf[b], acc[a][b], 0, 0, 0);
}
// host: LDS layout and need (bytes) of a workgroup: [patch(es) up to wgt_off | nbuf weight tiles], overlaid by the staged BJ-row output tile and by
// `other` bytes (the fused skip's staging slots); behind it the zero line (128 B) and the bias vector (BI floats)
static inline int ht32_lds(int BI, int BJ, int wgt, int nbuf, int other, int* wgt_off, int* zero_off, int* bias_off) {
  const int ops = wgt + nbuf * BI * 64;
  const int stage = BJ * (BI * 2 + 16);
  int body = ops > stage ? ops : stage;
  if (other > body) body = other;
  if (wgt_off) *wgt_off = wgt;
  if (zero_off) *zero_off = body;
  if (bias_off) *bias_off = body + 128;
  return body + 128 + BI * 4;
}
