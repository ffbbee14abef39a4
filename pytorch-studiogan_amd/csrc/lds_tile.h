// lds_tile.h -- the [rows][32 channels] bf16 tile image in LDS that attn.hip, mha.hip and vit.hip feed their MFMAs from, and the fragment / statistics
// helpers of the kernels built on it.
//
// Image: 64-byte rows, 16 rows per 1 KiB group, written by LDS-DMA (global_load_lds, 16 B per lane, lane-linear inside a group: lane = 4 * row + chunk).
// The lane fetches logical 16-byte chunk (lane & 3) ^ ((row >> 2) & 3) -- the XOR sits on the SOURCE side -- so that logical chunk c of row r lives in
// slot c ^ ((r >> 2) & 3) and both the ds_read_b128 of lt_frag and the transposing ds_read_b64_tr_b16 of lt_vfrag are bank-conflict free
// (MI355X_MICROARCH.md §LDS). Fetches that fall outside the matrix come from a 64-byte zero line, never from beyond the tensor.
#pragma once
#include "common.h"

typedef __attribute__((address_space(1))) const void* lt_gptr_t;
typedef __attribute__((address_space(3))) void* lt_lptr_t;

static __device__ u32x4 lt_zero[4];

// `rows` rows (a multiple of 16) x 32 channels starting at channel c0 of a [rows][ld] matrix, by NW waves; 8-channel chunks at or beyond C are zeros
template <int NW> __device__ __forceinline__ void lt_stage_cols(char* img, const bf16_t* src, int rows, int ld, int c0, int C, int wave, int lane) {
  const int r16 = lane >> 2;
  const int chunk = (lane & 3) ^ ((lane >> 4) & 3);     // logical 16-byte chunk this lane fetches (row >> 2 == lane >> 4 inside a group)
  const int c = c0 + chunk * 8;
  for (int g = wave; g < rows / 16; g += NW) {
    const int row = g * 16 + r16;
    const bf16_t* p = (c < C) ? (src + (long long)row * ld + c) : (const bf16_t*)lt_zero;
    __builtin_amdgcn_global_load_lds((lt_gptr_t)p, (lt_lptr_t)(img + g * 1024), 16, 0, 0);
  }
}
// 128 rows row0 .. x 32 channels starting at channel c0 of a [.][ld] matrix, by 4 waves; rows >= nrows are zeros
__device__ __forceinline__ void lt_stage_rows(char* img, const bf16_t* src, int row0, int nrows, int ld, int c0, int wave, int lane) {
  const int r16 = lane >> 2;
  const int chunk = (lane & 3) ^ ((lane >> 4) & 3);
#pragma unroll
  for (int g = wave; g < 8; g += 4) {
    const int row = row0 + g * 16 + r16;
    const bf16_t* p = (row < nrows) ? (src + (long long)row * ld + c0 + chunk * 8) : (const bf16_t*)lt_zero;
    __builtin_amdgcn_global_load_lds((lt_gptr_t)p, (lt_lptr_t)(img + g * 1024), 16, 0, 0);
  }
}
// Ordering rule of LDS-DMA: the data is visible to a ds_read only after the ISSUING wave's vmcnt has retired the load and the reader has passed a barrier
// behind that. Every wave -- one that skips the arithmetic in between included -- therefore drains its own DMA right in front of the barrier, explicitly:
// nothing that calls this relies on where the compiler happens to place its own waits. (The asm is also a scheduling barrier.)
__device__ __forceinline__ void lt_drain_barrier() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
// MFMA 32x32x16 A / B fragment: image rows row0 + (lane & 31), k = 8 channels starting at 16 t + 8 h of the staged 32 (h = lane >> 5)
__device__ __forceinline__ bf16x8_t lt_frag_rows(const char* img, int row0, int t, int lane) {
  const int row = row0 + (lane & 31);
  const int slot = (2 * t + (lane >> 5)) ^ ((row >> 2) & 3);
  const u32x4 v = *(const u32x4*)(img + row * 64 + slot * 16);
  return __builtin_bit_cast(bf16x8_t, v);
}
// the same with the first row given as a 32-row block index. (Not written as lt_frag_rows(img, kb * 32, ..): hipcc then schedules k_mha_fwd and the
// attention kernels differently from their code objects as measured; the two bodies must stay the same swizzle.)
__device__ __forceinline__ bf16x8_t lt_frag(const char* img, int kb, int t, int lane) {
  const int row = kb * 32 + (lane & 31);
  const int slot = (2 * t + (lane >> 5)) ^ ((row >> 2) & 3);
  const u32x4 v = *(const u32x4*)(img + row * 64 + slot * 16);
  return __builtin_bit_cast(bf16x8_t, v);
}
// transposed fragment: channel = lane & 31 of this 32-channel image, rows kbase .. kbase + 3 (elements 0-3) and kbase + 8 .. + 11 (elements 4-7), by
// ds_read_b64_tr_b16; kbase is a multiple of 4, so the four rows one 16-lane group reads share their swizzle key
__device__ __forceinline__ bf16x8_t lt_vfrag(const char* img, int kbase, int lane) {
  const int g16 = lane >> 4, t = lane & 15;
  const int row = kbase + (t >> 2);
  const int slot = (2 * (g16 & 1) + ((t & 3) >> 1)) ^ ((row >> 2) & 3);
  const char* p = img + row * 64 + slot * 16 + 8 * (t & 1);
  const int slot2 = (2 * (g16 & 1) + ((t & 3) >> 1)) ^ (((row + 8) >> 2) & 3);
  const char* p2 = img + (row + 8) * 64 + slot2 * 16 + 8 * (t & 1);
  const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p);
  const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p2);
  s16x8 r;
  r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3];
  r[4] = b[0]; r[5] = b[1]; r[6] = b[2]; r[7] = b[3];
  return __builtin_bit_cast(bf16x8_t, r);
}
// exchange between the two lane halves of a wave (lanes l and l + 32 hold the same query / key): v_permlane32_swap_b32 (gfx950) swaps lanes 32-63 of one
// register with lanes 0-31 of another in the vector pipe; with both registers = v, every lane ends up holding {its own value, its partner's} in the pair, in
// either order -- which a maximum or a sum does not care about. (__shfl_xor(v, 32) is a ds_bpermute_b32: an LDS round trip on the per-block
// MFMA -> max -> exp -> MFMA chain of the streaming forward.)
__device__ __forceinline__ float lt_half_max(float v) {
  const uint32_t u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float lt_half_sum(float v) {
  const uint32_t u = __float_as_uint(v);
  const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// host: let `kernel` be launched with up to `bytes` of dynamic LDS (call once: `static const bool ok = lt_allow_lds(...)`)
template <typename K> static bool lt_allow_lds(K kernel, int bytes) {
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
}
