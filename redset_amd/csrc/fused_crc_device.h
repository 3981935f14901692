// fused_crc_device.h -- what the kernels that run a CRC-32 from the registers
// of a codec pass share (encode_crc_kernels.hip, verify_crc_kernels.hip): the
// shape of a block's tile -- rows of 1 KiB, one 16-B vector per lane, four
// waves of 32 rows -- its LDS image, and the lane's per-row remainder step.
#pragma once

#include "codec_device.h"
#include "crc32_device.h"

namespace redset_hip {

namespace {

constexpr int kEcRowVecs = 64;                                // a row: one vector per lane
constexpr int kEcTileRows = kCrcTile / (16 * kEcRowVecs);     // 128
constexpr int kEcWaveRows = kEcTileRows / (kCrcLanes / 64);   // 32
constexpr int kEcSegVecs = kCrcSeg / 16;
constexpr int kEcGfWords = kMaxIn * kTableBytes / 4;          // 2 KiB
constexpr int kEcAdvLevel = 1;                                // kCrcSeg << 1 = a row
constexpr int kEcLdsWords = kEcGfWords + kSliceWords + kFoldWords;
static_assert((kCrcSeg << kEcAdvLevel) == 16 * kEcRowVecs, "the fold level advances by one row");
static_assert(kCrcLanes == 256 && kEcWaveRows == 32, "four waves of 32 rows");

// the lane's remainder of one cell after one more row
__device__ __forceinline__ unsigned ec_row(const unsigned* sl, const unsigned* adv, unsigned rem, const v4u& x) {
  return advance(adv, rem) ^ step16(sl, 0u, make_uint4(x.x, x.y, x.z, x.w));
}

__device__ __forceinline__ v4u ec_gather(const uint32_t (&acc)[16], int j) {
  v4u r;
  r.x = gather_byte(acc[0], acc[1], acc[2], acc[3], j);
  r.y = gather_byte(acc[4], acc[5], acc[6], acc[7], j);
  r.z = gather_byte(acc[8], acc[9], acc[10], acc[11], j);
  r.w = gather_byte(acc[12], acc[13], acc[14], acc[15], j);
  return r;
}

// inputs [I0, I0 + N) at vector `at` of their cells
template <int I0, int N, int NIN>
__device__ __forceinline__ void ec_load(v4u (&x)[N], g_cu4* const (&in)[NIN], long long at) {
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = __builtin_nontemporal_load(in[I0 + i] + at);
}

}  // namespace

}  // namespace redset_hip
