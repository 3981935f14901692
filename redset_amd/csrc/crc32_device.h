// crc32_device.h -- the CRC-32 table layout of crc_device_tables() and the
// device arithmetic on remainders (crc32.h) shared by the kernels that run a
// CRC: crc32_kernels.hip, encode_crc_kernels.hip and verify_crc_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "crc32.h"

namespace redset_hip {

namespace {

constexpr unsigned kPoly = 0xEDB88320u;
// crc_device_tables(): kSliceTables slicing tables (table k: the byte followed
// by k zero bytes), then per fold level lv four 256-entry tables that advance
// a remainder by kCrcSeg << lv bytes
constexpr int kSliceTables = 16;
constexpr int kFoldLevels = 8;  // 2^8 = kCrcLanes segments
constexpr int kSliceWords = kSliceTables * 256;
constexpr int kFoldWords = 4 * 256;
constexpr int kTableWords = kSliceWords + kFoldLevels * kFoldWords;

__device__ __forceinline__ unsigned mulmod_dev(unsigned a, unsigned b) {
  unsigned p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= (a & 0x80000000u) ? b : 0u;
    a <<= 1;
    b = (b >> 1) ^ ((b & 1u) ? kPoly : 0u);
  }
  return p;
}

// 16 more bytes through the register
__device__ __forceinline__ unsigned step16(const unsigned* sl, unsigned crc, uint4 w) {
  const unsigned a = w.x ^ crc, b = w.y, c = w.z, d = w.w;
  return sl[15 * 256 + (a & 255u)] ^ sl[14 * 256 + ((a >> 8) & 255u)] ^ sl[13 * 256 + ((a >> 16) & 255u)] ^
         sl[12 * 256 + (a >> 24)] ^ sl[11 * 256 + (b & 255u)] ^ sl[10 * 256 + ((b >> 8) & 255u)] ^
         sl[9 * 256 + ((b >> 16) & 255u)] ^ sl[8 * 256 + (b >> 24)] ^ sl[7 * 256 + (c & 255u)] ^
         sl[6 * 256 + ((c >> 8) & 255u)] ^ sl[5 * 256 + ((c >> 16) & 255u)] ^ sl[4 * 256 + (c >> 24)] ^
         sl[3 * 256 + (d & 255u)] ^ sl[2 * 256 + ((d >> 8) & 255u)] ^ sl[1 * 256 + ((d >> 16) & 255u)] ^
         sl[0 * 256 + (d >> 24)];
}

// a remainder advanced by one fold level's byte count
__device__ __forceinline__ unsigned advance(const unsigned* t, unsigned r) {
  return t[r & 255u] ^ t[256 + ((r >> 8) & 255u)] ^ t[512 + ((r >> 16) & 255u)] ^ t[768 + (r >> 24)];
}

}  // namespace

}  // namespace redset_hip
