// crc32.h -- zlib CRC-32 of byte ranges in device memory: the launch
// descriptors shared by the kernels (crc32_kernels.hip), the plan
// (redset_hip.cpp) and the streaming pipeline (stream_pipeline.cpp), and the
// host arithmetic on CRC remainders.
//
// A remainder is the CRC register (reflected, polynomial 0xEDB88320) run over
// some bytes from register 0 with no final XOR: linear over GF(2), unchanged
// by leading zero bytes, and raw(A || B) = raw(A) * x^(8 len B) + raw(B)
// modulo the polynomial. zlib's value is raw(M) ^ crc_xinit(len M).
#pragma once

#include <cstddef>
#include <cstdint>

namespace redset_hip {

// A range is cut, on the grid of 16-B aligned addresses starting at its
// pointer rounded down, into segments of kCrcSeg bytes; the segments that end
// inside the range are the lanes' work, kCrcLanes per tile, and the < kCrcSeg
// + 16 bytes after the last of them are the range's tail (crc32_kernels.hip).
constexpr int kCrcSeg = 512;
constexpr int kCrcLanes = 256;
constexpr size_t kCrcTile = static_cast<size_t>(kCrcSeg) * kCrcLanes;

struct CrcRange {
  const uint8_t* ptr;
  unsigned long long len;
  unsigned xinit;   // crc_xinit(len): what the initial and the final XOR add to the remainder
  unsigned xchunk;  // x^(8 * kCrcTile * c), c = tiles per lane of the finishing wave
};

// One execute over ranges [0, nranges): tiles [tile0, tile0 + ntiles) in the
// numbering of tile_base (tile_base[r] = first tile of range r, nranges + 1
// entries; the pointers may point into longer tables).
struct CrcLaunch {
  const CrcRange* ranges;  // device
  const int* tile_base;    // device
  int nranges;
  int tile0, ntiles;
  unsigned* rem;           // device: one remainder per tile, indexed by tile number
  unsigned* crcs;          // device: one CRC per range
  const unsigned* tables;  // device: crc_device_tables()
  unsigned xtile;          // x^(8 * kCrcTile)
};

// a * b and x^(8 n) modulo the polynomial (bit 31 = x^0)
unsigned crc_mulmod(unsigned a, unsigned b);
unsigned crc_xpow8(unsigned long long nbytes);
unsigned crc_xinit(unsigned long long len);
// tiles of a range, and its descriptor
unsigned long long crc_tiles(const void* ptr, unsigned long long len);
CrcRange crc_range(const void* ptr, unsigned long long len);
// the current device's lookup tables (uploaded once per device, kept; not for
// the execute path); nullptr on failure
const unsigned* crc_device_tables();
// both kernels of one execute on `stream`; returns hipError_t as int
int launch_crc32(const CrcLaunch& L, void* stream);

}  // namespace redset_hip
