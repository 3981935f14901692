// crc32_kernels.hip -- zlib CRC-32 of byte ranges in device memory (gfx950).
//
// gfx950 has no carry-less multiply, so the CRC runs on lookup tables in LDS.
// A range is cut into segments of kCrcSeg bytes on its 16-B aligned address
// grid (crc32.h). crc32_tiles_kernel: every lane runs the slicing-by-16
// recurrence over one segment with 16-B loads (the one segment a range may
// enter mid-vector takes its first 16 bytes byte by byte), from register 0, so
// bytes that are not there at the FRONT of a segment or a tile cost nothing: a
// range's short tile is its first, filled from the last lane down. The 256
// remainders of a tile are folded with "advance by 2^k segments" operators
// (four 256-entry tables per level, in LDS beside the slicing tables): six
// levels of wave shuffles, two over the block's four waves. One remainder
// per tile goes to scratch. crc32_finish_kernel, after the launch boundary:
// one wave per range folds the range's tile remainders (multiplication by
// powers of x modulo the polynomial, 32 shift-and-XOR steps), runs the
// range's tail bytes and adds what the initial and final XOR contribute.
//
// No block waits on another: a block's tiles are its own, the only ordering
// between blocks is the boundary between the two launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "codec_kernels.h"
#include "crc32.h"

namespace redset_hip {

namespace {

constexpr unsigned kPoly = 0xEDB88320u;
constexpr int kSliceTables = 16;
constexpr int kFoldLevels = 8;  // 2^8 = kCrcLanes segments
constexpr int kSliceWords = kSliceTables * 256;
constexpr int kTableWords = kSliceWords + kFoldLevels * 4 * 256;
static_assert(kCrcLanes == 256 && kCrcSeg % 64 == 0, "the fold is written for 4 waves of 64 lanes");

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

// the 16 bytes at `a` (16-B aligned) with those before `first` read as zero
__device__ uint4 load16_from(const uint8_t* a, uintptr_t first) {
  unsigned w[4] = {0, 0, 0, 0};
  for (int b = 0; b < 16; ++b)
    if (reinterpret_cast<uintptr_t>(a + b) >= first) w[b >> 2] |= static_cast<unsigned>(a[b]) << (8 * (b & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// full segments of a range (crc32.h)
__device__ __forceinline__ unsigned long long segments_of(uintptr_t p0, unsigned long long len) {
  return (p0 + len - (p0 & ~static_cast<uintptr_t>(15))) / kCrcSeg;
}

__global__ __launch_bounds__(kCrcLanes) void crc32_tiles_kernel(CrcLaunch L) {
  __shared__ __attribute__((aligned(16))) unsigned tab[kTableWords];
  __shared__ unsigned wave_rem[kCrcLanes / 64];
  {
    const uint4* src = reinterpret_cast<const uint4*>(L.tables);
    uint4* dst = reinterpret_cast<uint4*>(tab);
    for (int i = threadIdx.x; i < kTableWords / 4; i += kCrcLanes) dst[i] = src[i];
  }
  __syncthreads();
  const unsigned* sl = tab;
  const unsigned* fold = tab + kSliceWords;
  const int lane = threadIdx.x;
  for (int t = blockIdx.x; t < L.ntiles; t += gridDim.x) {
    const int gt = L.tile0 + t;
    // the range of tile gt: the last r with tile_base[r] <= gt
    int lo = 0, hi = L.nranges;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (L.tile_base[mid] <= gt) lo = mid;
      else hi = mid;
    }
    const CrcRange R = L.ranges[lo];
    const long long k = gt - L.tile_base[lo];
    const uintptr_t p0 = reinterpret_cast<uintptr_t>(R.ptr), a0 = p0 & ~static_cast<uintptr_t>(15);
    const long long nseg = static_cast<long long>(segments_of(p0, R.len));
    const long long ntiles = (nseg + kCrcLanes - 1) / kCrcLanes;
    // the range's first tile holds the odd segments, in its last lanes
    const long long seg = k * kCrcLanes + lane - (ntiles * kCrcLanes - nseg);
    unsigned crc = 0;
    if (seg >= 0 && seg < nseg) {
      const uint8_t* s = reinterpret_cast<const uint8_t*>(a0) + seg * kCrcSeg;
      const uint4* v = reinterpret_cast<const uint4*>(s);
      const bool head = seg == 0 && p0 != a0;
      for (int g = 0; g < kCrcSeg / 64; ++g) {
        uint4 w[4];
        if (g == 0 && head) {
          w[0] = load16_from(s, p0);
        } else {
          w[0] = v[4 * g];
        }
        w[1] = v[4 * g + 1];
        w[2] = v[4 * g + 2];
        w[3] = v[4 * g + 3];
        crc = step16(sl, crc, w[0]);
        crc = step16(sl, crc, w[1]);
        crc = step16(sl, crc, w[2]);
        crc = step16(sl, crc, w[3]);
      }
    }
    // lane 63 of a wave: the wave's 64 segments
    for (int lv = 0; lv < 6; ++lv) {
      const unsigned left = __shfl_up(crc, 1u << lv, 64);
      crc ^= advance(fold + lv * 1024, left);
    }
    if ((lane & 63) == 63) wave_rem[lane >> 6] = crc;
    __syncthreads();
    if (lane == 0) {
      const unsigned r01 = advance(fold + 6 * 1024, wave_rem[0]) ^ wave_rem[1];
      const unsigned r23 = advance(fold + 6 * 1024, wave_rem[2]) ^ wave_rem[3];
      L.rem[gt] = advance(fold + 7 * 1024, r01) ^ r23;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void crc32_finish_kernel(CrcLaunch L) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const CrcRange R = L.ranges[r];
  const int t0 = L.tile_base[r], nt = L.tile_base[r + 1] - t0;
  // lane j folds c tiles in order, the last lane the range's last
  const long long c = (nt + 63) / 64;
  const long long end = nt - (63 - lane) * c;
  unsigned acc = 0;
  for (long long k = end - c > 0 ? end - c : 0; k < end; ++k) acc = mulmod_dev(acc, L.xtile) ^ L.rem[t0 + k];
  unsigned m = R.xchunk;
  for (int lv = 0; lv < 6; ++lv) {
    const unsigned left = __shfl_up(acc, 1u << lv, 64);
    acc ^= mulmod_dev(left, m);
    m = mulmod_dev(m, m);
  }
  if (lane != 63) return;
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(R.ptr), a0 = p0 & ~static_cast<uintptr_t>(15);
  const unsigned long long nseg = segments_of(p0, R.len);
  const uint8_t* q = nseg ? reinterpret_cast<const uint8_t*>(a0) + nseg * kCrcSeg : R.ptr;
  const uint8_t* const stop = R.ptr + R.len;
  for (; q < stop; ++q) acc = L.tables[(acc ^ *q) & 255u] ^ (acc >> 8);
  L.crcs[r] = acc ^ R.xinit;
}

std::vector<unsigned> host_tables() {
  std::vector<unsigned> t(kTableWords);
  for (unsigned b = 0; b < 256; ++b) {
    unsigned c = b;
    for (int i = 0; i < 8; ++i) c = (c & 1u) ? (c >> 1) ^ kPoly : c >> 1;
    t[b] = c;
  }
  // table k: the byte followed by k zero bytes
  for (int k = 1; k < kSliceTables; ++k)
    for (unsigned b = 0; b < 256; ++b) {
      const unsigned c = t[(k - 1) * 256 + b];
      t[k * 256 + b] = (c >> 8) ^ t[c & 255u];
    }
  for (int lv = 0; lv < kFoldLevels; ++lv) {
    const unsigned x = crc_xpow8(static_cast<unsigned long long>(kCrcSeg) << lv);
    for (int j = 0; j < 4; ++j)
      for (unsigned b = 0; b < 256; ++b) t[kSliceWords + (lv * 4 + j) * 256 + b] = crc_mulmod(b << (8 * j), x);
  }
  return t;
}

}  // namespace

unsigned crc_mulmod(unsigned a, unsigned b) {
  unsigned p = 0;
  for (int i = 0; i < 32 && a; ++i) {
    if (a & 0x80000000u) p ^= b;
    a <<= 1;
    b = (b & 1u) ? (b >> 1) ^ kPoly : b >> 1;
  }
  return p;
}

unsigned crc_xpow8(unsigned long long nbytes) {
  unsigned p = 0x80000000u, sq = 0x00800000u;  // 1, x^8
  for (; nbytes; nbytes >>= 1) {
    if (nbytes & 1u) p = crc_mulmod(p, sq);
    sq = crc_mulmod(sq, sq);
  }
  return p;
}

unsigned crc_xinit(unsigned long long len) { return crc_mulmod(0xFFFFFFFFu, crc_xpow8(len)) ^ 0xFFFFFFFFu; }

unsigned long long crc_tiles(const void* ptr, unsigned long long len) {
  const uintptr_t p0 = reinterpret_cast<uintptr_t>(ptr);
  const unsigned long long nseg = (p0 + len - (p0 & ~static_cast<uintptr_t>(15))) / kCrcSeg;
  return (nseg + kCrcLanes - 1) / kCrcLanes;
}

CrcRange crc_range(const void* ptr, unsigned long long len) {
  const unsigned long long c = (crc_tiles(ptr, len) + 63) / 64;
  return CrcRange{static_cast<const uint8_t*>(ptr), len, crc_xinit(len), crc_xpow8(c * kCrcTile)};
}

const unsigned* crc_device_tables() {
  static std::mutex mu;
  static unsigned* tables[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> g(mu);
  if (!tables[dev]) {
    const std::vector<unsigned> t = host_tables();
    void* d = nullptr;
    if (hipMalloc(&d, t.size() * sizeof(unsigned)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, t.data(), t.size() * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess) {
      (void) hipFree(d);
      return nullptr;
    }
    tables[dev] = static_cast<unsigned*>(d);
  }
  return tables[dev];
}

int launch_crc32(const CrcLaunch& L, void* stream) {
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (L.nranges <= 0) return hipSuccess;
  if (L.ntiles > 0) {
    // three blocks of 48 KiB of LDS a CU
    const int grid = std::min(L.ntiles, 3 * device_cu_count());
    hipLaunchKernelGGL(crc32_tiles_kernel, dim3(grid), dim3(kCrcLanes), 0, s, L);
    if (hipError_t e = hipGetLastError()) return e;
  }
  hipLaunchKernelGGL(crc32_finish_kernel, dim3(L.nranges), dim3(64), 0, s, L);
  return hipGetLastError();
}

}  // namespace redset_hip
