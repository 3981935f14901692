// encode_crc_kernels.hip -- encode a set and take the zlib CRC-32 of all its
// cells in one read (gfx950); descriptors in encode_crc.h.
//
// encode_crc_kernel<NIN, NOUT, XOR>: block (stripe, tile) of 256 threads takes
// one 128 KiB tile (kCrcTile, the grid of crc32.h: the range's short tile is
// its first, filled from the back) of every cell of one stripe. A row is
// 1 KiB: lane j of a wave holds the 16-B vector at column j of the row for
// each of the NIN data cells (direct global loads, the next row's issued
// before this row's arithmetic; stripes of more than kRingChunk inputs in two
// chunks), forms the NOUT parity vectors with the codec's nibble tables
// (codec_device.h; XOR: a plain XOR) and stores them non-temporally. Wave w
// walks rows 32 w .. 32 w + 31 of the tile.
//
// The CRC is taken from those registers. A lane keeps one running remainder
// per cell, of the sparse byte stream "my vectors, zero elsewhere":
//   rem = rem * x^(8 * 1024) + raw(vector)
// -- the "advance by 2 segments" fold level (4 lookups) and the 16 slicing
// tables from register 0 (16 lookups) of crc_device_tables(), copied to LDS
// beside the GF tables: 2 + 16 + 4 KiB. The CRC is linear, so the tile's
// remainder is the XOR of the lanes' streams, each first moved to the tile's
// end: one multiplication by a power of x per (thread, cell) and tile -- the
// 256 powers come from the host (encode_crc_xpow) -- then wave shuffles and
// four words through LDS. One remainder per (cell, tile) goes to the plan's
// scratch, exactly what crc32_tiles_kernel writes for the range (cell, C), and
// crc32_finish_kernel finishes every cell unchanged after the launch boundary:
// it folds the tiles, runs the < 512 tail bytes from memory, adds crc_xinit.
//
// Bytes [512 * (C / 512), C) of the parity cells belong to no tile: the block
// of the stripe's last tile forms them, whole vectors as above and the last
// C % 16 bytes one by one. Only bytes [0, C) of a parity cell are written.
//
// No block waits on another: no ring, no claim counter, no spin, and the
// kernel has no access to the ring-fault and hang-fault words.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "encode_crc.h"
#include "fused_crc_device.h"

namespace redset_hip {

namespace {

// waves per SIMD the kernels are compiled for (the cap on their VGPRs): what
// every instantiation reaches without scratch
constexpr int ec_waves(int nin) { return nin <= kRingChunk ? 4 : 3; }

// The combine of one 16-B position: begin(), add<I0>(x, ok) for inputs
// [I0, I0 + N) -- each also goes through its cell's remainder -- then
// finish(at, ok) stores the outputs and runs them through theirs. ok: the
// lane's position lies in the cell; where it does not, the remainders stay 0.
template <int NIN, int NOUT, bool XOR>
struct EcAcc {
  const uint32_t* gf;
  const unsigned* sl;
  const unsigned* adv;
  g_u4* out[NOUT];
  unsigned rem[NIN + NOUT];
  uint32_t acc[16];
  v4u xr;

  __device__ __forceinline__ void begin() {
    if constexpr (XOR) {
      xr = v4u{0, 0, 0, 0};
    } else {
#pragma unroll
      for (int b = 0; b < 16; ++b) acc[b] = 0;
    }
  }
  template <int I0, int N>
  __device__ __forceinline__ void add(const v4u (&x)[N], bool ok) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if constexpr (XOR) xr ^= x[i];
      else gf_acc_input<0>(gf, x[i], I0 + i, acc);
      const unsigned next = ec_row(sl, adv, rem[I0 + i], x[i]);
      rem[I0 + i] = ok ? next : 0u;
      // with nothing but lookups to order, the scheduler would start every
      // input's at once and spill what they return
      if constexpr (XOR) __builtin_amdgcn_sched_barrier(0);
    }
  }
  __device__ __forceinline__ void finish(long long at, bool ok) {
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
      v4u r;
      if constexpr (XOR) r = xr;
      else r = ec_gather(acc, j);
      store_vec(out[j], static_cast<size_t>(at), r);
      const unsigned next = ec_row(sl, adv, rem[NIN + j], r);
      rem[NIN + j] = ok ? next : 0u;
    }
  }
};

template <int NIN, int NOUT, bool XOR>
__global__ __launch_bounds__(kCrcLanes) __attribute__((amdgpu_waves_per_eu(ec_waves(NIN), ec_waves(NIN)))) void
encode_crc_kernel(EncodeCrcLaunch L) {
  constexpr int NC = NIN + NOUT;
  constexpr int N0 = NIN < kRingChunk ? NIN : kRingChunk, N1 = NIN - N0;
  __shared__ __attribute__((aligned(16))) unsigned lds[kEcLdsWords];
  __shared__ unsigned wave_rem[kCrcLanes / 64][NC];
  const int T = L.tiles > 0 ? L.tiles : 1;
  const int job = blockIdx.x / T, k = blockIdx.x - job * T;
  const GfJob& J = L.jobs[job];
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);

  if constexpr (!XOR) build_tables(lds, J, NIN, NOUT);
  if (L.tiles > 0) {
    uint4* dst = reinterpret_cast<uint4*>(lds + kEcGfWords);
    const uint4* sl = reinterpret_cast<const uint4*>(L.tables);
    const uint4* ad = reinterpret_cast<const uint4*>(L.tables + kSliceWords + kEcAdvLevel * kFoldWords);
    for (int i = tid; i < kSliceWords / 4; i += kCrcLanes) dst[i] = sl[i];
    for (int i = tid; i < kFoldWords / 4; i += kCrcLanes) dst[kSliceWords / 4 + i] = ad[i];
  }
  __syncthreads();

  const long long nseg = static_cast<long long>(L.nbytes / kCrcSeg);
  if (L.tiles > 0) {
    EcAcc<NIN, NOUT, XOR> A;
    A.gf = lds;
    A.sl = lds + kEcGfWords;
    A.adv = lds + kEcGfWords + kSliceWords;
    g_cu4* in[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) in[i] = (g_cu4*) (J.in[i]);
#pragma unroll
    for (int j = 0; j < NOUT; ++j) A.out[j] = (g_u4*) (J.out[j]);
#pragma unroll
    for (int c = 0; c < NC; ++c) A.rem[c] = 0;

    // The first tile lacks `pad` segments at its front: its rows before
    // pad / 2 are not there, and of row pad / 2 the first half when pad is
    // odd. The lanes of that half row keep the loop free of branches: they
    // work at vector 0 of the cells, which lane 32 of the same row owns --
    // they load what it loads and store, to the same bytes of the parity
    // cells, what it stores -- and their remainders stay 0.
    const long long pad = static_cast<long long>(L.tiles) * kCrcLanes - nseg;
    const long long vb = (static_cast<long long>(k) * kCrcLanes - pad) * kEcSegVecs + lane;  // row 0 of the tile
    const int first = k == 0 ? static_cast<int>(pad / 2) : 0;
    const int r1 = (w + 1) * kEcWaveRows;
    int r = std::max(w * kEcWaveRows, first);
    if (r < r1) {
      v4u x0[N0];
      ec_load<0, N0>(x0, in, std::max(0ll, vb + static_cast<long long>(r) * kEcRowVecs));
      for (; r < r1; ++r) {
        const long long v = vb + static_cast<long long>(r) * kEcRowVecs;
        const bool ok = v >= 0;
        const long long at = ok ? v : 0;
        // after the wave's last row: that row again, loaded and not used
        const long long next = r + 1 < r1 ? v + kEcRowVecs : at;
        A.begin();
        if constexpr (N1 > 0) {
          v4u x1[N1];
          ec_load<N0, N1>(x1, in, at);
          A.template add<0>(x0, ok);
          ec_load<0, N0>(x0, in, next);
          A.template add<N0>(x1, ok);
        } else {
          v4u nx[N0];
          ec_load<0, N0>(nx, in, next);
          A.template add<0>(x0, ok);
#pragma unroll
          for (int i = 0; i < N0; ++i) x0[i] = nx[i];
        }
        A.finish(at, ok);
      }
    }

    // every stream to the tile's end, then their XOR: shuffles, 4 words via LDS
    // (mulmod_dev for all the cells at once: they share the multiplier's steps)
    unsigned xp = L.xpow[tid];
    unsigned m[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) m[c] = 0;
#pragma unroll 1
    for (int i = 0; i < 32; ++i) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        m[c] ^= (A.rem[c] & 0x80000000u) ? xp : 0u;
        A.rem[c] <<= 1;
      }
      xp = (xp >> 1) ^ ((xp & 1u) ? kPoly : 0u);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) m[c] ^= __shfl_xor(m[c], s, 64);
      if (lane == 0) wave_rem[w][c] = m[c];
    }
    __syncthreads();
    if (tid < NC) {
      const size_t slot = static_cast<size_t>(L.slot[job * NC + tid]);
      L.rem[slot * L.tiles + k] = wave_rem[0][tid] ^ wave_rem[1][tid] ^ wave_rem[2][tid] ^ wave_rem[3][tid];
    }
  }

  // the parity bytes after the last whole segment: the stripe's last block
  if (k != T - 1) return;
  const size_t nvec = L.nbytes / 16;
  const size_t v = static_cast<size_t>(nseg) * kEcSegVecs + tid;  // < kEcSegVecs of them
  if (v < nvec) {
    uint32_t acc[16];
    v4u xr = v4u{0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b) acc[b] = 0;
#pragma unroll 1
    for (int i = 0; i < NIN; ++i) {
      const v4u x = __builtin_nontemporal_load((g_cu4*) (J.in[i]) + v);
      if constexpr (XOR) xr ^= x;
      else gf_acc_input<0>(lds, x, i, acc);
    }
#pragma unroll
    for (int j = 0; j < NOUT; ++j) store_vec((g_u4*) (J.out[j]), v, XOR ? xr : ec_gather(acc, j));
  }
  const size_t b = nvec * 16 + tid;
  if (b < L.nbytes) {
    uint32_t r[NOUT];
#pragma unroll
    for (int j = 0; j < NOUT; ++j) r[j] = 0;
#pragma unroll 1
    for (int i = 0; i < NIN; ++i) {
      const uint32_t x = J.in[i][b];
#pragma unroll
      for (int j = 0; j < NOUT; ++j) r[j] ^= XOR ? x : gf_mul_dev(J.coef[j][i], x);
    }
#pragma unroll
    for (int j = 0; j < NOUT; ++j) J.out[j][b] = static_cast<uint8_t>(r[j]);
  }
}

using EcKernel = void (*)(EncodeCrcLaunch);
// [nin - 1][nout - 1], and [nin - 1][kMaxOut] for XOR
#define EC_ROW(N)                                                                                    \
  {&encode_crc_kernel<N, 1, false>, &encode_crc_kernel<N, 2, false>, &encode_crc_kernel<N, 3, false>, \
   &encode_crc_kernel<N, 4, false>, &encode_crc_kernel<N, 1, true>}
const EcKernel kEcKernels[kMaxIn][kMaxOut + 1] = {EC_ROW(1),  EC_ROW(2),  EC_ROW(3),  EC_ROW(4),  EC_ROW(5),  EC_ROW(6),
                                                  EC_ROW(7),  EC_ROW(8),  EC_ROW(9),  EC_ROW(10), EC_ROW(11), EC_ROW(12),
                                                  EC_ROW(13), EC_ROW(14), EC_ROW(15), EC_ROW(16)};
#undef EC_ROW

}  // namespace

void encode_crc_xpow(unsigned* xpow) {
  for (int t = 0; t < kCrcLanes; ++t) {
    const int w = t >> 6, j = t & 63;
    xpow[t] = crc_xpow8(static_cast<unsigned long long>(kCrcLanes / 64 - 1 - w) * kEcWaveRows * 16 * kEcRowVecs +
                        16ull * (63 - j));
  }
}

int launch_encode_crc(const EncodeCrcLaunch& L, void* stream) {
  if (L.njobs <= 0) return hipSuccess;
  if (L.nin < 1 || L.nin > kMaxIn || L.nout < 1 || L.nout > kMaxOut || (L.xor_only && L.nout != 1))
    return hipErrorInvalidValue;
  const EcKernel kernel = kEcKernels[L.nin - 1][L.xor_only ? kMaxOut : L.nout - 1];
  const unsigned grid = static_cast<unsigned>(L.njobs) * static_cast<unsigned>(std::max(1, L.tiles));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kCrcLanes), 0, static_cast<hipStream_t>(stream), L);
  if (hipError_t e = hipGetLastError()) return e;
  return launch_crc32_finish(L.finish, stream);
}

}  // namespace redset_hip
