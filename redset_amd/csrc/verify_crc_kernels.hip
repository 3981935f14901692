// verify_crc_kernels.hip -- scrub a set and take the zlib CRC-32 of all its
// cells in one read (gfx950); descriptors in verify_crc.h.
//
// verify_crc_kernel<NIN, NOUT, XOR>: the split of encode_crc_kernels.hip with
// the parity stores turned into parity loads. Block (stripe, tile) of 256
// threads takes one 128 KiB tile (kCrcTile, the grid of crc32.h: the range's
// short tile is its first, filled from the back) of every cell of one stripe.
// A row is 1 KiB: lane j of a wave holds the 16-B vector at column j of the
// row for each of the NIN data cells AND each of the NOUT stored parity cells
// -- direct non-temporal global loads, the next row's issued before this
// row's arithmetic; stripes of more than kRingChunk inputs load in two
// chunks, and there the stored vectors of a row ride with its second chunk,
// under the first chunk's lookups. Wave w walks rows 32 w .. 32 w + 31.
//
// Check: the lane forms the NOUT parity vectors with the codec's nibble
// tables (codec_device.h; XOR: a plain XOR) and XORs each with the stored
// one: the position's syndrome. Zero is the fast path -- an OR, no atomics.
// Else the lane counts the differing bytes per parity row in a register
// (CheckTally) and sends its first differing byte offset to the report at
// once (64-bit atomicMin: a lane meets its rows in ascending order, so only
// its first difference can be its smallest); after its last position a lane
// with a nonzero count adds it (atomicAdd). The report rows and the tile
// remainders are all the kernel writes.
//
// Checksum: one running remainder per cell and lane, advanced from the
// registers as in encode_crc_kernels.hip; a parity cell's from the vector
// that was LOADED, never the one computed -- on a damaged set they differ,
// and the sidecar holds the stored bytes' CRC. The tile end is that file's
// too: the x-power multiply (encode_crc_xpow), wave shuffles, four words
// through LDS, one remainder per (cell, tile) for crc32_finish_kernel.
//
// Bytes [512 * (C / 512), C) belong to no tile: the block of the stripe's
// last tile checks them, whole vectors with the tables and the last C % 16
// bytes one by one, and counts them like any other; their CRC is the finish
// launch's, from memory.
//
// No block waits on another: no ring, no claim counter, no spin, and the
// kernel has no access to the ring-fault and hang-fault words.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fused_crc_device.h"
#include "verify_crc.h"

namespace redset_hip {

namespace {

// waves per SIMD the kernels are compiled for (the cap on their VGPRs): what
// every instantiation reaches without scratch. Up to kRingChunk inputs two
// rows of all nin + nout vectors are live at once, 8 VGPRs a cell: 9 cells fit
// under the 128 VGPRs of 4 waves, wider stripes take the 168 of 3.
constexpr int vc_waves(int nin, int nout) { return nin + nout <= kRingChunk + 1 ? 4 : 3; }

// The check of one 16-B position: begin(), add<I0>(x, ok) for inputs
// [I0, I0 + N) -- each also goes through its cell's remainder -- then
// finish(s, at, ok) compares with the stored vectors s and runs THOSE through
// their cells' remainders. ok: the lane's position lies in the cell; where it
// does not, the remainders stay 0 and nothing is counted.
template <int NIN, int NOUT, bool XOR>
struct VcAcc {
  const uint32_t* gf;
  const unsigned* sl;
  const unsigned* adv;
  unsigned rem[NIN + NOUT];
  uint32_t acc[16];
  v4u xr;
  CheckTally tally[NOUT];
  CheckWhere where;  // of the stripe's row 0; row j is j words on

  __device__ __forceinline__ CheckWhere row(int j) const {
    return CheckWhere{where.count + j, where.first + j, where.base};
  }
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
      // as in encode_crc_kernels.hip: without it the scheduler starts every
      // input's lookups at once and spills what they return
      if constexpr (XOR) __builtin_amdgcn_sched_barrier(0);
    }
  }
  // syndrome vector of parity row j against the stored vector s
  __device__ __forceinline__ v4u syndrome(int j, const v4u& s) const {
    if constexpr (XOR) return xr ^ s;
    else return ec_gather(acc, j) ^ s;
  }
  __device__ __forceinline__ void finish(const v4u (&s)[NOUT], long long at, bool ok) {
    v4u r[NOUT];
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < NOUT; ++j) {
      r[j] = syndrome(j, s[j]);
      any |= r[j].x | r[j].y | r[j].z | r[j].w;
      const unsigned next = ec_row(sl, adv, rem[NIN + j], s[j]);
      rem[NIN + j] = ok ? next : 0u;
    }
    // The remainders are complete before the branch: left alone, the compiler
    // sinks their XORs below it and spills every looked-up word across it.
#pragma unroll
    for (int c = 0; c < NIN + NOUT; ++c) asm volatile("" : "+v"(rem[c]));
    if (any == 0 || !ok) return;
#pragma unroll
    for (int j = 0; j < NOUT; ++j)
      if ((r[j].x | r[j].y | r[j].z | r[j].w) != 0) tally[j].note_vec(row(j), static_cast<size_t>(at), r[j]);
  }
};

template <int NIN, int NOUT, bool XOR>
__global__ __launch_bounds__(kCrcLanes)
__attribute__((amdgpu_waves_per_eu(vc_waves(NIN, NOUT), vc_waves(NIN, NOUT)))) void
verify_crc_kernel(VerifyCrcLaunch L) {
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

  VcAcc<NIN, NOUT, XOR> A;
  A.gf = lds;
  A.sl = lds + kEcGfWords;
  A.adv = lds + kEcGfWords + kSliceWords;
  A.where = CheckWhere{L.report + job * NOUT, L.report + L.report_rows + job * NOUT, 0ull};
#pragma unroll
  for (int j = 0; j < NOUT; ++j) A.tally[j].reset();

  const long long nseg = static_cast<long long>(L.nbytes / kCrcSeg);
  if (L.tiles > 0) {
    g_cu4* in[NIN];
    g_cu4* out[NOUT];
#pragma unroll
    for (int i = 0; i < NIN; ++i) in[i] = (g_cu4*) (J.in[i]);
#pragma unroll
    for (int j = 0; j < NOUT; ++j) out[j] = (g_cu4*) (J.out[j]);
#pragma unroll
    for (int c = 0; c < NC; ++c) A.rem[c] = 0;

    // The first tile lacks `pad` segments at its front: its rows before
    // pad / 2 are not there, and of row pad / 2 the first half when pad is
    // odd. The lanes of that half row keep the loop free of a second trip
    // count: they work at vector 0 of the cells, which lane 32 of the same row
    // owns, with their remainders held at 0, and they count nothing -- a wrong
    // byte in [0, 16) is lane 32's to report.
    const long long pad = static_cast<long long>(L.tiles) * kCrcLanes - nseg;
    const long long vb = (static_cast<long long>(k) * kCrcLanes - pad) * kEcSegVecs + lane;  // row 0 of the tile
    const int first = k == 0 ? static_cast<int>(pad / 2) : 0;
    const int r1 = (w + 1) * kEcWaveRows;
    int r = std::max(w * kEcWaveRows, first);
    if (r < r1) {
      v4u x0[N0], s0[NOUT];
      const long long at0 = std::max(0ll, vb + static_cast<long long>(r) * kEcRowVecs);
      ec_load<0, N0>(x0, in, at0);
      if constexpr (N1 == 0) ec_load<0, NOUT>(s0, out, at0);
      for (; r < r1; ++r) {
        const long long v = vb + static_cast<long long>(r) * kEcRowVecs;
        const bool ok = v >= 0;
        const long long at = ok ? v : 0;
        // after the wave's last row: that row again, loaded and not checked
        const long long next = r + 1 < r1 ? v + kEcRowVecs : at;
        A.begin();
        if constexpr (N1 > 0) {
          v4u x1[N1];
          ec_load<N0, N1>(x1, in, at);
          ec_load<0, NOUT>(s0, out, at);
          A.template add<0>(x0, ok);
          ec_load<0, N0>(x0, in, next);
          A.template add<N0>(x1, ok);
          A.finish(s0, at, ok);
        } else {
          v4u nx[N0], ns[NOUT];
          ec_load<0, N0>(nx, in, next);
          ec_load<0, NOUT>(ns, out, next);
          A.template add<0>(x0, ok);
          A.finish(s0, at, ok);
#pragma unroll
          for (int i = 0; i < N0; ++i) x0[i] = nx[i];
#pragma unroll
          for (int j = 0; j < NOUT; ++j) s0[j] = ns[j];
        }
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

  // the bytes after the last whole segment: the stripe's last block, each
  // thread at offsets above every one it met in the tile
  if (k == T - 1) {
    const size_t nvec = L.nbytes / 16;
    const size_t v = static_cast<size_t>(nseg) * kEcSegVecs + tid;  // < kEcSegVecs of them
    if (v < nvec) {
      A.begin();
#pragma unroll 1
      for (int i = 0; i < NIN; ++i) {
        const v4u x = __builtin_nontemporal_load((g_cu4*) (J.in[i]) + v);
        if constexpr (XOR) A.xr ^= x;
        else gf_acc_input<0>(lds, x, i, A.acc);
      }
#pragma unroll
      for (int j = 0; j < NOUT; ++j) {
        const v4u r = A.syndrome(j, __builtin_nontemporal_load((g_cu4*) (J.out[j]) + v));
        if ((r.x | r.y | r.z | r.w) != 0) A.tally[j].note_vec(A.row(j), v, r);
      }
    }
    const size_t b = nvec * 16 + tid;
    if (b < L.nbytes) {
      uint32_t r[NOUT];
#pragma unroll
      for (int j = 0; j < NOUT; ++j) r[j] = J.out[j][b];
#pragma unroll 1
      for (int i = 0; i < NIN; ++i) {
        const uint32_t x = J.in[i][b];
#pragma unroll
        for (int j = 0; j < NOUT; ++j) r[j] ^= XOR ? x : gf_mul_dev(J.coef[j][i], x);
      }
#pragma unroll
      for (int j = 0; j < NOUT; ++j)
        if (r[j] != 0) A.tally[j].note(A.row(j), b, 1u);
    }
  }
#pragma unroll
  for (int j = 0; j < NOUT; ++j) A.tally[j].flush(A.row(j));
}

using VcKernel = void (*)(VerifyCrcLaunch);
// [nin - 1][nout - 1], and [nin - 1][kMaxOut] for XOR
#define VC_ROW(N)                                                                                    \
  {&verify_crc_kernel<N, 1, false>, &verify_crc_kernel<N, 2, false>, &verify_crc_kernel<N, 3, false>, \
   &verify_crc_kernel<N, 4, false>, &verify_crc_kernel<N, 1, true>}
const VcKernel kVcKernels[kMaxIn][kMaxOut + 1] = {VC_ROW(1),  VC_ROW(2),  VC_ROW(3),  VC_ROW(4),  VC_ROW(5),  VC_ROW(6),
                                                  VC_ROW(7),  VC_ROW(8),  VC_ROW(9),  VC_ROW(10), VC_ROW(11), VC_ROW(12),
                                                  VC_ROW(13), VC_ROW(14), VC_ROW(15), VC_ROW(16)};
#undef VC_ROW

}  // namespace

int launch_verify_crc(const VerifyCrcLaunch& L, void* stream) {
  if (L.njobs <= 0) return hipSuccess;
  if (L.nin < 1 || L.nin > kMaxIn || L.nout < 1 || L.nout > kMaxOut || (L.xor_only && L.nout != 1) || !L.report ||
      L.report_rows != L.njobs * L.nout)
    return hipErrorInvalidValue;
  if (int e = reset_report(L.report, L.report_rows, 0, L.report_rows, stream)) return e;
  const VcKernel kernel = kVcKernels[L.nin - 1][L.xor_only ? kMaxOut : L.nout - 1];
  const unsigned grid = static_cast<unsigned>(L.njobs) * static_cast<unsigned>(std::max(1, L.tiles));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kCrcLanes), 0, static_cast<hipStream_t>(stream), L);
  if (hipError_t e = hipGetLastError()) return e;
  return launch_crc32_finish(L.finish, stream);
}

}  // namespace redset_hip
