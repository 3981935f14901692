// repair_wide_kernels.hip -- column-wise repair of RS stripes with E = 5..8
// parity rows, up to E / 2 wrong bytes per byte column (gfx950); descriptors
// in repair_wide.h, the arithmetic in include/redset_hip.h ("repair_wide").
//
// gf_repair_wide_kernel<E>: one job is one stripe of d data cells and E stored
// parity cells, 256-thread blocks, blocks_per_job of them side by side over
// the columns. The clean path belongs to a lane, the damaged path to a wave:
//
// * Clean columns, per lane: the nibble tables of the d inputs in LDS, 8-byte
//   entries (rows 0-3 in the low dword, rows 4..E-1 in the high), 256 B per
//   input, so a column's packed syndrome S costs two ds_read_b64 per data
//   byte; 16-B global loads, four inputs in flight; the stored parity bytes
//   are transposed into the same packing. Every lane of a wave runs the same
//   number of steps (a lane past the end holds S = 0), and a wave whose 64
//   lanes all hold 16 clean columns goes on after one ballot.
//
// * Damaged columns, per wave: the wave takes its damaged columns one at a
//   time, all 64 lanes on one column. The owner's S comes over by __shfl,
//   2 E broadcast LDS reads (the nibble tables of W^-1) give the power sums
//   S'_k, and for nu = 1 .. max_errors every lane solves the nu x nu Hankel
//   system for the locator by the same unrolled elimination on log/exp tables
//   (wave-uniform, registers only) and checks the remaining power sums. Lane
//   l then evaluates the locator at the points of cells l, l + 64, l + 128,
//   l + 192; ballots count the roots; a lane that holds a root X divides the
//   locator by (z ^ X) to get its error value y / u; the proposal's own
//   syndrome is an XOR butterfly over the wave of the lanes' table entries
//   and is compared with S before anything is written. The column's owner
//   lane then does the one-byte read-modify-writes.
//   No __syncthreads and no LDS write after the prologue: the loop is bounded
//   by 16 columns x 64 lanes a step.
//
// LDS, bytes: [0, 256 d) input tables | 256 E W^-1 nibble tables | 512 exp
// (2^i, i < 512) | 256 log | 256 1/u per cell | 256 alpha per cell:
// 256 (d + E) + 1280, 66816 at (248, 8).
//
// Reports: the lane that evaluates a cell's point counts that cell's
// corrections and keeps their first offset in registers, and flushes them
// with one 64-bit atomic pair at the end; the owner lane counts its unlocated
// columns; lane 0 of a wave flushes the wave's nu histogram. Footprint: a
// correction is a one-byte read-modify-write by the lane that owns the column;
// dry runs and unlocated columns store nothing. No block waits on another: no
// ring, no claim counter, no spin, and the kernel has no access to the
// ring-fault and hang-fault words. Every loop bound is known at launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "codec_kernels.h"
#include "gf256.h"
#include "repair_wide.h"

namespace redset_hip {

namespace {

constexpr int kWave = 64;
constexpr int kPerLane = kRepairBlock / kWave;  // cells whose points one lane evaluates (d + E <= 256)

__device__ __forceinline__ uint32_t gf_mul_bits(uint32_t a, uint32_t b) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    r ^= (b & 1u) ? a : 0u;
    b >>= 1;
    a <<= 1;
    a ^= (a & 0x100u) ? 0x11Du : 0u;
  }
  return r;
}

// the LDS view of one block
struct WideLds {
  const uint2* tab;      // d x 32 entries: input m, nibble half h, value n at m * 32 + h * 16 + n
  const uint2* w;        // E x 32 entries, the same shape over the syndrome's bytes
  const uint8_t* ex;     // 512
  const uint8_t* lg;     // 256
  const uint8_t* invu;   // 256
  const uint8_t* alpha;  // 256
  __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) const {
    return (a != 0 && b != 0) ? ex[lg[a] + lg[b]] : 0u;
  }
  // a / b, b != 0
  __device__ __forceinline__ uint32_t div(uint32_t a, uint32_t b) const { return a != 0 ? ex[lg[a] + 255u - lg[b]] : 0u; }
};

__device__ __forceinline__ void acc_word(const uint2* T, uint32_t w, uint32_t* lo, uint32_t* hi) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const uint2 x = T[(w >> (8 * b)) & 15u], y = T[16 + ((w >> (8 * b + 4)) & 15u)];
    lo[b] ^= x.x ^ y.x;
    hi[b] ^= x.y ^ y.y;
  }
}

__device__ __forceinline__ void acc_vec(const uint2* T, const uint4& x, uint32_t (&lo)[16], uint32_t (&hi)[16]) {
  acc_word(T, x.x, lo, hi);
  acc_word(T, x.y, lo + 4, hi + 4);
  acc_word(T, x.z, lo + 8, hi + 8);
  acc_word(T, x.w, lo + 12, hi + 12);
}

// s[b] ^= byte b of r0..r3 as one dword (rows past NR are absent)
template <int NR>
__device__ __forceinline__ void acc_rows(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t* s) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    uint32_t v = (r0 >> (8 * b)) & 255u;
    if (NR > 1) v |= ((r1 >> (8 * b)) & 255u) << 8;
    if (NR > 2) v |= ((r2 >> (8 * b)) & 255u) << 16;
    if (NR > 3) v |= ((r3 >> (8 * b)) & 255u) << 24;
    s[b] ^= v;
  }
}

__device__ __forceinline__ uint32_t word_of(const uint4& r, int q) {
  return q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w;
}

__device__ __forceinline__ uint32_t byte_of(uint32_t lo, uint32_t hi, int k) {
  return ((k < 4 ? lo : hi) >> (8 * (k & 3))) & 255u;
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v ^= __shfl_xor(v, o, kWave);
  return v;
}

// What one wave found. Every member is a register of the lane it is named for.
template <int E>
struct WideRepairer {
  const RepairWideLaunch& L;
  const RepairWideJob& J;
  const WideLds& M;
  const int lane;
  unsigned cnt[kPerLane];              // corrections of cell lane + 64 k, whichever lane owned the column
  unsigned long long first[kPerLane];  // the first of them (a wave meets its columns in ascending order)
  unsigned ucnt;                       // unlocated columns this lane owns
  unsigned multi[kWideMaxT - 1];       // wave-uniform: columns corrected with nu = 2..4 wrong bytes

  // the packed syndrome of error x in `cell`
  __device__ __forceinline__ uint2 syndrome_of(int cell, uint32_t x) const {
    if (cell < L.d) {
      const uint2 a = M.tab[cell * 32 + (x & 15u)], b = M.tab[cell * 32 + 16 + (x >> 4)];
      return make_uint2(a.x ^ b.x, a.y ^ b.y);
    }
    const int j = cell - L.d;
    return j < 4 ? make_uint2(x << (8 * j), 0u) : make_uint2(0u, x << (8 * (j - 4)));
  }

  // Level nu (1 .. T) of the rule: true when the column is corrected with nu
  // wrong bytes. P: the power sums, byte k = S'_k; (lo, hi): S; `off` and
  // `owner`: the column and its lane. One body for every nu: the system is
  // padded to T x T with identity rows, so every index is static.
  __device__ __forceinline__ bool level(int nu, unsigned long long P, uint32_t lo, uint32_t hi, size_t off, int owner) {
    constexpr int T = E / 2;
    auto sp = [&](int k) { return static_cast<uint32_t>(P >> (8 * (k < E ? k : E - 1))) & 255u; };
    // the Hankel system sum_k sigma_k S'_(j+k) = S'_(j+nu), j < nu: Gauss-Jordan
    uint32_t A[T][T + 1];
#pragma unroll
    for (int j = 0; j < T; ++j) {
#pragma unroll
      for (int k = 0; k < T; ++k) A[j][k] = (j < nu && k < nu) ? sp(j + k) : (j == k ? 1u : 0u);
      A[j][T] = j < nu ? sp(j + nu) : 0u;
    }
    bool solved = true;
#pragma unroll
    for (int c = 0; c < T; ++c) {
#pragma unroll
      for (int r = c + 1; r < T; ++r) {
        const bool swap = A[c][c] == 0 && A[r][c] != 0;
#pragma unroll
        for (int k = c; k <= T; ++k) {
          const uint32_t a = A[c][k], b = A[r][k];
          A[c][k] = swap ? b : a;
          A[r][k] = swap ? a : b;
        }
      }
      const uint32_t piv = A[c][c];
      solved = solved && piv != 0;
      const uint32_t pv = piv != 0 ? piv : 1u;
#pragma unroll
      for (int k = c; k <= T; ++k) A[c][k] = M.div(A[c][k], pv);
#pragma unroll
      for (int r = 0; r < T; ++r) {
        if (r == c) continue;
        const uint32_t f = A[r][c];
#pragma unroll
        for (int k = c; k <= T; ++k) A[r][k] ^= M.mul(f, A[c][k]);
      }
    }
    if (!solved) return false;
    // the locator's coefficients c_0 .. c_T: sigma below nu, 1 at nu, 0 above
    uint32_t cf[T + 1];
#pragma unroll
    for (int k = 0; k <= T; ++k) cf[k] = (k < T ? A[k][T] : 0u) ^ (k == nu ? 1u : 0u);
    // every remaining power sum
    uint32_t rest = 0;
#pragma unroll
    for (int j = 1; j + 1 < E; ++j) {
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k <= T; ++k) v ^= M.mul(cf[k], sp(j + k));
      rest |= (j >= nu && j + nu < E) ? v : 0u;
    }
    if (rest != 0) return false;
    // roots among the stripe's points, error values where there is one
    const int n = L.d + E;
    uint32_t xv[kPerLane];
    unsigned long long roots[kPerLane];
    int nroots = 0;
    uint32_t zero_value = 0;
    uint2 own = make_uint2(0u, 0u);
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
      roots[q] = 0;
      xv[q] = 0;
      if (q * kWave >= n) continue;  // uniform
      const int cell = lane + q * kWave;
      bool root = false;
      if (cell < n) {
        const uint32_t X = M.alpha[cell];
        // b(z) = locator / (z ^ X), remainder locator(X): y = sum_k b_k S'_k / b(X)
        uint32_t b = cf[T], num = 0, den = 0;
#pragma unroll
        for (int k = T - 1; k >= 0; --k) {
          num ^= M.mul(b, sp(k));
          den = M.mul(den, X) ^ b;
          b = M.mul(b, X) ^ cf[k];
        }
        root = b == 0;
        if (root) {
          xv[q] = den != 0 ? M.mul(M.div(num, den), M.invu[cell]) : 0u;
          zero_value |= xv[q] == 0 ? 1u : 0u;
          const uint2 mine = syndrome_of(cell, xv[q]);
          own.x ^= mine.x;
          own.y ^= mine.y;
        }
      }
      roots[q] = __ballot(root);
      nroots += __popcll(roots[q]);
    }
    if (nroots != nu) return false;
    if (__ballot(zero_value != 0) != 0) return false;
    // the guard: what is proposed must give this very syndrome
    if (wave_xor(own.x) != lo || wave_xor(own.y) != hi) return false;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
      if (q * kWave >= n) continue;
      if ((roots[q] >> lane) & 1ull) {
        if (cnt[q] == 0) first[q] = L.base + off;
        ++cnt[q];
      }
      if (!L.apply) continue;
      // at most nu bits over all q
      for (unsigned long long mask = roots[q]; mask != 0; mask &= mask - 1) {
        const int src = __ffsll(mask) - 1;
        const uint32_t x = __shfl(xv[q], src, kWave);
        if (lane == owner) {
          uint8_t* b = J.cells[src + q * kWave] + off;
          *b = static_cast<uint8_t>(*b ^ x);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kWideMaxT - 1; ++i) multi[i] += nu == i + 2 ? 1u : 0u;
    return true;
  }

  // the column at cell offset `off`, owned by lane `owner`, has the nonzero packed syndrome (lo, hi)
  __device__ __forceinline__ void column(size_t off, uint32_t lo, uint32_t hi, int owner) {
    uint2 P = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const uint32_t b = byte_of(lo, hi, k);
      const uint2 x = M.w[k * 32 + (b & 15u)], y = M.w[k * 32 + 16 + (b >> 4)];
      P.x ^= x.x ^ y.x;
      P.y ^= x.y ^ y.y;
    }
    const unsigned long long P64 = (static_cast<unsigned long long>(P.y) << 32) | P.x;
    bool done = false;
#pragma unroll 1
    for (int nu = 1; nu <= L.max_errors && !done; ++nu) done = level(nu, P64, lo, hi, off, owner);
    if (!done && lane == owner) {
      if (ucnt == 0) atomicMin(L.stripe_report + L.nstripes + J.row, L.base + off);
      ++ucnt;
    }
  }

  // One step of the wave: lane l holds the columns at cell offsets first_off +
  // l * stride + c, c < 16, with the packed syndromes (lo[c], hi[c]) (zero for
  // a column that is not there).
  __device__ __forceinline__ void step(size_t first_off, int stride, const uint32_t (&lo)[16],
                                       const uint32_t (&hi)[16]) {
    uint32_t cm = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) cm |= (lo[c] | hi[c]) != 0 ? 1u << c : 0u;
    unsigned long long damaged = __ballot(cm != 0);
    if (damaged == 0) return;
#pragma unroll 1
    for (; damaged != 0; damaged &= damaged - 1) {
      const int owner = __ffsll(damaged) - 1;
#pragma unroll 1
      for (uint32_t ocm = __shfl(cm, owner, kWave); ocm != 0; ocm &= ocm - 1) {
        const int c = __ffs(ocm) - 1;
        uint32_t a = 0, b = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          a = i == c ? lo[i] : a;
          b = i == c ? hi[i] : b;
        }
        column(first_off + static_cast<size_t>(owner) * stride + c, __shfl(a, owner, kWave), __shfl(b, owner, kWave),
               owner);
      }
    }
  }

  __device__ __forceinline__ void finish() {
    const int n = L.d + E;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
      const int cell = lane + q * kWave;
      if (cell >= n || cnt[q] == 0) continue;
      const size_t at = static_cast<size_t>(J.row) * L.p + J.member[cell];
      atomicAdd(L.cell_report + at, static_cast<unsigned long long>(cnt[q]));
      atomicMin(L.cell_report + L.ncells + at, first[q]);
    }
    if (ucnt != 0) atomicAdd(L.stripe_report + J.row, static_cast<unsigned long long>(ucnt));
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kWideMaxT - 1; ++i)
        if (multi[i] != 0)
          atomicAdd(L.multi_report + static_cast<size_t>(J.row) * (kWideMaxT - 1) + i,
                    static_cast<unsigned long long>(multi[i]));
    }
  }
};

template <int E>
__global__ __launch_bounds__(kRepairBlock) void gf_repair_wide_kernel(RepairWideLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int d = L.d;
  const int job = blockIdx.x / L.blocks_per_job, blk = blockIdx.x % L.blocks_per_job;
  if (job >= L.njobs) return;
  const RepairWideJob& G = L.jobs[job];  // in global memory: W^-1 is indexed there
  const RepairWideJob J = G;
  uint2* tab = reinterpret_cast<uint2*>(lds);
  uint2* wtab = tab + d * 32;
  uint8_t* bytes = reinterpret_cast<uint8_t*>(wtab + E * 32);
  for (int t = threadIdx.x; t < d * 32; t += kRepairBlock) {
    const int i = t >> 5, h = (t >> 4) & 1, n = t & 15;
    const uint32_t x = static_cast<uint32_t>(n) << (4 * h);
    uint2 v = make_uint2(0u, 0u);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const uint32_t m = gf_mul_bits(J.coef[j * d + i], x);
      if (j < 4) v.x |= m << (8 * j);
      else v.y |= m << (8 * (j - 4));
    }
    tab[t] = v;
  }
  {
    const int t = threadIdx.x;  // kRepairBlock == 256: one entry of every table per thread
    if (t < E * 32) {
      // W^-1 nibble tables: syndrome byte k = t >> 5, nibble h, value n -> the E power sums' share
      const int k = t >> 5, h = (t >> 4) & 1, n = t & 15;
      const uint32_t x = static_cast<uint32_t>(n) << (4 * h);
      uint2 v = make_uint2(0u, 0u);
#pragma unroll
      for (int r = 0; r < E; ++r) {
        const uint32_t m = gf_mul_bits(G.winv[r * E + k], x);
        if (r < 4) v.x |= m << (8 * r);
        else v.y |= m << (8 * (r - 4));
      }
      wtab[t] = v;
    }
    bytes[t] = L.gf[t];
    bytes[256 + t] = L.gf[256 + t];
    bytes[512 + t] = L.gf[512 + t];
    bytes[768 + t] = t < d + E ? J.invu[t] : 0;
    bytes[1024 + t] = t < d + E ? J.alpha[t] : 0;
  }
  __syncthreads();

  const WideLds M{tab, wtab, bytes, bytes + 512, bytes + 768, bytes + 1024};
  const int lane = threadIdx.x & (kWave - 1);
  WideRepairer<E> R{L, J, M, lane, {0u, 0u, 0u, 0u}, {0ull, 0ull, 0ull, 0ull}, 0u, {0u, 0u, 0u}};
  const size_t step = static_cast<size_t>(L.blocks_per_job) * kRepairBlock;
  const size_t lane0 = static_cast<size_t>(blk) * kRepairBlock + threadIdx.x;
  const size_t nvec = J.bytes_only ? 0 : L.nbytes / 16;

  // Every lane of the block runs the same number of steps, since the damaged
  // path needs whole waves: the 16-B steps, then byte columns -- the whole job
  // when a cell is unaligned, else the tail after the last whole vector
  // (block 0 of the job).
  const size_t vsteps = (nvec + step - 1) / step;
  const size_t b0 = nvec * 16;
  const bool bytes_here = J.bytes_only || blk == 0;
  const size_t bstep = J.bytes_only ? step : kRepairBlock;
  const size_t bl0 = J.bytes_only ? lane0 : threadIdx.x;
  const size_t bsteps = bytes_here ? (L.nbytes - b0 + bstep - 1) / bstep : 0;
#pragma unroll 1
  for (size_t it = 0; it < vsteps + bsteps; ++it) {
    uint32_t lo[16], hi[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) lo[b] = hi[b] = 0;
    const bool vec = it < vsteps;
    const size_t v = lane0 + it * step;
    const size_t o = b0 + bl0 + (it - vsteps) * bstep;
    if (vec && v < nvec) {
      int m = 0;
      for (; m + 4 <= d; m += 4) {
        const uint4 x0 = reinterpret_cast<const uint4*>(J.cells[m])[v];
        const uint4 x1 = reinterpret_cast<const uint4*>(J.cells[m + 1])[v];
        const uint4 x2 = reinterpret_cast<const uint4*>(J.cells[m + 2])[v];
        const uint4 x3 = reinterpret_cast<const uint4*>(J.cells[m + 3])[v];
        acc_vec(tab + m * 32, x0, lo, hi);
        acc_vec(tab + (m + 1) * 32, x1, lo, hi);
        acc_vec(tab + (m + 2) * 32, x2, lo, hi);
        acc_vec(tab + (m + 3) * 32, x3, lo, hi);
      }
      for (; m < d; ++m) acc_vec(tab + m * 32, reinterpret_cast<const uint4*>(J.cells[m])[v], lo, hi);
      // the stored parity rows, transposed into the tables' packing
      uint4 r[E];
#pragma unroll
      for (int j = 0; j < E; ++j) r[j] = reinterpret_cast<const uint4*>(J.cells[d + j])[v];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc_rows<4>(word_of(r[0], q), word_of(r[1], q), word_of(r[2], q), word_of(r[3], q), lo + 4 * q);
        acc_rows<E - 4>(word_of(r[4], q), word_of(r[E > 5 ? 5 : 4], q), word_of(r[E > 6 ? 6 : 4], q),
                        word_of(r[E > 7 ? 7 : 4], q), hi + 4 * q);
      }
    } else if (!vec && o < L.nbytes) {
      for (int m = 0; m < d; ++m) {
        const uint32_t b = J.cells[m][o];
        const uint2 x = tab[m * 32 + (b & 15u)], y = tab[m * 32 + 16 + (b >> 4)];
        lo[0] ^= x.x ^ y.x;
        hi[0] ^= x.y ^ y.y;
      }
#pragma unroll
      for (int j = 0; j < E; ++j) {
        const uint32_t b = J.cells[d + j][o];
        if (j < 4) lo[0] ^= b << (8 * j);
        else hi[0] ^= b << (8 * (j - 4));
      }
    }
    if (vec) R.step((v - lane) * 16, 16, lo, hi);
    else R.step(o - lane, 1, lo, hi);
  }
  R.finish();
}

__global__ __launch_bounds__(kRepairBlock) void repair_wide_reset_kernel(RepairWideLaunch L) {
  for (int i = threadIdx.x; i < L.ncells; i += kRepairBlock) {
    L.cell_report[i] = 0;
    L.cell_report[L.ncells + i] = ~0ull;
  }
  for (int i = threadIdx.x; i < L.nstripes; i += kRepairBlock) {
    L.stripe_report[i] = 0;
    L.stripe_report[L.nstripes + i] = ~0ull;
  }
  for (int i = threadIdx.x; i < L.nstripes * (kWideMaxT - 1); i += kRepairBlock) L.multi_report[i] = 0;
}

size_t up16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

template <int E>
hipError_t prepare(size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&gf_repair_wide_kernel<E>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
}

template <int E>
void launch(const RepairWideLaunch& L, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(gf_repair_wide_kernel<E>, grid, dim3(kRepairBlock), repair_wide_lds_bytes(L.d, E), stream, L);
}

}  // namespace

size_t repair_wide_lds_bytes(int d, int e) { return static_cast<size_t>(d + e) * 256 + 1280; }

int repair_wide_prepare(int d, int e) {
  if (d < 1 || d + e > kRepairBlock || repair_wide_lds_bytes(d, e) > kWideLdsLimit) return hipErrorInvalidValue;
  // the widest stripe of this e, so that a later, narrower plan never lowers it
  const size_t bytes = repair_wide_lds_bytes(kRepairBlock - e, e);
  switch (e) {
    case 5: return prepare<5>(bytes);
    case 6: return prepare<6>(bytes);
    case 7: return prepare<7>(bytes);
    case 8: return prepare<8>(bytes);
  }
  return hipErrorInvalidValue;
}

int repair_wide_upload(const std::vector<RepairWideJobDesc>& jobs, int d, int e, void** blob_out, RepairWideLaunch& L) {
  *blob_out = nullptr;
  L.jobs = nullptr;
  L.gf = nullptr;
  const size_t n = jobs.size();
  // the field tables, the job array, then per job: cell pointers, member
  // indices, coefficients, points, 1/u
  const size_t o_jobs = 768;
  const size_t o_per = o_jobs + up16(n * sizeof(RepairWideJob));
  const size_t s_cells = up16(static_cast<size_t>(d + e) * sizeof(uint8_t*));
  const size_t s_member = up16(static_cast<size_t>(d + e) * sizeof(int));
  const size_t s_coef = up16(static_cast<size_t>(e) * d);
  const size_t s_n = up16(static_cast<size_t>(d + e));
  const size_t per = s_cells + s_member + s_coef + 2 * s_n;
  const size_t bytes = o_per + n * per;
  void* dev = nullptr;
  if (hipError_t err = hipMalloc(&dev, bytes)) return err;
  std::vector<char> host(bytes, 0);
  char* const dbase = static_cast<char*>(dev);
  const Field& F = field();
  std::memcpy(host.data(), F.exp_, 512);
  std::memcpy(host.data() + 512, F.log_, 256);
  for (size_t k = 0; k < n; ++k) {
    const RepairWideJobDesc& D = jobs[k];
    const size_t o = o_per + k * per;
    uint8_t** cells = reinterpret_cast<uint8_t**>(host.data() + o);
    int* member = reinterpret_cast<int*>(host.data() + o + s_cells);
    uint8_t* coef = reinterpret_cast<uint8_t*>(host.data() + o + s_cells + s_member);
    uint8_t* alpha = coef + s_coef;
    uint8_t* invu = alpha + s_n;
    bool al = true;
    for (int i = 0; i < d; ++i) cells[i] = D.cells.data[static_cast<size_t>(i)];
    for (int j = 0; j < e; ++j) cells[d + j] = D.cells.parity[static_cast<size_t>(j)];
    for (int i = 0; i < d + e; ++i) {
      al = al && (reinterpret_cast<uintptr_t>(cells[i]) & 15u) == 0;
      member[i] = D.cells.member[static_cast<size_t>(i)];
      alpha[i] = D.alpha[static_cast<size_t>(i)];
      invu[i] = D.invu[static_cast<size_t>(i)];
    }
    std::memcpy(coef, D.cells.coef.data(), static_cast<size_t>(e) * d);
    RepairWideJob J;
    std::memset(&J, 0, sizeof(J));
    J.cells = reinterpret_cast<uint8_t* const*>(dbase + o);
    J.member = reinterpret_cast<const int*>(dbase + o + s_cells);
    J.coef = reinterpret_cast<const uint8_t*>(dbase + o + s_cells + s_member);
    J.alpha = J.coef + s_coef;
    J.invu = J.alpha + s_n;
    std::memcpy(J.winv, D.winv.data(), static_cast<size_t>(e) * e);
    J.row = D.cells.row;
    J.bytes_only = al ? 0 : 1;
    std::memcpy(host.data() + o_jobs + k * sizeof(RepairWideJob), &J, sizeof(J));
  }
  if (hipError_t err = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice)) {
    (void) hipFree(dev);
    return err;
  }
  *blob_out = dev;
  L.gf = reinterpret_cast<const uint8_t*>(dev);
  L.jobs = reinterpret_cast<const RepairWideJob*>(dbase + o_jobs);
  return hipSuccess;
}

int launch_repair_wide_reset(const RepairWideLaunch& L, void* stream) {
  hipLaunchKernelGGL(repair_wide_reset_kernel, dim3(1), dim3(kRepairBlock), 0, static_cast<hipStream_t>(stream), L);
  return hipGetLastError();
}

int launch_repair_wide(const RepairWideLaunch& L, void* stream) {
  if (L.njobs <= 0 || L.nbytes == 0) return hipSuccess;
  if (L.d < 1 || L.d + L.e > kRepairBlock || L.blocks_per_job < 1 || !L.jobs || !L.gf || L.max_errors < 1 ||
      L.max_errors > L.e / 2)
    return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(L.njobs) * static_cast<unsigned>(L.blocks_per_job));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  switch (L.e) {
    case 5: launch<5>(L, grid, s); break;
    case 6: launch<6>(L, grid, s); break;
    case 7: launch<7>(L, grid, s); break;
    case 8: launch<8>(L, grid, s); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace redset_hip
