// rebuild_checked_wide_kernels.hip -- errors-and-erasures rebuild of RS stripes
// with 5 to 8 parity rows, up to (e - k) / 2 wrong survivor bytes per byte
// column (gfx950); descriptors in rebuild_checked_wide.h, the arithmetic in
// include/redset_hip.h ("checked rebuild, wide").
//
// gf_rebuild_checked_wide_kernel<S>: one job is one stripe with k lost cells
// and S = e - k spare rows, 256-thread blocks, blocks_per_job of them side by
// side over the columns. S is the template parameter (the decode's register
// indices are static); k is a launch-time value.
//
// * Tables: S + k = e <= 8, so survivor m's whole column of [C ; B] fits one
//   8-byte entry: check rows in the low S bytes, rebuild rows above them. The
//   nibble tables of all ns survivors lie in dynamic LDS, 256 B each, and the
//   packed [T | v] of a byte column is one 64-bit accumulator at two
//   ds_read_b64 per survivor byte. The host has folded W^-1 and the erasure
//   locator into C: surviving parity cells go through tables like data cells.
//
// * Clean columns, per lane: 16-B global loads, four survivors in flight, 16
//   columns per lane in registers. Every lane of a block runs the same number
//   of steps (a lane past the end holds zero and stores nothing); a wave
//   whose 64 x 16 columns all have zero low-S bytes goes on after one ballot.
//   Then every lost cell gets its 16 bytes in one 16-B store. Jobs with a cell
//   that is not 16-B aligned, and the tail after the last whole vector, go
//   byte by byte in the same loop.
//
// * Damaged columns, per wave: the wave takes its damaged columns one at a
//   time, all 64 lanes on one column. The owner's T comes over by __shfl; for
//   nu = 1 .. max_errors every lane solves the nu x nu Hankel system (padded
//   to S/2 x S/2) on log/exp tables in LDS and checks the remaining
//   equations; lane l evaluates the locator at the points of survivors l,
//   l + 64, l + 128, l + 192 by the synthetic division that also yields the
//   error value; ballots decide "exactly nu roots"; the proposal's 64-bit
//   image is an XOR butterfly of the lanes' table entries. Its low S bytes
//   must equal T before anything changes; its high bytes are then XORed into
//   the owner's accumulator, which takes the errors out of v before the
//   store. The owner does the one-byte read-modify-writes of fix_survivors.
//
// LDS, bytes: [0, 256 ns) tables | 512 exp (2^i, i < 512) | 256 log | 256
// 1 / u' per survivor | 256 alpha per survivor: 256 ns + 1280.
//
// Footprint: every byte of the first nbytes of a lost cell is stored exactly
// once and never read; nothing beyond them is written; a survivor byte is
// written only with fix_survivors, and only a located one. The reports are
// the only other writes. No ring, no claim counter, no spin: no block waits
// on another, every loop bound is known at launch, and there is no
// __syncthreads and no LDS write after the prologue.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "codec_kernels.h"
#include "gf256.h"
#include "rebuild_checked_wide.h"

namespace redset_hip {

namespace {

constexpr int kWave = 64;
constexpr int kPerLane = kCheckedBlock / kWave;  // survivors whose points one lane evaluates (ns < 256)

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
struct CwLds {
  const uint2* tab;      // ns x 32 entries: survivor m, nibble half h, value n at m * 32 + h * 16 + n
  const uint8_t* ex;     // 512
  const uint8_t* lg;     // 256
  const uint8_t* invu;   // 256
  const uint8_t* alpha;  // 256
  __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) const {
    return (a != 0 && b != 0) ? ex[lg[a] + lg[b]] : 0u;
  }
  // a / b, b != 0
  __device__ __forceinline__ uint32_t div(uint32_t a, uint32_t b) const { return a != 0 ? ex[lg[a] + 255u - lg[b]] : 0u; }
  // survivor m's column of [C ; B] times x
  __device__ __forceinline__ uint2 image(int m, uint32_t x) const {
    const uint2 a = tab[m * 32 + (x & 15u)], b = tab[m * 32 + 16 + (x >> 4)];
    return make_uint2(a.x ^ b.x, a.y ^ b.y);
  }
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

// byte B (static after unrolling) of four packed columns as one dword
__device__ __forceinline__ uint32_t gather_row(int B, const uint32_t* lo, const uint32_t* hi) {
  const uint32_t* a = B < 4 ? lo : hi;
  const int sh = 8 * (B & 3);
  return ((a[0] >> sh) & 255u) | (((a[1] >> sh) & 255u) << 8) | (((a[2] >> sh) & 255u) << 16) |
         (((a[3] >> sh) & 255u) << 24);
}

__device__ __forceinline__ uint32_t wave_xor(uint32_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v ^= __shfl_xor(v, o, kWave);
  return v;
}

// What one wave found. Every member is a register of the lane it is named for.
template <int S>
struct WideChecker {
  static constexpr int T = S / 2;
  // the low S bytes of a packed column
  static constexpr uint32_t kLoMask = S >= 4 ? 0xFFFFFFFFu : (1u << (8 * (S & 3))) - 1u;
  static constexpr uint32_t kHiMask = S <= 4 ? 0u : (1u << (8 * (S - 4))) - 1u;
  const CheckedWideLaunch& L;
  const CheckedWideJob& J;
  const CwLds& M;
  const int lane;
  unsigned cnt[kPerLane];              // corrections of survivor lane + 64 q, whichever lane owned the column
  unsigned long long first[kPerLane];  // the first of them (a wave meets its columns in ascending order)
  unsigned ucnt;                       // unlocated columns this lane owns
  unsigned multi[kCwMaxT - 1];         // wave-uniform: columns corrected with nu = 2, 3 wrong bytes

  // Level nu (1 .. T) of the rule: true when the column is explained by nu
  // wrong survivor bytes, with their image under [C ; B] in `img`. P: the
  // sums, byte j = T_j; `off` and `owner`: the column and its lane. One body
  // for every nu: the system is padded to T x T with identity rows, so every
  // index is static.
  __device__ __forceinline__ bool level(int nu, unsigned long long P, size_t off, int owner, uint2& img) {
    constexpr int TT = T > 0 ? T : 1;
    auto sp = [&](int k) { return static_cast<uint32_t>(P >> (8 * (k < S ? k : S - 1))) & 255u; };
    // the Hankel system sum_k sigma_k T_(j+k) = T_(j+nu), j < nu: Gauss-Jordan
    uint32_t A[TT][TT + 1];
#pragma unroll
    for (int j = 0; j < TT; ++j) {
#pragma unroll
      for (int k = 0; k < TT; ++k) A[j][k] = (j < nu && k < nu) ? sp(j + k) : (j == k ? 1u : 0u);
      A[j][TT] = j < nu ? sp(j + nu) : 0u;
    }
    bool solved = true;
#pragma unroll
    for (int c = 0; c < TT; ++c) {
#pragma unroll
      for (int r = c + 1; r < TT; ++r) {
        const bool swap = A[c][c] == 0 && A[r][c] != 0;
#pragma unroll
        for (int k = c; k <= TT; ++k) {
          const uint32_t a = A[c][k], b = A[r][k];
          A[c][k] = swap ? b : a;
          A[r][k] = swap ? a : b;
        }
      }
      const uint32_t piv = A[c][c];
      solved = solved && piv != 0;
      const uint32_t pv = piv != 0 ? piv : 1u;
#pragma unroll
      for (int k = c; k <= TT; ++k) A[c][k] = M.div(A[c][k], pv);
#pragma unroll
      for (int r = 0; r < TT; ++r) {
        if (r == c) continue;
        const uint32_t f = A[r][c];
#pragma unroll
        for (int k = c; k <= TT; ++k) A[r][k] ^= M.mul(f, A[c][k]);
      }
    }
    if (!solved) return false;
    // the locator's coefficients c_0 .. c_T: sigma below nu, 1 at nu, 0 above
    uint32_t cf[TT + 1];
#pragma unroll
    for (int k = 0; k <= TT; ++k) cf[k] = (k < TT ? A[k][TT] : 0u) ^ (k == nu ? 1u : 0u);
    // every remaining equation
    uint32_t rest = 0;
#pragma unroll
    for (int j = 1; j + 1 < S; ++j) {
      uint32_t v = 0;
#pragma unroll
      for (int k = 0; k <= TT; ++k) v ^= M.mul(cf[k], sp(j + k));
      rest |= (j >= nu && j + nu < S) ? v : 0u;
    }
    if (rest != 0) return false;
    // roots among the survivors' points, error values where there is one
    const int n = L.ns;
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
        // b(z) = locator / (z ^ X), remainder locator(X): y = sum_k b_k T_k / b(X)
        uint32_t b = cf[TT], num = 0, den = 0;
#pragma unroll
        for (int k = TT - 1; k >= 0; --k) {
          num ^= M.mul(b, sp(k));
          den = M.mul(den, X) ^ b;
          b = M.mul(b, X) ^ cf[k];
        }
        root = b == 0;
        if (root) {
          xv[q] = den != 0 ? M.mul(M.div(num, den), M.invu[cell]) : 0u;
          zero_value |= xv[q] == 0 ? 1u : 0u;
          const uint2 mine = M.image(cell, xv[q]);
          own.x ^= mine.x;
          own.y ^= mine.y;
        }
      }
      roots[q] = __ballot(root);
      nroots += __popcll(roots[q]);
    }
    if (nroots != nu) return false;
    if (__ballot(zero_value != 0) != 0) return false;
    // the guard: what is proposed must give these very sums
    const uint2 all = make_uint2(wave_xor(own.x), wave_xor(own.y));
    if ((all.x & kLoMask) != static_cast<uint32_t>(P) || (all.y & kHiMask) != static_cast<uint32_t>(P >> 32)) return false;
    img = all;
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
      if (q * kWave >= n) continue;
      if ((roots[q] >> lane) & 1ull) {
        if (cnt[q] == 0) first[q] = L.base + off;
        ++cnt[q];
      }
      if (!L.fix_survivors) continue;
      // at most nu bits over all q
      for (unsigned long long mask = roots[q]; mask != 0; mask &= mask - 1) {
        const int src = __ffsll(mask) - 1;
        const uint32_t x = __shfl(xv[q], src, kWave);
        if (lane == owner) {
          uint8_t* b = J.in[src + q * kWave] + off;
          *b = static_cast<uint8_t>(*b ^ x);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kCwMaxT - 1; ++i) multi[i] += nu == i + 2 ? 1u : 0u;
    return true;
  }

  // The column at cell offset `off`, owned by lane `owner`, has the nonzero
  // sums (lo, hi), already masked; returns what to XOR into its accumulator.
  __device__ __forceinline__ uint2 column(size_t off, uint32_t lo, uint32_t hi, int owner) {
    const unsigned long long P64 = (static_cast<unsigned long long>(hi) << 32) | lo;
    uint2 img = make_uint2(0u, 0u);
    bool done = false;
    if (T > 0) {
#pragma unroll 1
      for (int nu = 1; nu <= L.max_errors && !done; ++nu) done = level(nu, P64, off, owner, img);
    }
    if (!done && lane == owner) {
      if (ucnt == 0) atomicMin(L.stripe_report + L.nstripes + J.row, L.base + off);
      ++ucnt;
    }
    return img;
  }

  // One step of the wave: lane l holds the columns at cell offsets first_off +
  // l * stride + c, c < 16, packed in (lo[c], hi[c]) (zero for a column that
  // is not there). Located errors are taken out of the owner's columns.
  __device__ __forceinline__ void step(size_t first_off, int stride, uint32_t (&lo)[16], uint32_t (&hi)[16]) {
    uint32_t cm = 0;
#pragma unroll
    for (int c = 0; c < 16; ++c) cm |= ((lo[c] & kLoMask) | (hi[c] & kHiMask)) != 0 ? 1u << c : 0u;
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
        const uint2 img = column(first_off + static_cast<size_t>(owner) * stride + c, __shfl(a & kLoMask, owner, kWave),
                                 __shfl(b & kHiMask, owner, kWave), owner);
        const bool mine = lane == owner;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          lo[i] ^= (mine && i == c) ? img.x : 0u;
          hi[i] ^= (mine && i == c) ? img.y : 0u;
        }
      }
    }
  }

  __device__ __forceinline__ void finish() {
#pragma unroll
    for (int q = 0; q < kPerLane; ++q) {
      const int cell = lane + q * kWave;
      if (cell >= L.ns || cnt[q] == 0) continue;
      const size_t at = static_cast<size_t>(J.row) * L.p + J.member[cell];
      atomicAdd(L.cell_report + at, static_cast<unsigned long long>(cnt[q]));
      atomicMin(L.cell_report + L.ncells + at, first[q]);
    }
    if (ucnt != 0) atomicAdd(L.stripe_report + J.row, static_cast<unsigned long long>(ucnt));
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kCwMaxT - 1; ++i)
        if (multi[i] != 0)
          atomicAdd(L.multi_report + static_cast<size_t>(J.row) * (kCwMaxT - 1) + i,
                    static_cast<unsigned long long>(multi[i]));
    }
  }
};

template <int S>
__global__ __launch_bounds__(kCheckedBlock) void gf_rebuild_checked_wide_kernel(CheckedWideLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int ns = L.ns, k = L.k;
  const int job = blockIdx.x / L.blocks_per_job, blk = blockIdx.x % L.blocks_per_job;
  if (job >= L.njobs) return;
  const CheckedWideJob J = L.jobs[job];
  uint2* tab = reinterpret_cast<uint2*>(lds);
  uint8_t* bytes = reinterpret_cast<uint8_t*>(tab + ns * 32);
  for (int t = threadIdx.x; t < ns * 32; t += kCheckedBlock) {
    const int i = t >> 5, h = (t >> 4) & 1, n = t & 15;
    const uint32_t x = static_cast<uint32_t>(n) << (4 * h);
    uint2 v = make_uint2(0u, 0u);
#pragma unroll
    for (int j = 0; j < kWideMaxE; ++j) {
      if (j >= S + k) break;
      const uint32_t m = gf_mul_bits(J.coef[j * ns + i], x);
      if (j < 4) v.x |= m << (8 * j);
      else v.y |= m << (8 * (j - 4));
    }
    tab[t] = v;
  }
  {
    const int t = threadIdx.x;  // kCheckedBlock == 256: one entry of every table per thread
    bytes[t] = L.gf[t];
    bytes[256 + t] = L.gf[256 + t];
    bytes[512 + t] = L.gf[512 + t];
    bytes[768 + t] = t < ns ? J.invu[t] : 0;
    bytes[1024 + t] = t < ns ? J.alpha[t] : 0;
  }
  __syncthreads();

  const CwLds M{tab, bytes, bytes + 512, bytes + 768, bytes + 1024};
  const int lane = threadIdx.x & (kWave - 1);
  WideChecker<S> R{L, J, M, lane, {0u, 0u, 0u, 0u}, {0ull, 0ull, 0ull, 0ull}, 0u, {0u, 0u}};
  const size_t step = static_cast<size_t>(L.blocks_per_job) * kCheckedBlock;
  const size_t lane0 = static_cast<size_t>(blk) * kCheckedBlock + threadIdx.x;
  const size_t nvec = J.bytes_only ? 0 : L.nbytes / 16;

  // Every lane of the block runs the same number of steps, since the damaged
  // path needs whole waves: the 16-B steps, then byte columns -- the whole job
  // when a cell is unaligned, else the tail after the last whole vector
  // (block 0 of the job).
  const size_t vsteps = (nvec + step - 1) / step;
  const size_t b0 = nvec * 16;
  const bool bytes_here = J.bytes_only || blk == 0;
  const size_t bstep = J.bytes_only ? step : kCheckedBlock;
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
      for (; m + 4 <= ns; m += 4) {
        const uint4 x0 = reinterpret_cast<const uint4*>(J.in[m])[v];
        const uint4 x1 = reinterpret_cast<const uint4*>(J.in[m + 1])[v];
        const uint4 x2 = reinterpret_cast<const uint4*>(J.in[m + 2])[v];
        const uint4 x3 = reinterpret_cast<const uint4*>(J.in[m + 3])[v];
        acc_vec(tab + m * 32, x0, lo, hi);
        acc_vec(tab + (m + 1) * 32, x1, lo, hi);
        acc_vec(tab + (m + 2) * 32, x2, lo, hi);
        acc_vec(tab + (m + 3) * 32, x3, lo, hi);
      }
      for (; m < ns; ++m) acc_vec(tab + m * 32, reinterpret_cast<const uint4*>(J.in[m])[v], lo, hi);
    } else if (!vec && o < L.nbytes) {
      for (int m = 0; m < ns; ++m) {
        const uint32_t b = J.in[m][o];
        const uint2 x = tab[m * 32 + (b & 15u)], y = tab[m * 32 + 16 + (b >> 4)];
        lo[0] ^= x.x ^ y.x;
        hi[0] ^= x.y ^ y.y;
      }
    }
    if (vec) R.step((v - lane) * 16, 16, lo, hi);
    else R.step(o - lane, 1, lo, hi);
    // the rebuilt bytes: byte S + i of every packed column is lost cell i's
    if (vec && v < nvec) {
#pragma unroll
      for (int i = 0; i < kWideMaxE - S; ++i) {
        if (i >= k) break;
        uint4 w;
        w.x = gather_row(S + i, lo, hi);
        w.y = gather_row(S + i, lo + 4, hi + 4);
        w.z = gather_row(S + i, lo + 8, hi + 8);
        w.w = gather_row(S + i, lo + 12, hi + 12);
        reinterpret_cast<uint4*>(J.out[i])[v] = w;
      }
    } else if (!vec && o < L.nbytes) {
#pragma unroll
      for (int i = 0; i < kWideMaxE - S; ++i) {
        if (i >= k) break;
        J.out[i][o] = static_cast<uint8_t>(gather_row(S + i, lo, hi));
      }
    }
  }
  R.finish();
}

__global__ __launch_bounds__(kCheckedBlock) void checked_wide_reset_kernel(CheckedWideLaunch L) {
  for (int i = threadIdx.x; i < L.ncells; i += kCheckedBlock) {
    L.cell_report[i] = 0;
    L.cell_report[L.ncells + i] = ~0ull;
  }
  for (int i = threadIdx.x; i < L.nstripes; i += kCheckedBlock) {
    L.stripe_report[i] = 0;
    L.stripe_report[L.nstripes + i] = ~0ull;
  }
  for (int i = threadIdx.x; i < L.nstripes * (kCwMaxT - 1); i += kCheckedBlock) L.multi_report[i] = 0;
}

size_t up16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

template <int S>
hipError_t prepare(size_t bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&gf_rebuild_checked_wide_kernel<S>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
}

template <int S>
void launch(const CheckedWideLaunch& L, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(gf_rebuild_checked_wide_kernel<S>, grid, dim3(kCheckedBlock), checked_wide_lds_bytes(L.ns), stream,
                     L);
}

}  // namespace

size_t checked_wide_lds_bytes(int ns) { return static_cast<size_t>(ns) * 256 + 1280; }

int checked_wide_prepare(int ns, int s) {
  if (ns < 1 || ns >= kCheckedBlock || checked_wide_lds_bytes(ns) > kWideLdsLimit) return hipErrorInvalidValue;
  // the most survivors a stripe can have, so that a later, narrower plan never lowers it
  const size_t bytes = checked_wide_lds_bytes(kCheckedBlock - 1);
  switch (s) {
    case 1: return prepare<1>(bytes);
    case 2: return prepare<2>(bytes);
    case 3: return prepare<3>(bytes);
    case 4: return prepare<4>(bytes);
    case 5: return prepare<5>(bytes);
    case 6: return prepare<6>(bytes);
    case 7: return prepare<7>(bytes);
  }
  return hipErrorInvalidValue;
}

int checked_wide_upload(const std::vector<CheckedWideJobDesc>& jobs, int ns, int e, int k, void** blob_out,
                        CheckedWideLaunch& L) {
  *blob_out = nullptr;
  L.jobs = nullptr;
  L.gf = nullptr;
  const size_t n = jobs.size();
  // the field tables, the job array, then per job: survivor pointers, output
  // pointers, member indices, coefficients, points, 1 / u'
  const size_t o_jobs = 768;
  const size_t o_per = o_jobs + up16(n * sizeof(CheckedWideJob));
  const size_t s_in = up16(static_cast<size_t>(ns) * sizeof(uint8_t*));
  const size_t s_out = up16(static_cast<size_t>(k) * sizeof(uint8_t*));
  const size_t s_member = up16(static_cast<size_t>(ns) * sizeof(int));
  const size_t s_coef = up16(static_cast<size_t>(e) * ns);
  const size_t s_ns = up16(static_cast<size_t>(ns));
  const size_t per = s_in + s_out + s_member + s_coef + 2 * s_ns;
  const size_t bytes = o_per + n * per;
  void* dev = nullptr;
  if (hipError_t err = hipMalloc(&dev, bytes)) return err;
  std::vector<char> host(bytes, 0);
  char* const dbase = static_cast<char*>(dev);
  const Field& F = field();
  std::memcpy(host.data(), F.exp_, 512);
  std::memcpy(host.data() + 512, F.log_, 256);
  for (size_t q = 0; q < n; ++q) {
    const CheckedWideJobDesc& D = jobs[q];
    const size_t o = o_per + q * per;
    uint8_t** in = reinterpret_cast<uint8_t**>(host.data() + o);
    uint8_t** out = reinterpret_cast<uint8_t**>(host.data() + o + s_in);
    int* member = reinterpret_cast<int*>(host.data() + o + s_in + s_out);
    uint8_t* coef = reinterpret_cast<uint8_t*>(host.data() + o + s_in + s_out + s_member);
    uint8_t* alpha = coef + s_coef;
    uint8_t* invu = alpha + s_ns;
    bool al = true;
    for (int i = 0; i < ns; ++i) {
      in[i] = D.cells.in[static_cast<size_t>(i)];
      member[i] = D.cells.member[static_cast<size_t>(i)];
      alpha[i] = D.alpha[static_cast<size_t>(i)];
      invu[i] = D.invu[static_cast<size_t>(i)];
      al = al && (reinterpret_cast<uintptr_t>(in[i]) & 15u) == 0;
    }
    for (int i = 0; i < k; ++i) {
      out[i] = D.cells.out[static_cast<size_t>(i)];
      al = al && (reinterpret_cast<uintptr_t>(out[i]) & 15u) == 0;
    }
    std::memcpy(coef, D.cells.coef.data(), static_cast<size_t>(e) * ns);
    CheckedWideJob J;
    std::memset(&J, 0, sizeof(J));
    J.in = reinterpret_cast<uint8_t* const*>(dbase + o);
    J.out = reinterpret_cast<uint8_t* const*>(dbase + o + s_in);
    J.member = reinterpret_cast<const int*>(dbase + o + s_in + s_out);
    J.coef = reinterpret_cast<const uint8_t*>(dbase + o + s_in + s_out + s_member);
    J.alpha = J.coef + s_coef;
    J.invu = J.alpha + s_ns;
    J.row = D.cells.row;
    J.bytes_only = al ? 0 : 1;
    std::memcpy(host.data() + o_jobs + q * sizeof(CheckedWideJob), &J, sizeof(J));
  }
  if (hipError_t err = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice)) {
    (void) hipFree(dev);
    return err;
  }
  *blob_out = dev;
  L.gf = reinterpret_cast<const uint8_t*>(dev);
  L.jobs = reinterpret_cast<const CheckedWideJob*>(dbase + o_jobs);
  return hipSuccess;
}

int launch_checked_wide_reset(const CheckedWideLaunch& L, void* stream) {
  hipLaunchKernelGGL(checked_wide_reset_kernel, dim3(1), dim3(kCheckedBlock), 0, static_cast<hipStream_t>(stream), L);
  return hipGetLastError();
}

int launch_checked_wide(const CheckedWideLaunch& L, void* stream) {
  if (L.njobs <= 0 || L.nbytes == 0) return hipSuccess;
  const int s = L.e - L.k;
  if (L.e < kWideMinE || L.e > kWideMaxE || L.k < 1 || s < 1 || L.ns < 1 || L.ns >= kCheckedBlock ||
      L.blocks_per_job < 1 || !L.jobs || !L.gf || L.max_errors < 0 || L.max_errors > s / 2)
    return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(L.njobs) * static_cast<unsigned>(L.blocks_per_job));
  const hipStream_t st = static_cast<hipStream_t>(stream);
  switch (s) {
    case 1: launch<1>(L, grid, st); break;
    case 2: launch<2>(L, grid, st); break;
    case 3: launch<3>(L, grid, st); break;
    case 4: launch<4>(L, grid, st); break;
    case 5: launch<5>(L, grid, st); break;
    case 6: launch<6>(L, grid, st); break;
    default: launch<7>(L, grid, st); break;
  }
  return hipGetLastError();
}

}  // namespace redset_hip
