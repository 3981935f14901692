// repair2_kernels.hip -- column-wise repair of RS stripes with four parity
// rows, up to two wrong bytes per byte column (gfx950); descriptors in
// repair2.h, the arithmetic in include/redset_hip.h ("repair2").
//
// gf_repair2_kernel: one job is one stripe of d data cells and 4 stored parity
// cells, 256-thread blocks, blocks_per_job of them side by side over the
// columns. Where the work goes:
//
// * Clean columns, the common case, are gf_repair_kernel's: the encode's
//   nibble tables of the d inputs in LDS (128 B per input, each entry packing
//   the products for the 4 parity rows into one dword), so the packed
//   syndrome S costs two LDS reads per data byte; 16-B global loads, four
//   inputs in flight; a lane whose 16 columns all have S == 0 goes on. Jobs
//   with an unaligned cell and the tail after the last whole vector take
//   byte columns.
//
// * A damaged column leaves the A basis at once. Eight more LDS reads (the
//   nibble tables of W^-1) turn S into the power sums S'_t = sum y_i X_i^t,
//   t = 0..3, over the wrong cells' points X_i, and everything after that is
//   O(1) field arithmetic on log/exp tables:
//     one wrong byte   X = S'1 / S'0, S'2 = S'1 X, S'3 = S'2 X; the cell is
//                      map[X], the error S'0 / u. No loop over the d inputs.
//     two wrong bytes  D = S'0 S'2 ^ S'1^2, sigma1 = (S'0 S'3 ^ S'1 S'2) / D,
//                      sigma2 = (S'2^2 ^ S'1 S'3) / D; the roots of
//                      z^2 ^ sigma1 z ^ sigma2 are sigma1 Q[sigma2 / sigma1^2]
//                      and that ^ sigma1, Q[c] solving w^2 ^ w = c (half of
//                      all c have no solution: flag 0x100); both must be
//                      points of cells of the stripe; y1 = (S'0 X2 ^ S'1) /
//                      sigma1, y2 = S'0 ^ y1, the errors y / u.
//   Whatever this proposes is applied only if its own syndrome, taken from
//   the input tables and the parity unit columns, equals S.
//
// LDS, dwords: [0, 32 d) input tables | 128 W^-1 nibble tables | 128 Q
// (16-bit entries) | 128 exp (2^i, i < 512) | 64 log | 64 map alpha -> cell
// (0xFF: no cell of this stripe) | 64 1/u per cell | 64 alpha per cell:
// 128 d + 2560 bytes, 34816 at d = 252.
//
// Footprint: a correction is a one-byte read-modify-write of a wrong byte by
// the lane that owns the column, one or two per column; nothing else is
// stored to a cell, and dry runs and unlocated columns store nothing. The
// reports are the only other writes (64-bit atomics from lanes that found
// something). No block waits on another: no ring, no claim counter, no spin,
// and the kernel has no access to the ring-fault and hang-fault words. Every
// loop bound is known at launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "codec_kernels.h"
#include "gf256.h"
#include "repair2.h"

namespace redset_hip {

namespace {

constexpr int kW = 0, kQ = 128, kExp = 256, kLog = 384, kMap = 448, kInvU = 512, kAlpha = 576, kAuxWords = 640;

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

// a[b] ^= packed products of byte b of w, b = 0..3 (T: the input's tables)
__device__ __forceinline__ void acc_word(const uint32_t* T, uint32_t w, uint32_t* a) {
#pragma unroll
  for (int b = 0; b < 4; ++b) a[b] ^= T[(w >> (8 * b)) & 15u] ^ T[16 + ((w >> (8 * b + 4)) & 15u)];
}

__device__ __forceinline__ void acc_vec(const uint32_t* T, const uint4& x, uint32_t (&acc)[16]) {
  acc_word(T, x.x, acc);
  acc_word(T, x.y, acc + 4);
  acc_word(T, x.z, acc + 8);
  acc_word(T, x.w, acc + 12);
}

// byte j of a0..a3 as one dword
__device__ __forceinline__ uint32_t gather_row(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, int j) {
  return ((a0 >> (8 * j)) & 255u) | (((a1 >> (8 * j)) & 255u) << 8) | (((a2 >> (8 * j)) & 255u) << 16) |
         (((a3 >> (8 * j)) & 255u) << 24);
}

__device__ __forceinline__ uint32_t word_of(const uint4& r, int q) {
  return q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w;
}

// What one lane found, and where it goes. A lane meets its columns in
// ascending order, so the first column of a run of corrections to one cell is
// the smallest of that run: it goes to the report's offset word at once, the
// count when the run ends. Two runs are open at a time, one per byte of a
// pair, so that a stretch damaged in two members costs two atomics a lane.
struct Repairer2 {
  const Repair2Launch& L;
  const Repair2Job& J;
  const uint32_t* tab;  // LDS: d x 32 words
  const uint32_t* aux;  // LDS: the power-basis tables
  int cur0, cur1;       // cells of the open runs (-1: none)
  unsigned cnt0, cnt1, ucnt, pcnt;

  __device__ __forceinline__ uint32_t lg(uint32_t a) const { return reinterpret_cast<const uint8_t*>(aux + kLog)[a]; }
  __device__ __forceinline__ uint32_t ex(uint32_t i) const { return reinterpret_cast<const uint8_t*>(aux + kExp)[i]; }
  __device__ __forceinline__ uint32_t mul(uint32_t a, uint32_t b) const {
    return (a != 0 && b != 0) ? ex(lg(a) + lg(b)) : 0u;
  }
  // a / b, b != 0
  __device__ __forceinline__ uint32_t div(uint32_t a, uint32_t b) const { return a != 0 ? ex(lg(a) + 255u - lg(b)) : 0u; }
  // the packed syndrome of error x in `cell`
  __device__ __forceinline__ uint32_t syndrome_of(int cell, uint32_t x) const {
    return cell < L.d ? tab[cell * 32 + (x & 15u)] ^ tab[cell * 32 + 16 + (x >> 4)] : x << (8 * (cell - L.d));
  }

  __device__ __forceinline__ void flush(int cell, unsigned& cnt) {
    if (cell >= 0 && cnt != 0)
      atomicAdd(L.cell_report + static_cast<size_t>(J.row) * L.p + J.member[cell], static_cast<unsigned long long>(cnt));
    cnt = 0;
  }
  __device__ __forceinline__ void finish() {
    flush(cur0, cnt0);
    flush(cur1, cnt1);
    if (ucnt != 0) atomicAdd(L.stripe_report + J.row, static_cast<unsigned long long>(ucnt));
    if (pcnt != 0) atomicAdd(L.pair_report + J.row, static_cast<unsigned long long>(pcnt));
  }
  __device__ __forceinline__ void correct(int& cur, unsigned& cnt, int cell, uint32_t x, size_t off) {
    if (cell != cur) {
      flush(cur, cnt);
      cur = cell;
      atomicMin(L.cell_report + L.ncells + static_cast<size_t>(J.row) * L.p + J.member[cell], L.base + off);
    }
    ++cnt;
    if (L.apply) {
      uint8_t* b = J.cells[cell] + off;
      *b = static_cast<uint8_t>(*b ^ x);
    }
  }

  // the column at cell offset `off` has the nonzero packed syndrome S
  __device__ __forceinline__ void column(size_t off, uint32_t S) {
    const uint8_t* map = reinterpret_cast<const uint8_t*>(aux + kMap);
    const uint8_t* invu = reinterpret_cast<const uint8_t*>(aux + kInvU);
    uint32_t P = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t b = (S >> (8 * k)) & 255u;
      P ^= aux[kW + k * 32 + (b & 15u)] ^ aux[kW + k * 32 + 16 + (b >> 4)];
    }
    const uint32_t s0 = P & 255u, s1 = (P >> 8) & 255u, s2 = (P >> 16) & 255u, s3 = P >> 24;
    int c1 = -1, c2 = -1;
    uint32_t x1 = 0, x2 = 0;
    const uint32_t X = s0 != 0 ? div(s1, s0) : 0u;
    if (s0 != 0 && mul(s1, X) == s2 && mul(s2, X) == s3) {
      // one wrong byte at point X, if that is a cell of this stripe
      const int cell = map[X];
      if (cell != 0xFF) c1 = cell, x1 = mul(s0, invu[cell]);
    } else {
      const uint32_t D = mul(s0, s2) ^ mul(s1, s1);
      const uint32_t g1 = D != 0 ? div(mul(s0, s3) ^ mul(s1, s2), D) : 0u;
      if (g1 != 0) {  // g1 == 0: no two distinct roots
        const uint32_t g2 = div(mul(s2, s2) ^ mul(s1, s3), D);
        const uint32_t q = reinterpret_cast<const uint16_t*>(aux + kQ)[div(g2, mul(g1, g1))];
        const uint32_t X1 = mul(g1, q & 255u), X2 = X1 ^ g1;
        const int a = map[X1], b = map[X2];
        if (q < 0x100u && a != 0xFF && b != 0xFF) {
          const uint32_t y1 = div(mul(s0, X2) ^ s1, g1);
          const uint32_t v1 = mul(y1, invu[a]), v2 = mul(s0 ^ y1, invu[b]);
          if (v1 != 0 && v2 != 0) {
            // ascending cell order: a stretch damaged in the same two cells keeps its two runs
            c1 = a < b ? a : b;
            c2 = a < b ? b : a;
            x1 = a < b ? v1 : v2;
            x2 = a < b ? v2 : v1;
          }
        }
      }
    }
    // the guard: what is proposed must give this very syndrome
    uint32_t own = 0;
    if (c1 >= 0) own ^= syndrome_of(c1, x1);
    if (c2 >= 0) own ^= syndrome_of(c2, x2);
    if (c1 < 0 || own != S) {
      if (ucnt == 0) atomicMin(L.stripe_report + L.nstripes + J.row, L.base + off);
      ++ucnt;
      return;
    }
    correct(cur0, cnt0, c1, x1, off);
    if (c2 >= 0) {
      correct(cur1, cnt1, c2, x2, off);
      ++pcnt;
    }
  }
};

__global__ __launch_bounds__(kRepairBlock) void gf_repair2_kernel(Repair2Launch L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr int E = kRepair2E;
  const int d = L.d;
  const int job = blockIdx.x / L.blocks_per_job, blk = blockIdx.x % L.blocks_per_job;
  if (job >= L.njobs) return;
  const Repair2Job J = L.jobs[job];
  uint32_t* aux = lds + d * 32;
  for (int t = threadIdx.x; t < d * 32; t += kRepairBlock) {
    const int i = t >> 5, h = (t >> 4) & 1, n = t & 15;
    const uint32_t x = static_cast<uint32_t>(n) << (4 * h);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) v |= gf_mul_bits(J.coef[j * d + i], x) << (8 * j);
    lds[t] = v;
  }
  {
    const int t = threadIdx.x;  // kRepairBlock == 256: one entry of every table per thread
    uint8_t* bytes = reinterpret_cast<uint8_t*>(aux);
    if (t < 128) {
      // W^-1 nibble tables: syndrome byte k = t >> 5, nibble h, value n -> the four power sums' share
      const int k = t >> 5, h = (t >> 4) & 1, n = t & 15;
      const uint32_t x = static_cast<uint32_t>(n) << (4 * h);
      uint32_t v = 0;
#pragma unroll
      for (int r = 0; r < E; ++r) v |= gf_mul_bits(L.jobs[job].winv[r * E + k], x) << (8 * r);  // from global: no indexed copy
      aux[kW + t] = v;
    }
    reinterpret_cast<uint16_t*>(aux + kQ)[t] = 0x100;
    bytes[4 * kExp + t] = L.gf[t];
    bytes[4 * kExp + 256 + t] = L.gf[256 + t];
    bytes[4 * kLog + t] = L.gf[512 + t];
    bytes[4 * kMap + t] = 0xFF;
    if (t < d + E) {
      bytes[4 * kInvU + t] = J.invu[t];
      bytes[4 * kAlpha + t] = J.alpha[t];
    }
    __syncthreads();
    // w and w ^ 1 solve the same c: the even one writes
    if ((t & 1) == 0) reinterpret_cast<uint16_t*>(aux + kQ)[gf_mul_bits(t, t) ^ t] = static_cast<uint16_t>(t);
    if (t < d + E) bytes[4 * kMap + bytes[4 * kAlpha + t]] = static_cast<uint8_t>(t);
  }
  __syncthreads();

  Repairer2 R{L, J, lds, aux, -1, -1, 0u, 0u, 0u, 0u};
  const size_t step = static_cast<size_t>(L.blocks_per_job) * kRepairBlock;
  const size_t lane0 = static_cast<size_t>(blk) * kRepairBlock + threadIdx.x;
  const size_t nvec = J.bytes_only ? 0 : L.nbytes / 16;

  for (size_t v = lane0; v < nvec; v += step) {
    uint32_t acc[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) acc[b] = 0;
    int m = 0;
    for (; m + 4 <= d; m += 4) {
      const uint4 x0 = reinterpret_cast<const uint4*>(J.cells[m])[v];
      const uint4 x1 = reinterpret_cast<const uint4*>(J.cells[m + 1])[v];
      const uint4 x2 = reinterpret_cast<const uint4*>(J.cells[m + 2])[v];
      const uint4 x3 = reinterpret_cast<const uint4*>(J.cells[m + 3])[v];
      acc_vec(lds + m * 32, x0, acc);
      acc_vec(lds + (m + 1) * 32, x1, acc);
      acc_vec(lds + (m + 2) * 32, x2, acc);
      acc_vec(lds + (m + 3) * 32, x3, acc);
    }
    for (; m < d; ++m) acc_vec(lds + m * 32, reinterpret_cast<const uint4*>(J.cells[m])[v], acc);
    // r[j] = the syndrome of row j over the 16 columns
    uint4 r[E];
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) {
      r[j] = reinterpret_cast<const uint4*>(J.cells[d + j])[v];
      r[j].x ^= gather_row(acc[0], acc[1], acc[2], acc[3], j);
      r[j].y ^= gather_row(acc[4], acc[5], acc[6], acc[7], j);
      r[j].z ^= gather_row(acc[8], acc[9], acc[10], acc[11], j);
      r[j].w ^= gather_row(acc[12], acc[13], acc[14], acc[15], j);
      any |= r[j].x | r[j].y | r[j].z | r[j].w;
    }
    if (any == 0) continue;
#pragma unroll 1
    for (int col = 0; col < 16; ++col) {
      uint32_t S = 0;
#pragma unroll
      for (int j = 0; j < E; ++j) S |= ((word_of(r[j], col >> 2) >> (8 * (col & 3))) & 255u) << (8 * j);
      if (S != 0) R.column(v * 16 + col, S);
    }
  }

  // byte columns: the whole job when a cell is unaligned, else the tail after
  // the last whole vector (block 0 of the job)
  const size_t b0 = nvec * 16;
  if (J.bytes_only || blk == 0) {
    for (size_t o = b0 + (J.bytes_only ? lane0 : threadIdx.x); o < L.nbytes; o += J.bytes_only ? step : kRepairBlock) {
      uint32_t S = 0;
      for (int m = 0; m < d; ++m) {
        const uint32_t b = J.cells[m][o];
        S ^= lds[m * 32 + (b & 15u)] ^ lds[m * 32 + 16 + (b >> 4)];
      }
#pragma unroll
      for (int j = 0; j < E; ++j) S ^= static_cast<uint32_t>(J.cells[d + j][o]) << (8 * j);
      if (S != 0) R.column(o, S);
    }
  }
  R.finish();
}

__global__ __launch_bounds__(kRepairBlock) void repair2_reset_kernel(Repair2Launch L) {
  for (int i = threadIdx.x; i < L.ncells; i += kRepairBlock) {
    L.cell_report[i] = 0;
    L.cell_report[L.ncells + i] = ~0ull;
  }
  for (int i = threadIdx.x; i < L.nstripes; i += kRepairBlock) {
    L.stripe_report[i] = 0;
    L.stripe_report[L.nstripes + i] = ~0ull;
    L.pair_report[i] = 0;
  }
}

size_t up16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

}  // namespace

size_t repair2_lds_bytes(int d) { return static_cast<size_t>(d) * 128 + kAuxWords * 4; }

int repair2_upload(const std::vector<Repair2JobDesc>& jobs, int d, void** blob_out, Repair2Launch& L) {
  *blob_out = nullptr;
  L.jobs = nullptr;
  L.gf = nullptr;
  const size_t n = jobs.size();
  const int e = kRepair2E;
  // the field tables, the job array, then per job: cell pointers, member
  // indices, coefficients, points, 1/u
  const size_t o_jobs = 768;
  const size_t o_per = o_jobs + up16(n * sizeof(Repair2Job));
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
    const Repair2JobDesc& D = jobs[k];
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
    Repair2Job J;
    J.cells = reinterpret_cast<uint8_t* const*>(dbase + o);
    J.member = reinterpret_cast<const int*>(dbase + o + s_cells);
    J.coef = reinterpret_cast<const uint8_t*>(dbase + o + s_cells + s_member);
    J.alpha = J.coef + s_coef;
    J.invu = J.alpha + s_n;
    std::memcpy(J.winv, D.winv, sizeof(J.winv));
    J.row = D.cells.row;
    J.bytes_only = al ? 0 : 1;
    std::memcpy(host.data() + o_jobs + k * sizeof(Repair2Job), &J, sizeof(J));
  }
  if (hipError_t err = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice)) {
    (void) hipFree(dev);
    return err;
  }
  *blob_out = dev;
  L.gf = reinterpret_cast<const uint8_t*>(dev);
  L.jobs = reinterpret_cast<const Repair2Job*>(dbase + o_jobs);
  return hipSuccess;
}

int launch_repair2_reset(const Repair2Launch& L, void* stream) {
  hipLaunchKernelGGL(repair2_reset_kernel, dim3(1), dim3(kRepairBlock), 0, static_cast<hipStream_t>(stream), L);
  return hipGetLastError();
}

int launch_repair2(const Repair2Launch& L, void* stream) {
  if (L.njobs <= 0 || L.nbytes == 0) return hipSuccess;
  if (L.d < 1 || L.d + kRepair2E > kRepairBlock || L.blocks_per_job < 1 || !L.jobs || !L.gf) return hipErrorInvalidValue;
  const dim3 grid(static_cast<unsigned>(L.njobs) * static_cast<unsigned>(L.blocks_per_job));
  hipLaunchKernelGGL(gf_repair2_kernel, grid, dim3(kRepairBlock), repair2_lds_bytes(L.d), static_cast<hipStream_t>(stream),
                     L);
  return hipGetLastError();
}

}  // namespace redset_hip
