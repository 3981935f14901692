// repair_kernels.hip -- column-wise locate and repair of damaged RS stripes
// in device memory (gfx950); descriptors in repair.h.
//
// gf_repair_kernel<E>: one job is one stripe of d data cells and E stored
// parity cells. The block builds the encode's nibble tables for all d inputs
// in LDS (codec_device.h: input m's low-nibble table at word 32 m, its
// high-nibble table 16 words on, each entry packing the products for the E
// parity rows into one dword: 128 B per input, 32 KiB at d = 254), so the
// packed syndrome of a byte column
//   S = sum_m T_m[data_m]  ^  (stored parity row j) << 8 j
// costs two LDS reads per data byte. A lane takes a 16-B position of every
// cell (16-B global loads; S == 0 for all 16 columns is the fast path) or, in
// jobs with a cell that is not 16-B aligned and in the tail after the last
// whole vector, single byte columns.
//
// A nonzero column is located exactly as redset_hip_rs_locate_syndrome does
// on the host: one nonzero row i -> parity row i's byte is wrong by s[i];
// otherwise, over the data inputs m in order, x = s[j0] / A[j0][m] (j0 = the
// first row with a nonzero coefficient; the host precomputes j0 and the
// inverse) explains the column when x != 0 and A[.][m] * x == S, which is
// T_m[x] == S with the tables already in LDS; exactly one such m is the
// answer, none or several leave the column unlocated and untouched.
//
// Footprint: a correction is a one-byte read-modify-write of the one wrong
// byte, by the lane that owns the column; nothing else is stored to a cell.
// The reports are the only other writes (64-bit atomics from lanes that found
// something). No block waits on another: no ring, no claim counter, no spin,
// and the kernel has no access to the ring-fault and hang-fault words.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "codec_kernels.h"
#include "gf256.h"
#include "repair.h"

namespace redset_hip {

namespace {

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
// ascending order, so the first column of a run of corrections to one cell
// (and its first unlocated column) is the smallest of that run: it goes to
// the report's offset word at once, the counts when the run ends.
template <int E>
struct Repairer {
  const RepairLaunch& L;
  const RepairJob& J;
  const uint32_t* tab;  // LDS: d x 32 words
  const uint8_t* aux;   // LDS: d inverses, then d rows j0
  int cur;              // cell of the open run of corrections (-1: none)
  unsigned cnt, ucnt;

  __device__ __forceinline__ void flush_run() {
    if (cur >= 0 && cnt != 0)
      atomicAdd(L.cell_report + static_cast<size_t>(J.row) * L.p + J.member[cur], static_cast<unsigned long long>(cnt));
    cnt = 0;
  }
  __device__ __forceinline__ void finish() {
    flush_run();
    if (ucnt != 0) atomicAdd(L.stripe_report + J.row, static_cast<unsigned long long>(ucnt));
  }

  // the column at cell offset `off` has the nonzero packed syndrome S
  __device__ __forceinline__ void column(size_t off, uint32_t S) {
    const int d = L.d;
    int nz = 0, only = 0;
#pragma unroll
    for (int j = 0; j < E; ++j)
      if ((S >> (8 * j)) & 255u) ++nz, only = j;
    int cell = -1;
    uint32_t x = 0;
    if (nz == 1) {
      cell = d + only;
      x = (S >> (8 * only)) & 255u;
    } else {
      int matches = 0;
      for (int m = 0; m < d; ++m) {
        const uint32_t xm = gf_mul_bits((S >> (8 * aux[d + m])) & 255u, aux[m]);
        const uint32_t prod = tab[m * 32 + (xm & 15u)] ^ tab[m * 32 + 16 + (xm >> 4)];
        if (xm != 0 && prod == S) {
          cell = m;
          x = xm;
          ++matches;
        }
      }
      if (matches != 1) cell = -1;
    }
    const unsigned long long where = L.base + off;
    if (cell < 0) {
      if (ucnt == 0) atomicMin(L.stripe_report + L.nstripes + J.row, where);
      ++ucnt;
      return;
    }
    if (cell != cur) {
      flush_run();
      cur = cell;
      atomicMin(L.cell_report + L.ncells + static_cast<size_t>(J.row) * L.p + J.member[cell], where);
    }
    ++cnt;
    if (L.apply) {
      uint8_t* b = J.cells[cell] + off;
      *b = static_cast<uint8_t>(*b ^ x);
    }
  }
};

template <int E>
__global__ __launch_bounds__(kRepairBlock) void gf_repair_kernel(RepairLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  const int d = L.d;
  const int job = blockIdx.x / L.blocks_per_job, blk = blockIdx.x % L.blocks_per_job;
  if (job >= L.njobs) return;
  const RepairJob J = L.jobs[job];
  uint8_t* aux = reinterpret_cast<uint8_t*>(lds + d * 32);
  for (int t = threadIdx.x; t < d * 32; t += kRepairBlock) {
    const int i = t >> 5, h = (t >> 4) & 1, n = t & 15;
    const uint32_t x = static_cast<uint32_t>(n) << (4 * h);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) v |= gf_mul_bits(J.coef[j * d + i], x) << (8 * j);
    lds[t] = v;
  }
  for (int t = threadIdx.x; t < d; t += kRepairBlock) {
    aux[t] = J.inv[t];
    aux[d + t] = J.j0[t];
  }
  __syncthreads();

  Repairer<E> R{L, J, lds, aux, -1, 0u, 0u};
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

__global__ __launch_bounds__(kRepairBlock) void repair_reset_kernel(RepairLaunch L) {
  for (int i = threadIdx.x; i < L.ncells; i += kRepairBlock) {
    L.cell_report[i] = 0;
    L.cell_report[L.ncells + i] = ~0ull;
  }
  for (int i = threadIdx.x; i < L.nstripes; i += kRepairBlock) {
    L.stripe_report[i] = 0;
    L.stripe_report[L.nstripes + i] = ~0ull;
  }
}

size_t up16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

}  // namespace

int repair_upload(const std::vector<RepairJobDesc>& jobs, int d, int e, void** blob_out, const RepairJob** jobs_out) {
  *blob_out = nullptr;
  *jobs_out = nullptr;
  const size_t n = jobs.size();
  if (n == 0) return hipSuccess;
  // per job: cell pointers, member indices, coefficients, inverses, rows j0
  const size_t o_cells = up16(n * sizeof(RepairJob));
  const size_t s_cells = up16(static_cast<size_t>(d + e) * sizeof(uint8_t*));
  const size_t s_member = up16(static_cast<size_t>(d + e) * sizeof(int));
  const size_t s_coef = up16(static_cast<size_t>(e) * d);
  const size_t s_d = up16(static_cast<size_t>(d));
  const size_t per = s_cells + s_member + s_coef + 2 * s_d;
  const size_t bytes = o_cells + n * per;
  void* dev = nullptr;
  if (hipError_t err = hipMalloc(&dev, bytes)) return err;
  std::vector<char> host(bytes, 0);
  char* const dbase = static_cast<char*>(dev);
  const Field& F = field();
  for (size_t k = 0; k < n; ++k) {
    const RepairJobDesc& D = jobs[k];
    const size_t o = o_cells + k * per;
    uint8_t** cells = reinterpret_cast<uint8_t**>(host.data() + o);
    int* member = reinterpret_cast<int*>(host.data() + o + s_cells);
    uint8_t* coef = reinterpret_cast<uint8_t*>(host.data() + o + s_cells + s_member);
    uint8_t* inv = coef + s_coef;
    uint8_t* j0 = inv + s_d;
    bool al = true;
    for (int i = 0; i < d; ++i) cells[i] = D.data[static_cast<size_t>(i)];
    for (int j = 0; j < e; ++j) cells[d + j] = D.parity[static_cast<size_t>(j)];
    for (int i = 0; i < d + e; ++i) {
      al = al && (reinterpret_cast<uintptr_t>(cells[i]) & 15u) == 0;
      member[i] = D.member[static_cast<size_t>(i)];
    }
    std::memcpy(coef, D.coef.data(), static_cast<size_t>(e) * d);
    for (int i = 0; i < d; ++i) {
      inv[i] = 0;
      j0[i] = 0;
      for (int j = 0; j < e; ++j)
        if (coef[j * d + i]) {
          inv[i] = F.inv(coef[j * d + i]);
          j0[i] = static_cast<uint8_t>(j);
          break;
        }
    }
    RepairJob J;
    J.cells = reinterpret_cast<uint8_t* const*>(dbase + o);
    J.member = reinterpret_cast<const int*>(dbase + o + s_cells);
    J.coef = reinterpret_cast<const uint8_t*>(dbase + o + s_cells + s_member);
    J.inv = J.coef + s_coef;
    J.j0 = J.inv + s_d;
    J.row = D.row;
    J.bytes_only = al ? 0 : 1;
    std::memcpy(host.data() + k * sizeof(RepairJob), &J, sizeof(J));
  }
  if (hipError_t err = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice)) {
    (void) hipFree(dev);
    return err;
  }
  *blob_out = dev;
  *jobs_out = reinterpret_cast<const RepairJob*>(dev);
  return hipSuccess;
}

int repair_blocks_per_job(int njobs, size_t nbytes) {
  // eight 256-thread blocks a CU over all the jobs; at least one 16-B vector per thread
  const long target = static_cast<long>(device_cu_count()) * 8;
  long bpj = std::max<long>(1, target / std::max(1, njobs));
  const long vec_blocks = static_cast<long>((nbytes / 16 + kRepairBlock - 1) / kRepairBlock);
  return static_cast<int>(std::min(bpj, std::max<long>(1, vec_blocks)));
}

int launch_repair_reset(const RepairLaunch& L, void* stream) {
  hipLaunchKernelGGL(repair_reset_kernel, dim3(1), dim3(kRepairBlock), 0, static_cast<hipStream_t>(stream), L);
  return hipGetLastError();
}

int launch_repair(const RepairLaunch& L, void* stream) {
  if (L.njobs <= 0 || L.nbytes == 0) return hipSuccess;
  if (L.e < 2 || L.e > kMaxOut || L.d < 1 || L.blocks_per_job < 1) return hipErrorInvalidValue;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(L.njobs) * static_cast<unsigned>(L.blocks_per_job));
  // the tables, then the inverses and rows j0
  const size_t lds = up16(static_cast<size_t>(L.d) * 128 + 2 * static_cast<size_t>(L.d));
  switch (L.e) {
    case 2: hipLaunchKernelGGL(gf_repair_kernel<2>, grid, dim3(kRepairBlock), lds, s, L); break;
    case 3: hipLaunchKernelGGL(gf_repair_kernel<3>, grid, dim3(kRepairBlock), lds, s, L); break;
    default: hipLaunchKernelGGL(gf_repair_kernel<4>, grid, dim3(kRepairBlock), lds, s, L); break;
  }
  return hipGetLastError();
}

}  // namespace redset_hip
