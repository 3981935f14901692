// rebuild_checked_kernels.hip -- errors-and-erasures rebuild of RS stripes in
// device memory (gfx950); descriptors in rebuild_checked.h.
//
// gf_rebuild_checked_kernel<E, K>: one job is one stripe with K lost cells,
// 0 < K < E. The block builds nibble tables for all ns = d + E - K survivors
// in dynamic LDS (as gf_repair_kernel: survivor m's low-nibble table at word
// 32 m, its high-nibble table 16 words on, 128 B per survivor), each entry
// packing the products with survivor m's column of the check matrix M
// (stripe_map.h rs_check_matrix): the E - K check rows in the low bytes, the
// K rebuild rows above them. The packed dword of a byte column
//   [R | v] = sum_m T_m[c_m]
// then holds the reduced syndrome R and the rebuilt bytes v, at two LDS reads
// per survivor byte. A lane takes a 16-B position of every survivor (16-B
// global loads) and gives every lost cell its 16 rebuilt bytes in one 16-B
// store or, in jobs with a cell that is not 16-B aligned and in the tail after
// the last whole vector, single byte columns.
//
// A column with R != 0 is located exactly as redset_hip_rs_locate_reduced
// does on the host: over the survivors m in order, x = R[j0] / M[j0][m] (j0 =
// the first check row with a nonzero coefficient; the host precomputes j0 and
// the inverse) explains the column when x != 0 and the low bytes of T_m[x]
// equal R; exactly one such m is the answer, and the high bytes of T_m[x] are
// what its wrong byte added to v: they are XORed out IN REGISTERS, before the
// store. None or several (always so with one check row) leave v as computed
// and count the column as unlocated.
//
// Footprint: every byte of the first nbytes of a lost cell is stored exactly
// once and never read; nothing beyond them is written. A survivor byte is
// written only with fix_survivors, as a one-byte read-modify-write of the one
// located byte by the lane that owns the column. The reports are the only
// other writes (64-bit atomics from lanes that found something). No block
// waits on another: no ring, no claim counter, no spin, and the kernel has no
// access to the ring-fault and hang-fault words.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "codec_kernels.h"
#include "gf256.h"
#include "rebuild_checked.h"

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

// a[b] ^= packed products of byte b of w, b = 0..3 (T: the survivor's tables)
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

// What one lane found, and where it goes; as gf_repair_kernel's Repairer: a
// lane meets its columns in ascending order, so the first column of a run of
// corrections to one cell (and its first unlocated column) is the smallest of
// that run.
template <int E, int K>
struct Checker {
  static constexpr uint32_t kCheckMask = (1u << (8 * (E - K))) - 1u;
  const CheckedLaunch& L;
  const CheckedJob& J;
  const uint32_t* tab;  // LDS: ns x 32 words
  const uint8_t* aux;   // LDS: ns inverses, then ns rows j0
  int cur;              // survivor of the open run of corrections (-1: none)
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

  // The column at cell offset `off` has the packed dword P with nonzero check
  // bytes; returns P with a located survivor's error taken out.
  __device__ __forceinline__ uint32_t column(size_t off, uint32_t P) {
    const int ns = L.ns;
    const uint32_t R = P & kCheckMask;
    int cell = -1;
    uint32_t x = 0, fix = 0;
    if (E - K >= 2) {  // one check row: every survivor explains the column
      int matches = 0;
      for (int m = 0; m < ns; ++m) {
        const uint32_t xm = gf_mul_bits((R >> (8 * aux[ns + m])) & 255u, aux[m]);
        const uint32_t prod = tab[m * 32 + (xm & 15u)] ^ tab[m * 32 + 16 + (xm >> 4)];
        if (xm != 0 && (prod & kCheckMask) == R) {
          cell = m;
          x = xm;
          fix = prod;
          ++matches;
        }
      }
      if (matches != 1) cell = -1;
    }
    const unsigned long long where = L.base + off;
    if (cell < 0) {
      if (ucnt == 0) atomicMin(L.stripe_report + L.nstripes + J.row, where);
      ++ucnt;
      return P;
    }
    if (cell != cur) {
      flush_run();
      cur = cell;
      atomicMin(L.cell_report + L.ncells + static_cast<size_t>(J.row) * L.p + J.member[cell], where);
    }
    ++cnt;
    if (L.fix_survivors) {
      uint8_t* b = J.in[cell] + off;
      *b = static_cast<uint8_t>(*b ^ x);
    }
    return P ^ fix;
  }
};

template <int E, int K>
__global__ __launch_bounds__(kCheckedBlock) void gf_rebuild_checked_kernel(CheckedLaunch L) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr uint32_t kCheckMask = Checker<E, K>::kCheckMask;
  const int ns = L.ns;
  const int job = blockIdx.x / L.blocks_per_job, blk = blockIdx.x % L.blocks_per_job;
  if (job >= L.njobs) return;
  const CheckedJob J = L.jobs[job];
  uint8_t* aux = reinterpret_cast<uint8_t*>(lds + ns * 32);
  for (int t = threadIdx.x; t < ns * 32; t += kCheckedBlock) {
    const int i = t >> 5, h = (t >> 4) & 1, n = t & 15;
    const uint32_t x = static_cast<uint32_t>(n) << (4 * h);
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < E; ++j) v |= gf_mul_bits(J.coef[j * ns + i], x) << (8 * j);
    lds[t] = v;
  }
  for (int t = threadIdx.x; t < ns; t += kCheckedBlock) {
    aux[t] = J.inv[t];
    aux[ns + t] = J.j0[t];
  }
  __syncthreads();

  Checker<E, K> C{L, J, lds, aux, -1, 0u, 0u};
  const size_t step = static_cast<size_t>(L.blocks_per_job) * kCheckedBlock;
  const size_t lane0 = static_cast<size_t>(blk) * kCheckedBlock + threadIdx.x;
  const size_t nvec = J.bytes_only ? 0 : L.nbytes / 16;

  for (size_t v = lane0; v < nvec; v += step) {
    uint32_t acc[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) acc[b] = 0;
    int m = 0;
    for (; m + 4 <= ns; m += 4) {
      const uint4 x0 = reinterpret_cast<const uint4*>(J.in[m])[v];
      const uint4 x1 = reinterpret_cast<const uint4*>(J.in[m + 1])[v];
      const uint4 x2 = reinterpret_cast<const uint4*>(J.in[m + 2])[v];
      const uint4 x3 = reinterpret_cast<const uint4*>(J.in[m + 3])[v];
      acc_vec(lds + m * 32, x0, acc);
      acc_vec(lds + (m + 1) * 32, x1, acc);
      acc_vec(lds + (m + 2) * 32, x2, acc);
      acc_vec(lds + (m + 3) * 32, x3, acc);
    }
    for (; m < ns; ++m) acc_vec(lds + m * 32, reinterpret_cast<const uint4*>(J.in[m])[v], acc);
    uint32_t any = 0;
#pragma unroll
    for (int b = 0; b < 16; ++b) any |= acc[b];
    if ((any & kCheckMask) != 0) {
      // rare: the columns one at a time, acc[] kept in registers by selects
#pragma unroll 1
      for (int col = 0; col < 16; ++col) {
        uint32_t P = 0;
#pragma unroll
        for (int b = 0; b < 16; ++b) P = b == col ? acc[b] : P;
        if ((P & kCheckMask) == 0) continue;
        P = C.column(v * 16 + col, P);
#pragma unroll
        for (int b = 0; b < 16; ++b) acc[b] = b == col ? P : acc[b];
      }
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
      uint4 o;
      o.x = gather_row(acc[0], acc[1], acc[2], acc[3], E - K + i);
      o.y = gather_row(acc[4], acc[5], acc[6], acc[7], E - K + i);
      o.z = gather_row(acc[8], acc[9], acc[10], acc[11], E - K + i);
      o.w = gather_row(acc[12], acc[13], acc[14], acc[15], E - K + i);
      reinterpret_cast<uint4*>(J.out[i])[v] = o;
    }
  }

  // byte columns: the whole job when a cell is unaligned, else the tail after
  // the last whole vector (block 0 of the job)
  const size_t b0 = nvec * 16;
  if (J.bytes_only || blk == 0) {
    for (size_t o = b0 + (J.bytes_only ? lane0 : threadIdx.x); o < L.nbytes; o += J.bytes_only ? step : kCheckedBlock) {
      uint32_t P = 0;
      for (int m = 0; m < ns; ++m) {
        const uint32_t b = J.in[m][o];
        P ^= lds[m * 32 + (b & 15u)] ^ lds[m * 32 + 16 + (b >> 4)];
      }
      if ((P & kCheckMask) != 0) P = C.column(o, P);
#pragma unroll
      for (int i = 0; i < K; ++i) J.out[i][o] = static_cast<uint8_t>(P >> (8 * (E - K + i)));
    }
  }
  C.finish();
}

__global__ __launch_bounds__(kCheckedBlock) void checked_reset_kernel(CheckedLaunch L) {
  for (int i = threadIdx.x; i < L.ncells; i += kCheckedBlock) {
    L.cell_report[i] = 0;
    L.cell_report[L.ncells + i] = ~0ull;
  }
  for (int i = threadIdx.x; i < L.nstripes; i += kCheckedBlock) {
    L.stripe_report[i] = 0;
    L.stripe_report[L.nstripes + i] = ~0ull;
  }
}

size_t up16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

template <int E, int K>
void launch_ek(const CheckedLaunch& L, dim3 grid, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((gf_rebuild_checked_kernel<E, K>), grid, dim3(kCheckedBlock), lds, s, L);
}

}  // namespace

int checked_upload(const std::vector<CheckedJobDesc>& jobs, int ns, int e, int k, void** blob_out,
                   const CheckedJob** jobs_out) {
  *blob_out = nullptr;
  *jobs_out = nullptr;
  const size_t n = jobs.size();
  if (n == 0) return hipSuccess;
  // per job: survivor pointers, output pointers, member indices, coefficients, inverses, rows j0
  const size_t o_first = up16(n * sizeof(CheckedJob));
  const size_t s_in = up16(static_cast<size_t>(ns) * sizeof(uint8_t*));
  const size_t s_out = up16(static_cast<size_t>(k) * sizeof(uint8_t*));
  const size_t s_member = up16(static_cast<size_t>(ns) * sizeof(int));
  const size_t s_coef = up16(static_cast<size_t>(e) * ns);
  const size_t s_ns = up16(static_cast<size_t>(ns));
  const size_t per = s_in + s_out + s_member + s_coef + 2 * s_ns;
  const size_t bytes = o_first + n * per;
  void* dev = nullptr;
  if (hipError_t err = hipMalloc(&dev, bytes)) return err;
  std::vector<char> host(bytes, 0);
  char* const dbase = static_cast<char*>(dev);
  const Field& F = field();
  const int nck = e - k;
  for (size_t q = 0; q < n; ++q) {
    const CheckedJobDesc& D = jobs[q];
    const size_t o = o_first + q * per;
    uint8_t** in = reinterpret_cast<uint8_t**>(host.data() + o);
    uint8_t** out = reinterpret_cast<uint8_t**>(host.data() + o + s_in);
    int* member = reinterpret_cast<int*>(host.data() + o + s_in + s_out);
    uint8_t* coef = reinterpret_cast<uint8_t*>(host.data() + o + s_in + s_out + s_member);
    uint8_t* inv = coef + s_coef;
    uint8_t* j0 = inv + s_ns;
    bool al = true;
    for (int i = 0; i < ns; ++i) {
      in[i] = D.in[static_cast<size_t>(i)];
      member[i] = D.member[static_cast<size_t>(i)];
      al = al && (reinterpret_cast<uintptr_t>(in[i]) & 15u) == 0;
    }
    for (int i = 0; i < k; ++i) {
      out[i] = D.out[static_cast<size_t>(i)];
      al = al && (reinterpret_cast<uintptr_t>(out[i]) & 15u) == 0;
    }
    std::memcpy(coef, D.coef.data(), static_cast<size_t>(e) * ns);
    for (int i = 0; i < ns; ++i) {
      inv[i] = 0;
      j0[i] = 0;
      for (int j = 0; j < nck; ++j)
        if (coef[j * ns + i]) {
          inv[i] = F.inv(coef[j * ns + i]);
          j0[i] = static_cast<uint8_t>(j);
          break;
        }
    }
    CheckedJob J;
    J.in = reinterpret_cast<uint8_t* const*>(dbase + o);
    J.out = reinterpret_cast<uint8_t* const*>(dbase + o + s_in);
    J.member = reinterpret_cast<const int*>(dbase + o + s_in + s_out);
    J.coef = reinterpret_cast<const uint8_t*>(dbase + o + s_in + s_out + s_member);
    J.inv = J.coef + s_coef;
    J.j0 = J.inv + s_ns;
    J.row = D.row;
    J.bytes_only = al ? 0 : 1;
    std::memcpy(host.data() + q * sizeof(CheckedJob), &J, sizeof(J));
  }
  if (hipError_t err = hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice)) {
    (void) hipFree(dev);
    return err;
  }
  *blob_out = dev;
  *jobs_out = reinterpret_cast<const CheckedJob*>(dev);
  return hipSuccess;
}

int checked_blocks_per_job(int njobs, size_t nbytes) {
  // eight 256-thread blocks a CU over all the jobs; at least one 16-B vector per thread
  const long target = static_cast<long>(device_cu_count()) * 8;
  long bpj = std::max<long>(1, target / std::max(1, njobs));
  const long vec_blocks = static_cast<long>((nbytes / 16 + kCheckedBlock - 1) / kCheckedBlock);
  return static_cast<int>(std::min(bpj, std::max<long>(1, vec_blocks)));
}

int launch_checked_reset(const CheckedLaunch& L, void* stream) {
  hipLaunchKernelGGL(checked_reset_kernel, dim3(1), dim3(kCheckedBlock), 0, static_cast<hipStream_t>(stream), L);
  return hipGetLastError();
}

int launch_checked(const CheckedLaunch& L, void* stream) {
  if (L.njobs <= 0 || L.nbytes == 0) return hipSuccess;
  if (L.e < 2 || L.e > kMaxOut || L.k < 1 || L.k >= L.e || L.ns < 1 || L.blocks_per_job < 1)
    return hipErrorInvalidValue;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(static_cast<unsigned>(L.njobs) * static_cast<unsigned>(L.blocks_per_job));
  // the tables, then the inverses and rows j0
  const size_t lds = up16(static_cast<size_t>(L.ns) * 128 + 2 * static_cast<size_t>(L.ns));
  switch (L.e * 4 + L.k) {
    case 2 * 4 + 1: launch_ek<2, 1>(L, grid, lds, s); break;
    case 3 * 4 + 1: launch_ek<3, 1>(L, grid, lds, s); break;
    case 3 * 4 + 2: launch_ek<3, 2>(L, grid, lds, s); break;
    case 4 * 4 + 1: launch_ek<4, 1>(L, grid, lds, s); break;
    case 4 * 4 + 2: launch_ek<4, 2>(L, grid, lds, s); break;
    default: launch_ek<4, 3>(L, grid, lds, s); break;
  }
  return hipGetLastError();
}

}  // namespace redset_hip
