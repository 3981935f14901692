// repair_wide.h -- repair of RS sets with 5 to 8 parity rows, up to
// t = floor(e / 2) wrong bytes per byte column: the power-basis arithmetic on
// the host (stripe_map.cpp) and the launch descriptors shared by the kernel
// (repair_wide_kernels.hip), the plan (redset_hip.cpp) and the host-resident
// form (repair_stream.cpp).
//
// A job is what repair2.h's is with e parity cells: d data cells, e stored
// parity cells, the e x d parity coefficients, the member of every cell, the
// point alpha and 1/u of every cell and the e x e transform W^-1 that turns
// the stored syndrome into the power sums S'_k = sum y_i X_i^k, k = 0..e-1
// (include/redset_hip.h, "repair_wide").
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "repair.h"
#include "stripe_map.h"

namespace redset_hip {

constexpr int kWideMinE = 5, kWideMaxE = 8;
constexpr int kWideMaxT = kWideMaxE / 2;
// LDS of one gfx950 CU: what a block's dynamic LDS is checked against
constexpr size_t kWideLdsLimit = 160u << 10;

// rs_power_basis for 5 <= e <= 8: alpha, u (d + e each, rs_verify_map order)
// and winv (e x e, row-major) with winv * H[:, i] = u[i] * alpha[i]^k,
// k = 0..e-1, H = [A | I]. Checked column by column before it returns.
int rs_power_basis_wide(const redset_hip_rs* rs, int c, std::vector<uint8_t>& alpha, std::vector<uint8_t>& u,
                        std::vector<uint8_t>& winv);

// The rule of redset_hip_rs_locate_syndrome_wide on the stored syndrome S (e
// bytes): *count_out = nu with the columns (rs_verify_map order, ascending)
// and their error values, or 0. REDSET_* code.
int locate_wide(const redset_hip_rs* rs, int c, const uint8_t* S, int max_errors, int* cols_out, uint8_t* values_out,
                int* count_out);

// Device view of a job. All arrays are device memory (one blob per job list,
// repair_wide_upload).
struct RepairWideJob {
  uint8_t* const* cells;  // d data-cell pointers, then e parity-cell pointers (row order)
  const uint8_t* coef;    // e x d, row-major: A[j][m] of data input m
  const uint8_t* alpha;   // d + e: the cell's evaluation point
  const uint8_t* invu;    // d + e: 1 / u of the cell
  const int* member;      // d + e: the set member holding each cell
  uint8_t winv[kWideMaxE * kWideMaxE];  // W^-1, e x e row-major
  int row;                // the job's stripe row in the reports
  int bytes_only;         // 1: a cell is not 16-B aligned, every column takes the byte path
};

// One launch over `njobs` jobs of `nbytes` columns each. cell_report and
// stripe_report are repair.h's; multi_report[job.row * 3 + nu - 2] counts the
// columns corrected with nu = 2..4 wrong bytes. gf: 512 bytes of exp (2^i,
// doubled), then 256 of log.
struct RepairWideLaunch {
  const RepairWideJob* jobs;
  const uint8_t* gf;
  int njobs;
  int d, e, p;
  int blocks_per_job;
  int apply;       // 0: dry run, no cell byte is written
  int max_errors;  // 1 .. e / 2
  size_t nbytes;
  unsigned long long base;
  unsigned long long* cell_report;
  int ncells;
  unsigned long long* stripe_report;
  unsigned long long* multi_report;
  int nstripes;
};

// Host description of a job, for repair_wide_upload.
struct RepairWideJobDesc {
  RepairJobDesc cells;               // pointers, coefficients, members, row
  std::vector<uint8_t> alpha, invu;  // d + e
  std::vector<uint8_t> winv;         // e x e
};

// The job of stripe c with its cells at the given device pointers (data[i] for
// rs_verify_map's in[i], parity[j] for out[j]); REDSET_* code.
int repair_wide_job(const redset_hip_rs* rs, int c, const std::vector<uint8_t*>& data,
                    const std::vector<uint8_t*>& parity, int row, RepairWideJobDesc& out);
// Places the jobs and the field tables in one device allocation (*blob_out, to
// hipFree) and fills L.jobs and L.gf. Synchronous; not for the execute path.
// Returns hipError_t as int.
int repair_wide_upload(const std::vector<RepairWideJobDesc>& jobs, int d, int e, void** blob_out, RepairWideLaunch& L);
// dynamic LDS of one block, bytes
size_t repair_wide_lds_bytes(int d, int e);
// Raises gf_repair_wide_kernel<e>'s dynamic-LDS limit to what (d, e) takes;
// once per plan build, never on the execute path. Returns hipError_t as int
// (hipErrorInvalidValue for a shape past kWideLdsLimit: the caller names it).
int repair_wide_prepare(int d, int e);
// the three reports back to "nothing found", by a one-block kernel on `stream`
int launch_repair_wide_reset(const RepairWideLaunch& L, void* stream);
// the kernel on `stream`; returns hipError_t as int
int launch_repair_wide(const RepairWideLaunch& L, void* stream);

}  // namespace redset_hip
