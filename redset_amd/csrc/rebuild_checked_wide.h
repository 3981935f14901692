// rebuild_checked_wide.h -- errors-and-erasures rebuild of RS stripes with 5
// to 8 parity rows, up to floor((e - k) / 2) wrong survivor bytes per byte
// column: the host arithmetic (stripe_map.cpp) and the launch descriptors
// shared by the kernel (rebuild_checked_wide_kernels.hip), the plan
// (redset_hip.cpp) and the host-resident form (rebuild_checked_stream.cpp).
//
// A job is one stripe (or a column window of one) with k lost cells, 0 < k <
// e, s = e - k spare rows: its ns = d + e - k surviving cells, its k lost
// cells, the survivors' columns of [C ; B] (include/redset_hip.h, "checked
// rebuild, wide": s check rows in the power basis with the erasure locator
// folded in, then the k rebuild rows of redset_hip_rs_decode_matrix), and
// every survivor's point alpha and 1 / u'.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "rebuild_checked.h"
#include "repair_wide.h"
#include "stripe_map.h"

namespace redset_hip {

constexpr int kCwMaxS = kWideMaxE - 1;  // spare rows: 1..7
constexpr int kCwMaxT = kCwMaxS / 2;    // wrong survivor bytes located per column: up to 3

// What redset_hip_rs_check_basis_wide returns for one stripe. X.M is [C ; B],
// e x (d + e) row-major over X.cells (rs_verify_map order); alpha and uprime
// have d + e entries, uprime = u * Gamma(alpha), zero on the lost columns.
struct CheckBasisWide {
  CheckMatrix X;
  std::vector<uint8_t> alpha, uprime;
};

// Builds and checks the basis of stripe c: C's closed form on all d + e
// columns, B's identity on the lost ones (every full rebuild row lies in the
// row space of H). REDSET_* code.
int rs_check_basis_wide(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int c, CheckBasisWide& out);

// The rule of redset_hip_rs_locate_reduced_wide on the s bytes T: *count_out =
// nu with the columns (X.cells order, ascending) and their error values, or 0.
// max_errors: 1 .. s / 2, and 0 where s == 1. REDSET_* code.
int locate_reduced_wide(const CheckBasisWide& Bs, const uint8_t* T, int max_errors, int* cols_out, uint8_t* values_out,
                        int* count_out);

// Device view of a job. All arrays are device memory (one blob per job list,
// checked_wide_upload).
struct CheckedWideJob {
  uint8_t* const* in;    // ns surviving cells (written only by fix_survivors)
  uint8_t* const* out;   // k lost cells, in rebuild_ranks order
  const uint8_t* coef;   // e x ns, row-major: s check rows, then k rebuild rows
  const uint8_t* alpha;  // ns: the survivor's evaluation point
  const uint8_t* invu;   // ns: 1 / u' of the survivor
  const int* member;     // ns: the set member holding each survivor
  int row;               // the job's stripe row in the reports
  int bytes_only;        // 1: a cell is not 16-B aligned, every column takes the byte path
};

// One launch over `njobs` jobs of `nbytes` columns each. cell_report and
// stripe_report are rebuild_checked.h's; multi_report[job.row * 2 + nu - 2]
// counts the columns corrected with nu = 2, 3 wrong survivor bytes. gf: 512
// bytes of exp (2^i, doubled), then 256 of log.
struct CheckedWideLaunch {
  const CheckedWideJob* jobs;
  const uint8_t* gf;
  int njobs;
  int ns, e, k, p;
  int blocks_per_job;
  int fix_survivors;  // 1: XOR the located survivor bytes right; 0: no survivor byte is written
  int max_errors;     // 0 .. (e - k) / 2
  size_t nbytes;
  unsigned long long base;
  unsigned long long* cell_report;
  int ncells;
  unsigned long long* stripe_report;
  unsigned long long* multi_report;
  int nstripes;
};

// Host description of a job, for checked_wide_upload.
struct CheckedWideJobDesc {
  CheckedJobDesc cells;              // pointers, [C ; B] over the survivors, members, row
  std::vector<uint8_t> alpha, invu;  // ns
};

// The job of a stripe with its surviving columns at `in` (ascending column
// order) and its lost columns at `out` (rebuild_ranks order).
void checked_wide_job(const CheckBasisWide& Bs, const std::vector<uint8_t*>& in, const std::vector<uint8_t*>& out,
                      int row, CheckedWideJobDesc& J);
// Places the jobs and the field tables in one device allocation (*blob_out, to
// hipFree) and fills L.jobs and L.gf. Synchronous; not for the execute path.
// Returns hipError_t as int.
int checked_wide_upload(const std::vector<CheckedWideJobDesc>& jobs, int ns, int e, int k, void** blob_out,
                        CheckedWideLaunch& L);
// dynamic LDS of one block, bytes
size_t checked_wide_lds_bytes(int ns);
// Raises gf_rebuild_checked_wide_kernel<s>'s dynamic-LDS limit to what ns
// survivors take; once per plan build, never on the execute path. Returns
// hipError_t as int (hipErrorInvalidValue for a shape past kWideLdsLimit: the
// caller names it).
int checked_wide_prepare(int ns, int s);
// the three reports back to "nothing found", by a one-block kernel on `stream`
int launch_checked_wide_reset(const CheckedWideLaunch& L, void* stream);
// the decode kernel on `stream`; returns hipError_t as int
int launch_checked_wide(const CheckedWideLaunch& L, void* stream);

}  // namespace redset_hip
