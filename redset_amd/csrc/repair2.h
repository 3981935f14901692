// repair2.h -- repair with two wrong bytes per column (RS sets with e = 4):
// the power-basis arithmetic on the host (stripe_map.cpp) and the launch
// descriptors shared by the kernel (repair2_kernels.hip), the plan
// (redset_hip.cpp) and the host-resident form (repair_stream.cpp).
//
// A job is what repair.h's is -- one stripe, or a column window of one: d data
// cells, 4 stored parity cells, the 4 x d parity coefficients, the member of
// every cell -- plus the stripe's power basis (include/redset_hip.h,
// "repair2"): the point alpha and 1/u of every cell and the 4 x 4 transform
// W^-1 that turns the stored syndrome into power sums.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "repair.h"
#include "stripe_map.h"

namespace redset_hip {

constexpr int kRepair2E = 4;

// Power basis of stripe c over its d + e cells in rs_verify_map order (data
// inputs, then parity rows): alpha, u (d + e each) and winv (e x e, row-major)
// with winv * H[:, i] = u[i] * (1, alpha[i], alpha[i]^2, alpha[i]^3), H =
// [A | I]. Checked column by column before it returns; REDSET_* code.
int rs_power_basis(const redset_hip_rs* rs, int c, std::vector<uint8_t>& alpha, std::vector<uint8_t>& u,
                   std::vector<uint8_t>& winv);

// The pair rule of redset_hip_rs_locate_syndrome2 on the stored syndrome S (4
// bytes) of a column no single cell explains: *count_out = 2 with the two
// columns (rs_verify_map order) and their error values, or 0. REDSET_* code.
int locate_pair(const redset_hip_rs* rs, int c, const uint8_t* S, int* cols_out, uint8_t* values_out, int* count_out);

// Device view of a job. All arrays are device memory (one blob per job list,
// repair2_upload).
struct Repair2Job {
  uint8_t* const* cells;  // d data-cell pointers, then 4 parity-cell pointers (row order)
  const uint8_t* coef;    // 4 x d, row-major: A[j][m] of data input m
  const uint8_t* alpha;   // d + 4: the cell's evaluation point
  const uint8_t* invu;    // d + 4: 1 / u of the cell
  const int* member;      // d + 4: the set member holding each cell
  uint8_t winv[16];       // W^-1, row-major
  int row;                // the job's stripe row in the reports
  int bytes_only;         // 1: a cell is not 16-B aligned, every column takes the byte path
};

// One launch over `njobs` jobs of `nbytes` columns each. cell_report and
// stripe_report are repair.h's; pair_report[job.row] counts the columns
// corrected as a pair. gf: 512 bytes of exp (2^i, doubled), then 256 of log.
struct Repair2Launch {
  const Repair2Job* jobs;
  const uint8_t* gf;
  int njobs;
  int d, p;
  int blocks_per_job;
  int apply;  // 0: dry run, no cell byte is written
  size_t nbytes;
  unsigned long long base;
  unsigned long long* cell_report;
  int ncells;
  unsigned long long* stripe_report;
  unsigned long long* pair_report;
  int nstripes;
};

// Host description of a job, for repair2_upload.
struct Repair2JobDesc {
  RepairJobDesc cells;               // pointers, coefficients, members, row
  std::vector<uint8_t> alpha, invu;  // d + 4
  uint8_t winv[16];
};

// The job of stripe c with its cells at the given device pointers (data[i] for
// rs_verify_map's in[i], parity[j] for out[j]); REDSET_* code.
int repair2_job(const redset_hip_rs* rs, int c, const std::vector<uint8_t*>& data, const std::vector<uint8_t*>& parity,
                int row, Repair2JobDesc& out);
// Places the jobs and the field tables in one device allocation (*blob_out, to
// hipFree) and fills L.jobs and L.gf. Synchronous; not for the execute path.
// Returns hipError_t as int.
int repair2_upload(const std::vector<Repair2JobDesc>& jobs, int d, void** blob_out, Repair2Launch& L);
// dynamic LDS of one block, bytes
size_t repair2_lds_bytes(int d);
// the three reports back to "nothing found", by a one-block kernel on `stream`
int launch_repair2_reset(const Repair2Launch& L, void* stream);
// the repair2 kernel on `stream`; returns hipError_t as int
int launch_repair2(const Repair2Launch& L, void* stream);

}  // namespace redset_hip
