// repair.h -- column-wise locate and repair of damaged RS stripes in device
// memory: the launch descriptors shared by the kernel (repair_kernels.hip),
// the plan (redset_hip.cpp) and the host-resident form (repair_stream.cpp).
//
// A job is one stripe (or a column window of one): its d data cells, its e
// stored parity cells (2 <= e <= kMaxOut), the e x d parity coefficients the
// encode uses and, per cell, the member that holds it. For every byte column
// the kernel forms the syndrome, applies the rule of
// redset_hip_rs_locate_syndrome (include/redset_hip.h) and, when asked to,
// XORs the one wrong byte right.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace redset_hip {

constexpr int kRepairBlock = 256;

// Device view of a job. All arrays are device memory (one blob per job list,
// repair_upload).
struct RepairJob {
  uint8_t* const* cells;  // d data-cell pointers, then e parity-cell pointers (row order)
  const uint8_t* coef;    // e x d, row-major: A[j][m] of data input m
  const uint8_t* inv;     // d: 1 / A[j0][m], j0 = first row with A[j][m] != 0; 0 if no such row
  const uint8_t* j0;      // d: that row (0 if none)
  const int* member;      // d + e: the set member holding each cell
  int row;                // the job's stripe row in the reports
  int bytes_only;         // 1: a cell is not 16-B aligned, every column takes the byte path
};

// One launch over `njobs` jobs of `nbytes` columns each. Reports: cell_report
// = ncells corrected-byte counts then ncells smallest corrected cell offsets,
// indexed [job.row * p + member]; stripe_report = nstripes unlocated-column
// counts then nstripes smallest unlocated offsets, indexed [job.row]. Offsets
// are `base` + the column's offset in the launch's cells; ~0 means none.
struct RepairLaunch {
  const RepairJob* jobs;
  int njobs;
  int d, e, p;
  int blocks_per_job;
  int apply;  // 0: dry run, no cell byte is written
  size_t nbytes;
  unsigned long long base;
  unsigned long long* cell_report;
  int ncells;
  unsigned long long* stripe_report;
  int nstripes;
};

// Host description of a job, for repair_upload.
struct RepairJobDesc {
  std::vector<uint8_t*> data, parity;  // device pointers
  std::vector<uint8_t> coef;           // e x d
  std::vector<int> member;             // d + e
  int row = 0;
};

// Places the jobs in one device allocation (*blob_out, to hipFree) and
// returns the device job array. Synchronous; not for the execute path.
// Returns hipError_t as int.
int repair_upload(const std::vector<RepairJobDesc>& jobs, int d, int e, void** blob_out, const RepairJob** jobs_out);
// blocks per job for `njobs` jobs side by side over nbytes columns
int repair_blocks_per_job(int njobs, size_t nbytes);
// both reports back to "nothing found", by a one-block kernel on `stream`
int launch_repair_reset(const RepairLaunch& L, void* stream);
// the repair kernel on `stream`; returns hipError_t as int
int launch_repair(const RepairLaunch& L, void* stream);

}  // namespace redset_hip
