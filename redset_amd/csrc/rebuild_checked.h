// rebuild_checked.h -- errors-and-erasures rebuild of RS stripes in device
// memory: the launch descriptors shared by the kernel
// (rebuild_checked_kernels.hip), the plan (redset_hip.cpp) and the
// host-resident form (rebuild_checked_stream.cpp).
//
// A job is one stripe (or a column window of one) with k lost cells, 0 < k <
// e <= kMaxOut: its d + e - k surviving cells, its k lost cells, and the
// survivors' columns of the check matrix M (stripe_map.h rs_check_matrix):
// e - k check rows, then k rebuild rows. For every byte column the kernel
// forms [R | v] = sum_m M_m * c_m, applies the rule of
// redset_hip_rs_locate_reduced (include/redset_hip.h) to R and stores v,
// corrected when one survivor explains R.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace redset_hip {

constexpr int kCheckedBlock = 256;

// Device view of a job. All arrays are device memory (one blob per job list,
// checked_upload).
struct CheckedJob {
  uint8_t* const* in;   // ns = d + e - k surviving cells (written only by fix_survivors)
  uint8_t* const* out;  // k lost cells, in rebuild_ranks order
  const uint8_t* coef;  // e x ns, row-major: M[j][m] of survivor m (check rows first)
  const uint8_t* inv;   // ns: 1 / M[j0][m], j0 = first check row with M[j][m] != 0; 0 if none
  const uint8_t* j0;    // ns: that row (0 if none)
  const int* member;    // ns: the set member holding each survivor
  int row;              // the job's stripe row in the reports
  int bytes_only;       // 1: a cell is not 16-B aligned, every column takes the byte path
};

// One launch over `njobs` jobs of `nbytes` columns each. Reports as repair.h
// RepairLaunch: cell_report = ncells corrected-byte counts then ncells
// smallest corrected cell offsets, indexed [job.row * p + member];
// stripe_report = nstripes unlocated-column counts then nstripes smallest
// unlocated offsets, indexed [job.row]. Offsets are `base` + the column's
// offset in the launch's cells; ~0 means none.
struct CheckedLaunch {
  const CheckedJob* jobs;
  int njobs;
  int ns, e, k, p;
  int blocks_per_job;
  int fix_survivors;  // 1: XOR a located survivor byte right; 0: no survivor byte is written
  size_t nbytes;
  unsigned long long base;
  unsigned long long* cell_report;
  int ncells;
  unsigned long long* stripe_report;
  int nstripes;
};

// Host description of a job, for checked_upload.
struct CheckedJobDesc {
  std::vector<uint8_t*> in, out;  // device pointers
  std::vector<uint8_t> coef;      // e x ns
  std::vector<int> member;        // ns
  int row = 0;
};

// Places the jobs in one device allocation (*blob_out, to hipFree) and
// returns the device job array. Synchronous; not for the execute path.
// Returns hipError_t as int.
int checked_upload(const std::vector<CheckedJobDesc>& jobs, int ns, int e, int k, void** blob_out,
                   const CheckedJob** jobs_out);
// blocks per job for `njobs` jobs side by side over nbytes columns
int checked_blocks_per_job(int njobs, size_t nbytes);
// both reports back to "nothing found", by a one-block kernel on `stream`
int launch_checked_reset(const CheckedLaunch& L, void* stream);
// the decode kernel on `stream`; returns hipError_t as int
int launch_checked(const CheckedLaunch& L, void* stream);

}  // namespace redset_hip
