// stripe_map.h -- which cells a stripe reads and writes, and with which
// GF(2^8) coefficients, independent of where the cells live (device set
// layout, pinned staging buffers, files). Shared by the device plans
// (redset_hip.cpp) and the host streaming pipeline (stream_pipeline.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

struct redset_hip_rs {
  int ranks;
  int encoding;
  std::vector<uint8_t> mat;  // (p+e) x p
};

namespace redset_hip {

enum CellKind { kData = 0, kParity = 1 };

// A cell of the set: member `rank`'s logical-file segment `index` (kData) or
// redundancy slot `index` (kParity).
struct CellRef {
  int rank;
  int kind;
  int index;
};

// outputs = coef (nout x nin, row-major) * inputs, byte by byte
struct StripeMap {
  std::vector<CellRef> in;
  std::vector<CellRef> out;
  std::vector<uint8_t> coef;
  bool xor_only = false;  // XOR scheme: every coefficient is 1
  bool accumulate = false;  // XOR into the outputs (redset_hip_plan_combine jobs)
};

// cell of member `rank` in RS stripe `chunk` (src/redset_reedsolomon_common.c:822-853)
CellRef rs_cell(const redset_hip_rs* rs, int rank, int chunk);

// RS encode of stripe c: d data cells -> e parity cells (row p+i at member
// (c - i) mod p's slot i). src/redset_reedsolomon.c:329-376.
int rs_encode_map(const redset_hip_rs* rs, int c, StripeMap& m);

// RS verify of stripe c: the encode map with its outputs in parity-row order
// (out[i] = the stored cell of row p+i, member (c - i) mod p's slot i), so
// that output i reports to the stripe's report row i.
int rs_verify_map(const redset_hip_rs* rs, int c, StripeMap& m);

// RS rebuild of stripe c: the lost members' cells from the surviving cells
// with a nonzero decode coefficient. Reproduces redset_rs_reduce_decode +
// redset_rs_gaussian_solve (common.c:855-899, :570-630) as one linear map.
int rs_rebuild_map(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int c, StripeMap& m);

// decode map of stripe c as (missing x p); column s = member s's cell
int rs_decode_matrix(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int c, std::vector<uint8_t>& D);

// Errors-and-erasures view of stripe c with `missing` lost members (ascending
// ranks, 1 <= missing <= e): M = W * [A | I], e x (d + e), over the stripe's
// cells in rs_verify_map order (column i < d: data input i, column d + j:
// parity row j). Rows 0 .. e-missing-1 (check rows) vanish on the lost
// members' columns; rows e-missing .. e-1 (rebuild rows) are the identity on
// them and, on the survivors, exactly rs_decode_matrix's coefficients.
struct CheckMatrix {
  int d = 0, e = 0, k = 0;
  std::vector<uint8_t> M;      // e x (d + e), row-major
  std::vector<int> lost_cols;  // k: the column of rebuild_ranks[i]
  std::vector<CellRef> cells;  // d + e: the cell of each column
};
int rs_check_matrix(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int c, CheckMatrix& out);
// The locate rule over the check rows (include/redset_hip.h
// redset_hip_rs_locate_reduced): *col_out = the one surviving column whose
// single wrong byte gives the reduced syndrome R (e - k bytes), *value_out
// that byte's error; -1 / 0 when R is zero or none or several columns match.
void locate_reduced(const CheckMatrix& X, const uint8_t* R, int* col_out, uint8_t* value_out);

// XOR stripe c: member c's parity = XOR of the other members' cells
// (src/redset_xor.c:251-266); rebuild of `root` from all others.
int xor_encode_map(int ranks, int c, StripeMap& m);
int xor_rebuild_map(int ranks, int root, int c, StripeMap& m);

// error reporting shared by all C-ABI entry points
int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
const char* last_error();

// Enqueue one stripe's map on `stream` over cells at the given device
// pointers (in[i] for m.in[i], out[j] for m.out[j]), split into passes of
// <= 16 inputs x <= 4 outputs. blocks_total: grid size budget (0 = fill GPU).
// accumulate: XOR into the outputs instead of overwriting them.
int run_stripe(const StripeMap& m, const uint8_t* const* in, uint8_t* const* out, size_t nbytes, void* stream,
               int blocks_total, bool accumulate = false);

// Set verification of one stripe (redset_hip.cpp). `m` is the stripe's ENCODE
// map (in: the data cells, out: the parity cells); in[i] / stored[j] are the
// device pointers of those cells' bytes [base, base + nbytes): the check
// kernels compare the parity of in[] with stored[] and add what differs to
// rows [row0, row0 + m.out.size()) of `report` (codec_kernels.h
// GfCheckLaunch), which the caller has reset. Fused (verify_fused: <= 16
// inputs and <= 4 parity rows; XOR: <= 16 cells) it is one launch that writes
// nothing; wider maps compute <= 4 rows at a time into `scratch`
// (verify_scratch_bytes, at most 32 MiB) in column windows of <= 8 MiB and
// check those. With `count` set nothing is launched: only the algorithmic
// bytes and launches are tallied.
struct VerifyCount {
  unsigned long long bytes_read = 0, bytes_written = 0;
  int launches = 0;
};
bool verify_fused(const StripeMap& m);
size_t verify_scratch_bytes(const StripeMap& m, size_t nbytes);
int run_verify_stripe(const StripeMap& m, const uint8_t* const* in, const uint8_t* const* stored, size_t nbytes,
                      size_t base, unsigned long long* report, int report_rows, int row0, uint8_t* scratch,
                      void* stream, VerifyCount* count = nullptr);
// rows [row0, row0 + nrows) of a device report to "nothing differs" on `stream`; REDSET_* code
int verify_report_reset(unsigned long long* report, int report_rows, int row0, int nrows, void* stream);

}  // namespace redset_hip
