/*
 * redset_hip.h -- C ABI of the MI355X (gfx950) Reed-Solomon / XOR codec that
 * replaces redset's encode/decode backends.
 *
 * Everything here is plain C: integers, sizes and pointers. Buffers named
 * "device" are HIP device pointers; `stream` is a hipStream_t passed as
 * void* (NULL = the default stream). Return codes follow redset:
 * REDSET_SUCCESS (0, src/redset.h:24) or REDSET_FAILURE (1,
 * src/redset_util.h:19); HIP errors map to REDSET_FAILURE and
 * redset_hip_last_error() says why.
 *
 * Where the reference dispatches to a backend (src/redset_reedsolomon.c:
 * 522-545, :986-1006; src/redset_xor.c:399-420, :650-671), a maintainer adds
 * a REDSET_ENCODE_HIP case that calls these functions; INTEGRATION.md shows
 * that glue.
 *
 * Data layout in HBM ("set layout"): member r of a redundancy set of p
 * members owns a logical-file region lofi[r] holding its data cells
 * (p-e for RS, p-1 for XOR) and a redundancy region parity[r] holding its
 * e parity cells (1 for XOR). Cell s of either region starts at
 * base + s * cell_stride, cell_stride >= chunk_size. This mirrors the
 * reference's logical file (segment s at s*chunk_size, src/redset_
 * reedsolomon.c:334-335) and redundancy file (slot i at header + i*chunk_size,
 * :380-381) with an optional pad so every cell can start 16-B aligned.
 * Cells at a 16-B aligned address take the vector path; others work, slowly.
 */
#ifndef REDSET_HIP_H
#define REDSET_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef REDSET_SUCCESS
#define REDSET_SUCCESS (0)
#endif
#ifndef REDSET_FAILURE
#define REDSET_FAILURE (1)
#endif

typedef struct redset_hip_rs redset_hip_rs;      /* GF tables + encoding matrix */
typedef struct redset_hip_plan redset_hip_plan;  /* prepared kernel launches */

enum {
  REDSET_HIP_PLAN_RS_ENCODE = 1,
  REDSET_HIP_PLAN_RS_REBUILD = 2,
  REDSET_HIP_PLAN_XOR_ENCODE = 3,
  REDSET_HIP_PLAN_XOR_REBUILD = 4,
  REDSET_HIP_PLAN_RS_VERIFY = 5,
  REDSET_HIP_PLAN_XOR_VERIFY = 6,
  REDSET_HIP_PLAN_CRC32 = 7,
  REDSET_HIP_PLAN_RS_REPAIR = 8,
  REDSET_HIP_PLAN_RS_REBUILD_CHECKED = 9
};

typedef struct {
  int kind;                          /* REDSET_HIP_PLAN_* */
  int ranks;                         /* p */
  int encoding;                      /* e (1 for XOR) */
  int missing;                       /* erased members (rebuild plans) */
  int launches;                      /* kernel launches per execute */
  int jobs;                          /* stripe jobs over all launches */
  size_t chunk_size;                 /* bytes per cell */
  unsigned long long bytes_read;     /* algorithmic bytes read per execute */
  unsigned long long bytes_written;  /* algorithmic bytes written per execute */
} redset_hip_plan_info;

/* ---- field, matrix, layout ------------------------------------------- */

/* Build GF(2^8) tables and the (p+e) x p encoding matrix.
 * Replaces redset_rs_gf_alloc (src/redset_reedsolomon_common.c:727-757) as
 * called from redset_construct_rs (src/redset_reedsolomon.c:169-185); same
 * validity rule: 1 <= encoding < ranks, ranks + encoding <= 256. */
int redset_hip_rs_create(int ranks, int encoding, redset_hip_rs** out);
/* Replaces redset_rs_gf_delete (src/redset_reedsolomon_common.c:759-769). */
void redset_hip_rs_destroy(redset_hip_rs* rs);
/* Copies the (p+e) x p matrix (state->mat, src/redset_internal.h:88) as bytes. */
int redset_hip_rs_matrix(const redset_hip_rs* rs, unsigned char* mat_out);
/* ranks (p) and encoding (e) of a codec (d->ranks, state->encoding). */
int redset_hip_rs_shape(const redset_hip_rs* rs, int* ranks, int* encoding);
/* Same results as redset_rs_get_encoding_id / redset_rs_get_data_id
 * (src/redset_reedsolomon_common.c:822-853). */
int redset_hip_rs_get_encoding_id(int ranks, int encoding, int rank, int chunk_id);
int redset_hip_rs_get_data_id(int ranks, int encoding, int rank, int chunk_id);

/* ---- whole-set plans (all members' cells resident on one device) ----- */

/* Recommended cell_stride for a set held in one device allocation: chunk_size
 * rounded up to 256 B, plus 16 MiB when that is a multiple of 16 MiB. Cells
 * of a power-of-two size such as 64 MiB otherwise start at addresses equal
 * modulo 2^24..2^26, and a stripe's 11 streams then share DRAM channels and
 * banks; the pad staggers them (+2.0% on the RS(8+3) step at 64 MiB cells,
 * profiles/r02_ab_cell_pad.txt; the bench uses this layout). Any stride >=
 * chunk_size is correct; this one is only faster. */
size_t redset_hip_cell_stride(size_t chunk_size);

/* Parity of every stripe of the set: the work redset_reedsolomon_encode
 * (src/redset_reedsolomon.c:280-402) does across all p ranks; member r's
 * parity slot i = stripe (r+i) mod p, row p+i. lofi/parity: p device pointers. */
int redset_hip_rs_plan_encode(const redset_hip_rs* rs, unsigned char* const* lofi,
                              unsigned char* const* parity, size_t chunk_size,
                              size_t cell_stride, redset_hip_plan** out);

/* Rebuild the cells of `missing` erased members (ascending, as
 * redset_recover_rs builds them, src/redset_reedsolomon.c:1111-1119) in every
 * stripe; replaces redset_reedsolomon_decode (src/redset_reedsolomon.c:
 * 570-785) / redset_recover_rs_rebuild_serial (src/redset_reedsolomon_
 * serial.c:165-343). Outputs land in the erased members' lofi/parity cells.
 * Fails if missing > encoding (src/redset_reedsolomon.c:1096). */
int redset_hip_rs_plan_rebuild(const redset_hip_rs* rs, int missing, const int* rebuild_ranks,
                               unsigned char* const* lofi, unsigned char* const* parity,
                               size_t chunk_size, size_t cell_stride, redset_hip_plan** out);

/* XOR parity of every stripe: member r's cell = XOR of every other member's
 * cell of stripe r (src/redset_xor.c:220-295). xorc: p device pointers. */
int redset_hip_xor_plan_encode(int ranks, unsigned char* const* lofi, unsigned char* const* xorc,
                               size_t chunk_size, size_t cell_stride, redset_hip_plan** out);

/* Rebuild member `root` (src/redset_xor.c:441-531,
 * src/redset_xor_serial.c:161-275). */
int redset_hip_xor_plan_rebuild(int ranks, int root, unsigned char* const* lofi,
                                unsigned char* const* xorc, size_t chunk_size, size_t cell_stride,
                                redset_hip_plan** out);

/* Enqueue the plan's kernels on `stream`; no host synchronisation, no
 * allocation (safe inside hipStreamBeginCapture). A big-cell RS(8+3)
 * encode plan runs as one launch whose blocks claim their rows at run time
 * (DESIGN.md §4), with the claim counters in the plan: one plan must not
 * execute on two streams at once (its outputs would race anyway). */
int redset_hip_plan_execute(const redset_hip_plan* plan, void* stream);
int redset_hip_plan_get_info(const redset_hip_plan* plan, redset_hip_plan_info* info);
void redset_hip_plan_destroy(redset_hip_plan* plan);

/* ---- set verification (scrub) ---------------------------------------- */
/*
 * Does the stored parity still match the stored data, and if not, where and
 * in which member? A verify plan reads every cell of the set once, writes no
 * cell, and leaves one report row per (stripe, parity row): how many bytes of
 * that stored parity cell differ from the parity of the stored data (the
 * syndrome's nonzero bytes) and the first such byte. A damaged DATA cell
 * shows in all e rows of its stripe, a damaged PARITY cell in its own row
 * only; with e >= 2 that names the damaged member (locate, below), which
 * redset_hip_rs_plan_rebuild then repairs. The reference has no counterpart:
 * it finds a damaged file only when a restart reads it.
 */
typedef struct {
  unsigned long long mismatch_bytes;  /* bytes of this parity row that differ from the data's parity */
  unsigned long long first_offset;    /* smallest differing byte offset in the cell; ~0ULL if none */
} redset_hip_verify_row;              /* row [stripe * e + i]: stripe's parity row i (e = 1 for XOR) */

/* Verify plans execute through redset_hip_plan_execute like any plan: kernel
 * launches only (the report is reset by one), no allocation and no
 * host synchronisation (safe inside hipStreamBeginCapture); every execute
 * first resets the report on the stream, so a replay starts clean. No cell is
 * modified. Stripes of d = p - e <= 16 data cells and e <= 4 (XOR: p <= 16)
 * run FUSED: one pass reads each cell once and writes nothing
 * (plan info: bytes_written == 0, bytes_read == p*(d+e)*chunk_size for RS,
 * p*p*chunk_size for XOR). Wider shapes -- any valid (p, e) works -- compute
 * the parity of <= 4 rows at a time into plan-owned scratch with the
 * combine passes, in column windows of <= 8 MiB, and check the scratch
 * against the stored cells: the scratch is bounded by 4 x 8 MiB = 32 MiB
 * whatever the set, and counts in bytes_written. An XOR row's report names
 * the stripe, not a cell: one parity row cannot tell which cell is wrong. */
int redset_hip_rs_plan_verify(const redset_hip_rs* rs, unsigned char* const* lofi,
                              unsigned char* const* parity, size_t chunk_size, size_t cell_stride,
                              redset_hip_plan** out);
int redset_hip_xor_plan_verify(int ranks, unsigned char* const* lofi, unsigned char* const* xorc,
                               size_t chunk_size, size_t cell_stride, redset_hip_plan** out);
/* The report of the plan's last execute: p * e rows (nrows must be at least
 * that; rows and total_mismatch_bytes may each be NULL). Ordered on `stream`
 * after the work already there; waits for it. */
int redset_hip_plan_verify_report(const redset_hip_plan* plan, void* stream, redset_hip_verify_row* rows,
                                  int nrows, unsigned long long* total_mismatch_bytes);

/* Locate (host): `syndrome` is e bytes of one byte column of stripe chunk_id
 * (stored parity ^ parity of stored data, row by row). *member_out = the one
 * member whose single wrong byte explains it, or -1 (clean, e < 2, or no
 * single member explains it). Rule: exactly one nonzero row i names the
 * holder of parity row i, member (chunk_id - i) mod p; otherwise the answer
 * is the unique data member m for which one value x gives
 * syndrome[j] = A[j][m] * x for every row j (A = the parity rows of the
 * encoding matrix). Any two columns of [A | I] are independent -- the code
 * rebuilds any e erasures -- so with e >= 2 a single wrong member is never
 * mistaken for another; two wrong members in one column may look like a
 * third when e == 2, as with any code of distance 3. */
int redset_hip_rs_locate_syndrome(const redset_hip_rs* rs, int chunk_id, const unsigned char* syndrome,
                                  int* member_out);
/* After an execute of an RS verify plan: reads back the p bytes of `stripe`
 * at its first differing offset (ordered on `stream`, waits) and locates.
 * *offset_out = that offset (~0ULL and member -1 if the stripe is clean).
 * XOR plans answer -1: one parity row locates nothing. */
int redset_hip_plan_verify_locate(const redset_hip_plan* plan, void* stream, int stripe, int* member_out,
                                  unsigned long long* offset_out);

/* ---- repair (single-error-per-column correction) ---------------------- */
/*
 * What follows a scrub that found damage, short of a rebuild: for every byte
 * column of a damaged stripe, form the syndrome, apply exactly the rule of
 * redset_hip_rs_locate_syndrome and XOR the one wrong byte right. Only the
 * wrong bytes are written. Members each damaged at different offsets -- more
 * members than a rebuild has erasures for -- are repaired as long as every
 * byte column has at most one wrong byte. RS sets with 2 <= e <= 4 only: one
 * parity row (e = 1, XOR sets) locates nothing, and e > 4 is not built.
 * Capability per e: a column with one wrong byte is always corrected; a
 * column with two wrong bytes is reported unlocated for e >= 3 and, for
 * e == 2 (distance 3), may be reported unlocated or MIScorrected into a third
 * member -- the member checksums below arbitrate (setfiles.repair_set
 * checksums=True). Columns no single member explains are left as found.
 */
typedef struct {
  unsigned long long corrected_bytes;  /* bytes of this member's cell of this stripe that were (apply) or would be (dry run) corrected */
  unsigned long long first_offset;     /* smallest such cell offset; ~0ULL if none */
} redset_hip_repair_cell;              /* [stripe * p + member] */
typedef struct {
  unsigned long long unlocated_columns; /* nonzero-syndrome byte columns no single member explains */
  unsigned long long first_unlocated;   /* ~0ULL if none */
} redset_hip_repair_stripe;             /* [stripe] */

/* Repair plan over `nstripes` stripes (stripes[k] in 0 .. p-1, each at most
 * once; NULL: all p, in order). apply == 0 is a dry run: the same report, no
 * cell byte written. Executes through redset_hip_plan_execute like any plan:
 * kernel launches only (the report is reset by one), no allocation, no host
 * synchronisation (safe inside hipStreamBeginCapture), no block waits on
 * another, so neither the ring nor the hang count can move. 16-B aligned
 * stripes take the vector path, stripes with an unaligned cell and tails the
 * byte path. Plan info: kind 8, jobs = stripes planned, bytes_read =
 * stripes * (d + e) * chunk_size, bytes_written = 0: the corrections are
 * data-dependent (one byte read again and written per corrected byte) and
 * not counted. One plan must not execute on two streams at once. */
int redset_hip_rs_plan_repair(const redset_hip_rs* rs, unsigned char* const* lofi, unsigned char* const* parity,
                              size_t chunk_size, size_t cell_stride, int nstripes, const int* stripes /* NULL: all p */,
                              int apply, redset_hip_plan** out);
/* The report of the plan's last execute, for the planned stripes in plan
 * order: cells[k * p + member] (ncells at least planned stripes * p) and
 * stripes[k] (nstripes at least the planned stripes); either may be NULL.
 * Ordered on `stream` after the work already there; waits for it. */
int redset_hip_plan_repair_report(const redset_hip_plan* plan, void* stream, redset_hip_repair_cell* cells, int ncells,
                                  redset_hip_repair_stripe* stripes, int nstripes);

typedef struct { unsigned long long verify_mismatch_bytes, corrected_bytes, unlocated_columns,
                 remaining_mismatch_bytes; int damaged_stripes, repair_units, cells_written; } redset_hip_repair_summary;

/* ---- checked rebuild (errors-and-erasures decode) ---------------------- */
/*
 * A rebuild that checks its survivors. With k lost members of an RS set,
 * 0 < k < e <= 4, the e - k parity rows a rebuild does not need form a
 * checkable code over the d + e - k surviving cells of every byte column
 * (distance e - k + 1). Capability per e - k: >= 2, one wrong survivor byte
 * per column is located and taken out of the rebuilt bytes; >= 3, two wrong
 * survivor bytes in a column are detected (unlocated); == 2, two wrong bytes
 * may be unlocated or MIScorrected (the member checksums arbitrate,
 * setfiles.rebuild_set checksums=True); == 1, damage is detected, never
 * located. k == 0 is the repair plan's case, k == e the plain rebuild's.
 *
 * The arithmetic, per stripe: H = [A | I], e x (d + e), A the stripe's parity
 * coefficients as the verify and repair plans use them; column i < d is data
 * input i (the data-holding members in ascending order), column d + j parity
 * row j. M = W * H with W invertible and W * H_L = [0 ; I_k] on the lost
 * members' columns L: rows 0 .. e-k-1 (check rows, G) vanish on L, rows
 * e-k .. e-1 (rebuild rows, B) are the identity on L and, on the survivors,
 * exactly redset_hip_rs_decode_matrix's coefficients. R = sum over survivors
 * of G_m * c_m is the reduced syndrome (zero for consistent survivors),
 * v = sum over survivors of B_m * c_m what redset_hip_rs_plan_rebuild stores.
 */

/* M for stripe chunk_id: mat_out e x (d + e) bytes row-major, check rows
 * first; cols_lost_out (may be NULL): the column of rebuild_ranks[i].
 * 1 <= missing <= e (missing == e: no check rows), ranks ascending. Host only. */
int redset_hip_rs_check_matrix(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int chunk_id,
                               unsigned char* mat_out, int* cols_lost_out);
/* Locate (host; the rule the kernel applies literally): reduced_syndrome is
 * the e - k bytes R of one byte column. For each surviving column m in
 * order: j0 = the first check row with G[j0][m] != 0, x = R[j0] / G[j0][m];
 * m explains the column when x != 0 and G[j][m] * x == R[j] in every check
 * row. Exactly one match: *member_out = the member holding that cell,
 * *value_out (may be NULL) = x: that cell's byte is wrong by x and the
 * rebuilt bytes by B_m * x. Otherwise (R zero, none or several match, always
 * so with e - k == 1) -1 and 0. */
int redset_hip_rs_locate_reduced(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int chunk_id,
                                 const unsigned char* reduced_syndrome, int* member_out, unsigned char* value_out);

/* Checked rebuild plan over all p stripes: every lost cell gets its rebuilt
 * bytes, with the error of a located survivor byte taken out before the
 * store; unlocated columns store the bytes the plain rebuild would.
 * fix_survivors != 0 also XORs the located survivor byte right (a one-byte
 * read-modify-write); otherwise no survivor byte is written. Exactly
 * chunk_size bytes of each lost cell are written, nothing in the padding up
 * to cell_stride. Executes through redset_hip_plan_execute like any plan:
 * two kernel launches (report reset, decode), no allocation, no host
 * synchronisation (safe inside hipStreamBeginCapture), no block waits on
 * another, so neither the ring nor the hang count can move. Plan info: kind
 * 9, jobs = p, bytes_read = p * (d + e - k) * chunk_size, bytes_written =
 * p * k * chunk_size. Refused at plan time: missing == 0, missing == e,
 * missing > e, e > 4, duplicate, unsorted or out-of-range ranks. One plan
 * must not execute on two streams at once. */
int redset_hip_rs_plan_rebuild_checked(const redset_hip_rs* rs, int missing, const int* rebuild_ranks,
                                       unsigned char* const* lofi, unsigned char* const* parity, size_t chunk_size,
                                       size_t cell_stride, int fix_survivors, redset_hip_plan** out);
/* The report of the plan's last execute, shaped as the repair plan's:
 * cells[stripe * p + member] (ncells at least p * p): survivor bytes located
 * as wrong (corrected with fix_survivors; their effect on the rebuilt bytes
 * is removed either way) and the smallest such offset; stripes[stripe]
 * (nstripes at least p): unlocated columns. Either may be NULL. Ordered on
 * `stream` after the work already there; waits for it. */
int redset_hip_plan_rebuild_checked_report(const redset_hip_plan* plan, void* stream, redset_hip_repair_cell* cells,
                                           int ncells, redset_hip_repair_stripe* stripes, int nstripes);

typedef struct { unsigned long long corrected_bytes, unlocated_columns;
                 int stripes_with_findings, cells_written; } redset_hip_rebuild_checked_summary;

/* ---- member checksums (zlib CRC-32 on the device) --------------------- */
/*
 * The parity says whether a stripe is consistent, not which bytes are wrong
 * (an XOR row names no cell; two wrong members may look like a third), and a
 * plain rebuild trusts every survivor (the checked rebuild above does not,
 * within its distance). A content checksum per member answers both.
 * It is the CRC-32 of zlib (reflected polynomial 0xEDB88320, initial value
 * and final XOR 0xFFFFFFFF, 0 for no bytes): what the reference computes in
 * redset_crc32 (src/redset_io.c:477-510) and never stored (the crc_on_copy
 * blocks, src/redset_reedsolomon.c:557-563, :1018-1050). Computed where the
 * cells already are; redset_amd/setfiles.py keeps it beside the set.
 */

/* zlib's crc32_combine: CRC of A||B from crc(A), crc(B), len(B). Host only. */
unsigned redset_hip_crc32_combine(unsigned crc_a, unsigned crc_b, unsigned long long len_b);

typedef struct {
  const unsigned char* ptr;  /* device memory; any byte address */
  size_t len;                /* any length; 0 gives CRC 0 (ptr may then be NULL) */
} redset_hip_crc_range;

/* One CRC per range; arrays copied, buffers must outlive the plan. Executes
 * through redset_hip_plan_execute like any plan (launches only, capture-safe:
 * no allocation, no host synchronisation, and no block waits on another, so
 * neither the ring nor the hang count can move); every execute recomputes
 * from the bytes then in memory. Ranges may overlap. 16-B aligned interiors
 * take the vector path, heads and tails the byte path. Plan info: kind 7,
 * jobs = nranges, bytes_read = the ranges' lengths summed, bytes_written 0.
 * One plan must not execute on two streams at once (its scratch is its own). */
int redset_hip_plan_crc32(const redset_hip_crc_range* ranges, int nranges, redset_hip_plan** out);
/* The CRCs of the last execute (ncrcs at least the plan's ranges); ordered on
 * `stream` after the work already there, waits for it. */
int redset_hip_plan_crc32_report(const redset_hip_plan* plan, void* stream, unsigned* crcs, int ncrcs);

/* ---- stripe primitives (one stripe, device pointers) ----------------- */

/* out[j] = (out[j] ^) sum_i coeffs[j*nin + i] * in[i] over GF(2^8), for
 * nbytes bytes; 1 <= nin, nout <= 256. Up to 16 inputs x 4 outputs run as
 * one kernel pass; wider calls run 16-input accumulate passes per group of
 * 4 outputs (outputs must not alias inputs then). One pass replaces nout*nin
 * calls of redset_rs_reduce_buffer_multadd (src/redset_reedsolomon_common.c:
 * 786-819) and, with a decode matrix, redset_rs_reduce_decode +
 * redset_rs_gaussian_solve (:855-899, :570-630). */
int redset_hip_gf_combine(const unsigned char* const* in, int nin, unsigned char* const* out,
                          int nout, const unsigned char* coeffs, size_t nbytes, int accumulate,
                          void* stream);

/* out = (out ^) XOR of nin inputs, 1 <= nin <= 256 (reduce_xor, src/redset_xor.c:35-42). */
int redset_hip_xor_combine(const unsigned char* const* in, int nin, unsigned char* out,
                           size_t nbytes, int accumulate, void* stream);

/* Many stripe combines of nbytes each as one plan (the gf_mac / xor kernels
 * with the set plans' job orders: jobs of one shape share a launch): job k is
 * out[j] = (out[j] ^) sum_i coef[j*nin + i] * in[i], as redset_hip_gf_combine;
 * a job with one output and every coefficient 1 runs on the XOR kernel. No
 * job's output may be another job's input. The arrays are copied; the
 * buffers must outlive the plan. Used by the sharded plans' partial-sum
 * shape (REDSET_HIP_SHAPE_REDUCE). */
typedef struct {
  int nin, nout;
  const unsigned char* const* in;   /* nin device pointers */
  unsigned char* const* out;        /* nout device pointers */
  const unsigned char* coef;        /* nout x nin */
  int accumulate;                   /* XOR into the outputs */
} redset_hip_combine_job;
int redset_hip_plan_combine(const redset_hip_combine_job* jobs, int njobs, size_t nbytes,
                            redset_hip_plan** out);

/* Host-side decode matrix for one stripe: rows = missing outputs, columns =
 * the p members (0 for erased members / unused cells). coef_out: missing x p
 * bytes. Equals the reference's reduce_decode + gaussian_solve as one linear
 * map. */
int redset_hip_rs_decode_matrix(const redset_hip_rs* rs, int missing, const int* rebuild_ranks,
                                int chunk_id, unsigned char* coef_out);

/* ---- host-resident streaming pipeline (pinned staging <-> HBM) ------- */
/*
 * Encode / rebuild a set whose cells live outside the GPU (host memory or
 * files): cells stream through pinned host buffers, hipMemcpyAsync to HBM,
 * the gf_mac / xor kernel, and back, with reads, H2D, compute, D2H and writes
 * of successive (stripe, slice) units overlapped. This is the shape of the
 * reference's own loop -- slices of redset_mpi_buf_size read via
 * redset_lofi_pread, combined, written after the header
 * (src/redset_reedsolomon.c:309-391) -- with the arithmetic on the GPU.
 */
#define REDSET_HIP_CELL_DATA (0)    /* logical-file segment `index` */
#define REDSET_HIP_CELL_PARITY (1)  /* redundancy slot `index` */

typedef struct {
  /* Read / write `len` bytes at byte `offset` of a cell of member `rank`
   * (kind DATA: logical-file offset index*chunk_size + offset; kind PARITY:
   * redundancy-file offset header + index*chunk_size + offset). Return 0 on
   * success. Called concurrently from the pipeline's I/O threads. */
  int (*read)(void* ctx, int rank, int kind, int index, unsigned long long offset, size_t len, void* dst);
  int (*write)(void* ctx, int rank, int kind, int index, unsigned long long offset, size_t len, const void* src);
  /* Optional (may be NULL): host address of the cell bytes at `offset` if
   * that memory is page-locked, so the pipeline can DMA it directly instead
   * of staging it through read/write; NULL = use read/write. */
  void* (*map)(void* ctx, int rank, int kind, int index, unsigned long long offset);
  void* ctx;
} redset_hip_io;

typedef struct {
  double seconds;                    /* wall time of the call */
  unsigned long long bytes_read;     /* algorithmic bytes of cells read */
  unsigned long long bytes_written;  /* algorithmic bytes of cells written */
  unsigned long long units;          /* (stripe, slice) units */
  double read_seconds;               /* summed time inside io->read */
  double write_seconds;              /* summed time inside io->write */
  double gpu_seconds;                /* H2D + kernels + D2H, event-timed */
} redset_hip_stream_stats;

/* Stripes [first_stripe, first_stripe + nstripes) (nstripes <= 0: all).
 * slice_bytes: per-cell slice (0 = 8 MiB); io_threads (0 = 8). */
int redset_hip_rs_encode_stream(const redset_hip_rs* rs, size_t chunk_size, int first_stripe, int nstripes,
                                size_t slice_bytes, int io_threads, const redset_hip_io* io,
                                redset_hip_stream_stats* stats);
int redset_hip_rs_rebuild_stream(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, size_t chunk_size,
                                 int first_stripe, int nstripes, size_t slice_bytes, int io_threads,
                                 const redset_hip_io* io, redset_hip_stream_stats* stats);
int redset_hip_xor_encode_stream(int ranks, size_t chunk_size, int first_stripe, int nstripes, size_t slice_bytes,
                                 int io_threads, const redset_hip_io* io, redset_hip_stream_stats* stats);
int redset_hip_xor_rebuild_stream(int ranks, int root, size_t chunk_size, int first_stripe, int nstripes,
                                  size_t slice_bytes, int io_threads, const redset_hip_io* io,
                                  redset_hip_stream_stats* stats);

/* Verify a host-resident set (see "set verification" above): the same read ->
 * H2D -> kernel pipeline with the check kernels, and no D2H or write stage:
 * io->write is never called (it may be NULL), page-locked cells (io->map) are
 * read in place. rows: (stripe - first_stripe) * e + i for the stripes of
 * the call, nrows at least that many; offsets are cell offsets whatever the
 * slice. Returns REDSET_SUCCESS when the check RAN (damage is in the rows,
 * not in the return code), REDSET_FAILURE on I/O or device errors or when the
 * hang count moved. Wide stripes use <= 32 MiB of device scratch. */
int redset_hip_rs_verify_stream(const redset_hip_rs* rs, size_t chunk_size, int first_stripe, int nstripes,
                                size_t slice_bytes, int io_threads, const redset_hip_io* io,
                                redset_hip_stream_stats* stats, redset_hip_verify_row* rows, int nrows);
int redset_hip_xor_verify_stream(int ranks, size_t chunk_size, int first_stripe, int nstripes, size_t slice_bytes,
                                 int io_threads, const redset_hip_io* io, redset_hip_stream_stats* stats,
                                 redset_hip_verify_row* rows, int nrows);

/* Repair a host-resident set (memory or files, see "repair" above):
 * 1. redset_hip_rs_verify_stream over the stripes; a clean result returns at
 *    once (repair_units == 0, no repair launch): a clean scrub costs what it
 *    costs today.
 * 2. every stripe with a nonzero row, slice by slice, synchronously: io->read
 *    the stripe's p cell slices, run the repair kernel on them, read the
 *    slice's report (offsets are cell offsets) and, with apply, io->write
 *    only the cells corrected in that slice, only that slice's range
 *    (cells_written counts them; repair_units the slices).
 * 3. with apply, the check kernels again over the repaired stripes:
 *    remaining_mismatch_bytes (a correction that falls into a logical file's
 *    zero padding is dropped by the file I/O's write rule and shows here);
 *    without, remaining_mismatch_bytes == verify_mismatch_bytes.
 * cells[(stripe - first_stripe) * p + member] and stripes[stripe -
 * first_stripe] are summed over the slices (each may be NULL). Returns
 * REDSET_SUCCESS when the procedure RAN (damage is in the outputs),
 * REDSET_FAILURE on I/O or device errors. io->write may be NULL when
 * apply == 0. Device and pinned memory are allocated per call. */
int redset_hip_rs_repair_stream(const redset_hip_rs* rs, size_t chunk_size, int first_stripe, int nstripes,
                                size_t slice_bytes, int io_threads, const redset_hip_io* io, int apply,
                                redset_hip_stream_stats* stats, redset_hip_repair_cell* cells, int ncells,
                                redset_hip_repair_stripe* stripes, int nstripes_out, redset_hip_repair_summary* summary);

/* Checked rebuild of a host-resident set (memory or files, see "checked
 * rebuild" above). For every stripe of the call and every slice,
 * synchronously: io->read the survivors' slices, run the decode kernel on
 * them (report offsets are cell offsets), io->write the k rebuilt slices
 * and, with fix_survivors, only those survivor cells corrected in that
 * slice, only that slice's range. cells[(stripe - first_stripe) * p +
 * member] and stripes[stripe - first_stripe] are summed over the slices
 * (each may be NULL); summary: corrected survivor bytes, unlocated columns,
 * stripes with any finding, and cells written (rebuilt and corrected
 * slices). Refuses what the plan refuses. Returns REDSET_SUCCESS when the
 * rebuild RAN (findings are in the outputs). Device and pinned memory are
 * allocated per call and freed on every way out. */
int redset_hip_rs_rebuild_checked_stream(const redset_hip_rs* rs, int missing, const int* rebuild_ranks,
                                         size_t chunk_size, int first_stripe, int nstripes, size_t slice_bytes,
                                         int io_threads, const redset_hip_io* io, int fix_survivors,
                                         redset_hip_stream_stats* stats, redset_hip_repair_cell* cells, int ncells,
                                         redset_hip_repair_stripe* stripes, int nstripes_out,
                                         redset_hip_rebuild_checked_summary* summary);

/* CRC-32 of byte spans of a host-resident set, in the members' own
 * coordinates: the same read -> H2D -> kernel pipeline with the CRC kernels,
 * no D2H of cells and no write stage (io->write is never called, it may be
 * NULL; page-locked cells, io->map, are copied to the device from where they
 * lie, with no read and no staging copy). A span is cut at cell
 * boundaries (cell index = offset / chunk_size) and at slice boundaries
 * within the cell, the pieces' CRCs are computed on the device and joined on
 * the host with redset_hip_crc32_combine. Spans may be empty (CRC 0), overlap
 * and cross any number of cells; a DATA span reaching past the member's last
 * file reads the logical file's zero padding, as every cell read does. */
typedef struct {
  int rank, kind;              /* REDSET_HIP_CELL_DATA: bytes of the member's logical file;
                                  REDSET_HIP_CELL_PARITY: bytes of its redundancy payload (after the header) */
  unsigned long long offset;   /* first byte, in that coordinate */
  unsigned long long len;
} redset_hip_crc_span;
int redset_hip_crc32_stream(size_t chunk_size, const redset_hip_crc_span* spans, int nspans, size_t slice_bytes,
                            int io_threads, const redset_hip_io* io, redset_hip_stream_stats* stats,
                            unsigned* crcs /* nspans */);

/* The streaming calls keep a successful call's three streams and (up to
 * 256 MiB pinned, 1 GiB of device memory) its staging buffers for the next
 * call; REDSET_HIP_SCRATCH_CACHE=0 allocates and frees per call. This frees
 * what is cached. */
void redset_hip_release_scratch(void);

/* Built-in I/O over host memory laid out like the device set layout
 * (lofi[r] + s*cell_stride, parity[r] + i*cell_stride). pinned != 0 declares
 * the memory page-locked (hipHostMalloc / hipHostRegister): cells are then
 * DMAed directly, with no staging copy. */
typedef struct redset_hip_hostio redset_hip_hostio;
int redset_hip_hostio_create(int ranks, unsigned char* const* lofi, unsigned char* const* parity, size_t cell_stride,
                             int pinned, redset_hip_io* io_out, redset_hip_hostio** out);
void redset_hip_hostio_destroy(redset_hip_hostio* h);

/* Built-in I/O over files with redset's logical-file semantics
 * (src/redset_lofi.c:30-173): member r's logical file is the concatenation
 * of its nfiles[r] data files (paths/sizes flattened member by member);
 * reads past a file's recorded size return zeros, writes past it are
 * dropped. Member r's parity goes to redundancy_paths[r] at
 * header_sizes[r] + slot*chunk_size (src/redset_reedsolomon.c:380-381).
 * Data files of members with writable[r] != 0 are created / extended to their
 * recorded size (rebuild targets); other data files are opened read-only.
 * redundancy_paths may be NULL (data-only I/O, e.g. for the per-rank MPI
 * backends, which use their own fd_chunk). */
typedef struct redset_hip_fileio redset_hip_fileio;
int redset_hip_fileio_create(int ranks, const int* nfiles, const char* const* paths,
                             const unsigned long long* sizes, const char* const* redundancy_paths,
                             const unsigned long long* header_sizes, size_t chunk_size, const int* writable,
                             redset_hip_io* io_out, redset_hip_fileio** out);
void redset_hip_fileio_destroy(redset_hip_fileio* f);

/* ---- sets sharded over the GPUs of a node (multi-rank rebuild) ------- */
/*
 * Replaces the reference's MPI rings for a redundancy set whose members live
 * on different GPUs: the decode's reduce ring (src/redset_reedsolomon.c:
 * 646-703) becomes ONE grouped exchange that gathers, onto every GPU, its
 * column slice of each cell the decode reads; every GPU runs the gf_mac
 * kernel on its slice of every stripe; a second grouped exchange returns the
 * rebuilt slices to the GPUs hosting the lost members (the gather of :713-733).
 * Byte j of an output depends only on byte j of its stripe's inputs
 * (SURVEY.md §8e), so the column slices are independent. Encode works the
 * same way (all data cells in, all parity cells back; replaces :329-377).
 *
 * World: `world` processes (one per GPU), this one is `rank`. The caller
 * places `nsets` sets of p members: member r of set k is hosted by process
 * host[k*p + r] at hosted index slot[k*p + r] (< max_hosted). Every cell is
 * cut into `world` column slices of `slice_bytes` (W) bytes
 * (redset_hip_shard_slice_bytes); slice q covers cell bytes [q*W, q*W + W)
 * clipped to chunk_size. Buffers of this process (device memory for the HIP
 * compute and RCCL; any memory the transport and compute can address):
 *   hosted_data     [world][max_hosted][d][W]   slice q of data cell s of my
 *                                               hosted member j
 *   hosted_parity   [world][max_hosted][e][W]   same for parity slot i
 *   gathered_data   [world][max_hosted][d][W]   my slice of data cell s of the
 *                                               member hosted at (h, j)
 *   gathered_parity [world][max_hosted][e][W]
 * (d = p - e). A member's logical file is thus stored as `world` column slabs.
 */
typedef struct {
  int peer;     /* process in the transport's world; == own rank: a local copy */
  int send;     /* 1: send buf to peer; 0: receive buf from peer (local copy:
                   the send entry is the source, the receive entry right after
                   it the destination) */
  void* buf;
  size_t len;
} redset_hip_xfer;

typedef struct {
  int world, rank;
  /* Run one exchange: every transfer of the list concurrently (sends and
   * receives between a pair of processes are listed in the same order on
   * both sides, with equal lengths). Stream-ordered transports (RCCL) enqueue
   * on `stream` and return; others complete before returning, after waiting
   * for work already on `stream`. Return 0 on success. */
  int (*exchange)(void* ctx, const redset_hip_xfer* xfers, int n, void* stream);
  void* ctx;
} redset_hip_transport;

typedef struct {
  /* Optional compute (NULL run = the HIP gf_mac plans): encode (kind
   * REDSET_HIP_PLAN_RS_ENCODE) or rebuild (..._RS_REBUILD, `missing` erased
   * members) of one set whose cells are at lofi/parity in the set layout
   * (cell_stride apart, nbytes each). Tests put the CPU oracle here. */
  int (*run)(void* ctx, int kind, int missing, const int* rebuild_ranks, unsigned char* const* lofi,
             unsigned char* const* parity, size_t nbytes, size_t cell_stride, void* stream);
  void* ctx;
} redset_hip_compute;

typedef struct {
  int nsets;
  const int* host;              /* [nsets * p] */
  const int* slot;              /* [nsets * p] */
  int max_hosted;
  size_t chunk_size;
  size_t slice_bytes;           /* W */
  unsigned char* hosted_data;
  unsigned char* hosted_parity;
  unsigned char* gathered_data;
  unsigned char* gathered_parity;
} redset_hip_shard_layout;

typedef struct {
  int kind;                               /* REDSET_HIP_PLAN_RS_ENCODE / _REBUILD */
  int world, rank, nsets, missing;
  size_t my_slice_len;                    /* cell bytes of this process's slice */
  int gather_messages, return_messages;   /* peer messages after merging (no local copies) */
  unsigned long long gather_bytes_sent;   /* to other processes, per execute */
  unsigned long long gather_bytes_recv;
  unsigned long long return_bytes_sent;
  unsigned long long return_bytes_recv;
  unsigned long long local_bytes;         /* copied within this process: 0 (own slices computed in place) */
  unsigned long long compute_bytes;       /* algorithmic bytes of this process's slice */
  unsigned long long gather_msg_max;      /* largest / smallest peer message this process sends */
  unsigned long long gather_msg_min;
  unsigned long long return_msg_max;
  unsigned long long return_msg_min;
  int gather_recv_messages, return_recv_messages; /* peer messages this process receives */
} redset_hip_sharded_info;

typedef struct redset_hip_sharded redset_hip_sharded;

/* Phases of one execute, in this order. The gather shape: gather the input
 * slices, compute, return the output slices (ACCUMULATE does nothing). The
 * partial-sum shape (REDSET_HIP_SHAPE_REDUCE): GATHER does nothing, COMPUTE
 * makes this process's partial sums, RETURN sends them to the outputs' hosts,
 * ACCUMULATE adds what arrived (and this process's own inputs) into the
 * outputs. Running the four in order is one execute in either shape. */
enum {
  REDSET_HIP_PHASE_GATHER = 0,
  REDSET_HIP_PHASE_COMPUTE = 1,
  REDSET_HIP_PHASE_RETURN = 2,
  REDSET_HIP_PHASE_ACCUMULATE = 3
};

/* Column slice width for chunk_size bytes over `world` processes: ceil(C/world)
 * rounded up to 256 B (so every slice starts 16-B aligned). */
size_t redset_hip_shard_slice_bytes(size_t chunk_size, int world);

/* Plan the sharded encode (kind REDSET_HIP_PLAN_RS_ENCODE, missing 0) or
 * rebuild of `missing` members (ascending rebuild_ranks, the same in every
 * set) of every set. Collective in the sense that every process plans with
 * the same placement; planning itself does no communication. The rebuild
 * gathers only the cells some stripe's decode reads (surviving data and the
 * parity rows identify_rows selects, src/redset_reedsolomon_common.c:
 * 425-564) and never a lost member's. */
int redset_hip_rs_sharded_plan(const redset_hip_rs* rs, int kind, int missing, const int* rebuild_ranks,
                               const redset_hip_shard_layout* layout, const redset_hip_transport* transport,
                               const redset_hip_compute* compute, redset_hip_sharded** out);
/* The same for an XOR set (e = 1; kind REDSET_HIP_PLAN_XOR_ENCODE, or
 * REDSET_HIP_PLAN_XOR_REBUILD of member `root`): the layout's cells are the
 * p - 1 logical-file segments and the one XOR chunk of every member. The
 * rebuild gathers every survivor's every cell; it replaces the pipelined
 * reduce to the lost member (src/redset_xor.c:466-524). */
int redset_hip_xor_sharded_plan(int ranks, int kind, int root, const redset_hip_shard_layout* layout,
                                const redset_hip_transport* transport, const redset_hip_compute* compute,
                                redset_hip_sharded** out);
/* The same plans with only some processes computing: compute_on[g] != 0 for
 * the K processes that take a column slice each (in rank order, slices
 * 0 .. K - 1; slice_bytes >= ceil(chunk_size / K); NULL: all of them, as
 * above). The others only send the cells they host and receive their
 * members' outputs -- e.g. a rebuild whose lost members then receive just
 * their own cells instead of also gathering a slice of every decode input.
 * Every process must pass the same mask. */
int redset_hip_rs_sharded_plan_on(const redset_hip_rs* rs, int kind, int missing, const int* rebuild_ranks,
                                  const redset_hip_shard_layout* layout, const int* compute_on,
                                  const redset_hip_transport* transport, const redset_hip_compute* compute,
                                  redset_hip_sharded** out);
int redset_hip_xor_sharded_plan_on(int ranks, int kind, int root, const redset_hip_shard_layout* layout,
                                   const int* compute_on, const redset_hip_transport* transport,
                                   const redset_hip_compute* compute, redset_hip_sharded** out);
/* The exchange's shape (redset_hip_sharded_opts.shape).
 * GATHER: every computing process gathers its column slice of every cell a
 *   stripe reads and returns its slice of every output -- (inputs + outputs)
 *   x (world - 1) / world cells per stripe cross the fabric.
 * REDUCE: the code is linear, so every process combines the inputs IT hosts
 *   into partial outputs (the stripe's own coefficients) and sends one
 *   partial per output and contributing process to the output's host, which
 *   XORs them in: outputs x (contributing processes - 1) cells per stripe,
 *   the shape of the reference's XOR ring, which moves partial sums
 *   (src/redset_xor.c:251-279), where its RS decode gathers inputs
 *   (src/redset_reedsolomon.c:690-733). The partials use the gathered slabs
 *   as scratch; a plan whose partials do not fit them, or with over 64
 *   processes, cannot take it.
 * AUTO: whichever moves fewer bytes through the busiest process (max over
 *   processes of max(bytes sent, bytes received) per execute; ties: GATHER).
 *   Every process computes every process's counts, so all choose alike. */
enum { REDSET_HIP_SHAPE_AUTO = 0, REDSET_HIP_SHAPE_GATHER = 1, REDSET_HIP_SHAPE_REDUCE = 2 };

typedef struct {
  size_t struct_size;             /* sizeof(redset_hip_sharded_opts): checked */
  int shape;                      /* REDSET_HIP_SHAPE_* */
  const int* compute_on;          /* as redset_hip_rs_sharded_plan_on (GATHER only; NULL = all) */
  const redset_hip_compute* compute; /* whole-set compute callback (GATHER; NULL = HIP plans) */
  /* the REDUCE shape's compute callback (NULL = HIP plans, redset_hip_plan_combine):
   * run the `njobs` combines of one phase of one set, each over nbytes */
  int (*combine)(void* ctx, const redset_hip_combine_job* jobs, int njobs, size_t nbytes, void* stream);
  void* combine_ctx;
} redset_hip_sharded_opts;

/* The plans above with options: the exchange's shape and the callbacks. The
 * four-argument forms above are this with shape GATHER (their callers run the
 * gather shape's phases themselves, e.g. the per-rank slot). AUTO (or REDUCE)
 * with a whole-set `compute` callback and no `combine` plans GATHER. */
int redset_hip_rs_sharded_plan_ex(const redset_hip_rs* rs, int kind, int missing, const int* rebuild_ranks,
                                  const redset_hip_shard_layout* layout, const redset_hip_transport* transport,
                                  const redset_hip_sharded_opts* opts, redset_hip_sharded** out);
int redset_hip_xor_sharded_plan_ex(int ranks, int kind, int root, const redset_hip_shard_layout* layout,
                                   const redset_hip_transport* transport, const redset_hip_sharded_opts* opts,
                                   redset_hip_sharded** out);

/* Both shapes' byte counts and the one planned. */
typedef struct {
  size_t struct_size;                       /* set by the library */
  int shape;                                /* REDSET_HIP_SHAPE_GATHER or _REDUCE */
  int reduce_possible;                      /* the partial sums fit the scratch */
  unsigned long long gather_busiest_bytes;  /* max over processes of max(sent, received), per execute */
  unsigned long long reduce_busiest_bytes;  /* the same for REDUCE (0 if not possible) */
  unsigned long long gather_bytes_sent, gather_bytes_recv;  /* this process, GATHER */
  unsigned long long reduce_bytes_sent, reduce_bytes_recv;  /* this process, REDUCE */
  unsigned long long scratch_bytes_needed;  /* REDUCE: this process's partial-sum rows */
  unsigned long long scratch_bytes;         /* the gathered slabs */
  int reduce_messages, reduce_recv_messages; /* REDUCE: peer messages per execute, after merging */
  int reduce_fused;                         /* REDUCE: a host folds its own inputs in with the
                                               partials it makes (its inputs read once; needs
                                               more scratch), else it combines them again after
                                               the exchange */
} redset_hip_sharded_shape_info;
/* Copies min(size, sizeof) bytes: callers built against an older header get
 * the fields they know, never a write past their struct. */
int redset_hip_sharded_get_shape(const redset_hip_sharded* plan, redset_hip_sharded_shape_info* info, size_t size);

/* All phases, ordered after the work already on `stream`; work
 * enqueued on `stream` afterwards sees the results. With the HIP plans as
 * compute (compute == NULL at plan time) the sets are pipelined: every set's
 * gather and return is an exchange of its own on a second stream the plan
 * owns, so set k+1's gather (and the first returns) overlap set k's gf_mac on
 * `stream`; in the partial-sum shape set k's exchange overlaps set k+1's
 * combines and set k's accumulate follows its exchange. With a compute (or
 * combine) callback the phases run one after another. */
int redset_hip_sharded_execute(redset_hip_sharded* plan, void* stream);
/* One phase (REDSET_HIP_PHASE_*), so callers can time them apart; the four in
 * order are one execute. */
int redset_hip_sharded_execute_phase(redset_hip_sharded* plan, int phase, void* stream);
int redset_hip_sharded_get_info(const redset_hip_sharded* plan, redset_hip_sharded_info* info);
void redset_hip_sharded_destroy(redset_hip_sharded* plan);

/* RCCL transport over xGMI (grouped ncclSend / ncclRecv on the caller's
 * stream; local copies as hipMemcpyAsync). One process calls
 * redset_hip_rccl_unique_id, the caller distributes the 128 bytes (any
 * channel: MPI_Bcast, torch.distributed, a file), then every process creates
 * its transport collectively (ncclCommInitRank) on its current device. */
typedef struct redset_hip_rccl redset_hip_rccl;
/* 1 if librccl can be loaded in this process (no communication), else 0 */
int redset_hip_rccl_available(void);
int redset_hip_rccl_unique_id(unsigned char id_out[128]);
int redset_hip_rccl_transport_create(const unsigned char id[128], int world, int rank, redset_hip_transport* out,
                                     redset_hip_rccl** handle);
void redset_hip_rccl_transport_destroy(redset_hip_rccl* handle);

/* The kernels count two kinds of capped waits, per device and process-wide
 * (concurrent callers share the counts):
 *
 * Capped handshake SPINS of the loader-wave ring (redset_hip_ring_faults),
 * since the last clearing read. A capped spin never costs correctness: the
 * waiting consumer (or, after a capped loader, every consumer of the rest of
 * the launch) loads its bytes straight from HBM. A nonzero count in the
 * shipped build (cap 2^24 polls) means a ring stalled and ran slower -- a
 * performance event worth reporting, not an error. It happened once in
 * development, from a since-fixed missing barrier (round 2). Synchronises the
 * device; `clear` resets the count. */
int redset_hip_ring_faults(unsigned* count, int clear);

/* Capped HANG waits (redset_hip_hang_faults): waits that end by construction
 * and have no fallback -- the streamed and claimed kernels' table hand-over,
 * claim records and end-of-sequence agreement. Their cap (2^26 polls) only
 * keeps a bug from hanging the GPU; a capped one proceeds with another job's
 * tables or drops rows, so THAT LAUNCH'S OUTPUTS ARE WRONG. The synchronous
 * entry points that run kernels -- the streaming calls, the per-rank backends
 * of redset_hip_mpi.h (host and sharded exchanges) and the offline rebuild
 * tool -- read this count before and after their work and return
 * REDSET_FAILURE when it moved, so they never report success with wrong
 * bytes (a concurrent caller's hang on the same device fails them too). The
 * asynchronous ones (redset_hip_plan_execute, redset_hip_sharded_execute,
 * the stripe primitives) cannot: their caller reads this after its own sync.
 * The read is ordered on `stream` after the work already there and waits
 * for it; NULL reads on the library's own non-blocking stream, ordered after
 * nothing (sync the work to be counted first). `clear` resets the count. */
int redset_hip_hang_faults(void* stream, unsigned* count, int clear);

/* 1 if this is the test twin library (built with REDSET_HIP_TEST_KNOBS: it
 * honours the environment knobs the test suite uses to force job orders,
 * ring fallbacks and injected failures), 0 for the product library, which
 * reads none of them. */
int redset_hip_test_build(void);

/* Text of the last failure on this thread ("" if none). */
const char* redset_hip_last_error(void);
/* For layers built on this library (the per-rank backends of
 * redset_hip_mpi.h): record `msg` as this thread's last failure; returns
 * REDSET_FAILURE. */
int redset_hip_record_error(const char* msg);
/* Library version string. */
const char* redset_hip_version(void);
/* The revision of this header's struct layouts (REDSET_HIP_ABI_VERSION) the
 * library was built with. It changes whenever a struct that crosses this
 * ABI changes size or layout; a caller compares it with the header it was
 * built against and refuses to run on a mismatch (the Python binding and the
 * per-rank backends do), so a stale caller fails loudly instead of writing
 * past a struct. 6: round 6 (combine jobs, sharded options and
 * shape info; PHASE_ACCUMULATE). */
#define REDSET_HIP_ABI_VERSION 6
int redset_hip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* REDSET_HIP_H */
