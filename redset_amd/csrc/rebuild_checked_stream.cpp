// rebuild_checked_stream.cpp -- errors-and-erasures rebuild of a host-resident
// set (memory or files) through the redset_hip_io callbacks
// (include/redset_hip.h, redset_hip_rs_rebuild_checked_stream).
//
// A synchronous loop in the manner of repair_stream.cpp step 2: every stripe
// goes slice by slice through read (survivors) -> H2D ->
// gf_rebuild_checked_kernel -> report and D2H of the k rebuilt slices ->
// write, plus (fix_survivors) D2H and write of the survivor cells corrected
// in that slice. Staging memory is allocated per call and freed on return.
// redset_hip_rs_rebuild_checked_wide_stream is the same loop (checked_loop)
// with gf_rebuild_checked_wide_kernel: what differs is behind StripeDriver.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "codec_kernels.h"
#include "rebuild_checked.h"
#include "rebuild_checked_wide.h"
#include "redset_hip.h"
#include "stripe_map.h"

using redset_hip::CellRef;
using redset_hip::fail;

namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int hip_ok(hipError_t e, const char* what) { return e == hipSuccess ? 0 : fail("%s: %s", what, hipGetErrorString(e)); }

// what the call allocates, freed on every way out
struct Staging {
  void* host = nullptr;
  void* dev = nullptr;
  void* report = nullptr;
  void* blob = nullptr;
  hipStream_t stream = nullptr;
  ~Staging() {
    if (blob) (void) hipFree(blob);
    if (report) (void) hipFree(report);
    if (dev) (void) hipFree(dev);
    if (host) (void) hipHostFree(host);
    if (stream) (void) hipStreamDestroy(stream);
  }
};

// What the two decode kernels differ in: a stripe's matrix, its one job over
// the staging cells, and the launch.
struct StripeDriver {
  const char* name;     // of the entry point, for messages
  size_t report_words;  // 2 p cell words, 2 stripe words, then the kernel's own
  virtual ~StripeDriver() {}
  // stripe first_stripe + q: its cells, lost columns and matrix; REDSET_* code
  virtual int prepare(int q, int c) = 0;
  virtual const redset_hip::CheckMatrix& matrix(int q) const = 0;
  // stripe q's job with survivors at `in`, lost cells at `out`, reports at `report`; hipError_t as int
  virtual int upload(int q, const std::vector<uint8_t*>& in, const std::vector<uint8_t*>& out,
                     unsigned long long* report, void** blob_out) = 0;
  virtual int reset(hipStream_t s) = 0;
  virtual int launch(size_t len, size_t off, hipStream_t s) = 0;
  // one slice's report words past the first 2 p + 2
  virtual void extra(const unsigned long long* words) { (void) words; }
};

// The loop both entry points run; the caller has checked e, k and max_errors.
int checked_loop(const redset_hip_rs* rs, int missing, size_t chunk_size, int first_stripe, int nstripes,
                 size_t slice_bytes, const redset_hip_io* io, int fix_survivors, redset_hip_stream_stats* stats,
                 redset_hip_repair_cell* cells, int ncells, redset_hip_repair_stripe* stripes, int nstripes_out,
                 redset_hip_rebuild_checked_summary* summary, StripeDriver& D) {
  const int p = rs->ranks, k = missing, ns = p - k;
  if (nstripes <= 0) {
    first_stripe = 0;
    nstripes = p;
  }
  if (first_stripe < 0 || first_stripe + nstripes > p)
    return fail("stripe range [%d, %d) outside 0..%d", first_stripe, first_stripe + nstripes, p);
  const int lo = first_stripe, n = nstripes;
  if (cells && ncells < n * p) return fail("%s: room for %d cells, the call reports %d", D.name, ncells, n * p);
  if (stripes && nstripes_out < n) return fail("%s: room for %d stripes, the call reports %d", D.name, nstripes_out, n);
  // every stripe's matrix first: bad ranks are refused before anything is read
  for (int q = 0; q < n; ++q)
    if (int rc = D.prepare(q, lo + q)) return rc;
  for (int i = 0; cells && i < n * p; ++i) cells[i] = redset_hip_repair_cell{0, ~0ull};
  for (int i = 0; stripes && i < n; ++i) stripes[i] = redset_hip_repair_stripe{0, ~0ull};
  redset_hip_rebuild_checked_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  redset_hip_stream_stats st;
  std::memset(&st, 0, sizeof(st));
  const double t0 = now_s();
  auto done = [&](int rc) {
    st.seconds = now_s() - t0;
    if (stats) *stats = st;
    if (summary) *summary = sum;
    return rc;
  };
  if (chunk_size == 0) return done(REDSET_SUCCESS);

  // the verify stream's slice rule
  const size_t chunk = chunk_size;
  size_t slice = slice_bytes;
  if (slice == 0) slice = chunk > (8u << 20) ? (8u << 20) : std::max<size_t>(256u << 10, chunk / 16);
  slice = std::min(slice, chunk);
  slice = (slice + 255) & ~static_cast<size_t>(255);
  Staging S;
  // staging cell i < ns: survivor i; ns + i: lost cell i
  const size_t stage_in = static_cast<size_t>(ns) * slice, stage = static_cast<size_t>(p) * slice;
  const size_t report_words = D.report_words;
  if (int rc = hip_ok(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking), "hipStreamCreate")) return done(rc);
  if (int rc = hip_ok(hipHostMalloc(&S.host, stage, hipHostMallocDefault), "hipHostMalloc(checked rebuild staging)"))
    return done(rc);
  if (int rc = hip_ok(hipMalloc(&S.dev, stage), "hipMalloc(checked rebuild staging)")) return done(rc);
  if (int rc = hip_ok(hipMalloc(&S.report, report_words * sizeof(unsigned long long)), "hipMalloc(checked rebuild report)"))
    return done(rc);
  uint8_t* const host = static_cast<uint8_t*>(S.host);
  uint8_t* const dev = static_cast<uint8_t*>(S.dev);
  std::vector<unsigned long long> raw(report_words);
  for (int q = 0; q < n; ++q) {
    const redset_hip::CheckMatrix& M = D.matrix(q);
    std::vector<CellRef> in, out;
    std::vector<uint8_t*> in_dev, out_dev;
    for (int i = 0; i < p; ++i) {
      if (std::find(M.lost_cols.begin(), M.lost_cols.end(), i) != M.lost_cols.end()) continue;
      in_dev.push_back(dev + in.size() * slice);
      in.push_back(M.cells[static_cast<size_t>(i)]);
    }
    for (int i : M.lost_cols) {
      out_dev.push_back(dev + (static_cast<size_t>(ns) + out.size()) * slice);
      out.push_back(M.cells[static_cast<size_t>(i)]);
    }
    if (S.blob) (void) hipFree(S.blob);
    S.blob = nullptr;
    if (int rc = hip_ok(static_cast<hipError_t>(
                            D.upload(q, in_dev, out_dev, static_cast<unsigned long long*>(S.report), &S.blob)),
                        "checked rebuild job upload"))
      return done(rc);
    bool finding = false;
    for (size_t off = 0; off < chunk; off += slice) {
      const size_t len = std::min(slice, chunk - off);
      const double tr = now_s();
      for (size_t i = 0; i < in.size(); ++i)
        if (io->read(io->ctx, in[i].rank, in[i].kind, in[i].index, off, len, host + i * slice) != 0)
          return done(fail("stream I/O callback failed"));
      st.read_seconds += now_s() - tr;
      st.bytes_read += static_cast<unsigned long long>(ns) * len;
      const double tg = now_s();
      if (int rc = hip_ok(hipMemcpyAsync(dev, host, stage_in, hipMemcpyHostToDevice, S.stream), "checked rebuild H2D"))
        return done(rc);
      if (int rc = hip_ok(static_cast<hipError_t>(D.reset(S.stream)), "checked rebuild report reset")) return done(rc);
      if (int rc = hip_ok(static_cast<hipError_t>(D.launch(len, off, S.stream)), "gf_rebuild_checked launch"))
        return done(rc);
      if (int rc = hip_ok(hipMemcpyAsync(raw.data(), S.report, report_words * sizeof(unsigned long long),
                                         hipMemcpyDeviceToHost, S.stream),
                          "checked rebuild report copy"))
        return done(rc);
      if (int rc = hip_ok(hipMemcpyAsync(host + stage_in, dev + stage_in, static_cast<size_t>(k) * slice,
                                         hipMemcpyDeviceToHost, S.stream),
                          "checked rebuild D2H"))
        return done(rc);
      if (int rc = hip_ok(hipStreamSynchronize(S.stream), "checked rebuild sync")) return done(rc);
      st.gpu_seconds += now_s() - tg;
      st.units += 1;
      double tw = now_s();
      for (size_t i = 0; i < out.size(); ++i) {
        if (io->write(io->ctx, out[i].rank, out[i].kind, out[i].index, off, len, host + stage_in + i * slice) != 0)
          return done(fail("stream I/O callback failed"));
        sum.cells_written += 1;
      }
      st.write_seconds += now_s() - tw;
      st.bytes_written += static_cast<unsigned long long>(k) * len;
      D.extra(raw.data() + 2 * static_cast<size_t>(p) + 2);
      const unsigned long long un = raw[2 * static_cast<size_t>(p)];
      if (un) {
        finding = true;
        sum.unlocated_columns += un;
        if (stripes) {
          stripes[q].unlocated_columns += un;
          stripes[q].first_unlocated = std::min(stripes[q].first_unlocated, raw[2 * static_cast<size_t>(p) + 1]);
        }
      }
      for (size_t i = 0; i < in.size(); ++i) {
        const size_t mem = static_cast<size_t>(in[i].rank);
        if (raw[mem] == 0) continue;
        finding = true;
        sum.corrected_bytes += raw[mem];
        if (cells) {
          redset_hip_repair_cell& c = cells[static_cast<size_t>(q) * p + mem];
          c.corrected_bytes += raw[mem];
          c.first_offset = std::min(c.first_offset, raw[p + mem]);
        }
        if (!fix_survivors) continue;
        // only this cell, only this slice's range
        if (int rc = hip_ok(hipMemcpy(host + i * slice, dev + i * slice, len, hipMemcpyDeviceToHost), "checked rebuild D2H"))
          return done(rc);
        tw = now_s();
        if (io->write(io->ctx, in[i].rank, in[i].kind, in[i].index, off, len, host + i * slice) != 0)
          return done(fail("stream I/O callback failed"));
        st.write_seconds += now_s() - tw;
        st.bytes_written += len;
        sum.cells_written += 1;
      }
    }
    if (finding) sum.stripes_with_findings += 1;
  }
  return done(REDSET_SUCCESS);
}

// gf_rebuild_checked_kernel<E, K> over rs_check_matrix
struct NarrowDriver : StripeDriver {
  const redset_hip_rs* rs;
  const int* ranks;
  int k, fix;
  std::vector<redset_hip::CheckMatrix> X;
  redset_hip::CheckedLaunch R;
  int prepare(int q, int c) override {
    X.resize(static_cast<size_t>(q) + 1);
    return redset_hip::rs_check_matrix(rs, k, ranks, c, X[static_cast<size_t>(q)]);
  }
  const redset_hip::CheckMatrix& matrix(int q) const override { return X[static_cast<size_t>(q)]; }
  int upload(int q, const std::vector<uint8_t*>& in, const std::vector<uint8_t*>& out, unsigned long long* report,
             void** blob_out) override {
    const redset_hip::CheckMatrix& M = X[static_cast<size_t>(q)];
    const int p = rs->ranks, e = rs->encoding, ns = p - k;
    std::vector<redset_hip::CheckedJobDesc> job(1);
    job[0].in = in;
    job[0].out = out;
    std::vector<int> cols;
    for (int i = 0; i < p; ++i)
      if (std::find(M.lost_cols.begin(), M.lost_cols.end(), i) == M.lost_cols.end()) cols.push_back(i);
    for (int i : cols) job[0].member.push_back(M.cells[static_cast<size_t>(i)].rank);
    for (int j = 0; j < e; ++j)
      for (int i : cols) job[0].coef.push_back(M.M[static_cast<size_t>(j) * p + i]);
    job[0].row = 0;
    std::memset(&R, 0, sizeof(R));
    if (int err = redset_hip::checked_upload(job, ns, e, k, blob_out, &R.jobs)) return err;
    R.njobs = 1;
    R.ns = ns;
    R.e = e;
    R.k = k;
    R.p = p;
    R.fix_survivors = fix;
    R.cell_report = report;
    R.ncells = p;
    R.stripe_report = R.cell_report + 2 * static_cast<size_t>(p);
    R.nstripes = 1;
    return hipSuccess;
  }
  int reset(hipStream_t s) override { return redset_hip::launch_checked_reset(R, s); }
  int launch(size_t len, size_t off, hipStream_t s) override {
    R.nbytes = len;
    R.base = off;
    R.blocks_per_job = redset_hip::checked_blocks_per_job(1, len);
    return redset_hip::launch_checked(R, s);
  }
};

// gf_rebuild_checked_wide_kernel<S> over rs_check_basis_wide
struct WideDriver : StripeDriver {
  const redset_hip_rs* rs;
  const int* ranks;
  int k, fix, max_errors;
  std::vector<redset_hip::CheckBasisWide> B;
  redset_hip::CheckedWideLaunch R;
  unsigned long long multi[redset_hip::kCwMaxT - 1] = {0, 0};
  int prepare(int q, int c) override {
    B.resize(static_cast<size_t>(q) + 1);
    return redset_hip::rs_check_basis_wide(rs, k, ranks, c, B[static_cast<size_t>(q)]);
  }
  const redset_hip::CheckMatrix& matrix(int q) const override { return B[static_cast<size_t>(q)].X; }
  int upload(int q, const std::vector<uint8_t*>& in, const std::vector<uint8_t*>& out, unsigned long long* report,
             void** blob_out) override {
    const int p = rs->ranks, e = rs->encoding, ns = p - k;
    std::vector<redset_hip::CheckedWideJobDesc> job(1);
    redset_hip::checked_wide_job(B[static_cast<size_t>(q)], in, out, 0, job[0]);
    std::memset(&R, 0, sizeof(R));
    if (int err = redset_hip::checked_wide_upload(job, ns, e, k, blob_out, R)) return err;
    R.njobs = 1;
    R.ns = ns;
    R.e = e;
    R.k = k;
    R.p = p;
    R.fix_survivors = fix;
    R.max_errors = max_errors;
    R.cell_report = report;
    R.ncells = p;
    R.stripe_report = R.cell_report + 2 * static_cast<size_t>(p);
    R.multi_report = R.stripe_report + 2;
    R.nstripes = 1;
    return hipSuccess;
  }
  int reset(hipStream_t s) override { return redset_hip::launch_checked_wide_reset(R, s); }
  int launch(size_t len, size_t off, hipStream_t s) override {
    R.nbytes = len;
    R.base = off;
    R.blocks_per_job = redset_hip::checked_blocks_per_job(1, len);
    return redset_hip::launch_checked_wide(R, s);
  }
  void extra(const unsigned long long* words) override {
    for (int i = 0; i < redset_hip::kCwMaxT - 1; ++i) multi[i] += words[i];
  }
};

}  // namespace

extern "C" int redset_hip_rs_rebuild_checked_stream(const redset_hip_rs* rs, int missing, const int* rebuild_ranks,
                                                    size_t chunk_size, int first_stripe, int nstripes,
                                                    size_t slice_bytes, int io_threads, const redset_hip_io* io,
                                                    int fix_survivors, redset_hip_stream_stats* stats,
                                                    redset_hip_repair_cell* cells, int ncells,
                                                    redset_hip_repair_stripe* stripes, int nstripes_out,
                                                    redset_hip_rebuild_checked_summary* summary) {
  (void) io_threads;  // the loop is synchronous
  if (!rs) return fail("null rs state");
  if (!io || !io->read || !io->write) return fail("rebuild_checked_stream: null redset_hip_io (read and write)");
  const int p = rs->ranks, e = rs->encoding, k = missing;
  if (e > redset_hip::kMaxOut)
    return fail("rebuild_checked_stream: encoding %d: the checked rebuild is built for 2..%d parity rows", e,
                redset_hip::kMaxOut);
  if (k == 0) return fail("rebuild_checked_stream: no member is lost (use redset_hip_rs_repair_stream)");
  if (k < 0 || k > e) return fail("rebuild_checked_stream: cannot rebuild %d members with %d parity chunks", k, e);
  if (k == e)
    return fail("rebuild_checked_stream: %d lost members of %d parity rows: nothing left to check (use "
                "redset_hip_rs_rebuild_stream)", k, e);
  NarrowDriver D;
  D.name = "rebuild_checked_stream";
  D.report_words = 2 * static_cast<size_t>(p) + 2;
  D.rs = rs;
  D.ranks = rebuild_ranks;
  D.k = k;
  D.fix = fix_survivors ? 1 : 0;
  return checked_loop(rs, k, chunk_size, first_stripe, nstripes, slice_bytes, io, fix_survivors, stats, cells, ncells,
                      stripes, nstripes_out, summary, D);
}

extern "C" int redset_hip_rs_rebuild_checked_wide_stream(const redset_hip_rs* rs, int missing, const int* rebuild_ranks,
                                                         size_t chunk_size, int first_stripe, int nstripes,
                                                         size_t slice_bytes, int io_threads, const redset_hip_io* io,
                                                         int fix_survivors, int max_errors,
                                                         redset_hip_stream_stats* stats, redset_hip_repair_cell* cells,
                                                         int ncells, redset_hip_repair_stripe* stripes,
                                                         int nstripes_out, redset_hip_rebuild_checked_summary* summary,
                                                         unsigned long long* multi_columns_out) {
  (void) io_threads;  // the loop is synchronous
  if (!rs) return fail("null rs state");
  if (!io || !io->read || !io->write) return fail("rebuild_checked_wide_stream: null redset_hip_io (read and write)");
  const int p = rs->ranks, e = rs->encoding, k = missing, s = e - k;
  if (e < redset_hip::kWideMinE || e > redset_hip::kWideMaxE)
    return fail("rebuild_checked_wide_stream: encoding %d: the wide checked rebuild is built for %d..%d parity rows", e,
                redset_hip::kWideMinE, redset_hip::kWideMaxE);
  if (k == 0) return fail("rebuild_checked_wide_stream: no member is lost (use redset_hip_rs_repair_wide_stream)");
  if (k < 0 || k > e) return fail("rebuild_checked_wide_stream: cannot rebuild %d members with %d parity chunks", k, e);
  if (k == e)
    return fail("rebuild_checked_wide_stream: %d lost members of %d parity rows: nothing left to check (use "
                "redset_hip_rs_rebuild_stream)", k, e);
  if (max_errors < std::min(1, s / 2) || max_errors > s / 2)
    return fail("rebuild_checked_wide_stream: max_errors %d: %d spare rows locate %d..%d wrong bytes per column",
                max_errors, s, std::min(1, s / 2), s / 2);
  if (int rc = hip_ok(static_cast<hipError_t>(redset_hip::checked_wide_prepare(p - k, s)),
                      "wide checked rebuild LDS attribute"))
    return rc;
  WideDriver D;
  D.name = "rebuild_checked_wide_stream";
  D.report_words = 2 * static_cast<size_t>(p) + 2 + (redset_hip::kCwMaxT - 1);
  D.rs = rs;
  D.ranks = rebuild_ranks;
  D.k = k;
  D.fix = fix_survivors ? 1 : 0;
  D.max_errors = max_errors;
  const int rc = checked_loop(rs, k, chunk_size, first_stripe, nstripes, slice_bytes, io, fix_survivors, stats, cells,
                              ncells, stripes, nstripes_out, summary, D);
  for (int i = 0; multi_columns_out && i < redset_hip::kCwMaxT - 1; ++i) multi_columns_out[i] = D.multi[i];
  return rc;
}
