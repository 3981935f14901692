// rebuild_checked_stream.cpp -- errors-and-erasures rebuild of a host-resident
// set (memory or files) through the redset_hip_io callbacks
// (include/redset_hip.h, redset_hip_rs_rebuild_checked_stream).
//
// A synchronous loop in the manner of repair_stream.cpp step 2: every stripe
// goes slice by slice through read (survivors) -> H2D ->
// gf_rebuild_checked_kernel -> report and D2H of the k rebuilt slices ->
// write, plus (fix_survivors) D2H and write of the survivor cells corrected
// in that slice. Staging memory is allocated per call and freed on return.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "codec_kernels.h"
#include "rebuild_checked.h"
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
  const int p = rs->ranks, e = rs->encoding, k = missing, ns = p - k;
  if (e > redset_hip::kMaxOut)
    return fail("rebuild_checked_stream: encoding %d: the checked rebuild is built for 2..%d parity rows", e,
                redset_hip::kMaxOut);
  if (k == 0) return fail("rebuild_checked_stream: no member is lost (use redset_hip_rs_repair_stream)");
  if (k < 0 || k > e) return fail("rebuild_checked_stream: cannot rebuild %d members with %d parity chunks", k, e);
  if (k == e)
    return fail("rebuild_checked_stream: %d lost members of %d parity rows: nothing left to check (use "
                "redset_hip_rs_rebuild_stream)", k, e);
  if (nstripes <= 0) {
    first_stripe = 0;
    nstripes = p;
  }
  if (first_stripe < 0 || first_stripe + nstripes > p)
    return fail("stripe range [%d, %d) outside 0..%d", first_stripe, first_stripe + nstripes, p);
  const int lo = first_stripe, n = nstripes;
  if (cells && ncells < n * p)
    return fail("rebuild_checked_stream: room for %d cells, the call reports %d", ncells, n * p);
  if (stripes && nstripes_out < n)
    return fail("rebuild_checked_stream: room for %d stripes, the call reports %d", nstripes_out, n);
  // every stripe's matrix first: bad ranks are refused before anything is read
  std::vector<redset_hip::CheckMatrix> X(static_cast<size_t>(n));
  for (int q = 0; q < n; ++q)
    if (int rc = redset_hip::rs_check_matrix(rs, k, rebuild_ranks, lo + q, X[static_cast<size_t>(q)])) return rc;
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
  const size_t report_words = 2 * static_cast<size_t>(p) + 2;
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
    const redset_hip::CheckMatrix& M = X[static_cast<size_t>(q)];
    std::vector<CellRef> in, out;
    std::vector<redset_hip::CheckedJobDesc> job(1);
    for (int i = 0; i < p; ++i) {
      if (std::find(M.lost_cols.begin(), M.lost_cols.end(), i) != M.lost_cols.end()) continue;
      job[0].in.push_back(dev + in.size() * slice);
      job[0].member.push_back(M.cells[static_cast<size_t>(i)].rank);
      in.push_back(M.cells[static_cast<size_t>(i)]);
    }
    for (int i : M.lost_cols) {
      job[0].out.push_back(dev + (static_cast<size_t>(ns) + out.size()) * slice);
      out.push_back(M.cells[static_cast<size_t>(i)]);
    }
    for (int j = 0; j < e; ++j)
      for (int i = 0; i < p; ++i)
        if (std::find(M.lost_cols.begin(), M.lost_cols.end(), i) == M.lost_cols.end())
          job[0].coef.push_back(M.M[static_cast<size_t>(j) * p + i]);
    job[0].row = 0;
    redset_hip::CheckedLaunch R;
    std::memset(&R, 0, sizeof(R));
    if (S.blob) (void) hipFree(S.blob);
    S.blob = nullptr;
    if (int rc = hip_ok(static_cast<hipError_t>(redset_hip::checked_upload(job, ns, e, k, &S.blob, &R.jobs)),
                        "checked rebuild job upload"))
      return done(rc);
    R.njobs = 1;
    R.ns = ns;
    R.e = e;
    R.k = k;
    R.p = p;
    R.fix_survivors = fix_survivors ? 1 : 0;
    R.cell_report = static_cast<unsigned long long*>(S.report);
    R.ncells = p;
    R.stripe_report = R.cell_report + 2 * static_cast<size_t>(p);
    R.nstripes = 1;
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
      R.nbytes = len;
      R.base = off;
      R.blocks_per_job = redset_hip::checked_blocks_per_job(1, len);
      if (int rc = hip_ok(static_cast<hipError_t>(redset_hip::launch_checked_reset(R, S.stream)),
                          "checked rebuild report reset"))
        return done(rc);
      if (int rc = hip_ok(static_cast<hipError_t>(redset_hip::launch_checked(R, S.stream)), "gf_rebuild_checked launch"))
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
