// repair_stream.cpp -- column-wise repair of a host-resident set (memory or
// files) through the redset_hip_io callbacks (include/redset_hip.h,
// redset_hip_rs_repair_stream).
//
// Damage is rare, so this is not a pipeline: the existing verify stream finds
// the damaged stripes (a clean set ends there, at today's cost), and every
// damaged stripe then goes slice by slice, synchronously, through read ->
// H2D -> gf_repair_kernel -> report -> (apply) D2H and write of the corrected
// cells only. Staging memory is allocated per call and freed on return.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "codec_kernels.h"
#include "redset_hip.h"
#include "repair.h"
#include "stripe_map.h"

using redset_hip::CellRef;
using redset_hip::fail;
using redset_hip::StripeMap;

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

extern "C" int redset_hip_rs_repair_stream(const redset_hip_rs* rs, size_t chunk_size, int first_stripe, int nstripes,
                                           size_t slice_bytes, int io_threads, const redset_hip_io* io, int apply,
                                           redset_hip_stream_stats* stats, redset_hip_repair_cell* cells, int ncells,
                                           redset_hip_repair_stripe* stripes, int nstripes_out,
                                           redset_hip_repair_summary* summary) {
  if (!rs) return fail("null rs state");
  if (!io || !io->read) return fail("null redset_hip_io");
  if (apply && !io->write) return fail("repair_stream: apply needs io->write");
  const int p = rs->ranks, e = rs->encoding;
  if (e < 2)
    return fail("repair_stream: encoding %d: one parity row locates nothing (rebuild the member a checksum names)", e);
  if (e > redset_hip::kMaxOut)
    return fail("repair_stream: encoding %d: repair is built for 2..%d parity rows", e, redset_hip::kMaxOut);
  if (nstripes <= 0) {
    first_stripe = 0;
    nstripes = p;
  }
  if (first_stripe < 0 || first_stripe + nstripes > p)
    return fail("stripe range [%d, %d) outside 0..%d", first_stripe, first_stripe + nstripes, p);
  const int lo = first_stripe, n = nstripes;
  if (cells && ncells < n * p) return fail("repair_stream: room for %d cells, the call reports %d", ncells, n * p);
  if (stripes && nstripes_out < n)
    return fail("repair_stream: room for %d stripes, the call reports %d", nstripes_out, n);
  for (int i = 0; cells && i < n * p; ++i) cells[i] = redset_hip_repair_cell{0, ~0ull};
  for (int i = 0; stripes && i < n; ++i) stripes[i] = redset_hip_repair_stripe{0, ~0ull};
  redset_hip_repair_summary sum;
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

  // 1. the scrub as it is
  std::vector<redset_hip_verify_row> rows(static_cast<size_t>(n) * e);
  if (int rc = redset_hip_rs_verify_stream(rs, chunk_size, lo, n, slice_bytes, io_threads, io, &st, rows.data(), n * e))
    return done(rc);
  std::vector<int> damaged;
  for (int k = 0; k < n; ++k) {
    unsigned long long m = 0;
    for (int i = 0; i < e; ++i) m += rows[static_cast<size_t>(k) * e + i].mismatch_bytes;
    sum.verify_mismatch_bytes += m;
    if (m) damaged.push_back(lo + k);
  }
  sum.remaining_mismatch_bytes = sum.verify_mismatch_bytes;
  sum.damaged_stripes = static_cast<int>(damaged.size());
  if (damaged.empty()) return done(REDSET_SUCCESS);

  // 2. the damaged stripes, slice by slice (the verify stream's slice rule)
  const size_t chunk = chunk_size;
  size_t slice = slice_bytes;
  if (slice == 0) slice = chunk > (8u << 20) ? (8u << 20) : std::max<size_t>(256u << 10, chunk / 16);
  slice = std::min(slice, std::max<size_t>(chunk, 1));
  slice = (slice + 255) & ~static_cast<size_t>(255);
  Staging S;
  const size_t stage = static_cast<size_t>(p) * slice;
  const size_t report_words = 2 * static_cast<size_t>(p) + 2;
  if (int rc = hip_ok(hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking), "hipStreamCreate")) return done(rc);
  if (int rc = hip_ok(hipHostMalloc(&S.host, stage, hipHostMallocDefault), "hipHostMalloc(repair staging)")) return done(rc);
  if (int rc = hip_ok(hipMalloc(&S.dev, stage), "hipMalloc(repair staging)")) return done(rc);
  if (int rc = hip_ok(hipMalloc(&S.report, report_words * sizeof(unsigned long long)), "hipMalloc(repair report)"))
    return done(rc);
  uint8_t* const host = static_cast<uint8_t*>(S.host);
  uint8_t* const dev = static_cast<uint8_t*>(S.dev);
  std::vector<unsigned long long> raw(report_words);
  for (int c : damaged) {
    StripeMap m;
    redset_hip::rs_verify_map(rs, c, m);
    std::vector<CellRef> ref(m.in);
    ref.insert(ref.end(), m.out.begin(), m.out.end());
    // staging cell i holds ref[i]: the data cells, then the parity rows
    std::vector<redset_hip::RepairJobDesc> job(1);
    for (size_t i = 0; i < ref.size(); ++i) {
      (i < m.in.size() ? job[0].data : job[0].parity).push_back(dev + i * slice);
      job[0].member.push_back(ref[i].rank);
    }
    job[0].coef = m.coef;
    job[0].row = 0;
    redset_hip::RepairLaunch R;
    std::memset(&R, 0, sizeof(R));
    if (S.blob) (void) hipFree(S.blob);
    S.blob = nullptr;
    if (int rc = hip_ok(static_cast<hipError_t>(redset_hip::repair_upload(job, p - e, e, &S.blob, &R.jobs)),
                        "repair job upload"))
      return done(rc);
    R.njobs = 1;
    R.d = p - e;
    R.e = e;
    R.p = p;
    R.apply = apply ? 1 : 0;
    R.cell_report = static_cast<unsigned long long*>(S.report);
    R.ncells = p;
    R.stripe_report = R.cell_report + 2 * static_cast<size_t>(p);
    R.nstripes = 1;
    for (size_t off = 0; off < chunk; off += slice) {
      const size_t len = std::min(slice, chunk - off);
      const double tr = now_s();
      for (size_t i = 0; i < ref.size(); ++i)
        if (io->read(io->ctx, ref[i].rank, ref[i].kind, ref[i].index, off, len, host + i * slice) != 0)
          return done(fail("stream I/O callback failed"));
      st.read_seconds += now_s() - tr;
      st.bytes_read += static_cast<unsigned long long>(ref.size()) * len;
      const double tg = now_s();
      if (int rc = hip_ok(hipMemcpyAsync(dev, host, stage, hipMemcpyHostToDevice, S.stream), "repair H2D")) return done(rc);
      R.nbytes = len;
      R.base = off;
      R.blocks_per_job = redset_hip::repair_blocks_per_job(1, len);
      if (int rc = hip_ok(static_cast<hipError_t>(redset_hip::launch_repair_reset(R, S.stream)), "repair report reset"))
        return done(rc);
      if (int rc = hip_ok(static_cast<hipError_t>(redset_hip::launch_repair(R, S.stream)), "gf_repair launch")) return done(rc);
      if (int rc = hip_ok(hipMemcpyAsync(raw.data(), S.report, report_words * sizeof(unsigned long long),
                                         hipMemcpyDeviceToHost, S.stream),
                          "repair report copy"))
        return done(rc);
      if (int rc = hip_ok(hipStreamSynchronize(S.stream), "repair sync")) return done(rc);
      st.gpu_seconds += now_s() - tg;
      sum.repair_units += 1;
      st.units += 1;
      const size_t k = static_cast<size_t>(c - lo);
      sum.unlocated_columns += raw[2 * static_cast<size_t>(p)];
      if (stripes && raw[2 * static_cast<size_t>(p)]) {
        stripes[k].unlocated_columns += raw[2 * static_cast<size_t>(p)];
        stripes[k].first_unlocated = std::min(stripes[k].first_unlocated, raw[2 * static_cast<size_t>(p) + 1]);
      }
      for (size_t i = 0; i < ref.size(); ++i) {
        const size_t mem = static_cast<size_t>(ref[i].rank);
        if (raw[mem] == 0) continue;
        sum.corrected_bytes += raw[mem];
        if (cells) {
          cells[k * p + mem].corrected_bytes += raw[mem];
          cells[k * p + mem].first_offset = std::min(cells[k * p + mem].first_offset, raw[p + mem]);
        }
        if (!apply) continue;
        // only this cell, only this slice's range
        if (int rc = hip_ok(hipMemcpy(host + i * slice, dev + i * slice, len, hipMemcpyDeviceToHost), "repair D2H"))
          return done(rc);
        const double tw = now_s();
        if (io->write(io->ctx, ref[i].rank, ref[i].kind, ref[i].index, off, len, host + i * slice) != 0)
          return done(fail("stream I/O callback failed"));
        st.write_seconds += now_s() - tw;
        st.bytes_written += len;
        sum.cells_written += 1;
      }
    }
  }

  // 3. the check kernels again over the repaired stripes
  if (apply) {
    sum.remaining_mismatch_bytes = 0;
    redset_hip_stream_stats again;
    for (int c : damaged) {
      if (int rc = redset_hip_rs_verify_stream(rs, chunk_size, c, 1, slice_bytes, io_threads, io, &again, rows.data(), e))
        return done(rc);
      for (int i = 0; i < e; ++i) sum.remaining_mismatch_bytes += rows[static_cast<size_t>(i)].mismatch_bytes;
      st.bytes_read += again.bytes_read;
      st.units += again.units;
    }
  }
  return done(REDSET_SUCCESS);
}
