// redset_hip.cpp -- C ABI (include/redset_hip.h): GF state, whole-set plans
// for RS / XOR encode and rebuild, and stripe primitives.
//
// A plan turns the reference's per-rank, per-slice loops (encode:
// src/redset_reedsolomon.c:309-391, decode: :631-768, XOR: src/redset_xor.c:
// 243-288, src/redset_xor_serial.c:202-273) into a few kernel launches over
// whole cells: one job per stripe, each reading its input cells once and
// writing its output cells once. Planning happens once on the host; execute
// only enqueues kernels, so it can be captured into a hipGraph.
#include "redset_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <tuple>
#include <vector>

#include "codec_kernels.h"
#include "crc32.h"
#include "gf256.h"
#include "rebuild_checked.h"
#include "repair.h"
#include "stripe_map.h"

using redset_hip::CellRef;
using redset_hip::fail;
using redset_hip::GfCheckLaunch;
using redset_hip::GfJob;
using redset_hip::GfLaunch;
using redset_hip::kMaxIn;
using redset_hip::kMaxOut;
using redset_hip::StripeMap;
using redset_hip::XorCheckLaunch;
using redset_hip::XorJob;
using redset_hip::XorLaunch;

// widest stripe primitive call: p + e <= 256 bounds any redset stripe
constexpr int kMaxCombine = 256;

struct redset_hip_plan {
  redset_hip_plan_info info{};
  GfJob* d_gf = nullptr;  // device job arrays
  XorJob* d_xor = nullptr;
  unsigned* d_claim = nullptr;  // kJobsClaimed launches' queue counters
  std::vector<GfLaunch> gf_launches;
  std::vector<XorLaunch> xor_launches;
  // verify plans (REDSET_HIP_PLAN_*_VERIFY): fused check launches over the
  // device job arrays above, or wide stripes run one after another through
  // the scratch; the report all of them add to; what locate needs
  std::vector<redset_hip::GfCheckLaunch> gf_checks;
  std::vector<redset_hip::XorCheckLaunch> xor_checks;
  struct WideStripe {
    StripeMap map;
    std::vector<const uint8_t*> in, stored;
    int row0;
  };
  std::vector<WideStripe> wide;
  unsigned long long* d_report = nullptr;  // report_rows counts, then report_rows first offsets
  int report_rows = 0;
  uint8_t* d_scratch = nullptr;
  std::vector<uint8_t> mat;             // RS: the encoding matrix
  std::vector<const uint8_t*> cells;    // [stripe * p + member]: that member's cell of the stripe
  // CRC plans (REDSET_HIP_PLAN_CRC32): the launch over the plan's device
  // tables (ranges, tile numbering, one remainder per tile, the CRCs)
  redset_hip::CrcLaunch crc{};
  void* d_crc = nullptr;
  // repair plans (REDSET_HIP_PLAN_RS_REPAIR): the launch over the plan's
  // device job blob, and both reports in one allocation
  redset_hip::RepairLaunch repair{};
  void* d_repair = nullptr;
  unsigned long long* d_repair_report = nullptr;
  // checked rebuild plans (REDSET_HIP_PLAN_RS_REBUILD_CHECKED): the same
  redset_hip::CheckedLaunch checked{};
  void* d_checked = nullptr;
  unsigned long long* d_checked_report = nullptr;
};

namespace {

int hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return REDSET_SUCCESS;
  return fail("%s: %s", what, hipGetErrorString(e));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Test builds only (REDSET_HIP_TEST_KNOBS, codec_kernels.h): an environment
// override of a planning choice; the product library always takes `dflt`.
// Read at every plan build.
int test_knob(const char* name, int dflt) {
#if REDSET_HIP_TEST_KNOBS
  const char* s = std::getenv(name);
  if (s && s[0] >= '0' && s[0] <= '9') return std::atoi(s);
#else
  (void) name;
#endif
  return dflt;
}

// Resident blocks per CU the codec aims for: one block of the ring's 1024
// threads (1 loader + 15 consumer waves, codec_kernels.h), alone on the CU
// (it takes 146 KiB of LDS).
int target_blocks_per_cu(int occupancy) { return std::max(1, std::min(1, occupancy)); }

// Resident XOR blocks per CU: one, as for gf_mac (the ring's block fills the
// CU's LDS; with the per-wave sweep before it, one 256-thread block per CU
// also beat two, profiles/r01_ab_xor_blocks.txt).
int xor_blocks_cap() { return 1; }

// Job order of a plan's launches (codec_kernels.h). Stripes in sequence, one
// launch each over the whole grid (kJobsInLaunches), keep one stripe's ~11
// cell streams in flight instead of every stripe's ~120: +6.5% on the 64 MiB
// RS(8+3) step; two or three stripes per launch cost 3% / 6%, and one launch
// looping over the stripes (kJobsInKernel) 5% (profiles/r01_sequential_jobs.txt).
// Each launch pays a ramp-up and a drain, so sequence only pays for big cells:
// side by side wins at 16 MiB cells (5.30 vs 5.14 TB/s), sequence at 24 MiB
// (5.43 vs 5.16) and 32 MiB (5.46 vs 5.11); grouping 2-6 stripes per launch
// never beats both (profiles/r01_sequential_jobs.txt, cell-size sweeps). Sets
// with smaller cells keep their stripes side by side in one launch (0).
// Round 3, with the loader ring: GF stripes of <= 8 inputs over whole 16-B
// vectors (RS(8+3) encode and rebuild) run all in ONE launch whose blocks
// claim their items at run time (kJobsClaimed, codec_device.h
// gf_mac_claimed): one continuous loader ring per block over all the
// stripes, the blocks of each XCD sweeping its rows together, so no launch
// gaps, one tail per set instead of per stripe, and no drift between blocks:
// +3.5% on the RS(8+3) step against one launch per stripe, +1.5% against
// streamed pairs. Streamed (kJobsStreamed, static items) pays off only in
// pairs (+1.5..2.5%): with more stripes per launch the blocks drift apart
// and sweep different stripes at once (all 11: -3.5%); it stays the order of
// XOR A/B runs (profiles/r03_ab_stream.txt).
// Test builds: REDSET_HIP_SEQUENTIAL=0..4 forces an order (XOR launches take
// 1 for 4); REDSET_HIP_STREAM_JOBS sets the stripes per streamed or claimed
// launch (0 = all), REDSET_HIP_STRIPES_PER_LAUNCH those side by side per
// launch in sequence mode.
constexpr size_t kSequentialMinCell = 24u << 20;

// can_stream: the kernel has a streamed path for these jobs (GF: <= 8
// inputs, XOR: <= 8 inputs, both over whole 16-B vectors); can_claim: a
// claimed one (the same jobs: GF and XOR of <= 8 inputs over whole 16-B
// vectors; XOR claiming is off by default, xor_claim_default);
// claim_default / stream_default: which is the default for big cells.
int sequential_jobs(int njobs, size_t nbytes, bool can_stream, bool can_claim, bool claim_default,
                     bool stream_default) {
  if (njobs < 2) return 0;
  int order = nbytes >= kSequentialMinCell
                  ? (can_claim && claim_default ? redset_hip::kJobsClaimed
                     : can_stream && stream_default ? redset_hip::kJobsStreamed
                                                    : redset_hip::kJobsInLaunches)
                  : 0;
  const int forced = test_knob("REDSET_HIP_SEQUENTIAL", -1);
  if (forced >= 0 && forced <= 4) order = forced;
  if ((order == redset_hip::kJobsStreamed && !can_stream) || (order == redset_hip::kJobsClaimed && !can_claim))
    order = redset_hip::kJobsInLaunches;
  return order;
}

// Stripes per launch: in sequence mode side by side within the launch
// (default 1); streamed, two stripes one after another through the ring;
// claimed, the whole set in one launch (0 = all).
int stripes_per_launch(int order) {
  if (order == redset_hip::kJobsStreamed || order == redset_hip::kJobsClaimed)
    return test_knob("REDSET_HIP_STREAM_JOBS", order == redset_hip::kJobsClaimed ? 0 : 2);
  return std::max(1, test_knob("REDSET_HIP_STRIPES_PER_LAUNCH", 1));
}

// XOR plans keep a launch per stripe: streamed pairs (xor_stream) measured
// within the XOR leg's run-to-run spread, 6.26 against 6.30 TB/s over three
// alternating pairs (profiles/r03_ab_stream.txt). Test builds:
// REDSET_HIP_XOR_STREAM=1 streams them in pairs.
bool xor_stream_default() { return test_knob("REDSET_HIP_XOR_STREAM", 0) == 1; }

// XOR plans with claimed items (claimed_sweep, one launch per set): a measured
// negative, kept as a twin-only order (REDSET_HIP_XOR_CLAIM=1 or
// REDSET_HIP_SEQUENTIAL=4) the suite checks bit for bit: the XOR leg 5.60
// against 5.98-6.09 TB/s. Its one-row items and claim bookkeeping cost +27%
// SALU, +44% VALU and +54% LDS instructions per byte at equal HBM traffic,
// and with consumers this light the loader's per-item instruction stream sets
// the pace (profiles/r04s5_ab_xor_claim.txt, r04s6_xor_claim_pmc_sq.txt)
bool xor_claim_default() { return test_knob("REDSET_HIP_XOR_CLAIM", 0) == 1; }

int launches_of(int order, int njobs, int group) {
  if (order == redset_hip::kJobsStreamed || order == redset_hip::kJobsClaimed)
    return group > 0 ? (njobs + group - 1) / group : 1;
  return order == redset_hip::kJobsInLaunches ? (njobs + group - 1) / group : 1;
}

// jobs that share one launch's grid
int jobs_sharing_grid(int order, int njobs, int group) {
  return order == redset_hip::kJobsInLaunches                                            ? std::min(group, njobs)
         : (order == redset_hip::kJobsInKernel || order == redset_hip::kJobsStreamed ||
            order == redset_hip::kJobsClaimed)
             ? 1
                                                                                       : njobs;
}

// Blocks per job so the whole launch fits in one resident wave of blocks.
int blocks_per_job(int njobs, size_t nbytes, int occupancy, int blocks_total = 0) {
  const long target = blocks_total > 0
                          ? blocks_total
                          : static_cast<long>(redset_hip::device_cu_count()) * target_blocks_per_cu(occupancy);
  long bpj = std::max<long>(1, target / std::max(1, njobs));
  // at least one 16-B vector per thread per block
  const long vec_blocks = static_cast<long>((nbytes / 16 + redset_hip::kBlock - 1) / redset_hip::kBlock);
  bpj = std::min(bpj, std::max<long>(1, vec_blocks));
  return static_cast<int>(bpj);
}

// Device address of a cell in the set layout of include/redset_hip.h.
struct SetLayout {
  unsigned char* const* lofi;
  unsigned char* const* parity;
  size_t stride;
  uint8_t* at(const CellRef& c) const {
    return (c.kind == redset_hip::kData ? lofi[c.rank] : parity[c.rank]) + static_cast<size_t>(c.index) * stride;
  }
};

// Split stripe maps into launches of <= kMaxIn inputs x <= kMaxOut outputs.
// Output groups are independent; input groups of one output group run in
// order, the first overwriting and the rest accumulating. Jobs with equal
// shapes share a launch. XOR maps go to the XOR kernel.
int build_plan(redset_hip_plan* plan, const std::vector<StripeMap>& maps, const SetLayout& L, size_t nbytes) {
  struct GfPending {
    std::vector<GfJob> jobs;
    int nin, nout, accumulate, bytes_only;
  };
  struct XorPending {
    std::vector<XorJob> jobs;
    int nin, accumulate, bytes_only;
  };
  // (input group, nin, nout, unaligned, accumulate) / (input group, nin, unaligned, accumulate)
  std::map<std::tuple<int, int, int, int, int>, GfPending> gf;
  std::map<std::tuple<int, int, int, int>, XorPending> xr;
  unsigned long long rd = 0, wr = 0;
  for (const StripeMap& m : maps) {
    const int nin = static_cast<int>(m.in.size());
    const int nt = static_cast<int>(m.out.size());
    if (nt == 0) continue;
    if (nin == 0) return fail("stripe with outputs but no inputs");
    for (int og = 0; og * kMaxOut < nt; ++og) {
      const int o0 = og * kMaxOut, no = std::min(kMaxOut, nt - o0);
      if (m.xor_only && no != 1) return fail("XOR stripe with %d outputs", no);
      for (int ig = 0; ig * kMaxIn < nin; ++ig) {
        const int i0 = ig * kMaxIn, ni = std::min(kMaxIn, nin - i0);
        bool al = true;
        const int acc = ig > 0 || m.accumulate;
        rd += static_cast<unsigned long long>(ni + (acc ? no : 0)) * nbytes;
        wr += static_cast<unsigned long long>(no) * nbytes;
        if (m.xor_only) {
          XorJob J;
          std::memset(&J, 0, sizeof(J));
          for (int i = 0; i < ni; ++i) {
            J.in[i] = L.at(m.in[i0 + i]);
            al = al && aligned16(J.in[i]);
          }
          J.out = L.at(m.out[o0]);
          al = al && aligned16(J.out);
          XorPending& P = xr[std::make_tuple(ig, ni, al ? 0 : 1, acc)];
          P.nin = ni;
          P.accumulate = acc;
          P.bytes_only = al ? 0 : 1;
          P.jobs.push_back(J);
          continue;
        }
        GfJob J;
        std::memset(&J, 0, sizeof(J));
        for (int i = 0; i < ni; ++i) {
          J.in[i] = L.at(m.in[i0 + i]);
          al = al && aligned16(J.in[i]);
        }
        for (int j = 0; j < no; ++j) {
          J.out[j] = L.at(m.out[o0 + j]);
          al = al && aligned16(J.out[j]);
          for (int i = 0; i < ni; ++i) J.coef[j][i] = m.coef[static_cast<size_t>(o0 + j) * nin + i0 + i];
        }
        GfPending& P = gf[std::make_tuple(ig, ni, no, al ? 0 : 1, acc)];
        P.nin = ni;
        P.nout = no;
        P.accumulate = acc;
        P.bytes_only = al ? 0 : 1;
        P.jobs.push_back(J);
      }
    }
  }
  plan->info.bytes_read = rd;
  plan->info.bytes_written = wr;
  std::vector<GfJob> gall;
  std::vector<XorJob> xall;
  for (auto& kv : gf) {
    GfPending& P = kv.second;
    GfLaunch G;
    std::memset(&G, 0, sizeof(G));
    G.jobs = reinterpret_cast<const GfJob*>(gall.size());  // offset, patched below
    G.njobs = static_cast<int>(P.jobs.size());
    G.nin = P.nin;
    G.nout = P.nout;
    G.accumulate = P.accumulate;
    G.bytes_only = P.bytes_only;
    G.nbytes = nbytes;
    const bool whole = P.nin <= 8 && !P.bytes_only && nbytes % 16 == 0;
    // claimed items for 3-4 outputs (the RS(8+3) encode: 6.45-6.47 TB/s against
    // 6.22-6.27 streamed in pairs on two boxes); pairs for 1-2 (the rebuild:
    // 6.35-6.41 against 5.99-6.33 claimed; its lighter consumers leave the
    // loader, whose per-item cost the claimed order raises, setting the pace)
    G.sequential = sequential_jobs(G.njobs, nbytes, whole, whole, P.nout >= 3, true);
    G.group = stripes_per_launch(G.sequential);
    G.blocks_per_job = blocks_per_job(jobs_sharing_grid(G.sequential, G.njobs, G.group), nbytes,
                                      redset_hip::gf_blocks_per_cu(P.nin));
    gall.insert(gall.end(), P.jobs.begin(), P.jobs.end());
    plan->gf_launches.push_back(G);
  }
  for (auto& kv : xr) {
    XorPending& P = kv.second;
    XorLaunch X;
    std::memset(&X, 0, sizeof(X));
    X.jobs = reinterpret_cast<const XorJob*>(xall.size());
    X.njobs = static_cast<int>(P.jobs.size());
    X.nin = P.nin;
    X.accumulate = P.accumulate;
    X.bytes_only = P.bytes_only;
    X.nbytes = nbytes;
    const bool whole = P.nin <= 8 && !P.bytes_only && nbytes % 16 == 0;
    X.sequential = sequential_jobs(X.njobs, nbytes, whole, whole, xor_claim_default(), xor_stream_default());
    X.group = stripes_per_launch(X.sequential);
    X.blocks_per_job = blocks_per_job(jobs_sharing_grid(X.sequential, X.njobs, X.group), nbytes, xor_blocks_cap());
    xall.insert(xall.end(), P.jobs.begin(), P.jobs.end());
    plan->xor_launches.push_back(X);
  }
  plan->info.jobs = static_cast<int>(gall.size() + xall.size());
  plan->info.launches = 0;
  for (const GfLaunch& G : plan->gf_launches) plan->info.launches += launches_of(G.sequential, G.njobs, G.group);
  for (const XorLaunch& X : plan->xor_launches) plan->info.launches += launches_of(X.sequential, X.njobs, X.group);
  if (!gall.empty()) {
    if (int rc = hip_check(hipMalloc(&plan->d_gf, gall.size() * sizeof(GfJob)), "hipMalloc(plan jobs)")) return rc;
    if (int rc = hip_check(hipMemcpy(plan->d_gf, gall.data(), gall.size() * sizeof(GfJob), hipMemcpyHostToDevice),
                           "hipMemcpy(plan jobs)"))
      return rc;
    for (GfLaunch& G : plan->gf_launches) G.jobs = plan->d_gf + reinterpret_cast<uintptr_t>(G.jobs);
  }
  // claimed launches (the kernel takes them over whole 16-B vectors and <= 8
  // inputs only, as the streamed ones): their queue counters, zeroed
  size_t nclaim = 0;
  for (GfLaunch& G : plan->gf_launches)
    if (G.sequential == redset_hip::kJobsClaimed) ++nclaim;
  for (XorLaunch& X : plan->xor_launches)
    if (X.sequential == redset_hip::kJobsClaimed) ++nclaim;
  if (nclaim > 0) {
    const size_t bytes = nclaim * redset_hip::kClaimWords * sizeof(unsigned);
    if (int rc = hip_check(hipMalloc(&plan->d_claim, bytes), "hipMalloc(claim queues)")) return rc;
    if (int rc = hip_check(hipMemset(plan->d_claim, 0, bytes), "hipMemset(claim queues)")) return rc;
    size_t k = 0;
    for (GfLaunch& G : plan->gf_launches)
      if (G.sequential == redset_hip::kJobsClaimed) G.claim = plan->d_claim + (k++) * redset_hip::kClaimWords;
    for (XorLaunch& X : plan->xor_launches)
      if (X.sequential == redset_hip::kJobsClaimed) X.claim = plan->d_claim + (k++) * redset_hip::kClaimWords;
  }
  if (!xall.empty()) {
    if (int rc = hip_check(hipMalloc(&plan->d_xor, xall.size() * sizeof(XorJob)), "hipMalloc(plan jobs)")) return rc;
    if (int rc = hip_check(hipMemcpy(plan->d_xor, xall.data(), xall.size() * sizeof(XorJob), hipMemcpyHostToDevice),
                           "hipMemcpy(plan jobs)"))
      return rc;
    for (XorLaunch& X : plan->xor_launches) X.jobs = plan->d_xor + reinterpret_cast<uintptr_t>(X.jobs);
  }
  return REDSET_SUCCESS;
}

int check_set_args(const void* const* a, const void* const* b, int ranks, size_t chunk_size, size_t stride,
                   redset_hip_plan** out) {
  if (!out) return fail("null plan out-pointer");
  *out = nullptr;
  if (!a || !b) return fail("null member pointer array");
  for (int r = 0; r < ranks; ++r)
    if (!a[r] || !b[r]) return fail("null device pointer for member %d", r);
  if (stride < chunk_size) return fail("cell_stride (%zu) < chunk_size (%zu)", stride, chunk_size);
  return REDSET_SUCCESS;
}

int finish_plan(int kind, int ranks, int encoding, int missing, size_t chunk, const std::vector<StripeMap>& maps,
                const SetLayout& L, redset_hip_plan** out) {
  redset_hip_plan* plan = new (std::nothrow) redset_hip_plan;
  if (!plan) return fail("out of host memory");
  plan->info.kind = kind;
  plan->info.ranks = ranks;
  plan->info.encoding = encoding;
  plan->info.missing = missing;
  plan->info.chunk_size = chunk;
  if (int rc = build_plan(plan, maps, L, chunk)) {
    redset_hip_plan_destroy(plan);
    return rc;
  }
  *out = plan;
  return REDSET_SUCCESS;
}

}  // namespace

namespace redset_hip {

int run_stripe(const StripeMap& m, const uint8_t* const* in, uint8_t* const* out, size_t nbytes, void* stream,
               int blocks_total, bool accumulate) {
  const int nin = static_cast<int>(m.in.size()), nt = static_cast<int>(m.out.size());
  for (int og = 0; og * kMaxOut < nt; ++og) {
    const int o0 = og * kMaxOut, no = std::min(kMaxOut, nt - o0);
    for (int ig = 0; ig * kMaxIn < nin; ++ig) {
      const int i0 = ig * kMaxIn, ni = std::min(kMaxIn, nin - i0);
      bool al = true;
      int e;
      if (m.xor_only) {
        XorJob J;
        std::memset(&J, 0, sizeof(J));
        for (int i = 0; i < ni; ++i) {
          J.in[i] = in[i0 + i];
          al = al && aligned16(J.in[i]);
        }
        J.out = out[o0];
        al = al && aligned16(J.out);
        XorLaunch X;
        std::memset(&X, 0, sizeof(X));
        X.njobs = 1;
        X.nin = ni;
        X.accumulate = accumulate || ig > 0;
        X.bytes_only = al ? 0 : 1;
        X.nbytes = nbytes;
        X.blocks_per_job = blocks_per_job(1, nbytes, xor_blocks_cap(), blocks_total);
        e = launch_xor_single(X, J, stream);
      } else {
        GfJob J;
        std::memset(&J, 0, sizeof(J));
        for (int i = 0; i < ni; ++i) {
          J.in[i] = in[i0 + i];
          al = al && aligned16(J.in[i]);
        }
        for (int j = 0; j < no; ++j) {
          J.out[j] = out[o0 + j];
          al = al && aligned16(J.out[j]);
          for (int i = 0; i < ni; ++i) J.coef[j][i] = m.coef[static_cast<size_t>(o0 + j) * nin + i0 + i];
        }
        GfLaunch G;
        std::memset(&G, 0, sizeof(G));
        G.njobs = 1;
        G.nin = ni;
        G.nout = no;
        G.accumulate = accumulate || ig > 0;
        G.bytes_only = al ? 0 : 1;
        G.nbytes = nbytes;
        G.blocks_per_job = blocks_per_job(1, nbytes, gf_blocks_per_cu(ni), blocks_total);
        e = launch_gf_single(G, J, stream);
      }
      if (e) return hip_check(static_cast<hipError_t>(e), "stripe kernel launch");
    }
  }
  return REDSET_SUCCESS;
}

// ---- set verification ----------------------------------------------------

// column window and rows per pass of a wide stripe's check: the scratch is
// kVerifyRows x kVerifyWindow at most, whatever the set
constexpr size_t kVerifyWindow = size_t(8) << 20;
constexpr int kVerifyRows = kMaxOut;

bool verify_fused(const StripeMap& m) {
  const int nin = static_cast<int>(m.in.size()), nout = static_cast<int>(m.out.size());
  return m.xor_only ? nin + 1 <= kMaxIn : (nin <= kMaxIn && nout <= kMaxOut);
}

namespace {
size_t verify_window(size_t nbytes) { return std::min(kVerifyWindow, (nbytes + 255) & ~size_t(255)); }
}  // namespace

size_t verify_scratch_bytes(const StripeMap& m, size_t nbytes) {
  if (verify_fused(m) || m.out.empty()) return 0;
  return static_cast<size_t>(std::min<int>(kVerifyRows, static_cast<int>(m.out.size()))) * verify_window(nbytes);
}

int verify_report_reset(unsigned long long* report, int report_rows, int row0, int nrows, void* stream) {
  return hip_check(static_cast<hipError_t>(reset_report(report, report_rows, row0, nrows, stream)), "report reset");
}

namespace {
// one check launch of a single job passed by value
int check_gf_single(const GfJob& J, int nin, int nout, size_t nbytes, size_t base, unsigned long long* report,
                    int report_rows, int row0, void* stream) {
  bool al = true;
  for (int i = 0; i < nin; ++i) al = al && aligned16(J.in[i]);
  for (int j = 0; j < nout; ++j) al = al && aligned16(J.out[j]);
  GfCheckLaunch C;
  std::memset(&C, 0, sizeof(C));
  C.g.njobs = 1;
  C.g.nin = nin;
  C.g.nout = nout;
  C.g.bytes_only = al ? 0 : 1;
  C.g.nbytes = nbytes;
  C.g.blocks_per_job = blocks_per_job(1, nbytes, gf_blocks_per_cu(nin));
  C.report = report;
  C.report_rows = report_rows;
  C.row0 = row0;
  C.row_stride = nout;
  C.base = base;
  return hip_check(static_cast<hipError_t>(launch_gf_check(C, &J, stream)), "gf_check launch");
}
int check_xor_single(const XorJob& J, int nin, size_t nbytes, size_t base, unsigned long long* report,
                     int report_rows, int row0, void* stream) {
  bool al = true;
  for (int i = 0; i < nin; ++i) al = al && aligned16(J.in[i]);
  XorCheckLaunch C;
  std::memset(&C, 0, sizeof(C));
  C.x.njobs = 1;
  C.x.nin = nin;
  C.x.bytes_only = al ? 0 : 1;
  C.x.nbytes = nbytes;
  C.x.blocks_per_job = blocks_per_job(1, nbytes, xor_blocks_cap());
  C.report = report;
  C.report_rows = report_rows;
  C.row0 = row0;
  C.row_stride = 1;
  C.base = base;
  return hip_check(static_cast<hipError_t>(launch_xor_check(C, &J, stream)), "xor_check launch");
}
}  // namespace

int run_verify_stripe(const StripeMap& m, const uint8_t* const* in, const uint8_t* const* stored, size_t nbytes,
                      size_t base, unsigned long long* report, int report_rows, int row0, uint8_t* scratch,
                      void* stream, VerifyCount* count) {
  const int nin = static_cast<int>(m.in.size()), nt = static_cast<int>(m.out.size());
  if (nt == 0 || nbytes == 0) return REDSET_SUCCESS;
  if (nin == 0) return fail("stripe with parity but no data cells");
  if (m.xor_only && nt != 1) return fail("XOR stripe with %d parity cells", nt);
  if (verify_fused(m)) {
    if (count) {
      count->bytes_read += static_cast<unsigned long long>(nin + nt) * nbytes;
      count->launches += 1;
      return REDSET_SUCCESS;
    }
    if (m.xor_only) {
      XorJob J;
      std::memset(&J, 0, sizeof(J));
      for (int i = 0; i < nin; ++i) J.in[i] = in[i];
      J.in[nin] = stored[0];
      return check_xor_single(J, nin + 1, nbytes, base, report, report_rows, row0, stream);
    }
    GfJob J;
    std::memset(&J, 0, sizeof(J));
    for (int i = 0; i < nin; ++i) J.in[i] = in[i];
    for (int j = 0; j < nt; ++j) {
      J.out[j] = const_cast<uint8_t*>(stored[j]);  // only read (gf_check_kernel)
      for (int i = 0; i < nin; ++i) J.coef[j][i] = m.coef[static_cast<size_t>(j) * nin + i];
    }
    return check_gf_single(J, nin, nt, nbytes, base, report, report_rows, row0, stream);
  }
  // wide: <= kVerifyRows parity rows of one column window into the scratch
  // with the combine passes, then the scratch against the stored cells
  if (!count && !scratch) return fail("wide verify without scratch");
  const size_t W = verify_window(nbytes);
  const int passes = (nin + kMaxIn - 1) / kMaxIn;
  std::vector<const uint8_t*> win(static_cast<size_t>(nin));
  for (int o0 = 0; o0 < nt; o0 += kVerifyRows) {
    const int no = std::min(kVerifyRows, nt - o0);
    StripeMap sub;
    sub.in = m.in;
    sub.out.assign(m.out.begin() + o0, m.out.begin() + o0 + no);
    sub.coef.assign(m.coef.begin() + static_cast<size_t>(o0) * nin, m.coef.begin() + static_cast<size_t>(o0 + no) * nin);
    sub.xor_only = m.xor_only;
    for (size_t woff = 0; woff < nbytes; woff += W) {
      const size_t len = std::min(W, nbytes - woff);
      if (count) {
        // every pass reads its inputs and, after the first, the scratch rows
        // it accumulates into; the check reads the scratch and the stored rows
        count->bytes_read += (static_cast<unsigned long long>(nin) + static_cast<unsigned long long>(passes - 1) * no +
                              2ull * no) * len;
        count->bytes_written += static_cast<unsigned long long>(passes) * no * len;
        count->launches += passes + 1;
        continue;
      }
      uint8_t* rows[kVerifyRows];
      for (int j = 0; j < no; ++j) rows[j] = scratch + static_cast<size_t>(j) * W;
      for (int i = 0; i < nin; ++i) win[static_cast<size_t>(i)] = in[i] + woff;
      if (int rc = run_stripe(sub, win.data(), rows, len, stream, 0)) return rc;
      if (m.xor_only) {
        XorJob J;
        std::memset(&J, 0, sizeof(J));
        J.in[0] = rows[0];
        J.in[1] = stored[0] + woff;
        if (int rc = check_xor_single(J, 2, len, base + woff, report, report_rows, row0, stream)) return rc;
      } else {
        // one input of coefficient 1 per row: parity row j = 1 * scratch row j
        GfJob J;
        std::memset(&J, 0, sizeof(J));
        for (int j = 0; j < no; ++j) {
          J.in[j] = rows[j];
          J.out[j] = const_cast<uint8_t*>(stored[o0 + j] + woff);
          J.coef[j][j] = 1;
        }
        if (int rc = check_gf_single(J, no, no, len, base + woff, report, report_rows, row0 + o0, stream)) return rc;
      }
    }
  }
  return REDSET_SUCCESS;
}

}  // namespace redset_hip

namespace {

// Whole-set verify plan from the stripes' encode maps. Fused stripes share
// launches over a device job array: runs of consecutive stripes with the same
// alignment, so a launch's jobs report to consecutive rows.
int build_verify_plan(redset_hip_plan* plan, const std::vector<StripeMap>& maps, const SetLayout& L, size_t nbytes) {
  const int e = plan->info.encoding;
  plan->report_rows = static_cast<int>(maps.size()) * e;
  {
    void* rp = nullptr;
    const size_t bytes = 2 * static_cast<size_t>(std::max(1, plan->report_rows)) * sizeof(unsigned long long);
    if (int rc = hip_check(hipMalloc(&rp, bytes), "hipMalloc(verify report)")) return rc;
    plan->d_report = static_cast<unsigned long long*>(rp);
  }
  if (int rc = hip_check(static_cast<hipError_t>(redset_hip::reset_report(plan->d_report, plan->report_rows, 0,
                                                                          plan->report_rows, nullptr)),
                         "report reset"))
    return rc;
  if (int rc = hip_check(hipStreamSynchronize(nullptr), "report reset")) return rc;
  redset_hip::VerifyCount cnt;
  std::vector<GfJob> gall;
  std::vector<XorJob> xall;
  size_t scratch = 0;
  int run_al = -1;  // alignment of the open run of fused stripes
  for (size_t c = 0; c < maps.size(); ++c) {
    const StripeMap& m = maps[c];
    const int nin = static_cast<int>(m.in.size()), nt = static_cast<int>(m.out.size());
    if (nt != e || nin == 0) return fail("verify: stripe %zu has %d parity and %d data cells", c, nt, nin);
    if (!redset_hip::verify_fused(m)) {
      redset_hip_plan::WideStripe w;
      w.map = m;
      for (const CellRef& r : m.in) w.in.push_back(L.at(r));
      for (const CellRef& r : m.out) w.stored.push_back(L.at(r));
      w.row0 = static_cast<int>(c) * e;
      scratch = std::max(scratch, redset_hip::verify_scratch_bytes(m, nbytes));
      if (int rc = redset_hip::run_verify_stripe(m, w.in.data(), w.stored.data(), nbytes, 0, nullptr, 0, 0, nullptr,
                                                 nullptr, &cnt))
        return rc;
      plan->wide.push_back(std::move(w));
      run_al = -1;
      continue;
    }
    cnt.bytes_read += static_cast<unsigned long long>(nin + nt) * nbytes;
    bool al = true;
    if (m.xor_only) {
      XorJob J;
      std::memset(&J, 0, sizeof(J));
      for (int i = 0; i < nin; ++i) J.in[i] = L.at(m.in[i]);
      J.in[nin] = L.at(m.out[0]);
      for (int i = 0; i <= nin; ++i) al = al && aligned16(J.in[i]);
      if (run_al != (al ? 1 : 0)) {
        redset_hip::XorCheckLaunch C;
        std::memset(&C, 0, sizeof(C));
        C.x.jobs = reinterpret_cast<const XorJob*>(xall.size());  // offset, patched below
        C.x.nin = nin + 1;
        C.x.bytes_only = al ? 0 : 1;
        C.x.nbytes = nbytes;
        C.row0 = static_cast<int>(c) * e;
        plan->xor_checks.push_back(C);
        run_al = al ? 1 : 0;
      }
      plan->xor_checks.back().x.njobs += 1;
      xall.push_back(J);
    } else {
      GfJob J;
      std::memset(&J, 0, sizeof(J));
      for (int i = 0; i < nin; ++i) {
        J.in[i] = L.at(m.in[i]);
        al = al && aligned16(J.in[i]);
      }
      for (int j = 0; j < nt; ++j) {
        J.out[j] = L.at(m.out[j]);  // the stored parity: only read
        al = al && aligned16(J.out[j]);
        for (int i = 0; i < nin; ++i) J.coef[j][i] = m.coef[static_cast<size_t>(j) * nin + i];
      }
      if (run_al != (al ? 1 : 0)) {
        redset_hip::GfCheckLaunch C;
        std::memset(&C, 0, sizeof(C));
        C.g.jobs = reinterpret_cast<const GfJob*>(gall.size());
        C.g.nin = nin;
        C.g.nout = nt;
        C.g.bytes_only = al ? 0 : 1;
        C.g.nbytes = nbytes;
        C.row0 = static_cast<int>(c) * e;
        plan->gf_checks.push_back(C);
        run_al = al ? 1 : 0;
      }
      plan->gf_checks.back().g.njobs += 1;
      gall.push_back(J);
    }
  }
  // the per-job body only: stripes side by side for small cells, a launch
  // per stripe for big ones (sequential_jobs, as the plans whose kernels have
  // no streamed or claimed order)
  auto shape = [&](auto& C, auto& Lh, int occupancy) {
    Lh.sequential = sequential_jobs(Lh.njobs, nbytes, false, false, false, false);
    Lh.group = stripes_per_launch(Lh.sequential);
    Lh.blocks_per_job = blocks_per_job(jobs_sharing_grid(Lh.sequential, Lh.njobs, Lh.group), nbytes, occupancy);
    C.report = plan->d_report;
    C.report_rows = plan->report_rows;
    C.row_stride = e;
    C.reset = 1;
    cnt.launches += launches_of(Lh.sequential, Lh.njobs, Lh.group);
  };
  for (auto& C : plan->gf_checks) shape(C, C.g, redset_hip::gf_blocks_per_cu(C.g.nin));
  for (auto& C : plan->xor_checks) shape(C, C.x, xor_blocks_cap());
  plan->info.bytes_read = cnt.bytes_read;
  plan->info.bytes_written = cnt.bytes_written;
  plan->info.launches = cnt.launches;
  plan->info.jobs = static_cast<int>(maps.size());
  if (!gall.empty()) {
    if (int rc = hip_check(hipMalloc(&plan->d_gf, gall.size() * sizeof(GfJob)), "hipMalloc(plan jobs)")) return rc;
    if (int rc = hip_check(hipMemcpy(plan->d_gf, gall.data(), gall.size() * sizeof(GfJob), hipMemcpyHostToDevice),
                           "hipMemcpy(plan jobs)"))
      return rc;
    for (auto& C : plan->gf_checks) C.g.jobs = plan->d_gf + reinterpret_cast<uintptr_t>(C.g.jobs);
  }
  if (!xall.empty()) {
    if (int rc = hip_check(hipMalloc(&plan->d_xor, xall.size() * sizeof(XorJob)), "hipMalloc(plan jobs)")) return rc;
    if (int rc = hip_check(hipMemcpy(plan->d_xor, xall.data(), xall.size() * sizeof(XorJob), hipMemcpyHostToDevice),
                           "hipMemcpy(plan jobs)"))
      return rc;
    for (auto& C : plan->xor_checks) C.x.jobs = plan->d_xor + reinterpret_cast<uintptr_t>(C.x.jobs);
  }
  if (scratch > 0) {
    void* sp = nullptr;
    if (int rc = hip_check(hipMalloc(&sp, scratch), "hipMalloc(verify scratch)")) return rc;
    plan->d_scratch = static_cast<uint8_t*>(sp);
  }
  return REDSET_SUCCESS;
}

int finish_verify_plan(int kind, int ranks, int encoding, size_t chunk, const std::vector<StripeMap>& maps,
                       const SetLayout& L, const redset_hip_rs* rs, redset_hip_plan** out) {
  redset_hip_plan* plan = new (std::nothrow) redset_hip_plan;
  if (!plan) return fail("out of host memory");
  plan->info.kind = kind;
  plan->info.ranks = ranks;
  plan->info.encoding = encoding;
  plan->info.chunk_size = chunk;
  plan->cells.resize(static_cast<size_t>(ranks) * ranks);
  for (int c = 0; c < ranks; ++c)
    for (int s = 0; s < ranks; ++s) {
      const CellRef cell = rs ? redset_hip::rs_cell(rs, s, c)
                              : (s == c ? CellRef{s, redset_hip::kParity, 0}
                                        : CellRef{s, redset_hip::kData, redset_hip::xor_segment(s, c)});
      plan->cells[static_cast<size_t>(c) * ranks + s] = L.at(cell);
    }
  if (rs) plan->mat = rs->mat;
  if (int rc = build_verify_plan(plan, maps, L, chunk)) {
    redset_hip_plan_destroy(plan);
    return rc;
  }
  *out = plan;
  return REDSET_SUCCESS;
}

bool is_verify(const redset_hip_plan* plan) {
  return plan->info.kind == REDSET_HIP_PLAN_RS_VERIFY || plan->info.kind == REDSET_HIP_PLAN_XOR_VERIFY;
}

// the plan's report as rows, ordered on `stream` after the work there
int read_report(const redset_hip_plan* plan, void* stream, std::vector<redset_hip_verify_row>& rows) {
  const size_t n = static_cast<size_t>(plan->report_rows);
  std::vector<unsigned long long> raw(2 * n);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (n > 0)
    if (int rc = hip_check(hipMemcpyAsync(raw.data(), plan->d_report, raw.size() * sizeof(unsigned long long),
                                          hipMemcpyDeviceToHost, s),
                           "verify report copy"))
      return rc;
  if (int rc = hip_check(hipStreamSynchronize(s), "verify report sync")) return rc;
  rows.resize(n);
  for (size_t i = 0; i < n; ++i) rows[i] = redset_hip_verify_row{raw[i], raw[n + i]};
  return REDSET_SUCCESS;
}

}  // namespace

extern "C" {

int redset_hip_test_build(void) { return redset_hip::test_knobs(); }

int redset_hip_ring_faults(unsigned* count, int clear) {
  if (!count) return fail("ring_faults: null argument");
  return hip_check(static_cast<hipError_t>(redset_hip::read_ring_faults(count, clear)), "ring_faults");
}
int redset_hip_hang_faults(void* stream, unsigned* count, int clear) {
  if (!count) return fail("hang_faults: null argument");
  return hip_check(static_cast<hipError_t>(redset_hip::read_hang_faults(stream, count, clear)), "hang_faults");
}
const char* redset_hip_last_error(void) { return redset_hip::last_error(); }
int redset_hip_record_error(const char* msg) { return fail("%s", msg ? msg : "unknown error"); }

int redset_hip_rs_shape(const redset_hip_rs* rs, int* ranks, int* encoding) {
  if (!rs) return fail("rs_shape: null codec");
  if (ranks) *ranks = rs->ranks;
  if (encoding) *encoding = rs->encoding;
  return REDSET_SUCCESS;
}
const char* redset_hip_version(void) { return "redset-hip 0.3 (gfx950)"; }
int redset_hip_abi_version(void) { return REDSET_HIP_ABI_VERSION; }

int redset_hip_rs_create(int ranks, int encoding, redset_hip_rs** out) {
  if (!out) return fail("null out-pointer");
  *out = nullptr;
  // same rules as redset_construct_rs, src/redset_reedsolomon.c:158-185
  if (encoding < 1 || encoding >= ranks) return fail("invalid encoding %d for %d ranks", encoding, ranks);
  if (ranks + encoding > 256) return fail("ranks + encoding = %d exceeds GF(2^8)", ranks + encoding);
  redset_hip_rs* rs = new (std::nothrow) redset_hip_rs;
  if (!rs) return fail("out of host memory");
  rs->ranks = ranks;
  rs->encoding = encoding;
  rs->mat = redset_hip::encoding_matrix(ranks, encoding);
  *out = rs;
  return REDSET_SUCCESS;
}

void redset_hip_rs_destroy(redset_hip_rs* rs) { delete rs; }

int redset_hip_rs_matrix(const redset_hip_rs* rs, unsigned char* mat_out) {
  if (!rs || !mat_out) return fail("null argument");
  std::memcpy(mat_out, rs->mat.data(), rs->mat.size());
  return REDSET_SUCCESS;
}

int redset_hip_rs_get_encoding_id(int ranks, int encoding, int rank, int chunk_id) {
  return redset_hip::encoding_id(ranks, encoding, rank, chunk_id);
}

int redset_hip_rs_get_data_id(int ranks, int encoding, int rank, int chunk_id) {
  return redset_hip::data_id(ranks, encoding, rank, chunk_id);
}

int redset_hip_rs_decode_matrix(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int chunk_id,
                                unsigned char* coef_out) {
  if (!rs || !coef_out || !rebuild_ranks) return fail("null argument");
  if (chunk_id < 0 || chunk_id >= rs->ranks) return fail("chunk id %d out of range", chunk_id);
  std::vector<uint8_t> D;
  if (int rc = redset_hip::rs_decode_matrix(rs, missing, rebuild_ranks, chunk_id, D)) return rc;
  std::memcpy(coef_out, D.data(), D.size());
  return REDSET_SUCCESS;
}

size_t redset_hip_cell_stride(size_t chunk_size) {
  constexpr size_t kAlign = 256, kPad = size_t(16) << 20;
  size_t stride = (chunk_size + kAlign - 1) / kAlign * kAlign;
  if (stride == 0) stride = kAlign;
  if (stride % kPad == 0) stride += kPad;
  return stride;
}

int redset_hip_rs_plan_encode(const redset_hip_rs* rs, unsigned char* const* lofi, unsigned char* const* parity,
                              size_t chunk_size, size_t stride, redset_hip_plan** out) {
  if (!rs) return fail("null rs state");
  if (int rc = check_set_args(reinterpret_cast<const void* const*>(lofi), reinterpret_cast<const void* const*>(parity),
                              rs->ranks, chunk_size, stride, out))
    return rc;
  std::vector<StripeMap> maps(rs->ranks);
  for (int c = 0; c < rs->ranks; ++c) redset_hip::rs_encode_map(rs, c, maps[c]);
  return finish_plan(REDSET_HIP_PLAN_RS_ENCODE, rs->ranks, rs->encoding, 0, chunk_size, maps,
                     SetLayout{lofi, parity, stride}, out);
}

int redset_hip_rs_plan_rebuild(const redset_hip_rs* rs, int missing, const int* rebuild_ranks,
                               unsigned char* const* lofi, unsigned char* const* parity, size_t chunk_size,
                               size_t stride, redset_hip_plan** out) {
  if (!rs) return fail("null rs state");
  if (int rc = check_set_args(reinterpret_cast<const void* const*>(lofi), reinterpret_cast<const void* const*>(parity),
                              rs->ranks, chunk_size, stride, out))
    return rc;
  if (missing < 0 || missing > rs->encoding)
    return fail("cannot rebuild %d members with %d parity chunks", missing, rs->encoding);
  if (missing > 0 && !rebuild_ranks) return fail("null rebuild_ranks");
  std::vector<StripeMap> maps;
  for (int c = 0; c < rs->ranks && missing > 0; ++c) {
    StripeMap m;
    if (int rc = redset_hip::rs_rebuild_map(rs, missing, rebuild_ranks, c, m)) return rc;
    maps.push_back(std::move(m));
  }
  return finish_plan(REDSET_HIP_PLAN_RS_REBUILD, rs->ranks, rs->encoding, missing, chunk_size, maps,
                     SetLayout{lofi, parity, stride}, out);
}

int redset_hip_xor_plan_encode(int ranks, unsigned char* const* lofi, unsigned char* const* xorc, size_t chunk_size,
                               size_t stride, redset_hip_plan** out) {
  if (ranks < 2) return fail("XOR needs at least 2 ranks, got %d", ranks);
  if (int rc = check_set_args(reinterpret_cast<const void* const*>(lofi), reinterpret_cast<const void* const*>(xorc),
                              ranks, chunk_size, stride, out))
    return rc;
  std::vector<StripeMap> maps(ranks);
  for (int c = 0; c < ranks; ++c) redset_hip::xor_encode_map(ranks, c, maps[c]);
  return finish_plan(REDSET_HIP_PLAN_XOR_ENCODE, ranks, 1, 0, chunk_size, maps, SetLayout{lofi, xorc, stride}, out);
}

int redset_hip_xor_plan_rebuild(int ranks, int root, unsigned char* const* lofi, unsigned char* const* xorc,
                                size_t chunk_size, size_t stride, redset_hip_plan** out) {
  if (ranks < 2) return fail("XOR needs at least 2 ranks, got %d", ranks);
  if (root < 0 || root >= ranks) return fail("root %d out of range", root);
  if (int rc = check_set_args(reinterpret_cast<const void* const*>(lofi), reinterpret_cast<const void* const*>(xorc),
                              ranks, chunk_size, stride, out))
    return rc;
  std::vector<StripeMap> maps(ranks);
  for (int c = 0; c < ranks; ++c) redset_hip::xor_rebuild_map(ranks, root, c, maps[c]);
  return finish_plan(REDSET_HIP_PLAN_XOR_REBUILD, ranks, 1, 1, chunk_size, maps, SetLayout{lofi, xorc, stride}, out);
}

int redset_hip_plan_combine(const redset_hip_combine_job* jobs, int njobs, size_t nbytes, redset_hip_plan** out) {
  if (!out) return fail("plan_combine: null out-pointer");
  *out = nullptr;
  if (njobs < 0 || (njobs > 0 && !jobs)) return fail("plan_combine: bad job list");
  // every job's cells as entries of one pointer table, so the set planner
  // (build_plan) takes them as cells of a layout with stride 0: cell
  // (rank = table index, index 0)
  std::vector<unsigned char*> table;
  std::vector<StripeMap> maps(static_cast<size_t>(njobs));
  for (int k = 0; k < njobs; ++k) {
    const redset_hip_combine_job& J = jobs[k];
    if (J.nin < 1 || J.nin > kMaxCombine || J.nout < 1 || J.nout > kMaxCombine || !J.in || !J.out || !J.coef)
      return fail("plan_combine: job %d: nin=%d, nout=%d (1..%d) or null array", k, J.nin, J.nout, kMaxCombine);
    StripeMap& m = maps[static_cast<size_t>(k)];
    bool ones = J.nout == 1;
    for (int i = 0; i < J.nin; ++i) {
      if (!J.in[i]) return fail("plan_combine: job %d: null input %d", k, i);
      m.in.push_back(redset_hip::CellRef{static_cast<int>(table.size()), redset_hip::kData, 0});
      table.push_back(const_cast<unsigned char*>(J.in[i]));
    }
    for (int j = 0; j < J.nout; ++j) {
      if (!J.out[j]) return fail("plan_combine: job %d: null output %d", k, j);
      m.out.push_back(redset_hip::CellRef{static_cast<int>(table.size()), redset_hip::kData, 0});
      table.push_back(J.out[j]);
    }
    m.coef.assign(J.coef, J.coef + static_cast<size_t>(J.nin) * J.nout);
    for (uint8_t c : m.coef) ones = ones && c == 1;
    m.xor_only = ones;  // one output, every coefficient 1: the XOR kernel
    m.accumulate = J.accumulate != 0;
  }
  return finish_plan(0, 0, 0, 0, nbytes, maps, SetLayout{table.data(), table.data(), 0}, out);
}

int redset_hip_rs_plan_verify(const redset_hip_rs* rs, unsigned char* const* lofi, unsigned char* const* parity,
                              size_t chunk_size, size_t stride, redset_hip_plan** out) {
  if (!rs) return fail("null rs state");
  if (int rc = check_set_args(reinterpret_cast<const void* const*>(lofi), reinterpret_cast<const void* const*>(parity),
                              rs->ranks, chunk_size, stride, out))
    return rc;
  std::vector<StripeMap> maps(rs->ranks);
  for (int c = 0; c < rs->ranks; ++c) redset_hip::rs_verify_map(rs, c, maps[c]);
  return finish_verify_plan(REDSET_HIP_PLAN_RS_VERIFY, rs->ranks, rs->encoding, chunk_size, maps,
                            SetLayout{lofi, parity, stride}, rs, out);
}

int redset_hip_xor_plan_verify(int ranks, unsigned char* const* lofi, unsigned char* const* xorc, size_t chunk_size,
                               size_t stride, redset_hip_plan** out) {
  if (ranks < 2) return fail("XOR needs at least 2 ranks, got %d", ranks);
  if (int rc = check_set_args(reinterpret_cast<const void* const*>(lofi), reinterpret_cast<const void* const*>(xorc),
                              ranks, chunk_size, stride, out))
    return rc;
  std::vector<StripeMap> maps(ranks);
  for (int c = 0; c < ranks; ++c) redset_hip::xor_encode_map(ranks, c, maps[c]);
  return finish_verify_plan(REDSET_HIP_PLAN_XOR_VERIFY, ranks, 1, chunk_size, maps, SetLayout{lofi, xorc, stride},
                            nullptr, out);
}

int redset_hip_plan_verify_report(const redset_hip_plan* plan, void* stream, redset_hip_verify_row* rows, int nrows,
                                  unsigned long long* total_mismatch_bytes) {
  if (!plan) return fail("verify_report: null plan");
  if (!is_verify(plan)) return fail("verify_report: not a verify plan (kind %d)", plan->info.kind);
  if (rows && nrows < plan->report_rows)
    return fail("verify_report: room for %d rows, the plan reports %d", nrows, plan->report_rows);
  std::vector<redset_hip_verify_row> got;
  if (int rc = read_report(plan, stream, got)) return rc;
  unsigned long long total = 0;
  for (size_t i = 0; i < got.size(); ++i) {
    total += got[i].mismatch_bytes;
    if (rows) rows[i] = got[i];
  }
  if (total_mismatch_bytes) *total_mismatch_bytes = total;
  return REDSET_SUCCESS;
}

int redset_hip_rs_locate_syndrome(const redset_hip_rs* rs, int chunk_id, const unsigned char* syndrome,
                                  int* member_out) {
  if (!rs || !syndrome || !member_out) return fail("locate_syndrome: null argument");
  const int p = rs->ranks, e = rs->encoding;
  if (chunk_id < 0 || chunk_id >= p) return fail("locate_syndrome: chunk id %d out of range", chunk_id);
  *member_out = -1;
  int nz = 0, only = -1;
  for (int j = 0; j < e; ++j)
    if (syndrome[j]) ++nz, only = j;
  if (e < 2 || nz == 0) return REDSET_SUCCESS;
  if (nz == 1) {
    // the holder of parity row `only`: member (chunk_id - only) mod p
    for (int r = 0; r < p; ++r)
      if (redset_hip::encoding_id(p, e, r, chunk_id) == p + only) *member_out = r;
    return REDSET_SUCCESS;
  }
  const redset_hip::Field& F = redset_hip::field();
  int found = -1, matches = 0;
  for (int m = 0; m < p; ++m) {
    if (redset_hip::encoding_id(p, e, m, chunk_id) >= p) continue;  // holds parity in this stripe
    int j0 = -1;
    for (int j = 0; j < e && j0 < 0; ++j)
      if (rs->mat[static_cast<size_t>(p + j) * p + m]) j0 = j;
    if (j0 < 0) continue;
    const uint8_t x = F.mul(syndrome[j0], F.inv(rs->mat[static_cast<size_t>(p + j0) * p + m]));
    bool ok = x != 0;
    for (int j = 0; j < e && ok; ++j) ok = F.mul(rs->mat[static_cast<size_t>(p + j) * p + m], x) == syndrome[j];
    if (ok) found = m, ++matches;
  }
  if (matches == 1) *member_out = found;
  return REDSET_SUCCESS;
}

int redset_hip_plan_verify_locate(const redset_hip_plan* plan, void* stream, int stripe, int* member_out,
                                  unsigned long long* offset_out) {
  if (!plan || !member_out || !offset_out) return fail("verify_locate: null argument");
  if (!is_verify(plan)) return fail("verify_locate: not a verify plan (kind %d)", plan->info.kind);
  const int p = plan->info.ranks, e = plan->info.encoding;
  if (stripe < 0 || stripe >= p) return fail("verify_locate: stripe %d out of range", stripe);
  *member_out = -1;
  *offset_out = ~0ull;
  std::vector<redset_hip_verify_row> rows;
  if (int rc = read_report(plan, stream, rows)) return rc;
  unsigned long long off = ~0ull;
  for (int i = 0; i < e; ++i) {
    const redset_hip_verify_row& r = rows[static_cast<size_t>(stripe) * e + i];
    if (r.mismatch_bytes) off = std::min(off, r.first_offset);
  }
  *offset_out = off;
  if (off == ~0ull || plan->info.kind != REDSET_HIP_PLAN_RS_VERIFY) return REDSET_SUCCESS;
  // the stripe's byte column at that offset, member by member
  std::vector<uint8_t> col(static_cast<size_t>(p));
  const hipStream_t s = static_cast<hipStream_t>(stream);
  for (int m = 0; m < p; ++m)
    if (int rc = hip_check(hipMemcpyAsync(&col[m], plan->cells[static_cast<size_t>(stripe) * p + m] + off, 1,
                                          hipMemcpyDeviceToHost, s),
                           "verify_locate copy"))
      return rc;
  if (int rc = hip_check(hipStreamSynchronize(s), "verify_locate sync")) return rc;
  const redset_hip::Field& F = redset_hip::field();
  std::vector<uint8_t> syn(static_cast<size_t>(e), 0);
  for (int m = 0; m < p; ++m) {
    const int enc = redset_hip::encoding_id(p, e, m, stripe);
    if (enc >= p) {
      syn[enc - p] ^= col[m];
      continue;
    }
    for (int j = 0; j < e; ++j) syn[j] ^= F.mul(plan->mat[static_cast<size_t>(p + j) * p + m], col[m]);
  }
  redset_hip_rs rs{p, e, plan->mat};
  return redset_hip_rs_locate_syndrome(&rs, stripe, syn.data(), member_out);
}

unsigned redset_hip_crc32_combine(unsigned crc_a, unsigned crc_b, unsigned long long len_b) {
  // the initial and final XORs of the two CRCs cancel: crc(A||B) = crc(A) * x^(8 len B) + crc(B)
  return redset_hip::crc_mulmod(crc_a, redset_hip::crc_xpow8(len_b)) ^ crc_b;
}

int redset_hip_plan_crc32(const redset_hip_crc_range* ranges, int nranges, redset_hip_plan** out) {
  if (!out) return fail("plan_crc32: null plan out-pointer");
  *out = nullptr;
  if (!ranges) return fail("plan_crc32: null range array");
  if (nranges <= 0) return fail("plan_crc32: %d ranges", nranges);
  unsigned long long total = 0, tiles = 0;
  for (int r = 0; r < nranges; ++r) {
    if (!ranges[r].ptr && ranges[r].len > 0) return fail("plan_crc32: range %d: null pointer with %zu bytes", r, ranges[r].len);
    total += ranges[r].len;
    tiles += redset_hip::crc_tiles(ranges[r].ptr, ranges[r].len);
  }
  if (tiles > 0x7fffffffull) return fail("plan_crc32: %llu bytes are more than one plan takes", total);
  // one device block: ranges, tile numbering, remainders, CRCs (each 16-B aligned)
  std::vector<redset_hip::CrcRange> hr(static_cast<size_t>(nranges));
  std::vector<int> base(static_cast<size_t>(nranges) + 1, 0);
  for (int r = 0; r < nranges; ++r) {
    hr[r] = redset_hip::crc_range(ranges[r].ptr, ranges[r].len);
    base[r + 1] = base[r] + static_cast<int>(redset_hip::crc_tiles(ranges[r].ptr, ranges[r].len));
  }
  auto up16 = [](size_t n) { return (n + 15) & ~size_t(15); };
  const size_t o_base = up16(hr.size() * sizeof(redset_hip::CrcRange));
  const size_t o_rem = o_base + up16(base.size() * sizeof(int));
  const size_t o_crc = o_rem + up16(static_cast<size_t>(tiles) * sizeof(unsigned));
  const size_t bytes = o_crc + up16(static_cast<size_t>(nranges) * sizeof(unsigned));
  redset_hip_plan* plan = new (std::nothrow) redset_hip_plan;
  if (!plan) return fail("out of host memory");
  plan->info.kind = REDSET_HIP_PLAN_CRC32;
  plan->info.jobs = nranges;
  plan->info.launches = tiles > 0 ? 2 : 1;
  plan->info.bytes_read = total;
  int rc = hip_check(hipMalloc(&plan->d_crc, bytes), "hipMalloc(crc plan)");
  char* d = static_cast<char*>(plan->d_crc);
  rc = rc ? rc : hip_check(hipMemset(d, 0, bytes), "hipMemset(crc plan)");
  rc = rc ? rc : hip_check(hipMemcpy(d, hr.data(), hr.size() * sizeof(redset_hip::CrcRange), hipMemcpyHostToDevice),
                           "hipMemcpy(crc ranges)");
  rc = rc ? rc : hip_check(hipMemcpy(d + o_base, base.data(), base.size() * sizeof(int), hipMemcpyHostToDevice),
                           "hipMemcpy(crc tiles)");
  const unsigned* tables = rc ? nullptr : redset_hip::crc_device_tables();
  if (!rc && !tables) rc = fail("plan_crc32: cannot place the lookup tables on the device");
  if (rc) {
    redset_hip_plan_destroy(plan);
    return rc;
  }
  plan->crc.ranges = reinterpret_cast<const redset_hip::CrcRange*>(d);
  plan->crc.tile_base = reinterpret_cast<const int*>(d + o_base);
  plan->crc.nranges = nranges;
  plan->crc.tile0 = 0;
  plan->crc.ntiles = static_cast<int>(tiles);
  plan->crc.rem = reinterpret_cast<unsigned*>(d + o_rem);
  plan->crc.crcs = reinterpret_cast<unsigned*>(d + o_crc);
  plan->crc.tables = tables;
  plan->crc.xtile = redset_hip::crc_xpow8(redset_hip::kCrcTile);
  *out = plan;
  return REDSET_SUCCESS;
}

int redset_hip_plan_crc32_report(const redset_hip_plan* plan, void* stream, unsigned* crcs, int ncrcs) {
  if (!plan || !crcs) return fail("crc32_report: null argument");
  if (plan->info.kind != REDSET_HIP_PLAN_CRC32) return fail("crc32_report: not a CRC plan (kind %d)", plan->info.kind);
  if (ncrcs < plan->crc.nranges) return fail("crc32_report: room for %d CRCs, the plan reports %d", ncrcs, plan->crc.nranges);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = hip_check(hipMemcpyAsync(crcs, plan->crc.crcs, static_cast<size_t>(plan->crc.nranges) * sizeof(unsigned),
                                        hipMemcpyDeviceToHost, s),
                         "crc32 report copy"))
    return rc;
  return hip_check(hipStreamSynchronize(s), "crc32 report sync");
}

int redset_hip_rs_plan_repair(const redset_hip_rs* rs, unsigned char* const* lofi, unsigned char* const* parity,
                              size_t chunk_size, size_t stride, int nstripes, const int* stripes, int apply,
                              redset_hip_plan** out) {
  if (!rs) return fail("null rs state");
  if (int rc = check_set_args(reinterpret_cast<const void* const*>(lofi), reinterpret_cast<const void* const*>(parity),
                              rs->ranks, chunk_size, stride, out))
    return rc;
  const int p = rs->ranks, e = rs->encoding, d = p - e;
  if (e < 2)
    return fail("plan_repair: encoding %d: one parity row locates nothing (rebuild the member a checksum names)", e);
  if (e > kMaxOut) return fail("plan_repair: encoding %d: repair is built for 2..%d parity rows", e, kMaxOut);
  if (!stripes) nstripes = p;
  if (nstripes < 0 || nstripes > p) return fail("plan_repair: %d stripes of a set of %d", nstripes, p);
  std::vector<char> seen(static_cast<size_t>(p), 0);
  std::vector<redset_hip::RepairJobDesc> jobs(static_cast<size_t>(nstripes));
  const SetLayout L{lofi, parity, stride};
  for (int k = 0; k < nstripes; ++k) {
    const int c = stripes ? stripes[k] : k;
    if (c < 0 || c >= p) return fail("plan_repair: stripe %d out of range", c);
    if (seen[c]) return fail("plan_repair: stripe %d listed twice", c);
    seen[c] = 1;
    StripeMap m;
    redset_hip::rs_verify_map(rs, c, m);
    redset_hip::RepairJobDesc& J = jobs[static_cast<size_t>(k)];
    for (const CellRef& r : m.in) J.data.push_back(L.at(r)), J.member.push_back(r.rank);
    for (const CellRef& r : m.out) J.parity.push_back(L.at(r)), J.member.push_back(r.rank);
    J.coef = m.coef;
    J.row = k;
    if (static_cast<int>(J.data.size()) != d || static_cast<int>(J.parity.size()) != e)
      return fail("plan_repair: stripe %d has %zu data and %zu parity cells", c, J.data.size(), J.parity.size());
  }
  redset_hip_plan* plan = new (std::nothrow) redset_hip_plan;
  if (!plan) return fail("out of host memory");
  plan->info.kind = REDSET_HIP_PLAN_RS_REPAIR;
  plan->info.ranks = p;
  plan->info.encoding = e;
  plan->info.chunk_size = chunk_size;
  plan->info.jobs = nstripes;
  plan->info.launches = nstripes > 0 && chunk_size > 0 ? 2 : 1;
  plan->info.bytes_read = static_cast<unsigned long long>(nstripes) * p * chunk_size;
  redset_hip::RepairLaunch& R = plan->repair;
  R.njobs = nstripes;
  R.d = d;
  R.e = e;
  R.p = p;
  R.apply = apply ? 1 : 0;
  R.nbytes = chunk_size;
  R.base = 0;
  R.ncells = nstripes * p;
  R.nstripes = nstripes;
  const size_t words = 2 * static_cast<size_t>(R.ncells) + 2 * static_cast<size_t>(R.nstripes);
  void* rp = nullptr;
  int rc = hip_check(hipMalloc(&rp, std::max<size_t>(1, words) * sizeof(unsigned long long)), "hipMalloc(repair report)");
  plan->d_repair_report = static_cast<unsigned long long*>(rp);
  R.cell_report = plan->d_repair_report;
  R.stripe_report = plan->d_repair_report + 2 * static_cast<size_t>(R.ncells);
  rc = rc ? rc : hip_check(static_cast<hipError_t>(redset_hip::repair_upload(jobs, d, e, &plan->d_repair, &R.jobs)),
                           "repair plan upload");
  // a report read before the first execute says "nothing found"
  rc = rc ? rc : hip_check(static_cast<hipError_t>(redset_hip::launch_repair_reset(R, nullptr)), "repair report reset");
  rc = rc ? rc : hip_check(hipStreamSynchronize(nullptr), "repair report reset");
  if (rc) {
    redset_hip_plan_destroy(plan);
    return rc;
  }
  R.blocks_per_job = redset_hip::repair_blocks_per_job(nstripes, chunk_size);
  *out = plan;
  return REDSET_SUCCESS;
}

int redset_hip_plan_repair_report(const redset_hip_plan* plan, void* stream, redset_hip_repair_cell* cells, int ncells,
                                  redset_hip_repair_stripe* stripes, int nstripes) {
  if (!plan) return fail("repair_report: null plan");
  if (plan->info.kind != REDSET_HIP_PLAN_RS_REPAIR)
    return fail("repair_report: not a repair plan (kind %d)", plan->info.kind);
  const redset_hip::RepairLaunch& R = plan->repair;
  if (cells && ncells < R.ncells) return fail("repair_report: room for %d cells, the plan reports %d", ncells, R.ncells);
  if (stripes && nstripes < R.nstripes)
    return fail("repair_report: room for %d stripes, the plan reports %d", nstripes, R.nstripes);
  const size_t nc = static_cast<size_t>(R.ncells), ns = static_cast<size_t>(R.nstripes);
  std::vector<unsigned long long> raw(2 * nc + 2 * ns);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (!raw.empty())
    if (int rc = hip_check(hipMemcpyAsync(raw.data(), plan->d_repair_report, raw.size() * sizeof(unsigned long long),
                                          hipMemcpyDeviceToHost, s),
                           "repair report copy"))
      return rc;
  if (int rc = hip_check(hipStreamSynchronize(s), "repair report sync")) return rc;
  for (size_t i = 0; cells && i < nc; ++i) cells[i] = redset_hip_repair_cell{raw[i], raw[nc + i]};
  for (size_t i = 0; stripes && i < ns; ++i) stripes[i] = redset_hip_repair_stripe{raw[2 * nc + i], raw[2 * nc + ns + i]};
  return REDSET_SUCCESS;
}

int redset_hip_rs_check_matrix(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int chunk_id,
                               unsigned char* mat_out, int* cols_lost_out) {
  if (!rs || !mat_out) return fail("check_matrix: null argument");
  redset_hip::CheckMatrix X;
  if (int rc = redset_hip::rs_check_matrix(rs, missing, rebuild_ranks, chunk_id, X)) return rc;
  std::memcpy(mat_out, X.M.data(), X.M.size());
  for (int i = 0; cols_lost_out && i < missing; ++i) cols_lost_out[i] = X.lost_cols[static_cast<size_t>(i)];
  return REDSET_SUCCESS;
}

int redset_hip_rs_locate_reduced(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int chunk_id,
                                 const unsigned char* reduced_syndrome, int* member_out, unsigned char* value_out) {
  if (!rs || !reduced_syndrome || !member_out) return fail("locate_reduced: null argument");
  *member_out = -1;
  if (value_out) *value_out = 0;
  redset_hip::CheckMatrix X;
  if (int rc = redset_hip::rs_check_matrix(rs, missing, rebuild_ranks, chunk_id, X)) return rc;
  int col = -1;
  uint8_t x = 0;
  redset_hip::locate_reduced(X, reduced_syndrome, &col, &x);
  if (col >= 0) {
    *member_out = X.cells[static_cast<size_t>(col)].rank;
    if (value_out) *value_out = x;
  }
  return REDSET_SUCCESS;
}

int redset_hip_rs_plan_rebuild_checked(const redset_hip_rs* rs, int missing, const int* rebuild_ranks,
                                       unsigned char* const* lofi, unsigned char* const* parity, size_t chunk_size,
                                       size_t stride, int fix_survivors, redset_hip_plan** out) {
  if (!rs) return fail("null rs state");
  if (int rc = check_set_args(reinterpret_cast<const void* const*>(lofi), reinterpret_cast<const void* const*>(parity),
                              rs->ranks, chunk_size, stride, out))
    return rc;
  const int p = rs->ranks, e = rs->encoding, k = missing, ns = p - k;
  if (e > kMaxOut)
    return fail("plan_rebuild_checked: encoding %d: the checked rebuild is built for 2..%d parity rows", e, kMaxOut);
  if (k == 0) return fail("plan_rebuild_checked: no member is lost (use the repair plan, redset_hip_rs_plan_repair)");
  if (k < 0 || k > e) return fail("plan_rebuild_checked: cannot rebuild %d members with %d parity chunks", k, e);
  if (k == e)
    return fail("plan_rebuild_checked: %d lost members of %d parity rows: nothing left to check (use the rebuild "
                "plan, redset_hip_rs_plan_rebuild)", k, e);
  std::vector<redset_hip::CheckedJobDesc> jobs(static_cast<size_t>(p));
  const SetLayout L{lofi, parity, stride};
  for (int c = 0; c < p; ++c) {
    redset_hip::CheckMatrix X;
    if (int rc = redset_hip::rs_check_matrix(rs, k, rebuild_ranks, c, X)) return rc;
    redset_hip::CheckedJobDesc& J = jobs[static_cast<size_t>(c)];
    std::vector<int> cols;
    for (int i = 0; i < p; ++i)
      if (std::find(X.lost_cols.begin(), X.lost_cols.end(), i) == X.lost_cols.end()) cols.push_back(i);
    for (int i : cols) J.in.push_back(L.at(X.cells[static_cast<size_t>(i)])), J.member.push_back(X.cells[static_cast<size_t>(i)].rank);
    for (int i : X.lost_cols) J.out.push_back(L.at(X.cells[static_cast<size_t>(i)]));
    for (int j = 0; j < e; ++j)
      for (int i : cols) J.coef.push_back(X.M[static_cast<size_t>(j) * p + i]);
    J.row = c;
  }
  redset_hip_plan* plan = new (std::nothrow) redset_hip_plan;
  if (!plan) return fail("out of host memory");
  plan->info.kind = REDSET_HIP_PLAN_RS_REBUILD_CHECKED;
  plan->info.ranks = p;
  plan->info.encoding = e;
  plan->info.missing = k;
  plan->info.chunk_size = chunk_size;
  plan->info.jobs = p;
  plan->info.launches = chunk_size > 0 ? 2 : 1;
  plan->info.bytes_read = static_cast<unsigned long long>(p) * ns * chunk_size;
  plan->info.bytes_written = static_cast<unsigned long long>(p) * k * chunk_size;
  redset_hip::CheckedLaunch& R = plan->checked;
  R.njobs = p;
  R.ns = ns;
  R.e = e;
  R.k = k;
  R.p = p;
  R.fix_survivors = fix_survivors ? 1 : 0;
  R.nbytes = chunk_size;
  R.base = 0;
  R.ncells = p * p;
  R.nstripes = p;
  const size_t words = 2 * static_cast<size_t>(R.ncells) + 2 * static_cast<size_t>(R.nstripes);
  void* rp = nullptr;
  int rc = hip_check(hipMalloc(&rp, words * sizeof(unsigned long long)), "hipMalloc(checked rebuild report)");
  plan->d_checked_report = static_cast<unsigned long long*>(rp);
  R.cell_report = plan->d_checked_report;
  R.stripe_report = plan->d_checked_report + 2 * static_cast<size_t>(R.ncells);
  rc = rc ? rc : hip_check(static_cast<hipError_t>(redset_hip::checked_upload(jobs, ns, e, k, &plan->d_checked, &R.jobs)),
                           "checked rebuild plan upload");
  // a report read before the first execute says "nothing found"
  rc = rc ? rc : hip_check(static_cast<hipError_t>(redset_hip::launch_checked_reset(R, nullptr)), "checked rebuild report reset");
  rc = rc ? rc : hip_check(hipStreamSynchronize(nullptr), "checked rebuild report reset");
  if (rc) {
    redset_hip_plan_destroy(plan);
    return rc;
  }
  R.blocks_per_job = redset_hip::checked_blocks_per_job(p, chunk_size);
  *out = plan;
  return REDSET_SUCCESS;
}

int redset_hip_plan_rebuild_checked_report(const redset_hip_plan* plan, void* stream, redset_hip_repair_cell* cells,
                                           int ncells, redset_hip_repair_stripe* stripes, int nstripes) {
  if (!plan) return fail("rebuild_checked_report: null plan");
  if (plan->info.kind != REDSET_HIP_PLAN_RS_REBUILD_CHECKED)
    return fail("rebuild_checked_report: not a checked rebuild plan (kind %d)", plan->info.kind);
  const redset_hip::CheckedLaunch& R = plan->checked;
  if (cells && ncells < R.ncells)
    return fail("rebuild_checked_report: room for %d cells, the plan reports %d", ncells, R.ncells);
  if (stripes && nstripes < R.nstripes)
    return fail("rebuild_checked_report: room for %d stripes, the plan reports %d", nstripes, R.nstripes);
  const size_t nc = static_cast<size_t>(R.ncells), ns = static_cast<size_t>(R.nstripes);
  std::vector<unsigned long long> raw(2 * nc + 2 * ns);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = hip_check(hipMemcpyAsync(raw.data(), plan->d_checked_report, raw.size() * sizeof(unsigned long long),
                                        hipMemcpyDeviceToHost, s),
                         "checked rebuild report copy"))
    return rc;
  if (int rc = hip_check(hipStreamSynchronize(s), "checked rebuild report sync")) return rc;
  for (size_t i = 0; cells && i < nc; ++i) cells[i] = redset_hip_repair_cell{raw[i], raw[nc + i]};
  for (size_t i = 0; stripes && i < ns; ++i) stripes[i] = redset_hip_repair_stripe{raw[2 * nc + i], raw[2 * nc + ns + i]};
  return REDSET_SUCCESS;
}

int redset_hip_plan_execute(const redset_hip_plan* plan, void* stream) {
  if (!plan) return fail("null plan");
  for (const auto& C : plan->gf_checks)
    if (int e = redset_hip::launch_gf_check(C, nullptr, stream)) return hip_check(static_cast<hipError_t>(e), "gf_check launch");
  for (const auto& C : plan->xor_checks)
    if (int e = redset_hip::launch_xor_check(C, nullptr, stream)) return hip_check(static_cast<hipError_t>(e), "xor_check launch");
  for (const auto& w : plan->wide) {
    const int rows = static_cast<int>(w.stored.size());
    if (int rc = redset_hip::verify_report_reset(plan->d_report, plan->report_rows, w.row0, rows, stream)) return rc;
    if (int rc = redset_hip::run_verify_stripe(w.map, w.in.data(), w.stored.data(), plan->info.chunk_size, 0,
                                               plan->d_report, plan->report_rows, w.row0, plan->d_scratch, stream))
      return rc;
  }
  if (plan->info.kind == REDSET_HIP_PLAN_CRC32)
    return hip_check(static_cast<hipError_t>(redset_hip::launch_crc32(plan->crc, stream)), "crc32 launch");
  if (plan->info.kind == REDSET_HIP_PLAN_RS_REPAIR) {
    if (int e = redset_hip::launch_repair_reset(plan->repair, stream))
      return hip_check(static_cast<hipError_t>(e), "repair report reset");
    return hip_check(static_cast<hipError_t>(redset_hip::launch_repair(plan->repair, stream)), "gf_repair launch");
  }
  if (plan->info.kind == REDSET_HIP_PLAN_RS_REBUILD_CHECKED) {
    if (int e = redset_hip::launch_checked_reset(plan->checked, stream))
      return hip_check(static_cast<hipError_t>(e), "checked rebuild report reset");
    return hip_check(static_cast<hipError_t>(redset_hip::launch_checked(plan->checked, stream)),
                     "gf_rebuild_checked launch");
  }
  for (const GfLaunch& G : plan->gf_launches)
    if (int e = redset_hip::launch_gf(G, stream)) return hip_check(static_cast<hipError_t>(e), "gf_mac launch");
  for (const XorLaunch& X : plan->xor_launches)
    if (int e = redset_hip::launch_xor(X, stream)) return hip_check(static_cast<hipError_t>(e), "xor launch");
  return REDSET_SUCCESS;
}

int redset_hip_plan_get_info(const redset_hip_plan* plan, redset_hip_plan_info* info) {
  if (!plan || !info) return fail("null argument");
  *info = plan->info;
  return REDSET_SUCCESS;
}

void redset_hip_plan_destroy(redset_hip_plan* plan) {
  if (!plan) return;
  if (plan->d_gf) (void) hipFree(plan->d_gf);
  if (plan->d_xor) (void) hipFree(plan->d_xor);
  if (plan->d_claim) (void) hipFree(plan->d_claim);
  if (plan->d_report) (void) hipFree(plan->d_report);
  if (plan->d_scratch) (void) hipFree(plan->d_scratch);
  if (plan->d_crc) (void) hipFree(plan->d_crc);
  if (plan->d_repair) (void) hipFree(plan->d_repair);
  if (plan->d_repair_report) (void) hipFree(plan->d_repair_report);
  if (plan->d_checked) (void) hipFree(plan->d_checked);
  if (plan->d_checked_report) (void) hipFree(plan->d_checked_report);
  delete plan;
}

int redset_hip_gf_combine(const unsigned char* const* in, int nin, unsigned char* const* out, int nout,
                          const unsigned char* coeffs, size_t nbytes, int accumulate, void* stream) {
  if (nin < 1 || nin > kMaxCombine || nout < 1 || nout > kMaxCombine)
    return fail("gf_combine: nin=%d, nout=%d (1..%d)", nin, nout, kMaxCombine);
  if (!in || !out || !coeffs) return fail("gf_combine: null argument");
  if (nin > kMaxIn || nout > kMaxOut) {
    // wider than one kernel pass: 16-input accumulate passes x 4-output groups
    redset_hip::StripeMap m;
    m.in.resize(nin);
    m.out.resize(nout);
    m.coef.assign(coeffs, coeffs + static_cast<size_t>(nin) * nout);
    for (int i = 0; i < nin; ++i)
      if (!in[i]) return fail("gf_combine: null input %d", i);
    for (int j = 0; j < nout; ++j)
      if (!out[j]) return fail("gf_combine: null output %d", j);
    return redset_hip::run_stripe(m, in, out, nbytes, stream, 0, accumulate != 0);
  }
  GfJob J;
  std::memset(&J, 0, sizeof(J));
  bool al = true;
  for (int i = 0; i < nin; ++i) {
    if (!in[i]) return fail("gf_combine: null input %d", i);
    J.in[i] = in[i];
    al = al && aligned16(in[i]);
  }
  for (int j = 0; j < nout; ++j) {
    if (!out[j]) return fail("gf_combine: null output %d", j);
    J.out[j] = out[j];
    al = al && aligned16(out[j]);
    for (int i = 0; i < nin; ++i) J.coef[j][i] = coeffs[j * nin + i];
  }
  GfLaunch G;
  std::memset(&G, 0, sizeof(G));
  G.njobs = 1;
  G.nin = nin;
  G.nout = nout;
  G.accumulate = accumulate ? 1 : 0;
  G.bytes_only = al ? 0 : 1;
  G.nbytes = nbytes;
  G.blocks_per_job = blocks_per_job(1, nbytes, redset_hip::gf_blocks_per_cu(nin));
  return hip_check(static_cast<hipError_t>(redset_hip::launch_gf_single(G, J, stream)), "gf_combine launch");
}

int redset_hip_xor_combine(const unsigned char* const* in, int nin, unsigned char* out, size_t nbytes, int accumulate,
                           void* stream) {
  if (nin < 1 || nin > kMaxCombine) return fail("xor_combine: nin=%d (1..%d)", nin, kMaxCombine);
  if (!in || !out) return fail("xor_combine: null argument");
  if (nin > kMaxIn) {
    redset_hip::StripeMap m;
    m.in.resize(nin);
    m.out.resize(1);
    m.coef.assign(static_cast<size_t>(nin), 1);
    m.xor_only = true;
    for (int i = 0; i < nin; ++i)
      if (!in[i]) return fail("xor_combine: null input %d", i);
    return redset_hip::run_stripe(m, in, &out, nbytes, stream, 0, accumulate != 0);
  }
  XorJob J;
  std::memset(&J, 0, sizeof(J));
  bool al = aligned16(out);
  for (int i = 0; i < nin; ++i) {
    if (!in[i]) return fail("xor_combine: null input %d", i);
    J.in[i] = in[i];
    al = al && aligned16(in[i]);
  }
  J.out = out;
  XorLaunch X;
  std::memset(&X, 0, sizeof(X));
  X.njobs = 1;
  X.nin = nin;
  X.accumulate = accumulate ? 1 : 0;
  X.bytes_only = al ? 0 : 1;
  X.nbytes = nbytes;
  X.blocks_per_job = blocks_per_job(1, nbytes, xor_blocks_cap());
  return hip_check(static_cast<hipError_t>(redset_hip::launch_xor_single(X, J, stream)), "xor_combine launch");
}

}  // extern "C"
