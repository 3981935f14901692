// stripe_map.cpp -- see stripe_map.h.
#include "stripe_map.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "gf256.h"

namespace redset_hip {

thread_local std::string g_last_error;

int fail(const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return 1;  // REDSET_FAILURE
}

const char* last_error() { return g_last_error.c_str(); }

CellRef rs_cell(const redset_hip_rs* rs, int rank, int chunk) {
  const int p = rs->ranks, e = rs->encoding;
  const int enc = encoding_id(p, e, rank, chunk);
  if (enc < p) return CellRef{rank, kData, data_id(p, e, rank, chunk)};
  return CellRef{rank, kParity, enc - p};
}

int rs_encode_map(const redset_hip_rs* rs, int c, StripeMap& m) {
  const int p = rs->ranks, e = rs->encoding;
  m = StripeMap();
  std::vector<int> data_ranks;
  for (int s = 0; s < p; ++s) {
    if (encoding_id(p, e, s, c) < p) {
      data_ranks.push_back(s);
      m.in.push_back(rs_cell(rs, s, c));
    }
  }
  for (int r = 0; r < p; ++r) {
    const int row = encoding_id(p, e, r, c);
    if (row < p) continue;
    m.out.push_back(CellRef{r, kParity, row - p});
    for (int s : data_ranks) m.coef.push_back(rs->mat[static_cast<size_t>(row) * p + s]);
  }
  return 0;
}

int rs_verify_map(const redset_hip_rs* rs, int c, StripeMap& m) {
  StripeMap enc;
  if (int rc = rs_encode_map(rs, c, enc)) return rc;
  const size_t nin = enc.in.size(), nout = enc.out.size();
  m = enc;
  for (size_t j = 0; j < nout; ++j) {
    const size_t row = static_cast<size_t>(enc.out[j].index);  // slot i holds row p + i
    m.out[row] = enc.out[j];
    for (size_t i = 0; i < nin; ++i) m.coef[row * nin + i] = enc.coef[j * nin + i];
  }
  return 0;
}

int rs_decode_matrix(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int chunk,
                     std::vector<uint8_t>& D) {
  const int p = rs->ranks, e = rs->encoding;
  const Field& F = field();
  if (missing < 1 || missing > e) return fail("cannot rebuild %d members with %d parity chunks", missing, e);
  std::vector<int> unknowns(missing);
  std::vector<char> erased(p, 0);
  for (int i = 0; i < missing; ++i) {
    if (rebuild_ranks[i] < 0 || rebuild_ranks[i] >= p) return fail("rebuild rank %d out of range", rebuild_ranks[i]);
    if (i > 0 && rebuild_ranks[i] <= rebuild_ranks[i - 1]) return fail("rebuild_ranks must be ascending");
    erased[rebuild_ranks[i]] = 1;
    unknowns[i] = encoding_id(p, e, rebuild_ranks[i], chunk);
  }
  std::vector<uint8_t> sys;
  std::vector<int> rows;
  identify_rows(rs->mat, p, e, missing, unknowns.data(), sys, rows);
  for (int i = 0; i < missing; ++i)
    if (rows[i] < 0) return fail("no parity row available for unknown %d", i);
  const std::vector<uint8_t> T = solve_transform(sys, missing);
  // accumulator k (redset_rs_reduce_decode, src/redset_reedsolomon_common.c:
  // 855-899) = sum over surviving members s of a_k(s) * cell_s; the solved
  // buffer i = sum_k T[i][k] * accumulator k
  D.assign(static_cast<size_t>(missing) * p, 0);
  for (int s = 0; s < p; ++s) {
    if (erased[s]) continue;
    const int enc = encoding_id(p, e, s, chunk);
    for (int k = 0; k < missing; ++k) {
      const int row = rows[k] + p;
      const uint8_t a = enc < p ? rs->mat[static_cast<size_t>(row) * p + s] : static_cast<uint8_t>(enc == row);
      if (!a) continue;
      for (int i = 0; i < missing; ++i)
        D[static_cast<size_t>(i) * p + s] ^= F.mul(T[static_cast<size_t>(i) * missing + k], a);
    }
  }
  return 0;
}

int rs_rebuild_map(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int c, StripeMap& m) {
  const int p = rs->ranks;
  m = StripeMap();
  std::vector<uint8_t> D;
  if (int rc = rs_decode_matrix(rs, missing, rebuild_ranks, c, D)) return rc;
  std::vector<int> cols;
  for (int s = 0; s < p; ++s) {
    bool used = false;
    for (int i = 0; i < missing; ++i) used = used || D[static_cast<size_t>(i) * p + s] != 0;
    if (!used) continue;
    cols.push_back(s);
    m.in.push_back(rs_cell(rs, s, c));
  }
  for (int i = 0; i < missing; ++i) {
    m.out.push_back(rs_cell(rs, rebuild_ranks[i], c));
    for (int s : cols) m.coef.push_back(D[static_cast<size_t>(i) * p + s]);
  }
  return 0;
}

int rs_check_matrix(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int c, CheckMatrix& X) {
  const int p = rs->ranks, e = rs->encoding, d = p - e, n = p;
  const Field& F = field();
  if (c < 0 || c >= p) return fail("check_matrix: chunk id %d out of range", c);
  if (missing < 1 || missing > e) return fail("check_matrix: %d lost members with %d parity rows", missing, e);
  if (!rebuild_ranks) return fail("check_matrix: null rebuild_ranks");
  std::vector<char> erased(static_cast<size_t>(p), 0);
  for (int i = 0; i < missing; ++i) {
    const int r = rebuild_ranks[i];
    if (r < 0 || r >= p) return fail("check_matrix: rebuild rank %d out of range", r);
    if (erased[r]) return fail("check_matrix: rebuild rank %d listed twice", r);
    erased[r] = 1;
  }
  std::vector<uint8_t> D;
  if (int rc = rs_decode_matrix(rs, missing, rebuild_ranks, c, D)) return rc;
  StripeMap vm;
  rs_verify_map(rs, c, vm);
  X = CheckMatrix();
  X.d = d;
  X.e = e;
  X.k = missing;
  X.cells = vm.in;
  X.cells.insert(X.cells.end(), vm.out.begin(), vm.out.end());
  std::vector<int> col_of(static_cast<size_t>(p), -1);
  for (int i = 0; i < n; ++i) col_of[X.cells[i].rank] = i;
  for (int i = 0; i < missing; ++i) X.lost_cols.push_back(col_of[rebuild_ranks[i]]);
  // H = [A | I], then eliminate the lost columns: the rows left without a
  // pivot vanish on them
  std::vector<uint8_t> H(static_cast<size_t>(e) * n, 0);
  for (int j = 0; j < e; ++j) {
    for (int i = 0; i < d; ++i) H[static_cast<size_t>(j) * n + i] = vm.coef[static_cast<size_t>(j) * d + i];
    H[static_cast<size_t>(j) * n + d + j] = 1;
  }
  std::vector<char> used(static_cast<size_t>(e), 0);
  for (int i = 0; i < missing; ++i) {
    const int col = X.lost_cols[i];
    int r = -1;
    for (int j = 0; j < e && r < 0; ++j)
      if (!used[j] && H[static_cast<size_t>(j) * n + col]) r = j;
    if (r < 0) return fail("check_matrix: lost columns of stripe %d are dependent", c);
    used[r] = 1;
    const uint8_t s = F.inv(H[static_cast<size_t>(r) * n + col]);
    for (int t = 0; t < n; ++t) H[static_cast<size_t>(r) * n + t] = F.mul(H[static_cast<size_t>(r) * n + t], s);
    for (int j = 0; j < e; ++j) {
      const uint8_t f = H[static_cast<size_t>(j) * n + col];
      if (j == r || !f) continue;
      for (int t = 0; t < n; ++t) H[static_cast<size_t>(j) * n + t] ^= F.mul(f, H[static_cast<size_t>(r) * n + t]);
    }
  }
  X.M.assign(static_cast<size_t>(e) * n, 0);
  int row = 0;
  for (int j = 0; j < e; ++j)
    if (!used[j]) std::copy(H.begin() + static_cast<size_t>(j) * n, H.begin() + static_cast<size_t>(j + 1) * n,
                            X.M.begin() + static_cast<size_t>(row++) * n);
  // the rebuild rows are the decode's own linear map, so an unchecked column
  // gets the bytes the plain rebuild gives
  for (int i = 0; i < missing; ++i, ++row) {
    for (int s = 0; s < p; ++s)
      if (!erased[s]) X.M[static_cast<size_t>(row) * n + col_of[s]] = D[static_cast<size_t>(i) * p + s];
    X.M[static_cast<size_t>(row) * n + X.lost_cols[i]] = 1;
  }
  return 0;
}

void locate_reduced(const CheckMatrix& X, const uint8_t* R, int* col_out, uint8_t* value_out) {
  const int n = X.d + X.e, nck = X.e - X.k;
  const Field& F = field();
  *col_out = -1;
  *value_out = 0;
  bool any = false;
  for (int j = 0; j < nck; ++j) any = any || R[j] != 0;
  if (!any || nck < 2) return;  // one check row: every survivor explains the column
  int found = -1, matches = 0;
  uint8_t val = 0;
  for (int m = 0; m < n; ++m) {
    bool lost = false;
    for (int l : X.lost_cols) lost = lost || l == m;
    if (lost) continue;
    int j0 = -1;
    for (int j = 0; j < nck && j0 < 0; ++j)
      if (X.M[static_cast<size_t>(j) * n + m]) j0 = j;
    if (j0 < 0) continue;
    const uint8_t x = F.mul(R[j0], F.inv(X.M[static_cast<size_t>(j0) * n + m]));
    bool ok = x != 0;
    for (int j = 0; j < nck && ok; ++j) ok = F.mul(X.M[static_cast<size_t>(j) * n + m], x) == R[j];
    if (ok) found = m, val = x, ++matches;
  }
  if (matches == 1) *col_out = found, *value_out = val;
}

namespace {
CellRef xor_cell(int s, int c) { return s == c ? CellRef{s, kParity, 0} : CellRef{s, kData, xor_segment(s, c)}; }
}  // namespace

int xor_encode_map(int ranks, int c, StripeMap& m) {
  m = StripeMap();
  m.xor_only = true;
  for (int s = 0; s < ranks; ++s)
    if (s != c) m.in.push_back(xor_cell(s, c));
  m.out.push_back(CellRef{c, kParity, 0});
  m.coef.assign(m.in.size(), 1);
  return 0;
}

int xor_rebuild_map(int ranks, int root, int c, StripeMap& m) {
  if (root < 0 || root >= ranks) return fail("root %d out of range", root);
  m = StripeMap();
  m.xor_only = true;
  for (int s = 0; s < ranks; ++s)
    if (s != root) m.in.push_back(xor_cell(s, c));
  m.out.push_back(xor_cell(root, c));
  m.coef.assign(m.in.size(), 1);
  return 0;
}

}  // namespace redset_hip
