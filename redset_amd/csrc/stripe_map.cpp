// stripe_map.cpp -- see stripe_map.h.
#include "stripe_map.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "gf256.h"
#include "rebuild_checked_wide.h"
#include "repair2.h"
#include "repair_wide.h"

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

int rs_power_basis(const redset_hip_rs* rs, int c, std::vector<uint8_t>& alpha, std::vector<uint8_t>& u,
                   std::vector<uint8_t>& winv) {
  const int p = rs->ranks, e = rs->encoding, d = p - e, n = p + e;
  const Field& F = field();
  if (e != kRepair2E) return fail("power_basis: encoding %d: the two-error repair is built for 4 parity rows", e);
  if (c < 0 || c >= p) return fail("power_basis: chunk id %d out of range", c);
  if (n > 256) return fail("power_basis: %d points do not fit the field", n);
  StripeMap m;
  rs_verify_map(rs, c, m);
  if (static_cast<int>(m.in.size()) != d || static_cast<int>(m.out.size()) != e)
    return fail("power_basis: stripe %d has %zu data and %zu parity cells", c, m.in.size(), m.out.size());
  alpha.assign(static_cast<size_t>(d + e), 0);
  u.assign(static_cast<size_t>(d + e), 0);
  winv.assign(static_cast<size_t>(e) * e, 0);
  for (int i = 0; i < d + e; ++i) {
    const int a = i < d ? m.in[static_cast<size_t>(i)].rank : p + (i - d);
    uint8_t prod = 1;
    for (int b = 0; b < n; ++b)
      if (b != a) prod = F.mul(prod, static_cast<uint8_t>(a ^ b));
    alpha[i] = static_cast<uint8_t>(a);
    u[i] = F.inv(prod);
  }
  auto power_column = [&](int i, uint8_t* out) {  // u_i * alpha_i^t, 0^0 = 1
    uint8_t v = u[i];
    for (int t = 0; t < e; ++t, v = F.mul(v, alpha[i])) out[t] = v;
  };
  for (int j = 0; j < e; ++j) {
    uint8_t col[kRepair2E];
    power_column(d + j, col);
    for (int t = 0; t < e; ++t) winv[static_cast<size_t>(t) * e + j] = col[t];
  }
  // the structure is checked, not assumed: W^-1 H[:, i] over every column
  for (int i = 0; i < d + e; ++i) {
    uint8_t want[kRepair2E];
    power_column(i, want);
    for (int t = 0; t < e; ++t) {
      uint8_t got = 0;
      for (int j = 0; j < e; ++j) {
        const uint8_t h = i < d ? m.coef[static_cast<size_t>(j) * d + i] : static_cast<uint8_t>(j == i - d);
        got ^= F.mul(winv[static_cast<size_t>(t) * e + j], h);
      }
      if (got != want[t])
        return fail("power_basis: stripe %d column %d is not u * alpha^%d in the power basis (RS(%d,%d))", c, i, t, p, e);
    }
  }
  return 0;
}

int locate_pair(const redset_hip_rs* rs, int c, const uint8_t* S, int* cols_out, uint8_t* values_out, int* count_out) {
  const int e = kRepair2E;
  const Field& F = field();
  *count_out = 0;
  std::vector<uint8_t> alpha, u, winv;
  if (int rc = rs_power_basis(rs, c, alpha, u, winv)) return rc;
  const int n = static_cast<int>(alpha.size()), d = n - e;
  uint8_t s[kRepair2E] = {0, 0, 0, 0};
  for (int t = 0; t < e; ++t)
    for (int j = 0; j < e; ++j) s[t] ^= F.mul(winv[static_cast<size_t>(t) * e + j], S[j]);
  auto div = [&](uint8_t a, uint8_t b) { return F.mul(a, F.inv(b)); };
  const uint8_t D = F.mul(s[0], s[2]) ^ F.mul(s[1], s[1]);
  if (D == 0) return 0;
  const uint8_t sg2 = div(F.mul(s[2], s[2]) ^ F.mul(s[1], s[3]), D);
  const uint8_t sg1 = div(F.mul(s[0], s[3]) ^ F.mul(s[1], s[2]), D);
  int X[2], nroots = 0;
  for (int z = 0; z < 256; ++z) {
    const uint8_t zz = static_cast<uint8_t>(z);
    if ((F.mul(zz, zz) ^ F.mul(sg1, zz) ^ sg2) != 0) continue;
    if (nroots < 2) X[nroots] = z;
    ++nroots;
  }
  if (nroots != 2) return 0;
  int col[2];
  for (int k = 0; k < 2; ++k) {
    col[k] = -1;
    for (int i = 0; i < n; ++i)
      if (alpha[i] == X[k]) col[k] = i;
    if (col[k] < 0) return 0;  // a shortened position or a point past p + e
  }
  const uint8_t y1 = div(F.mul(s[0], static_cast<uint8_t>(X[1])) ^ s[1], static_cast<uint8_t>(X[0] ^ X[1]));
  const uint8_t y[2] = {y1, static_cast<uint8_t>(s[0] ^ y1)};
  uint8_t x[2];
  for (int k = 0; k < 2; ++k) {
    x[k] = div(y[k], u[col[k]]);
    if (x[k] == 0) return 0;
  }
  // the pair's own syndrome
  StripeMap m;
  rs_verify_map(rs, c, m);
  for (int j = 0; j < e; ++j) {
    uint8_t got = 0;
    for (int k = 0; k < 2; ++k)
      got ^= col[k] < d ? F.mul(m.coef[static_cast<size_t>(j) * d + col[k]], x[k])
                        : static_cast<uint8_t>(j == col[k] - d ? x[k] : 0);
    if (got != S[j]) return 0;
  }
  for (int k = 0; k < 2; ++k) cols_out[k] = col[k], values_out[k] = x[k];
  *count_out = 2;
  return 0;
}

int repair2_job(const redset_hip_rs* rs, int c, const std::vector<uint8_t*>& data, const std::vector<uint8_t*>& parity,
                int row, Repair2JobDesc& out) {
  const Field& F = field();
  std::vector<uint8_t> u, winv;
  if (int rc = rs_power_basis(rs, c, out.alpha, u, winv)) return rc;
  StripeMap m;
  rs_verify_map(rs, c, m);
  if (data.size() != m.in.size() || parity.size() != m.out.size())
    return fail("repair2: stripe %d takes %zu data and %zu parity cells", c, m.in.size(), m.out.size());
  out.cells = RepairJobDesc();
  out.cells.data = data;
  out.cells.parity = parity;
  out.cells.coef = m.coef;
  for (const CellRef& r : m.in) out.cells.member.push_back(r.rank);
  for (const CellRef& r : m.out) out.cells.member.push_back(r.rank);
  out.cells.row = row;
  out.invu.resize(u.size());
  for (size_t i = 0; i < u.size(); ++i) out.invu[i] = F.inv(u[i]);
  std::copy(winv.begin(), winv.end(), out.winv);
  return 0;
}

int rs_power_basis_wide(const redset_hip_rs* rs, int c, std::vector<uint8_t>& alpha, std::vector<uint8_t>& u,
                        std::vector<uint8_t>& winv) {
  const int p = rs->ranks, e = rs->encoding, d = p - e, n = p + e;
  const Field& F = field();
  if (e < kWideMinE || e > kWideMaxE)
    return fail("power_basis_wide: encoding %d: the wide repair is built for %d..%d parity rows", e, kWideMinE, kWideMaxE);
  if (c < 0 || c >= p) return fail("power_basis_wide: chunk id %d out of range", c);
  if (n > 256) return fail("power_basis_wide: p + e = %d points do not fit the field (p + e > 256)", n);
  StripeMap m;
  rs_verify_map(rs, c, m);
  if (static_cast<int>(m.in.size()) != d || static_cast<int>(m.out.size()) != e)
    return fail("power_basis_wide: stripe %d has %zu data and %zu parity cells", c, m.in.size(), m.out.size());
  alpha.assign(static_cast<size_t>(d + e), 0);
  u.assign(static_cast<size_t>(d + e), 0);
  winv.assign(static_cast<size_t>(e) * e, 0);
  for (int i = 0; i < d + e; ++i) {
    const int a = i < d ? m.in[static_cast<size_t>(i)].rank : p + (i - d);
    uint8_t prod = 1;
    for (int b = 0; b < n; ++b)
      if (b != a) prod = F.mul(prod, static_cast<uint8_t>(a ^ b));
    alpha[i] = static_cast<uint8_t>(a);
    u[i] = F.inv(prod);
  }
  auto power_column = [&](int i, uint8_t* out) {  // u_i * alpha_i^k, 0^0 = 1
    uint8_t v = u[i];
    for (int k = 0; k < e; ++k, v = F.mul(v, alpha[i])) out[k] = v;
  };
  for (int j = 0; j < e; ++j) {
    uint8_t col[kWideMaxE];
    power_column(d + j, col);
    for (int k = 0; k < e; ++k) winv[static_cast<size_t>(k) * e + j] = col[k];
  }
  // the structure is checked, not assumed: W^-1 H[:, i] over every column
  for (int i = 0; i < d + e; ++i) {
    uint8_t want[kWideMaxE];
    power_column(i, want);
    for (int k = 0; k < e; ++k) {
      uint8_t got = 0;
      for (int j = 0; j < e; ++j) {
        const uint8_t h = i < d ? m.coef[static_cast<size_t>(j) * d + i] : static_cast<uint8_t>(j == i - d);
        got ^= F.mul(winv[static_cast<size_t>(k) * e + j], h);
      }
      if (got != want[k])
        return fail("power_basis_wide: stripe %d column %d is not u * alpha^%d in the power basis (RS(%d,%d))", c, i, k, p,
                    e);
    }
  }
  return 0;
}

int locate_wide(const redset_hip_rs* rs, int c, const uint8_t* S, int max_errors, int* cols_out, uint8_t* values_out,
                int* count_out) {
  const Field& F = field();
  *count_out = 0;
  std::vector<uint8_t> alpha, u, winv;
  if (int rc = rs_power_basis_wide(rs, c, alpha, u, winv)) return rc;
  const int e = rs->encoding, n = static_cast<int>(alpha.size()), d = n - e, t = e / 2;
  if (max_errors < 1 || max_errors > t)
    return fail("locate_syndrome_wide: max_errors %d: %d parity rows correct 1..%d wrong bytes per column", max_errors, e, t);
  bool any = false;
  for (int j = 0; j < e; ++j) any = any || S[j] != 0;
  if (!any) return 0;
  uint8_t s[kWideMaxE] = {0};
  for (int k = 0; k < e; ++k)
    for (int j = 0; j < e; ++j) s[k] ^= F.mul(winv[static_cast<size_t>(k) * e + j], S[j]);
  StripeMap m;
  rs_verify_map(rs, c, m);
  for (int nu = 1; nu <= max_errors; ++nu) {
    // the Hankel system sum_k sigma_k S'_(j+k) = S'_(j+nu), j = 0..nu-1, by elimination
    uint8_t M[kWideMaxT][kWideMaxT + 1];
    for (int j = 0; j < nu; ++j)
      for (int k = 0; k <= nu; ++k) M[j][k] = s[j + k];
    bool singular = false;
    for (int col = 0; col < nu && !singular; ++col) {
      int piv = -1;
      for (int r = col; r < nu && piv < 0; ++r)
        if (M[r][col]) piv = r;
      if (piv < 0) {
        singular = true;
        break;
      }
      for (int k = 0; k <= nu; ++k) std::swap(M[col][k], M[piv][k]);
      const uint8_t inv = F.inv(M[col][col]);
      for (int k = 0; k <= nu; ++k) M[col][k] = F.mul(M[col][k], inv);
      for (int r = 0; r < nu; ++r) {
        const uint8_t f = M[r][col];
        if (r == col || !f) continue;
        for (int k = 0; k <= nu; ++k) M[r][k] ^= F.mul(f, M[col][k]);
      }
    }
    if (singular) continue;
    uint8_t sigma[kWideMaxT + 1];
    for (int k = 0; k < nu; ++k) sigma[k] = M[k][nu];
    sigma[nu] = 1;
    // every remaining power sum
    bool ok = true;
    for (int j = nu; j + nu < e && ok; ++j) {
      uint8_t v = 0;
      for (int k = 0; k <= nu; ++k) v ^= F.mul(sigma[k], s[j + k]);
      ok = v == 0;
    }
    if (!ok) continue;
    // exactly nu of this stripe's points are roots of z^nu ^ sigma_(nu-1) z^(nu-1) ^ ... ^ sigma_0
    int col[kWideMaxT], nroots = 0;
    for (int i = 0; i < n; ++i) {
      uint8_t v = 0;
      for (int k = nu; k >= 0; --k) v = F.mul(v, alpha[i]) ^ sigma[k];
      if (v != 0) continue;
      if (nroots < nu) col[nroots] = i;
      ++nroots;
    }
    if (nroots != nu) continue;
    // the Vandermonde system sum_i y_i X_i^k = S'_k, k < nu: with b(z) = locator / (z ^ X_i),
    // y_i = sum_k b_k S'_k / b(X_i)
    uint8_t x[kWideMaxT];
    for (int i = 0; i < nu && ok; ++i) {
      const uint8_t X = alpha[col[i]];
      uint8_t b = 1, num = 0, den = 0;
      for (int k = nu - 1; k >= 0; --k) {
        num ^= F.mul(b, s[k]);
        den = F.mul(den, X) ^ b;
        b = F.mul(b, X) ^ sigma[k];
      }
      x[i] = den ? F.mul(F.mul(num, F.inv(den)), F.inv(u[col[i]])) : 0;
      ok = x[i] != 0;
    }
    if (!ok) continue;
    // the correction's own syndrome
    for (int j = 0; j < e && ok; ++j) {
      uint8_t got = 0;
      for (int i = 0; i < nu; ++i)
        got ^= col[i] < d ? F.mul(m.coef[static_cast<size_t>(j) * d + col[i]], x[i])
                          : static_cast<uint8_t>(j == col[i] - d ? x[i] : 0);
      ok = got == S[j];
    }
    if (!ok) continue;
    for (int i = 0; i < nu; ++i) cols_out[i] = col[i], values_out[i] = x[i];
    *count_out = nu;
    return 0;
  }
  return 0;
}

int repair_wide_job(const redset_hip_rs* rs, int c, const std::vector<uint8_t*>& data,
                    const std::vector<uint8_t*>& parity, int row, RepairWideJobDesc& out) {
  const Field& F = field();
  std::vector<uint8_t> u;
  if (int rc = rs_power_basis_wide(rs, c, out.alpha, u, out.winv)) return rc;
  StripeMap m;
  rs_verify_map(rs, c, m);
  if (data.size() != m.in.size() || parity.size() != m.out.size())
    return fail("repair_wide: stripe %d takes %zu data and %zu parity cells", c, m.in.size(), m.out.size());
  out.cells = RepairJobDesc();
  out.cells.data = data;
  out.cells.parity = parity;
  out.cells.coef = m.coef;
  for (const CellRef& r : m.in) out.cells.member.push_back(r.rank);
  for (const CellRef& r : m.out) out.cells.member.push_back(r.rank);
  out.cells.row = row;
  out.invu.resize(u.size());
  for (size_t i = 0; i < u.size(); ++i) out.invu[i] = F.inv(u[i]);
  return 0;
}

int rs_check_basis_wide(const redset_hip_rs* rs, int missing, const int* rebuild_ranks, int c, CheckBasisWide& out) {
  const int p = rs->ranks, e = rs->encoding, d = p - e, n = p, k = missing, s = e - k;
  const Field& F = field();
  if (e < kWideMinE || e > kWideMaxE)
    return fail("check_basis_wide: encoding %d: the wide checked rebuild is built for %d..%d parity rows", e, kWideMinE,
                kWideMaxE);
  if (k < 1 || k >= e)
    return fail("check_basis_wide: %d lost members of %d parity rows: the wide checked rebuild takes 1..%d", k, e, e - 1);
  if (!rebuild_ranks) return fail("check_basis_wide: null rebuild_ranks");
  for (int i = 0; i < k; ++i) {
    if (rebuild_ranks[i] < 0 || rebuild_ranks[i] >= p)
      return fail("check_basis_wide: rebuild rank %d out of range", rebuild_ranks[i]);
    if (i > 0 && rebuild_ranks[i] == rebuild_ranks[i - 1])
      return fail("check_basis_wide: rebuild rank %d listed twice", rebuild_ranks[i]);
    if (i > 0 && rebuild_ranks[i] < rebuild_ranks[i - 1]) return fail("check_basis_wide: rebuild_ranks must be ascending");
  }
  std::vector<uint8_t> u, winv;
  if (int rc = rs_power_basis_wide(rs, c, out.alpha, u, winv)) return rc;  // chunk id, p + e > 256
  // B, the cells and the lost columns are rs_check_matrix's: the decode's own rows
  if (int rc = rs_check_matrix(rs, k, rebuild_ranks, c, out.X)) return rc;
  CheckMatrix& X = out.X;
  StripeMap vm;
  rs_verify_map(rs, c, vm);
  auto h = [&](int j, int i) {  // H = [A | I]
    return i < d ? vm.coef[static_cast<size_t>(j) * d + i] : static_cast<uint8_t>(j == i - d);
  };
  // Gamma(z) = prod over the lost columns of (z ^ alpha_l), coefficients g[0..k], g[k] = 1
  uint8_t g[kWideMaxE + 1] = {1};
  for (int i = 0; i < k; ++i) {
    const uint8_t a = out.alpha[static_cast<size_t>(X.lost_cols[static_cast<size_t>(i)])];
    g[i + 1] = 0;
    for (int m = i + 1; m > 0; --m) g[m] = static_cast<uint8_t>(g[m - 1] ^ F.mul(g[m], a));
    g[0] = F.mul(g[0], a);
  }
  // C = F * (W^-1 * H), F[j][j + m] = g[m]
  std::vector<uint8_t> P(static_cast<size_t>(e) * n, 0);
  for (int t = 0; t < e; ++t)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < e; ++j) P[static_cast<size_t>(t) * n + i] ^= F.mul(winv[static_cast<size_t>(t) * e + j], h(j, i));
  for (int j = 0; j < s; ++j)
    for (int i = 0; i < n; ++i) {
      uint8_t v = 0;
      for (int m = 0; m <= k; ++m) v ^= F.mul(g[m], P[static_cast<size_t>(j + m) * n + i]);
      X.M[static_cast<size_t>(j) * n + i] = v;
    }
  // the structure is checked, not assumed: column i of C is u_i Gamma(alpha_i) (1, alpha_i, ..), zero where lost
  out.uprime.assign(static_cast<size_t>(n), 0);
  for (int i = 0; i < n; ++i) {
    const uint8_t a = out.alpha[static_cast<size_t>(i)];
    uint8_t ga = 0;
    for (int m = k; m >= 0; --m) ga = static_cast<uint8_t>(F.mul(ga, a) ^ g[m]);
    const bool lost = std::find(X.lost_cols.begin(), X.lost_cols.end(), i) != X.lost_cols.end();
    if (lost != (ga == 0))
      return fail("check_basis_wide: stripe %d: the erasure locator and the lost columns disagree at column %d", c, i);
    uint8_t v = F.mul(u[static_cast<size_t>(i)], ga);
    out.uprime[static_cast<size_t>(i)] = v;
    for (int j = 0; j < s; ++j, v = F.mul(v, a))
      if (X.M[static_cast<size_t>(j) * n + i] != v)
        return fail("check_basis_wide: stripe %d column %d is not u' * alpha^%d in check row %d (RS(%d,%d), %d lost)", c,
                    i, j, j, p, e, k);
  }
  // every rebuild row, with its one on its lost column, is y * H for y = its parity columns
  for (int r = 0; r < k; ++r) {
    const uint8_t* b = X.M.data() + static_cast<size_t>(s + r) * n;
    for (int l = 0; l < k; ++l)
      if (b[X.lost_cols[static_cast<size_t>(l)]] != (l == r ? 1 : 0))
        return fail("check_basis_wide: stripe %d rebuild row %d is not the identity on the lost columns", c, r);
    for (int i = 0; i < d; ++i) {
      uint8_t v = 0;
      for (int j = 0; j < e; ++j) v ^= F.mul(b[d + j], h(j, i));
      if (v != b[i]) return fail("check_basis_wide: stripe %d rebuild row %d is not a combination of the parity rows", c, r);
    }
  }
  return 0;
}

int locate_reduced_wide(const CheckBasisWide& Bs, const uint8_t* T, int max_errors, int* cols_out, uint8_t* values_out,
                        int* count_out) {
  const Field& F = field();
  const CheckMatrix& X = Bs.X;
  const int n = X.d + X.e, s = X.e - X.k, t = s / 2;
  *count_out = 0;
  if (max_errors < std::min(1, t) || max_errors > t)
    return fail("locate_reduced_wide: max_errors %d: %d spare rows locate %d..%d wrong bytes per column", max_errors, s,
                std::min(1, t), t);
  bool any = false;
  for (int j = 0; j < s; ++j) any = any || T[j] != 0;
  if (!any) return 0;
  for (int nu = 1; nu <= max_errors; ++nu) {
    // the Hankel system sum_k sigma_k T_(j+k) = T_(j+nu), j = 0..nu-1, by elimination
    uint8_t M[kCwMaxT][kCwMaxT + 1];
    for (int j = 0; j < nu; ++j)
      for (int k = 0; k <= nu; ++k) M[j][k] = T[j + k];
    bool singular = false;
    for (int col = 0; col < nu && !singular; ++col) {
      int piv = -1;
      for (int r = col; r < nu && piv < 0; ++r)
        if (M[r][col]) piv = r;
      if (piv < 0) {
        singular = true;
        break;
      }
      for (int k = 0; k <= nu; ++k) std::swap(M[col][k], M[piv][k]);
      const uint8_t inv = F.inv(M[col][col]);
      for (int k = 0; k <= nu; ++k) M[col][k] = F.mul(M[col][k], inv);
      for (int r = 0; r < nu; ++r) {
        const uint8_t f = M[r][col];
        if (r == col || !f) continue;
        for (int k = 0; k <= nu; ++k) M[r][k] ^= F.mul(f, M[col][k]);
      }
    }
    if (singular) continue;
    uint8_t sigma[kCwMaxT + 1];
    for (int k = 0; k < nu; ++k) sigma[k] = M[k][nu];
    sigma[nu] = 1;
    // every remaining equation
    bool ok = true;
    for (int j = nu; j + nu < s && ok; ++j) {
      uint8_t v = 0;
      for (int k = 0; k <= nu; ++k) v ^= F.mul(sigma[k], T[j + k]);
      ok = v == 0;
    }
    if (!ok) continue;
    // exactly nu of the surviving cells' points are roots
    int col[kCwMaxT], nroots = 0;
    for (int i = 0; i < n; ++i) {
      if (Bs.uprime[static_cast<size_t>(i)] == 0) continue;  // a lost column
      uint8_t v = 0;
      for (int k = nu; k >= 0; --k) v = F.mul(v, Bs.alpha[static_cast<size_t>(i)]) ^ sigma[k];
      if (v != 0) continue;
      if (nroots < nu) col[nroots] = i;
      ++nroots;
    }
    if (nroots != nu) continue;
    // with b(z) = locator / (z ^ X_i): y_i = sum_k b_k T_k / b(X_i), x_i = y_i / u'_i
    uint8_t x[kCwMaxT];
    for (int i = 0; i < nu && ok; ++i) {
      const uint8_t Xi = Bs.alpha[static_cast<size_t>(col[i])];
      uint8_t b = 1, num = 0, den = 0;
      for (int k = nu - 1; k >= 0; --k) {
        num ^= F.mul(b, T[k]);
        den = F.mul(den, Xi) ^ b;
        b = F.mul(b, Xi) ^ sigma[k];
      }
      x[i] = den ? F.mul(F.mul(num, F.inv(den)), F.inv(Bs.uprime[static_cast<size_t>(col[i])])) : 0;
      ok = x[i] != 0;
    }
    if (!ok) continue;
    // the correction's own image under the check rows
    for (int j = 0; j < s && ok; ++j) {
      uint8_t got = 0;
      for (int i = 0; i < nu; ++i) got ^= F.mul(X.M[static_cast<size_t>(j) * n + col[i]], x[i]);
      ok = got == T[j];
    }
    if (!ok) continue;
    for (int i = 0; i < nu; ++i) cols_out[i] = col[i], values_out[i] = x[i];
    *count_out = nu;
    return 0;
  }
  return 0;
}

void checked_wide_job(const CheckBasisWide& Bs, const std::vector<uint8_t*>& in, const std::vector<uint8_t*>& out,
                      int row, CheckedWideJobDesc& J) {
  const Field& F = field();
  const CheckMatrix& X = Bs.X;
  const int n = X.d + X.e;
  J = CheckedWideJobDesc();
  J.cells.in = in;
  J.cells.out = out;
  J.cells.row = row;
  std::vector<int> cols;
  for (int i = 0; i < n; ++i)
    if (std::find(X.lost_cols.begin(), X.lost_cols.end(), i) == X.lost_cols.end()) cols.push_back(i);
  for (int i : cols) {
    J.cells.member.push_back(X.cells[static_cast<size_t>(i)].rank);
    J.alpha.push_back(Bs.alpha[static_cast<size_t>(i)]);
    J.invu.push_back(F.inv(Bs.uprime[static_cast<size_t>(i)]));
  }
  for (int j = 0; j < X.e; ++j)
    for (int i : cols) J.cells.coef.push_back(X.M[static_cast<size_t>(j) * n + i]);
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
