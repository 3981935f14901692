"""Brute-force numpy reference of the errors-and-erasures rebuild, shared by
the checked-rebuild tests (test_rebuild_checked_host.py,
test_gpu_rebuild_checked*.py). Not a test module.

It takes no matrix W and nothing of the check matrix under test: only the
encoding matrix and the cell numbering (codec.matrix(), encoding_id / data_id,
pinned against the CPU oracle by tests/test_abi.py) and the CPU oracle's GF
product. For a byte column with survivor bytes c, survivor m with value x
explains the column if and only if there are lost bytes v_L with H c = 0 after
c_m ^= x, i.e. H_L v_L = s ^ H_m x with s = H_S c_S. That is decided by plain
Gaussian elimination of the augmented system [H_L | rhs] (`solve`): it is
consistent iff the rows left without a pivot end up zero. Elimination is
linear in the right-hand side, so the rows without a pivot of rhs = H_m x are
tabulated once per (m, x) and a column is explained by (m, x) iff its own
such rows equal that entry. The verdict is exactly one (m, x), else unlocated."""
import numpy as np

from repair_ref import NO, mul_table  # noqa: F401

_inv = {}


def inv_table(mul):
    if "t" not in _inv:
        _inv["t"] = np.array([0] + [int(np.nonzero(mul[a] == 1)[0][0]) for a in range(1, 256)], np.uint8)
    return _inv["t"]


def solve(mul, HL, T):
    """Gaussian elimination of [HL | T] over GF(2^8): HL [e, k] (independent
    columns), T [e, N]. Returns (rest [e - k, N], v [k, N]): the right-hand
    sides of the rows without a pivot (all zero iff HL v = T has a solution)
    and the pivot rows' right-hand sides (the solution v when it has)."""
    A = HL.astype(np.uint8).copy()
    T = T.astype(np.uint8).copy()
    e, k = A.shape
    inv = inv_table(mul)
    used, piv = [False] * e, []
    for i in range(k):
        r = next(j for j in range(e) if not used[j] and A[j, i])
        used[r] = True
        piv.append(r)
        s = inv[A[r, i]]
        A[r] = mul[s, A[r]]
        T[r] = mul[s, T[r]]
        for j in range(e):
            f = A[j, i]
            if j != r and f:
                A[j] ^= mul[f, A[r]]
                T[j] ^= mul[f, T[r]]
    rest = [j for j in range(e) if not used[j]]
    assert not A[rest].any()
    return T[rest], T[piv]


def pack(rows):
    """[r, N] bytes -> [N] packed keys (row j in bits 8j)."""
    out = np.zeros(rows.shape[1], np.uint32)
    for j in range(rows.shape[0]):
        out |= rows[j].astype(np.uint32) << np.uint32(8 * j)
    return out


class Stripe:
    """Stripe c of an RS(p, e) set with the members `lost` gone."""

    def __init__(self, oracle, codec, c, lost):
        p, e = codec.ranks, codec.encoding
        self.p, self.e, self.d, self.c = p, e, p - e, c
        self.lost = sorted(lost)
        self.k = len(self.lost)
        self.surv = [m for m in range(p) if m not in self.lost]
        self.mul = mul_table(oracle)
        A = codec.matrix()[p:, :]
        self.H = np.zeros((e, p), np.uint8)  # member m's column of [A | I]
        self.row = [-1] * p    # parity row the member holds, or -1
        self.index = [0] * p   # the member's cell among its d data + e parity cells
        for m in range(p):
            enc = codec.encoding_id(m, c)
            if enc < p:
                self.index[m] = codec.data_id(m, c)
                self.H[:, m] = A[:, m]
            else:
                self.row[m] = enc - p
                self.index[m] = self.d + enc - p
                self.H[enc - p, m] = 1
        # the stripe's cells in the order of check_matrix's columns
        self.col_member = [m for m in range(p) if self.row[m] < 0] + \
                          [self.row.index(j) for j in range(e)]
        self.HL = self.H[:, self.lost]
        x = np.arange(1, 256)
        self.keys = {}  # survivor m: packed no-pivot rows of H_m x, x = 1..255
        for m in self.surv:
            rest, _ = solve(self.mul, self.HL, self.mul[self.H[:, m][:, None], x[None, :]])
            self.keys[m] = pack(rest)

    def matvec(self, Mat, by):
        """Mat [r, n] * by [n, N] over GF(2^8)."""
        out = np.zeros((Mat.shape[0], by.shape[1]), np.uint8)
        for j in range(Mat.shape[0]):
            for i in range(Mat.shape[1]):
                if Mat[j, i]:
                    out[j] ^= self.mul[Mat[j, i], by[i]]
        return out

    def explain(self, by):
        """by [p, N]: the members' bytes of N columns (lost members' rows are
        ignored). Returns (nonzero[N], member[N], x[N], v[k, N]): whether the
        survivors are inconsistent; the unique (member, x) that explains the
        column (-1, 0: consistent, or none or several do); the lost bytes
        after that correction (without one: the solution's pivot rows as they
        come, meaningful only for consistent columns)."""
        by = by.copy()
        by[self.lost] = 0
        s = self.matvec(self.H, by)
        rest, v = solve(self.mul, self.HL, s)
        key = pack(rest) if rest.shape[0] else np.zeros(by.shape[1], np.uint32)
        nonzero = key != 0
        hits = np.zeros(key.shape, np.int64)
        member = np.full(key.shape, -1, np.int64)
        xs = np.zeros(key.shape, np.uint8)
        for m in self.surv:
            # every x whose H_m x leaves the column's no-pivot rows counts
            order = np.argsort(self.keys[m], kind="stable")
            sk = self.keys[m][order]
            lo = np.searchsorted(sk, key, side="left")
            hi = np.searchsorted(sk, key, side="right")
            n = np.where(nonzero, hi - lo, 0)
            hits += n
            one = n > 0
            member[one] = m
            xs[one] = (order[np.minimum(lo[one], 254)] + 1).astype(np.uint8)
        bad = hits != 1
        member[bad] = -1
        xs[bad] = 0
        fix = member >= 0
        if fix.any():
            Hm = self.H[:, member[fix]]  # [e, nfix]
            t = s[:, fix] ^ self.mul[Hm, xs[fix][None, :]]
            rest2, v2 = solve(self.mul, self.HL, t)
            assert not rest2.any()
            v[:, fix] = v2
        return nonzero, member, xs, v


def predict(st, image, chunk, cols):
    """What a checked rebuild of stripe st must report for `image`
    ([p, d + e, stride] host bytes), examining the columns `cols` (every
    column that can be inconsistent): (corrected[p], first[p], unlocated,
    first_unlocated, located) with located = (member[n], col[n], x[n],
    v[k, n]) for the located columns."""
    cols = np.unique(np.asarray(cols, np.int64))
    by = np.stack([image[m, st.index[m], cols] for m in range(st.p)])
    nonzero, member, xs, v = st.explain(by)
    corrected = np.zeros(st.p, np.uint64)
    first = np.full(st.p, NO, np.uint64)
    for m in st.surv:
        mine = cols[member == m]
        if mine.size:
            corrected[m] = mine.size
            first[m] = mine.min()
    un = cols[nonzero & (member < 0)]
    fix = member >= 0
    return corrected, first, int(un.size), (int(un.min()) if un.size else NO), (member[fix], cols[fix], xs[fix], v[:, fix])


# ---- set images for the GPU tests ------------------------------------------

SENTINEL = 0xA5
GARBAGE = 0xEE  # what the lost cells hold before a rebuild
_images = {}


def stride_of(chunk, packed):
    return chunk if packed else -(-chunk // 256) * 256


def clean_image(oracle, p, e, chunk, packed=False):
    """[p, d + e, stride] host bytes of an oracle-encoded set, sentinel in the
    padding. Made once per (shape, chunk, layout), shared, never modified."""
    key = (p, e, chunk, packed)
    if key not in _images:
        d = p - e
        lofi, parity = oracle.random_set(p, d, e, chunk, seed=7000 + 100 * p + e + chunk % 991)
        oracle.OracleRS(p, e).encode_set(lofi, parity, chunk)
        img = np.full((p, d + e, stride_of(chunk, packed)), SENTINEL, np.uint8)
        for r in range(p):
            img[r, :d, :chunk] = lofi[r].reshape(d, chunk)
            img[r, d:, :chunk] = parity[r].reshape(e, chunk)
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def lose(img, lost, chunk):
    """A copy with the lost members' cells overwritten (padding kept)."""
    out = img.copy()
    out[lost, :, :chunk] = GARBAGE
    return out


def oracle_rebuild(oracle, img, e, lost, chunk):
    """The CPU oracle's plain rebuild of the lost members from the image's
    survivors as they are: a copy of the image with their cells filled in."""
    p, cells, _ = img.shape
    d = cells - e
    lofi = [np.ascontiguousarray(img[r, :d, :chunk]).reshape(-1).copy() for r in range(p)]
    parity = [np.ascontiguousarray(img[r, d:, :chunk]).reshape(-1).copy() for r in range(p)]
    assert oracle.OracleRS(p, e).rebuild_set(lost, lofi, parity, chunk) == 0
    out = img.copy()
    for r in lost:
        out[r, :d, :chunk] = lofi[r].reshape(d, chunk)
        out[r, d:, :chunk] = parity[r].reshape(e, chunk)
    return out


def predict_set(oracle, codec, img, lost, chunk, cols_by_stripe):
    """What a checked rebuild of the whole set must do with `img` (survivors
    as they are; the lost members' cells are ignored): the report
    (corrected[p, p], first[p, p], unlocated[p], first_unlocated[p]) and two
    images, (rebuilt with the survivors untouched, rebuilt with the located
    survivor bytes corrected). cols_by_stripe: {stripe: the columns that can
    be inconsistent}; other stripes are consistent."""
    p, e = codec.ranks, codec.encoding
    corrected, first = np.zeros((p, p), np.uint64), np.full((p, p), NO, np.uint64)
    unloc, first_un = np.zeros(p, np.uint64), np.full(p, NO, np.uint64)
    kept = oracle_rebuild(oracle, img, e, lost, chunk)  # unlocated and consistent columns: the plain rebuild
    for c, cols in cols_by_stripe.items():
        st = Stripe(oracle, codec, c, lost)
        corrected[c], first[c], unloc[c], first_un[c], (member, col, xs, v) = predict(st, img, chunk, cols)
        for i, r in enumerate(st.lost):
            kept[r, st.index[r], col] = v[i]
    fixed = kept.copy()
    for c, cols in cols_by_stripe.items():
        st = Stripe(oracle, codec, c, lost)
        _, _, _, _, (member, col, xs, v) = predict(st, img, chunk, cols)
        for m in np.unique(member):
            sel = member == m
            fixed[m, st.index[m], col[sel]] ^= xs[sel]
    return (corrected, first, unloc, first_un), kept, fixed


class Dev:
    """An image in one device tensor (spare bytes around it, sentinel-filled;
    `shift` moves the image off 16-B alignment)."""

    def __init__(self, img, chunk, e, shift=0):
        import torch

        self.torch = torch
        self.p, self.cells, self.stride = img.shape
        self.e, self.d, self.chunk = e, self.cells - e, chunk
        self.buf = torch.full((img.size + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.off = (-self.buf.data_ptr()) % 16 + 16 + shift
        self.upload(img)

    def upload(self, img):
        self.buf[self.off:self.off + img.size].copy_(self.torch.from_numpy(np.array(img).reshape(-1)))

    def download(self):
        self.torch.cuda.synchronize()
        return self.buf.cpu().numpy()

    def expect(self, img):
        want = np.full(self.buf.numel(), SENTINEL, np.uint8)
        want[self.off:self.off + img.size] = img.reshape(-1)
        return want

    def lofi(self):
        base = self.buf.data_ptr() + self.off
        return [base + r * self.cells * self.stride for r in range(self.p)]

    def parity(self):
        return [x + self.d * self.stride for x in self.lofi()]
