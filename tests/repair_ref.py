"""Brute-force numpy oracle of column-wise locate and repair, shared by the
repair tests (test_repair_host.py, test_gpu_repair*.py). Not a test module.

Nothing here comes from the code under test but the encoding matrix and the
cell numbering (codec.matrix(), encoding_id / data_id, themselves pinned
against the CPU oracle by tests/test_abi.py): the GF product is the CPU
oracle's, and the verdict on a byte column is found by trying, for each of the
p members, every byte value 1..255 as that member's error and accepting only a
unique member."""
import numpy as np

NO = (1 << 64) - 1

_mul = {}


def mul_table(oracle):
    """MUL[a, b] = a * b over GF(2^8), every product asked of the CPU oracle."""
    if "t" not in _mul:
        rs = oracle.OracleRS(4, 2)
        t = np.zeros((256, 256), np.uint8)
        for a in range(1, 256):
            for b in range(a, 256):
                t[a, b] = t[b, a] = rs.mult(a, b)
        _mul["t"] = t
    return _mul["t"]


class Stripe:
    """Stripe c of an RS(p, e) set: which cell each member holds, the parity
    coefficients, and for each member the 255 syndromes its single wrong byte
    can give (packed: row j in bits 8j)."""

    def __init__(self, oracle, codec, c):
        p, e = codec.ranks, codec.encoding
        self.p, self.e, self.d, self.c = p, e, p - e, c
        self.mul = mul_table(oracle)
        self.A = codec.matrix()[p:, :]  # [e, p]
        self.row = [-1] * p     # parity row the member holds, or -1
        self.index = [0] * p    # the member's cell among its d data + e parity cells
        for m in range(p):
            enc = codec.encoding_id(m, c)
            if enc < p:
                self.index[m] = codec.data_id(m, c)
            else:
                self.row[m] = enc - p
                self.index[m] = self.d + enc - p
        x = np.arange(1, 256)
        self.keys = []  # per member: packed syndrome of error value x, x = 1..255
        for m in range(p):
            k = np.zeros(255, np.uint32)
            for j in range(e):
                sj = self.mul[self.A[j, m], x] if self.row[m] < 0 else (x if j == self.row[m] else 0 * x)
                k |= sj.astype(np.uint32) << np.uint32(8 * j)
            self.keys.append(k)

    def kind(self, m):
        return "data" if self.row[m] < 0 else "parity"

    def syndrome(self, cols):
        """cols[p, n]: the members' bytes of n columns -> packed syndromes [n]."""
        S = np.zeros(cols.shape[1], np.uint32)
        for m in range(self.p):
            for j in range(self.e):
                if self.row[m] < 0:
                    S ^= self.mul[self.A[j, m], cols[m]].astype(np.uint32) << np.uint32(8 * j)
                elif self.row[m] == j:
                    S ^= cols[m].astype(np.uint32) << np.uint32(8 * j)
        return S

    def locate(self, S):
        """(member[n], x[n]): the unique member one of whose 255 error values
        gives the packed syndrome, and that value; member -1 where the column
        is clean or no member, or more than one, explains it."""
        hits = np.zeros(S.shape, np.int64)
        member = np.full(S.shape, -1, np.int64)
        xs = np.zeros(S.shape, np.uint8)
        for m in range(self.p):
            order = np.argsort(self.keys[m], kind="stable")
            sk = self.keys[m][order]
            pos = np.minimum(np.searchsorted(sk, S), 254)
            ok = (sk[pos] == S) & (S != 0)
            hits += ok
            member[ok] = m
            xs[ok] = (order[pos[ok]] + 1).astype(np.uint8)
        bad = hits != 1
        member[bad] = -1
        xs[bad] = 0
        return member, xs


def miscorrecting_pair(st, a, b):
    """(x1, x2, t, x3): error values of members a and b in one column whose
    syndrome is also that of member t's error x3 alone -- the miscorrection a
    code of distance 3 (e = 2) cannot avoid. None if there is none."""
    for x1 in range(1, 256):
        S = st.keys[a][x1 - 1] ^ st.keys[b]
        member, xs = st.locate(S)
        hit = np.nonzero(member >= 0)[0]
        if hit.size:
            x2 = int(hit[0]) + 1
            return x1, x2, int(member[hit[0]]), int(xs[hit[0]])
    return None


def unpack(S, e):
    return [[(int(s) >> (8 * j)) & 255 for j in range(e)] for s in S]


def predict(st, image, chunk, cols=None):
    """What a repair of stripe st must do to `image` ([p, d + e, stride] host
    bytes): (corrected[p], first[p], unlocated, first_unlocated, fixes) with
    fixes = (member[k], col[k], x[k]). `cols`: the only columns that can be
    nonzero (default: all are examined)."""
    cols = np.arange(chunk) if cols is None else np.unique(np.asarray(cols, np.int64))
    by = np.stack([image[m, st.index[m], cols] for m in range(st.p)])
    S = st.syndrome(by)
    member, xs = st.locate(S)
    corrected = np.zeros(st.p, np.uint64)
    first = np.full(st.p, NO, np.uint64)
    for m in range(st.p):
        mine = cols[member == m]
        if mine.size:
            corrected[m] = mine.size
            first[m] = mine.min()
    un = cols[(S != 0) & (member < 0)]
    fix = member >= 0
    return corrected, first, int(un.size), (int(un.min()) if un.size else NO), (member[fix], cols[fix], xs[fix])


def apply_fixes(st, image, fixes):
    member, cols, xs = fixes
    for m in np.unique(member):
        sel = member == m
        image[m, st.index[m], cols[sel]] ^= xs[sel]
