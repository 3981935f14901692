"""Brute-force numpy oracle of repair with up to two wrong bytes per column
(e = 4), shared by test_repair2_host.py and test_gpu_repair2.py. Not a test
module.

As in repair_ref.py nothing comes from the code under test but the encoding
matrix and the cell numbering. The verdict on a packed syndrome S != 0 is the
unique single member that explains it (repair_ref.Stripe.locate) or, failing
that, the unique pair (a, x1), (b, x2), a < b, with keys[a][x1] ^ keys[b][x2]
== S, found by looking S ^ (every member's every error) up in the sorted list
of every member's every error; anything else is unlocated."""
import numpy as np

from repair_ref import NO


def locate2(st, S):
    """Per column of the packed syndromes S[n]: [] (clean or unlocated), or
    the one or two (member, x) that explain it, ascending by member."""
    S = np.asarray(S, np.uint32)
    member, xs = st.locate(S)
    flat = np.concatenate(st.keys)  # entry 255 m + (x - 1)
    order = np.argsort(flat, kind="stable")
    sk = flat[order]
    out = []
    for i, s in enumerate(S):
        if member[i] >= 0:
            out.append([(int(member[i]), int(xs[i]))])
            continue
        out.append([])
        if s == 0:
            continue
        want = s ^ flat
        pos = np.minimum(np.searchsorted(sk, want), sk.size - 1)
        a = np.nonzero(sk[pos] == want)[0]
        b = order[pos[a]]
        keep = a // 255 < b // 255
        a, b = a[keep], b[keep]
        if a.size == 1:
            out[-1] = [(int(a[0]) // 255, int(a[0]) % 255 + 1), (int(b[0]) // 255, int(b[0]) % 255 + 1)]
    return out


def predict(st, image, chunk, cols):
    """What a two-error repair of stripe st must do to `image` ([p, d + e,
    stride] host bytes) given the only columns that can be nonzero:
    (corrected[p], first[p], unlocated, first_unlocated, pair_columns) and the
    fixes [(member, col, x)]."""
    cols = np.unique(np.asarray(cols, np.int64))
    S = st.syndrome(np.stack([image[m, st.index[m], cols] for m in range(st.p)]))
    corrected, first = np.zeros(st.p, np.uint64), np.full(st.p, NO, np.uint64)
    un, pairs, fixes = [], 0, []
    for col, s, verdict in zip(cols, S, locate2(st, S)):
        if s and not verdict:
            un.append(int(col))
        pairs += len(verdict) == 2
        for m, x in verdict:
            corrected[m] += 1
            first[m] = min(int(first[m]), int(col))
            fixes.append((m, int(col), x))
    return (corrected, first, len(un), min(un) if un else NO, pairs), fixes


def apply_fixes(st, image, fixes):
    for m, col, x in fixes:
        image[m, st.index[m], col] ^= x
