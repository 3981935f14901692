"""Helper of the wide-repair tests (test_repair_wide_host.py,
test_gpu_repair_wide.py). Not a test module.

The reference is the undamaged set: a column with at most max_errors wrong
bytes has one right answer, the original bytes, so nothing here decodes. What
is computed is the syndrome of chosen errors, from the encoding matrix and the
cell numbering that repair_ref.Stripe takes, with the CPU oracle's products."""
import numpy as np


def syndrome(st, cols):
    """cols[p, n]: the members' bytes of n columns -> syndromes [e, n]."""
    S = np.zeros((st.e, cols.shape[1]), np.uint8)
    for m in range(st.p):
        if st.row[m] >= 0:
            S[st.row[m]] ^= cols[m]
        else:
            for j in range(st.e):
                S[j] ^= st.mul[st.A[j, m], cols[m]]
    return S


def syndrome_of(st, errors):
    """The e syndrome bytes of one column with errors [(member, value), ...]."""
    col = np.zeros((st.p, 1), np.uint8)
    for m, x in errors:
        col[m, 0] ^= x
    return syndrome(st, col)[:, 0].tolist()


def members_of(st):
    """(data members, parity members) of the stripe, ascending."""
    return [m for m in range(st.p) if st.row[m] < 0], [m for m in range(st.p) if st.row[m] >= 0]


def error_sets(st, nu, rng):
    """Sets of nu (member, value): one through member 0 or the first data
    member (point 0 where member 0 holds data), parity cells only, and mixed."""
    data, par = members_of(st)
    mix = lambda a, b: [m for pair in zip(a, b) for m in pair]  # noqa: E731
    picks = [data[:nu], par[:nu], mix(data, par[::-1])[:nu], mix(par[1:], data[1:])[:nu]]
    out = []
    for mem in picks:
        mem = sorted(set(mem))
        if len(mem) == nu:
            out.append([(m, int(x)) for m, x in zip(mem, rng.integers(1, 256, nu))])
    return out
