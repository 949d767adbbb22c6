"""NumPy model of the two-pass Strassen combine of the eigenvalue path (csrc/tbk_hk_dense.hip hk_strassen2_first_kernel and
hk_strassen2_close_kernel), CPU only.

The first pass takes the outer products p1 = 0 .. 5 -- in the kernel's order 0, 1, 3, 2, 4, 5, every quadrant leaving as soon
as it is final -- stores C12, C21 and C22 and parks the partial C11; the closing pass adds the quadrants of M7 (p1 = 6).  The
order of the terms inside every sum is that of the single pass, so the result must be that of combine2 of
test_strassen2_model.py bit for bit.  Stores honour the k bound the way the kernels do (rows >= nk are never written).
"""

import numpy as np
import pytest

from test_strassen2_model import combine2

FIRST_PASS_ORDER = (0, 1, 3, 2, 4, 5)  # hk_strassen2_first_kernel


def inner(P, p1):
    m1, m2, m3, m4, m5, m6, m7 = P[7 * p1:7 * p1 + 7]
    return [[((m1 + m4) - m5) + m7, m3 + m5], [m2 + m4, ((m1 - m2) + m3) + m6]]


def first_pass(P, mq, quarter, nk, C):
    """Stores the twelve finished quarter blocks into C[:nk]; returns the parked partial C11, part[2 a2 + c2]."""
    c = {}

    def store(a1, c1):
        for a2 in range(2):
            for c2 in range(2):
                aq, cq = 2 * a1 + a2, 2 * c1 + c2
                rows = max(0, min(mq, nk - aq * mq))  # kout = k' + aq Mq < nk
                C[aq * mq:aq * mq + rows, cq * quarter:(cq + 1) * quarter] = c[a1, c1, a2, c2][:rows]

    part = None
    for p1 in FIRST_PASS_ORDER:
        v = inner(P, p1)
        for a2 in range(2):
            for c2 in range(2):
                x = v[a2][c2]
                if p1 == 0:
                    c[0, 0, a2, c2] = x.copy()
                    c[1, 1, a2, c2] = x.copy()
                elif p1 == 1:
                    c[1, 0, a2, c2] = x.copy()
                    c[1, 1, a2, c2] -= x
                elif p1 == 2:
                    c[0, 1, a2, c2] = x.copy()
                    c[1, 1, a2, c2] += x
                elif p1 == 3:
                    c[0, 0, a2, c2] += x
                    c[1, 0, a2, c2] += x
                elif p1 == 4:
                    c[0, 0, a2, c2] -= x
                    c[0, 1, a2, c2] += x
                else:
                    c[1, 1, a2, c2] += x
        if p1 == 3:
            store(1, 0)
        if p1 == 4:
            store(0, 1)
            part = [c[0, 0, a2, c2].copy() for a2 in range(2) for c2 in range(2)]
        if p1 == 5:
            store(1, 1)
    return part


def closing_pass(P, part, mq, quarter, nk, C):
    v = inner(P, 6)
    for a2 in range(2):
        for c2 in range(2):
            rows = max(0, min(mq, nk - a2 * mq))
            C[a2 * mq:a2 * mq + rows, c2 * quarter:(c2 + 1) * quarter] = (part[2 * a2 + c2] + v[a2][c2])[:rows]


def combine2_two_passes(P, mq, quarter, nk):
    C = np.full((nk, 4 * quarter, 2), np.nan)  # every element must be stored by exactly the two passes
    part = first_pass(P, mq, quarter, nk, C)
    # the first pass leaves C11 alone, and nothing else is missing
    todo = np.isnan(C[..., 0])
    assert todo[:min(nk, 2 * mq), :2 * quarter].all() and todo.sum() == min(nk, 2 * mq) * 2 * quarter
    closing_pass(P, part, mq, quarter, nk, C)
    return C


def products(mq, quarter, seed):
    rng = np.random.default_rng(seed)
    # magnitudes spread over many binades: a changed association shows in the last bits
    return [rng.standard_normal((mq, quarter, 2)) * 10.0 ** rng.integers(-6, 7, size=(mq, quarter, 2)) for _ in range(49)]


# whole quarters; a ragged last quarter; a ragged third quarter and an empty fourth; one k-point
@pytest.mark.parametrize("mq,quarter,nk", [(128, 64, 512), (128, 64, 500), (128, 128, 259), (128, 64, 1), (256, 64, 769)])
def test_two_passes_equal_single_pass_bit_for_bit(mq, quarter, nk):
    P = products(mq, quarter, 1000 * mq + quarter + nk)
    single = combine2(P, mq, quarter)[:nk]
    two = combine2_two_passes(P, mq, quarter, nk)
    assert not np.isnan(two).any()
    assert np.array_equal(single.view(np.uint64), two.view(np.uint64))


def test_first_pass_reads_no_product_of_m7():
    """The first pass runs while products 42 .. 48 are still being computed: poisoning them must not change what it stores."""
    mq, quarter, nk = 128, 64, 400
    P = products(mq, quarter, 5)
    C0 = np.full((nk, 4 * quarter, 2), np.nan)
    part0 = first_pass(P, mq, quarter, nk, C0)
    Q = [p if i < 42 else np.full_like(p, np.inf) for i, p in enumerate(P)]
    C1 = np.full((nk, 4 * quarter, 2), np.nan)
    part1 = first_pass(Q, mq, quarter, nk, C1)
    assert np.array_equal(C0, C1, equal_nan=True)
    assert all(np.array_equal(x, y) for x, y in zip(part0, part1))

