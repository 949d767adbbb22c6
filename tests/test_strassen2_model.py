"""NumPy model of the two-level Strassen contraction of the dense H(k) path, CPU only.

It mirrors csrc/tbk_phase.hip (phase_rows_strassen2_kernel: the 16 quadrant phases, the outer table quadrant by quadrant, the
inner table of each), csrc/tbk_stage.hip (tbk_stage_strassen2: the table on the halves of Bt, then on the quadrants of each
block), and csrc/tbk_hk_dense.hip (launch_strassen2: 49 quarter-size products; hk_strassen2_finish_kernel: the streaming
combine with 16 accumulators).  "The same association as the nested form" is checked as it is meant: bit for bit against the
one-level model of test_strassen_model.py applied to each of its own seven products.
"""

import numpy as np
import pytest

from test_strassen_model import BK, BM, BNP, colmap_pairs, phases, round_up, stage, strassen, unpack


def left_table(v):
    """The seven left operands from quadrants v[k half][K half] (tbk_phase.hip strassen_left)."""
    return [v[0][0] + v[1][1], v[1][0] + v[1][1], v[0][0], v[1][1], v[0][0] + v[0][1], v[1][0] - v[0][0], v[0][1] - v[1][1]]


def right_table(b):
    """The seven right operands from quadrants b[K half][slot half] (tbk_stage.hip stage_strassen_kernel)."""
    return [b[0][0] + b[1][1], b[0][0], b[0][1] - b[1][1], b[1][0] - b[0][0], b[1][1], b[0][0] + b[0][1], b[1][0] + b[1][1]]


def left_operands2(A, mq):
    """As2[49]: A is [K][4 Mq]; quarter 2 a1 + a2 of the k-points, 2 b1 + b2 of the K rows."""
    kq = A.shape[0] // 4
    q = [[A[b * kq:(b + 1) * kq, a * mq:(a + 1) * mq] for b in range(4)] for a in range(4)]  # q[k quarter][K quarter]
    outer = [[left_table([[q[a2][b2], q[a2][2 + b2]], [q[2 + a2][b2], q[2 + a2][2 + b2]]]) for b2 in range(2)] for a2 in range(2)]
    out = []
    for p1 in range(7):
        out.extend(left_table([[outer[0][0][p1], outer[0][1][p1]], [outer[1][0][p1], outer[1][1][p1]]]))
    return out


def right_operands2(B):
    """Bs2[49]: the table on the halves of B [K][ncol_pad][2], then on the quadrants of each of the seven blocks."""
    def quadrants(x):
        kh, half = x.shape[0] // 2, x.shape[1] // 2
        return [[x[b * kh:(b + 1) * kh, c * half:(c + 1) * half] for c in range(2)] for b in range(2)]

    out = []
    for block in right_table(quadrants(B)):
        out.extend(right_table(quadrants(block)))
    return out


def combine2(P, mq, quarter):
    """hk_strassen2_finish_kernel: walk p1 = 1 .. 7, finish M_p1's quadrants, accumulate them into the outer C11 .. C22."""
    c = {}
    for p1 in range(7):
        m1, m2, m3, m4, m5, m6, m7 = P[7 * p1:7 * p1 + 7]
        inner = [[((m1 + m4) - m5) + m7, m3 + m5], [m2 + m4, ((m1 - m2) + m3) + m6]]
        for a2 in range(2):
            for c2 in range(2):
                v = inner[a2][c2]
                if p1 == 0:
                    c[0, 0, a2, c2] = v.copy()
                    c[1, 1, a2, c2] = v.copy()
                elif p1 == 1:
                    c[1, 0, a2, c2] = v.copy()
                    c[1, 1, a2, c2] -= v
                elif p1 == 2:
                    c[0, 1, a2, c2] = v.copy()
                    c[1, 1, a2, c2] += v
                elif p1 == 3:
                    c[0, 0, a2, c2] += v
                    c[1, 0, a2, c2] += v
                elif p1 == 4:
                    c[0, 0, a2, c2] -= v
                    c[0, 1, a2, c2] += v
                elif p1 == 5:
                    c[1, 1, a2, c2] += v
                else:
                    c[0, 0, a2, c2] += v
    C = np.zeros((4 * mq, 4 * quarter, 2))
    for (a1, c1, a2, c2), v in c.items():
        aq, cq = 2 * a1 + a2, 2 * c1 + c2
        C[aq * mq:(aq + 1) * mq, cq * quarter:(cq + 1) * quarter] = v
    return C


def strassen2(A, B, nk):
    """C[k][slot][plane] from the 49 quarter-size products; A is [K][4 Mq], B is [K][ncol_pad][2]."""
    mq, quarter = A.shape[1] // 4, B.shape[1] // 4
    P = [np.einsum("km,ken->men", a_, b_) for a_, b_ in zip(left_operands2(A, mq), right_operands2(B))]
    assert len(P) == 49 and P[0].shape == (mq, quarter, 2)
    return combine2(P, mq, quarter)[:nk]


def nested(A, B, nk):
    """The one-level model applied to each of its own seven products (halves of 2 Mq k-points)."""
    kh, half, mh = B.shape[0] // 2, B.shape[1] // 2, A.shape[1] // 2
    (p11, p12), (p21, p22) = [[A[b * kh:(b + 1) * kh, a * mh:(a + 1) * mh] for b in range(2)] for a in range(2)]
    (b11, b12), (b21, b22) = [[B[b * kh:(b + 1) * kh, c * half:(c + 1) * half] for c in range(2)] for b in range(2)]
    As = [p11 + p22, p21 + p22, p11, p22, p11 + p12, p21 - p11, p12 - p22]
    Bs = [b11 + b22, b11, b12 - b22, b21 - b11, b22, b11 + b12, b21 + b22]
    m1, m2, m3, m4, m5, m6, m7 = [strassen(a_, b_, mh) for a_, b_ in zip(As, Bs)]
    C = np.zeros((2 * mh, 2 * half, 2))
    C[:mh, :half] = ((m1 + m4) - m5) + m7
    C[:mh, half:] = m3 + m5
    C[mh:, :half] = m2 + m4
    C[mh:, half:] = ((m1 - m2) + m3) + m6
    return C[:nk]


def operands(n_orb, n_r, nk, dim, seed):
    rng = np.random.default_rng(seed)
    R = rng.integers(-4, 5, size=(n_r, dim))
    hop = rng.standard_normal((n_r, n_orb, n_orb)) + 1j * rng.standard_normal((n_r, n_orb, n_orb))
    k = rng.random((nk, dim)) * 4 - 2
    cm = colmap_pairs(n_orb)
    n_r_pad = round_up(n_r, 2 * BK)  # K / 4 = n_r_pad / 2 rows: whole stages in each quarter
    ncol_pad = round_up(len(cm), 4 * BNP)  # whole 64-slot tiles in each quarter
    assert (2 * n_r_pad // 4) % BK == 0 and (ncol_pad // 4) % BNP == 0
    mq = round_up((nk + 3) // 4, BM)  # tbk_strassen_mq
    assert 4 * mq >= nk
    return R, hop, k, cm, stage(hop, n_r_pad, ncol_pad, cm), phases(k, R, 4 * mq, n_r_pad), mq


# (the existing file's shapes, and 257 k-points: Mq = 128, quarters of 128, 128, 1 and 0 k-points -- the last one only padding)
@pytest.mark.parametrize("n_orb,n_r,nk", [(5, 37, 301), (4, 16, 256), (7, 50, 129), (13, 23, 1), (9, 40, 3), (6, 30, 257)])
def test_two_levels_match_nested_form_and_classical(n_orb, n_r, nk):
    R, hop, k, cm, B, A, mq = operands(n_orb, n_r, nk, 3, n_orb * 1000 + n_r + nk)
    fast = strassen2(A, B, nk)
    assert np.array_equal(fast, nested(A, B, nk))  # the same association: the same bits
    classical = np.einsum("km,ken->men", A, B)[:nk]
    scale = np.abs(classical).max()
    assert np.abs(fast - classical).max() <= 1e-13 * scale
    H = unpack(fast, cm, n_orb)
    p = np.exp(2j * np.pi * (k @ R.T))
    ref = np.einsum("kr,rij->kij", p, hop)
    ref = ref + ref.conj().transpose(0, 2, 1)
    assert np.abs(H - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.all(np.diagonal(H, axis1=1, axis2=2).imag == 0)


def test_two_levels_padded_k_rows_add_nothing():
    """Padded k rows carry phase 0 (not cos 0 = 1): the padding of the later quarters must not leak into the first."""
    n_orb, n_r, nk = 3, 20, 259  # Mq = 128: the third quarter holds 3 real k-points, the fourth none
    R, hop, k, cm, B, A, mq = operands(n_orb, n_r, nk, 2, 7)
    assert mq == 128 and not A[:, nk:].any()
    fast = strassen2(A, B, nk)
    one = strassen2(phases(k[:1], R, 4 * mq, A.shape[0] // 2), B, 1)
    assert np.abs(fast[:1] - one).max() <= 1e-13 * np.abs(one).max()
