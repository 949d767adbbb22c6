"""NumPy model of the one-level Strassen contraction of the dense H(k) path, CPU only.

It mirrors the block algebra of csrc/tbk_phase.hip (phase_rows_strassen_kernel), csrc/tbk_stage.hip
(stage_strassen_kernel) and csrc/tbk_hk_dense.hip (launch_strassen, hk_strassen_finish_kernel): the padding of the
halves, the seven-entry table, the order of the combine, and the packed-slot map with diagonal pairs. It checks the
result against the classical product and against H(k) formed directly from the hoppings.
"""

import numpy as np
import pytest

BM, BK, BNP, CT = 128, 16, 64, 16
PAIR = 0x8000


def round_up(x, q):
    return (x + q - 1) // q * q


def colmap_pairs(n_orb):
    """Packed slots of a dense tight-binding model (tbk_api.hip create_common, pair_diagonal)."""
    cm = []
    for i in range(n_orb):
        if i % 2 == 0:
            cm.append((i << 16) | PAIR | (i + 1) if i + 1 < n_orb else (i << 16) | i)
        cm.extend((i << 16) | j for j in range(i + 1, n_orb))
    return cm


def stage(hop, n_r_pad, ncol_pad, cm):
    """Bt[2 n_r_pad][ncol_pad / 16][2][16] of tbk_stage.hip, as [K][slot][plane]."""
    n_r = hop.shape[0]
    B = np.zeros((2 * n_r_pad, ncol_pad, 2))
    for e, ij in enumerate(cm):
        i, j = ij >> 16, ij & 0x7FFF
        if ij & PAIR:
            B[0:2 * n_r:2, e, 0] = 2 * hop[:, i, i].real
            B[0:2 * n_r:2, e, 1] = 2 * hop[:, j, j].real
            B[1:2 * n_r:2, e, 0] = -2 * hop[:, i, i].imag
            B[1:2 * n_r:2, e, 1] = -2 * hop[:, j, j].imag
        else:
            h, g = hop[:, i, j], hop[:, j, i]
            B[0:2 * n_r:2, e, 0] = h.real + g.real
            B[0:2 * n_r:2, e, 1] = h.imag - g.imag
            B[1:2 * n_r:2, e, 0] = -(h.imag + g.imag)
            B[1:2 * n_r:2, e, 1] = h.real - g.real
    return B


def phases(k, R, nk_rows, n_r_pad):
    """A[2 n_r_pad][nk_rows]: cos / sin rows; k-points past len(k) and padding lattice vectors are 0."""
    A = np.zeros((2 * n_r_pad, nk_rows))
    x = 2 * np.pi * (k @ R.T)  # [nk][n_r]
    A[0:2 * len(R):2, :len(k)] = np.cos(x).T
    A[1:2 * len(R):2, :len(k)] = np.sin(x).T
    return A


def strassen(A, B, nk):
    """C[k][slot][plane] from the seven half-size products; A is [K][2 Mh], B is [K][ncol_pad][2]."""
    K, ncol_pad = B.shape[0], B.shape[1]
    kh, half, mh = K // 2, ncol_pad // 2, A.shape[1] // 2
    P = [[A[b * kh:(b + 1) * kh, a * mh:(a + 1) * mh] for b in range(2)] for a in range(2)]  # P[a][b] is K-half b x k-half a
    Bq = [[B[b * kh:(b + 1) * kh, c * half:(c + 1) * half] for c in range(2)] for b in range(2)]
    (p11, p12), (p21, p22) = P
    (b11, b12), (b21, b22) = Bq
    As = [p11 + p22, p21 + p22, p11, p22, p11 + p12, p21 - p11, p12 - p22]  # tbk_phase.hip order
    Bs = [b11 + b22, b11, b12 - b22, b21 - b11, b22, b11 + b12, b21 + b22]  # tbk_stage.hip order
    M = [np.einsum("km,ken->men", a_, b_) for a_, b_ in zip(As, Bs)]
    m1, m2, m3, m4, m5, m6, m7 = M
    C = np.zeros((2 * mh, ncol_pad, 2))
    C[:mh, :half] = ((m1 + m4) - m5) + m7
    C[:mh, half:] = m3 + m5
    C[mh:, :half] = m2 + m4
    C[mh:, half:] = ((m1 - m2) + m3) + m6
    return C[:nk]


def unpack(C, cm, n_orb):
    """H[k][i][j] (Hermitian, FULL mode) from the packed slots -- store_slot of tbk_hk_dense.hip."""
    H = np.zeros((C.shape[0], n_orb, n_orb), complex)
    for e, ij in enumerate(cm):
        i, j = ij >> 16, ij & 0x7FFF
        if ij & PAIR:
            H[:, i, i] = C[:, e, 0]
            H[:, j, j] = C[:, e, 1]
        else:
            H[:, i, j] = C[:, e, 0] + 1j * C[:, e, 1]
            H[:, j, i] = C[:, e, 0] - 1j * C[:, e, 1]
    return H


@pytest.mark.parametrize("n_orb,n_r,nk", [(5, 37, 301), (4, 16, 256), (7, 50, 129), (13, 23, 1), (9, 40, 3)])
def test_strassen_block_algebra_matches_classical(n_orb, n_r, nk):
    rng = np.random.default_rng(n_orb * 1000 + n_r + nk)
    R = rng.integers(-4, 5, size=(n_r, 3))
    hop = rng.standard_normal((n_r, n_orb, n_orb)) + 1j * rng.standard_normal((n_r, n_orb, n_orb))
    k = rng.random((nk, 3)) * 4 - 2
    cm = colmap_pairs(n_orb)
    n_r_pad = round_up(n_r, BK)  # K / 2 = n_r_pad rows: whole stages in each half
    ncol_pad = round_up(len(cm), 2 * BNP)  # whole 64-slot tiles in each half
    cm_pad = cm + [-1] * (ncol_pad - len(cm))
    assert n_r_pad % BK == 0 and (ncol_pad // 2) % BNP == 0
    B = stage(hop, n_r_pad, ncol_pad, cm_pad[: len(cm)])
    mh = round_up((nk + 1) // 2, BM)
    assert 2 * mh >= nk
    A = phases(k, R, 2 * mh, n_r_pad)
    classical = np.einsum("km,ken->men", A, B)[:nk]
    fast = strassen(A, B, nk)
    scale = np.abs(classical).max()
    assert np.abs(fast - classical).max() <= 1e-13 * scale
    # (padding slots of the right half are NOT exactly zero: C22 = M1 - M2 + M3 + M6 cancels left-half terms at rounding
    # level -- the combine skips them through colmap < 0)
    assert np.abs(fast[:, len(cm):]).max() <= 1e-13 * scale
    # and the unpacked result is H(k) of the hoppings: sum_R e^{2 pi i k.R} (h_R + h_{-R}^dagger), written as p h + conj(p) h^H
    H = unpack(fast, cm, n_orb)
    p = np.exp(2j * np.pi * (k @ R.T))
    ref = np.einsum("kr,rij->kij", p, hop)
    ref = ref + ref.conj().transpose(0, 2, 1)
    assert np.abs(H - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.all(np.diagonal(H, axis1=1, axis2=2).imag == 0)


def test_strassen_padded_k_rows_add_nothing():
    """Padded k rows carry phase 0 (not cos 0 = 1): the second half's padding must not leak into the first half."""
    rng = np.random.default_rng(7)
    n_orb, n_r, nk = 3, 20, 131  # Mh = 128: the second half holds 3 real k-points and 125 padding rows
    R = rng.integers(-3, 4, size=(n_r, 2))
    hop = rng.standard_normal((n_r, n_orb, n_orb)) + 1j * rng.standard_normal((n_r, n_orb, n_orb))
    k = rng.random((nk, 2))
    cm = colmap_pairs(n_orb)
    n_r_pad, ncol_pad = round_up(n_r, BK), round_up(len(cm), 2 * BNP)
    B = stage(hop, n_r_pad, ncol_pad, cm)
    mh = round_up((nk + 1) // 2, BM)
    A = phases(k, R, 2 * mh, n_r_pad)
    assert not A[:, nk:].any()
    fast = strassen(A, B, nk)
    one = strassen(phases(k[:1], R, 2 * mh, n_r_pad), B, 1)
    assert np.abs(fast[:1] - one).max() <= 1e-13 * np.abs(one).max()
