"""
The lattice Berry flux and the Chern numbers of a uniform k mesh (Fukui, Hatsugai, Suzuki 2005), stated in NumPy: what
csrc/tbk_berry.hip computes and what the tests compare it with.  DESIGN.md section 18 has the derivations.

Mesh and mesh points are those of ``Model.occupations``: ``k = (i_1 / n_1, ..., i_dim / n_dim)`` in mesh order (last axis fastest),
``dim`` 2 or 3, and ``k+e_d`` is the point with index ``(i_d + 1) mod n_d``.  ``U[k][i][b]`` are eigenvectors in convention 2.
``D(e_d)`` is 1 for convention 2 and ``exp(-2 pi i pos[i][d] / n_d)`` for convention 1 (``chi_model.phase_table`` for ``q = e_d``).
A band set is a half-open range ``[lo, hi)``, ``m = hi - lo``.  For every set, axis ``d`` and mesh point ``k``::

    M_d(k)     = U[k][:, lo:hi]^H  D(e_d)  U[k+e_d][:, lo:hi]                       (m x m)
    L_d(k)     = det M_d(k)          LU with partial pivoting: the pivot is the largest |Re| + |Im|, a tie goes to the lowest row
    a_d(k)     = round(arg L_d(k) / (2 pi) * 2^64) mod 2^64                         the uint64 angle word; arg 0 = 0 for L = 0
    F_ab(k)    = a_a(k) + a_b(k+e_a) - a_a(k+e_b) - a_b(k)                          wrapping 64-bit arithmetic, read as int64; a < b
    flux_ab(k) = float(F_ab(k)) * (2 pi 2^-64)
    C_ab(i_c)  = (sum over the plane's k of F_ab(k)) / 2^64                         one integer per index of the remaining axis c

Planes in the order (0,1), (0,2), (1,2).  Every word enters the sum of a closed plane once with each sign, so the sum of the wrapped
plaquettes is 0 modulo 2^64: the low word of the 128-bit sum is identically zero and C is an integer without rounding.

Sign.  ``arg L_d(k) ~ -A_d(k) / n_d`` with the Berry connection ``A_d = i tr <u| d/dk_d |u>``, so ``flux_ab ~ -Omega_ab / (n_a n_b)`` with
``Omega_ab = d_a A_b - d_b A_a``, and ``C_ab = -(1 / 2 pi) int Omega_ab``.  The lower band of the Qi-Wu-Zhang model
``sin K_x sigma_x + sin K_y sigma_y + (u + cos K_x + cos K_y) sigma_z`` has C = +1 for 0 < u < 2 and -1 for -2 < u < 0.
"""

import itertools

import numpy as np

TWO_PI = 2.0 * np.pi
TURN = float(np.ldexp(TWO_PI, -64))  # radians per unit of an angle word: (double)F * TURN is the flux
PLANES = {2: ((0, 1),), 3: ((0, 1), (0, 2), (1, 2))}


def mesh_shape(mesh):
    shape = tuple(int(n) for n in mesh)
    if len(shape) not in (2, 3) or min(shape) < 1:
        raise ValueError("mesh must have 2 or 3 positive entries")
    return shape


def band_sets(bands, n):
    """``[(lo, hi), ...]`` from an int ``n_occ`` (``[(0, n_occ)]``) or a sequence of pairs; 1 to 16 sets inside ``[0, n]``."""
    if isinstance(bands, (int, np.integer)) and not isinstance(bands, (bool, np.bool_)):
        bands = [(0, int(bands))]
    sets = [(int(lo), int(hi)) for lo, hi in bands]
    if not 1 <= len(sets) <= 16:
        raise ValueError("1 to 16 band sets")
    for lo, hi in sets:
        if lo < 0 or hi > n or lo >= hi:
            raise ValueError("a band set must satisfy 0 <= lo < hi <= n")
    return sets


def remaining_axis(dim, plane):
    """The axis c a plane (a, b) leaves over, or None in two dimensions."""
    rest = [d for d in range(dim) if d not in plane]
    return rest[0] if rest else None


def phase_table(mesh, pos):
    """D[dim][n] of convention 1: row d is exp(-2 pi i pos[i][d] / n_d), chi_model.phase_table's row for q = e_d."""
    shape = mesh_shape(mesh)
    pos = np.asarray(pos, dtype=float)
    angle = np.zeros((len(shape), pos.shape[0]))
    for d, n_d in enumerate(shape):
        angle[d] = -TWO_PI * ((1.0 * pos[:, d]) / float(n_d))
    return np.cos(angle) + 1j * np.sin(angle)


def _on_mesh(U, mesh):
    shape = mesh_shape(mesh)
    U = np.asarray(U)
    n = U.shape[-1]
    return U.reshape(shape + (n, n)), shape, n


def link_matrices(U, mesh, d, lo, hi, phases=None):
    """M_d(k) for every mesh point: complex [NK][m][m].  phases: D[dim][n] or None."""
    grid, shape, n = _on_mesh(U, mesh)
    here = grid[..., :, lo:hi]
    there = np.roll(grid, -1, axis=d)[..., :, lo:hi]
    if phases is not None:
        there = np.asarray(phases)[d][:, None] * there
    prod = np.einsum("...ib,...ic->...bc", here.conj(), there)
    return prod.reshape((-1, hi - lo, hi - lo))


def lu_det(M):
    """det of every matrix of M [B][m][m] by the textbook LU with partial pivoting, the pivot the largest |Re| + |Im| of the column
    from the diagonal down, a tie to the lowest row; a zero pivot gives 0."""
    A = np.array(M, dtype=np.complex128)
    count, m = A.shape[0], A.shape[1]
    det = np.ones(count, dtype=np.complex128)
    rows = np.arange(count)
    for j in range(m):
        size = np.abs(A[:, j:, j].real) + np.abs(A[:, j:, j].imag)
        p = j + np.argmax(size, axis=1)  # (argmax takes the first of equals: the lowest row)
        swap = p != j
        top, low = A[rows, j].copy(), A[rows, p].copy()
        A[rows, j], A[rows, p] = low, top
        pivot = A[:, j, j]
        det = det * np.where(swap, -pivot, pivot)
        safe = np.where(pivot == 0.0, 1.0, pivot)
        factor = A[:, j + 1:, j] / safe[:, None]
        A[:, j + 1:, j + 1:] -= factor[:, :, None] * A[:, j, None, j + 1:]
    return det


def links(U, mesh, ranges, phases=None):
    """L complex [S][dim][NK]."""
    shape = mesh_shape(mesh)
    out = np.empty((len(ranges), len(shape), int(np.prod(shape))), dtype=np.complex128)
    for s, (lo, hi) in enumerate(ranges):
        for d in range(len(shape)):
            out[s, d] = lu_det(link_matrices(U, mesh, d, lo, hi, phases))
    return out


def sigma_min(U, mesh, ranges, phases=None):
    """The smallest singular value of the M of every set: float [S]."""
    shape = mesh_shape(mesh)
    out = np.empty(len(ranges))
    for s, (lo, hi) in enumerate(ranges):
        out[s] = min(np.linalg.svd(link_matrices(U, mesh, d, lo, hi, phases), compute_uv=False).min() for d in range(len(shape)))
    return out


def angle_words(L):
    """a = round(arg L / (2 pi) 2^64) mod 2^64 as uint64; 0 for L = 0."""
    L = np.asarray(L, dtype=np.complex128)
    turns = np.arctan2(L.imag, L.real) / TWO_PI
    turns = np.where((L.real == 0.0) & (L.imag == 0.0), 0.0, turns)
    scaled = np.rint(np.ldexp(turns, 64))  # in [-2^63, 2^63]: whole numbers
    size = np.abs(scaled).astype(np.uint64)
    return np.where(scaled < 0.0, np.uint64(0) - size, size).astype(np.uint64)


def word_angles(words):
    """The angle in [-pi, pi) an angle word stands for."""
    return np.asarray(words, dtype=np.uint64).view(np.int64).astype(np.float64) * TURN


def wrapped_difference(a, b):
    """|a - b| of two angles in radians modulo 2 pi, in [0, pi]."""
    diff = np.mod(np.asarray(a) - np.asarray(b) + np.pi, TWO_PI) - np.pi
    return np.abs(diff)


def plaquettes(words, mesh):
    """F int64 [S][P][NK] from words uint64 [S][dim][NK], in wrapping 64-bit arithmetic."""
    shape = mesh_shape(mesh)
    dim = len(shape)
    words = np.asarray(words, dtype=np.uint64)
    sets = words.shape[0]
    grid = words.reshape((sets, dim) + shape)
    out = np.empty((sets, len(PLANES[dim]), int(np.prod(shape))), dtype=np.int64)
    for p, (a, b) in enumerate(PLANES[dim]):
        wa, wb = grid[:, a], grid[:, b]
        total = wa + np.roll(wb, -1, axis=1 + a) - np.roll(wa, -1, axis=1 + b) - wb  # (uint64 arrays wrap)
        out[:, p] = total.view(np.int64).reshape(sets, -1)
    return out


def plane_sums(F, mesh):
    """The exact sums of F over every plane: a list of P arrays of Python integers (object dtype) of shape (S, n_c)."""
    shape = mesh_shape(mesh)
    dim = len(shape)
    F = np.asarray(F, dtype=np.int64)
    sets = F.shape[0]
    sums = []
    for p, plane in enumerate(PLANES[dim]):
        grid = F[:, p].reshape((sets,) + shape)
        high, low = grid >> 32, grid & 0xFFFFFFFF  # (fewer than 2^31 points: neither sum overflows)
        axes = tuple(1 + d for d in plane)
        total = high.sum(axis=axes).astype(object) * (1 << 32) + low.sum(axis=axes).astype(object)
        sums.append(total.reshape(sets, -1))
    return sums


def flux_from_words(words, mesh):
    """(flux float64 [S][P][NK], chern: list of P arrays int64 (S, n_c), low: the low words of the sums, all 0)."""
    F = plaquettes(words, mesh)
    sums = plane_sums(F, mesh)
    chern = [np.array([[int(v) >> 64 for v in row] for row in total], dtype=np.int64) for total in sums]
    low = [np.array([[int(v) & ((1 << 64) - 1) for v in row] for row in total], dtype=np.uint64) for total in sums]
    return F.astype(np.float64) * TURN, chern, low


def chern_flat(chern):
    """int64 (S, sum of n_c): the planes side by side, the layout of the C interface."""
    return np.ascontiguousarray(np.concatenate(chern, axis=1))


def link_tolerance(n, m, smallest):
    """The angle error of one link in radians for n orbitals, a set of m bands and the smallest singular value of M."""
    return ((n + 8.0 * m) * m / smallest + 8.0) * 2.0 ** -53


def berry_flux(U, mesh, bands, phases=None):
    """The whole quantity on eigenvectors U: dict with sets, planes, L, words, flux [S][P][NK], chern (list of P), low, link_min [S]."""
    _, shape, n = _on_mesh(U, mesh)
    sets = band_sets(bands, n)
    L = links(U, mesh, sets, phases)
    words = angle_words(L)
    flux, chern, low = flux_from_words(words, mesh)
    return {"sets": sets, "planes": PLANES[len(shape)], "L": L, "words": words, "flux": flux, "chern": chern, "low": low,
            "link_min": np.abs(L).reshape(len(sets), -1).min(axis=1)}


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
SIGMA = (np.array([[0, 1], [1, 0]], dtype=complex), np.array([[0, -1j], [1j, 0]], dtype=complex), np.array([[1, 0], [0, -1]], dtype=complex))


def qwz_hoppings(u, dim=2):
    """The Qi-Wu-Zhang model as half-space hoppings {R: matrix} (the R = 0 block stored halved, as ``contains_cc=False`` takes it):
    H = sin K_x sigma_x + sin K_y sigma_y + (u + cos K_x + cos K_y [+ cos K_z]) sigma_z, K = 2 pi k."""
    sx, sy, sz = SIGMA
    zero = (0,) * dim
    hop = {zero: u * sz / 2.0, (1, 0) + (0,) * (dim - 2): sz / 2.0 - 0.5j * sx, (0, 1) + (0,) * (dim - 2): sz / 2.0 - 0.5j * sy}
    if dim == 3:
        hop[(0, 0, 1)] = sz / 2.0
    return hop


def mesh_points(mesh):
    shape = mesh_shape(mesh)
    return np.array(list(itertools.product(*[range(n) for n in shape])), dtype=float).reshape(-1, len(shape)) / np.array(shape, dtype=float)


def hamiltonians(hop, k):
    """H(k) of half-space hoppings in convention 2: sum_R exp(2 pi i k.R) hop[R] + h.c."""
    k = np.asarray(k, dtype=float)
    size = next(iter(hop.values())).shape[0]
    H = np.zeros((k.shape[0], size, size), dtype=complex)
    for R, mat in hop.items():
        H += np.exp(TWO_PI * 1j * (k @ np.array(R, dtype=float)))[:, None, None] * np.asarray(mat)[None]
    return H + np.conj(np.swapaxes(H, 1, 2))


def eigenvectors(hop, mesh):
    """U [NK][n][n] of numpy.linalg.eigh on the mesh points."""
    return np.linalg.eigh(hamiltonians(hop, mesh_points(mesh)))[1]


def random_phases(dim, n, spread, seed):
    """A table D[dim][n] of unit phases with angles uniform in [-spread, spread]: what convention 1 gives for positions of that size
    (in units of the mesh step); small enough that the links of smooth_unitaries stay well conditioned."""
    angle = np.random.default_rng(seed).uniform(-spread, spread, (dim, n))
    return np.ascontiguousarray(np.cos(angle) + 1j * np.sin(angle))


def smooth_unitaries(mesh, n, amplitude, seed):
    """U(k) = exp(i G(k)) with a first-harmonic Hermitian field G(k) = A_0 + sum_d (A_d exp(2 pi i k_d) + h.c.), the A random with
    entries of the size amplitude / sqrt(n): periodic, smooth, and close enough to 1 that every link is well conditioned."""
    shape = mesh_shape(mesh)
    rng = np.random.default_rng(seed)
    scale = amplitude / np.sqrt(n)
    coeff = [scale * (rng.normal(size=(n, n)) + 1j * rng.normal(size=(n, n))) for _ in range(len(shape) + 1)]
    k = mesh_points(mesh)
    G = np.zeros((k.shape[0], n, n), dtype=complex)
    G += (coeff[0] + coeff[0].conj().T)[None] / 2.0
    for d in range(len(shape)):
        term = np.exp(TWO_PI * 1j * k[:, d])[:, None, None] * coeff[1 + d][None]
        G += term + np.conj(np.swapaxes(term, 1, 2))
    w, V = np.linalg.eigh(G)
    U = np.einsum("kij,kj,klj->kil", V, np.exp(1j * w), V.conj())
    return np.ascontiguousarray(U, dtype=np.complex128)
