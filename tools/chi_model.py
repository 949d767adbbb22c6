#!/usr/bin/env python3
"""
NumPy model of csrc/tbk_chi.hip: the bare (Lindhard) static susceptibility chi_0(q) of a uniform, periodic k mesh (DESIGN.md
section 15).

    M(k, q)[b][b'] = sum_i conj(U[k][i][b]) D(q)[i] U[k+q][i][b']
    chi_0(q)       = -(1 / NK) sum_k sum_{b b'} F(E[k][b], E[k+q][b']) |M(k, q)[b][b']|^2
    F(a, b)        = (f(a) - f(b)) / (a - b),   F(a, a) = f'(a),   f(x) = 1 / (1 + exp((x - mu) / T))

``k+q`` is the mesh point with the indices (i_d + q_d) mod n_d, ``q`` an integer vector in mesh units (the wavevector is q_d / n_d),
``U[k][i][b]`` component i of band b (convention 2) and ``D(q)`` the orbital phases of convention 1, ``exp(-2 pi i sum_d q_d pos[i][d]
/ n_d)`` with the unreduced q_d, or 1.  Without matrix elements ``|M|^2 = 1``.

F is never evaluated as the quotient, which cancels.  With the pair ordered lo <= hi and y = (lo - hi) / T <= 0,

    F = -f(lo) (1 - f(hi)) h(y) / T,     h(y) = expm1(y) / y,  h(0) = 1

f(x) from t = exp(-|x - mu| / T), 1 - f(x) as f(2 mu - x) from the same t (the mirrored distance from mu is -(x - mu)
exactly): every factor is non-negative, nothing overflows, a = b is the same branch.

The dynamic chi_0(q, omega + i eta) of DESIGN.md section 16 is `dynamic_susceptibility`, with the occupation difference in the stable
form of `pair_difference` and the bound `dynamic_tolerance`.  The orbital-resolved chi_0[i][j](q) of section 17 is `orbital_susceptibility`
(`orbital_susceptibility_naive`: F as the quotient), with the bound `orbital_tolerance`.  The four-index chi_0[i, l; j, m](q) of section
29 is `susceptibility_tensor` (the definition), `susceptibility_tensor_factored` (the kernels' P Q form) and
`susceptibility_tensor_naive` (F as the quotient), with the bound `tensor_tolerance`.  The orbital-resolved dynamic
chi_0[i][j](q, omega + i eta) of section 31 is `dynamic_orbital_susceptibility` (`dynamic_orbital_susceptibility_naive`: f - f' as a
difference), with the bound `dynamic_orbital_tolerance`.

`python tools/chi_model.py` prints one small case by the stable and by the naive F.  Design tooling: nothing in the product imports it.
"""

import itertools

import numpy as np


def fermi_tables(E, mu, T):
    """(f(E), 1 - f(E)) as chi_fermi_kernel stores them per state: both from one t = exp(-|E - mu| / T), the second as f at the
    mirrored energy 2 mu - E, whose distance from mu is -(E - mu) without a rounding."""
    d = np.asarray(E, dtype=float) - mu
    t = np.exp(-np.abs(d) / T)
    small, big = t / (1.0 + t), 1.0 / (1.0 + t)
    return np.where(d > 0.0, small, big), np.where(d < 0.0, small, big)


def _h(y):
    """expm1(y) / y with h(0) = 1, for y <= 0."""
    y = np.asarray(y, dtype=float)
    safe = np.where(y < 0.0, y, -1.0)
    return np.where(y < 0.0, np.expm1(safe) / safe, 1.0)


def pair_weight(a, b, fa, ga, fb, gb, T):
    """f(lo) (1 - f(hi)) h((lo - hi) / T) >= 0 from the tables of both states: -T F(a, b)."""
    a_low = a <= b
    lo, hi = np.where(a_low, a, b), np.where(a_low, b, a)
    return np.where(a_low, fa, fb) * np.where(a_low, gb, ga) * _h((lo - hi) / T)


def pair_factor(a, b, mu, T):
    """F(a, b) <= 0 in the stable form (broadcasts)."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float))
    fa, ga = fermi_tables(a, mu, T)
    fb, gb = fermi_tables(b, mu, T)
    return -pair_weight(a, b, fa, ga, fb, gb, T) / T


def pair_factor_naive(a, b, mu, T):
    """The quotient as written (f' on the diagonal): for comparison where it is well conditioned."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float))
    f = lambda x: 1.0 / (1.0 + np.exp((x - mu) / T))  # noqa: E731
    same = a == b
    diff = np.where(same, 1.0, a - b)
    return np.where(same, -f(a) * (1.0 - f(a)) / T, (f(a) - f(b)) / diff)


def mesh_indices(mesh):
    """The index vectors of the mesh points in mesh order (last axis fastest), int64 [NK][dim]."""
    mesh = [int(n) for n in mesh]
    return np.array(list(itertools.product(*[range(n) for n in mesh])), dtype=np.int64).reshape(-1, len(mesh))


def shifted_points(mesh, q):
    """The flat index of k+q for every mesh point k, int64 [NK]."""
    mesh = np.array([int(n) for n in mesh], dtype=np.int64)
    q = np.mod(np.asarray(q).astype(np.int64), mesh)
    moved = np.mod(mesh_indices(mesh) + q[None, :], mesh[None, :])
    return np.ravel_multi_index(tuple(moved.T), tuple(int(n) for n in mesh))


def phase_table(mesh, q, pos):
    """D[NQ][n] of convention 1: exp(-2 pi i sum_d q_d pos[i][d] / n_d) with the unreduced q_d."""
    mesh = np.array([float(n) for n in mesh])
    q = np.asarray(q).astype(np.int64).reshape(-1, len(mesh))
    angle = np.zeros((q.shape[0], np.asarray(pos).shape[0]))
    for d in range(len(mesh)):
        angle = angle + (q[:, d].astype(float)[:, None] * np.asarray(pos, dtype=float)[None, :, d]) / mesh[d]
    angle = -2.0 * np.pi * angle
    return np.cos(angle) + 1j * np.sin(angle)


def overlaps(U, mesh, q, phases=None):
    """M[NK][n][n] for ONE vector q: M[k][b][b'] = sum_i conj(U[k][i][b]) D[i] U[k+q][i][b'] (phases: D[n] or None)."""
    n = np.asarray(U).shape[-1]
    flat = np.asarray(U).reshape(-1, n, n)
    other = flat[shifted_points(mesh, q)]
    if phases is not None:
        other = np.asarray(phases)[None, :, None] * other
    return np.einsum("kib,kic->kbc", flat.conj(), other)


def susceptibility(E, U, mesh, q, mu, T, matrix_elements=True, phases=None, factor=None):
    """chi_0[NQ] for the integer vectors ``q`` of shape (NQ, dim).  ``E``: mesh + (n,) or (NK, n); ``U`` (not read without matrix
    elements): mesh + (n, n) or (NK, n, n); ``phases``: None or D[NQ][n].  ``factor``: another F(a, b, mu, T) than the stable one."""
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    flat_e = E.reshape(-1, n)
    n_k = flat_e.shape[0]
    q = np.asarray(q)
    if q.dtype.kind not in "iu":
        raise ValueError("q must be integers")
    q = q.astype(np.int64).reshape(-1, len(mesh))
    f, g = fermi_tables(flat_e, mu, T)
    out = np.zeros(q.shape[0])
    for index, vector in enumerate(q):
        to = shifted_points(mesh, vector)
        a, b = flat_e[:, :, None], flat_e[to][:, None, :]
        if factor is None:
            weight = pair_weight(a, b, f[:, :, None], g[:, :, None], f[to][:, None, :], g[to][:, None, :], T)
        else:
            weight = -T * factor(a, b, mu, T)
        if matrix_elements:
            weight = weight * np.abs(overlaps(U, mesh, vector, None if phases is None else np.asarray(phases)[index])) ** 2
        out[index] = weight.sum() / T / n_k
    return out


ULP_EXP = 2.0    # allowance, in ulps, for exp on one side against the exact value (the device's against NumPy's
ULP_EXPM1 = 2.0  # was measured at most 1 ulp apart for either function over the arguments of the tests; twice that)


def tolerance(n_k, n, T, matrix_elements=True):
    """tol_chi of DESIGN.md 15.4: the bound on |chi - chi'| of two evaluations (the kernels, this model) of the SAME (E, U, mu, T),
    each with IEEE double arithmetic in any order of summation and exp / expm1 within ULP_EXP / ULP_EXPM1 ulps.  With u = 2^-53,
    per side and in units of 1 / T:  the sum of NK n^2 non-negative terms whose total is at most NK s, s = n / 4 (n^2 / 4 without
    matrix elements: F in [-1 / (4 T), 0], the rows of |M|^2 add up to 1), divided by NK: NK n^2 s u;  the factors of a term,
    relative: (4 ULP_EXP + ULP_EXPM1 + 15) s u;  the part of exp's argument error that grows with |E - mu| / T, absolute because
    x exp(-x) <= 1 / e: 4 u per unit of |M|^2, 4 n u (4 n^2 u);  and |M|^2: an element of M is a sum of 2 n real products per
    component whose moduli add up to at most 1 (and one complex multiply by D), |dM| <= (3 n + 5) u, so sum F |d(|M|^2)| <=
    ((3 n + 5) n^(3/2) / 2 + 3 n / 4) u by sum |M| <= n^(3/2)."""
    u = 2.0 ** -53
    s = n / 4.0 if matrix_elements else n * n / 4.0
    unit = n if matrix_elements else n * n
    side = n_k * n * n * s + (4 * ULP_EXP + ULP_EXPM1 + 15) * s + 4 * unit
    if matrix_elements:
        side += (3 * n + 5) * n ** 1.5 / 2 + 0.75 * n
    return 2.0 * side * u / T


def pair_difference(a, b, fa, ga, fb, gb, T):
    """g = f(a) - f(b) from the tables of both states, not as the difference: with the pair ordered lo <= hi and y = (lo - hi) / T,
    f(lo) - f(hi) = f(lo) (1 - f(hi)) (-expm1(y)) >= 0, and g carries the sign of the order (+ where a <= b).  Nothing cancels,
    nothing overflows, and a == b gives a zero."""
    a_low = a <= b
    lo, hi = np.where(a_low, a, b), np.where(a_low, b, a)
    value = np.where(a_low, fa, fb) * np.where(a_low, gb, ga) * (-np.expm1((lo - hi) / T))
    return np.where(a_low, value, -value)


def occupation_difference(a, b, mu, T):
    """f(a) - f(b) in the stable form (broadcasts)."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float))
    fa, ga = fermi_tables(a, mu, T)
    fb, gb = fermi_tables(b, mu, T)
    return pair_difference(a, b, fa, ga, fb, gb, T)


def _frequencies(omega, eta):
    omega = np.asarray(omega, dtype=float)
    if omega.ndim == 0:
        omega = omega.reshape(1)
    if omega.ndim != 1 or omega.size < 1 or not np.all(np.isfinite(omega)):
        raise ValueError("omega must be one finite number or a list of them")
    eta = float(eta)
    if not np.isfinite(eta) or not eta > 0.0 or not eta * eta > 0.0:
        raise ValueError("eta must be finite and positive (and its square must not underflow)")
    return omega, eta


def dynamic_susceptibility(E, U, mesh, q, mu, T, omega, eta, matrix_elements=True, phases=None):
    """chi_0(q, omega + i eta), complex [NQ][NW], of DESIGN.md section 16:

        chi_0(q, z) = -(1 / NK) sum_k sum_{b b'} (f(E[k][b]) - f(E[k+q][b'])) / (E[k][b] - E[k+q][b'] + z) |M(k, q)[b][b']|^2

    The arguments are those of `susceptibility`; ``omega``: real frequencies, any sign and order, or one number; ``eta > 0``.
    Per pair of states p = g |M|^2 with g of `pair_difference` and Delta = E[k][b] - E[k+q][b'] (one rounding), per frequency
    x = Delta + omega, r = 1 / (x^2 + eta^2), t = p r, and the sums of t x and of -(t eta) are taken away from +0 and divided by
    NK: Re chi = (0 - sum t x) / NK, Im chi = (0 - sum -(t eta)) / NK -- so that a sum of zeros of either sign gives +0."""
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    flat_e = E.reshape(-1, n)
    n_k = flat_e.shape[0]
    q = np.asarray(q)
    if q.dtype.kind not in "iu":
        raise ValueError("q must be integers")
    q = q.astype(np.int64).reshape(-1, len(mesh))
    omega, eta = _frequencies(omega, eta)
    f, g = fermi_tables(flat_e, mu, T)
    out = np.zeros((q.shape[0], omega.size), dtype=complex)
    for index, vector in enumerate(q):
        to = shifted_points(mesh, vector)
        a, b = flat_e[:, :, None], flat_e[to][:, None, :]
        p = pair_difference(a, b, f[:, :, None], g[:, :, None], f[to][:, None, :], g[to][:, None, :], T)
        if matrix_elements:
            p = p * np.abs(overlaps(U, mesh, vector, None if phases is None else np.asarray(phases)[index])) ** 2
        delta = a - b
        for j, w in enumerate(omega):
            x = delta + w
            t = p * (1.0 / (x * x + eta * eta))
            out[index, j] = complex((0.0 - (t * x).sum()) / n_k, (0.0 - (-(t * eta)).sum()) / n_k)
    return out


def dynamic_susceptibility_naive(E, U, mesh, q, mu, T, omega, eta, matrix_elements=True, phases=None):
    """The formula as written, in complex arithmetic with f(a) - f(b) as the difference of two Fermi functions: for comparison
    where that difference is well conditioned (tests/test_chi_dynamic_model.py states the condition)."""
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    flat_e = E.reshape(-1, n)
    q = np.asarray(q).astype(np.int64).reshape(-1, len(mesh))
    omega, eta = _frequencies(omega, eta)
    with np.errstate(over="ignore"):
        occ = 1.0 / (1.0 + np.exp((flat_e - mu) / T))
    out = np.zeros((q.shape[0], omega.size), dtype=complex)
    for index, vector in enumerate(q):
        to = shifted_points(mesh, vector)
        weight = (occ[:, :, None] - occ[to][:, None, :]).astype(complex)
        if matrix_elements:
            weight = weight * np.abs(overlaps(U, mesh, vector, None if phases is None else np.asarray(phases)[index])) ** 2
        delta = flat_e[:, :, None] - flat_e[to][:, None, :]
        for j, w in enumerate(omega):
            out[index, j] = -(weight / (delta + complex(w, eta))).sum() / flat_e.shape[0]
    return out


ULP_DIV = 2.0  # allowance for the quotient 1 / (x^2 + eta^2), in units of u = 2^-53: a correctly rounded quotient (IEEE division, which
#                both sides use) has 1


def dynamic_tolerance(n_k, n, T, eta, spread, matrix_elements=True):
    """tol of DESIGN.md 16.4: the bound on either component of chi - chi' of two evaluations (the kernels, this model) of the SAME
    (E, U, mu, T, omega, eta), each in IEEE doubles with any order of summation, fused or unfused multiply-adds, exp / expm1 within
    ULP_EXP / ULP_EXPM1 ulps and the quotient within ULP_DIV u.  ``spread`` = 2 bandwidth + |omega| (a number, or an array per
    frequency: the bound is per frequency).  With u = 2^-53, |g| <= 1, |1 / (x + i eta)| <= 1 / eta, per side and in units of
    1 / eta, S = n (n^2 without matrix elements) the most the moduli of one k-point's terms add up to:  the sum of NK n^2 terms of
    either sign: NK n^2 S u;  the factors of a term, relative: (4 ULP_EXP + ULP_EXPM1 + ULP_DIV + 18) S u;  the unbounded part of
    the exponential's argument error, absolute, 2 u per table entry: 4 S u;  x = fl(fl(E - E') + omega) is off by at most
    u (2 |Delta| + |omega|) <= u spread and |d/dx 1 / (x + i eta)| <= 1 / eta^2: S spread / eta u;  |M|^2 as in 15.4 with the weight
    |g| / eta <= 1 / eta in place of 1 / (4 T): (2 (3 n + 5) n^(3/2) + 3 n) u.  T does not enter: it is kept in the signature for
    the callers that pass the call's arguments through."""
    del T
    u = 2.0 ** -53
    big_s = float(n if matrix_elements else n * n)
    side = n_k * n * n * big_s + (4 * ULP_EXP + ULP_EXPM1 + ULP_DIV + 18) * big_s + 4 * big_s + big_s * np.asarray(spread, dtype=float) / eta
    if matrix_elements:
        side = side + 2 * (3 * n + 5) * n ** 1.5 + 3 * n
    return 2.0 * side * u / eta


def _orbital_selection(orbitals, n):
    if orbitals is None:
        return np.arange(n, dtype=np.int64)
    chosen = np.asarray(orbitals)
    if chosen.dtype.kind not in "iu" or chosen.ndim != 1 or chosen.size < 1:
        raise ValueError("orbitals must be a list of integers")
    chosen = chosen.astype(np.int64)
    if chosen.min() < 0 or chosen.max() >= n or np.unique(chosen).size != chosen.size:
        raise ValueError("orbitals must be distinct indices in [0, %d)" % n)
    return chosen


def orbital_amplitudes(U, mesh, q, phases=None, orbitals=None):
    """A[NK][m][n][n] for ONE vector q: A[k][i][b][b'] = (conj(U[k][i][b]) D[i]) U[k+q][i][b'] for the selected orbitals i."""
    n = np.asarray(U).shape[-1]
    flat = np.asarray(U).reshape(-1, n, n)
    chosen = _orbital_selection(orbitals, n)
    left = flat[:, chosen, :].conj()
    if phases is not None:
        left = left * np.asarray(phases)[None, chosen, None]
    return left[:, :, :, None] * flat[shifted_points(mesh, q)][:, chosen, None, :]


def orbital_susceptibility(E, U, mesh, q, mu, T, phases=None, orbitals=None):
    """chi_0[NQ][m][m], complex, of DESIGN.md section 17, for the integer vectors ``q`` of shape (NQ, dim):

        A(k, q)[i; b, b'] = conj(U[k][i][b]) D(q)[i] U[k+q][i][b']
        chi_0[i][j](q)    = (1 / (T NK)) sum_k sum_{b b'} t(E[k][b], E[k+q][b']) A[i; b, b'] conj(A[j; b, b'])

    with t = `pair_weight` >= 0 (-T F).  ``E``, ``U``, ``phases`` as for `susceptibility`; ``orbitals``: None or m distinct indices in
    the caller's order.  Per k-point one matrix product, (t A reshaped to (m, n^2)) A^H, so that BLAS does the n^4 part; the upper
    triangle is kept, the lower is its conjugate and the diagonal's imaginary part is +0, as the kernels write them."""
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    flat_e = E.reshape(-1, n)
    n_k = flat_e.shape[0]
    q = np.asarray(q)
    if q.dtype.kind not in "iu":
        raise ValueError("q must be integers")
    q = q.astype(np.int64).reshape(-1, len(mesh))
    chosen = _orbital_selection(orbitals, n)
    m = chosen.size
    flat_u = np.asarray(U).reshape(-1, n, n)
    f, g = fermi_tables(flat_e, mu, T)
    out = np.zeros((q.shape[0], m, m), dtype=complex)
    for index, vector in enumerate(q):
        to = shifted_points(mesh, vector)
        a, b = flat_e[:, :, None], flat_e[to][:, None, :]
        weight = pair_weight(a, b, f[:, :, None], g[:, :, None], f[to][:, None, :], g[to][:, None, :], T)
        left = flat_u[:, chosen, :].conj()
        if phases is not None:
            left = left * np.asarray(phases)[index][None, chosen, None]
        total = np.zeros((m, m), dtype=complex)
        for k in range(n_k):  # (A of one k-point at a time: m n^2 numbers)
            y = (left[k][:, :, None] * flat_u[to[k]][chosen][:, None, :]).reshape(m, n * n)
            total += (weight[k].reshape(1, n * n) * y) @ y.conj().T
        total = total / T / n_k
        upper = np.triu(total, 1)
        out[index] = upper + upper.conj().T + np.diag(total.diagonal().real)
    return out + (0.0 + 0.0j)  # (-0 from the conjugate of a zero becomes +0)


def orbital_susceptibility_naive(E, U, mesh, q, mu, T, phases=None, orbitals=None):
    """The formula with F as the quotient (`pair_factor_naive`) in one einsum: for comparison where the quotient is well conditioned."""
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    flat_e = E.reshape(-1, n)
    q = np.asarray(q)
    if q.dtype.kind not in "iu":
        raise ValueError("q must be integers")
    q = q.astype(np.int64).reshape(-1, len(mesh))
    chosen = _orbital_selection(orbitals, n)
    out = np.zeros((q.shape[0], chosen.size, chosen.size), dtype=complex)
    for index, vector in enumerate(q):
        to = shifted_points(mesh, vector)
        factor = pair_factor_naive(flat_e[:, :, None], flat_e[to][:, None, :], mu, T)
        amp = orbital_amplitudes(U, mesh, vector, None if phases is None else np.asarray(phases)[index], chosen)
        out[index] = -np.einsum("kbc,kibc,kjbc->ij", factor, amp, amp.conj()) / flat_e.shape[0]
    return out


ROUNDINGS_AMPLITUDES = 14.0  # c_A of DESIGN.md 17.5: a term t A_i conj(A_j) holds two amplitudes, each two complex products of three
#                              roundings per component (conj(U) D, then U'), one scale by t and one product


def orbital_tolerance(n_k, n, T):
    """tol of DESIGN.md 17.5: the bound on either component of one element of chi - chi' of two evaluations (the kernels, this
    model) of the SAME (E, U, mu, T), derived as `tolerance` is.  New: sum_{b b'} |A_i| |A_j| <= 1 by Cauchy-Schwarz on the unit
    rows of U(k) and U(k+q), so per k the moduli of an element's terms add up to at most s = 1 / 4 in units of 1 / T.  Per side:
    the sum of NK n^2 terms, NK n^2 s u;  the factors of a term, relative, (4 ULP_EXP + ULP_EXPM1 + 15 + ROUNDINGS_AMPLITUDES) s u;
    the unbounded part of the exponential's argument error, absolute, 4 u per unit of sum |A_i| |A_j|: 4 u."""
    u = 2.0 ** -53
    side = (n_k * n * n + 4 * ULP_EXP + ULP_EXPM1 + 15 + ROUNDINGS_AMPLITUDES) / 4.0 + 4.0
    return 2.0 * side * u / T


def dynamic_orbital_susceptibility(E, U, mesh, q, mu, T, omega, eta, phases=None, orbitals=None):
    """chi_0[NQ][NW][m][m], complex, of DESIGN.md section 31, for the integer vectors ``q`` of shape (NQ, dim):

        A(k, q)[i; b, b']  = conj(U[k][i][b]) D(q)[i] U[k+q][i][b']
        chi_0[i][j](q, z)  = -(1 / NK) sum_k sum_{b b'} g(E[k][b], E[k+q][b']) / (E[k][b] - E[k+q][b'] + z) A[i; b, b'] conj(A[j; b, b'])

    with z = omega + i eta and g = `pair_difference`.  ``E``, ``U``, ``phases``, ``orbitals`` as for `orbital_susceptibility`, ``omega``
    and ``eta`` as for `dynamic_susceptibility`.  Per pair of states g and Delta = E[k][b] - E[k+q][b'] (one rounding) once; per
    frequency, unfused and in this order, x = Delta + omega, r = 1 / (x^2 + eta^2), gr = g r, c = (gr x, -(gr eta)); X = c A, and per
    k-point one matrix product X A^H (reshaped to (m, n^2)) so that BLAS does the n^4 part.  The sum is taken away from +0 and divided by
    NK per component, so that a sum of zeros of either sign gives +0.  The matrix is not Hermitian: nothing is mirrored."""
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    flat_e = E.reshape(-1, n)
    n_k = flat_e.shape[0]
    q = np.asarray(q)
    if q.dtype.kind not in "iu":
        raise ValueError("q must be integers")
    q = q.astype(np.int64).reshape(-1, len(mesh))
    omega, eta = _frequencies(omega, eta)
    chosen = _orbital_selection(orbitals, n)
    m = chosen.size
    flat_u = np.asarray(U).reshape(-1, n, n)
    f, g = fermi_tables(flat_e, mu, T)
    out = np.zeros((q.shape[0], omega.size, m, m), dtype=complex)
    for index, vector in enumerate(q):
        to = shifted_points(mesh, vector)
        a, b = flat_e[:, :, None], flat_e[to][:, None, :]
        gd = pair_difference(a, b, f[:, :, None], g[:, :, None], f[to][:, None, :], g[to][:, None, :], T)
        delta = a - b
        left = flat_u[:, chosen, :].conj()
        if phases is not None:
            left = left * np.asarray(phases)[index][None, chosen, None]
        total = np.zeros((omega.size, m, m), dtype=complex)
        for k in range(n_k):  # (A of one k-point at a time: m n^2 numbers)
            y = (left[k][:, :, None] * flat_u[to[k]][chosen][:, None, :]).reshape(m, n * n)
            yh = y.conj().T
            for j, w in enumerate(omega):
                x = delta[k] + w
                gr = gd[k] * (1.0 / (x * x + eta * eta))
                c = (gr * x + 1j * (-(gr * eta))).reshape(1, n * n)
                total[j] += (c * y) @ yh
        out[index] = ((0.0 - total.real) / n_k) + 1j * ((0.0 - total.imag) / n_k)
    return out


def dynamic_orbital_susceptibility_naive(E, U, mesh, q, mu, T, omega, eta, phases=None, orbitals=None):
    """The formula as written, in complex arithmetic with f(a) - f(b) as the difference of two Fermi functions and one einsum over
    (k, b, b'): for comparison where that difference is well conditioned."""
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    flat_e = E.reshape(-1, n)
    q = np.asarray(q).astype(np.int64).reshape(-1, len(mesh))
    omega, eta = _frequencies(omega, eta)
    chosen = _orbital_selection(orbitals, n)
    with np.errstate(over="ignore"):
        occ = 1.0 / (1.0 + np.exp((flat_e - mu) / T))
    out = np.zeros((q.shape[0], omega.size, chosen.size, chosen.size), dtype=complex)
    for index, vector in enumerate(q):
        to = shifted_points(mesh, vector)
        weight = occ[:, :, None] - occ[to][:, None, :]
        delta = flat_e[:, :, None] - flat_e[to][:, None, :]
        amp = orbital_amplitudes(U, mesh, vector, None if phases is None else np.asarray(phases)[index], chosen)
        for j, w in enumerate(omega):
            out[index, j] = -np.einsum("kbc,kibc,kjbc->ij", weight / (delta + complex(w, eta)), amp, amp.conj()) / flat_e.shape[0]
    return out


ROUNDINGS_COMPLEX_SCALE = 3.0  # X = c A is a complex product, three roundings per component (two unfused), where ROUNDINGS_AMPLITUDES
#                                counts one for the real scale by t: taken in full, on top


def dynamic_orbital_tolerance(n_k, n, T, eta, spread):
    """tol of DESIGN.md 31.5: the bound on either component of one element of chi - chi' of two evaluations (the kernels, this model)
    of the SAME (E, U, mu, T, omega, eta), derived as `dynamic_tolerance` and `orbital_tolerance` are.  ``spread`` = 2 bandwidth +
    |omega| (a number, or an array per frequency).  Per k the moduli of an element's terms add up to at most S = 1 in units of 1 / eta:
    sum_{b b'} |A_i| |A_j| <= 1 by Cauchy-Schwarz on the unit rows of U(k) and U(k+q), |g| <= 1 and |1 / (x + i eta)| <= 1 / eta; an
    error of a complex term's modulus bounds that of either component.  Per side:  the sum of NK n^2 terms in any order, NK n^2 u;  the
    factors of a term, relative: 16.4's (4 ULP_EXP + ULP_EXPM1 + ULP_DIV + 18) for g, x and the Lorentzian, 17.5's
    ROUNDINGS_AMPLITUDES for the two amplitudes and ROUNDINGS_COMPLEX_SCALE for the complex weight;  the unbounded part of the
    exponential's argument error, absolute: 4 u;  the rounding of Delta + omega under the Lorentzian's slope, 16.4's: spread / eta u.
    T does not enter (kept in the signature as in `dynamic_tolerance`); no number from the kernels does."""
    del T
    u = 2.0 ** -53
    factors = 4 * ULP_EXP + ULP_EXPM1 + ULP_DIV + 18 + ROUNDINGS_AMPLITUDES + ROUNDINGS_COMPLEX_SCALE
    side = n_k * n * n + factors + 4.0 + np.asarray(spread, dtype=float) / eta
    return 2.0 * side * u / eta


def _tensor_arguments(E, U, mesh, q, orbitals):
    E = np.asarray(E, dtype=float)
    n = E.shape[-1]
    flat_e = E.reshape(-1, n)
    q = np.asarray(q)
    if q.dtype.kind not in "iu":
        raise ValueError("q must be integers")
    q = q.astype(np.int64).reshape(-1, len(mesh))
    chosen = _orbital_selection(orbitals, n)
    return flat_e, np.asarray(U).reshape(-1, n, n), q, chosen


def _tensor_hermitian(total):
    """The (m, m, m, m) sum as the kernels write it: as an m^2 x m^2 matrix with rows (i, l) and columns (j, m) the upper triangle is
    kept, the lower is its conjugate, the diagonal's imaginary part is +0 and no -0 stays."""
    m = total.shape[0]
    matrix = total.reshape(m * m, m * m)
    upper = np.triu(matrix, 1)
    matrix = upper + upper.conj().T + np.diag(matrix.diagonal().real)
    return matrix.reshape(m, m, m, m) + (0.0 + 0.0j)


def _per_reduced_vector(mesh, q, one):
    """[one(vector) for vector in q], computed once per vector modulo the mesh: q and q + n_d e_d are the same sum."""
    sizes = np.array([int(s) for s in mesh], dtype=np.int64)
    done = {}
    rows = []
    for vector in q:
        key = tuple(int(x) for x in np.mod(vector, sizes))
        if key not in done:
            done[key] = one(vector)
        rows.append(done[key])
    return np.array(rows)


def susceptibility_tensor(E, U, mesh, q, mu, T, orbitals=None):
    """chi_0[NQ][m][m][m][m], complex, indexed [q, i, l, j, m], of DESIGN.md section 29 (convention 2 only: no phases), for the integer
    vectors ``q`` of shape (NQ, dim):

        chi_0[i, l; j, m](q) = (1 / (T NK)) sum_k sum_{b b'} t(E[k][b], E[k+q][b'])
                               conj(U[k][i][b]) U[k+q][l][b'] U[k][j][b] conj(U[k+q][m][b'])

    with t = `pair_weight` >= 0 (-T F).  The definition as it stands: with the pair amplitude a[(i, l); b, b'] = conj(U[k][i][b])
    U[k+q][l][b'] the k-point's term is the contraction ``einsum("c,pc,rc->pr", t, a, conj(a))`` over c = (b, b') all at once, as one
    matrix product so that BLAS does the n^2 m^4 part.  The sum over b' is NOT taken first: the kernels' factorisation
    (`susceptibility_tensor_factored`) does not enter, the two are held together by the tests.  ``E``, ``U``, ``orbitals`` as for
    `orbital_susceptibility`.  The output is made Hermitian as the kernels make it (`_tensor_hermitian`)."""
    flat_e, flat_u, q, chosen = _tensor_arguments(E, U, mesh, q, orbitals)
    n_k, n = flat_e.shape
    m = chosen.size
    f, g = fermi_tables(flat_e, mu, T)

    def one(vector):
        to = shifted_points(mesh, vector)
        a, b = flat_e[:, :, None], flat_e[to][:, None, :]
        weight = pair_weight(a, b, f[:, :, None], g[:, :, None], f[to][:, None, :], g[to][:, None, :], T)
        total = np.zeros((m * m, m * m), dtype=complex)
        for k in range(n_k):  # (the amplitudes of one k-point at a time: m^2 n^2 numbers)
            left, right = flat_u[k][chosen].conj(), flat_u[to[k]][chosen]
            amp = (left[:, None, :, None] * right[None, :, None, :]).reshape(m * m, n * n)
            total += (weight[k].reshape(1, n * n) * amp) @ amp.conj().T
        return _tensor_hermitian((total / T / n_k).reshape(m, m, m, m))

    return _per_reduced_vector(mesh, q, one)


def susceptibility_tensor_factored(E, U, mesh, q, mu, T, orbitals=None):
    """The same tensor in the kernels' algebra: per k-point and band b, P[i, j] = conj(U[k][i][b]) U[k][j][b] and Q[l, m] = sum_b'
    t[b, b'] U[k+q][l][b'] conj(U[k+q][m][b']), chi_0[i, l; j, m] = (1 / (T NK)) sum_{k b} P[i, j] Q[l, m].  n times fewer
    multiplications than the definition; held to `susceptibility_tensor` within `tensor_tolerance`."""
    flat_e, flat_u, q, chosen = _tensor_arguments(E, U, mesh, q, orbitals)
    n_k = flat_e.shape[0]
    m = chosen.size
    f, g = fermi_tables(flat_e, mu, T)

    def one(vector):
        to = shifted_points(mesh, vector)
        a, b = flat_e[:, :, None], flat_e[to][:, None, :]
        weight = pair_weight(a, b, f[:, :, None], g[:, :, None], f[to][:, None, :], g[to][:, None, :], T)
        total = np.zeros((m, m, m, m), dtype=complex)
        for k in range(n_k):
            here, there = flat_u[k][chosen], flat_u[to[k]][chosen]
            p = np.einsum("ib,jb->bij", here.conj(), here)
            w = np.einsum("lc,mc->clm", there, there.conj())
            big_q = np.einsum("bc,clm->blm", weight[k], w)
            total += np.einsum("bij,blm->iljm", p, big_q)
        return _tensor_hermitian(total / T / n_k)

    return _per_reduced_vector(mesh, q, one)


def susceptibility_tensor_naive(E, U, mesh, q, mu, T, orbitals=None):
    """The formula with F as the quotient (`pair_factor_naive`) in one einsum over (k, b, b'), nothing made Hermitian: for comparison
    where the quotient is well conditioned."""
    flat_e, flat_u, q, chosen = _tensor_arguments(E, U, mesh, q, orbitals)
    out = []
    for vector in q:
        to = shifted_points(mesh, vector)
        factor = pair_factor_naive(flat_e[:, :, None], flat_e[to][:, None, :], mu, T)
        here, there = flat_u[:, chosen, :], flat_u[to][:, chosen, :]
        out.append(-np.einsum("kbc,kib,klc,kjb,kmc->iljm", factor, here.conj(), there, here, there.conj(), optimize=True) / flat_e.shape[0])
    return np.array(out)


ROUNDINGS_TENSOR = 10.0  # c_T of DESIGN.md 29.5: a term t conj(U_i) U_j U'_l conj(U'_m) as the unfused model forms it holds two complex
#                          products of two eigenvector factors (three roundings per component each), the scale by t (one) and the
#                          complex product of the two pairs (three)


def tensor_tolerance(n_k, n, T):
    """tol of DESIGN.md 29.5: the bound on either component of one entry of chi - chi' of two evaluations (the kernels, this model) of
    the SAME (E, U, mu, T), derived as `orbital_tolerance` is.  Per k the moduli of an entry's terms add up to at most s = 1 / 4 in
    units of 1 / T: sum_b |U[k][i][b]| |U[k][j][b]| <= 1 and sum_b' |U[k+q][l][b']| |U[k+q][m][b']| <= 1 by Cauchy-Schwarz on unit
    rows, t <= 1 / 4.  Per side: the sum of NK n^2 terms in any order, NK n^2 s u -- which covers the two-level sum of the factorised
    form, n - 1 additions over b' inside and NK n - 1 over (k, b) outside, fewer than NK n^2 for every n, its products being those
    counted in ROUNDINGS_TENSOR with the sum over b' between them;  the factors of a term, relative,
    (4 ULP_EXP + ULP_EXPM1 + 15 + ROUNDINGS_TENSOR) s u;  the unbounded part of the exponential's argument error, absolute, 4 u.
    Together [NK n^2 / 2 + 25.5] u / T."""
    u = 2.0 ** -53
    side = (n_k * n * n + 4 * ULP_EXP + ULP_EXPM1 + 15 + ROUNDINGS_TENSOR) / 4.0 + 4.0
    return 2.0 * side * u / T


def static_limit(E, mu, T):
    """chi_0(0) with matrix elements: (1 / NK) sum_{k b} f (1 - f) / T, from the eigenvalues alone."""
    E = np.asarray(E, dtype=float)
    f, g = fermi_tables(E, mu, T)
    return float((f * g).sum() / T / (E.size // E.shape[-1]))


def main():
    rng = np.random.default_rng(7)
    mesh, n, mu, T = (2, 3, 2), 5, 0.1, 0.05
    n_k = int(np.prod(mesh))
    hams = rng.normal(size=(n_k, n, n)) + 1j * rng.normal(size=(n_k, n, n))
    eig, vec = np.linalg.eigh(hams + hams.conj().transpose(0, 2, 1))
    q = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [1, 2, 1], [3, 2, 1]])
    for me in (True, False):
        stable = susceptibility(eig, vec, mesh, q, mu, T, me)
        naive = susceptibility(eig, vec, mesh, q, mu, T, me, factor=pair_factor_naive)
        print("random 5-orbital model, mesh %s, mu = %g, T = %g, matrix elements: %s" % (mesh, mu, T, me))
        for vector, s, v in zip(q, stable, naive):
            print("    q = %-12s chi_0 = %.15f   naive F: %.15f   difference %.1e" % (tuple(int(x) for x in vector), s, v, abs(s - v)))
    print("    chi_0(0) from the eigenvalues alone: %.15f" % static_limit(eig, mu, T))
    print("    4 T chi_0 at T = 1e9 bandwidths: %s (n = %d)" % (4 * 1e9 * np.ptp(eig) * susceptibility(eig, vec, mesh, q[:2], mu, 1e9 * np.ptp(eig)), n))


if __name__ == "__main__":
    main()
