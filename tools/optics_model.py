#!/usr/bin/env python3
"""
NumPy model of csrc/tbk_optics.hip: the Kubo optical (current-current) conductivity sigma[a][c](omega) of a uniform, periodic k mesh
(DESIGN.md section 27), the statement every test compares with.

Mesh points k = (i_1 / n_1, ..., i_dim / n_dim), ``E, U`` of ``eigh(k, convention=2)``; reduced coordinates, e = hbar = 1, per unit
cell, no spin factor::

    D^a(k)      = sum_R  i R_a exp(2 pi i k.R) hop[R]  +  h.c.            = (1 / 2 pi) dH/dk_a      (Hermitian, R = 0 drops out)
    V^a(k)      = U^H D^a U                                               convention 2
    V^a[b,b']  += i (E_b - E_b') (U^H diag(pos[:, a]) U)[b,b']            convention 1 only: the positions inside the cell
    w[b,b']     = -(f(E_b) - f(E_b')) / (E_b - E_b')  >= 0                 = t / T, t = chi_model.pair_weight; equal energies: -f'(E)
    sigma[a,c](omega) = (i / NK) sum_k sum_{b,b'}  w[b,b'] V^a[b,b'] conj(V^c[b,b']) / (omega + i eta + E_b - E_b')

``w`` is evaluated as the susceptibilities evaluate it (chi_model.fermi_tables, chi_model.pair_weight): nothing cancels, and the
intraband (Drude) term is the same branch.  `conductivity` is that statement, `conductivity_naive` a triple loop with the quotient as
written, `conductivity_convention1` the convention-1 result a second, independent way: the convention-1 Hamiltonian of
``oracle.hamilton`` differentiated directly, with its own eigenvectors.  `tolerance` is the bound of DESIGN.md 27.4.

`python tools/optics_model.py` prints the Hall plateau of the Qi-Wu-Zhang model.  Design tooling: nothing in the product imports it.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chi_model  # noqa: E402  pylint: disable=wrong-import-position

TWO_PI = 2.0 * np.pi


def mesh_kpoints(mesh):
    """The mesh points in mesh order (last axis fastest), float [NK][dim]."""
    return chi_model.mesh_indices(mesh).astype(float) / np.array([float(n) for n in mesh])


def derivative(r_vec, hop, k, axis):
    """D^a(k) = (1 / 2 pi) dH/dk_a of the packed half-space hoppings (``oracle.hamilton``'s arguments), convention 2:
    complex [NK][n][n], Hermitian."""
    r_vec = np.asarray(r_vec)
    hop = np.asarray(hop, dtype=np.complex128)
    k = np.asarray(k, dtype=float).reshape(-1, r_vec.shape[1])
    out = np.zeros((k.shape[0],) + hop.shape[1:], dtype=np.complex128)
    for R, mat in zip(r_vec, hop):
        if R[axis] != 0:
            out += (1j * float(R[axis]) * np.exp(2j * np.pi * (k @ R.astype(float))))[:, None, None] * mat[None]
    return out + out.conj().transpose(0, 2, 1)


def derivatives(r_vec, hop, k):
    """D[NK][dim][n][n]: every axis, the layout of ``tbk_optics_from_eigensystem``."""
    dim = np.asarray(r_vec).shape[1]
    return np.ascontiguousarray(np.stack([derivative(r_vec, hop, k, a) for a in range(dim)], axis=1))


def derivative_convention1(r_vec, hop, k, axis, pos):
    """(1 / 2 pi) d/dk_a of the convention-1 Hamiltonian, term by term from its formula: H_1[i][j] = sum_R exp(2 pi i k.(R + pos_j -
    pos_i)) hop[R][i][j] + h.c., so every term takes the factor i (R_a + pos[j][a] - pos[i][a])."""
    r_vec = np.asarray(r_vec)
    hop = np.asarray(hop, dtype=np.complex128)
    pos = np.asarray(pos, dtype=float)
    k = np.asarray(k, dtype=float).reshape(-1, r_vec.shape[1])
    shift = pos[None, :, :] - pos[:, None, :]  # [i][j][d] = pos_j - pos_i
    out = np.zeros((k.shape[0],) + hop.shape[1:], dtype=np.complex128)
    for R, mat in zip(r_vec, hop):
        arm = R.astype(float)[None, None, :] + shift
        phase = np.exp(2j * np.pi * np.einsum("kd,ijd->kij", k, arm))
        out += 1j * arm[None, :, :, axis] * phase * mat[None]
    return out + out.conj().transpose(0, 2, 1)


def derivative_bound(r_vec, hop, pos=None):
    """(2 pi)^2 max|R|^3 sum|hop|: a bound on every element of the second derivative of D^a along an axis (max |R| the largest entry
    of a lattice vector -- for convention 1, ``pos`` given, of R + pos_j - pos_i --, sum |hop| over both halves of the lattice)."""
    r_max = float(np.abs(np.asarray(r_vec)).max()) if len(r_vec) else 0.0
    if pos is not None:
        r_max += float(np.ptp(np.asarray(pos, dtype=float), axis=0).max())
    return TWO_PI ** 2 * r_max ** 3 * 2.0 * float(np.abs(np.asarray(hop)).sum())


def derivative_step(r_vec, hop, pos=None):
    """The step h of the central difference (H(k + h e_a) - H(k - h e_a)) / (4 pi h) and the bound on its distance from D^a: the
    truncation h^2 B / 6 with B = `derivative_bound` plus the rounding of the difference, 4 u sum|hop| / (4 pi h); h balances them."""
    u = 2.0 ** -53
    total = 2.0 * float(np.abs(np.asarray(hop)).sum())
    bound = max(derivative_bound(r_vec, hop, pos), 1e-300)
    h = (3.0 * u * total / (np.pi * bound)) ** (1.0 / 3.0) if total > 0.0 else 1e-5
    return h, h * h * bound / 6.0 + 8.0 * u * total / (4.0 * np.pi * h) + 64.0 * u * total


def velocities(E, U, D, pos=None):
    """V[NK][dim][n][n] in the band basis: U^H D^a U, plus the position term of convention 1 when ``pos`` [n][dim] is given."""
    E = np.asarray(E, dtype=float)
    U = np.asarray(U)
    D = np.asarray(D)
    left = U.conj().transpose(0, 2, 1)[:, None]  # U^H per k-point, broadcast over the axes: matrix products, not an n^4 einsum
    V = left @ (D @ U[:, None])
    if pos is not None:
        scaled = np.asarray(pos, dtype=float).T[None, :, :, None] * U[:, None]  # [k][a][i][c] = pos[i][a] U[k][i][c]
        V = V + 1j * (E[:, None, :, None] - E[:, None, None, :]) * (left @ scaled)
    return V


def _frequencies(omega, eta):
    return chi_model._frequencies(omega, eta)  # pylint: disable=protected-access


def conductivity(E, U, D, mu, T, omega, eta, pos=None):
    """sigma complex [NW][dim][dim] from E [NK][n], U [NK][n][n], D [NK][dim][n][n] (`derivatives`), ``pos`` for convention 1."""
    E = np.asarray(E, dtype=float)
    n_k = E.shape[0]
    omega, eta = _frequencies(omega, eta)
    V = velocities(E, U, D, pos)
    f, g = chi_model.fermi_tables(E, mu, T)
    a, b = E[:, :, None], E[:, None, :]
    t = chi_model.pair_weight(a, b, f[:, :, None], g[:, :, None], f[:, None, :], g[:, None, :], T)
    p = t[:, None, None, :, :] * V[:, :, None, :, :] * V.conj()[:, None, :, :, :]  # [k][a][c][b][b']
    delta = a - b
    out = np.zeros((omega.size, V.shape[1], V.shape[1]), dtype=complex)
    for j, w in enumerate(omega):
        x = delta + w
        r = (x - 1j * eta) * (1.0 / (x * x + eta * eta))
        s = (p * r[:, None, None, :, :]).sum(axis=(0, 3, 4))
        out[j] = (0.0 - s.imag) / T / n_k + 1j * ((0.0 + s.real) / T / n_k)
    return out


def conductivity_naive(E, U, D, mu, T, omega, eta, pos=None):
    """The formula as written, in a triple loop per frequency, with w as the quotient of Fermi functions (-f' on equal energies): for
    comparison where the quotient is well conditioned."""
    E = np.asarray(E, dtype=float)
    U = np.asarray(U)
    D = np.asarray(D)
    omega, eta = _frequencies(omega, eta)
    n_k, n = E.shape
    dim = D.shape[1]
    occ = 1.0 / (1.0 + np.exp((E - mu) / T))
    out = np.zeros((omega.size, dim, dim), dtype=complex)
    for k in range(n_k):
        V = [U[k].conj().T @ D[k, a] @ U[k] for a in range(dim)]
        if pos is not None:
            for a in range(dim):
                P = U[k].conj().T @ np.diag(np.asarray(pos, dtype=float)[:, a]) @ U[k]
                V[a] = V[a] + 1j * (E[k][:, None] - E[k][None, :]) * P
        for b in range(n):
            for c in range(n):
                gap = E[k, b] - E[k, c]
                w = occ[k, b] * (1.0 - occ[k, b]) / T if gap == 0.0 else -(occ[k, b] - occ[k, c]) / gap
                for j in range(omega.size):
                    r = 1.0 / (omega[j] + 1j * eta + gap)
                    for a in range(dim):
                        for d in range(dim):
                            out[j, a, d] += 1j * w * V[a][b, c] * np.conj(V[d][b, c]) * r / n_k
    return out


def conductivity_convention1(r_vec, hop, pos, mesh, mu, T, omega, eta):
    """Convention 1 without the band-basis term: H_1(k) of ``oracle.hamilton``'s formula, its own eigenvectors, its own derivative."""
    k = mesh_kpoints(mesh)
    r_vec = np.asarray(r_vec)
    pos = np.asarray(pos, dtype=float)
    hop = np.asarray(hop, dtype=np.complex128)
    H = np.zeros((k.shape[0],) + hop.shape[1:], dtype=np.complex128)
    for R, mat in zip(r_vec, hop):
        H += np.exp(2j * np.pi * (k @ R.astype(float)))[:, None, None] * mat[None]
    H = H + H.conj().transpose(0, 2, 1)
    orb = np.exp(2j * np.pi * (k @ pos.T))
    H = orb.conj()[:, :, None] * H * orb[:, None, :]
    E, U = np.linalg.eigh(H)
    D = np.stack([derivative_convention1(r_vec, hop, k, a, pos) for a in range(r_vec.shape[1])], axis=1)
    return conductivity(E, U, D, mu, T, omega, eta)


def cartesian(sigma, uc):
    """uc^T sigma uc / |det uc| per frequency: the tensor in Cartesian axes per unit volume (rows of ``uc`` are the lattice vectors)."""
    uc = np.asarray(uc, dtype=float)
    return np.einsum("ia,wij,jc->wac", uc, np.asarray(sigma), uc) / abs(np.linalg.det(uc))


def drude(E_of_k, v_of_k, mu, T, omega, eta):
    """The closed form of a one-band model: sigma[a][c] = i / (omega + i eta) (1 / NK) sum_k (-f'(E)) v_a v_c, v = D^a(k) (real)."""
    E = np.asarray(E_of_k, dtype=float)
    v = np.asarray(v_of_k, dtype=float)
    f, g = chi_model.fermi_tables(E, mu, T)
    weight = np.einsum("k,ka,kc->ac", f * g / T, v, v) / E.size
    omega, eta = _frequencies(omega, eta)
    return (1j / (omega + 1j * eta))[:, None, None] * weight[None]


def velocity_norm(D, E=None, pos=None):
    """G of `tolerance`: a bound on the Frobenius norm of every V^a(k) -- max_k,a ||D^a(k)||_F, plus for convention 1 the bandwidth
    times ||pos[:, a]||_2 (the position term is (E_b - E_b') times an element of a matrix of that norm at most)."""
    D = np.asarray(D)
    norm = float(np.sqrt((np.abs(D) ** 2).sum(axis=(-1, -2))).max())
    if pos is not None:
        norm += float(np.ptp(np.asarray(E, dtype=float))) * float(np.sqrt((np.asarray(pos, dtype=float) ** 2).sum(axis=0)).max())
    return norm


def tolerance(n_k, n, T, eta, spread, norm, products=2, extra=0.0, shift=0.0):
    """tol of DESIGN.md 27.4: the bound on either component of one element of sigma - sigma' of two evaluations (the kernels, this
    model) of the SAME (E, U, D, mu, T, omega, eta), each in IEEE doubles with any order of summation, fused or unfused multiply-adds,
    exp / expm1 within chi_model.ULP_EXP / ULP_EXPM1 ulps and the quotient within chi_model.ULP_DIV u.  ``spread`` = 2 bandwidth +
    |omega| (per frequency), ``norm`` = G of `velocity_norm`, ``products`` = the n-term matrix products behind V (2; 3 with the
    position term), ``extra`` = a bound on ||dV||_F / G from elsewhere, in units of u (a D^a that is itself rounded).

    With u = 2^-53, t <= 1 / 4, |1 / (x + i eta)| <= 1 / eta and sum_{b b'} |V^a| |V^c| <= G^2 (Cauchy-Schwarz), the moduli of one
    k-point's terms add up to at most S = G^2 / (4 T eta).  Per side, in units of S u:  the sum of NK n^2 terms: NK n^2;  the factors
    of a term, relative: 4 ULP_EXP + ULP_EXPM1 + ULP_DIV + 30 (the tables, h, the quotient, two complex products and the scale);  the
    unbounded part of the exponential's argument error, absolute, 4 u per unit of |V^a| |V^c|: 16;  x = fl(fl(E - E') + omega) is off by
    at most u spread under the slope 1 / eta^2 of the Lorentzian: spread / eta;  V itself: every product is a sum of 2 n real terms
    per component, ||dV||_F <= products (2 n + 3) sqrt(n) G u, and it enters twice: 2 products (2 n + 3) sqrt(n) + 2 extra.

    ``shift`` (an energy; 0 for the same eigensystem on both sides) is for two evaluations that each solved their own eigenproblem: a
    backward-stable solver returns the exact eigensystem of H + dH with ||dH||_2 <= shift.  For a fixed operator D^a the sum over
    (b, b') is sum g(E_b, E_b') |<b| D |b'>|^2-like with the kernel g = t / (T (omega + i eta + E_b - E_b')), a smooth function of both
    energies (t / T is a divided difference of f); its derivatives are bounded by |g| (1 / eta + 1 / T) per energy, so a perturbation
    of H of that size moves the sum by at most 2 (1 / eta + 1 / T) shift S per side (two energies per term), whatever it does to the
    eigenvectors inside clusters: 2 (1 / eta + 1 / T) shift / u in the units above."""
    u = 2.0 ** -53
    s = norm * norm / (4.0 * T * eta)
    side = (n_k * n * n + 4 * chi_model.ULP_EXP + chi_model.ULP_EXPM1 + chi_model.ULP_DIV + 30 + 16
            + np.asarray(spread, dtype=float) / eta + 2.0 * products * (2 * n + 3) * np.sqrt(n) + 2.0 * extra
            + 2.0 * (1.0 / eta + 1.0 / T) * shift / u)
    return 2.0 * side * s * u + 4.0 * np.finfo(float).tiny


def eigensolver_shift(H):
    """`shift` of `tolerance` for numpy.linalg.eigh on the matrices H[NK][n][n]: the backward error of LAPACK's Hermitian solvers, taken
    as n u max_k ||H(k)||_2 (Anderson et al., LAPACK Users' Guide 4.7: p(n) u ||H||_2 with a modestly growing p(n))."""
    H = np.asarray(H)
    return H.shape[-1] * 2.0 ** -53 * float(np.abs(np.linalg.eigvalsh(H)).max())


def qwz_packed(u):
    """The Qi-Wu-Zhang model as packed half-space hoppings (r_vec int64 [3][2], hop complex [3][2][2], the R = 0 block halved)."""
    import berry_model  # pylint: disable=import-outside-toplevel

    hop = berry_model.qwz_hoppings(u)
    keys = sorted(hop)
    return np.array(keys, dtype=np.int64), np.array([hop[key] for key in keys], dtype=np.complex128)


def main():
    import berry_model  # pylint: disable=import-outside-toplevel

    for mesh in ((8, 8), (12, 12)):
        for u_par in (-3.0, -1.0, 1.0, 3.0):
            r_vec, hop = qwz_packed(u_par)
            k = mesh_kpoints(mesh)
            H = berry_model.hamiltonians(berry_model.qwz_hoppings(u_par), k)
            E, U = np.linalg.eigh(H)
            sigma = conductivity(E, U, derivatives(r_vec, hop, k), 0.0, 0.02, [0.0], 0.05)
            chern = int(berry_model.berry_flux(U, mesh, 1)["chern"][0][0, 0])
            print("QWZ u = %+.0f on %s: 2 pi sigma_xy(0) = %+.6f, C = %+d" % (u_par, mesh, TWO_PI * sigma[0, 0, 1].real, chern))


if __name__ == "__main__":
    main()
