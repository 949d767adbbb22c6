#!/usr/bin/env python3
"""
Band structure along a k path, a k.p expansion beside it, and a (projected) density of states from a uniform mesh -- the
pattern of the reference's `examples/kdotp/run.py` (single-k calls in a loop) plus the batched calls this package
is built for.  Runs on the silicon model of the reference's test-suite (tests/golden/cli_eigenvals); needs a GPU.

    python examples/bands_and_dos.py [model.hdf5]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tbmodels_amd  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "cli_eigenvals", "silicon_model.hdf5")
    model = tbmodels_amd.io.load(path)
    print(model)

    # 1. the reference's example: one k-point per call along a line, tight-binding against its k.p expansion
    k_star, k_dir = np.array([0.1, 0.2, 0.3]), np.array([0.3, -0.1, 0.1])
    xs = np.linspace(-0.05, 0.05, 21)
    model_kp = model.construct_kdotp(k_star, order=2)
    t0 = time.perf_counter()
    bands_tb = np.array([model.eigenval(k_star + x * k_dir) for x in xs])
    per_call = (time.perf_counter() - t0) / len(xs)
    bands_kp = np.array([model_kp.eigenval(x * k_dir) for x in xs])
    print("line of %d single-k calls: %.0f us per call; max |E_tb - E_kp| on the line: %.2e"
          % (len(xs), per_call * 1e6, np.abs(bands_tb - bands_kp).max()))

    # 2. the same line as ONE batched call
    t0 = time.perf_counter()
    batched = model.eigenval_array(k_star + xs[:, None] * k_dir)
    print("the same line as one call: %.0f us; identical to the loop within %.1e"
          % ((time.perf_counter() - t0) * 1e6, np.abs(batched - bands_tb).max()))

    # 3. density of states from a 60 x 60 x 60 mesh (folded evaluation: every mesh plane is a 2-D model)
    n = 60
    axis = np.linspace(0, 1, n, endpoint=False)
    mesh = np.stack([m.reshape(-1) for m in np.meshgrid(axis, axis, axis, indexing="ij")], axis=1)
    model.eigenval_array(mesh[:4096])  # warm up
    t0 = time.perf_counter()
    eig = model.eigenval_array(mesh)
    dt = time.perf_counter() - t0
    print("%d mesh points in %.1f ms (%.1f M k-points/s); bands span [%.3f, %.3f]"
          % (len(mesh), dt * 1e3, len(mesh) / dt / 1e6, eig.min(), eig.max()))
    # the tetrahedron method on the same mesh: the eigenvalues stay on the GPU, 401 numbers come back
    energies = np.linspace(eig.min() - 0.5, eig.max() + 0.5, 401)
    model.dos((n, n, n), energies[:2])  # warm up
    t0 = time.perf_counter()
    result = model.dos((n, n, n), energies)
    dt = time.perf_counter() - t0
    mid = 0.5 * (result.energies[1:] + result.energies[:-1])
    peak = np.argmax(result.dos)
    print("tetrahedron DOS on the same mesh in %.1f ms: %.6f states below %.3f, peak %.3f states per energy unit at %.3f"
          % (dt * 1e3, result.nos[-1], energies[-1], result.dos[peak], mid[peak]))

    # the Fermi level of the same mesh at half filling (one state per band and cell, no spin factor) and the gap, if there is one:
    # a search on doubles with the eigenvalues on the GPU, four numbers come back
    t0 = time.perf_counter()
    level = model.fermi_level((n, n, n), model.size / 2)
    dt = time.perf_counter() - t0
    if level.lower < level.upper:
        print("Fermi level at half filling in %.1f ms: mu = %.6f in the gap [%.6f, %.6f] of %.6f"
              % (dt * 1e3, level.mu, level.lower, level.upper, level.upper - level.lower))
    else:
        print("Fermi level at half filling in %.1f ms: mu = %.12f (no gap on this mesh), %.12f states below it" % (dt * 1e3, level.mu, level.nos))

    # 4. the orbital character of that spectrum: s and p orbitals (the model's sp3 basis, s first on both atoms).  Eigenvectors
    # are reduced to four weights per (k, band) where they are produced; 4 x 401 numbers come back
    if model.size == 8:
        groups = {"s": [0, 4], "p": [1, 2, 3, 5, 6, 7]}
        model.pdos((n, n, n), energies[:2], list(groups.values()))  # warm up
        t0 = time.perf_counter()
        projected = model.pdos((n, n, n), energies, list(groups.values()))
        dt = time.perf_counter() - t0
        print("projected DOS on the same mesh in %.1f ms; s + p against the total: %.1e" % (dt * 1e3, np.abs(projected.nos.sum(axis=0) - result.nos).max()))
        for name, nos, dos in zip(groups, projected.nos, projected.dos):
            peak = np.argmax(dos)
            print("  %s: %.4f states in all, peak %.3f states per energy unit at %.3f" % (name, nos[-1], dos[peak], mid[peak]))

        # 5. the valence charge per orbital: four filled bands, every state weighted by its tetrahedron integration weight at the
        # Fermi level of step 3 and by |U|^2; weights and eigenvectors stay on the GPU, 3 x 8 + 4 numbers come back
        model.occupations((n, n, n), n_electrons=4)  # warm up
        t0 = time.perf_counter()
        occ = model.occupations((n, n, n), n_electrons=4)
        dt = time.perf_counter() - t0
        print("valence charge per orbital at n = 4 in %.1f ms (mu = %.6f): %s, %.12f in all"
              % (dt * 1e3, occ.mu.mu, " ".join("%.4f" % x for x in occ.orbital_occ), occ.orbital_occ.sum()))
        print("  band occupations %s, band energy %.6f per cell" % (" ".join("%g" % x for x in occ.band_occ), occ.band_energy.sum()))

        # 6. the density matrix of those four bands at the model's own hopping vectors: the bond order between the first orbitals
        # of the two atoms across the nearest-neighbour bond, and the band energy again, now as a sum over bonds --
        # 2 Re sum_R sum_ij conj(rho(R)_ij) hop[R]_ij for the stored half of the hoppings; NR x 8 x 8 complex numbers come back
        model.density_matrix((n, n, n), n_electrons=4)  # warm up
        t0 = time.perf_counter()
        dm = model.density_matrix((n, n, n), n_electrons=4)
        dt = time.perf_counter() - t0
        _, hop = model.packed_hop()
        bonds = 2.0 * np.real(np.conj(dm.rho) * hop).sum(axis=(1, 2))
        # rho(R)[i][j] joins orbital i of the home cell and orbital j of cell R; the stored half holds R or -R, and
        # rho(-R) = rho(R)^H.  The nearest image of orbital 4 as seen from orbital 0, by the Cartesian length of pos[4] + R - pos[0]:
        pos = np.asarray(model.pos, dtype=float)
        cell = np.eye(model.dim) if model.uc is None else np.asarray(model.uc, dtype=float)
        signed = np.concatenate([dm.R, -dm.R])
        nearest = int(np.argmin(np.linalg.norm((pos[4] + signed - pos[0]) @ cell, axis=1)))
        index, flipped = nearest % len(dm.R), nearest >= len(dm.R)
        order = np.conj(dm.rho[index][4, 0]) if flipped else dm.rho[index][0, 4]
        print("density matrix at %d lattice vectors in %.1f ms: nearest-neighbour bond order between orbitals 0 and 4 %.4f at R = %s"
              % (len(dm.R), dt * 1e3, order.real, tuple(int(x) for x in signed[nearest])))
        print("  band energy from the bonds %.6f per cell (occupations: %.6f), largest single vector %.6f"
              % (bonds.sum(), occ.band_energy.sum(), bonds[np.argmax(np.abs(bonds))]))

        # 7. the bare susceptibility chi_0(q) along Gamma - X, q = (j, 0, j) / 20 in reduced coordinates (X = (1/2, 0, 1/2)), at k_B T = 0.05 with the chemical
        # potential in the gap: one n x n overlap per (k, q) pair on the matrix pipe, one number per q comes back
        m = 20
        line = np.array([[j, 0, j] for j in range(m // 2 + 1)], dtype=np.int64)
        model.susceptibility((m, m, m), line, temperature=0.05, n_electrons=4)  # warm up
        t0 = time.perf_counter()
        chi = model.susceptibility((m, m, m), line, temperature=0.05, n_electrons=4)
        dt = time.perf_counter() - t0
        print("chi_0 along Gamma - X on a %d^3 mesh at k_B T = 0.05 in %.1f ms (mu = %.6f):" % (m, dt * 1e3, chi.mu.mu))
        print("  " + " ".join("%.4f" % x for x in chi.chi))

        # 8. the dynamic chi_0(q, omega + i eta) at X over a dozen frequencies: the same overlaps, the frequencies walked in registers.  Im chi_0
        # (>= 0 at positive frequencies with this sign of chi_0) is the particle-hole spectrum: nothing below the gap but the tail of the broadening eta
        omega = np.linspace(0.0, 11.0, 12)
        x_point = np.array([[m // 2, 0, m // 2]], dtype=np.int64)
        model.dynamic_susceptibility((m, m, m), x_point, omega, eta=0.1, temperature=0.05, n_electrons=4)  # warm up
        t0 = time.perf_counter()
        dyn = model.dynamic_susceptibility((m, m, m), x_point, omega, eta=0.1, temperature=0.05, n_electrons=4)
        dt = time.perf_counter() - t0
        print("Im chi_0(X, omega + 0.1 i) at omega = %g ... %g on the same mesh in %.1f ms (Re chi_0(X, 0.1 i) = %.4f):" % (omega[0], omega[-1], dt * 1e3, dyn.chi[0, 0].real))
        print("  " + " ".join("%.4f" % x for x in dyn.chi[0].imag))

        # 9. the orbital-resolved chi_0[i, j](q) on the same line: an 8 x 8 Hermitian matrix per q, one rank-(NK n^2) update on the matrix pipe.  Its
        # largest eigenvalue is what a Stoner / RPA criterion reads (an instability where U times it reaches 1); the sum of its entries is chi_0(q) of step 7
        model.orbital_susceptibility((m, m, m), line, temperature=0.05, n_electrons=4)  # warm up
        t0 = time.perf_counter()
        orb = model.orbital_susceptibility((m, m, m), line, temperature=0.05, n_electrons=4)
        dt = time.perf_counter() - t0
        print("largest eigenvalue of chi_0[i, j](q) along Gamma - X on the same mesh in %.1f ms (max |sum_ij chi_0[i, j] - chi_0| = %.1e):"
              % (dt * 1e3, np.abs(orb.chi.sum(axis=(1, 2)) - chi.chi).max()))
        print("  " + " ".join("%.4f" % x for x in np.linalg.eigvalsh(orb.chi)[:, -1]))


if __name__ == "__main__":
    main()
