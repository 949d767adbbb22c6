#!/usr/bin/env python3
"""Every output of the tetrahedron family (csrc/tbk_tetra.h and the four files that include it) on fixed, seeded inputs, in one .npz:
the tool for "does this build give the same bits as that one".  The inputs are the smallest that reach every kernel instantiation
and every tile edge (two and three dimensions, every group tile of the projected kernel, grids that cross a bin tile, two probe
launches, the second band block above 256 orbitals, tied corners and energies on corners), then the Model methods on silicon with
one handle and with two, and the smallest shapes that reach every edge of the cut of a mesh into slabs: meshes (2, 3, 2), (3, 4) and
(1, 4, 3) on the caller's arrays, silicon on (3, 4, 4) with the device lists [0], [0, 0] (slabs of 2 + 1 planes, with neighbour planes)
and [0, 0, 0, 0] (a short slab and an empty one), on (1, 4, 3) with [0, 0] (one busy handle that holds the whole axis), TBK_OPT_K_CHUNK
0 and 5 for the calls that walk eigenvectors, and the density matrix and the susceptibility once on two handles.

    python tools/tetra_dump.py OUT.npz                  (TBK_LIBTBK=/path/to/libtbk.so selects another build of the library)
    python tools/tetra_dump.py --compare A.npz B.npz    exit status 1 unless every array agrees bit for bit (NaN == NaN)
"""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import tetra_exact  # noqa: E402  pylint: disable=wrong-import-position
import tbmodels_amd  # noqa: E402  pylint: disable=wrong-import-position
from tbmodels_amd import _lib  # noqa: E402  pylint: disable=wrong-import-position

MESHES = ((2, 3, 2), (4, 4, 4), (1, 5), (3, 4))
E_MIN = -0.75  # with steps 2^-4 and 2^-11 the grids hit the levels of tetra_exact.tie_rich_inputs exactly


def c_call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*[_lib.ptr(a) if isinstance(a, np.ndarray) else a for a in args]))


def eigenvalue_calls(out, tag, mesh, eig, rng):
    dim, n_orb, nk = len(mesh), eig.shape[-1], int(np.prod(mesh))
    mesh_a = np.array(mesh, dtype=np.int32)
    head = (0, dim, mesh_a, n_orb, eig)

    def run(key, name, result, *args, tail=()):
        c_call(name, *head, *args, *(result if isinstance(result, tuple) else (result,)), *tail)
        out["%s/%s" % (tag, key)] = np.concatenate(result) if isinstance(result, tuple) else result

    for n_e, step in ((37, 2.0 ** -4), (4099, 2.0 ** -11)):
        run("dos%d" % n_e, "tbk_dos_from_eigenvalues", np.empty(n_e), E_MIN, step, n_e)
    for groups, n_e in ((1, 37), (2, 37), (3, 37), (5, 37), (16, 37), (16, 259)):
        weights = rng.uniform(0.0, 1.0, (nk, groups, n_orb))
        nos = out["%s/pdos%d_%d" % (tag, groups, n_e)] = np.empty((groups, n_e))
        c_call("tbk_pdos_from_eigensystem", 0, dim, mesh_a, n_orb, groups, eig, weights, E_MIN, 2.0 ** -4 if n_e == 37 else 2.0 ** -7, n_e, nos)
    corners = np.ravel(eig)[:: max(1, eig.size // 11)][:11]
    probes = np.concatenate([[eig.min() - 1.0], corners, np.linspace(eig.min(), eig.max(), 17 - 2 - len(corners)), [eig.max() + 1.0]])
    run("nos_at", "tbk_nos_at_from_eigenvalues", np.empty(17), probes, 17)
    run("edges", "tbk_band_edges_from_eigenvalues", (np.empty(n_orb), np.empty(n_orb)))
    third = n_orb / 3.0 + (0.1 if n_orb % 3 == 0 else 0.0)
    for i, filling in enumerate((0.5, third, n_orb - 0.25)):
        run("fermi%d" % i, "tbk_fermi_from_eigenvalues", np.empty(4), float(filling), tail=(None,))
    for i, energy in enumerate((float(corners[3 % len(corners)]), 0.0625 + 2.0 ** -9, -0.3)):
        run("weights%d" % i, "tbk_tetra_weights_from_eigenvalues", np.empty(eig.shape), energy)


def library_calls(out):
    rng = np.random.default_rng(20240229)
    for mesh in MESHES:
        for n_orb in (1, 3, 8, 65) + ((257,) if mesh == (2, 3, 2) else ()):
            tag = "x".join(map(str, mesh)) + "_n%d" % n_orb
            flat = (int(np.prod(mesh)), n_orb)
            eigenvalue_calls(out, tag + "_tie", mesh, np.ascontiguousarray(tetra_exact.tie_rich_inputs(mesh, n_orb, 1)[0].reshape(flat)), rng)
            eigenvalue_calls(out, tag + "_uni", mesh, np.sort(rng.uniform(-1.0, 1.0, flat), axis=-1), rng)
    # an integer filling on gapped bands: band b lies inside [3 b, 3 b + 1]
    mesh, gapped = np.array((2, 3, 2), dtype=np.int32), np.sort(rng.uniform(0.0, 1.0, (12, 3)), axis=-1) + 3.0 * np.arange(3)
    out["gapped/fermi"] = np.empty(4)
    c_call("tbk_fermi_from_eigenvalues", 0, 3, mesh, 3, gapped, 1.0, out["gapped/fermi"], None)
    for n in (3, 8, 65):
        eig = np.sort(rng.uniform(-1.0, 1.0, (12, n)), axis=-1)
        vec = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(12, n, n)) + 1j * rng.normal(size=(12, n, n)))[0])
        for k_chunk in (0, 1):
            q, f, eb = np.empty(n), np.empty(n), np.empty(n)
            c_call("tbk_occupations_from_eigensystem", 0, 3, mesh, n, eig, vec.view(np.float64), 0.125, k_chunk, q, f, eb)
            out["occ_n%d_chunk%d" % (n, k_chunk)] = np.concatenate([q, f, eb])


def occupation_calls(out, tag, mesh, eig, vec, chunks):
    mesh_a, n = np.array(mesh, dtype=np.int32), eig.shape[-1]
    for k_chunk in chunks:
        q, f, eb = np.empty(n), np.empty(n), np.empty(n)
        c_call("tbk_occupations_from_eigensystem", 0, len(mesh), mesh_a, n, eig, vec.view(np.float64), 0.125, k_chunk, q, f, eb)
        out["%s/occ_chunk%d" % (tag, k_chunk)] = np.concatenate([q, f, eb])


def slab_calls(out):
    rng = np.random.default_rng(20261021)
    for mesh in ((2, 3, 2), (3, 4), (1, 4, 3)):
        for n in (2, 9):
            nk, tag = int(np.prod(mesh)), "slab_" + "x".join(map(str, mesh)) + "_n%d" % n
            eig = np.sort(rng.uniform(-1.0, 1.0, (nk, n)), axis=-1)
            eigenvalue_calls(out, tag, mesh, eig, rng)
            vec = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(nk, n, n)) + 1j * rng.normal(size=(nk, n, n)))[0])
            occupation_calls(out, tag, mesh, eig, vec, (0, 5))
    g = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    grid, groups = np.linspace(-8.0, 14.0, 65), [[0, 1], [2, 3, 4], [5, 6, 7]]
    for mesh, lists in (((3, 4, 4), ([0], [0, 0], [0, 0, 0, 0])), ((1, 4, 3), ([0, 0],))):
        for devices in lists:
            model = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
            model.devices = devices
            tag = "si_%s_on%d" % ("x".join(map(str, mesh)), len(devices))
            out[tag + "/dos"] = model.dos(mesh, grid).nos
            out[tag + "/edges"] = np.concatenate(model.band_edges(mesh))
            out[tag + "/weights"] = model.tetra_weights(mesh, 3.0)
            for filling in (4, 4.5):
                out["%s/fermi%s" % (tag, filling)] = np.array(model.fermi_level(mesh, filling))
            for k_chunk in (0, 5):
                model.set_option(_lib.TBK_OPT_K_CHUNK, k_chunk)
                out["%s/pdos_chunk%d" % (tag, k_chunk)] = model.pdos(mesh, grid, groups).nos
                for key, how in (("energy", {"energy": 3.0}), ("electrons4", {"n_electrons": 4}), ("electrons4.5", {"n_electrons": 4.5})):
                    occ = model.occupations(mesh, **how)
                    out["%s/occ_%s_chunk%d" % (tag, key, k_chunk)] = np.concatenate([np.array(occ.mu), occ.orbital_occ, occ.band_occ, occ.band_energy])
            if mesh == (3, 4, 4) and len(devices) == 2:  # (the two other callers of the staged occupations)
                rho = model.density_matrix(mesh, n_electrons=4.5)
                out[tag + "/dm"], out[tag + "/dm_mu"] = rho.rho, np.array(rho.mu, dtype=np.float64)
                chi = model.susceptibility(mesh, [[1, 0, 0], [1, 2, 1]], temperature=0.1, n_electrons=4.5)
                out[tag + "/chi"], out[tag + "/chi_mu"] = chi.chi, np.array(chi.mu, dtype=np.float64)


def model_calls(out):
    g = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    single = tbmodels_amd.Model.from_packed(g["R"], g["hop"], pos=g["pos"], uc=g["uc"])
    twin = pickle.loads(pickle.dumps(single))
    twin.devices = [0, 0]
    mesh, grid = (4, 4, 4), np.linspace(-8.0, 14.0, 257)
    for tag, model in (("one", single), ("two", twin)):
        out["si_%s/dos" % tag] = model.dos(mesh, grid).nos
        out["si_%s/pdos" % tag] = model.pdos(mesh, grid, [[0, 1], [2, 3, 4], [5, 6, 7]]).nos
        out["si_%s/edges" % tag] = np.concatenate(model.band_edges(mesh))
        for filling in (4, 4.5):
            out["si_%s/fermi%s" % (tag, filling)] = np.array(model.fermi_level(mesh, filling))
            occ = model.occupations(mesh, n_electrons=filling)
            out["si_%s/occ%s" % (tag, filling)] = np.concatenate([np.array(occ.mu), occ.orbital_occ, occ.band_occ, occ.band_energy])
        out["si_%s/weights" % tag] = model.tetra_weights(mesh, 3.0)


def main(argv):
    if len(argv) == 3 and argv[0] == "--compare":
        a, b = np.load(argv[1]), np.load(argv[2])
        differ = [k for k in sorted(set(a.files) | set(b.files))
                  if k not in a.files or k not in b.files or not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]
        print("%d arrays, %d differ%s" % (len(a.files), len(differ), "".join("\n  " + k for k in differ)))
        return 1 if differ else 0
    if len(argv) != 1:
        print(__doc__)
        return 2
    out = {}
    library_calls(out)
    model_calls(out)
    slab_calls(out)
    np.savez(argv[0], **out)
    print("%s: %d arrays from %s" % (argv[0], len(out), _lib.LIB_PATH))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
