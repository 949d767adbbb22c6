#!/usr/bin/env python3
"""Every output of the calls on the complex FP64 MFMA blocks of csrc/tbk_zmfma.h that tools/lattice_dump.py does not reach -- the six
layered calls, the three susceptibilities, the Berry links and the optical conductivity -- on fixed, seeded inputs, in one .npz: the
tool for "does this build give the same bits as that one".  Everything goes through the `_from_matrices` / `_from_eigensystem` entry
points, so no eigensolver is involved.  The inputs are the smallest that reach every template: principal layers of 9, 20 and 40 rows
(NP = 16, 32, 64: a short last panel, tiles beyond n), 9, 20, 40 and 70 orbitals (BT = 1, BT = 4, two blocks per side), band sets of
5, 20 and 70 bands (BT = 1, BT = 4, the stored M), five frequencies (a short last register chunk).

    python tools/mfma_dump.py OUT.npz                  (TBK_LIBTBK=/path/to/libtbk.so selects another build of the library)
    python tools/mfma_dump.py --compare A.npz B.npz    exit status 1 unless every array agrees bit for bit (NaN == NaN)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tbmodels_amd import _lib  # noqa: E402  pylint: disable=wrong-import-position
import surface_model as sm  # noqa: E402  pylint: disable=wrong-import-position
import transport_model as tm  # noqa: E402  pylint: disable=wrong-import-position

Z = np.array([0.3 + 0.05j, -1.1 - 0.5j])  # either sign of Im z
LAYERS = ((9, 1), (10, 2), (20, 2))       # (n, L): principal layers of 9, 20 and 40 rows
NK, M, S = 2, 3, 2                        # in-plane points, layers of the device, samples of the ensemble
MESHES = ((2, 3, 2), (3, 4))
OMEGA = np.array([0.0, 0.2, -0.7, 0.35, 1.5])
MU, T, ETA = 0.05, 0.02, 0.04


def c_call(name, *args):
    _lib.check(getattr(_lib.lib(), name)(*[_lib.ptr(a) if isinstance(a, np.ndarray) else a for a in args]))


def layered_calls(out):
    nz = len(Z)
    for n, L in LAYERS:
        N = n * L
        _, H00, H01 = sm.random_case(n, L, NK, 29100 + 37 * n + L)
        V = tm.random_device(N, M, 29200 + N)
        rng = np.random.default_rng(29300 + N)
        onsite = np.ascontiguousarray(rng.uniform(-0.5, 0.5, (S, M, N)))
        matrices = np.ascontiguousarray(np.stack([tm.random_device(N, M, 29400 + N + s) for s in range(S)]))
        tag = "N%d" % N

        def new(name, shape, dtype=np.float64):
            a = out["%s/%s" % (name, tag)] = np.full(shape, -1 if dtype == np.int32 else np.nan, dtype=dtype)
            return a

        for spectral in (0, 1):
            shape, dtype = ((NK, nz, N), np.float64) if spectral else ((NK, nz, N, N), np.complex128)
            c_call("tbk_surface_from_matrices", 0, N, NK, H00, H01, nz, Z, 64, 0, spectral, new("surface%d/its" % spectral, (NK, nz), np.int32),
                   *[new("surface%d/%s" % (spectral, side), shape, dtype) for side in ("bottom", "top", "bulk")])
        c_call("tbk_transmission_from_matrices", 0, N, NK, H00, H01, M, V, nz, Z, 64, 0, new("transmission/its", (NK, nz), np.int32),
               new("transmission/T", (NK, nz)), new("transmission/G", (NK, nz, N, N), np.complex128))
        for form, v, e in (("matrix", matrices, None), ("onsite", None, onsite)):
            c_call("tbk_transmission_ensemble_from_matrices", 0, N, NK, H00, H01, M, S, v, e, nz, Z, 64, 0, 0,
                   new("ensemble_%s/its" % form, (NK, nz), np.int32), new("ensemble_%s/T" % form, (NK, nz, S)))
            c_call("tbk_transmission_channels_from_matrices", 0, N, NK, H00, H01, M, S, v, e, nz, Z, 64, 0, 0,
                   new("channels_%s/its" % form, (NK, nz), np.int32), new("channels_%s/T" % form, (NK, nz, S)),
                   new("channels_%s/channels" % form, (NK, nz, S, N)))
        rows = [new("device_green/" + name, (NK, nz, M, N)) for name in ("ldos", "left", "right")]
        c_call("tbk_device_green_from_matrices", 0, N, NK, H00, H01, M, V, nz, Z, 64, 0, 0, new("device_green/its", (NK, nz), np.int32),
               new("device_green/T", (NK, nz)), *rows, *[new("device_green/" + name, (NK, nz, M, N, N), np.complex128) for name in "GFC"])
        rows = [new("device_current/" + name, (NK, nz, M, N)) for name in ("ldos", "left", "right")]
        rows += [new("device_current/" + name, (NK, nz, M - 1, N)) for name in ("current_left", "current_right")]
        rows += [new("device_current/" + name, (NK, nz, M - (name[:5] == "inter"), N, N))
                 for name in ("inter_left", "inter_right", "intra_left", "intra_right")]  # (bonds=True)
        c_call("tbk_device_current_from_matrices", 0, N, NK, H00, H01, M, V, nz, Z, 64, 0, 0, new("device_current/its", (NK, nz), np.int32),
               new("device_current/T", (NK, nz)), *rows)


def eigensystem(rng, nk, n):
    """random ascending bands with an exactly degenerate pair inside every k-point, and a random unitary U"""
    eig = np.sort(rng.uniform(-1.0, 1.0, (nk, n)), axis=-1)
    eig[:, 2] = eig[:, 1]
    U = np.linalg.qr(rng.normal(size=(nk, n, n)) + 1j * rng.normal(size=(nk, n, n)))[0]
    return np.ascontiguousarray(eig), np.ascontiguousarray(U, dtype=np.complex128)


def unit_phases(rng, rows, n):
    angle = rng.uniform(0.0, 2.0 * np.pi, (rows, n))
    return np.ascontiguousarray(np.cos(angle) + 1j * np.sin(angle))


def mesh_calls(out):
    for mesh in MESHES:
        dim, nk = len(mesh), int(np.prod(mesh))
        mesh_a = np.array(mesh, dtype=np.int32)
        q = np.ascontiguousarray(np.concatenate([np.zeros((1, dim)), np.eye(dim), [[d + 1 for d in range(dim)]]]).astype(np.int64))
        for n in (9, 20, 40, 70):
            rng = np.random.default_rng(29500 + 41 * nk + n)
            eig, U = eigensystem(rng, nk, n)
            tables = {"plain": None, "phases": unit_phases(rng, len(q), n)}
            orbitals = np.arange(n, dtype=np.int32)
            for label, phases in tables.items():
                key = "%s_n%d_%s" % ("x".join(map(str, mesh)), n, label)
                chi = out["chi/" + key] = np.full(len(q), np.nan)
                c_call("tbk_chi_from_eigensystem", 0, dim, mesh_a, n, eig, U, MU, T, len(q), q, phases, chi)
                dyn = out["chi_dynamic/" + key] = np.full((len(q), len(OMEGA)), np.nan, dtype=np.complex128)
                c_call("tbk_chi_dynamic_from_eigensystem", 0, dim, mesh_a, n, eig, U, MU, T, len(q), q, phases, len(OMEGA), OMEGA, ETA, 0, dyn)
                orb = out["chi_orbital/" + key] = np.full((len(q), n, n), np.nan, dtype=np.complex128)
                c_call("tbk_chi_orbital_from_eigensystem", 0, dim, mesh_a, n, eig, U, MU, T, len(q), q, phases, n, orbitals, 0, 0, orb)
            if n == 70:
                continue  # (the optical conductivity: up to 40 orbitals here, the fused kernel's three templates)
            D = rng.normal(size=(nk, dim, n, n)) + 1j * rng.normal(size=(nk, dim, n, n))
            D = np.ascontiguousarray((D + D.conj().transpose(0, 1, 3, 2)) / 2.0)
            for label, pos in (("plain", None), ("pos", np.ascontiguousarray(rng.uniform(0.0, 1.0, (n, dim))))):
                sigma = out["optics/%s_n%d_%s" % ("x".join(map(str, mesh)), n, label)] = np.full((len(OMEGA), dim, dim), np.nan, dtype=np.complex128)
                c_call("tbk_optics_from_eigensystem", 0, dim, n, nk, eig, U, D, pos, MU, T, len(OMEGA), OMEGA, ETA, 0, sigma)
        # the Berry links: band sets of 5, 20 and 70 of 72 bands
        n, sets = 72, np.array([[0, 5], [5, 25], [2, 72]], dtype=np.int32)
        rng = np.random.default_rng(29600 + nk)
        _, U = eigensystem(rng, nk, n)
        for label, phases in (("plain", None), ("phases", unit_phases(rng, dim, n))):
            key = "%s_%s" % ("x".join(map(str, mesh)), label)
            links = out["berry/L_" + key] = np.full((len(sets), dim, nk), np.nan, dtype=np.complex128)
            words = out["berry/words_" + key] = np.zeros((len(sets), dim, nk), dtype=np.uint64)
            c_call("tbk_berry_links_from_eigensystem", 0, dim, mesh_a, n, U, len(sets), sets, phases, links, words)


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
    layered_calls(out)
    mesh_calls(out)
    np.savez(argv[0], **out)
    print("%s: %d arrays from %s" % (argv[0], len(out), _lib.LIB_PATH))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
