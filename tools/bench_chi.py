"""
Model.susceptibility measurements: prints one table.

For the silicon model on a 32^3 mesh and a synthetic dense model of 64 orbitals and 64 lattice vectors on a 24^3 mesh, each with
NQ = 1, 16 and 128 vectors q_j = (j, 0, 0), j = 1 .. NQ (a straight line; beyond the mesh it wraps, which costs the same), with
matrix elements, best of --reps after a warm-up:

1. wall time of Model.susceptibility;
2. the three stages of tbk_chi_timing per call: the Fermi tables, the overlaps with their epilogue, the reduction; and the rest of
   the call (wall time minus the stages: eigenvalues and mu by the slab route, then the eigensystem of the whole mesh);
3. the overlap stage's executed flops, 8 n_pad^3 per (k, q) pair with n_pad = n rounded up to 16, over its time, as a fraction of
   tbk_mfma_f64_peak of the same run;
4. the only route to the same numbers without this call: Model.eigh of the mesh to the host and tools/chi_model.py.  Both are
   TIMED ON THE FIRST TWO PLANES of the mesh (the model on those planes as a periodic mesh of their own, at most two vectors) AND
   SCALED to the mesh and to NQ, and printed as such.

With --omegas N[,N...] it prints the table of Model.dynamic_susceptibility instead: for every NW of the list,
NW frequencies evenly spaced over [0, 2 bandwidths), eta = --eta, NQ = 1 and 16; the same stages (the overlap stage now holds the
dynamic epilogue); the epilogue's share of the overlap stage as that stage's time less the static call's overlap stage for the same
vectors, measured in the same run; its f64 VALU rate, EPILOGUE_VALU instructions per (pair of states of the padded block, frequency) over that time, as a
fraction of --valu-peak (lane-instructions per second of the whole chip); and the host route, Model.eigh + chi_model.dynamic_susceptibility,
timed on two planes, at most two vectors and at most four frequencies and scaled.

With --orbital --omegas N[,N...] it prints the table of Model.dynamic_orbital_susceptibility: silicon on 32^3 and
the dense 64-orbital model on 24^3 with 64 of 64 and 16 of 64 orbitals, NQ = 1 and 8, NW from the list; the call and its three stages,
the update per (q, omega), its executed and written flops over tbk_mfma_f64_peak, the STATIC orbital call's update stage per vector
from the same session as the yardstick, and the host route timed on two planes at one (q, omega) and scaled (marked so).

With --orbital it prints the table of Model.orbital_susceptibility instead, NQ = 1 and 8 (--orbitals m: the
first m orbitals only): the same stages (the overlap stage is the rank-K update), the update's flops -- 2048 n n_pad per (k, q) and
tile of 16 x 16, n_pad = n rounded up to 16 -- over its time as a fraction of tbk_mfma_f64_peak, twice: for the tiles with i <= j of
the selection, which are the ones written, and for all the tiles the kernel multiplies (the four-wave template multiplies whole
64 x 64 blocks, the tiles of the padding and those below the diagonal of a diagonal block included); and the host route at one
vector, Model.eigh + chi_model.orbital_susceptibility, timed on two planes and scaled.

With --tensor it prints the table of Model.susceptibility_tensor instead for synthetic dense models: 10 of 10
orbitals on 32 x 32 and on 16^3, 16 of 64 on 16^3 and 3 of 8 on 64 x 64, NQ = 1 and 8: ms per vector (best, median and worst of --reps
calls after a warm-up), the three stages of the best call, the executed flops of stage A (Q = W t) and stage B (X += P Q^T) per
(k, q) as the kernel issues them -- whole blocks of 64 x 64, padding included -- stage B's rate over the kernel's whole time against
tbk_mfma_f64_peak, the same selection the direct way AS AN ESTIMATE (the rank-K update stage of Model.orbital_susceptibility times the
flop ratio 8 n^2 m^4 / 8 n^2 m^2 = m^2), and for the first shape the host route at one vector, Model.eigh + chi_model.susceptibility_tensor,
timed on two rows of the mesh and scaled.

    python tools/bench_chi.py [--reps 3] [--filling 0.3] [--temperature 0.05] [--quick] [--omegas 1,16,128 [--eta 0.05]] [--orbital [--orbitals m]] [--tensor]
"""

import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import tbmodels_amd  # noqa: E402  pylint: disable=wrong-import-position
from tbmodels_amd import _lib, synthetic  # noqa: E402  pylint: disable=wrong-import-position
import chi_model  # noqa: E402  pylint: disable=wrong-import-position
import dos_model  # noqa: E402  pylint: disable=wrong-import-position


def _best(call, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return min(times), out


def measure(name, model, mesh, counts, filling, T, reps, peak_tflops):
    lib = _lib.lib()
    n, n_k = model.size, int(np.prod(mesh))
    n_el = filling * n
    n_pad = (n + 15) // 16 * 16
    handle = model._staged()
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)

    # the host route on two planes: their eigensystem, then the model on them as a mesh of their own
    kpts = np.ascontiguousarray(dos_model.mesh_kpoints(mesh))
    plane = int(np.prod(mesh[1:]))
    sub_mesh = (2,) + tuple(mesh[1:])
    model.eigh(kpts[:plane])
    t_eigh, (eig2, vec2) = _best(lambda: model.eigh(kpts[:2 * plane]), max(1, reps - 1))

    for n_q in counts:
        q = np.zeros((n_q, len(mesh)), dtype=np.int64)
        q[:, 0] = np.arange(1, n_q + 1)
        model.susceptibility(mesh, q, temperature=T, n_electrons=n_el)  # warm-up
        t_call, result = _best(lambda: model.susceptibility(mesh, q, temperature=T, n_electrons=n_el), reps)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
        _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
        for _ in range(reps):
            model.susceptibility(mesh, q, temperature=T, n_electrons=n_el)
        _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
        model.timing(reset=True)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
        stages = [x / max(1, calls.value) for x in ms]
        flops = 8.0 * n_pad ** 3 * n_k * n_q
        fraction = flops / (stages[1] * 1e-3) / (peak_tflops * 1e12) if stages[1] > 0 else float("nan")
        few = min(n_q, 2)
        t_model, _ = _best(lambda: chi_model.susceptibility(eig2, vec2, sub_mesh, q[:few], result.mu.mu, T), max(1, reps - 1))
        t_host = (t_eigh + t_model / few * n_q) / 2 * mesh[0]
        print("| %s | %s | %d | %d | %.1f | %.1f | %.3f | %.3f | %.3f | %.3f | %.1f |"
              % (name, "x".join(str(x) for x in mesh), n, n_q, t_call * 1e3, t_call * 1e3 - sum(stages), stages[0], stages[1], stages[2], fraction,
                 t_host * 1e3))
        print("  (%s NQ = %d: mu = %.12g, chi(q_1) = %.12g, min chi = %.6g)" % (name, n_q, result.mu.mu, result.chi[0], result.chi.min()))
        sys.stdout.flush()


EPILOGUE_VALU = 16  # f64 vector instructions per (pair of states, frequency) in the built dynamic epilogue


def measure_dynamic(name, model, mesh, counts, n_ws, filling, T, eta, reps, valu_peak):
    lib = _lib.lib()
    n, n_k = model.size, int(np.prod(mesh))
    n_el = filling * n
    n_pad = (n + 15) // 16 * 16
    handle = model._staged()
    ms, calls = (ctypes.c_double * 3)(), ctypes.c_int64(0)
    kpts = np.ascontiguousarray(dos_model.mesh_kpoints(mesh))
    plane = int(np.prod(mesh[1:]))
    sub_mesh = (2,) + tuple(mesh[1:])
    model.eigh(kpts[:plane])
    t_eigh, (eig2, vec2) = _best(lambda: model.eigh(kpts[:2 * plane]), max(1, reps - 1))
    edges = model.band_edges(mesh)
    width = float(edges.emax.max() - edges.emin.min())

    def stages_of(call):
        call()  # warm-up
        t_call, result = _best(call, reps)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
        _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
        for _ in range(reps):
            call()
        _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
        model.timing(reset=True)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
        return t_call, result, [x / max(1, calls.value) for x in ms]

    for n_q in counts:
        q = np.zeros((n_q, len(mesh)), dtype=np.int64)
        q[:, 0] = np.arange(1, n_q + 1)
        _, _, static = stages_of(lambda: model.susceptibility(mesh, q, temperature=T, n_electrons=n_el))
        for n_w in n_ws:
            omega = np.arange(n_w) * (2.0 * width / n_w)
            t_call, result, stages = stages_of(lambda: model.dynamic_susceptibility(mesh, q, omega, eta=eta, temperature=T, n_electrons=n_el))
            epilogue = stages[1] - static[1]
            rate = EPILOGUE_VALU * float(n_pad) ** 2 * n_k * n_q * n_w / (epilogue * 1e-3) / (valu_peak * 1e9) if epilogue > 0 else float("nan")
            few_q, few_w = min(n_q, 2), min(n_w, 4)
            t_model, _ = _best(lambda: chi_model.dynamic_susceptibility(eig2, vec2, sub_mesh, q[:few_q], result.mu.mu, T, omega[:few_w], eta), 1)
            t_one, _ = _best(lambda: chi_model.dynamic_susceptibility(eig2, vec2, sub_mesh, q[:few_q], result.mu.mu, T, omega[:1], eta), 1)
            per_w = (t_model - t_one) / (few_w - 1) if few_w > 1 else 0.0
            t_host = (t_eigh + (t_one + per_w * (n_w - 1)) / few_q * n_q) / 2 * mesh[0]
            print("| %s | %s | %d | %d | %d | %.1f | %.1f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f |"
                  % (name, "x".join(str(x) for x in mesh), n, n_q, n_w, t_call * 1e3, t_call * 1e3 - sum(stages), stages[0], stages[1], stages[2], static[1],
                     epilogue, rate, t_host * 1e3))
            print("  (%s NQ = %d NW = %d: mu = %.12g, chi(q_1, omega_0) = %.12g%+.12gj)" % (name, n_q, n_w, result.mu.mu, result.chi[0, 0].real, result.chi[0, 0].imag))
            sys.stdout.flush()


def measure_orbital(name, model, mesh, counts, m, filling, T, reps, peak_tflops):
    lib = _lib.lib()
    n, n_k = model.size, int(np.prod(mesh))
    n_el = filling * n
    m = n if m <= 0 else min(m, n)
    chosen = None if m == n else np.arange(m)
    n_pad, tiles = (n + 15) // 16 * 16, (m + 15) // 16
    handle = model._staged()
    ms, calls, plan = (ctypes.c_double * 3)(), ctypes.c_int64(0), (ctypes.c_int64 * 6)()
    kpts = np.ascontiguousarray(dos_model.mesh_kpoints(mesh))
    plane = int(np.prod(mesh[1:]))
    sub_mesh = (2,) + tuple(mesh[1:])
    model.eigh(kpts[:plane])
    t_eigh, (eig2, vec2) = _best(lambda: model.eigh(kpts[:2 * plane]), max(1, reps - 1))
    for n_q in counts:
        q = np.zeros((n_q, len(mesh)), dtype=np.int64)
        q[:, 0] = np.arange(1, n_q + 1)
        call = lambda: model.orbital_susceptibility(mesh, q, temperature=T, n_electrons=n_el, orbitals=chosen)  # noqa: E731
        call()  # warm-up
        t_call, result = _best(call, reps)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
        _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
        best = None
        for _ in range(reps):  # the stages of the call with the shortest update
            call()
            _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
            if best is None or ms[1] < best[1]:
                best = list(ms)
        model.timing(reset=True)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
        _lib.check(lib.tbk_chi_orbital_plan(n_k, n, m, n_q, 0, 0, plan))
        per_tile = 2048.0 * n * n_pad * n_k * n_q
        issued_tiles = 16 * plan[1] if plan[0] == 4 else 1  # (plan: template, blocks, ...)
        fraction = per_tile * (tiles * (tiles + 1) // 2) / (best[1] * 1e-3) / (peak_tflops * 1e12) if best[1] > 0 else float("nan")
        issued = per_tile * issued_tiles / (best[1] * 1e-3) / (peak_tflops * 1e12) if best[1] > 0 else float("nan")
        host = ""
        if n_q == counts[0]:
            t_model, _ = _best(lambda: chi_model.orbital_susceptibility(eig2, vec2, sub_mesh, q[:1], result.mu.mu, T, None, chosen), 1)
            host = "%.1f" % ((t_eigh + t_model * n_q) / 2 * mesh[0] * 1e3)
        print("| %s | %s | %d | %d | %d | %d x %d | %.1f | %.1f | %.3f | %.3f | %.3f | %.3f | %.3f | %s |"
              % (name, "x".join(str(x) for x in mesh), n, m, n_q, plan[3], plan[2], t_call * 1e3, t_call * 1e3 - sum(best), best[0], best[1], best[2],
                 fraction, issued, host))
        print("  (%s NQ = %d: mu = %.12g, largest eigenvalue of chi(q_1) = %.12g, sum = %.12g)"
              % (name, n_q, result.mu.mu, np.linalg.eigvalsh(result.chi[0]).max(), result.chi[0].sum().real))
        sys.stdout.flush()


def measure_orbital_dynamic(name, model, mesh, counts, n_ws, m, filling, T, eta, reps, peak_tflops):
    """The table of Model.dynamic_orbital_susceptibility: per (NQ, NW) the call, its three stages, the time per
    (q, omega), the update's executed and written flops over the MFMA peak, and the static orbital call's update stage per vector from
    the same session as the yardstick."""
    lib = _lib.lib()
    n, n_k = model.size, int(np.prod(mesh))
    n_el = filling * n
    m = n if m <= 0 else min(m, n)
    chosen = None if m == n else np.arange(m)
    n_pad, tiles = (n + 15) // 16 * 16, (m + 15) // 16
    handle = model._staged()
    ms, calls, plan = (ctypes.c_double * 3)(), ctypes.c_int64(0), (ctypes.c_int64 * 10)()
    kpts = np.ascontiguousarray(dos_model.mesh_kpoints(mesh))
    plane = int(np.prod(mesh[1:]))
    sub_mesh = (2,) + tuple(mesh[1:])
    model.eigh(kpts[:plane])
    t_eigh, (eig2, vec2) = _best(lambda: model.eigh(kpts[:2 * plane]), max(1, reps - 1))
    edges = model.band_edges(mesh)
    width = float(edges.emax.max() - edges.emin.min())

    def stages_of(call):
        call()  # warm-up
        t_call, result = _best(call, reps)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
        _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
        best = None
        for _ in range(reps):  # the stages of the call with the shortest update
            call()
            _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
            if best is None or ms[1] < best[1]:
                best = list(ms)
        model.timing(reset=True)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
        return t_call, result, best

    host_done = False
    for n_q in counts:
        q = np.zeros((n_q, len(mesh)), dtype=np.int64)
        q[:, 0] = np.arange(1, n_q + 1)
        _, _, static = stages_of(lambda: model.orbital_susceptibility(mesh, q, temperature=T, n_electrons=n_el, orbitals=chosen))
        for n_w in n_ws:
            omega = np.arange(n_w) * (2.0 * width / n_w)
            t_call, result, best = stages_of(lambda: model.dynamic_orbital_susceptibility(mesh, q, omega, eta=eta, temperature=T, n_electrons=n_el,
                                                                                        orbitals=chosen))
            _lib.check(lib.tbk_chi_orbital_dynamic_plan(n_k, n, m, n_q, n_w, 0, 0, plan))
            chunk, w_pass, passes = plan[4], plan[7], plan[8]
            computed_w = sum(-(-min(w_pass, n_w - p * w_pass) // chunk) * chunk for p in range(passes))  # with the copies of short chunks
            per_tile = 2048.0 * n * n_pad * n_k * n_q
            issued_tiles = 16 * plan[1] if plan[0] == 4 else 1
            executed = per_tile * issued_tiles * computed_w / (best[1] * 1e-3) / (peak_tflops * 1e12) if best[1] > 0 else float("nan")
            written = per_tile * tiles * tiles * n_w / (best[1] * 1e-3) / (peak_tflops * 1e12) if best[1] > 0 else float("nan")
            host = ""
            if not host_done:
                t_model, _ = _best(lambda: chi_model.dynamic_orbital_susceptibility(eig2, vec2, sub_mesh, q[:1], result.mu.mu, T, omega[:1], eta, None,
                                                                                    chosen), 1)
                host = "%.1f (scaled)" % ((t_eigh + t_model * n_q * n_w) / 2 * mesh[0] * 1e3)
                host_done = True
            print("| %s | %s | %d | %d | %d | %d | %d x %d, passes of %d | %.1f | %.1f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %s |"
                  % (name, "x".join(str(x) for x in mesh), n, m, n_q, n_w, plan[3], plan[2], w_pass, t_call * 1e3, t_call * 1e3 - sum(best), best[0], best[1],
                     best[2], best[1] / (n_q * n_w), executed, written, static[1] / n_q, host))
            print("  (%s NQ = %d NW = %d: mu = %.12g, sum of chi(q_1, omega_0) = %.12g%+.12gj)"
                  % (name, n_q, n_w, result.mu.mu, result.chi[0, 0].sum().real, result.chi[0, 0].sum().imag))
            sys.stdout.flush()


def measure_tensor(name, model, mesh, counts, m, filling, T, reps, peak_tflops, host_route):
    lib = _lib.lib()
    n, n_k = model.size, int(np.prod(mesh))
    n_el = filling * n
    chosen = None if m == n else np.arange(m)
    handle = model._staged()
    ms, calls, plan = (ctypes.c_double * 3)(), ctypes.c_int64(0), (ctypes.c_int64 * 6)()
    panels = (n + 15) // 16
    for n_q in counts:
        q = np.zeros((n_q, len(mesh)), dtype=np.int64)
        q[:, 0] = np.arange(1, n_q + 1)
        call = lambda: model.susceptibility_tensor(mesh, q, temperature=T, n_electrons=n_el, orbitals=chosen)  # noqa: E731
        call()  # warm-up
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            result = call()
            times.append(time.perf_counter() - t0)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 1))
        _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
        runs = []
        for _ in range(reps):
            call()
            _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
            runs.append(list(ms))
        kernel = sorted(r[1] for r in runs)
        best = min(runs, key=lambda r: r[1])
        # the same selection through the orbital-resolved call: its update stage, for the estimate of the direct form
        direct = lambda: model.orbital_susceptibility(mesh, q, temperature=T, n_electrons=n_el, orbitals=chosen)  # noqa: E731
        direct()
        _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
        update = []
        for _ in range(reps):
            direct()
            _lib.check(lib.tbk_chi_timing(handle, ms, ctypes.byref(calls), 1))
            update.append(ms[1])
        model.timing(reset=True)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_TIMING, 0))
        _lib.check(lib.tbk_chi_tensor_plan(n_k, n, m, n_q, 0, 0, plan))
        blocks = plan[1]
        flops_b = 2048.0 * 256 * panels * blocks          # per (k, q): 64 MFMAs per wave and panel of b, four waves
        flops_a = 2048.0 * 32 * panels * panels * blocks  # ... 8 MFMAs per wave and pair of panels (b, b')
        rate_b = flops_b * n_k * n_q / (best[1] * 1e-3) / 1e12 if best[1] > 0 else float("nan")
        host = ""
        if host_route and n_q == counts[0]:
            kpts = np.ascontiguousarray(dos_model.mesh_kpoints(mesh))
            row = int(np.prod(mesh[1:]))
            sub_mesh = (2,) + tuple(mesh[1:])
            model.eigh(kpts[:row])
            t_eigh, (eig2, vec2) = _best(lambda: model.eigh(kpts[:2 * row]), max(1, reps - 1))
            t_model, _ = _best(lambda: chi_model.susceptibility_tensor(eig2, vec2, sub_mesh, q[:1], result.mu.mu, T, chosen), 1)
            host = "%.1f" % ((t_eigh + t_model) / 2 * mesh[0] * 1e3)
        times.sort()
        print("| %s | %s | %d | %d | %d | %d x %d, %d blocks | %.2f / %.2f / %.2f | %.3f | %.3f / %.3f / %.3f | %.3f | %.3g | %.3g | %.2f | %.3f | %.1f | %s |"
              % (name, "x".join(str(x) for x in mesh), n, m, n_q, plan[3], plan[2], blocks, times[0] * 1e3 / n_q, times[len(times) // 2] * 1e3 / n_q,
                 times[-1] * 1e3 / n_q, best[0], kernel[0], kernel[len(kernel) // 2], kernel[-1], best[2], flops_a, flops_b, rate_b, rate_b / peak_tflops,
                 min(update) * m * m, host))
        matrix = result.chi[0].reshape(m * m, m * m)
        print("  (%s NQ = %d: mu = %.12g, largest eigenvalue of chi(q_1) = %.12g, trace = %.12g)"
              % (name, n_q, result.mu.mu, np.linalg.eigvalsh(matrix).max(), matrix.trace().real))
        sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--filling", type=float, default=0.3, help="electrons per orbital")
    ap.add_argument("--temperature", type=float, default=0.05, help="k_B T in the model's energy units")
    ap.add_argument("--quick", action="store_true", help="small meshes and lists (a smoke run of the tool)")
    ap.add_argument("--omegas", type=str, default="", help="comma-separated numbers of frequencies: the table of Model.dynamic_susceptibility instead")
    ap.add_argument("--eta", type=float, default=0.05, help="the broadening of the dynamic call")
    ap.add_argument("--valu-peak", type=float, default=39321.6, help="f64 VALU peak in G lane-instructions per second: the data sheet's 78.6 TFLOP/s "
                    "of vector FP64 is one fused multiply-add per lane and cycle, 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz")
    ap.add_argument("--orbital", action="store_true", help="the table of Model.orbital_susceptibility instead")
    ap.add_argument("--orbitals", type=int, default=0, help="with --orbital: the first m orbitals only (0: all)")
    ap.add_argument("--tensor", action="store_true", help="the table of Model.susceptibility_tensor instead")
    args = ap.parse_args()
    if args.tensor:
        tf = ctypes.c_double(0.0)
        _lib.check(_lib.lib().tbk_mfma_f64_peak(0, ctypes.byref(tf)))
        print("FP64 MFMA peak: %.1f TFLOP/s" % tf.value)
        print("| model | mesh | orbitals | selected | NQ | slices x k-points, blocks | Model.susceptibility_tensor ms per vector (best / median / worst) | "
              "Fermi tables ms | two-stage kernel ms (best / median / worst) | reduction ms | stage A flops per (k, q) | stage B flops per (k, q) | "
              "stage B TFLOP/s over the kernel's time | of the MFMA peak | ESTIMATE of the direct form: orbital update stage x m^2, ms | today, one "
              "vector: Model.eigh to the host + tools/chi_model.py ms (two rows, scaled) |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        counts = (1, 2) if args.quick else (1, 8)
        shapes = [(10, 10, (8, 8), 2), (8, 3, (8, 8), 2)] if args.quick else [(10, 10, (32, 32), 2), (10, 10, (16,) * 3, 3), (64, 16, (16,) * 3, 3),
                                                                             (8, 3, (64, 64), 2)]
        for index, (n, m, mesh, dim) in enumerate(shapes):
            r_vec, hop, _ = synthetic.dense_model_arrays(n, 16, synthetic.MODEL_SEED + 40 + index, dim=dim)
            model = tbmodels_amd.Model.from_packed(r_vec, hop)
            measure_tensor("dense %d" % n, model, mesh, counts, m, args.filling, args.temperature, args.reps, tf.value, index == 0)
        return
    if args.orbital:
        tf = ctypes.c_double(0.0)
        _lib.check(_lib.lib().tbk_mfma_f64_peak(0, ctypes.byref(tf)))
        print("FP64 MFMA peak: %.1f TFLOP/s" % tf.value)
        print("| model | mesh | orbitals | selected | NQ | slices x k-points | Model.orbital_susceptibility ms | of it outside the chi kernels (eigenvalues, mu, "
              "eigensystem) ms | Fermi tables ms | rank-K update ms | reduction ms | update / MFMA peak (tiles with i <= j) | update / MFMA peak (all tiles multiplied) | today, one vector: Model.eigh "
              "to the host + tools/chi_model.py ms (two planes, scaled) |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        if args.omegas:
            n_ws = [int(x) for x in args.omegas.split(",")]
            print("| model | mesh | orbitals | selected | NQ | NW | slices x k-points, frequencies per pass | Model.dynamic_orbital_susceptibility ms | of it "
                  "outside the chi kernels ms | Fermi tables ms | complex rank-K update ms | reduction ms | update ms per (q, omega) | update / MFMA peak "
                  "(tiles executed) | update / MFMA peak (tiles written) | STATIC Model.orbital_susceptibility update ms per vector, same session | "
                  "today: Model.eigh to the host + tools/chi_model.py ms (two planes, one (q, omega), scaled) |")
            print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
            counts = (1, 2) if args.quick else (1, 8)
            data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
            silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
            measure_orbital_dynamic("silicon", silicon, (8,) * 3 if args.quick else (32,) * 3, counts, n_ws, 0, args.filling, args.temperature, args.eta,
                                    args.reps, tf.value)
            r_vec, hop, _ = synthetic.dense_model_arrays(64, 64, synthetic.MODEL_SEED + 2)
            dense = tbmodels_amd.Model.from_packed(r_vec, hop)
            for chosen in ((0,) if args.orbitals else (0, 16)):  # 64 of 64 and 16 of 64
                measure_orbital_dynamic("dense 64", dense, (6,) * 3 if args.quick else (24,) * 3, counts, n_ws, args.orbitals or chosen, args.filling,
                                        args.temperature, args.eta, args.reps, tf.value)
            return
        counts = (1, 2) if args.quick else (1, 8)
        data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
        silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
        measure_orbital("silicon", silicon, (8,) * 3 if args.quick else (32,) * 3, counts, args.orbitals, args.filling, args.temperature, args.reps, tf.value)
        r_vec, hop, _ = synthetic.dense_model_arrays(64, 64, synthetic.MODEL_SEED + 2)
        dense = tbmodels_amd.Model.from_packed(r_vec, hop)
        measure_orbital("dense 64", dense, (6,) * 3 if args.quick else (24,) * 3, counts, args.orbitals, args.filling, args.temperature, args.reps, tf.value)
        return
    if args.omegas:
        n_ws = [int(x) for x in args.omegas.split(",")]
        print("| model | mesh | orbitals | NQ | NW | Model.dynamic_susceptibility ms | of it outside the chi kernels ms | Fermi tables ms | overlaps + dynamic "
              "epilogue ms | reduction ms | static overlap stage, same vectors ms | epilogue (difference) ms | epilogue VALU / f64 vector peak | today: "
              "Model.eigh to the host + tools/chi_model.py ms (two planes, at most two vectors and four frequencies, scaled) |")
        print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        counts = (1, 4) if args.quick else (1, 16)
        data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
        silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
        measure_dynamic("silicon", silicon, (8,) * 3 if args.quick else (32,) * 3, counts, n_ws, args.filling, args.temperature, args.eta, args.reps, args.valu_peak)
        r_vec, hop, _ = synthetic.dense_model_arrays(64, 64, synthetic.MODEL_SEED + 2)
        dense = tbmodels_amd.Model.from_packed(r_vec, hop)
        measure_dynamic("dense 64", dense, (6,) * 3 if args.quick else (24,) * 3, counts, n_ws, args.filling, args.temperature, args.eta, args.reps, args.valu_peak)
        return
    tf = ctypes.c_double(0.0)
    _lib.check(_lib.lib().tbk_mfma_f64_peak(0, ctypes.byref(tf)))
    print("FP64 MFMA peak: %.1f TFLOP/s" % tf.value)
    print("| model | mesh | orbitals | NQ | Model.susceptibility ms | of it outside the chi kernels (eigenvalues, mu, eigensystem) ms | Fermi tables ms "
          "| overlaps + epilogue ms | reduction ms | overlap stage / MFMA peak | today: Model.eigh to the host + tools/chi_model.py ms (two planes, "
          "at most two vectors, scaled) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    counts = (1, 4) if args.quick else (1, 16, 128)
    data = np.load(os.path.join(ROOT, "tests", "golden", "silicon.npz"))
    silicon = tbmodels_amd.Model.from_packed(data["R"], data["hop"], pos=data["pos"])
    measure("silicon", silicon, (8,) * 3 if args.quick else (32,) * 3, counts, args.filling, args.temperature, args.reps, tf.value)
    r_vec, hop, _ = synthetic.dense_model_arrays(64, 64, synthetic.MODEL_SEED + 2)
    dense = tbmodels_amd.Model.from_packed(r_vec, hop)
    measure("dense 64", dense, (6,) * 3 if args.quick else (24,) * 3, counts, args.filling, args.temperature, args.reps, tf.value)


if __name__ == "__main__":
    main()
