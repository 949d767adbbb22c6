"""
ctypes binding of ``libtbk.so`` (C ABI: ``include/tbk.h``).

There is deliberately no fallback: if the library is missing or no GPU is visible, the compute
entry points raise.  Importing this module does not load the library -- :func:`lib` does, on first
use -- so the pure-host parts of the package (model construction, synthetic generators, argument
checks) work on a machine without a GPU or a build.
"""

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (TBK_LIBTBK: another build of the same library -- e.g. a -D variant build of tools/build_variants.sh -- under the package's
# Python paths; the product never sets it)
LIB_PATH = os.environ.get("TBK_LIBTBK") or os.path.join(_HERE, "libtbk.so")

TBK_OK = 0
TBK_ERR_ARGUMENT = 1
TBK_ERR_DEVICE = 2
TBK_ERR_MEMORY = 3
TBK_ERR_NOT_FINITE = 4
TBK_ERR_NO_CONVERGENCE = 5
TBK_ERR_SINGULAR = 6

TBK_EIG_AUTO, TBK_EIG_WAVE, TBK_EIG_ROCSOLVER = 0, 1, 2
TBK_OPT_EIGENSOLVER, TBK_OPT_K_CHUNK, TBK_OPT_TIMING, TBK_OPT_FOLD, TBK_OPT_STRASSEN, TBK_OPT_STRASSEN_LEVELS = 1, 2, 3, 4, 5, 6
TBK_OPT_STRASSEN_COMBINE = 7
TBK_REDUCE_AUTO, TBK_REDUCE_ONE_STAGE, TBK_REDUCE_TWO_STAGE = 0, 1, 2
TBK_CNT_EIGENVAL_CALLS, TBK_CNT_FOLDED_CALLS, TBK_CNT_FOLDED_KPOINTS, TBK_CNT_LIBRARY_CALLS, TBK_CNT_STRASSEN_LAUNCHES = 0, 1, 2, 3, 4
TBK_CNT_STRASSEN2_LAUNCHES = 5
TBK_CNT_STRASSEN2_SPLIT = 6
TBK_T_PHASE, TBK_T_HK, TBK_T_EIG, TBK_T_QL, TBK_T_COUNT = 0, 1, 2, 3, 4
STAGE_NAMES = ("phase", "hk", "eig", "ql")
TBK_PDOS_MAX_GROUPS = 16

_c_int = ctypes.c_int
_c_i64 = ctypes.c_int64
_vp = ctypes.c_void_p
_pp = ctypes.POINTER(ctypes.c_void_p)

#: name -> (restype, argtypes); one entry per function declared in include/tbk.h
SIGNATURES = {
    "tbk_version": (ctypes.c_char_p, []),
    "tbk_last_error": (ctypes.c_char_p, []),
    "tbk_device_count": (_c_int, [ctypes.POINTER(_c_int)]),
    "tbk_model_create_dense": (_c_int, [_c_int, _c_int, _c_int, _c_i64, _vp, _vp, _pp]),
    "tbk_model_create_csr": (_c_int, [_c_int, _c_int, _c_int, _c_i64, _vp, _vp, _vp, _vp, _vp, _pp]),
    "tbk_model_destroy": (None, [_vp]),
    "tbk_model_set_option": (_c_int, [_vp, _c_int, _c_i64]),
    "tbk_model_info": (
        _c_int,
        [_vp, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int), ctypes.POINTER(_c_int), ctypes.POINTER(_c_i64),
         ctypes.POINTER(_c_int), ctypes.POINTER(_c_i64)],
    ),
    "tbk_hamilton": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp, _vp]),
    "tbk_eigenval": (_c_int, [_vp, _vp, _c_i64, _vp]),
    "tbk_eigenval_multi": (_c_int, [_vp, _c_int, _vp, _c_i64, _vp]),
    "tbk_hamilton_multi": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_int, _vp, _vp]),
    "tbk_eigh": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp, _vp, _vp]),
    "tbk_eigh_multi": (_c_int, [_vp, _c_int, _vp, _c_i64, _c_int, _vp, _vp, _vp]),
    "tbk_eigh_device": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp, _vp, _vp]),
    "tbk_hamilton_device": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp, _vp]),
    "tbk_eigenval_device": (_c_int, [_vp, _vp, _c_i64, _vp]),
    "tbk_eigenval_device_hint": (_c_int, [_vp, _vp, _vp, _c_i64, _vp]),
    "tbk_model_counter": (_c_int, [_vp, _c_int, ctypes.POINTER(_c_i64)]),
    "tbk_eigenval_schedule": (_c_int, [_vp, _c_i64, ctypes.POINTER(_c_i64), _c_int, ctypes.POINTER(_c_int)]),
    "tbk_eigenval_check": (_c_int, [_vp]),
    "tbk_synchronize": (_c_int, [_vp]),
    "tbk_tridiagonal_reduce": (_c_int, [_c_int, _c_int, _c_i64, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_reduce_standalone": (_c_int, [_c_int, _c_int, _c_i64, _c_int, ctypes.POINTER(ctypes.c_double)]),
    "tbk_dos_from_eigenvalues": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp]),
    "tbk_dos": (_c_int, [_vp, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp]),
    "tbk_dos_multi": (_c_int, [_vp, _c_int, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp]),
    "tbk_dos_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_pdos_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _c_int, _vp, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp]),
    "tbk_pdos": (_c_int, [_vp, _vp, _vp, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp]),
    "tbk_pdos_multi": (_c_int, [_vp, _c_int, _vp, _vp, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp]),
    "tbk_pdos_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_nos_at_from_eigenvalues": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, _c_i64, _vp]),
    "tbk_band_edges_from_eigenvalues": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_fermi_from_eigenvalues": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, ctypes.c_double, _vp, ctypes.POINTER(ctypes.c_int32)]),
    "tbk_band_edges": (_c_int, [_vp, _vp, _vp, _vp]),
    "tbk_fermi": (_c_int, [_vp, _vp, ctypes.c_double, _vp]),
    "tbk_band_edges_multi": (_c_int, [_vp, _c_int, _vp, _vp, _vp]),
    "tbk_fermi_multi": (_c_int, [_vp, _c_int, _vp, ctypes.c_double, _vp]),
    "tbk_fermi_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_tetra_weights_from_eigenvalues": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, ctypes.c_double, _vp]),
    "tbk_occupations_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, ctypes.c_double, _c_i64, _vp, _vp, _vp]),
    "tbk_tetra_weights": (_c_int, [_vp, _vp, ctypes.c_double, _vp]),
    "tbk_occupations": (_c_int, [_vp, _vp, _c_int, ctypes.c_double, _vp, _vp, _vp, _vp]),
    "tbk_tetra_weights_multi": (_c_int, [_vp, _c_int, _vp, ctypes.c_double, _vp]),
    "tbk_occupations_multi": (_c_int, [_vp, _c_int, _vp, _c_int, ctypes.c_double, _vp, _vp, _vp, _vp]),
    "tbk_occ_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_density_matrix_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, ctypes.c_double, _c_i64, _c_i64, _vp, _vp]),
    "tbk_density_matrix": (_c_int, [_vp, _vp, _c_int, ctypes.c_double, _c_i64, _vp, _vp, _vp]),
    "tbk_density_matrix_multi": (_c_int, [_vp, _c_int, _vp, _c_int, ctypes.c_double, _c_i64, _vp, _vp, _vp]),
    "tbk_dm_plan": (_c_int, [_c_i64, _c_int, _c_i64, ctypes.POINTER(_c_i64)]),
    "tbk_dm_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_green_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, _c_i64, _c_i64, _c_i64, _vp, _c_i64, _vp, _vp]),
    "tbk_green_function": (_c_int, [_vp, _vp, _c_i64, _vp, _c_i64, _vp, _vp]),
    "tbk_green_function_multi": (_c_int, [_vp, _c_int, _vp, _c_i64, _vp, _c_i64, _vp, _vp]),
    "tbk_green_plan": (_c_int, [_c_i64, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, ctypes.POINTER(_c_i64)]),
    "tbk_green_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_green_dressed_from_matrices": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _c_i64, _c_i64, _c_i64, _vp, _vp, _c_i64, _vp, _vp]),
    "tbk_green_dressed": (_c_int, [_vp, _vp, _c_i64, _vp, _vp, _c_i64, _vp, _vp]),
    "tbk_green_dressed_multi": (_c_int, [_vp, _c_int, _vp, _c_i64, _vp, _vp, _c_i64, _vp, _vp]),
    "tbk_green_dressed_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_surface_from_matrices": (_c_int, [_c_int, _c_int, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _c_i64, _c_int, _vp, _vp, _vp, _vp]),
    "tbk_surface_green": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_i64, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    "tbk_surface_green_multi": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_i64, _c_i64, _vp, _c_int, _c_int, _vp, _vp, _vp, _vp]),
    "tbk_surface_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_transmission_from_matrices": (_c_int, [_c_int, _c_int, _c_i64, _vp, _vp, _c_int, _vp, _c_i64, _vp, _c_int, _c_i64, _vp, _vp, _vp]),
    "tbk_transmission": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_int, _vp, _c_i64, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_transmission_multi": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_i64, _c_int, _vp, _c_i64, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_transmission_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_transmission_ensemble_from_matrices": (_c_int, [_c_int, _c_int, _c_i64, _vp, _vp, _c_int, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _c_i64, _c_i64,
                                                         _vp, _vp]),
    "tbk_transmission_ensemble": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_int, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _vp, _vp]),
    "tbk_transmission_ensemble_multi": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_i64, _c_int, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _vp, _vp]),
    "tbk_transmission_ensemble_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_transmission_channels_from_matrices": (_c_int, [_c_int, _c_int, _c_i64, _vp, _vp, _c_int, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _c_i64, _c_i64,
                                                         _vp, _vp, _vp]),
    "tbk_transmission_channels": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_int, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_transmission_channels_multi": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_i64, _c_int, _c_i64, _vp, _vp, _c_i64, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_transmission_channels_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_device_green_from_matrices": (_c_int, [_c_int, _c_int, _c_i64, _vp, _vp, _c_int, _vp, _c_i64, _vp, _c_int, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp,
                                                _vp, _vp, _vp]),
    "tbk_device_green": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_int, _vp, _c_i64, _vp, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tbk_device_green_multi": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_i64, _c_int, _vp, _c_i64, _vp, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "tbk_device_green_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_device_current_from_matrices": (_c_int, [_c_int, _c_int, _c_i64, _vp, _vp, _c_int, _vp, _c_i64, _vp, _c_int, _c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _vp]),
    "tbk_device_current": (_c_int, [_vp, _c_int, _c_int, _vp, _c_i64, _c_int, _vp, _c_i64, _vp, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp]),
    "tbk_device_current_multi": (_c_int, [_vp, _c_int, _c_int, _c_int, _vp, _c_i64, _c_int, _vp, _c_i64, _vp, _c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _vp, _vp]),
    "tbk_device_current_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_chi_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _vp, _vp]),
    "tbk_susceptibility": (_c_int, [_vp, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_int, _c_int, _vp, _vp, _vp]),
    "tbk_susceptibility_multi": (_c_int, [_vp, _c_int, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_int, _c_int, _vp, _vp, _vp]),
    "tbk_chi_plan": (_c_int, [_c_i64, _c_int, _c_i64, _c_int, _c_i64, ctypes.POINTER(_c_i64)]),
    "tbk_chi_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_chi_dynamic_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _vp, _c_i64, _vp,
                                                  ctypes.c_double, _c_i64, _vp]),
    "tbk_dynamic_susceptibility": (_c_int, [_vp, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_i64, _vp, ctypes.c_double, _c_int, _c_int,
                                            _vp, _vp, _vp]),
    "tbk_dynamic_susceptibility_multi": (_c_int, [_vp, _c_int, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_i64, _vp, ctypes.c_double,
                                                  _c_int, _c_int, _vp, _vp, _vp]),
    "tbk_chi_dynamic_plan": (_c_int, [_c_i64, _c_int, _c_i64, _c_i64, _c_int, _c_i64, ctypes.POINTER(_c_i64)]),
    "tbk_chi_orbital_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _vp, _c_int, _vp,
                                                  _c_i64, _c_i64, _vp]),
    "tbk_orbital_susceptibility": (_c_int, [_vp, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_int, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_orbital_susceptibility_multi": (_c_int, [_vp, _c_int, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_int, _vp, _c_int, _vp,
                                                  _vp, _vp]),
    "tbk_chi_orbital_plan": (_c_int, [_c_i64, _c_int, _c_int, _c_i64, _c_i64, _c_i64, ctypes.POINTER(_c_i64)]),
    "tbk_chi_orbital_dynamic_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _vp,
                                                          _c_int, _vp, _c_i64, _vp, ctypes.c_double, _c_i64, _c_i64, _vp]),
    "tbk_dynamic_orbital_susceptibility": (_c_int, [_vp, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_i64, _vp, ctypes.c_double,
                                                    _c_int, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_dynamic_orbital_susceptibility_multi": (_c_int, [_vp, _c_int, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_i64, _vp,
                                                          ctypes.c_double, _c_int, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_chi_orbital_dynamic_plan": (_c_int, [_c_i64, _c_int, _c_int, _c_i64, _c_i64, _c_i64, _c_i64, ctypes.POINTER(_c_i64)]),
    "tbk_chi_tensor_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_int, _vp,
                                                 _c_i64, _c_i64, _vp]),
    "tbk_susceptibility_tensor": (_c_int, [_vp, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_susceptibility_tensor_multi": (_c_int, [_vp, _c_int, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_chi_tensor_plan": (_c_int, [_c_i64, _c_int, _c_int, _c_i64, _c_i64, _c_i64, ctypes.POINTER(_c_i64)]),
    "tbk_berry_links_from_eigensystem": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp]),
    "tbk_berry_flux_from_links": (_c_int, [_c_int, _c_int, _vp, _c_int, _vp, _vp, _vp]),
    "tbk_berry_flux": (_c_int, [_vp, _vp, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp]),
    "tbk_berry_flux_multi": (_c_int, [_vp, _c_int, _vp, _c_int, _vp, _c_int, _vp, _vp, _vp, _vp]),
    "tbk_berry_plan": (_c_int, [_c_i64, _c_int, _c_int, _vp, ctypes.POINTER(_c_i64)]),
    "tbk_berry_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_optical_conductivity": (_c_int, [_vp, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, ctypes.c_double, _c_int, _vp, _c_i64, _vp,
                                          _vp]),
    "tbk_optical_conductivity_multi": (_c_int, [_vp, _c_int, _vp, _c_int, ctypes.c_double, ctypes.c_double, _c_i64, _vp, ctypes.c_double, _c_int, _vp,
                                                _c_i64, _vp, _vp]),
    "tbk_optics_from_eigensystem": (_c_int, [_c_int, _c_int, _c_int, _c_i64, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _c_i64, _vp,
                                             ctypes.c_double, _c_i64, _vp]),
    "tbk_optics_plan": (_c_int, [_c_i64, _c_int, _c_int, _c_i64, _c_i64, ctypes.POINTER(_c_i64)]),
    "tbk_optics_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_hamilton_derivative_device": (_c_int, [_vp, _vp, _c_i64, _c_int, _vp]),
    "tbk_transport_distribution": (_c_int, [_vp, _vp, ctypes.c_double, ctypes.c_double, _c_i64, ctypes.c_double, _vp, _vp]),
    "tbk_transport_distribution_multi": (_c_int, [_vp, _c_int, _vp, ctypes.c_double, ctypes.c_double, _c_i64, ctypes.c_double, _vp, _vp]),
    "tbk_tdf_weights_from_eigensystem": (_c_int, [_c_int, _c_int, _c_int, _c_i64, _vp, _vp, _vp, ctypes.c_double, _vp, _vp]),
    "tbk_tdf_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_kdotp_create": (_c_int, [_c_int, _c_int, _c_int, _c_i64, _vp, _vp, _pp]),
    "tbk_kdotp_destroy": (None, [_vp]),
    "tbk_kdotp_hamilton": (_c_int, [_vp, _vp, _c_i64, _vp]),
    "tbk_kdotp_eigenval": (_c_int, [_vp, _vp, _c_i64, _vp]),
    "tbk_kdotp_eigenval_multi": (_c_int, [_vp, _c_int, _vp, _c_i64, _vp]),
    "tbk_kdotp_hamilton_multi": (_c_int, [_vp, _c_int, _vp, _c_i64, _vp]),
    "tbk_kdotp_eigh": (_c_int, [_vp, _vp, _c_i64, _vp, _vp]),
    "tbk_kdotp_eigh_multi": (_c_int, [_vp, _c_int, _vp, _c_i64, _vp, _vp]),
    "tbk_kdotp_coefficients": (_c_int, [_vp, _vp, _c_i64, _vp, _vp, _vp]),
    "tbk_device_malloc": (_c_int, [_c_int, _c_i64, _pp]),
    "tbk_device_free": (_c_int, [_c_int, _vp]),
    "tbk_memcpy_h2d": (_c_int, [_c_int, _vp, _vp, _c_i64]),
    "tbk_memcpy_d2h": (_c_int, [_c_int, _vp, _vp, _c_i64]),
    "tbk_device_mem_info": (_c_int, [_c_int, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)]),
    "tbk_get_timing": (_c_int, [_vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_c_i64), _c_int]),
    "tbk_comm_unique_id": (_c_int, [_vp]),
    "tbk_comm_create": (_c_int, [_c_int, _c_int, _c_int, _vp, _pp]),
    "tbk_comm_destroy": (None, [_vp]),
    "tbk_comm_ranks": (_c_int, [_vp, ctypes.POINTER(_c_int), ctypes.POINTER(_c_int)]),
    "tbk_comm_allgather_f64": (_c_int, [_vp, _vp, _vp, _vp, _c_i64]),
    "tbk_comm_allgather_f64_overlapped": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_int]),
    "tbk_comm_wait_slot": (_c_int, [_vp, _vp, _c_int]),
    "tbk_comm_synchronize": (_c_int, [_vp]),
    "tbk_comm_agree": (_c_int, [_vp, _c_int, _vp]),
    "tbk_comm_prepare_gather": (_c_int, [_vp, _c_int, _c_i64]),
    "tbk_eigenval_device_gather": (_c_int, [_vp, _vp, _vp, _vp, _c_i64, _c_i64, _c_int, _vp, _vp]),
    "tbk_mfma_f64_peak": (_c_int, [_c_int, ctypes.POINTER(ctypes.c_double)]),
}

_LIB = None


class TbkLibraryError(RuntimeError):
    """``libtbk.so`` is missing or cannot be loaded: the product path has no CPU fallback."""


def lib():
    """The loaded ``libtbk.so`` (loads it on first call; raises :class:`TbkLibraryError` if absent)."""
    global _LIB  # pylint: disable=global-statement
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise TbkLibraryError(
                "{} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C tbmodels_amd/csrc`). There is no CPU fallback.".format(LIB_PATH)
            )
        try:
            handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        except OSError as exc:
            raise TbkLibraryError("cannot load {}: {}".format(LIB_PATH, exc)) from exc
        for name, (restype, argtypes) in SIGNATURES.items():
            func = getattr(handle, name)
            func.restype = restype
            func.argtypes = argtypes
        _LIB = handle
    return _LIB


def last_error():
    msg = lib().tbk_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(status):
    """Map a ``tbk_status`` to the exception the reference's callers would see for the same condition."""
    if status == TBK_OK:
        return
    msg = last_error()
    if status in (TBK_ERR_ARGUMENT, TBK_ERR_NOT_FINITE):
        raise ValueError(msg)
    if status == TBK_ERR_MEMORY:
        raise MemoryError(msg)
    if status == TBK_ERR_NO_CONVERGENCE:
        raise np.linalg.LinAlgError(msg)  # what scipy.linalg.eigvalsh raises
    if status == TBK_ERR_SINGULAR:
        raise np.linalg.LinAlgError(msg)  # what numpy.linalg.inv raises
    raise RuntimeError(msg)


def ptr(array):
    """Address of a C-contiguous numpy array as an ``int`` (or None): what a ``void*`` parameter of the ctypes signatures takes.
    (``array.ctypes.data_as(c_void_p)`` builds two ctypes objects per call: 2.1 us against 0.9 -- three pointers per one-k call.)"""
    if array is None:
        return None
    assert array.flags.c_contiguous
    return array.__array_interface__["data"][0]


def device_count():
    count = ctypes.c_int(0)
    check(lib().tbk_device_count(ctypes.byref(count)))
    return count.value
