"""
``KdotpModel`` -- host-side mirror of ``tbmodels.kdotp.KdotpModel``
(``/root/reference/src/tbmodels/kdotp.py:20-100``), evaluated on the GPU.

``H(k) = sum_p prod_d k_d^{p_d} * C_p`` has the same shape as the tight-binding Fourier sum with the
phase rows replaced by monomial rows, so it runs through the same MFMA contraction and batched
eigensolver (``tbk_kdotp_*`` in ``include/tbk.h``).
"""

import ctypes
import threading

import numpy as np

from . import _lib, _outbuf
from ._model import _devices_from_env

__all__ = ("KdotpModel",)


class KdotpModel:
    """
    A k.p model.  ``taylor_coefficients`` maps a tuple of powers of the k components to a Hermitian
    matrix, e.g. ``{(1, 0, 2): [[1, 0], [0, -1]]}`` is ``k_x k_z^2 sigma_z``.
    """

    def __init__(self, taylor_coefficients):
        for mat in taylor_coefficients.values():
            if not np.allclose(mat, np.array(mat).T.conj()):
                raise ValueError("The provided Taylor coefficient {} is not hermitian".format(mat))
        self.taylor_coefficients = {
            tuple(key): np.array(mat, dtype=complex) for key, mat in taylor_coefficients.items()
        }
        self._handles = []
        self._staged_key = None
        self._pinned = False
        self._call_lock = threading.RLock()
        self._devices = _devices_from_env()

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_handles"] = []
        state["_staged_key"] = None
        state.pop("_call_lock", None)
        return state

    def __setstate__(self, state):
        legacy_device = state.pop("device", None)  # states written before a k.p model could sit on several devices
        state.pop("_handle", None)
        self.__dict__.update(state)
        self._handles = []
        if "_devices" not in state:
            self._devices = [int(legacy_device)] if legacy_device is not None else _devices_from_env()
        self._call_lock = threading.RLock()

    def __del__(self):
        self._drop_staging()

    # ------------------------------------------------------------------ devices (the surface of ``Model.devices``)
    @property
    def device(self):
        """The (first) GPU this model evaluates on; assigning an index makes it the only one."""
        return self._devices[0]

    @device.setter
    def device(self, index):
        self.devices = [int(index)]

    @property
    def devices(self):
        """
        GPU indices this model is staged on.  With more than one, ``hamilton`` / ``eigenval`` cut the k list into
        contiguous slabs, one per entry, and every device fills its rows of the result (``tbk_kdotp_eigenval_multi``) -- the
        single call of a single process of ``kdotp.py:51-100``.  Default: ``TBK_DEVICES`` / ``TBK_DEVICE`` / device 0; an
        index may repeat.
        """
        return list(self._devices)

    @devices.setter
    def devices(self, indices):
        indices = [int(i) for i in indices]
        if not indices or any(i < 0 for i in indices):
            raise ValueError("devices must be a non-empty list of GPU indices, got {!r}".format(indices))
        if indices != getattr(self, "_devices", None):
            self._drop_staging()
        self._devices = indices

    @property
    def _handle(self):
        return self._handles[0] if self._handles else None

    def _drop_staging(self):
        handles, self._handles = getattr(self, "_handles", []), []
        for handle in handles:
            try:
                _lib.lib().tbk_kdotp_destroy(handle)
            except Exception:  # pylint: disable=broad-except
                pass
        self._staged_key = None

    def pin_staging(self, pinned=True):
        """Skip the per-call content check of ``taylor_coefficients`` (the caller promises not to edit them)."""
        self._pinned = bool(pinned)

    def _staging_key(self):
        """What the staged copy is valid for: device, the power tuples in order, and the coefficient bytes.
        ``taylor_coefficients`` is a public, mutable dict that the reference reads on every call
        (``kdotp.py:51-82``), so the content is re-validated per call like ``Model``'s hoppings."""
        try:
            import xxhash  # pylint: disable=import-outside-toplevel

            running = xxhash.xxh3_64()
            update = running.update
            digest = running.intdigest
        except ImportError:  # pragma: no cover
            import hashlib  # pylint: disable=import-outside-toplevel

            running = hashlib.blake2b(digest_size=8)
            update = running.update
            digest = running.digest
        keys = []
        for key, mat in self.taylor_coefficients.items():
            keys.append(tuple(key))
            arr = np.ascontiguousarray(mat, dtype=np.complex128)
            keys.append(arr.shape)
            update(arr.view(np.uint8).reshape(-1).data)
        return (tuple(self._devices), tuple(keys), digest())

    def _shape(self):
        if not self.taylor_coefficients:
            raise ValueError("empty k.p model")
        key, mat = next(iter(self.taylor_coefficients.items()))
        return len(key), mat.shape[0]

    def _staged(self):
        """The ``tbk_kdotp*`` on the first device (re-staged when the coefficients changed)."""
        with self._call_lock:
            return self._staged_locked()[0]

    def _staged_locked(self):
        """One ``tbk_kdotp*`` per entry of ``self.devices``."""
        key = None
        if self._handles and not self._pinned:
            key = self._staging_key()
            if key != self._staged_key:
                self._drop_staging()
        if not self._handles:
            key = key if key is not None else self._staging_key()
            dim, size = self._shape()
            keys = list(self.taylor_coefficients.keys())
            powers = np.array(keys, dtype=np.int32).reshape(len(keys), dim)
            coeffs = np.ascontiguousarray(np.stack([self.taylor_coefficients[k] for k in keys]), dtype=np.complex128)
            handles = []
            try:
                for device in self._devices:  # the coefficients are replicated: every device holds the whole model
                    handle = ctypes.c_void_p()
                    _lib.check(
                        _lib.lib().tbk_kdotp_create(
                            device, dim, size, len(keys), _lib.ptr(powers), _lib.ptr(coeffs), ctypes.byref(handle)
                        )
                    )
                    handles.append(handle)
            except Exception:
                for handle in handles:
                    _lib.lib().tbk_kdotp_destroy(handle)
                raise
            self._handles = handles
            self._staged_key = key
        return self._handles

    def _handle_array(self):
        handles = self._staged_locked()
        return (ctypes.c_void_p * len(handles))(*[h.value for h in handles]), len(handles)

    def _k_array(self, k):
        dim, _ = self._shape()
        k_array = np.asarray(k)  # np.array(k, ndmin=1) without its copy: k is only read
        if k_array.ndim == 0:
            k_array = k_array.reshape(1)
        single = k_array.ndim == 1
        if single:
            k_array = k_array.reshape((1, -1))
        k_array = np.ascontiguousarray(k_array, dtype=np.float64)
        if k_array.ndim != 2 or k_array.shape[1] != dim:
            raise ValueError("operands could not be broadcast together: k has shape {}".format(k_array.shape))
        return k_array, single

    def hamilton(self, k):
        """H(k) at one k-point or a list of k-points (``kdotp.py:51-82``)."""
        k_array, single = self._k_array(k)
        _, size = self._shape()
        out = _outbuf.empty((k_array.shape[0], size, size), np.complex128)
        with self._call_lock:  # re-validating the staged copy and the call are one step for other threads
            handles, n_handles = self._handle_array()
            _lib.check(_lib.lib().tbk_kdotp_hamilton_multi(handles, n_handles, _lib.ptr(k_array), k_array.shape[0], _lib.ptr(out)))
        return out[0] if single else out

    def eigenval(self, k):
        """Eigenvalues at one k-point or a list of k-points (``kdotp.py:84-100``)."""
        out = self.eigenval_array(k)
        return out if out.ndim == 1 else list(out)

    def eigenval_array(self, k):
        """``eigenval`` as one ``(NK, N)`` array instead of a list of rows (see ``Model.eigenval_array``)."""
        k_array, single = self._k_array(k)
        _, size = self._shape()
        out = _outbuf.empty((k_array.shape[0], size), np.float64)
        with self._call_lock:
            handles, n_handles = self._handle_array()
            _lib.check(_lib.lib().tbk_kdotp_eigenval_multi(handles, n_handles, _lib.ptr(k_array), k_array.shape[0], _lib.ptr(out)))
        return out[0] if single else out

    def eigh(self, k):
        """Eigenvalues and eigenvectors at one k-point or a list of k-points: ``(E, U)`` as in ``Model.eigh``."""
        dim, size = self._shape()
        if np.shape(k) == (0,):  # an empty list of k-points
            k = np.zeros((0, dim))
        k_array, single = self._k_array(k)
        eig = _outbuf.empty((k_array.shape[0], size), np.float64)
        vec = _outbuf.empty((k_array.shape[0], size, size), np.complex128)
        with self._call_lock:
            handles, n_handles = self._handle_array()
            _lib.check(_lib.lib().tbk_kdotp_eigh_multi(handles, n_handles, _lib.ptr(k_array), k_array.shape[0], _lib.ptr(eig),
                                                       _lib.ptr(vec)))
        return (eig[0], vec[0]) if single else (eig, vec)

    # ------------------------------------------------------------------ HDF5 (``tbmodels.kdotp_model``)
    def to_hdf5(self):
        """
        The tree ``hdf5_lite.write`` stores for the reference's ``SimpleHDF5Mapping`` serialisation of this class
        (``kdotp.py:19-36``: one attribute, ``taylor_coefficients``, a dict with tuple keys).  ``fsc.hdf5_io`` (not
        installed here, and the reference ships no such file) writes a mapping as ``builtins.dict`` with ONE group
        ``items`` = ``list(obj.items())``, i.e. a ``builtins.list`` of ``builtins.tuple(key, value)`` pairs, and reads
        that (or, for legacy files, a ``value`` group of string keys) back: a ``keys`` + ``values`` pair of lists --
        what this method wrote until round 3 -- does not load there.  ``from_hdf5`` still reads both.
        """
        def number(x):
            return {"type_tag": "builtins.number", "value": np.int64(x)}

        def sequence(tag, items):
            tree = {"type_tag": tag}
            tree.update({str(i): item for i, item in enumerate(items)})
            return tree

        pairs = [
            sequence("builtins.tuple", [
                sequence("builtins.tuple", [number(x) for x in key]),
                {"type_tag": "numpy.ndarray", "value": np.asarray(mat, dtype=complex)},
            ])
            for key, mat in self.taylor_coefficients.items()
        ]
        return {
            "type_tag": "tbmodels.kdotp_model",
            "taylor_coefficients": {"type_tag": "builtins.dict", "items": sequence("builtins.list", pairs)},
        }

    @classmethod
    def from_hdf5(cls, tree):
        """Inverse of :meth:`to_hdf5` (``items``: a list of pairs); also accepts the ``keys`` + ``values`` lists that
        earlier versions of this package wrote."""
        def plain(node):
            if isinstance(node, dict):
                tag = node.get("type_tag")
                if isinstance(tag, bytes):
                    tag = tag.decode()
                if tag in ("builtins.list", "builtins.tuple"):
                    items = [plain(node[name]) for name in sorted((n for n in node if n != "type_tag"), key=int)]
                    return tuple(items) if tag == "builtins.tuple" else items
                if "value" in node:
                    return node["value"]
            return node

        coeff = tree["taylor_coefficients"]
        if "items" in coeff:
            pairs = plain(coeff["items"])
        else:
            pairs = zip(plain(coeff["keys"]), plain(coeff["values"]))
        return cls({tuple(int(x) for x in key): np.array(mat) for key, mat in pairs})
