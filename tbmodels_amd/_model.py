"""
``Model`` -- the host-side mirror of ``tbmodels.Model`` for the k-space evaluation path.

The reference has no plugin boundary: the hot path is two bound methods,
``Model.hamilton(k, convention=2)`` (``/root/reference/src/tbmodels/_tb_model.py:1076-1132``) and
``Model.eigenval(k)`` (``:1134-1150``), reading ``self.hop``, ``self.size``, ``self.dim``,
``self.pos`` and ``self._sparse``.  This class keeps that surface -- same constructor keywords, same
``hop`` storage convention (half-space lattice vectors, ``R = 0`` block halved; ``:175-218``,
``:247-298``), same ``add_hop`` / ``add_on_site`` / ``set_sparse`` mutators, same argument and return
conventions, same exceptions -- and evaluates both methods on the GPU through ``libtbk.so``
(``include/tbk.h``).  Nothing here computes H(k) on the CPU; without the library and a device the
two methods raise.

Device state is a cache of ``self.hop``: it is re-validated against a content fingerprint on every
call (``add_hop``, ``model.hop[R] += ...`` and ``set_sparse`` all mutate in place), dropped on pickling
and rebuilt lazily.
"""

import collections as co
import ctypes
import os
import threading
import warnings
import zlib

import numpy as np

from . import _lib, _outbuf
from ._sparse_matrix import csr as _csr

try:  # fast content hash for the staging fingerprint; zlib is the fallback
    import xxhash as _xxhash
except ImportError:  # pragma: no cover
    _xxhash = None

__all__ = ("Model", "DensityOfStates", "ProjectedDensityOfStates", "BandEdges", "FermiLevel", "Occupations")

#: what ``Model.dos`` returns: the energy grid (NE,), the number of states at its points (NE,), their difference quotient (NE - 1,)
DensityOfStates = co.namedtuple("DensityOfStates", ("energies", "nos", "dos"))
ProjectedDensityOfStates = co.namedtuple("ProjectedDensityOfStates", ("energies", "nos", "dos"))
#: what ``Model.band_edges`` returns: per band the minimum and the maximum over the mesh, (size,) each
BandEdges = co.namedtuple("BandEdges", ("emin", "emax"))
#: what ``Model.fermi_level`` returns: floats; ``lower < upper`` exactly when the mesh has a gap at the filling asked for
FermiLevel = co.namedtuple("FermiLevel", ("mu", "lower", "upper", "nos"))
Occupations = co.namedtuple("Occupations", ("mu", "orbital_occ", "band_occ", "band_energy"))
DensityMatrix = co.namedtuple("DensityMatrix", ("mu", "R", "rho"))
GreenFunction = co.namedtuple("GreenFunction", ("z", "R", "G"))
SurfaceGreenFunction = co.namedtuple("SurfaceGreenFunction", ("k", "z", "layers", "iterations", "bottom", "top", "bulk"))
Transmission = co.namedtuple("Transmission", ("k", "z", "layers", "length", "iterations", "transmission"))
TransmissionGreen = co.namedtuple("TransmissionGreen", Transmission._fields + ("green",))
TransmissionEnsemble = co.namedtuple("TransmissionEnsemble", ("k", "z", "layers", "length", "samples", "iterations", "transmission"))
TransmissionChannels = co.namedtuple("TransmissionChannels", ("k", "z", "layers", "length", "samples", "iterations", "transmission", "channels", "noise"))
DeviceGreen = co.namedtuple("DeviceGreen", Transmission._fields + ("ldos", "left", "right"))
DeviceGreenBlocks = co.namedtuple("DeviceGreenBlocks", DeviceGreen._fields + ("diagonal", "first", "last"))
DeviceCurrent = co.namedtuple("DeviceCurrent", DeviceGreen._fields + ("current_left", "current_right"))
DeviceCurrentBonds = co.namedtuple("DeviceCurrentBonds", DeviceCurrent._fields + ("inter_left", "inter_right", "intra_left", "intra_right"))
Susceptibility = co.namedtuple("Susceptibility", ("mu", "q", "chi"))
DynamicSusceptibility = co.namedtuple("DynamicSusceptibility", ("mu", "q", "omega", "chi"))
OrbitalSusceptibility = co.namedtuple("OrbitalSusceptibility", ("mu", "q", "orbitals", "chi"))
DynamicOrbitalSusceptibility = co.namedtuple("DynamicOrbitalSusceptibility", ("mu", "q", "omega", "orbitals", "chi"))
SusceptibilityTensor = co.namedtuple("SusceptibilityTensor", ("mu", "q", "orbitals", "chi"))
BerryFlux = co.namedtuple("BerryFlux", ("bands", "planes", "flux", "chern", "link_min"))
OpticalConductivity = co.namedtuple("OpticalConductivity", ("mu", "omega", "sigma"))
#: what ``Model.transport_distribution`` returns: the grid (NE,), int^E Sigma (dim, dim, NE) and Sigma at the bin midpoints (dim, dim, NE - 1)
TransportDistribution = co.namedtuple("TransportDistribution", ("energies", "cumulative", "tdf"))


def _devices_from_env():
    """``TBK_DEVICES=0,1,...`` (several GPUs behind one model), else ``TBK_DEVICE=i``, else device 0."""
    listed = os.environ.get("TBK_DEVICES", "").strip()
    if listed:
        return [int(part) for part in listed.replace(";", ",").split(",") if part.strip() != ""]
    return [int(os.environ.get("TBK_DEVICE", "0"))]


def _first_nonzero(vec):
    for x in vec:
        if x != 0:
            return x
    return 0


def _hash_bytes(running, array):
    data = np.ascontiguousarray(array)
    if _xxhash is not None:
        running.update(data.view(np.uint8).reshape(-1).data)
        return running
    return zlib.adler32(data.view(np.uint8).reshape(-1).data, running)


class _HopDict(co.defaultdict):
    """
    ``Model.hop``: a ``defaultdict`` (as in the reference, ``_tb_model.py:206``) that remembers whether a
    matrix may have been handed to outside code.

    The staged device copy has to follow in-place edits such as ``model.hop[R] += x``.  Hashing the hopping
    bytes on every call finds them but costs a pass over the model (1.3 ms for 512 matrices of 64 x 64) --
    more than a single-k ``hamilton`` call.  So: the model's own mutators (``add_hop``, ``add_on_site``,
    ``set_sparse``) go through the raw ``dict`` methods and bump ``version``; ANY outside access that can
    reach a matrix (``[]``, ``get``, ``values``, ``items``, ``pop``, ``update`` ...) sets ``exposed`` for good
    -- a reference handed out once can be written through at any later time -- and ``Model._staged`` falls
    back to the content hash from then on.  Untouched models (from files, from arrays) pay nothing.
    """

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.exposed = False
        self.version = 0

    def __reduce__(self):
        # pickle: the items are set through __setitem__ (which marks the new dict exposed) and the state is applied
        # AFTER them -- nobody holds references into a freshly unpickled dict, so it starts clean.  Iterating with
        # dict.items keeps pickling from marking the SOURCE exposed.
        return (type(self), (self.default_factory,), {"exposed": False, "version": 0}, None, iter(dict.items(self)))

    def __copy__(self):  # copy.copy(model.hop): the copy shares every matrix with the source
        self.exposed = True
        new = type(self)(self.default_factory)
        dict.update(new, self)
        new.exposed = True
        return new

    def __deepcopy__(self, memo):  # private copies of the matrices: a clean dict
        import copy as _copy  # pylint: disable=import-outside-toplevel

        new = type(self)(self.default_factory)
        for key, value in dict.items(self):
            dict.__setitem__(new, key, _copy.deepcopy(value, memo))
        return new

    def __iter__(self):
        # overriding __iter__ takes dict(hop), {**hop} and dict.update(other, hop) off CPython's exact-dict fast path:
        # they then go through keys() + __getitem__, which marks the exposure
        return dict.__iter__(self)

    def __or__(self, other):  # hop | {...}: the result holds the same matrix objects
        self.exposed = True
        return co.defaultdict.__or__(self, other)

    def __ror__(self, other):
        self.exposed = True
        return co.defaultdict.__ror__(self, other)

    def __ior__(self, other):  # hop |= {...}: contents change behind the edit counter
        self.exposed = True
        dict.update(self, other)
        return self

    def __getitem__(self, key):
        self.exposed = True
        return super().__getitem__(key)

    def __setitem__(self, key, value):
        self.exposed = True
        super().__setitem__(key, value)

    def __delitem__(self, key):
        self.exposed = True
        super().__delitem__(key)

    def _exposing(name):  # pylint: disable=no-self-argument
        def method(self, *args, **kwargs):
            self.exposed = True
            return getattr(co.defaultdict, name)(self, *args, **kwargs)

        method.__name__ = name
        return method

    get = _exposing("get")
    values = _exposing("values")
    items = _exposing("items")
    pop = _exposing("pop")
    popitem = _exposing("popitem")
    setdefault = _exposing("setdefault")
    update = _exposing("update")
    clear = _exposing("clear")
    copy = _exposing("copy")
    del _exposing

    # --- the model's own access: raw dict methods, edits counted in `version` ---
    def raw_items(self):
        return dict.items(self)

    def raw_values(self):
        return dict.values(self)

    def raw_get(self, key):
        """``self[key]`` with the defaultdict insertion on a miss, without marking the dict exposed."""
        if dict.__contains__(self, key):
            return dict.__getitem__(self, key)
        value = self.default_factory()
        dict.__setitem__(self, key, value)
        self.version += 1
        return value

    def raw_set(self, key, value):
        dict.__setitem__(self, key, value)
        self.version += 1


class Model:
    """
    Tight-binding model with GPU evaluation of ``hamilton`` / ``eigenval``.

    Keyword arguments are those of ``tbmodels.Model`` (``_tb_model.py:89-102``): ``on_site``,
    ``hop`` (dict ``R -> (size, size)`` matrix), ``size``, ``dim``, ``occ``, ``pos``, ``uc``,
    ``contains_cc``, ``cc_check_tolerance``, ``sparse``.
    """

    def __init__(
        self,
        *,
        on_site=None,
        hop=None,
        size=None,
        dim=None,
        occ=None,
        pos=None,
        uc=None,
        contains_cc=True,
        cc_check_tolerance=1e-12,
        sparse=False,
    ):
        hop = {} if hop is None else hop
        self._handles = []
        self._staged_fingerprint = None
        self._pinned = False
        self._call_lock = threading.RLock()
        self.devices = _devices_from_env()

        self.set_sparse(sparse)

        # size and dimension are inferred in the reference's order of precedence (:135-172)
        if size is not None:
            self.size = size
        elif on_site is not None:
            self.size = len(on_site)
        elif pos is not None:
            self.size = len(pos)
        elif hop:
            self.size = next(iter(hop.values())).shape[0]
        else:
            raise ValueError(
                "Empty hoppings dictionary supplied and no size, on-site energies or positions given. "
                "Cannot determine the size of the system."
            )
        if dim is not None:
            self.dim = dim
        elif pos is not None:
            self.dim = len(pos[0])
        elif hop:
            self.dim = len(next(iter(hop.keys())))
        elif uc is not None:
            self.dim = len(uc[0])
        else:
            raise ValueError(
                "No dimension specified and no positions, hoppings, or unit cell are given. "
                "The dimensionality of the system cannot be determined."
            )
        self._zero_vec = tuple([0] * self.dim)
        self.uc = None if uc is None else np.array(uc)

        blocks = {tuple(int(x) for x in key): self._as_dense(value) for key, value in hop.items()}

        if pos is None:
            self.pos = np.zeros((self.size, self.dim))
        else:
            if len(pos) != self.size:
                raise ValueError(
                    "Invalid argument for 'pos': The number of positions must be the same as the size "
                    "(number of orbitals) of the system."
                )
            if any(len(p) != self.dim for p in pos):
                raise ValueError(
                    "Invalid argument for 'pos': The length of each position must be the same as the "
                    "dimensionality of the system."
                )
            pos_arr, blocks = self._fold_into_home_cell(np.array(pos, dtype=float), blocks)
            self.pos = pos_arr

        if contains_cc:
            blocks = self._halve_conjugate_pairs(blocks, cc_check_tolerance)
        else:
            blocks = self._fold_to_half_space(blocks)

        self.hop = _HopDict(self._empty_matrix)
        for key, mat in blocks.items():
            if np.any(mat):
                self.hop.raw_set(key, self._matrix_type(mat))
        if on_site is not None:
            if len(on_site) != self.size:
                raise ValueError(
                    "The number of on-site energies {} does not match the size of the system {}".format(
                        len(on_site), self.size
                    )
                )
            self._hop_add(self._zero_vec, 0.5 * self._matrix_type(np.diag(np.array(on_site, dtype=complex))))

        for mat in self._hop_values():
            if mat.shape != (self.size, self.size):
                raise ValueError(
                    "Hopping matrix of shape {0} found, should be ({1},{1}).".format(mat.shape, self.size)
                )
        for key in self.hop.keys():
            if len(key) != self.dim:
                raise ValueError(
                    "The length of R = {} does not match the dimensionality of the system ({})".format(key, self.dim)
                )
        if self.uc is not None and self.uc.shape != (self.dim, self.dim):
            raise ValueError(
                "Inconsistend dimension of the unit cell: {}, does not match the dimensionality of the "
                "system ({})".format(self.uc.shape, self.dim)
            )
        self.occ = None if occ is None else int(occ)

    # ------------------------------------------------------------------ construction helpers
    @staticmethod
    def _as_dense(value):
        if hasattr(value, "toarray"):
            return np.asarray(value.toarray(), dtype=complex)
        return np.array(value, dtype=complex)

    def _fold_into_home_cell(self, pos, blocks):
        """
        Orbitals outside ``[0, 1)^dim`` are moved into the home cell and every hopping that touches
        them is re-labelled ``R -> R + shift[col] - shift[row]`` (``_tb_model.py:221-245``).
        """
        shift = np.floor(pos).astype(int)
        if not shift.any():
            return pos, blocks
        moved = co.defaultdict(lambda: np.zeros((self.size, self.size), dtype=complex))
        for key, mat in blocks.items():
            rows, cols = np.nonzero(mat)
            for i, j in zip(rows, cols):
                new_key = tuple(int(x) for x in (np.array(key, dtype=int) + shift[j] - shift[i]))
                moved[new_key][i, j] += mat[i, j]
        return pos % 1, dict(moved)

    @staticmethod
    def _halve_conjugate_pairs(blocks, tolerance):
        """
        ``contains_cc=True`` input lists both ``R`` and ``-R``: check ``hop[-R] == hop[R]^H``, keep the
        average on the half-space and HALF of it at ``R = 0`` (``_tb_model.py:247-279``).
        """
        kept = {}
        bad = []
        for key, mat in blocks.items():
            minus = tuple(-x for x in key)
            partner = blocks[minus].conj().T if minus in blocks else np.zeros_like(mat)
            delta = np.linalg.norm(mat - partner)
            if delta > tolerance:
                bad.append((key, delta))
            mean = (mat + partner) / 2
            lead = _first_nonzero(key)
            if lead > 0:
                kept[key] = mean
            elif lead == 0:
                kept[key] = mean / 2
        if bad:
            bad.sort(key=lambda item: -item[1])
            raise ValueError(
                "The provided hoppings do not correspond to a hermitian Hamiltonian. "
                "hoppings[-R] = hoppings[R].H is not fulfilled for the following values:\n"
                + "\n".join("R={}, delta_norm={}".format(key, delta) for key, delta in bad)
            )
        return kept

    def _fold_to_half_space(self, blocks):
        """``contains_cc=False``: a block at ``-R`` is stored as its conjugate transpose at ``+R`` (:281-298)."""
        folded = {}

        def accumulate(key, mat):
            folded[key] = folded[key] + mat if key in folded else mat.copy()

        for key, mat in blocks.items():
            lead = _first_nonzero(key)
            if lead > 0:
                accumulate(key, mat)
            elif lead < 0:
                accumulate(tuple(-x for x in key), mat.conj().T)
            else:
                accumulate(key, 0.5 * mat + 0.5 * mat.conj().T)
        return folded

    @classmethod
    def from_hop_list(cls, *, hop_list=(), size=None, **kwargs):
        """
        Build a model from ``(t, orbital_1, orbital_2, R)`` terms (``_tb_model.py:332-397``); repeated
        ``(orbital_1, orbital_2, R)`` entries add up.
        """
        if size is None:
            if "on_site" not in kwargs:
                raise ValueError(
                    "No on-site energies and no size given. The size of the system cannot be determined."
                )
            size = len(kwargs["on_site"])
        blocks = {}
        for amplitude, i, j, r_vec in hop_list:
            key = tuple(int(x) for x in r_vec)
            if key not in blocks:
                blocks[key] = np.zeros((size, size), dtype=complex)
            blocks[key][i, j] += amplitude
        return cls(size=size, hop=blocks, **kwargs)

    @classmethod
    def from_packed(cls, r_vec, hop, pos=None, **kwargs):
        """
        Build a model from packed half-space arrays ``R (n_r, dim)`` / ``hop (n_r, N, N)`` (the layout of
        the golden fixtures and of ``tbmodels_amd.synthetic``); equivalent to
        ``Model(hop={R: mat}, contains_cc=False, ...)``.
        """
        r_vec = np.asarray(r_vec)
        hop = np.asarray(hop)
        kwargs.setdefault("dim", r_vec.shape[1] if r_vec.ndim == 2 else None)
        if hop.ndim == 3 and hop.shape[0]:
            kwargs.setdefault("size", hop.shape[1])
        blocks = {tuple(int(x) for x in r): h for r, h in zip(r_vec, hop)}
        return cls(hop=blocks, pos=pos, contains_cc=False, **kwargs)

    @classmethod
    def from_wannier_files(
        cls,
        *,
        hr_file,
        wsvec_file=None,
        xyz_file=None,
        win_file=None,
        h_cutoff=0.0,
        ignore_orbital_order=False,
        pos_kind="wannier",
        distance_ratio_threshold=3.0,
        **kwargs,
    ):
        """
        Build a model from Wannier90 output (``*_hr.dat`` and optionally ``*_wsvec.dat``, ``*_centres.xyz``,
        ``*.win``): same keywords and results as ``tbmodels.Model.from_wannier_files``
        (``_tb_model.py:565-715``); the files are parsed array-wise by :mod:`tbmodels_amd.wannier`.
        """
        from . import wannier  # pylint: disable=import-outside-toplevel

        if win_file is not None:
            if "uc" in kwargs:
                raise ValueError(
                    "Ambiguous unit cell: It can be given either via 'uc' or the 'win_file' keywords, but not both."
                )
            kwargs["uc"] = wannier.read_win(win_file)["unit_cell_cart"]
        if xyz_file is not None:
            if "pos" in kwargs:
                raise ValueError(
                    "Ambiguous orbital positions: The positions can be given either via the 'pos' or the "
                    "'xyz_file' keywords, but not both."
                )
            if "uc" not in kwargs:
                raise ValueError(
                    "Positions cannot be read from .xyz file without unit cell given: Transformation from "
                    "cartesian to reduced coordinates not possible. Specify the unit cell using one of the "
                    "keywords 'uc' or 'win_file'."
                )
            kwargs["pos"] = wannier.positions_from_xyz(
                xyz_file, kwargs["uc"], pos_kind=pos_kind, distance_ratio_threshold=distance_ratio_threshold
            )
        num_wann, blocks = wannier.hop_blocks_from_wannier(
            hr_file, wsvec_file=wsvec_file, h_cutoff=h_cutoff, ignore_orbital_order=ignore_orbital_order
        )
        return cls(size=num_wann, hop=blocks, **kwargs)

    # ------------------------------------------------------------------ mutators (reference API)
    def add_hop(self, overlap, orbital_1, orbital_2, R):
        """
        Add ``<orbital_1, 0| H |orbital_2, R> = overlap``; the conjugate term is implied
        (``_tb_model.py:1153-1215``): a negative-half-space ``R`` is stored conjugated at ``-R`` and an
        ``R = 0`` term is split symmetrically.
        """
        R = tuple(R)
        if len(R) != self.dim:
            raise ValueError(
                "Dimension of R ({}) does not match the model dimension ({})".format(len(R), self.dim)
            )
        overlap = complex(overlap)
        mat = np.zeros((self.size, self.size), dtype=complex)
        lead = _first_nonzero(R)
        if lead == 0:
            mat[orbital_1, orbital_2] += overlap / 2.0
            mat[orbital_2, orbital_1] += overlap.conjugate() / 2.0
        elif lead > 0:
            mat[orbital_1, orbital_2] += overlap
        else:
            R = tuple(-x for x in R)
            mat[orbital_2, orbital_1] += overlap.conjugate()
        self._hop_add(R, self._matrix_type(mat))

    def add_on_site(self, on_site):
        """Add to the on-site energies (``_tb_model.py:1217-1234``)."""
        if self.size != len(on_site):
            raise ValueError(
                "The number of on-site energy terms should be {}, but is {}.".format(self.size, len(on_site))
            )
        for orbital, energy in enumerate(on_site):
            self.add_hop(energy / 2.0, orbital, orbital, self._zero_vec)

    def _empty_matrix(self):
        return self._matrix_type(np.zeros((self.size, self.size), dtype=complex))

    # ``self.hop`` as the model itself reads and edits it (see ``_HopDict``); a plain dict assigned by the
    # caller (``model.hop = {...}``) works too and is simply always content-hashed.
    def _hop_items(self):
        hop = self.hop
        return hop.raw_items() if isinstance(hop, _HopDict) else hop.items()

    def _hop_values(self):
        hop = self.hop
        return hop.raw_values() if isinstance(hop, _HopDict) else hop.values()

    def _hop_set(self, key, value):
        hop = self.hop
        if isinstance(hop, _HopDict):
            hop.raw_set(key, value)
        else:
            hop[key] = value

    def _hop_add(self, key, mat):
        hop = self.hop
        if isinstance(hop, _HopDict):
            hop.raw_set(key, hop.raw_get(key) + mat)
        else:
            hop[key] = hop[key] + mat if key in hop else self._empty_matrix() + mat

    def set_sparse(self, sparse=True):
        """Switch the storage of ``hop`` between dense arrays and CSR (``_tb_model.py:1294-1321``)."""
        if getattr(self, "_sparse", None) == sparse:
            return
        self._sparse = sparse
        self._matrix_type = _csr if sparse else np.array
        if hasattr(self, "hop"):
            for key, mat in list(self._hop_items()):
                self._hop_set(key, self._matrix_type(self._as_dense(mat) if sparse else np.array(mat)))

    def _array_cast(self, mat):
        return np.array(mat) if self._sparse else mat

    # ------------------------------------------------------------------ pickling
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_handles"] = []
        state["_staged_fingerprint"] = None
        state.pop("_call_lock", None)
        state.pop("_handle_array_cache", None)  # (a ctypes array of device handles: neither picklable nor valid elsewhere)
        return state

    def __setstate__(self, state):
        # (the hop dict's exposure flag / edit counter are NOT touched here: copy.copy(model) shares the dict with
        # the original, whose handed-out references stay live; a pickled dict resets itself in _HopDict.__reduce__)
        state = dict(state)
        state.pop("_handle", None)  # states written before a model could sit on several devices
        legacy_device = state.pop("device", None)
        self.__dict__.update(state)
        self._handles = []
        if "_devices" not in state:
            self._devices = [int(legacy_device)] if legacy_device is not None else _devices_from_env()
        self._call_lock = threading.RLock()

    def __del__(self):
        self._drop_staging()

    # ------------------------------------------------------------------ staging
    @property
    def device(self):
        """The (first) GPU this model evaluates on; assigning an index makes it the only one."""
        return self.devices[0]

    @device.setter
    def device(self, index):
        self.devices = [int(index)]

    @property
    def devices(self):
        """
        GPU indices this model is staged on.  With more than one, ``hamilton`` / ``eigenval`` cut the k list into
        contiguous slabs, one per entry, and every device fills its rows of the result (``tbk_eigenval_multi``): the
        same single call of a single process as in the reference (``_tb_model.py:1134-1150``), no launcher.  Default:
        ``TBK_DEVICES=0,1,...`` (or ``TBK_DEVICE=i``, or device 0).  An index may repeat (several staged copies on one GPU).
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
                _lib.lib().tbk_model_destroy(handle)
            except Exception:  # pylint: disable=broad-except  # interpreter shutdown
                pass
        self._staged_fingerprint = None

    def pin_staging(self, pinned=True):
        """
        Skip the per-call content check of ``self.hop`` (it costs one pass over the hopping bytes).
        The caller promises not to mutate the model while pinned.
        """
        self._pinned = bool(pinned)

    def _staging_key(self):
        """What the staged copy is valid for: the edit counter while no matrix has left the model (exact, and
        no pass over the bytes), the content fingerprint afterwards."""
        hop = self.hop
        if isinstance(hop, _HopDict) and not hop.exposed:
            return ("version", hop.version, tuple(self._devices), self.size, self.dim, bool(self._sparse))
        return self._fingerprint()

    def _fingerprint(self):
        running = _xxhash.xxh3_64() if _xxhash is not None else 1
        meta = [*self._devices, -1, self.size, self.dim, int(self._sparse), len(self.hop)]
        for key, mat in self._hop_items():
            meta.extend(key)
            if self._sparse:
                running = _hash_bytes(running, mat.indptr)
                running = _hash_bytes(running, mat.indices)
                running = _hash_bytes(running, mat.data)
            else:
                running = _hash_bytes(running, mat)
        digest = running.intdigest() if _xxhash is not None else running
        return (tuple(meta), digest)

    def packed_hop(self):
        """
        ``self.hop`` as the arrays the C ABI takes: ``R int32 (n_r, dim)`` plus either
        ``hop complex128 (n_r, N, N)`` (dense) or ``(r_ptr int64, row int32, col int32, val complex128)``.
        """
        stored = list(self._hop_items())
        keys = [key for key, _ in stored]
        r_vec = np.array(keys, dtype=np.int32).reshape(len(keys), self.dim)
        if not self._sparse:
            hop = np.empty((len(keys), self.size, self.size), dtype=np.complex128)
            for idx, (_, mat) in enumerate(stored):
                hop[idx] = mat
            return r_vec, hop
        r_ptr = [0]
        rows, cols, vals = [], [], []
        for _, mat in stored:
            coo = mat.tocoo()
            rows.append(coo.row.astype(np.int32))
            cols.append(coo.col.astype(np.int32))
            vals.append(coo.data.astype(np.complex128))
            r_ptr.append(r_ptr[-1] + coo.nnz)
        cat = lambda parts, dtype: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, dtype), dtype)
        return r_vec, (np.array(r_ptr, dtype=np.int64), cat(rows, np.int32), cat(cols, np.int32), cat(vals, np.complex128))

    def _staged(self):
        """The ``tbk_model*`` on the first device for the current contents of ``self.hop`` (re-staged when they changed)."""
        return self._staged_all()[0]

    def _staged_all(self):
        """One ``tbk_model*`` per entry of ``self.devices`` for the current contents of ``self.hop``."""
        if self._handles and self._pinned:
            return self._handles
        fingerprint = self._staging_key()
        if self._handles and fingerprint == self._staged_fingerprint:
            return self._handles
        self._drop_staging()
        lib = _lib.lib()
        r_vec, payload = self.packed_hop()
        handles = []
        try:
            for device in self._devices:  # the hoppings are replicated: every device holds the whole model
                handle = ctypes.c_void_p()
                if self._sparse:
                    r_ptr, row, col, val = payload
                    status = lib.tbk_model_create_csr(
                        device, self.dim, self.size, len(r_vec), _lib.ptr(r_vec), _lib.ptr(r_ptr), _lib.ptr(row),
                        _lib.ptr(col), _lib.ptr(val), ctypes.byref(handle),
                    )
                else:
                    status = lib.tbk_model_create_dense(
                        device, self.dim, self.size, len(r_vec), _lib.ptr(r_vec), _lib.ptr(payload), ctypes.byref(handle)
                    )
                _lib.check(status)
                handles.append(handle)
        except Exception:
            for handle in handles:
                lib.tbk_model_destroy(handle)
            raise
        self._handles = handles
        self._staged_fingerprint = fingerprint
        return handles

    def _handle_array(self):
        handles = self._staged_all()
        cached = getattr(self, "_handle_array_cache", None)
        if cached is None or cached[0] is not handles:  # (the list object changes whenever the model is re-staged)
            cached = (handles, (ctypes.c_void_p * len(handles))(*[h.value for h in handles]))
            self._handle_array_cache = cached
        return cached[1], len(handles)

    def set_option(self, option, value):
        """Forward a ``TBK_OPT_*`` option to the staged model (see ``include/tbk.h``)."""
        with self._call_lock:
            for handle in self._staged_all():
                _lib.check(_lib.lib().tbk_model_set_option(handle, option, int(value)))

    # ------------------------------------------------------------------ the hot path
    def _k_array(self, k):
        """``np.array(k, ndmin=1)``; 1-D (or scalar) means one k-point (``_tb_model.py:1103-1108``)."""
        k_array = np.asarray(k)  # np.array(k, ndmin=1) without its copy: k is only read
        if k_array.ndim == 0:
            k_array = k_array.reshape(1)
        single = k_array.ndim == 1
        if single:
            k_array = k_array.reshape((1, -1))
        k_array = np.ascontiguousarray(k_array, dtype=np.float64)
        if k_array.ndim != 2 or k_array.shape[1] != self.dim:
            # the reference fails inside np.dot(k_array, R) with a shape ValueError
            raise ValueError(
                "shapes {} and ({},) not aligned: k-point dimension does not match the model".format(
                    k_array.shape, self.dim
                )
            )
        return k_array, single

    def hamilton(self, k, convention=2):
        """
        The Hamilton matrix at one k-point (returns ``(size, size)``) or a list of k-points
        (``(NK, size, size)``), complex128; ``convention`` 1 or 2 as in PythTB
        (``_tb_model.py:1076-1132``).
        """
        if convention not in [1, 2]:
            raise ValueError(
                "Invalid value '{}' for 'convention': must be either '1' or '2'".format(convention)
            )
        k_array, single = self._k_array(k)
        n_k = k_array.shape[0]
        out = _outbuf.empty((n_k, self.size, self.size), np.complex128)
        pos = np.ascontiguousarray(self.pos, dtype=np.float64) if convention == 1 else None
        with self._call_lock:  # (re)staging and the call are one step for other threads (ctypes drops the GIL)
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_hamilton_multi(handles, n_handles, _lib.ptr(k_array), n_k, int(convention), _lib.ptr(pos),
                                              _lib.ptr(out))
            )
        return out[0] if single else out

    def eigenval(self, k):
        """
        Ascending eigenvalues at one k-point (1-D array) or a list of k-points (a list of 1-D arrays,
        like the reference: ``_tb_model.py:1134-1150``).
        """
        out = self.eigenval_array(k)
        return out if out.ndim == 1 else list(out)

    def eigenval_array(self, k):
        """
        ``eigenval`` without the list: one ``(NK, N)`` array for a list of k-points (``(N,)`` for one k-point).  Not in
        the reference; building the list of row views costs ~80 ns per k-point, more than the GPU work for small
        models (500 000 k-points of an 8-orbital model: 4.6 ms of kernels, 40 ms of ``list(out)``).
        """
        k_array, single = self._k_array(k)
        n_k = k_array.shape[0]
        out = _outbuf.empty((n_k, self.size), np.float64)
        with self._call_lock:
            # NaN / Inf in k or in the hoppings reach the eigenvalues; the library checks those on the device and
            # returns TBK_ERR_NOT_FINITE -> ValueError, scipy.linalg.eigvalsh(check_finite=True)'s answer to the
            # non-finite Hamiltonian (two np.isfinite passes here cost as much as the kernels for small models)
            handles, n_handles = self._handle_array()
            _lib.check(_lib.lib().tbk_eigenval_multi(handles, n_handles, _lib.ptr(k_array), n_k, _lib.ptr(out)))
        return out[0] if single else out

    def eigh(self, k, convention=2):
        """
        Eigenvalues and eigenvectors of ``hamilton(k, convention)``: ``(E, U)`` with ``E (N,)`` float64 and ``U (N, N)``
        complex128 for one k-point, ``E (NK, N)`` and ``U (NK, N, N)`` for a list of k-points (arrays, not lists).
        ``E`` is ascending and ``U[..., :, j]`` is a unit eigenvector for ``E[..., j]``, as in ``scipy.linalg.eigh``; the
        columns of ``U`` are orthonormal.  The phase of every column is unspecified, as in LAPACK, and so is the basis
        chosen inside a degenerate eigenspace.  Not in the reference (``_tb_model.py`` has only ``eigenval``).
        """
        if convention not in [1, 2]:
            raise ValueError(
                "Invalid value '{}' for 'convention': must be either '1' or '2'".format(convention)
            )
        if np.shape(k) == (0,):  # an empty list of k-points
            k = np.zeros((0, self.dim))
        k_array, single = self._k_array(k)
        n_k = k_array.shape[0]
        eig = _outbuf.empty((n_k, self.size), np.float64)
        vec = _outbuf.empty((n_k, self.size, self.size), np.complex128)
        pos = np.ascontiguousarray(self.pos, dtype=np.float64) if convention == 1 else None
        with self._call_lock:
            # NaN / Inf in k or in the hoppings: TBK_ERR_NOT_FINITE -> ValueError; no convergence -> LinAlgError
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_eigh_multi(handles, n_handles, _lib.ptr(k_array), n_k, int(convention), _lib.ptr(pos),
                                          _lib.ptr(eig), _lib.ptr(vec))
            )
        return (eig[0], vec[0]) if single else (eig, vec)

    def _mesh_argument(self, mesh, what="dos"):
        """The mesh check ``dos``, ``pdos``, ``band_edges``, ``fermi_level``, ``tetra_weights``, ``occupations``, ``density_matrix``, ``green_function``, ``susceptibility``, ``dynamic_susceptibility`` and ``berry_flux`` share: ``mesh int32 (dim,)`` or ``ValueError``."""
        if self.dim not in (2, 3):
            raise ValueError("{} needs a 2- or 3-dimensional model, this one has dimension {}".format(what, self.dim))
        try:
            mesh_list = list(mesh)
        except TypeError:
            raise ValueError("mesh must be a sequence of {} positive integers".format(self.dim)) from None
        if len(mesh_list) != self.dim:
            raise ValueError("mesh has {} entries but the model has dimension {}".format(len(mesh_list), self.dim))
        for entry in mesh_list:
            if isinstance(entry, (bool, np.bool_)) or not isinstance(entry, (int, np.integer)):
                raise ValueError("mesh entries must be integers, got {!r}".format(entry))
            if entry < 1:
                raise ValueError("mesh entries must be positive, got {!r}".format(entry))
        mesh_array = np.array(mesh_list, dtype=np.int64)
        if int(np.prod(mesh_array, dtype=object)) >= 2 ** 31:
            raise ValueError("the mesh has 2^31 points or more")
        return np.ascontiguousarray(mesh_array, dtype=np.int32)

    def _dos_arguments(self, mesh, energies):
        """The checks ``dos`` and ``pdos`` share: ``(mesh int32 (dim,), grid float64 (NE,), mean step)`` or ``ValueError``."""
        mesh_array = self._mesh_argument(mesh)
        grid = np.array(energies, dtype=np.float64)
        if grid.ndim != 1 or grid.shape[0] < 2:
            raise ValueError("energies must be a 1-D array of at least two points")
        if not np.all(np.isfinite(grid)):
            raise ValueError("energies must be finite")
        steps = np.diff(grid)
        step = float((grid[-1] - grid[0]) / (grid.shape[0] - 1))  # the mean step
        if not step > 0 or np.any(steps <= 0):
            raise ValueError("energies must be ascending")
        if np.abs(steps - step).max() > 1e-9 * step:
            raise ValueError("energies must be uniformly spaced")
        return mesh_array, grid, step

    def dos(self, mesh, energies):
        """
        Number of states and density of states from a uniform k mesh by the linear tetrahedron method, computed on the GPU
        from eigenvalues that never leave it.  Not in the reference (``_tb_model.py`` has no density of states).

        ``mesh`` is a sequence of ``dim`` positive integers ``(n_1, ..., n_dim)``: the Gamma-centred, periodic mesh
        ``k = (i_1 / n_1, ..., i_dim / n_dim)``.  ``energies`` is a 1-D ascending, uniformly spaced grid of at least two points
        (``max|diff - mean diff| <= 1e-9 mean diff``).  Returns the named tuple ``(energies, nos, dos)``: ``nos[j]`` (shape
        ``(NE,)``) is the number of states per unit cell with energy ``<= energies[j]``, ``dos = np.diff(nos) / step`` (shape
        ``(NE - 1,)``) belongs to the bin midpoints.  ``nos`` is bounded and exact in its state count for flat bands
        (``nos[-1] == size`` when the grid ends above the spectrum); the pointwise g(E) is not computed.

        Decomposition: band ``b`` (the b-th ascending eigenvalue at every mesh point) is interpolated linearly inside simplices.
        In three dimensions every mesh cell is cut into the 6 tetrahedra that share its main diagonal -- corners
        ``0, e_a, e_a + e_b, e_a + e_b + e_c`` for every order ``(a, b, c)`` of the axes, weight ``1 / (6 NK)`` each; in two
        dimensions into the 2 triangles ``0, e_a, e_a + e_b``, weight ``1 / (2 NK)``.  One-dimensional models raise
        ``ValueError``.  With several ``devices`` every device takes a slab of the mesh along its first axis.
        """
        mesh_array, grid, step = self._dos_arguments(mesh, energies)
        nos = np.empty(grid.shape[0], dtype=np.float64)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigenval
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_dos_multi(handles, n_handles, _lib.ptr(mesh_array), float(grid[0]), step, grid.shape[0],
                                         _lib.ptr(nos))
            )
        return DensityOfStates(grid, nos, np.diff(nos) / step)

    def pdos(self, mesh, energies, projections):
        """
        Orbital-projected number of states and density of states from a uniform k mesh by the linear tetrahedron method, computed
        on the GPU from eigenvalues and eigenvectors that never leave it.  Not in the reference (``_tb_model.py`` has neither a
        density of states nor eigenvectors).

        ``mesh`` and ``energies`` are those of :meth:`dos`, with the same checks.  ``projections`` is a non-empty sequence of G
        groups (at most ``TBK_PDOS_MAX_GROUPS`` = 16), each a non-empty sequence of orbital indices in ``[0, size)`` without repeats
        inside the group; an orbital may appear in several groups or in none.  Returns the named tuple ``(energies, nos, dos)``:
        ``nos[g, j]`` (shape ``(G, NE)``) is the number of states per unit cell with energy ``<= energies[j]``, every state
        ``(k, b)`` weighted by ``A_g(k, b) = sum_{i in g} |U[k][i][b]|^2`` with ``U`` the eigenvectors of ``eigh(k, convention=2)``;
        ``dos = np.diff(nos, axis=1) / step`` (shape ``(G, NE - 1)``) belongs to the bin midpoints.  Over groups that partition
        the orbitals ``nos.sum(axis=0)`` is the ``nos`` of :meth:`dos`.

        Inside a degenerate eigenspace the split of ``A_g`` over the bands depends on the basis, which is unspecified (see
        :meth:`eigh`); the sum of ``A_g`` over the degenerate cluster does not.  The effect on ``nos`` is of the order of the
        method's own discretisation error.

        Decomposition: the simplices of :meth:`dos` -- in three dimensions the 6 tetrahedra that share the main diagonal of every
        mesh cell (corners ``0, e_a, e_a + e_b, e_a + e_b + e_c`` for every order of the axes), in two dimensions the 2 triangles
        ``0, e_a, e_a + e_b`` -- inside which both the band energy and ``A_g`` are interpolated linearly between the corners
        (Bloechl's corner weights).  One-dimensional models raise ``ValueError``.  With several ``devices`` every device takes a
        slab of the mesh along its first axis.
        """
        mesh_array, grid, step = self._dos_arguments(mesh, energies)
        try:
            groups = [list(group) for group in projections]
        except TypeError:
            raise ValueError("projections must be a sequence of sequences of orbital indices") from None
        if not groups:
            raise ValueError("projections must hold at least one group")
        if len(groups) > _lib.TBK_PDOS_MAX_GROUPS:
            raise ValueError("projections has {} groups, at most {} are supported".format(len(groups), _lib.TBK_PDOS_MAX_GROUPS))
        for group in groups:
            if not group:
                raise ValueError("a projection group is empty")
            for index in group:
                if isinstance(index, (bool, np.bool_)) or not isinstance(index, (int, np.integer)):
                    raise ValueError("orbital indices must be integers, got {!r}".format(index))
                if not 0 <= index < self.size:
                    raise ValueError("orbital index {!r} is outside [0, {})".format(index, self.size))
            if len(set(int(index) for index in group)) != len(group):
                raise ValueError("an orbital repeats inside the projection group {!r}".format(group))
        offsets = np.ascontiguousarray(np.cumsum([0] + [len(group) for group in groups]), dtype=np.int32)
        orbitals = np.ascontiguousarray(np.concatenate(groups), dtype=np.int32)
        nos = np.empty((len(groups), grid.shape[0]), dtype=np.float64)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_pdos_multi(handles, n_handles, _lib.ptr(mesh_array), _lib.ptr(offsets), _lib.ptr(orbitals), len(groups),
                                          float(grid[0]), step, grid.shape[0], _lib.ptr(nos))
            )
        return ProjectedDensityOfStates(grid, nos, np.diff(nos, axis=1) / step)

    def band_edges(self, mesh):
        """
        Minimum and maximum of every band over a uniform k mesh, computed on the GPU from eigenvalues that never leave it.  Not in
        the reference.  ``mesh`` is that of :meth:`dos`.  Returns the named tuple ``(emin, emax)`` of two ``(size,)`` arrays:
        ``emin[b]`` / ``emax[b]`` is the smallest / largest b-th ascending eigenvalue among the mesh points -- band widths, and for
        ``m`` filled bands the valence-band top ``emax[m - 1]``, the conduction-band bottom ``emin[m]`` and the gap of the mesh.
        """
        mesh_array = self._mesh_argument(mesh, "band_edges")
        emin = np.empty(self.size, dtype=np.float64)
        emax = np.empty(self.size, dtype=np.float64)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigenval
            handles, n_handles = self._handle_array()
            _lib.check(_lib.lib().tbk_band_edges_multi(handles, n_handles, _lib.ptr(mesh_array), _lib.ptr(emin), _lib.ptr(emax)))
        return BandEdges(emin, emax)

    def fermi_level(self, mesh, n_electrons):
        """
        The Fermi level of a uniform k mesh for ``n_electrons`` states per unit cell by the linear tetrahedron method, found on the
        GPU from eigenvalues that never leave it.  Not in the reference.

        ``mesh`` and the simplices are those of :meth:`dos`, and states are counted as its ``nos`` counts them (no spin factor):
        ``n_electrons`` is a real number inside ``(0, size)``.  Returns the named tuple ``(mu, lower, upper, nos)`` of floats.

        * ``n_electrons`` is an integer ``m`` and the mesh has a gap above band ``m - 1``: ``lower`` is the top of that band,
          ``upper`` the bottom of the next (the values of :meth:`band_edges`), ``mu`` their midpoint and ``nos == m``.
        * Otherwise ``mu == lower == upper`` is the smallest double at which the number of states reaches ``n_electrons``, found by
          a search on doubles (no energy grid is involved), and ``nos`` is the number of states there.  Across a band that is
          constant over the mesh the number of states jumps: for ``n_electrons`` inside the jump ``mu`` is that band's energy.

        ``lower < upper`` exactly when the result came from the gap.  With several ``devices`` every device keeps the eigenvalues
        of a slab of the mesh along its first axis.
        """
        mesh_array = self._mesh_argument(mesh, "fermi_level")
        if isinstance(n_electrons, (bool, np.bool_)) or not isinstance(n_electrons, (int, float, np.integer, np.floating)):
            raise ValueError("n_electrons must be a real number, got {!r}".format(n_electrons))
        count = float(n_electrons)
        if not np.isfinite(count) or not 0.0 < count < self.size:
            raise ValueError("n_electrons must lie inside (0, {}), got {!r}".format(self.size, n_electrons))
        out = np.empty(4, dtype=np.float64)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigenval
            handles, n_handles = self._handle_array()
            _lib.check(_lib.lib().tbk_fermi_multi(handles, n_handles, _lib.ptr(mesh_array), count, _lib.ptr(out)))
        return FermiLevel(float(out[0]), float(out[1]), float(out[2]), float(out[3]))

    def tetra_weights(self, mesh, energy):
        """
        The tetrahedron integration weight of every state of a uniform k mesh at ``energy``, computed on the GPU from eigenvalues
        that never leave it.  Not in the reference.

        ``mesh`` and the simplices are those of :meth:`dos`; ``energy`` is a finite real number.  Returns an array ``w`` of shape
        ``mesh + (size,)``: ``w[i_1, ..., i_dim, b]`` is Bloechl's corner weight of the mesh point in every simplex that contains
        it (24 tetrahedra in three dimensions, 6 triangles in two), summed and divided by their number per cell times ``NK``.
        Any Brillouin-zone integral over the states below ``energy`` is ``(w * A).sum()`` for ``A`` of the same shape;
        ``w.sum()`` is the ``nos`` of :meth:`dos` at ``energy``, ``0 <= NK w <= 1``, ``w`` is exactly 0 below the spectrum and
        exactly the double nearest ``1 / NK`` above it.  For given eigenvalues the result is reproducible bit for bit.

        This is the one call of the family that returns ``NK * size`` doubles; :meth:`occupations` keeps the weights on the GPU.
        One-dimensional models raise ``ValueError``.  With several ``devices`` every device takes a slab of the mesh along its
        first axis.
        """
        mesh_array = self._mesh_argument(mesh, "tetra_weights")
        value = self._energy_argument(energy)
        out = np.empty(tuple(int(n) for n in mesh_array) + (self.size,), dtype=np.float64)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigenval
            handles, n_handles = self._handle_array()
            _lib.check(_lib.lib().tbk_tetra_weights_multi(handles, n_handles, _lib.ptr(mesh_array), value, _lib.ptr(out)))
        return out

    @staticmethod
    def _energy_argument(energy):
        if isinstance(energy, (bool, np.bool_)) or not isinstance(energy, (int, float, np.integer, np.floating)):
            raise ValueError("energy must be a real number, got {!r}".format(energy))
        value = float(energy)
        if not np.isfinite(value):
            raise ValueError("energy must be finite, got {!r}".format(energy))
        return value

    def occupations(self, mesh, *, energy=None, n_electrons=None):
        """
        Orbital occupations, band occupations and band energies of a uniform k mesh by the linear tetrahedron method, computed on
        the GPU from eigenvalues, eigenvectors and integration weights that never leave it.  Not in the reference.

        ``mesh`` is that of :meth:`dos`.  Exactly one of ``energy`` (the chemical potential, a finite real number) and
        ``n_electrons`` (a real number inside ``(0, size)``: the chemical potential is that of :meth:`fermi_level`, bit for bit) is
        given, else ``ValueError``.  Returns the named tuple ``(mu, orbital_occ, band_occ, band_energy)``:

        * ``mu`` is the :class:`FermiLevel` tuple ``(mu, lower, upper, nos)`` -- for ``energy`` all three are ``energy`` and ``nos``
          is the number of states there;
        * ``orbital_occ[i] = sum_k sum_b w[k][b] |U[k][i][b]|^2`` with ``w`` of :meth:`tetra_weights` at ``mu.mu`` and ``U`` the
          eigenvectors of ``eigh(k, convention=2)``: the charge on orbital ``i`` (no spin factor);
        * ``band_occ[b] = sum_k w[k][b]`` in ``[0, 1]``, exactly 1 for a full band and exactly 0 for an empty one;
        * ``band_energy[b] = sum_k w[k][b] E[k][b]``; ``band_energy.sum()`` is the band energy per unit cell.

        ``orbital_occ.sum() == band_occ.sum() == mu.nos`` up to ``size * 2^-40``.  Inside a degenerate eigenspace the split of a
        state's weight over the orbitals depends on the basis, which is unspecified (see :meth:`eigh`); the sum over the degenerate
        cluster does not, so filled clusters (an insulator's valence bands) give a basis-independent ``orbital_occ``.
        One-dimensional models raise ``ValueError``.  With several ``devices`` every device takes a slab of the mesh along its
        first axis.
        """
        mesh_array = self._mesh_argument(mesh, "occupations")
        mode, value = self._occupation_argument("occupations", energy, n_electrons)
        mu = np.empty(4, dtype=np.float64)
        orbital, band, energy_out = (np.empty(self.size, dtype=np.float64) for _ in range(3))
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_occupations_multi(handles, n_handles, _lib.ptr(mesh_array), mode, value, _lib.ptr(mu), _lib.ptr(orbital),
                                                 _lib.ptr(band), _lib.ptr(energy_out))
            )
        return Occupations(FermiLevel(float(mu[0]), float(mu[1]), float(mu[2]), float(mu[3])), orbital, band, energy_out)

    def _occupation_argument(self, what, energy, n_electrons):
        """``(mode, value)`` of the C calls from exactly one of ``energy`` and ``n_electrons``, or ``ValueError``."""
        if (energy is None) == (n_electrons is None):
            raise ValueError("{} takes exactly one of energy and n_electrons".format(what))
        if energy is not None:
            return 0, self._energy_argument(energy)
        if isinstance(n_electrons, (bool, np.bool_)) or not isinstance(n_electrons, (int, float, np.integer, np.floating)):
            raise ValueError("n_electrons must be a real number, got {!r}".format(n_electrons))
        value = float(n_electrons)
        if not np.isfinite(value) or not 0.0 < value < self.size:
            raise ValueError("n_electrons must lie inside (0, {}), got {!r}".format(self.size, n_electrons))
        return 1, value

    def _lattice_vectors_argument(self, R):
        """``R int64 (NR, dim)`` from an integer array-like of that shape, one vector, or ``None`` (the stored hopping vectors)."""
        if R is None:
            keys = [key for key, _ in self._hop_items()]
            if not keys:
                raise ValueError("the model has no hoppings: give R")
            return np.ascontiguousarray(np.array(keys, dtype=np.int64).reshape(len(keys), self.dim))
        return self._integer_vectors_argument(R, "R", "NR")

    def _integer_vectors_argument(self, value, name, count):
        """``int64 (count, dim)`` from an integer array-like of that shape or one vector, or ``ValueError`` (``R`` of
        ``density_matrix``, ``q`` of ``susceptibility``)."""
        try:
            array = np.asarray(value)
        except (TypeError, ValueError):
            raise ValueError("{} must be an integer array of shape ({}, {})".format(name, count, self.dim)) from None
        if array.dtype.kind not in "iu" or array.dtype == np.uint64:
            raise ValueError("{} must hold (64-bit signed) integers, got dtype {}".format(name, array.dtype))
        if array.ndim == 1:
            array = array.reshape(1, -1)
        if array.ndim != 2 or array.shape[1] != self.dim or array.shape[0] < 1:
            raise ValueError("{} must have shape ({}, {}) with {} >= 1, got {}".format(name, count, self.dim, count, array.shape))
        return np.ascontiguousarray(array, dtype=np.int64)

    def density_matrix(self, mesh, *, energy=None, n_electrons=None, R=None):
        """
        The real-space one-particle density matrix ``rho(R)`` of a uniform k mesh by the linear tetrahedron method, computed on the
        GPU from eigenvalues, eigenvectors and integration weights that never leave it.  Not in the reference.

        ``mesh``, ``energy`` and ``n_electrons`` are those of :meth:`occupations`: exactly one of the last two is given, else
        ``ValueError``.  ``R`` is an integer array-like of shape ``(NR, dim)`` or one vector; duplicates are allowed; ``None`` means
        the model's stored hopping vectors in the order of ``self.hop``.  Returns the named tuple ``(mu, R, rho)``: ``mu`` is the
        :class:`FermiLevel` tuple of :meth:`occupations`, ``R`` the vectors as ``int64 (NR, dim)`` and ``rho`` is
        ``complex128 (NR, size, size)``.

        Definition.  With ``w`` of :meth:`tetra_weights` at ``mu.mu``, ``U`` the eigenvectors of ``eigh(k, convention=2)`` and the
        mesh points ``k = (i_1 / n_1, ..., i_dim / n_dim)``::

            P(k)[i, j]   = sum_b w[k, b] U[k, i, b] conj(U[k, j, b])
            rho(R)[i, j] = sum_k exp(-2 pi i k . R) P(k)[i, j]

        The sign is that of the inverse of ``hamilton``: H(k) sums ``exp(+2 pi i k . R) hop[R]``.  ``k . R`` is reduced in integers
        before any floating-point operation (every ``(i_d R_d) mod n_d``, then the common denominator ``NK``), so
        ``rho(R + n_d e_d)`` has the bits of ``rho(R)``: the mesh cannot tell them apart.  No spin factor.

        Properties.  (1) ``rho(-R) = rho(R)^H``; ``rho(0)`` is Hermitian, its diagonal is ``orbital_occ`` of :meth:`occupations`
        and its trace ``mu.nos``.  (2) Over the dual cell of the mesh, ``sum_{R in [0, n_1) x ... x [0, n_dim)} exp(+2 pi i k' . R)
        rho(R) = NK P(k')`` at every mesh point ``k'``.  (3) With the stored half of the hoppings (``R=None``), ``2 Re sum_R sum_ij
        conj(rho(R)[i, j]) hop[R][i, j]`` is the band energy per cell, ``occupations(...).band_energy.sum()``.  (4) Above the
        spectrum ``rho(R)`` is the identity for ``R = 0`` modulo the mesh and 0 otherwise; below the spectrum it is exactly 0.
        Every element is a sum of ``NK size`` terms whose moduli add up to at most 1: the rounding error is at most
        ``4 (NK size + 32) 2^-53``.  Repeated calls give the same bits.

        Inside a degenerate eigenspace the split of a state's weight over the bands depends on the basis, which is unspecified (see
        :meth:`eigh`); ``rho`` of a cluster that is filled as a whole (an insulator's valence bands) does not.  One-dimensional
        models raise ``ValueError``.  With several ``devices`` every device contracts a slab of the mesh along its first axis and
        the host adds the slabs.
        """
        mesh_array = self._mesh_argument(mesh, "density_matrix")
        mode, value = self._occupation_argument("density_matrix", energy, n_electrons)
        vectors = self._lattice_vectors_argument(R)
        mu = np.empty(4, dtype=np.float64)
        rho = np.empty((vectors.shape[0], self.size, self.size), dtype=np.complex128)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_density_matrix_multi(handles, n_handles, _lib.ptr(mesh_array), mode, value, vectors.shape[0],
                                                    _lib.ptr(vectors), _lib.ptr(mu), _lib.ptr(rho))
            )
        return DensityMatrix(FermiLevel(float(mu[0]), float(mu[1]), float(mu[2]), float(mu[3])), vectors, rho)

    @staticmethod
    def _complex_energies_argument(z, *, off_axis=True):
        """``z complex128 (NZ,)`` from a complex number or a sequence of 1 to 4096 of them, every one finite and, unless
        ``off_axis`` is false, with ``Im z != 0``."""
        if z is None or isinstance(z, (str, bytes)):
            raise ValueError("z must be a complex number or a sequence of them, got {!r}".format(z))
        try:
            array = np.asarray(z)
            if array.dtype.kind not in "iufc":
                raise TypeError
            array = array.astype(np.complex128)
        except (TypeError, ValueError):
            raise ValueError("z must be a complex number or a sequence of them") from None
        if array.ndim == 0:
            array = array.reshape(1)
        if array.ndim != 1 or not 1 <= array.shape[0] <= 4096:
            raise ValueError("z must be one energy or a sequence of 1 to 4096, got shape {}".format(array.shape))
        if not (np.all(np.isfinite(array.real)) and np.all(np.isfinite(array.imag))):
            raise ValueError("z must be finite")
        if off_axis and np.any(array.imag == 0.0):
            raise ValueError("every z needs Im z != 0: the resolvent is evaluated off the real axis only")
        return np.ascontiguousarray(array)

    def _self_energy_argument(self, self_energy, z, n_z):
        """``Sigma complex128 (NZ, size, size)`` from an array-like of that shape (``(size, size)`` when ``z`` is one number), every
        entry finite."""
        if isinstance(self_energy, (str, bytes)):
            raise ValueError("self_energy must be a complex array of shape (NZ, size, size), got {!r}".format(self_energy))
        try:
            array = np.asarray(self_energy)
            if array.dtype.kind not in "iufc":
                raise TypeError
            array = array.astype(np.complex128)
        except (TypeError, ValueError):
            raise ValueError("self_energy must be a complex array of shape (NZ, size, size)") from None
        if array.ndim == 2 and np.ndim(z) == 0:
            array = array.reshape((1,) + array.shape)
        if array.shape != (n_z, self.size, self.size):
            raise ValueError(
                "self_energy must have shape ({}, {}, {}): one matrix per energy, got {}".format(n_z, self.size, self.size, array.shape)
            )
        if not (np.all(np.isfinite(array.real)) and np.all(np.isfinite(array.imag))):
            raise ValueError("self_energy must be finite")
        return np.ascontiguousarray(array)

    def green_function(self, mesh, z, *, R=None, self_energy=None):
        """
        The lattice Green's function (the resolvent) ``G(R, z)`` of a uniform k mesh at complex energies, computed on the GPU from
        eigenvalues and eigenvectors that never leave it.  Not in the reference.

        ``mesh`` is that of :meth:`occupations`.  ``z`` is a complex number or a sequence of 1 to 4096 of them, every one finite
        with ``Im z != 0`` of either sign (retarded, advanced, Matsubara or contour points), else ``ValueError``.  ``R`` is an
        integer array-like of shape ``(NR, dim)`` or one vector; duplicates are allowed; ``None`` means the model's stored hopping
        vectors in the order of ``self.hop``.  Returns the named tuple ``(z, R, G)``: ``z`` as ``complex128 (NZ,)``, ``R`` as
        ``int64 (NR, dim)`` and ``G`` as ``complex128 (NR, NZ, size, size)``.

        Definition.  With ``E, U`` of ``eigh(k, convention=2)`` at the mesh points ``k = (i_1 / n_1, ..., i_dim / n_dim)``::

            P(k, z)[i, j] = sum_b (1 / (z - E[k, b])) U[k, i, b] conj(U[k, j, b]) / NK
            G(R, z)[i, j] = sum_k exp(-2 pi i k . R) P(k, z)[i, j]

        that is ``(1 / NK) sum_k exp(-2 pi i k . R) (z - H(k))^-1``.  The sign is that of :meth:`density_matrix`, the inverse of
        ``hamilton``, and ``k . R`` is reduced in integers before any floating-point operation, so ``G(R + n_d e_d, z)`` has the
        bits of ``G(R, z)``.  ``R`` is a lattice vector: convention 2 only.  No spin factor.

        Properties.  (1) ``G(R, conj(z)) = G(-R, z)^H``.  (2) ``-Im tr G(0, w + i eta) / pi`` is the Lorentzian-broadened density
        of states ``(1 / NK) sum_{k, b} (eta / pi) / ((w - E[k, b])^2 + eta^2)``, its diagonal the orbital-resolved one.  (3) Over
        the dual cell of the mesh ``G`` solves the Dyson equation of the hoppings folded onto the mesh torus,
        ``sum_R' (z delta(R') - H(R')) G(R - R', z) = delta(R)``.  (4) ``z G(R, z)`` tends to the identity for ``R = 0`` modulo
        the mesh and to 0 otherwise as ``|z|`` grows.  (5) The bits of ``G(R, z)`` do not depend on the other entries of ``z`` and
        ``R``, on their order or number; a duplicate has the bits of its original and a second call the bits of the first.

        Error bound for a given eigensystem, with ``eta = min |Im z|``: every element is a sum of ``NK size`` terms whose moduli
        add up to at most ``1 / eta``, so the rounding error is at most ``4 (NK size + 32) 2^-53 / eta`` per component.  Against
        the exact resolvent the computed eigensystem adds ``(||U U^H - 1|| + ||H U - U E|| ||U|| / eta) / eta``.

        Work: ``8 size^3`` flops per mesh point and energy for the projectors and ``8 NR size^2`` for the transform, both on the
        FP64 matrix pipe, beside one eigensolve per mesh point whatever ``NZ``.  ``G`` and its partial sums (``NR NZ size^2``
        complex numbers, times the k slices of the transform) stay in device memory, else ``MemoryError``.  One-dimensional models
        raise ``ValueError``.  With several ``devices`` every device contracts a slab of the mesh along its first axis and the host
        adds the slabs.

        Dressed function.  ``self_energy`` is a local, energy-dependent self-energy ``Sigma``: a complex array-like of shape
        ``(NZ, size, size)``, one matrix per energy (a single ``(size, size)`` matrix when ``z`` is one number), every entry finite,
        else ``ValueError``.  It need not be Hermitian or causal.  With it ``z`` may be any finite complex number, real ones
        included (``Sigma`` carries its own broadening), and no eigensystem is computed: with ``H(k)`` of
        ``hamilton(k, convention=2)``::

            A(k, z) = z 1 - H(k) - Sigma(z)
            P(k, z) = A(k, z)^-1 / NK
            G(R, z) = sum_k exp(-2 pi i k . R) P(k, z)

        by one general inversion per mesh point and energy on the GPU -- Gauss-Jordan elimination with partial pivoting on
        ``|re| + |im|`` up to 64 orbitals, the library's LU above -- and the transform above.  A singular ``A(k, z)`` (a pivot that
        is exactly zero, or a non-finite element of the inverse) raises ``numpy.linalg.LinAlgError`` naming the first such mesh
        point and energy; no NaN is returned.  Properties.  (1) ``Sigma = 0`` reproduces the undressed ``G`` within the sum of both
        bounds.  (2) ``Sigma(z) = s(z) 1`` gives the undressed ``G`` at ``z - s(z)``.  (3) A constant Hermitian ``Sigma = S`` gives
        the undressed ``G`` of the model with ``S`` added on site.  (4) ``G(R, conj(z); Sigma^H) = G(-R, z; Sigma)^H``.  (5) Over the
        dual cell of the mesh ``sum_R' ((z - Sigma(z)) delta(R') - H(R')) G(R - R', z) = delta(R)``.  (6) The bits of ``G(R, z)``
        depend on ``(R, z, Sigma(z))`` alone: not on the other energies, their order, the other vectors or duplicates, and
        ``R + n_d e_d`` has the bits of ``R``.  Error bound per component, with ``u = 2^-53``, ``rho`` the growth factor of the
        elimination and the 2-norm condition number ``kappa_2``: ``max_k 8 size u rho kappa_2(A) ||A^-1|| + 4 (NK + 32) u max_k
        ||A^-1||``; for causal input ``||A^-1|| <= 1 / |Im z|``.  Work: ``8 size^3`` flops per mesh point and
        energy, no eigensolve.
        """
        mesh_array = self._mesh_argument(mesh, "green_function")
        energies = self._complex_energies_argument(z, off_axis=self_energy is None)
        vectors = self._lattice_vectors_argument(R)
        G = np.empty((vectors.shape[0], energies.shape[0], self.size, self.size), dtype=np.complex128)
        if self_energy is not None:
            sigma = self._self_energy_argument(self_energy, z, energies.shape[0])
            with self._call_lock:
                # a singular z - H(k) - Sigma(z): TBK_ERR_SINGULAR -> numpy.linalg.LinAlgError, as numpy.linalg.inv
                handles, n_handles = self._handle_array()
                _lib.check(
                    _lib.lib().tbk_green_dressed_multi(handles, n_handles, _lib.ptr(mesh_array), energies.shape[0], _lib.ptr(energies),
                                                       _lib.ptr(sigma), vectors.shape[0], _lib.ptr(vectors), _lib.ptr(G))
                )
            return GreenFunction(energies, vectors, G)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_green_function_multi(handles, n_handles, _lib.ptr(mesh_array), energies.shape[0], _lib.ptr(energies),
                                                    vectors.shape[0], _lib.ptr(vectors), _lib.ptr(G))
            )
        return GreenFunction(energies, vectors, G)

    def _stacking_arguments(self, k, z, axis, max_iterations):
        """(energies, axis index, cap, in-plane k array, L) of `surface_green_function` and `transmission`."""
        energies = self._complex_energies_argument(z, off_axis=True)
        try:
            axis_index = int(axis)
        except (TypeError, ValueError):
            raise ValueError("axis must be an integer, got {!r}".format(axis)) from None
        if axis_index != axis or not -self.dim <= axis_index < self.dim:
            raise ValueError("axis must be an integer in [-{0}, {0}), got {1!r}".format(self.dim, axis))
        axis_index %= self.dim
        try:
            cap = int(max_iterations)
        except (TypeError, ValueError):
            raise ValueError("max_iterations must be an integer from 1 to 4096, got {!r}".format(max_iterations)) from None
        if cap != max_iterations or not 1 <= cap <= 4096:
            raise ValueError("max_iterations must be an integer from 1 to 4096, got {!r}".format(max_iterations))
        if self.dim == 1 and (k is None or np.shape(k) == (0,)):
            k_array = np.zeros((1, 0), dtype=np.float64)
        else:
            if k is None:
                raise ValueError("k must be an array of shape (NK, {}), got None".format(self.dim - 1))
            k_array = np.asarray(k, dtype=np.float64)
            if k_array.ndim == 0 and self.dim == 2:
                k_array = k_array.reshape(1, 1)
            elif k_array.ndim == 1 and k_array.shape[0] == self.dim - 1:
                k_array = k_array.reshape(1, -1)
            if k_array.ndim != 2 or k_array.shape[1] != self.dim - 1:
                raise ValueError("k must have shape (NK, {}): in-plane points without component {}, got {}".format(
                    self.dim - 1, axis_index, np.shape(k)))
            k_array = np.ascontiguousarray(k_array)
        if not np.all(np.isfinite(k_array)):
            raise ValueError("k must be finite")
        layers = max([abs(int(R[axis_index])) for R in self.hop] or [0])
        return energies, axis_index, cap, k_array, layers

    def surface_green_function(self, k, z, *, axis=-1, spectral=False, max_iterations=64):
        """
        Surface and bulk Green's functions of the semi-infinite crystal stacked along ``axis``, by the iterative decimation of
        Lopez Sancho, Lopez Sancho and Rubio (J. Phys. F 15, 851 (1985)) on the GPU.  Not in the reference.

        ``k`` is an array-like of in-plane points of shape ``(NK, dim - 1)`` -- the reduced coordinates with component ``axis``
        removed -- or one such point; for a one-dimensional model it is ``None`` or of shape ``(NK, 0)``, and there is one point.
        ``z`` is a complex number or a sequence of 1 to 4096 of them, every one finite with ``Im z != 0`` of either sign, else
        ``ValueError``.  ``axis`` counts as Python indices do (``-1``: the last).  Returns the named tuple ``(k, z, layers,
        iterations, bottom, top, bulk)``: ``k`` as ``float64 (NK, dim - 1)``, ``z`` as ``complex128 (NZ,)``, ``layers`` the
        number ``L`` of cells in a principal layer, ``iterations`` as ``int32 (NK, NZ)`` and the three functions as ``complex128
        (NK, NZ, N, N)`` with ``N = size * max(L, 1)``.  With ``spectral=True`` the three are ``float64 (NK, NZ, N)`` holding
        ``-Im diag(G) / pi``, written by the kernel itself: no matrix leaves the device, which is what a map over a k path and an
        energy grid wants.  The leading axis is kept for a single point.

        Definition.  With ``hop_full[R]`` the full hopping matrices (``hamilton(k, convention=2) = sum_R exp(2 pi i k.R)
        hop_full[R]``), ``a`` the axis and ``kp`` an in-plane point::

            H_m(kp)   = sum_{R : R_a = m} exp(2 pi i kp.Rp) hop_full[R]       m = -L ... L,  L = max |R_a| over self.hop
            H00[p, q] = H_{q - p}                                             p, q = 0 ... L - 1: blocks of size x size
            H01[p, q] = H_{L + q - p} if q <= p else 0                        principal layer P to P + 1

        Block ``p`` is the cell at position ``p`` along ``+a`` inside its principal layer; within a block the orbitals keep the
        model's order.  Per ``(kp, z)``, from ``es = et = e = H00``, ``alpha = H01``, ``beta = H01^H``::

            repeat   g = (z - e)^-1
                     T = g alpha:   alpha' = alpha T,  et += beta T,  e += beta T
                     T = g beta:    es += alpha T,  e += alpha T,  beta' = beta T
            bottom = (z - es)^-1      the crystal on principal layers P >= 0; its surface cell is block 0
            top    = (z - et)^-1      the crystal on principal layers P <= 0; its surface cell is block L - 1
            bulk   = (z - e)^-1       a principal layer deep inside

        Stopping rule, part of the definition: after an update the iteration stops when ``max(|alpha|, |beta|) <= 2^-53 |H01|``,
        the norms being the largest row sums of ``|re| + |im|``; from there on the updates would change no bit.  It takes 6 to 17
        iterations for ``|Im z|`` between 0.5 and 0.001.  A ``(kp, z)`` that reaches ``max_iterations`` (1 to 4096) and a singular
        ``z - e`` (a zero pivot or a non-finite element of an inverse) raise ``numpy.linalg.LinAlgError`` naming the k index and
        the energy.  With ``L = 0`` (no hopping along the axis) there is no iteration and all three are ``(z - H00)^-1``.

        Properties.  (1) ``bottom = (z - H00 - H01 bottom H01^H)^-1`` and ``bulk = (z - H00 - H01 bottom H01^H - H01^H top
        H01)^-1``.  (2) ``G(conj(z)) = G(z)^H``.  (3) ``bottom[:N, :N]`` is the corner block of the resolvent of a slab of many
        principal layers, up to the slab's finite-size error.  (4) The bits of one ``(kp, z)`` depend on nothing else: not on the
        other points or energies, their order, or the chunking.  (5) ``-Im tr / pi`` of ``bottom`` over a k path and an energy
        grid is the surface spectral map; ``bulk`` has the bulk bands alone.

        Lead self-energy.  ``H01 @ bottom @ H01^H`` is the self-energy a semi-infinite lead on the ``+a`` side adds to the layer in
        front of it (``H01^H @ top @ H01`` for the ``-a`` side); for ``L = 1`` it has the shape ``green_function(self_energy=...)``
        takes.  ``H01`` is ``H_L`` summed directly from ``self.hop``, or the difference of the fixed point (1).

        Error bound per component, with ``u = 2^-53``, ``rho`` the growth factor of the eliminations and ``eta = |Im z|``:
        ``8 N u rho (|z| + |H00| + 2 |H01|) / eta^2 (iterations + 1)``: every step keeps ``e``, ``es``, ``et``
        causal, so ``|g| <= 1 / eta``.

        Work: per iteration one inversion and six products of ``N x N`` complex matrices, ``56 N^3`` flops, six sevenths of them
        plain products on the FP64 matrix pipe; one workgroup keeps a ``(kp, z)`` for the whole iteration.  ``H_m`` comes from
        ``hamilton`` at ``2 L + 1`` points along the axis by a discrete Fourier sum, so dense, CSR and folded models all work.
        Above ``N = 64``, and for a model with ``TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER``, the same iteration runs in lockstep over
        batches of ``(kp, z)`` on rocBLAS and rocSOLVER (``N`` up to 1024, else ``ValueError``); a member that has converged gets
        ``alpha = beta = 0`` exactly, so its bits do not depend on its neighbours.  With several ``devices`` the k list is split as
        for ``hamilton``.
        """
        energies, axis_index, cap, k_array, layers = self._stacking_arguments(k, z, axis, max_iterations)
        n_rows = self.size * max(layers, 1)
        if n_rows > 1024:
            raise ValueError("a principal layer of {} cells has {} rows: surface_green_function takes at most 1024".format(layers, n_rows))
        n_k, n_z = k_array.shape[0], energies.shape[0]
        shape = (n_k, n_z, n_rows) if spectral else (n_k, n_z, n_rows, n_rows)
        dtype = np.float64 if spectral else np.complex128
        iterations = np.zeros((n_k, n_z), dtype=np.int32)
        bottom, top, bulk = (np.empty(shape, dtype=dtype) for _ in range(3))
        with self._call_lock:
            # the cap reached: TBK_ERR_NO_CONVERGENCE, a singular z - e: TBK_ERR_SINGULAR -> numpy.linalg.LinAlgError
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_surface_green_multi(handles, n_handles, axis_index, layers, _lib.ptr(k_array) if k_array.size else None, n_k, n_z,
                                                   _lib.ptr(energies), cap, 1 if spectral else 0, _lib.ptr(iterations), _lib.ptr(bottom),
                                                   _lib.ptr(top), _lib.ptr(bulk))
            )
        return SurfaceGreenFunction(k_array, energies, layers, iterations, bottom, top, bulk)

    def transmission(self, k, z, *, axis=-1, device=None, length=1, max_iterations=64, green=False):
        """
        The two-terminal Landauer transmission ``T(kp, z)`` through a device of ``M`` principal layers between two semi-infinite
        leads of the crystal, stacked along ``axis``, on the GPU.  Not in the reference.

        ``k``, ``z``, ``axis``, ``max_iterations`` and the error messages are those of :meth:`surface_green_function`; ``H00``,
        ``H01``, ``N = size * L`` and the decimation with its stopping rule are its as well.  ``device`` is ``None`` --
        ``length`` pristine layers, ``V = 0`` -- or an array ``(M, N, N)`` of Hermitian matrices ``V_p``, ordered in blocks as
        ``H00`` and independent of ``kp``, or an array ``(M, N)`` of real on-site energies (expanded to diagonal matrices on the
        host); ``1 <= M <= 4096``.  A ``device`` with ``max|V - V^H| > 1e-12 max|V|`` raises ``ValueError``; otherwise it is
        passed as given.  A model without hopping along ``axis`` raises ``ValueError``.  Returns the named tuple ``(k, z, layers,
        length, iterations, transmission[, green])``: ``length`` is ``M``, ``transmission`` is ``float64 (NK, NZ)`` and, with
        ``green=True``, ``green`` is ``P_M`` as ``complex128 (NK, NZ, N, N)``.  Without it one double per ``(kp, z)`` leaves the
        GPU.

        Definition.  The device is the principal layers ``p = 1 ... M`` with on-site blocks ``H00(kp) + V_p``, ``H01`` between
        neighbouring layers and towards both leads; the left lead is the crystal on the layers ``P <= 0``, the right lead on
        ``P >= M + 1``.  Per ``(kp, z)``::

            es, et, iterations      the decimation, without its closing inversions
            Gamma_R = i (es - es^H),    Gamma_L = i (et - et^H)         es - H00, et - H00: the leads' self-energies
            D_1 = et + V_1
            for p = 1 ... M:    if p = M:  D_p += es - H00
                                g_p = (z - D_p)^-1
                                P_p = g_p  (p = 1),   g_p (H01^H P_{p-1})  (p > 1)
                                D_{p+1} = (H00 + V_{p+1}) + H01^H (g_p H01)   (p < M)
            T = Re tr[(Gamma_R P_M) (Gamma_L P_M^H)]

        ``P_M`` is block ``(M, 1)`` of the resolvent of the device with both self-energies attached.  The order of the operations
        is part of the definition.  The cap of the decimation and a singular ``z - D_p`` (a zero pivot, or a non-finite element of
        a ``g_p`` or of ``P_M``) raise ``numpy.linalg.LinAlgError`` naming the k index and the energy.

        Properties.  (1) Without a device potential and for ``Im z -> 0``, ``T`` is the number of right-moving bands at ``Re z``,
        whatever ``length``; it vanishes in a gap.  (2) ``T`` at ``conj(z)`` is the transmission from the other side: that of
        the reversed stack at ``z``; the two directions agree for ``Im z -> 0``.  (3) A barrier of growing height drives ``T`` to 0.  (4) The bits of one ``(kp, z)`` depend on
        nothing else: not on the other points or energies, their order, the chunking, or ``green``.  (5) The mean of ``T`` over
        ``kp`` is the conductance per cell in units of ``e^2 / h``.

        Error bound, with ``u = 2^-53``, ``rho`` the growth factor of the eliminations and ``eta = |Im z|``: ``|T - exact| <= 4 eps
        scale``, ``eps = 8 N u rho (|z| + |H00| + 2 |H01| + max |V_p|) / eta (iterations + M + 1)`` and ``scale = N (2 |H01|^2
        |G_bottom|) (2 |H01|^2 |G_top|) |P_M|^2`` in 2-norms.

        Work: ``56 N^3`` flops per iteration of the decimation and ``40 N^3`` per layer.  Up to ``N = 64`` one workgroup owns a
        ``(kp, z)`` from the first iteration to the trace; above, to 1024, and for a model with ``TBK_OPT_EIGENSOLVER =
        TBK_EIG_ROCSOLVER``, the decimation and the sweep run in lockstep batches on rocBLAS and rocSOLVER.  With several
        ``devices`` the k list is split as for ``hamilton``.
        """
        energies, axis_index, cap, k_array, layers, potential = self._device_arguments(k, z, axis, max_iterations, device, length, "transmission", 1024)
        n_rows = self.size * layers
        n_k, n_z, count = k_array.shape[0], energies.shape[0], potential.shape[0]
        iterations = np.zeros((n_k, n_z), dtype=np.int32)
        result = np.empty((n_k, n_z), dtype=np.float64)
        matrices = np.empty((n_k, n_z, n_rows, n_rows), dtype=np.complex128) if green else None
        with self._call_lock:
            # the cap reached: TBK_ERR_NO_CONVERGENCE, a singular z - D: TBK_ERR_SINGULAR -> numpy.linalg.LinAlgError
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_transmission_multi(handles, n_handles, axis_index, layers, _lib.ptr(k_array) if k_array.size else None, n_k, count,
                                                  _lib.ptr(potential), n_z, _lib.ptr(energies), cap, _lib.ptr(iterations), _lib.ptr(result),
                                                  _lib.ptr(matrices))
            )
        if green:
            return TransmissionGreen(k_array, energies, layers, count, iterations, result, matrices)
        return Transmission(k_array, energies, layers, count, iterations, result)

    def transmission_ensemble(self, k, z, devices, *, axis=-1, max_iterations=64):
        """
        The transmission :meth:`transmission` of an ensemble of ``S`` devices between the same two leads -- the disorder samples of
        one ``(kp, z)`` after ONE decimation -- on the GPU.  Not in the reference.

        ``k``, ``z``, ``axis``, ``max_iterations`` and their error messages are those of :meth:`transmission`.  ``devices`` is an
        array ``(S, M, N)`` of real on-site energies (Anderson disorder; a complex array raises ``ValueError``) or an array ``(S,
        M, N, N)`` of Hermitian matrices under :meth:`transmission`'s rule, ``max|V - V^H| <= 1e-12 max|V|`` over the whole
        array; the number of dimensions decides the form, and any other shape raises ``ValueError``.  ``1 <= S <= 4096``, ``1 <=
        M <= 4096``, the array finite and at most 256 MiB as staged: on-site energies stay diagonal all the way into the kernel,
        so ``S M N`` doubles are staged and not ``S M N^2`` complex numbers.  ``N = size * L <= 1024``; a model without hopping
        along ``axis`` raises ``ValueError``.  Returns the named tuple ``(k, z, layers, length, samples, iterations,
        transmission)``: ``length`` is ``M``, ``samples`` is ``S``, ``iterations`` is ``int32 (NK, NZ)`` and ``transmission`` is
        ``float64 (NK, NZ, S)``.  ``S`` doubles per ``(kp, z)`` leave the GPU; ``<ln T>``, the variance and the rest are one NumPy
        line on them.

        Definition.  ``transmission[k, z, s]`` is ``transmission(k, z, device=devices[s])``, unchanged down to the order of the
        operations.  The decimation does not depend on the device, so it is computed once for a group of samples; the sweep and
        the trace run once per sample on what it left.  The cap of the decimation and a singular ``z - D_p`` raise
        ``numpy.linalg.LinAlgError``; the message names the k index, the energy and, for a singular sweep, the sample -- the
        first offender in that order of precedence.

        Properties.  (1) Up to ``N = 64`` every ``transmission[k, z, s]`` and ``iterations[k, z]`` have the bits of
        :meth:`transmission` called with ``devices[s]`` alone.  (2) The on-site form has the bits of the matrix form on the
        expanded diagonal: the kernel adds the energy on the diagonal and ``0.0`` elsewhere in the same expressions.  (3) The
        bits of one ``(kp, z, s)`` depend on nothing else: not on the other samples or their order, the points, the energies,
        the chunking or the grouping of the samples.

        Error bound per sample: that of :meth:`transmission`.

        Work: ``56 N^3`` flops per iteration of the decimation, once per group of samples, and ``40 N^3`` per layer and sample; a
        loop over :meth:`transmission` pays ``(iterations 56 + M 40) / (M 40)`` times the flops for many samples, and ``H(k)``,
        the layers and a dense copy of ``V`` per call on top.  Up to ``N = 64`` a work item is ``(kp, z, group of samples)``: the
        samples are split into just enough groups to fill the device's resident workgroups, because every group repeats the
        decimation -- one ``(kp, z)`` with many samples still fills the GPU.  Above, to 1024, and for a model with
        ``TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER``, the library route of :meth:`transmission` runs its decimation once per
        lockstep batch and its sweep per sample.  With several ``devices`` of the model the k list is split as for ``hamilton``.
        """
        energies, axis_index, cap, k_array, layers = self._stacking_arguments(k, z, axis, max_iterations)
        if layers == 0:
            raise ValueError("the model has no hopping along axis {}: there is nothing to transmit".format(axis_index))
        n_rows = self.size * layers
        if n_rows > 1024:
            raise ValueError("a principal layer of {} cells has {} rows: transmission_ensemble takes at most 1024".format(layers, n_rows))
        staged = self._ensemble_devices_argument(devices, n_rows)
        samples, count = staged.shape[:2]
        n_k, n_z = k_array.shape[0], energies.shape[0]
        iterations = np.zeros((n_k, n_z), dtype=np.int32)
        result = np.empty((n_k, n_z, samples), dtype=np.float64)
        with self._call_lock:
            # the cap reached: TBK_ERR_NO_CONVERGENCE, a singular z - D: TBK_ERR_SINGULAR -> numpy.linalg.LinAlgError
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_transmission_ensemble_multi(handles, n_handles, axis_index, layers, _lib.ptr(k_array) if k_array.size else None, n_k,
                                                           count, samples, _lib.ptr(staged) if staged.ndim == 4 else None,
                                                           _lib.ptr(staged) if staged.ndim == 3 else None, n_z, _lib.ptr(energies), cap,
                                                           _lib.ptr(iterations), _lib.ptr(result))
            )
        return TransmissionEnsemble(k_array, energies, layers, count, samples, iterations, result)

    @staticmethod
    def _ensemble_devices_argument(devices, n_rows):
        """The devices of `transmission_ensemble` and `transmission_channels` as staged: float64 (S, M, N) or complex128 (S, M, N, N)."""
        given = np.asarray(devices)
        shapes = "devices must have shape (S, M, {0}) or (S, M, {0}, {0}) with S, M >= 1, got {1}".format(n_rows, given.shape)
        if given.ndim == 3:
            if given.shape[2] != n_rows or given.shape[0] < 1 or given.shape[1] < 1:
                raise ValueError(shapes)
            if np.iscomplexobj(given):
                raise ValueError("on-site energies of shape (S, M, {}) must be real".format(n_rows))
            staged = np.ascontiguousarray(given, dtype=np.float64)
        elif given.ndim == 4:
            if given.shape[2:] != (n_rows, n_rows) or given.shape[0] < 1 or given.shape[1] < 1:
                raise ValueError(shapes)
            staged = np.ascontiguousarray(given, dtype=np.complex128)
        else:
            raise ValueError(shapes)
        samples, count = staged.shape[:2]
        if samples > 4096 or count > 4096 or staged.nbytes > 256 << 20:
            raise ValueError("devices has {} samples of {} layers of {} rows: at most 4096 samples, 4096 layers and 256 MiB".format(
                samples, count, n_rows))
        if not np.all(np.isfinite(staged.view(np.float64))):
            raise ValueError("devices must be finite")
        if staged.ndim == 4:
            size = float(np.abs(staged).max())
            skew = max(float(np.abs(sample - np.conj(np.transpose(sample, (0, 2, 1)))).max()) for sample in staged)
            if skew > 1e-12 * size:
                raise ValueError("devices is not Hermitian: max|V - V^H| = {:.3e}".format(skew))
        return staged

    def transmission_channels(self, k, z, *, axis=-1, device=None, length=1, devices=None, max_iterations=64):
        """
        The transmission eigenvalues ``T_n`` of the device of :meth:`transmission` -- the channels of the Landauer-Buettiker
        picture -- and the shot noise ``sum_n T_n (1 - T_n)``, for one device or an ensemble of them, on the GPU.  Not in the
        reference.

        ``k``, ``z``, ``axis``, ``max_iterations`` and their error messages are those of :meth:`transmission`.  The device is
        given in one of two ways.  ``device`` and ``length`` are those of :meth:`transmission`: one sample.  ``devices`` is that
        of :meth:`transmission_ensemble`: ``S`` samples as on-site energies ``(S, M, N)``, which stay diagonal into the kernel,
        or Hermitian matrices ``(S, M, N, N)``.  Giving both ``device`` and ``devices`` raises ``ValueError``.  ``N = size * L
        <= 64``, else ``ValueError``.  Returns the named tuple ``(k, z, layers, length, samples, iterations, transmission,
        channels, noise)``: ``length`` is ``M``, ``samples`` is ``S`` (``1`` without ``devices``), ``iterations`` is ``int32
        (NK, NZ)``, ``transmission`` and ``noise`` are ``float64 (NK, NZ[, S])`` and ``channels`` is ``float64 (NK, NZ[, S],
        N)``, descending along its last axis; the ``S`` axis is there only with ``devices``.  ``N + 1`` doubles per ``(kp, z,
        sample)`` leave the GPU: no ``P_M``, no self-energy.

        Definition.  With ``es``, ``et`` and ``P_M`` of :meth:`transmission` and ``s = sign(Im z)``::

            B_R = s i (es - es^H),   B_L = s i (et - et^H)      positive semidefinite up to rounding for either sign of Im z
            B = L L^H                Cholesky with diagonal pivoting; it stops at rank r when the largest remaining diagonal is
                                     <= N u d0, d0 the largest diagonal of B, u = 2^-53: the other columns of L are exactly zero
            t = L_R^H (P_M L_L)      so that tr t^H t = tr[Gamma_R P_M Gamma_L P_M^H]
            T_n = the squared singular values of t, descending

        by a one-sided (Hestenes) Jacobi iteration on the columns of ``t`` -- of ``t^H`` when ``r_R < r_L``, so that the
        ``N - min(r_R, r_L)`` zero columns stay columns -- in the round-robin order: a pair of columns with ``a = |t_p|^2``, ``b =
        |t_q|^2``, ``c = t_p^H t_q`` is skipped when ``a == 0``, ``b == 0`` or ``|c| <= N u sqrt(a) sqrt(b)`` and rotated to
        orthogonality otherwise; the first sweep without a rotation is the last.  ``noise`` is ``sum_n T_n (1 - T_n)`` of the
        returned ``channels``, summed on the host; the Fano factor is ``noise / transmission``.  A lead with fewer open directions
        than rows (a singular ``H01``) is the normal case.  The errors are those of :meth:`transmission_ensemble`; a Jacobi
        that still rotates in its 48th sweep raises ``numpy.linalg.LinAlgError`` naming the channel iteration, the k index, the
        energy and the sample (the inputs of the tests need 20 sweeps at most).

        Properties.  (1) ``transmission`` and ``iterations`` have the bits of :meth:`transmission_ensemble` and, for one sample,
        of :meth:`transmission`; ``sum_n T_n`` agrees with ``transmission`` within its bound.  (2) ``T_n >= 0`` exactly and ``T_n
        <= 1`` within the bound; the entries beyond ``min(r_R, r_L)`` are exactly ``0.0``.  (3) Without a device potential and
        for ``Im z -> 0`` the number of ``T_n`` near 1 is the number of right-moving bands at ``Re z``.  (4) The bits of one
        ``(kp, z, sample)`` depend on nothing else: not on the other samples or their order, the points, the energies, the
        chunking or the grouping of the samples; the on-site form has the bits of the expanded matrices.  (5) The one-sided
        Jacobi keeps small ``T_n`` relatively accurate -- in the localised regime, where ``ln T`` is carried by one channel, an
        eigensolve of ``t^H t`` would bury the others under ``u T_max``.

        Error bound per ``T_n``, with ``eps`` and ``scale`` of :meth:`transmission``: ``(4 eps + (2 (N + 1)^2 + 8 N (sweeps + 2)
        + N^2) u) scale / N`` -- Weyl's bound for the four error-carrying factors, the backward error of the two Cholesky
        factors with the part dropped at the rank, and the Jacobi.

        Work: that of :meth:`transmission_ensemble`, and per sample ``2 N^3 / 3`` flops for the factors, ``16 N^3`` on the FP64
        matrix pipe for ``t`` and about ``18 N^3`` on the vector unit per Jacobi sweep, 5 to 20 sweeps; the closing costs
        about as much as the decimation and more than the sweep of a short device.  One workgroup owns a
        ``(kp, z, group of samples)`` from the first iteration to the last ``T_n``; the groups are chosen as in
        :meth:`transmission_ensemble`.  There is no route above 64 rows.  With several ``devices`` of the model the k list is
        split as for ``hamilton``.
        """
        if device is not None and devices is not None:
            raise ValueError("give device (one sample) or devices (an ensemble), not both")
        if devices is None:
            energies, axis_index, cap, k_array, layers, staged = self._device_arguments(k, z, axis, max_iterations, device, length,
                                                                                        "transmission_channels", 64)
            n_rows = self.size * layers
            staged = staged[None]
        else:
            energies, axis_index, cap, k_array, layers = self._stacking_arguments(k, z, axis, max_iterations)
            if layers == 0:
                raise ValueError("the model has no hopping along axis {}: there is nothing to transmit".format(axis_index))
            n_rows = self.size * layers
            if n_rows > 64:
                raise ValueError("a principal layer of {} cells has {} rows: transmission_channels takes at most 64".format(layers, n_rows))
            staged = self._ensemble_devices_argument(devices, n_rows)
        samples, count = staged.shape[:2]
        n_k, n_z = k_array.shape[0], energies.shape[0]
        iterations = np.zeros((n_k, n_z), dtype=np.int32)
        result = np.empty((n_k, n_z, samples), dtype=np.float64)
        channels = np.empty((n_k, n_z, samples, n_rows), dtype=np.float64)
        with self._call_lock:
            # the caps reached: TBK_ERR_NO_CONVERGENCE, a singular z - D: TBK_ERR_SINGULAR -> numpy.linalg.LinAlgError
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_transmission_channels_multi(handles, n_handles, axis_index, layers, _lib.ptr(k_array) if k_array.size else None, n_k,
                                                           count, samples, _lib.ptr(staged) if staged.ndim == 4 else None,
                                                           _lib.ptr(staged) if staged.ndim == 3 else None, n_z, _lib.ptr(energies), cap,
                                                           _lib.ptr(iterations), _lib.ptr(result), _lib.ptr(channels))
            )
        if devices is None:
            result, channels = result[:, :, 0], channels[:, :, 0]
        noise = (channels * (1.0 - channels)).sum(axis=-1)
        return TransmissionChannels(k_array, energies, layers, count, samples, iterations, result, channels, noise)

    def _device_arguments(self, k, z, axis, max_iterations, device, length, name, max_rows):
        """(energies, axis index, cap, in-plane k array, L, V as complex128 (M, N, N)) of `transmission` and `device_green_function`:
        `_stacking_arguments` and the device, given as ``device`` or as ``length`` pristine layers."""
        energies, axis_index, cap, k_array, layers = self._stacking_arguments(k, z, axis, max_iterations)
        if layers == 0:
            raise ValueError("the model has no hopping along axis {}: there is nothing to transmit".format(axis_index))
        n_rows = self.size * layers
        if n_rows > max_rows:
            raise ValueError("a principal layer of {} cells has {} rows: {} takes at most {}".format(layers, n_rows, name, max_rows))
        if device is None:
            try:
                count = int(length)
            except (TypeError, ValueError):
                raise ValueError("length must be an integer from 1 to 4096, got {!r}".format(length)) from None
            if count != length or not 1 <= count <= 4096:
                raise ValueError("length must be an integer from 1 to 4096, got {!r}".format(length))
            if count * n_rows * n_rows * 16 > 256 << 20:
                raise ValueError("a device of {} layers of {} rows takes more than 256 MiB".format(count, n_rows))
            potential = np.zeros((count, n_rows, n_rows), dtype=np.complex128)
        else:
            given = np.asarray(device)
            if given.ndim == 2 and given.shape[1] == n_rows and given.shape[0] >= 1:
                if np.iscomplexobj(given):
                    raise ValueError("on-site energies of shape (M, {}) must be real".format(n_rows))
                onsite = np.asarray(given, dtype=np.float64)
                potential = np.zeros((onsite.shape[0], n_rows, n_rows), dtype=np.complex128)
                index = np.arange(n_rows)
                potential[:, index, index] = onsite
            elif given.ndim == 3 and given.shape[0] >= 1 and given.shape[1:] == (n_rows, n_rows):
                potential = np.ascontiguousarray(given, dtype=np.complex128)
            else:
                raise ValueError("device must have shape (M, {0}, {0}) or (M, {0}) with M >= 1, got {1}".format(n_rows, given.shape))
            if not np.all(np.isfinite(potential.view(np.float64))):
                raise ValueError("device must be finite")
            if potential.shape[0] > 4096 or potential.nbytes > 256 << 20:
                raise ValueError("device has {} layers of {} rows: at most 4096 layers and 256 MiB".format(potential.shape[0], n_rows))
            size = float(np.abs(potential).max())
            skew = float(np.abs(potential - np.conj(np.transpose(potential, (0, 2, 1)))).max())
            if skew > 1e-12 * size:
                raise ValueError("device is not Hermitian: max|V - V^H| = {:.3e}".format(skew))
        return energies, axis_index, cap, k_array, layers, potential

    def device_green_function(self, k, z, *, axis=-1, device=None, length=1, max_iterations=64, green=False):
        """
        The layer-resolved Green's functions of the device of :meth:`transmission`: the local density of states per layer and
        orbital, the parts of it injected from the left and from the right lead, and the diagonal blocks of the resolvent, on the
        GPU.  Not in the reference.

        ``k``, ``z``, ``axis``, ``device``, ``length``, ``max_iterations`` and the error messages are those of
        :meth:`transmission`; ``H00``, ``H01``, ``N = size * L``, the decimation and the forward sweep with ``g_p``, ``D_p`` and
        ``T`` are its as well, unchanged down to the order of the operations.  Returns the named tuple ``(k, z, layers, length,
        iterations, transmission, ldos, left, right[, diagonal, first, last])``: ``ldos``, ``left`` and ``right`` are ``float64
        (NK, NZ, M, N)``; with ``green=True``, ``diagonal``, ``first`` and ``last`` hold ``G_p``, ``F_p`` and ``C_p`` as
        ``complex128 (NK, NZ, M, N, N)``.  Without it ``3 M N + 1`` doubles per ``(kp, z)`` leave the GPU.

        Definition.  With ``Q_p`` the ``P_p`` of :meth:`transmission`, per ``(kp, z)`` after its forward sweep::

            G_M = g_M,   C_M = g_M
            for p = M - 1 ... 1:    X = g_p H01,   Y = H01^H g_p
                                    G_p = g_p + (X G_{p+1}) Y          block (p, p) of the full resolvent
                                    C_p = X C_{p+1}                    block (p, M)
            F_1 = G_1;   F_p = G_p (H01^H Q_{p-1})  (1 < p < M);   F_M = Q_M  (M > 1)        block (p, 1)
            ldos[p, i]  = -Im G_p[i, i] / pi
            left[p, i]  = Re sum_j (F_p Gamma_L)[i, j] conj(F_p[i, j]) / (2 pi)
            right[p, i] = Re sum_j (C_p Gamma_R)[i, j] conj(C_p[i, j]) / (2 pi)

        Products are formed as bracketed; the order is part of the definition.  The cap of the decimation, a singular ``z - D_p``
        and a non-finite element of a ``g_p``, ``G_p``, ``F_p`` or ``C_p`` raise ``numpy.linalg.LinAlgError`` naming the k index
        and the energy.

        Properties.  (1) ``ldos - left - right = (Im z / pi) sum_q sum_j |G_pq[i, j]|^2``: it has the sign of ``Im z`` and vanishes
        as ``Im z -> 0``, where ``left + right`` is the whole density.  (2) With ``V = 0``, ``G_p`` is ``bulk`` of
        :meth:`surface_green_function` for every ``p``.  (3) ``first[:, :, M - 1]`` and ``transmission`` have the bits of
        ``transmission(..., green=True)``.  (4) The bits of one ``(kp, z)`` depend on nothing else: not on the other points or
        energies, their order, the chunking, or ``green``.

        Error bound per component of a block ``B`` of layer ``p``: ``E c(B) s(B)`` with ``E`` the ``eps`` of :meth:`transmission`,
        ``c`` the number of error-carrying factors behind ``B`` (``3 (M - p) + 1`` for ``G_p``, ``M - p + 1`` for ``C_p``, ``c(G_p)
        + p - 1`` for ``F_p``) and ``s`` the product of the 2-norms of the blocks ``B`` is formed from: ``s(G_p) = |g_p| + |X| |G_{p+1}|
        |Y|``, ``s(C_p) = |X| |C_{p+1}|``, ``s(F_p) = |G_p| |H01^H Q_{p-1}|``.

        Work: the decimation and ``40 N^3`` flops per layer of the forward sweep as for :meth:`transmission`, then eight products
        per layer of the backward sweep, ``64 N^3`` flops, all on the FP64 matrix pipe.  One workgroup owns a ``(kp, z)`` from the
        first iteration to the last output; the forward sweep leaves ``g_p`` and ``H01^H Q_{p-1}`` on a stack of ``2 M N^2`` complex
        numbers per workgroup in device memory, as many stacks as fit 1 GiB.  ``N`` is at most 64, else ``ValueError``: there is no
        library route, and a model with ``TBK_OPT_EIGENSOLVER = TBK_EIG_ROCSOLVER`` takes the own kernel too.  With several
        ``devices`` the k list is split as for ``hamilton``.
        """
        energies, axis_index, cap, k_array, layers, potential = self._device_arguments(k, z, axis, max_iterations, device, length,
                                                                                       "device_green_function", 64)
        n_rows = self.size * layers
        n_k, n_z, count = k_array.shape[0], energies.shape[0], potential.shape[0]
        iterations = np.zeros((n_k, n_z), dtype=np.int32)
        result = np.empty((n_k, n_z), dtype=np.float64)
        ldos, left, right = (np.empty((n_k, n_z, count, n_rows), dtype=np.float64) for _ in range(3))
        blocks = [np.empty((n_k, n_z, count, n_rows, n_rows), dtype=np.complex128) if green else None for _ in range(3)]
        with self._call_lock:
            # the cap reached: TBK_ERR_NO_CONVERGENCE, a singular z - D or a non-finite block: TBK_ERR_SINGULAR -> numpy.linalg.LinAlgError
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_device_green_multi(handles, n_handles, axis_index, layers, _lib.ptr(k_array) if k_array.size else None, n_k, count,
                                                  _lib.ptr(potential), n_z, _lib.ptr(energies), cap, _lib.ptr(iterations), _lib.ptr(result),
                                                  _lib.ptr(ldos), _lib.ptr(left), _lib.ptr(right), _lib.ptr(blocks[0]), _lib.ptr(blocks[1]),
                                                  _lib.ptr(blocks[2]))
            )
        if green:
            return DeviceGreenBlocks(k_array, energies, layers, count, iterations, result, ldos, left, right, blocks[0], blocks[1], blocks[2])
        return DeviceGreen(k_array, energies, layers, count, iterations, result, ldos, left, right)

    def device_current(self, k, z, *, axis=-1, device=None, length=1, max_iterations=64, bonds=False):
        """
        The bond currents of the device of :meth:`device_green_function`: per interface, orbital and, on request, bond, the current
        of the states injected from the left and from the right lead, on the GPU.  Not in the reference.

        ``k``, ``z``, ``axis``, ``device``, ``length``, ``max_iterations`` and the error messages are those of
        :meth:`transmission`; everything in front of the new lines is :meth:`device_green_function`, unchanged down to the order of
        the operations.  Returns the named tuple ``(k, z, layers, length, iterations, transmission, ldos, left, right, current_left,
        current_right[, inter_left, inter_right, intra_left, intra_right])``: ``current_left`` and ``current_right`` are ``float64
        (NK, NZ, M - 1, N)``, empty along that axis for ``M = 1``; with ``bonds=True``, ``inter_left`` and ``inter_right`` hold
        ``K`` as ``float64 (NK, NZ, M - 1, N, N)`` and ``intra_left`` and ``intra_right`` hold ``J`` as ``(NK, NZ, M, N, N)``.

        Definition.  With ``F_p``, ``C_p``, ``Gamma_L``, ``Gamma_R`` of :meth:`device_green_function` and ``H_pp = H00 + V_p``, per
        ``(kp, z)``::

            A^L_{p,q} = (F_p Gamma_L) F_q^H            A^R_{p,q} = (C_p Gamma_R) C_q^H
            K^L_p[i, j] = 2 Im(conj(H01[i, j]) A^L_{p,p+1}[i, j])    p = 1 ... M - 1   orbital i of layer p -> orbital j of layer p + 1
            J^L_p[i, j] = 2 Im(conj(H_pp[i, j]) A^L_{p,p}[i, j])     p = 1 ... M       orbital i -> orbital j inside layer p
            K^R, J^R: the same with A^R
            current_left[p, i] = sum_j K^L_p[i, j]     current_right[p, i] = sum_j K^R_p[i, j]

        in ``e / h`` per unit energy.  Products are formed as bracketed.  ``K^L`` flows towards the right lead (positive totals),
        ``K^R`` towards the left (negative totals); ``f_L K^L + f_R K^R`` is the kernel of a biased current.  A non-finite element of
        a ``K`` or ``J`` raises ``numpy.linalg.LinAlgError`` like one of a block.

        Properties, with the signed ``eta = Im z``.  (1) ``sum K^L_{p-1} - sum K^L_p = 4 pi eta sum_i left[p, i]`` for ``1 < p < M``
        and ``sum K^L_{M-1} - transmission = 4 pi eta sum_i left[M, i]``: the current is conserved as ``eta -> 0``, and every
        interface then carries ``transmission``.  (2) Per orbital ``j`` of an interior layer: ``sum_i K^L_{p-1}[i, j] - sum_k
        K^L_p[j, k] - sum_k J^L_p[j, k] = 4 pi eta left[p, j]``; the same with ``R`` and ``right``.  (3) ``sum K^R_{p-1} - sum K^R_p =
        4 pi eta sum_i right[p, i]``.  (4) ``K`` is exactly zero where ``H01`` is, ``J`` where ``H_pp`` is, and ``J`` is
        antisymmetric up to rounding (``H01`` and ``H00`` as the call takes them from Fourier sums of ``H(k)``: an absent hopping
        is zero there up to rounding).  (5) ``iterations``, ``transmission``, ``ldos``, ``left`` and ``right`` have the bits of
        :meth:`device_green_function`.  (6) The bits of one ``(kp, z)`` depend on nothing else: not on the other points or energies,
        their order, the chunking, ``bonds``, or the number of devices.

        Error bound per component, with ``E``, ``c`` and ``s`` of :meth:`device_green_function` and ``gamma_L = 2 |H01|^2 |G_top|``:
        ``2 max|H01| (c(F_p) + c(F_{p+1}) + 1) E s(F_p) s(F_{p+1}) gamma_L`` for ``K^L_p``, ``2 max|H_pp| (2 c(F_p) + 1) E s(F_p)^2
        gamma_L`` for ``J^L_p``, ``C`` and ``gamma_R`` for the right, ``N`` times ``K``'s for ``current_*``.

        Work: that of :meth:`device_green_function` and, per layer, two more products on the FP64 matrix pipe (four with
        ``bonds=True``, which forms ``J``), ``16 N^3`` (``32 N^3``) flops; ``F_p`` and ``C_p`` wait for the layer below in the
        stack's places of ``g_p`` and ``H01^H Q_{p-1}``, which are dead by then.  Without ``bonds``, ``2 (M - 1) N`` more doubles
        per ``(kp, z)`` leave the GPU; with it ``2 (2 M - 1) N^2`` more.  ``N`` is at most 64, else ``ValueError``.
        """
        energies, axis_index, cap, k_array, layers, potential = self._device_arguments(k, z, axis, max_iterations, device, length,
                                                                                       "device_current", 64)
        n_rows = self.size * layers
        n_k, n_z, count = k_array.shape[0], energies.shape[0], potential.shape[0]
        iterations = np.zeros((n_k, n_z), dtype=np.int32)
        result = np.empty((n_k, n_z), dtype=np.float64)
        ldos, left, right = (np.empty((n_k, n_z, count, n_rows), dtype=np.float64) for _ in range(3))
        rows = [np.empty((n_k, n_z, count - 1, n_rows), dtype=np.float64) for _ in range(2)]
        inter = [np.empty((n_k, n_z, count - 1, n_rows, n_rows), dtype=np.float64) if bonds else None for _ in range(2)]
        intra = [np.empty((n_k, n_z, count, n_rows, n_rows), dtype=np.float64) if bonds else None for _ in range(2)]
        with self._call_lock:
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_device_current_multi(handles, n_handles, axis_index, layers, _lib.ptr(k_array) if k_array.size else None, n_k, count,
                                                    _lib.ptr(potential), n_z, _lib.ptr(energies), cap, _lib.ptr(iterations), _lib.ptr(result),
                                                    _lib.ptr(ldos), _lib.ptr(left), _lib.ptr(right), _lib.ptr(rows[0]), _lib.ptr(rows[1]),
                                                    _lib.ptr(inter[0]), _lib.ptr(inter[1]), _lib.ptr(intra[0]), _lib.ptr(intra[1]))
            )
        plain = DeviceCurrent(k_array, energies, layers, count, iterations, result, ldos, left, right, rows[0], rows[1])
        if bonds:
            return DeviceCurrentBonds(*plain, inter[0], inter[1], intra[0], intra[1])
        return plain

    def susceptibility(self, mesh, q, *, temperature, energy=None, n_electrons=None, matrix_elements=True, convention=2):
        """
        The bare (Lindhard) static susceptibility ``chi_0(q)`` of a uniform k mesh, computed on the GPU from the eigensystem of
        the whole mesh, which never leaves it.  Not in the reference.

        ``mesh``, ``energy`` and ``n_electrons`` are those of :meth:`occupations`: exactly one of the last two is given, else
        ``ValueError``.  ``q`` is an integer array-like of shape ``(NQ, dim)`` or one vector, in mesh units: the wavevector is
        ``q_d / n_d``; any 64-bit integer and duplicates are allowed.  ``temperature`` is ``k_B T > 0`` in the model's energy
        units.  Returns the named tuple ``(mu, q, chi)``: ``mu`` is the :class:`FermiLevel` tuple of :meth:`occupations`, ``q``
        the vectors as ``int64 (NQ, dim)`` and ``chi`` is ``float64 (NQ,)``.

        Definition.  With ``E, U`` of ``eigh(k, convention=2)`` at the mesh points ``k = (i_1 / n_1, ..., i_dim / n_dim)`` and
        ``k+q`` the mesh point with the indices ``(i_d + q_d) mod n_d``::

            M(k, q)[b, b'] = sum_i conj(U[k, i, b]) D(q)[i] U[k+q, i, b']
            chi_0(q)       = -(1 / NK) sum_k sum_{b, b'} F(E[k, b], E[k+q, b']) |M(k, q)[b, b']|^2
            F(a, b)        = (f(a) - f(b)) / (a - b),   F(a, a) = f'(a),   f(x) = 1 / (1 + exp((x - mu) / T))

        ``D(q) = 1`` for ``convention=2``; for ``convention=1`` ``D(q)[i] = exp(-2 pi i sum_d q_d pos[i, d] / n_d)`` with the
        unreduced ``q_d`` (what ``U_1 = diag(exp(-2 pi i k . pos)) U_2`` gives).  ``matrix_elements=False`` sets ``|M|^2 = 1``,
        the constant-matrix-element Lindhard function; no eigenvector is computed then.  No spin factor; static only.

        ``mu`` is ``energy`` as given or, for ``n_electrons``, the tetrahedron Fermi level of :meth:`fermi_level`, bit for bit.
        The chemical potential of the Fermi function at ``temperature`` (which differs from it at finite ``T``) is not computed:
        give it as ``energy`` when it matters.

        ``F`` is not evaluated as the quotient, which cancels: with the pair ordered ``lo <= hi`` and ``y = (lo - hi) / T``,
        ``F = -f(lo) (1 - f(hi)) h(y) / T`` with ``h(y) = expm1(y) / y``, ``h(0) = 1``, ``f`` from ``exp(-|x - mu| / T)`` and
        ``1 - f(x)`` as ``f(2 mu - x)``: every factor is non-negative, nothing overflows, ``a = b`` is the same branch.

        Properties.  (1) ``chi_0(q) >= 0`` and ``chi_0(-q) = chi_0(q)``, both conventions.  (2) With matrix elements
        ``chi_0(0) = (1 / NK) sum_{k, b} f (1 - f) / T``, whatever the basis inside degenerate clusters.  (3) Without matrix
        elements the result is a function of the eigenvalues alone.  (4) ``4 T chi_0(q) -> size`` as ``T -> inf`` (the rows of
        ``M`` have unit norm).  (5) With ``mu`` 746 ``T`` or more below (or above) the spectrum every ``f`` (or ``1 - f``)
        underflows and ``chi_0`` is exactly 0.  (6) For ``convention=2`` ``q + n_d e_d`` has the bits of ``q``.  (7) The bits of
        ``chi_0(q)`` do not depend on the other entries of ``q``, on their order or on the number of ``devices``; a duplicate has
        the bits of its original and a second call the bits of the first.

        Error bound for a given eigensystem, with ``u = 2^-53`` and 2 ulps allowed for ``exp`` and ``expm1`` (DESIGN.md 15.4;
        ``tools/chi_model.py`` ``tolerance``); without matrix elements ``[NK size^4 / 2 + 20.5 size^2] u / T``::

            |error| <= [ NK size^3 / 2 + (3 size + 5) size^(3/2) + 22 size ] u / T

        One-dimensional models raise ``ValueError``.  The eigenvectors of the whole mesh must fit the device (``NK size^2``
        complex numbers), else ``MemoryError``.  With several ``devices`` every device holds the whole mesh's eigensystem and
        takes a contiguous share of ``q``.
        """
        mesh_array, vectors, t_value, mode, value, pos = self._susceptibility_arguments("susceptibility", mesh, q, temperature, energy, n_electrons,
                                                                                        matrix_elements, convention)
        mu = np.empty(4, dtype=np.float64)
        chi = np.empty(vectors.shape[0], dtype=np.float64)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_susceptibility_multi(handles, n_handles, _lib.ptr(mesh_array), mode, value, t_value, vectors.shape[0],
                                                    _lib.ptr(vectors), int(bool(matrix_elements)), int(convention), _lib.ptr(pos),
                                                    _lib.ptr(mu), _lib.ptr(chi))
            )
        return Susceptibility(FermiLevel(float(mu[0]), float(mu[1]), float(mu[2]), float(mu[3])), vectors, chi)

    @staticmethod
    def _positive_number_argument(value, name):
        """``float`` from a finite, positive real number or ``ValueError`` (``temperature``, ``eta``)."""
        if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise ValueError("{} must be a real number, got {!r}".format(name, value))
        number = float(value)
        if not np.isfinite(number) or not number > 0.0:
            raise ValueError("{} must be finite and positive, got {!r}".format(name, value))
        return number

    def _susceptibility_arguments(self, name, mesh, q, temperature, energy, n_electrons, matrix_elements, convention):
        """The checks ``susceptibility`` and ``dynamic_susceptibility`` share, in one order and one wording: ``(mesh int32 (dim,),
        q int64 (NQ, dim), temperature, mode, value, pos or None)`` or ``ValueError``."""
        mesh_array = self._mesh_argument(mesh, name)
        if q is None:
            raise ValueError("q must be an integer array of shape (NQ, {}), got None".format(self.dim))
        vectors = self._integer_vectors_argument(q, "q", "NQ")
        t_value, mode, value = self._thermal_arguments(name, temperature, energy, n_electrons)
        pos = self._convention_argument(convention)
        if not isinstance(matrix_elements, (bool, np.bool_)):
            raise ValueError("matrix_elements must be True or False, got {!r}".format(matrix_elements))
        return mesh_array, vectors, t_value, mode, value, pos

    def _thermal_arguments(self, name, temperature, energy, n_electrons):
        """``(temperature, mode, value)`` of the calls that weigh states with the Fermi function at one chemical potential."""
        t_value = self._positive_number_argument(temperature, "temperature")
        mode, value = self._occupation_argument(name, energy, n_electrons)
        return t_value, mode, value

    def _convention_argument(self, convention):
        """The positions the kernels take for ``convention=1``, ``None`` for ``convention=2``, else ``ValueError``."""
        if convention not in [1, 2]:
            raise ValueError("Invalid value '{}' for 'convention': must be either '1' or '2'".format(convention))
        return np.ascontiguousarray(self.pos, dtype=np.float64) if convention == 1 else None

    @staticmethod
    def _frequency_arguments(omega, eta):
        """The checks of ``omega`` and ``eta`` that ``dynamic_susceptibility``, ``dynamic_orbital_susceptibility`` and ``optical_conductivity`` share: ``(omega float64
        (NW,), eta)`` or ``ValueError``."""
        if omega is None or isinstance(omega, (str, bytes)):
            raise ValueError("omega must be a real number or a real array of shape (NW,), got {!r}".format(omega))
        try:
            frequencies = np.asarray(omega)
        except (TypeError, ValueError):
            raise ValueError("omega must be a real number or a real array of shape (NW,)") from None
        if frequencies.dtype.kind not in "iuf":
            raise ValueError("omega must hold real numbers, got dtype {}".format(frequencies.dtype))
        if frequencies.ndim == 0:
            frequencies = frequencies.reshape(1)
        if frequencies.ndim != 1 or frequencies.shape[0] < 1:
            raise ValueError("omega must have shape (NW,) with NW >= 1, got {}".format(frequencies.shape))
        frequencies = np.ascontiguousarray(frequencies, dtype=np.float64)
        if not np.all(np.isfinite(frequencies)):
            raise ValueError("omega must be finite")
        eta_value = Model._positive_number_argument(eta, "eta")
        if not eta_value * eta_value > 0.0:
            raise ValueError("eta must be finite and positive, got {!r} (its square underflows)".format(eta))
        return frequencies, eta_value

    def dynamic_susceptibility(self, mesh, q, omega, *, eta, temperature, energy=None, n_electrons=None, matrix_elements=True, convention=2):
        """
        The bare dynamic susceptibility ``chi_0(q, omega + i eta)`` of a uniform k mesh, computed on the GPU from the eigensystem
        of the whole mesh, which never leaves it.  Not in the reference.

        ``mesh``, ``q``, ``temperature``, ``energy``, ``n_electrons``, ``matrix_elements`` and ``convention`` are those of
        :meth:`susceptibility`, with the same errors.  ``omega`` is a real array-like of shape ``(NW,)`` with ``NW >= 1`` or one
        number: finite frequencies in the model's energy units, of any sign and order, duplicates allowed.  ``eta`` is one finite
        broadening ``> 0``.  Returns the named tuple ``(mu, q, omega, chi)``: ``mu`` and ``q`` as for :meth:`susceptibility`,
        ``omega`` as ``float64 (NW,)`` and ``chi`` as ``complex128 (NQ, NW)``.

        Definition.  With ``E``, ``U``, ``k+q``, ``M(k, q)`` and ``f`` of :meth:`susceptibility` and ``z = omega + i eta``::

            chi_0(q, z) = -(1 / NK) sum_k sum_{b, b'} (f(E[k, b]) - f(E[k+q, b'])) / (E[k, b] - E[k+q, b'] + z) |M(k, q)[b, b']|^2

        No spin factor; the sign is the static call's, so ``Re chi_0(q, i eta) -> chi_0(q)`` as ``eta -> 0`` except for the ``f'``
        terms of exactly degenerate pairs, which the dynamic function does not have.  ``mu`` is found as in
        :meth:`susceptibility`.

        The occupation difference is not formed as written: with the pair ordered ``lo <= hi`` and ``y = (lo - hi) / T``,
        ``f(lo) - f(hi) = f(lo) (1 - f(hi)) (-expm1(y)) >= 0`` from the static call's two tables -- nothing cancels, nothing
        overflows, equal energies give a zero -- and ``g`` is that value with the sign of the pair's order.  Per pair ``p = g |M|^2``
        and ``Delta = E[k, b] - E[k+q, b']`` are computed once; per frequency ``x = Delta + omega``, ``r = 1 / (x^2 + eta^2)``,
        ``Re chi -= p x r / NK``, ``Im chi += p eta r / NK``.  A frequency that hits a transition exactly (``x = 0``) is finite.

        Properties, both conventions.  (1) ``chi_0(-q, -omega + i eta) = conj chi_0(q, omega + i eta)``.  (2) ``0 <= Re chi_0(q, i
        eta) <= chi_0(q)`` of :meth:`susceptibility`: every term is the static term times ``Delta^2 / (Delta^2 + eta^2)``.  (3)
        ``omega [Im chi_0(q, omega + i eta) + Im chi_0(-q, omega + i eta)] >= 0``: the absorptive part has one sign, pair by pair
        (with this sign of ``chi_0``, ``Im chi_0 >= 0`` at positive frequencies where ``chi_0(-q) = chi_0(q)``).  (4) With matrix elements and ``convention=2``, ``chi_0(0, z) = 0``
        for every ``z``: no intraband response at ``q = 0``.  (5) With ``mu`` 746 ``T`` or more below or above the spectrum every
        entry is ``+0`` in both components.  (6) For ``convention=2`` ``q + n_d e_d`` has the bits of ``q``.  (7) The bits of
        ``chi_0(q, omega_j + i eta)`` do not depend on the other vectors or frequencies, on their order or on the number of
        ``devices``; duplicates have equal bits and a second call the bits of the first.

        Error bound of either component for a given eigensystem, with ``u = 2^-53``, ``S = size`` (``size^2`` without matrix
        elements), ``W`` the bandwidth and allowances of 2 for ``exp``, ``expm1`` and the quotient (DESIGN.md 16.4;
        ``tools/chi_model.py`` ``dynamic_tolerance``); without matrix elements the last bracket is absent::

            |error| <= 2 [ (NK size^2 + 34 + (2 W + |omega|) / eta) S + 2 (3 size + 5) size^(3/2) + 3 size ] u / eta

        The term ``(2 W + |omega|) / eta^2`` is the rounding of ``Delta + omega`` under the slope of the Lorentzian: it is why a
        broadening far below the level spacing of the mesh costs digits as well as meaning.

        One-dimensional models raise ``ValueError``.  The eigenvectors of the whole mesh must fit the device (``NK size^2``
        complex numbers), else ``MemoryError``.  The partial sums take ``16 NK ceil(size / 64)^2`` bytes per ``(q, omega)``; when
        one vector's do not fit 256 MiB the frequencies go in passes and the overlaps are computed again in each.  With several
        ``devices`` every device holds the whole mesh's eigensystem and takes a contiguous share of ``q`` with all frequencies.
        """
        mesh_array, vectors, t_value, mode, value, pos = self._susceptibility_arguments("dynamic_susceptibility", mesh, q, temperature, energy,
                                                                                        n_electrons, matrix_elements, convention)
        frequencies, eta_value = self._frequency_arguments(omega, eta)
        mu = np.empty(4, dtype=np.float64)
        chi = np.empty((vectors.shape[0], frequencies.shape[0]), dtype=np.complex128)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_dynamic_susceptibility_multi(handles, n_handles, _lib.ptr(mesh_array), mode, value, t_value, vectors.shape[0],
                                                            _lib.ptr(vectors), frequencies.shape[0], _lib.ptr(frequencies), eta_value,
                                                            int(bool(matrix_elements)), int(convention), _lib.ptr(pos), _lib.ptr(mu),
                                                            _lib.ptr(chi))
            )
        return DynamicSusceptibility(FermiLevel(float(mu[0]), float(mu[1]), float(mu[2]), float(mu[3])), vectors, frequencies, chi)

    def optical_conductivity(self, mesh, omega, *, eta, temperature, energy=None, n_electrons=None, convention=2, cartesian=False):
        """
        The Kubo optical (current-current) conductivity ``sigma[a, c](omega + i eta)`` of a uniform k mesh, computed on the GPU
        from the eigensystem and the derivative ``dH/dk`` of one chunk of the mesh at a time: the velocity matrices never leave
        the device.  Not in the reference.

        ``mesh``, ``temperature``, ``energy`` and ``n_electrons`` are those of :meth:`susceptibility`, ``omega`` and ``eta`` those
        of :meth:`dynamic_susceptibility`, all with the same errors.  Returns the named tuple ``(mu, omega, sigma)``: ``mu`` is the
        :class:`FermiLevel` tuple as in the susceptibilities (for ``n_electrons`` that of :meth:`fermi_level`, bit for bit),
        ``omega`` is ``float64 (NW,)`` and ``sigma`` is ``complex128 (NW, dim, dim)``.

        Definition.  Mesh points ``k = (i_1 / n_1, ..., i_dim / n_dim)``, ``E, U`` of ``eigh(k, convention=2)``; reduced
        coordinates, ``e = hbar = 1``, per unit cell, no spin factor::

            D^a(k)      = sum_R  i R_a exp(2 pi i k.R) hop[R]  +  h.c.          = (1 / 2 pi) dH/dk_a   (Hermitian, R = 0 drops out)
            V^a(k)      = U^H D^a U                                             convention 2
            V^a[b, b'] += i (E_b - E_b') (U^H diag(pos[:, a]) U)[b, b']         convention 1 only: the positions inside the cell
            w[b, b']    = -(f(E_b) - f(E_b')) / (E_b - E_b')  >= 0              equal energies give -f'(E): the Drude term is included
            sigma[a, c](omega) = (i / NK) sum_k sum_{b, b'} w[b, b'] V^a[b, b'] conj(V^c[b, b']) / (omega + i eta + E_b - E_b')

        ``w`` is evaluated as :meth:`susceptibility` evaluates ``-F``: from the two Fermi tables and one ``expm1``, nothing cancels.
        The convention-1 term is what differentiating the convention-1 Hamiltonian gives, rotated to the band basis.

        ``cartesian=True`` needs ``uc`` (else ``ValueError``) and returns ``uc^T sigma uc / |det uc|`` per frequency: the tensor
        along the Cartesian axes, per unit volume.  It is a host transform of the ``(NW, dim, dim)`` result.

        Properties, pair by pair and therefore up to the rounding of ``V``.  (1) ``sigma[a, c](-omega) = conj sigma[a, c](omega)``.
        (2) The Hermitian part ``(sigma + sigma^H) / 2`` over ``(a, c)`` is positive semidefinite at every ``omega``; in particular
        ``Re sigma[a, a] >= 0``.  (3) With ``mu`` 746 ``T`` or more outside the spectrum every entry is ``+0``.  (4) The bits of
        ``sigma(omega_j)`` do not depend on the other frequencies, their order or duplicates, on ``TBK_OPT_K_CHUNK``, on a second
        call or on the number of ``devices``: per-k partial sums are added in fixed groups of 256 consecutive mesh points in index
        order and the groups in index order, and devices take whole groups.  The chunk and the devices leave every bit alone for
        sparse models and for dense models on the matrix-vector H(k) kernel (up to 22 orbitals and fewer than 128 lattice vectors),
        whose walk stays in chunks of at most 4096 points; for a larger dense model chunks of up to 32 points and longer ones take
        different H(k) kernels, which differ in the last bit as :meth:`eigh`'s do.  (5) For a gapped 2-D model at low ``T`` and small
        ``eta``, ``2 pi sigma[0, 1](0)`` tends to the Chern number of the occupied bands as :meth:`berry_flux` returns it (QWZ model,
        12 x 12 mesh, ``eta = 0.05``, ``T = 0.02``: within 4.1e-4).

        Error bound of either component of an element for a given eigensystem and ``D^a``, with ``u = 2^-53``, ``G`` the largest
        Frobenius norm of a ``V^a(k)``, ``W`` the bandwidth and ``P`` = 2 (3 for ``convention=1``) matrix products (DESIGN.md 27.4;
        ``tools/optics_model.py`` ``tolerance``)::

            |error| <= [ NK size^2 + 58 + (2 W + |omega|) / eta + 2 P (2 size + 3) sqrt(size) ] G^2 u / (2 T eta)

        One-dimensional models raise ``ValueError``.  Dense and sparse models of every size :meth:`eigh` accepts; up to 64 orbitals
        one fused kernel rotates and contracts, above the products go through rocBLAS.  The partial sums take
        ``16 dim^2 NW NK`` bytes; when they do not fit 1 GiB (or a quarter of the free memory, if that is less) the frequencies go in passes and every
        pass computes the eigensystem and the derivatives of the mesh again.  With several ``devices`` each takes a contiguous share
        of the groups of mesh points with all frequencies.
        """
        mesh_array = self._mesh_argument(mesh, "optical_conductivity")
        frequencies, eta_value = self._frequency_arguments(omega, eta)
        t_value, mode, value = self._thermal_arguments("optical_conductivity", temperature, energy, n_electrons)
        pos = self._convention_argument(convention)
        if not isinstance(cartesian, (bool, np.bool_)):
            raise ValueError("cartesian must be True or False, got {!r}".format(cartesian))
        if cartesian and self.uc is None:
            raise ValueError("cartesian=True needs the unit cell: the model has no uc")
        mu = np.empty(4, dtype=np.float64)
        sigma = np.empty((frequencies.shape[0], self.dim, self.dim), dtype=np.complex128)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_optical_conductivity_multi(handles, n_handles, _lib.ptr(mesh_array), mode, value, t_value, frequencies.shape[0],
                                                          _lib.ptr(frequencies), eta_value, int(convention), _lib.ptr(pos), 0, _lib.ptr(mu),
                                                          _lib.ptr(sigma))
            )
        if cartesian:
            cell = np.asarray(self.uc, dtype=np.float64)
            sigma = np.einsum("ia,wij,jc->wac", cell, sigma, cell) / abs(np.linalg.det(cell))
        return OpticalConductivity(FermiLevel(float(mu[0]), float(mu[1]), float(mu[2]), float(mu[3])), frequencies, sigma)

    def _transport_scales(self):
        """The power-of-two scales ``s_g`` of the ``dim (dim + 1) / 2`` channels of :meth:`transport_distribution`, from the model
        alone: ``B_a = sum_R |R_a| ||hop[R]||_F`` over both halves of the lattice bounds ``||D^a(k)||_2``, so every row sum of
        ``|V^a|^2`` is at most ``B_a^2`` and every one of ``|V^a + V^c|^2`` at most ``(B_a + B_c)^2``; ``s_g`` is the power of two
        above 1.0000001 times that bound (1 when it is 0)."""
        bound = np.zeros(self.dim, dtype=np.float64)
        for key, mat in self._hop_items():
            norm = float(np.sqrt((np.abs(mat.data if self._sparse else mat) ** 2).sum()))
            bound += 2.0 * np.abs(np.array(key, dtype=np.float64)) * norm  # (the stored half and its conjugate)
        channel = [bound[a] ** 2 for a in range(self.dim)]
        channel += [(bound[a] + bound[c]) ** 2 for a in range(self.dim) for c in range(a + 1, self.dim)]
        return np.array([1.0 if b == 0.0 else float(np.ldexp(1.0, np.frexp(1.0000001 * b)[1])) for b in channel], dtype=np.float64)

    def transport_distribution(self, mesh, energies, *, degeneracy=1e-8, cartesian=False):
        """
        The transport distribution ``Sigma[a, c](E) = (1 / NK) sum_k sum_b v_a(k, b) v_c(k, b) delta(E - E_kb)`` of a uniform k mesh
        by the linear tetrahedron method, computed on the GPU from the eigensystem and ``dH/dk`` of one chunk of the mesh at a time:
        neither eigenvectors nor velocity matrices leave the device, ``dim (dim + 1) / 2 * NE`` doubles come back.  It is what
        Boltzmann transport in the relaxation-time approximation starts from (``tbmodels_amd.transport_coefficients``).  Not in
        the reference.

        ``mesh`` and ``energies`` are those of :meth:`dos`, with the same checks; the simplices, the half-open ranges and the stable
        sort are those of :meth:`dos` / :meth:`pdos`.  Returns the named tuple ``(energies, cumulative, tdf)``: ``cumulative`` is
        ``float64 (dim, dim, NE)``, ``int^E Sigma[a, c]`` at the grid energies, and ``tdf = diff(cumulative) / step`` (shape
        ``(dim, dim, NE - 1)``) belongs to the bin midpoints, like ``dos``.  Both are exactly symmetric in ``(a, c)``: ``a <= c`` is
        computed and the other half mirrored.

        Definition.  ``E, U`` of ``eigh(k, convention=2)``, ``D^a`` and ``V^a = U^H D^a U`` as in :meth:`optical_conductivity`;
        reduced coordinates, ``e = hbar = 1``, per unit cell, no spin factor::

            w[a, c](k, b) = Re sum_{b' : |E_kb - E_kb'| <= degeneracy}  V^a[b, b'] conj(V^c[b, b'])
            N[a, c](E)    = (1 / (S NK)) sum_simplices sum_b sum_corners  w_corner(E) w[a, c](corner, b)       = cumulative
            Sigma[a, c]   = diff(N[a, c]) / step

        For an isolated band ``w = v_a v_c``.  Inside a degenerate set the diagonal of ``V`` depends on the basis the eigensolver
        returns (see :meth:`eigh`); the sum of ``w`` over the set, ``Re tr(P V^a P V^c)``, does not -- the statement :meth:`pdos`
        makes about ``A_g``.  The pair criterion is the plain comparison of the doubles, not chained into clusters;
        ``degeneracy`` (energy units, ``>= 0`` and finite) is its threshold.  There is no ``convention`` argument: the term that
        convention 1 adds to ``V^a[b, b']`` carries the factor ``(E_b - E_b')``, which vanishes on the pairs that enter (up to
        ``degeneracy`` times a position, far below the rounding of ``V``), so both conventions give the same ``w``.

        ``cartesian=True`` needs ``uc`` (else ``ValueError``) and returns ``uc^T N uc / |det uc|`` per energy, a host transform, as
        in :meth:`optical_conductivity`.

        The device integrates ``dim (dim + 1) / 2`` non-negative channels -- ``sum |V^a|^2`` and, for ``a < c``,
        ``sum |V^a + V^c|^2`` -- each divided by a power of two derived from the hoppings alone, in the 64-bit fixed point of
        :meth:`pdos`; ``N[a, c] = (N+[a, c] - N[a, a] - N[c, c]) / 2`` is formed on the host.  The bits do not depend on a second call
        nor, for sparse models and dense models on the matrix-vector H(k) kernel, on ``TBK_OPT_K_CHUNK`` or the ``devices``.
        Error bound: DESIGN.md section 30 (``tools/tdf_model.py`` ``tolerance``).  One-dimensional models raise ``ValueError``;
        :class:`KdotpModel` has no Brillouin zone and no such method.
        """
        mesh_array, grid, step = self._dos_arguments(mesh, energies)
        if isinstance(degeneracy, (bool, np.bool_)) or not isinstance(degeneracy, (int, float, np.integer, np.floating)):
            raise ValueError("degeneracy must be a real number, got {!r}".format(degeneracy))
        threshold = float(degeneracy)
        if not np.isfinite(threshold) or threshold < 0.0:
            raise ValueError("degeneracy must be finite and >= 0, got {!r}".format(degeneracy))
        if not isinstance(cartesian, (bool, np.bool_)):
            raise ValueError("cartesian must be True or False, got {!r}".format(cartesian))
        if cartesian and self.uc is None:
            raise ValueError("cartesian=True needs the unit cell: the model has no uc")
        dim = self.dim
        scale = self._transport_scales()
        channels = np.empty((scale.shape[0], grid.shape[0]), dtype=np.float64)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_transport_distribution_multi(handles, n_handles, _lib.ptr(mesh_array), float(grid[0]), step, grid.shape[0],
                                                            threshold, _lib.ptr(scale), _lib.ptr(channels))
            )
        total = np.empty((dim, dim, grid.shape[0]), dtype=np.float64)
        pair = dim
        for a in range(dim):
            total[a, a] = channels[a]
            for c in range(a + 1, dim):
                total[a, c] = (channels[pair] - channels[a] - channels[c]) / 2.0
                total[c, a] = total[a, c]
                pair += 1
        if cartesian:
            cell = np.asarray(self.uc, dtype=np.float64)
            total = np.einsum("ia,ijw,jc->acw", cell, total, cell) / abs(np.linalg.det(cell))
            total = (total + total.transpose(1, 0, 2)) / 2.0  # (the transform of a symmetric tensor, symmetric to the bit again)
        return TransportDistribution(grid, total, np.diff(total, axis=2) / step)

    def _orbital_selection_argument(self, orbitals):
        """The checks of ``orbitals`` that ``orbital_susceptibility``, ``dynamic_orbital_susceptibility`` and ``susceptibility_tensor`` share: ``int64 (m,)`` distinct
        indices in ``[0, size)`` in the caller's order (``None``: all of them in order) or ``ValueError``."""
        if orbitals is None:
            selected = np.arange(self.size, dtype=np.int64)
        else:
            if isinstance(orbitals, (str, bytes)):
                raise ValueError("orbitals must be an integer array of shape (m,), got {!r}".format(orbitals))
            try:
                selected = np.asarray(orbitals)
            except (TypeError, ValueError):
                raise ValueError("orbitals must be an integer array of shape (m,)") from None
            if selected.dtype.kind not in "iu" or selected.dtype == np.uint64:
                raise ValueError("orbitals must hold (64-bit signed) integers, got dtype {}".format(selected.dtype))
            if selected.ndim == 0:
                selected = selected.reshape(1)
            if selected.ndim != 1 or selected.shape[0] < 1:
                raise ValueError("orbitals must have shape (m,) with m >= 1, got {}".format(selected.shape))
            selected = np.ascontiguousarray(selected, dtype=np.int64)
            if selected.min() < 0 or selected.max() >= self.size:
                raise ValueError("orbitals must lie in [0, {}), got {}".format(self.size, selected.tolist()))
            if np.unique(selected).shape[0] != selected.shape[0]:
                raise ValueError("orbitals must be distinct, got {}".format(selected.tolist()))
        return selected

    def orbital_susceptibility(self, mesh, q, *, temperature, energy=None, n_electrons=None, orbitals=None, convention=2):
        """
        The orbital-resolved bare static susceptibility ``chi_0[i, j](q)`` of a uniform k mesh -- the response of the density on
        orbital ``i`` to a field on orbital ``j``, what a multi-orbital RPA or a Stoner criterion per orbital starts from --
        computed on the GPU from the eigensystem of the whole mesh, which never leaves it.  Not in the reference.

        ``mesh``, ``q``, ``temperature``, ``energy``, ``n_electrons`` and ``convention`` are those of :meth:`susceptibility`, with
        the same errors; the eigenvectors are always used.  ``orbitals`` selects ``m`` distinct orbital indices in
        ``[0, size)``, in any order (an integer array-like of shape ``(m,)`` or one index); ``None`` means all of them in order.
        Returns the named tuple ``(mu, q, orbitals, chi)``: ``mu`` and ``q`` as for :meth:`susceptibility`, ``orbitals`` as
        ``int64 (m,)`` and ``chi`` as ``complex128 (NQ, m, m)`` in the order of ``orbitals``.

        Definition.  With ``E``, ``U``, ``k+q``, ``D(q)`` and ``f`` of :meth:`susceptibility` and
        ``t = f(lo) (1 - f(hi)) h(y) >= 0`` its pair weight (``-T F``)::

            A(k, q)[i; b, b'] = conj(U[k, i, b]) D(q)[i] U[k+q, i, b']
            chi_0[i, j](q)    = (1 / (T NK)) sum_k sum_{b, b'} t(E[k, b], E[k+q, b']) A[i; b, b'] conj(A[j; b, b'])

        No spin factor; static only.  ``sum_i A[i; b, b'] = M(k, q)[b, b']``, so the sum of all entries is ``chi_0(q)`` of
        :meth:`susceptibility`.

        Properties.  (1) ``chi_0(q)`` is Hermitian and positive semidefinite; the output is exactly Hermitian: entries with
        ``i <= j`` (in ascending orbital order) are computed, the others are their conjugates, and the diagonal's imaginary part is
        ``+0``.  (2) ``sum_ij chi_0[i, j](q) = chi_0(q)``.  (3) ``chi_0(-q) = chi_0(q)^T``.  (4) ``4 T chi_0(q) -> 1`` (the unit
        matrix) as ``T -> inf``.  (5) With ``mu`` 746 ``T`` or more outside the spectrum every entry is ``+0`` in both components.
        (6) For ``convention=2`` ``q + n_d e_d`` has the bits of ``q``.  (7) ``chi_0`` does not depend on the phases of the
        eigenvectors or on the basis inside degenerate clusters.  (8) The bits of ``chi_0[i, j](q)`` do not depend on the other
        entries of ``q``, on their order or on the number of ``devices``; a second call gives the bits of the first.  (9) A
        selection returns the bits of the same entries of the full matrix, whatever else is selected and in whatever order.

        Error bound of either component of an entry for a given eigensystem, with ``u = 2^-53`` and 2 ulps allowed for ``exp`` and
        ``expm1`` (``tools/chi_model.py`` ``orbital_tolerance``)::

            |error| <= [ NK size^2 / 2 + 27.5 ] u / T

        The work is ``8 size^2 m^2`` flops per ``(k, q)`` on the FP64 matrix pipe.  One-dimensional models raise ``ValueError``.
        The eigenvectors of the whole mesh must fit the device, else ``MemoryError``.  With several ``devices`` every device holds
        the whole mesh's eigensystem and takes a contiguous share of ``q``.
        """
        mesh_array, vectors, t_value, mode, value, pos = self._susceptibility_arguments("orbital_susceptibility", mesh, q, temperature, energy,
                                                                                        n_electrons, True, convention)
        selected = self._orbital_selection_argument(orbitals)
        chosen = np.ascontiguousarray(selected, dtype=np.int32)
        mu = np.empty(4, dtype=np.float64)
        chi = np.empty((vectors.shape[0], chosen.shape[0], chosen.shape[0]), dtype=np.complex128)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_orbital_susceptibility_multi(handles, n_handles, _lib.ptr(mesh_array), mode, value, t_value, vectors.shape[0],
                                                            _lib.ptr(vectors), chosen.shape[0], _lib.ptr(chosen), int(convention), _lib.ptr(pos),
                                                            _lib.ptr(mu), _lib.ptr(chi))
            )
        return OrbitalSusceptibility(FermiLevel(float(mu[0]), float(mu[1]), float(mu[2]), float(mu[3])), vectors, selected, chi)

    def dynamic_orbital_susceptibility(self, mesh, q, omega, *, eta, temperature, energy=None, n_electrons=None, orbitals=None, convention=2):
        """
        The orbital-resolved bare dynamic susceptibility ``chi_0[i, j](q, omega + i eta)`` of a uniform k mesh -- what a
        multi-orbital RPA needs once it leaves ``omega = 0``: spin-excitation spectra, orbital-resolved loss functions, the dynamic
        vertex ``(1 - chi_0 U)^-1 chi_0`` -- computed on the GPU from the eigensystem of the whole mesh, which never leaves it.  Not
        in the reference.

        ``mesh``, ``q``, ``temperature``, ``energy``, ``n_electrons`` and ``convention`` are those of :meth:`susceptibility`,
        ``omega`` and ``eta`` those of :meth:`dynamic_susceptibility`, ``orbitals`` that of :meth:`orbital_susceptibility`, all with
        the same errors; at most 65535 frequencies per call.  Returns the named tuple ``(mu, q, omega, orbitals, chi)``: ``mu``,
        ``q``, ``omega`` and ``orbitals`` as for those calls and ``chi`` as ``complex128 (NQ, NW, m, m)`` in the order of
        ``orbitals``.

        Definition.  With ``A`` of :meth:`orbital_susceptibility`, ``g = f(E[k, b]) - f(E[k+q, b'])`` and ``z = omega + i eta`` of
        :meth:`dynamic_susceptibility`::

            A(k, q)[i; b, b']  = conj(U[k, i, b]) D(q)[i] U[k+q, i, b']
            chi_0[i, j](q, z)  = -(1 / NK) sum_k sum_{b, b'} g / (E[k, b] - E[k+q, b'] + z) A[i; b, b'] conj(A[j; b, b'])

        No spin factor; the sign is that of the other susceptibilities.  ``g`` is evaluated without cancellation as in
        :meth:`dynamic_susceptibility`; per pair ``g`` and ``Delta = E[k, b] - E[k+q, b']`` are computed once, per frequency
        ``x = Delta + omega``, ``r = 1 / (x^2 + eta^2)``, ``c = (g r x, -(g r eta))``, and ``chi = (0 - sum c A conj(A)) / NK`` per
        component.  A frequency that hits a transition exactly (``x = 0``) is finite.  The matrix is not Hermitian --
        ``chi_0 = -(H_r + i H_i) / NK`` with two different Hermitian parts -- so all ``m^2`` entries are computed, as one
        complex-weighted product on the FP64 matrix pipe.

        Properties, with ``Herm(M) = (M + M^H) / 2`` and ``B(M) = (M - M^H) / (2i)``.  (1) ``chi_0[i, j](-q, -omega + i eta) = conj
        chi_0[i, j](q, omega + i eta)``.  (2) ``sum_ij chi_0[i, j](q, z)`` is ``chi_0(q, z)`` of :meth:`dynamic_susceptibility` with
        matrix elements.  (3) ``Herm chi_0(q, i eta)`` and ``orbital_susceptibility(q) - Herm chi_0(q, i eta)`` are positive
        semidefinite.  (4) ``omega [B(chi_0(q, omega + i eta)) + B(chi_0(-q, omega + i eta))^T]`` is positive semidefinite and
        exactly 0 at ``omega = 0``.  (5) With ``mu`` 746 ``T`` or more outside the spectrum every entry is ``+0`` in both
        components.  (6) For ``convention=2`` ``q + n_d e_d`` has the bits of ``q``.  (7) ``chi_0`` does not depend on the phases of
        the eigenvectors or on the basis inside degenerate clusters.  (8) The bits of ``chi_0[i, j](q, omega_j)`` do not depend on
        the other vectors or frequencies, on their order or on the number of ``devices``; duplicates have equal bits and a second
        call the bits of the first.  (9) A selection returns the bits of the same entries of the full matrix, whatever else is
        selected and in whatever order.

        Error bound of either component of an entry for a given eigensystem, with ``u = 2^-53``, ``W`` the bandwidth and allowances
        of 2 for ``exp``, ``expm1`` and the quotient (``tools/chi_model.py`` ``dynamic_orbital_tolerance``)::

            |error| <= 2 [ NK size^2 + 51 + (2 W + |omega|) / eta ] u / eta

        The work is ``8 size^2 m^2`` flops per ``(k, q, omega)``.  One-dimensional models raise ``ValueError``.  The eigenvectors of
        the whole mesh must fit the device, else ``MemoryError``.  The partial sums take ``16 slices m'^2`` bytes per ``(q,
        omega)`` (``m'``: ``m`` padded to 16, above 16 to 64); when one vector's do not fit 256 MiB the frequencies go in passes and
        the update is computed again in each.  With several ``devices`` every device holds the whole mesh's eigensystem and takes a
        contiguous share of ``q`` with all frequencies.
        """
        mesh_array, vectors, t_value, mode, value, pos = self._susceptibility_arguments("dynamic_orbital_susceptibility", mesh, q, temperature,
                                                                                        energy, n_electrons, True, convention)
        frequencies, eta_value = self._frequency_arguments(omega, eta)
        selected = self._orbital_selection_argument(orbitals)
        if frequencies.shape[0] > 65535:
            raise ValueError("dynamic_orbital_susceptibility takes up to 65535 frequencies per call, got {}".format(frequencies.shape[0]))
        chosen = np.ascontiguousarray(selected, dtype=np.int32)
        mu = np.empty(4, dtype=np.float64)
        chi = np.empty((vectors.shape[0], frequencies.shape[0], chosen.shape[0], chosen.shape[0]), dtype=np.complex128)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_dynamic_orbital_susceptibility_multi(handles, n_handles, _lib.ptr(mesh_array), mode, value, t_value,
                                                                    vectors.shape[0], _lib.ptr(vectors), frequencies.shape[0],
                                                                    _lib.ptr(frequencies), eta_value, chosen.shape[0], _lib.ptr(chosen),
                                                                    int(convention), _lib.ptr(pos), _lib.ptr(mu), _lib.ptr(chi))
            )
        return DynamicOrbitalSusceptibility(FermiLevel(float(mu[0]), float(mu[1]), float(mu[2]), float(mu[3])), vectors, frequencies, selected,
                                            chi)

    def susceptibility_tensor(self, mesh, q, *, temperature, energy=None, n_electrons=None, orbitals=None):
        """
        The four-index bare static susceptibility ``chi_0[i, l; j, m](q)`` of a uniform k mesh -- the full particle-hole bubble a
        multi-orbital RPA with Hund's coupling and pair hopping (the Kanamori ``U, U', J, J'`` vertices) starts from, of which
        :meth:`orbital_susceptibility` returns the density-density block ``i = l, j = m`` -- computed on the GPU from the
        eigensystem of the whole mesh, which never leaves it.  Not in the reference.

        ``mesh``, ``q``, ``temperature``, ``energy`` and ``n_electrons`` are those of :meth:`susceptibility`, ``orbitals`` that of
        :meth:`orbital_susceptibility` with ``1 <= m <= 16``, all with the same errors; more than 16 selected orbitals (or a model
        of more than 16 with ``orbitals=None``) raise ``ValueError``.  Returns the named tuple ``(mu, q, orbitals, chi)``: ``mu``
        and ``q`` as for :meth:`susceptibility`, ``orbitals`` as ``int64 (m,)`` and ``chi`` as ``complex128 (NQ, m, m, m, m)``
        indexed ``[q, i, l, j, m]`` in the order of ``orbitals``.

        Definition.  With ``E``, ``U`` (``eigh(k, convention=2)``), ``k+q`` and the pair weight ``t = f(lo) (1 - f(hi)) h(y) >= 0``
        (``-T F``) of :meth:`orbital_susceptibility`::

            chi_0[i, l; j, m](q) = (1 / (T NK)) sum_k sum_{b, b'} t(E[k, b], E[k+q, b'])
                                   conj(U[k, i, b]) U[k+q, l, b'] U[k, j, b] conj(U[k+q, m, b'])

        No spin factor; static only; the sign is that of :meth:`susceptibility`.  In the notation of Graser, Maier, Hirschfeld and
        Scalapino (New J. Phys. 11, 025016 (2009), eq. 5), whose numerator is ``a_mu^{l4}(k) a_mu^{l2*}(k) a_nu^{l1}(k+q)
        a_nu^{l3*}(k+q)``, this is ``chi_{l1 l2 l3 l4}`` with ``l2 = i, l1 = l, l4 = j, l3 = m``:
        ``chi_{l1 l2 l3 l4}(q) = chi[q, l2, l1, l4, l3]``, or ``numpy.transpose(chi, (0, 2, 1, 4, 3))`` indexed ``[q, l1, l2,
        l3, l4]``.

        Convention.  There is no ``convention`` argument: the tensor is that of the lattice-periodic gauge (convention 2), in which
        RPA codes work.  In convention 1 the pair amplitude ``conj(U[k, i, b]) U[k+q, l, b']`` carries ``exp(2 pi i k.(pos_i -
        pos_l))``, which depends on ``k`` whenever ``i != l`` and does not leave the k sum as a table ``D(q)``: that tensor is another
        operator (bond densities at the true positions).  On the block ``i = l, j = m`` the k dependence cancels and
        ``orbital_susceptibility(convention=1).chi[q, i, j] = D(q)[i] conj(D(q)[j]) chi[q, i, i, j, j]`` with ``D(q)[i] =
        exp(-2 pi i sum_d q_d pos[i, d] / n_d)``.

        Properties.  (1) As an ``m^2 x m^2`` matrix with rows ``(i, l)`` and columns ``(j, m)`` ``chi_0(q)`` is Hermitian and
        positive semidefinite; the output is exactly Hermitian: entries with ``(i, l) <= (j, m)`` (ascending orbital order) are
        computed, the others are their conjugates with the imaginary part formed as ``0 - x`` (no ``-0``), and the diagonal's
        imaginary part is ``+0``.  (2) ``chi_0[i, i; j, j](q)`` is ``chi_0[i, j](q)`` of :meth:`orbital_susceptibility` and (3)
        ``sum_ij chi_0[i, i; j, j](q)`` is ``chi_0(q)`` of :meth:`susceptibility`, each within the sum of the two bounds (the
        summation orders differ).  (4) ``chi_0(-q)[i, l; j, m] = chi_0(q)[m, j; l, i]``.  (5) ``4 T chi_0[i, l; j, m](q) ->
        delta_ij delta_lm`` as ``T -> inf``.  (6) With ``mu`` 746 ``T`` or more outside the spectrum every entry is ``+0`` in both
        components.  (7) ``q + n_d e_d`` has the bits of ``q``.  (8) ``chi_0`` does not depend on the phases of the eigenvectors
        or on the basis inside degenerate clusters.  (9) The bits of an entry do not depend on the other entries of ``q``, on
        their order or on the number of ``devices``; a second call gives the bits of the first.  (10) A selection returns the
        bits of the same entries of any other selection that holds their orbitals, in whatever order.

        Error bound of either component of an entry for a given eigensystem, with ``u = 2^-53`` and 2 ulps allowed for ``exp`` and
        ``expm1`` (``tools/chi_model.py`` ``tensor_tolerance``)::

            |error| <= [ NK size^2 / 2 + 25.5 ] u / T

        The kernels use the factorised form: per ``(k, b)`` ``P[i, j] = conj(U[k, i, b]) U[k, j, b]`` and ``Q[l, m] = sum_b' t
        U[k+q, l, b'] conj(U[k+q, m, b'])``, ``chi_0 = sum P Q / (T NK)``: about ``4 size m^4`` flops per ``(k, q)`` on the FP64
        matrix pipe instead of the ``8 size^2 m^4`` of the definition.  One-dimensional models raise ``ValueError``.  The
        eigenvectors of the whole mesh must fit the device, else ``MemoryError``.  With several ``devices`` every device holds the
        whole mesh's eigensystem and takes a contiguous share of ``q``.  Sparse models go through the same call.
        """
        mesh_array, vectors, t_value, mode, value, _ = self._susceptibility_arguments("susceptibility_tensor", mesh, q, temperature, energy,
                                                                                      n_electrons, True, 2)
        selected = self._orbital_selection_argument(orbitals)
        if selected.shape[0] > 16:
            raise ValueError("susceptibility_tensor takes up to 16 selected orbitals, got {}".format(selected.shape[0]))
        chosen = np.ascontiguousarray(selected, dtype=np.int32)
        m = chosen.shape[0]
        mu = np.empty(4, dtype=np.float64)
        chi = np.empty((vectors.shape[0], m, m, m, m), dtype=np.complex128)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_susceptibility_tensor_multi(handles, n_handles, _lib.ptr(mesh_array), mode, value, t_value, vectors.shape[0],
                                                           _lib.ptr(vectors), m, _lib.ptr(chosen), _lib.ptr(mu), _lib.ptr(chi))
            )
        return SusceptibilityTensor(FermiLevel(float(mu[0]), float(mu[1]), float(mu[2]), float(mu[3])), vectors, selected, chi)

    def _band_sets_argument(self, bands):
        """``int32 (S, 2)`` half-open band ranges from an int ``n_occ`` (``[(0, n_occ)]``) or a sequence of ``(lo, hi)`` pairs, or
        ``ValueError``."""
        def whole(value):
            return isinstance(value, (int, np.integer)) and not isinstance(value, (bool, np.bool_))

        if whole(bands):
            pairs = [(0, int(bands))]
        else:
            try:
                pairs = [tuple(pair) for pair in bands]
            except TypeError:
                raise ValueError("bands must be an integer or a sequence of (lo, hi) pairs, got {!r}".format(bands)) from None
        if not 1 <= len(pairs) <= 16:
            raise ValueError("bands must hold 1 to 16 band sets, got {}".format(len(pairs)))
        for pair in pairs:
            if len(pair) != 2 or not whole(pair[0]) or not whole(pair[1]):
                raise ValueError("a band set must be a pair of integers (lo, hi), got {!r}".format(pair))
            if pair[0] < 0 or pair[1] > self.size or pair[0] >= pair[1]:
                raise ValueError("a band set must satisfy 0 <= lo < hi <= {}, got {!r}".format(self.size, pair))
        return np.ascontiguousarray(np.array(pairs, dtype=np.int32).reshape(len(pairs), 2))

    def berry_flux(self, mesh, bands, *, convention=2):
        """
        The lattice Berry flux (the Fukui-Hatsugai-Suzuki field strength) of band sets on a uniform k mesh and their Chern numbers,
        computed on the GPU from the eigenvectors of the whole mesh, which never leave it.  Not in the reference.

        ``mesh`` is that of :meth:`occupations`.  ``bands`` is an int ``n_occ``, meaning the set ``[(0, n_occ)]``, or a sequence of 1
        to 16 half-open ranges ``(lo, hi)`` of ascending band indices with ``0 <= lo < hi <= size``.  Returns the named tuple
        ``(bands, planes, flux, chern, link_min)``: ``bands`` the sets as ``int32 (S, 2)``, ``planes`` the tuple of axis pairs
        ``((0, 1),)`` in two and ``((0, 1), (0, 2), (1, 2))`` in three dimensions, ``flux`` ``float64 (S, P, *mesh)``, ``chern`` a
        tuple of ``P`` arrays ``int64 (S, n_c)`` with ``c`` the axis the plane leaves over (``n_c = 1`` in two dimensions) and
        ``link_min`` ``float64 (S,)``.

        Definition.  With ``U`` of ``eigh(k, convention=2)`` at the mesh points ``k = (i_1 / n_1, ..., i_dim / n_dim)``, ``k+e_d`` the
        mesh point with index ``(i_d + 1) mod n_d`` on axis ``d`` and ``m = hi - lo``::

            M_d(k)     = U[k][:, lo:hi]^H D(e_d) U[k+e_d][:, lo:hi]                    (m x m)
            L_d(k)     = det M_d(k)
            a_d(k)     = round(arg L_d(k) / (2 pi) * 2^64) mod 2^64                    a uint64 "angle word"; arg 0 = 0 for L = 0
            F_ab(k)    = a_a(k) + a_b(k+e_a) - a_a(k+e_b) - a_b(k)                     wrapping 64-bit arithmetic, read as int64; a < b
            flux_ab(k) = float(F_ab(k)) * (2 pi 2^-64)                                 in [-pi, pi]
            C_ab(i_c)  = (sum over the plane's k of F_ab(k)) / 2^64
            link_min   = min over d and k of |L_d(k)|

        ``D(e_d) = 1`` for ``convention=2``; for ``convention=1`` ``D(e_d)[i] = exp(-2 pi i pos[i, d] / n_d)``, the table of
        :meth:`susceptibility` for ``q = e_d``.  The determinant comes from an LU factorisation with partial pivoting (the pivot is the
        largest ``|Re| + |Im|``, a tie goes to the lowest row).  Sign: ``flux_ab ~ -Omega_ab / (n_a n_b)`` with the Berry curvature
        ``Omega_ab = d_a A_b - d_b A_a`` of ``A_d = i tr <u| d/dk_d |u>``, so ``C_ab = -(1 / 2 pi) int Omega_ab``: the lower band of
        the Qi-Wu-Zhang model ``sin K_x sigma_x + sin K_y sigma_y + (u + cos K_x + cos K_y) sigma_z`` has ``C = +1`` for
        ``0 < u < 2``.

        Properties.  (1) Only the link angles carry rounding: every plaquette is an exact wrapped integer sum of four words, and
        the plaquettes of a closed plane add up to an exact multiple of ``2^64`` (the low word of the 128-bit sum is identically
        zero), so every Chern number is an integer without rounding, whatever the phases of the eigenvectors and whatever basis the
        eigensolver chooses inside the set.  (2) The Chern numbers do not change under a unitary mixing of the set's bands at every
        ``k``; the fluxes move by at most four links' rounding.  (3) The full set ``(0, size)`` has ``|L| = 1``, zero Chern numbers and
        fluxes of rounding size.  (4) Both conventions give the same Chern numbers.  (5) The bits of a set's links, fluxes and Chern
        numbers do not depend on the other sets, on their order or on the number of ``devices``; a duplicate has the bits of its
        original and a second call the bits of the first.

        Error bound of one link angle in radians for a given eigensystem, with ``u = 2^-53`` and ``sigma_min`` the smallest singular
        value of ``M`` (``tools/berry_model.py`` ``link_tolerance``); a flux carries four of these::

            |error| <= ((size + 8 m) m / sigma_min + 8) u

        Caveats.  The Chern number is that of the lattice field: it equals the continuum one when every ``|flux| < pi`` by a margin,
        which a finer mesh provides.  A small ``link_min`` means the mesh is too coarse or the set is not isolated from its
        neighbours.  A set whose edge cuts a degenerate cluster (``E[k, lo - 1] = E[k, lo]`` or ``E[k, hi - 1] = E[k, hi]`` at a mesh
        point) has ill-defined links there, since the basis inside the cluster is unspecified (see :meth:`eigh`): ``link_min`` shows
        it.  Degeneracies inside a set do no harm.

        One-dimensional models raise ``ValueError``.  The eigenvectors of the whole mesh must fit the device (``NK size^2`` complex
        numbers), else ``MemoryError``.  With several ``devices`` every device holds the whole mesh's eigenvectors and computes the
        links of a contiguous share of the mesh points.
        """
        mesh_array = self._mesh_argument(mesh, "berry_flux")
        sets = self._band_sets_argument(bands)
        if convention not in [1, 2]:
            raise ValueError("Invalid value '{}' for 'convention': must be either '1' or '2'".format(convention))
        pos = np.ascontiguousarray(self.pos, dtype=np.float64) if convention == 1 else None
        shape = tuple(int(n) for n in mesh_array)
        planes = ((0, 1),) if self.dim == 2 else ((0, 1), (0, 2), (1, 2))
        counts = [1] if self.dim == 2 else [shape[2], shape[1], shape[0]]
        n_sets = sets.shape[0]
        flux = np.empty((n_sets, len(planes)) + shape, dtype=np.float64)
        chern = np.empty((n_sets, sum(counts)), dtype=np.int64)
        link_min = np.empty(n_sets, dtype=np.float64)
        with self._call_lock:
            # NaN / Inf in the hoppings: TBK_ERR_NOT_FINITE -> ValueError, as for eigh
            handles, n_handles = self._handle_array()
            _lib.check(
                _lib.lib().tbk_berry_flux_multi(handles, n_handles, _lib.ptr(mesh_array), n_sets, _lib.ptr(sets), int(convention),
                                                _lib.ptr(pos), _lib.ptr(flux), _lib.ptr(chern), _lib.ptr(link_min))
            )
        edges = np.cumsum([0] + counts)
        return BerryFlux(sets, planes, flux, tuple(np.ascontiguousarray(chern[:, edges[p]:edges[p + 1]]) for p in range(len(planes))),
                         link_min)

    def construct_kdotp(self, k, order):
        """
        k.p model around the k-point ``k``: the Taylor expansion of H(k) (convention 2) up to total power
        ``order``, evaluated on the GPU (``Model.construct_kdotp``, ``_tb_model.py:942-982``).
        """
        import itertools  # pylint: disable=import-outside-toplevel
        import math  # pylint: disable=import-outside-toplevel

        from .kdotp import KdotpModel  # pylint: disable=import-outside-toplevel

        if order < 0:
            raise ValueError("The order for the k.p model must be positive.")
        k0 = np.ascontiguousarray(np.array(k, ndmin=1), dtype=np.float64)
        if k0.shape != (self.dim,):
            raise ValueError("k has shape {} but the model has dimension {}".format(k0.shape, self.dim))
        powers = [p for p in itertools.product(range(order + 1), repeat=self.dim) if sum(p) <= order]
        pw = np.array(powers, dtype=np.int32).reshape(len(powers), self.dim)
        pref = np.array(
            [(2j * np.pi) ** sum(p) / np.prod([math.factorial(x) for x in p]) for p in powers], dtype=np.complex128
        )
        source = self
        if self._sparse:  # the derivative kernel reads the dense staged operand
            r_vec, _ = self.packed_hop()
            dense = np.stack([np.array(m) for m in self._hop_values()]) if len(self.hop) else np.zeros((0, self.size, self.size))
            source = Model.from_packed(r_vec, dense, size=self.size, dim=self.dim)
            source.device = self.device
        coeffs = np.empty((len(powers), self.size, self.size), dtype=np.complex128)
        with source._call_lock:
            _lib.check(
                _lib.lib().tbk_kdotp_coefficients(
                    source._staged(), _lib.ptr(k0), len(powers), _lib.ptr(pw), _lib.ptr(pref), _lib.ptr(coeffs)
                )
            )
        return KdotpModel(taylor_coefficients={p: coeffs[i] for i, p in enumerate(powers)})

    # ------------------------------------------------------------------ HDF5 wire format
    @classmethod
    def from_hdf5_file(cls, hdf5_file, **kwargs):
        """
        Load a model stored by ``to_hdf5_file`` -- of this package or of the reference
        (``_tb_model.py:984-1011``).  Explicit keyword arguments take precedence over the file's.
        """
        from . import hdf5_lite  # pylint: disable=import-outside-toplevel

        tree = hdf5_lite.read(hdf5_file)
        if "type_tag" not in tree:
            warnings.warn(
                "The loaded file '{}' is stored in an outdated format. Consider loading and storing the "
                "file to update it.".format(hdf5_file),
                DeprecationWarning,
            )
        return cls.from_hdf5(tree, **kwargs)

    @classmethod
    def from_hdf5(cls, tree, **kwargs):
        """Build a model from the (nested dict) content of a model file (``_tb_model.py:1013-1036``)."""
        group = tree.get("tb_model", tree)  # a development version wrote a top-level 'tb_model' group
        new_kwargs = {"hop": {}}
        for key in ("uc", "occ", "size", "dim", "pos", "sparse"):
            if key in group:
                value = group[key]
                new_kwargs[key] = value.item() if isinstance(value, np.generic) else value
        if "hop" not in kwargs:
            sparse = bool(new_kwargs.get("sparse", False))
            for entry in group.get("hop", {}).values():
                r_vec = tuple(int(x) for x in entry["R"])
                if sparse:
                    new_kwargs["hop"][r_vec] = _csr(
                        (entry["data"], entry["indices"], entry["indptr"]),
                        shape=tuple(int(x) for x in entry["shape"]),
                    )
                else:
                    new_kwargs["hop"][r_vec] = np.array(entry["mat"])
            new_kwargs["contains_cc"] = False
        new_kwargs.update(kwargs)
        return cls(**new_kwargs)

    def to_hdf5(self):
        """The model as the nested dict ``hdf5_lite.write`` stores (``_tb_model.py:1038-1058``)."""
        tree = {"type_tag": "tbmodels.model"}
        if self.uc is not None:
            tree["uc"] = np.asarray(self.uc, dtype=float)
        if self.occ is not None:
            tree["occ"] = np.int64(self.occ)
        tree["size"] = np.int64(self.size)
        tree["dim"] = np.int64(self.dim)
        tree["pos"] = np.asarray(self.pos, dtype=float)
        tree["sparse"] = bool(self._sparse)
        hop = {}
        for i, (r_vec, mat) in enumerate(self._hop_items()):
            entry = {"R": np.array(r_vec, dtype=np.int64)}
            if self._sparse:
                mat = _csr(mat)
                entry["data"] = np.asarray(mat.data, dtype=complex)
                entry["indices"] = np.asarray(mat.indices, dtype=np.int32)
                entry["indptr"] = np.asarray(mat.indptr, dtype=np.int32)
                entry["shape"] = np.array(mat.shape, dtype=np.int64)
            else:
                entry["mat"] = np.asarray(mat, dtype=complex)
            hop[str(i)] = entry
        tree["hop"] = hop
        return tree

    def to_hdf5_file(self, hdf5_file):
        """Save the model to an HDF5 file the reference's ``Model.from_hdf5_file`` / ``io.load`` read."""
        from . import hdf5_lite  # pylint: disable=import-outside-toplevel

        hdf5_lite.write(hdf5_file, self.to_hdf5())

    # ------------------------------------------------------------------ introspection
    def timing(self, reset=True):
        """Per-stage HIP-event times of the staged model: ``{stage: (ms, launches)}`` (needs TBK_OPT_TIMING)."""
        ms = (ctypes.c_double * _lib.TBK_T_COUNT)()
        launches = (ctypes.c_int64 * _lib.TBK_T_COUNT)()
        _lib.check(_lib.lib().tbk_get_timing(self._staged(), ms, launches, int(bool(reset))))
        return {name: (ms[i], launches[i]) for i, name in enumerate(_lib.STAGE_NAMES)}

    def __repr__(self):
        return "tbmodels_amd.Model(hop=<{} matrices>, size={}, dim={}, sparse={})".format(
            len(self.hop), self.size, self.dim, self._sparse
        )
