"""
GPU tests (``-m gpu``) of the multi-GPU surfaces on the ONE GPU a test box has.

* the one-process-per-GPU form (``sharding.ShardedEigenval`` over RCCL, ``tbk_comm_*``): a world-1 communicator runs
  every line of the device-gather path -- RCCL accepts one rank;
* the single-process form behind the unchanged methods (``tbk_eigenval_multi`` / ``tbk_hamilton_multi``,
  ``Model.devices``): the device list ``[0, 0]`` = two staged handles on the one GPU, two host threads;
* ``bench.py --gpus N`` starting its own ranks.

What must stay true is the reference's: k-points are independent (``/root/reference/src/tbmodels/_tb_model.py:1111-1123``)
and results come back in caller order (``:1147-1150``).
"""

import ctypes
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import tbmodels_amd
from tbmodels_amd import _lib
from tbmodels_amd import synthetic as syn
from tbmodels_amd.rendezvous import FileGroup
from tbmodels_amd.sharding import ShardedEigenval
from oracle import tbk_oracle as oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def _grid(shape):
    axes = [np.linspace(0, 1, n, endpoint=False) for n in shape]
    return np.ascontiguousarray(np.stack([m.reshape(-1) for m in np.meshgrid(*axes, indexing="ij")], axis=1))


def _counter(model, which):
    value = ctypes.c_int64(-1)
    _lib.check(_lib.lib().tbk_model_counter(model._staged(), which, ctypes.byref(value)))
    return value.value


@pytest.fixture()
def small_model():
    n_orb, n_r = 12, 300
    r_vec, hop, pos = syn.dense_model_arrays(n_orb, n_r, syn.MODEL_SEED + 61)
    return tbmodels_amd.Model.from_packed(r_vec, hop, pos=pos), r_vec, hop


# ------------------------------------------------------------------------------------------------
# one process per GPU: world-1 RCCL communicator
# ------------------------------------------------------------------------------------------------
def test_sharded_eigenval_device_path_with_a_one_rank_communicator(tmp_path, small_model):
    """``ShardedEigenval(model, group, device=0)`` takes `_device_gather` (H2D of the slab, tbk_eigenval_device_hint,
    status word, ncclAllGather, D2H): bit-identical to the plain call on random k and on a ragged mesh slab (folded
    through the hint), and within 1e-10 of the oracle."""
    model, r_vec, hop = small_model
    group = FileGroup(0, 1, str(tmp_path / "rdzv"), token="t1")
    sharded = ShardedEigenval(model, group, device=0)
    try:
        rand = syn.random_kpoints(3001, seed=5)
        got = sharded(rand)
        assert got.shape == (3001, 12)
        assert np.array_equal(got, model.eigenval_array(rand))
        idx = np.random.default_rng(2).choice(len(rand), 16, replace=False)
        assert np.abs(got[idx] - np.array(oracle.eigenval(r_vec, hop, rand[idx]))).max() <= TOL

        comm = sharded._communicator()
        n_ranks, my_rank = ctypes.c_int(-1), ctypes.c_int(-1)
        _lib.check(_lib.lib().tbk_comm_ranks(comm, ctypes.byref(n_ranks), ctypes.byref(my_rank)))
        assert (n_ranks.value, my_rank.value) == (1, 0)

        slab = _grid((4, 40, 40))[211:5903]  # starts and ends inside a plane: ragged runs
        folded_before = _counter(model, _lib.TBK_CNT_FOLDED_CALLS)
        got = sharded(slab)
        assert _counter(model, _lib.TBK_CNT_FOLDED_CALLS) == folded_before + 1  # the hint reached the library
        assert np.array_equal(got, model.eigenval_array(slab))
        idx = np.random.default_rng(3).choice(len(slab), 16, replace=False)
        assert np.abs(got[idx] - np.array(oracle.eigenval(r_vec, hop, slab[idx]))).max() <= TOL

        one = sharded(rand[7])  # a single k-point is a 1-row list
        assert one.shape == (1, 12) and np.array_equal(one[0], model.eigenval_array(rand[7]))
        # the data path left nothing behind in the rendezvous directory beyond the RCCL id exchange
        assert len(os.listdir(group.path)) <= 2
    finally:
        sharded.close()
        group.close()


def test_sharded_eigenval_nan_slab_raises_then_recovers(tmp_path, small_model):
    """A NaN k-point: ValueError (scipy's check_finite, carried by the status word through the gather), then a clean call."""
    model, _, _ = small_model
    group = FileGroup(0, 1, str(tmp_path / "rdzv"), token="t2")
    sharded = ShardedEigenval(model, group, device=0)
    try:
        k = syn.random_kpoints(500, seed=8)
        bad = k.copy()
        bad[123, 1] = np.nan
        with pytest.raises(ValueError):
            sharded(bad)
        assert np.array_equal(sharded(k), model.eigenval_array(k))
    finally:
        sharded.close()
        group.close()


def test_overlapped_allgather_with_a_chunked_pipeline(small_model):
    """Six steps of ``tbk_comm_wait_slot`` / chunked ``tbk_eigenval_device_hint`` / ``tbk_comm_allgather_f64_overlapped``
    (the bench's step) reproduce the in-stream gather: with a small TBK_OPT_K_CHUNK the pipeline's other streams write
    d_E, the gather runs on the communicator's stream, and the buffers of a slot are reused two steps later."""
    model, r_vec, hop = small_model
    lib = _lib.lib()
    n_orb = 12
    handle = model._staged()
    uid = np.zeros(128, dtype=np.uint8)
    _lib.check(lib.tbk_comm_unique_id(_lib.ptr(uid)))
    comm = ctypes.c_void_p()
    _lib.check(lib.tbk_comm_create(0, 1, 0, _lib.ptr(uid), ctypes.byref(comm)))
    nk = 20_000
    lists = [np.ascontiguousarray(syn.random_kpoints(nk, seed=100 + s)) for s in range(6)]
    buffers = []

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        _lib.check(lib.tbk_device_malloc(0, nbytes, ctypes.byref(p)))
        buffers.append(p)
        return p

    try:
        d_k = [dmalloc(nk * 3 * 8) for _ in range(2)]
        d_e = [dmalloc(nk * n_orb * 8) for _ in range(2)]
        d_g = [dmalloc(nk * n_orb * 8) for _ in range(2)]
        reference = []
        for k in lists:  # in-stream form, default chunking
            _lib.check(lib.tbk_memcpy_h2d(0, d_k[0], _lib.ptr(k), k.nbytes))
            _lib.check(lib.tbk_eigenval_device(handle, d_k[0], nk, d_e[0]))
            _lib.check(lib.tbk_comm_allgather_f64(comm, handle, d_e[0], d_g[0], nk * n_orb))
            _lib.check(lib.tbk_eigenval_check(handle))
            out = np.empty((nk, n_orb))
            _lib.check(lib.tbk_memcpy_d2h(0, _lib.ptr(out), d_g[0], out.nbytes))
            reference.append(out)
        assert np.abs(reference[0][:8] - np.array(oracle.eigenval(r_vec, hop, lists[0][:8]))).max() <= TOL

        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, 4096))  # 5 chunks per call
        results = [None] * 6
        for step, k in enumerate(lists):
            slot = step & 1
            if step >= 2:  # the slot's previous gather must be complete before its result is read and its buffers reused
                _lib.check(lib.tbk_comm_synchronize(comm))
                out = np.empty((nk, n_orb))
                _lib.check(lib.tbk_memcpy_d2h(0, _lib.ptr(out), d_g[slot], out.nbytes))
                results[step - 2] = out
            _lib.check(lib.tbk_comm_wait_slot(comm, handle, slot))
            _lib.check(lib.tbk_memcpy_h2d(0, d_k[slot], _lib.ptr(k), k.nbytes))
            _lib.check(lib.tbk_eigenval_device_hint(handle, d_k[slot], _lib.ptr(k), nk, d_e[slot]))
            _lib.check(lib.tbk_comm_allgather_f64_overlapped(comm, handle, d_e[slot], d_g[slot], nk * n_orb, slot))
        _lib.check(lib.tbk_synchronize(handle))
        _lib.check(lib.tbk_comm_synchronize(comm))
        _lib.check(lib.tbk_eigenval_check(handle))
        for step in (4, 5):
            out = np.empty((nk, n_orb))
            _lib.check(lib.tbk_memcpy_d2h(0, _lib.ptr(out), d_g[step & 1], out.nbytes))
            results[step] = out
        for step in range(6):
            # chunking changes which tridiagonal solver a chunk takes: agreement to rounding, not to the bit
            assert np.abs(results[step] - reference[step]).max() < 1e-12, step
    finally:
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, 0))
        lib.tbk_comm_destroy(comm)
        for p in buffers:
            lib.tbk_device_free(0, p)


def _gather_call(lib, comm, handle, k, per, block_rows, chunk, host_status=0):
    """One tbk_eigenval_device_gather call of a world-1 communicator: (all rows [per][n], status words, return code)."""
    n_orb = 12
    buffers = []

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        _lib.check(lib.tbk_device_malloc(0, max(nbytes, 8), ctypes.byref(p)))
        buffers.append(p)
        return p

    os.environ["TBK_GATHER_BLOCK_ROWS"] = str(block_rows)
    try:
        k = np.ascontiguousarray(k)
        d_k = dmalloc(k.nbytes)
        d_all = dmalloc(per * n_orb * 8)
        d_st = dmalloc(8)
        junk = np.full((per, n_orb), 7.5)
        _lib.check(lib.tbk_memcpy_h2d(0, d_all, _lib.ptr(junk), junk.nbytes))
        if len(k):
            _lib.check(lib.tbk_memcpy_h2d(0, d_k, _lib.ptr(k), k.nbytes))
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, chunk))
        rc = lib.tbk_eigenval_device_gather(comm, handle, d_k, _lib.ptr(k) if len(k) else None, len(k), per, host_status, d_all, d_st)
        _lib.check(lib.tbk_comm_synchronize(comm))
        out = np.empty((per, n_orb))
        status = np.empty(1)
        _lib.check(lib.tbk_memcpy_d2h(0, _lib.ptr(out), d_all, out.nbytes))
        _lib.check(lib.tbk_memcpy_d2h(0, _lib.ptr(status), d_st, 8))
        return out, status, rc
    finally:
        os.environ.pop("TBK_GATHER_BLOCK_ROWS", None)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, 0))
        for p in buffers:
            lib.tbk_device_free(0, p)


def test_chunk_pipelined_gather_equals_the_in_stream_gather(small_model):
    """``tbk_eigenval_device_gather``: blocks of finished rows leave on the communicator's stream while later k chunks
    compute, land in a [rank][block] area and are moved to their rows -- bit for bit what the plain call with the same
    chunking writes, on a random list and on a ragged mesh slab (folded through the hint), for block sizes that do and do
    not divide the chunks, for a short slab (zero rows behind it) and an empty one; a NaN k-point travels as the status
    word and the flags are consumed; a rank that arrives with a failure computes nothing and reports it."""
    model, r_vec, hop = small_model
    lib = _lib.lib()
    handle = model._staged()
    uid = np.zeros(128, dtype=np.uint8)
    _lib.check(lib.tbk_comm_unique_id(_lib.ptr(uid)))
    comm = ctypes.c_void_p()
    _lib.check(lib.tbk_comm_create(0, 1, 0, _lib.ptr(uid), ctypes.byref(comm)))
    try:
        rand = syn.random_kpoints(20_011, seed=31)
        slab = _grid((4, 40, 40))[211:5903]
        for k in (rand, slab):
            nk = len(k)
            for chunk, block in ((4096, 1000), (4096, 4096), (0, 777), (4096, 10 ** 9), (8192, 3001)):
                _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, chunk))
                plain = model.eigenval_array(k)  # same handle, same chunking: the same kernels on the same rows
                _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, 0))
                out, status, rc = _gather_call(lib, comm, handle, k, nk, block, chunk)
                assert rc == 0 and status[0] == 0
                assert np.array_equal(out, plain), (nk, chunk, block)
        idx = np.random.default_rng(5).choice(len(slab), 16, replace=False)  # (`out` is the mesh slab's result here)
        assert np.abs(out[idx] - np.array(oracle.eigenval(r_vec, hop, slab[idx]))).max() <= TOL
        # short slab: nk < per -> zero rows behind the computed ones; empty slab: all zero
        out, status, rc = _gather_call(lib, comm, handle, rand[:5000], 6001, 1024, 2048)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, 2048))
        plain = model.eigenval_array(rand[:5000])
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, 0))
        assert rc == 0 and status[0] == 0 and np.array_equal(out[:5000], plain) and not out[5000:].any()
        out, status, rc = _gather_call(lib, comm, handle, rand[:0], 300, 128, 0)
        assert rc == 0 and status[0] == 0 and not out.any()
        # a path without chunk events (rocSOLVER): every block leaves behind the main stream at the end of the call
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_ROCSOLVER))
        try:
            plain = model.eigenval_array(rand[:3000])
            out, status, rc = _gather_call(lib, comm, handle, rand[:3000], 3000, 700, 0)
            assert rc == 0 and status[0] == 0 and np.array_equal(out, plain)
        finally:
            _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_EIGENSOLVER, _lib.TBK_EIG_AUTO))
        # a NaN k-point: the status word says so, the flags are consumed (tbk_eigenval_check is clean afterwards)
        bad = rand[:3000].copy()
        bad[1234, 2] = np.nan
        out, status, rc = _gather_call(lib, comm, handle, bad, 3000, 512, 1024)
        assert rc == 0 and int(status[0]) == _lib.TBK_ERR_NOT_FINITE
        _lib.check(lib.tbk_eigenval_check(handle))
        # a rank that arrives with a failure: nothing computed, its status gathered
        out, status, rc = _gather_call(lib, comm, handle, rand[:1000], 1000, 256, 0, host_status=_lib.TBK_ERR_MEMORY)
        assert int(status[0]) == _lib.TBK_ERR_MEMORY and not out.any()
        # a failure of THIS rank behind the argument checks (here: more k-points than its slab has rows) does not end the
        # call in front of the collectives -- the peers would wait in them: it travels as the status word, after the same
        # sequence of gathers, and comes back as the return code
        out, status, rc = _gather_call(lib, comm, handle, rand[:1000], 900, 256, 0)
        assert rc == _lib.TBK_ERR_ARGUMENT and int(status[0]) == _lib.TBK_ERR_ARGUMENT and not out.any()
        # the landing area is allocated in the agreement step (sharding.py): same results afterwards, bad shapes refused
        _lib.check(lib.tbk_comm_prepare_gather(comm, 12, 50_000))
        assert lib.tbk_comm_prepare_gather(comm, 0, 10) == _lib.TBK_ERR_ARGUMENT
        out, status, rc = _gather_call(lib, comm, handle, rand[:3000], 3000, 700, 1024)
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, 1024))
        plain = model.eigenval_array(rand[:3000])
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, 0))
        assert rc == 0 and status[0] == 0 and np.array_equal(out, plain)
        # the gather's hook was an argument of its own call: a plain call of several chunks (three of 128 k-points) on
        # this handle, behind all the gathers above, is bit for bit what a handle that never saw a gather computes
        fresh = tbmodels_amd.Model.from_packed(r_vec, hop)
        for mdl in (model, fresh):
            _lib.check(lib.tbk_model_set_option(mdl._staged(), _lib.TBK_OPT_K_CHUNK, 128))
        assert np.array_equal(model.eigenval_array(rand[:300]), fresh.eigenval_array(rand[:300]))
        _lib.check(lib.tbk_model_set_option(handle, _lib.TBK_OPT_K_CHUNK, 0))
        verdict = np.full(1, -1.0)
        _lib.check(lib.tbk_comm_agree(comm, 3, _lib.ptr(verdict)))
        assert verdict[0] == 3.0
        _lib.check(lib.tbk_comm_agree(comm, 0, _lib.ptr(verdict)))
        assert verdict[0] == 0.0
    finally:
        lib.tbk_comm_destroy(comm)


# ------------------------------------------------------------------------------------------------
# one process, several devices, unchanged methods
# ------------------------------------------------------------------------------------------------
def test_model_on_a_device_list_equals_the_single_device_result(small_model):
    model, r_vec, hop = small_model
    twin = pickle.loads(pickle.dumps(model))
    assert twin._handles == [] and twin.devices == model.devices
    twin.devices = [0, 0]  # two staged copies on the one GPU, two host threads
    rand = syn.random_kpoints(5001, seed=21)  # odd count: slabs of 2501 and 2500
    single = model.eigenval_array(rand)
    both = twin.eigenval_array(rand)
    assert len(twin._handles) == 2
    assert np.abs(both - single).max() < 1e-12  # slab sizes decide the tridiagonal solver of a chunk: rounding level
    idx = np.random.default_rng(4).choice(len(rand), 16, replace=False)
    assert np.abs(both[idx] - np.array(oracle.eigenval(r_vec, hop, rand[idx]))).max() <= TOL
    as_list = twin.eigenval(rand[:5])
    assert isinstance(as_list, list) and len(as_list) == 5 and as_list[0].shape == (12,)
    assert twin.eigenval(rand[0]).shape == (12,)  # one k-point: the second slab is empty

    slab = _grid((4, 40, 40))[211:5903]  # ragged mesh slab: each half is folded on its own
    assert np.abs(twin.eigenval_array(slab) - model.eigenval_array(slab)).max() < 1e-12
    assert _counter(twin, _lib.TBK_CNT_FOLDED_CALLS) >= 1

    ham = twin.hamilton(rand[:301], convention=1)
    assert np.array_equal(ham, model.hamilton(rand[:301], convention=1))
    assert np.abs(ham[:4] - oracle.hamilton(r_vec, hop, rand[:4], 1, pos=model.pos)).max() <= TOL

    bad = rand.copy()
    bad[4000, 2] = np.inf  # lands in the second slab only
    with pytest.raises(ValueError) as info:
        twin.eigenval(bad)
    assert "infs or NaNs" in str(info.value)
    assert np.abs(twin.eigenval_array(rand) - single).max() < 1e-12  # and the model is usable afterwards

    clone = pickle.loads(pickle.dumps(twin))  # pickling drops the handles, keeps the device list
    assert clone._handles == [] and clone.devices == [0, 0]
    twin.add_on_site([0.25] * 12)  # an edit re-stages every copy
    shifted = twin.eigenval_array(rand[:64])
    assert np.abs(shifted - (single[:64] + 0.25)).max() < 1e-12


def test_eigenval_multi_c_abi_argument_checks(small_model):
    model, _, _ = small_model
    lib = _lib.lib()
    handle = model._staged()
    k = syn.random_kpoints(10)
    out = np.empty((10, 12))
    assert lib.tbk_eigenval_multi(None, 1, _lib.ptr(k), 10, _lib.ptr(out)) == _lib.TBK_ERR_ARGUMENT
    pair = (ctypes.c_void_p * 2)(handle.value, None)
    assert lib.tbk_eigenval_multi(pair, 2, _lib.ptr(k), 10, _lib.ptr(out)) == _lib.TBK_ERR_ARGUMENT
    other = tbmodels_amd.Model.from_packed(*syn.dense_model_arrays(6, 4, 1)[:2])
    mixed = (ctypes.c_void_p * 2)(handle.value, other._staged().value)
    assert lib.tbk_eigenval_multi(mixed, 2, _lib.ptr(k), 10, _lib.ptr(out)) == _lib.TBK_ERR_ARGUMENT
    same = (ctypes.c_void_p * 3)(handle.value, handle.value, handle.value)  # one handle three times: serialised by its lock
    _lib.check(lib.tbk_eigenval_multi(same, 3, _lib.ptr(k), 10, _lib.ptr(out)))
    assert np.abs(out - model.eigenval_array(k)).max() < 1e-12
    _lib.check(lib.tbk_eigenval_multi(same, 3, _lib.ptr(k), 0, _lib.ptr(out)))  # empty list


# ------------------------------------------------------------------------------------------------
# bench.py --gpus N
# ------------------------------------------------------------------------------------------------
def _bench(extra_args, extra_env, timeout=600):
    env = dict(os.environ, TBK_BENCH_SKIP_CONFIGS="1", TBK_BENCH_SKIP_PEAK="1", **extra_env)
    for name in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(name, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--cpu-sample", "0"] + extra_args, env=env,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, check=False)


def test_bench_with_a_forced_one_rank_communicator():
    """``TBK_BENCH_FORCE_COMM=1 bench.py --gpus 1``: the overlapped RCCL all-gather inside the timed region reports one
    rank and costs (next to) nothing."""
    values = {}
    for attempt in range(2):  # a second pair if the first one was disturbed
        for forced in ("0", "1"):
            done = _bench(["--gpus", "1", "--steps", "5"], {"TBK_BENCH_FORCE_COMM": forced})
            assert done.returncode == 0, done.stderr.decode()[-2000:]
            line = json.loads(done.stdout.decode().strip().splitlines()[-1])
            assert line["n_gpus"] == 1 and line["max_abs_err_vs_oracle"] is None
            assert line["max_trace_identity_err_4096_rows"] <= TOL
            assert line["rccl_ranks"] == (1 if forced == "1" else 0)
            values[forced] = line["value"]
        if abs(values["1"] / values["0"] - 1.0) <= 0.02:
            break
    assert abs(values["1"] / values["0"] - 1.0) <= 0.02, values


def test_bench_strong_scaling_leg_with_a_one_rank_communicator():
    """The cfg4 leg of ``bench.py --gpus N`` (the 100^3 mesh in N slabs through ``tbk_eigenval_device_gather``, the gather
    inside its timing) with a one-rank communicator: its entry sits under ``configs``, its checks (oracle rows of the first
    and the last slab, trace identity on 4096 rows of the whole mesh) hold, the gather adds next to nothing at one rank.
    And the safety net: a leg that does not come back within its time limit must not take the main line with it -- the line is
    printed with "strong_scaling": "timeout" and the process ends with status 3."""
    env = {"TBK_BENCH_FORCE_COMM": "1", "TBK_BENCH_STRONG": "1"}
    done = _bench(["--gpus", "1", "--steps", "2"], env)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    lines = [ln for ln in done.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    leg = line["configs"]["cfg4_one_rank_communicator"]
    assert "error" not in leg, leg
    assert leg["scaling"] == "strong" and leg["rccl_ranks"] == 1 and leg["kpoints_per_rank"] == 10 ** 6
    assert leg["max_abs_err_vs_oracle"] <= TOL and leg["max_trace_identity_err_4096_rows"] <= TOL
    assert leg["value"] > 0.5 * 10 ** 6  # the folded path (a direct evaluation of the mesh runs at ~0.95 M k-points/s)
    assert abs(leg["per_rank"]["exposed_gather_ms"][0]) < 0.1 * leg["per_rank"]["compute_ms"][0]
    assert line["strong_scaling"] == "ok"
    # (round 5: the line is still printed, with a top-level verdict, and the STATUS tells the launcher -- the process exits, it is
    # never re-executed)
    done = _bench(["--gpus", "1", "--steps", "2"], dict(env, TBK_BENCH_STRONG_TIMEOUT="0.01"))
    assert done.returncode == 3, done.stderr.decode()[-2000:]
    lines = [ln for ln in done.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["value"] > 0 and "did not finish" in line["configs"]["cfg4_one_rank_communicator"]["error"]
    assert line["strong_scaling"] == "timeout"


def test_bench_starts_its_own_ranks_and_fails_for_rccl_reasons_on_one_gpu():
    """``bench.py --gpus 2`` with no launcher in the environment starts two rank processes itself.  On a one-GPU box both
    land on device 0 and RCCL refuses the communicator: a non-zero exit that names RCCL -- not the launcher."""
    if _lib.device_count() >= 2:
        done = _bench(["--gpus", "2", "--nk", "8192"], {})
        assert done.returncode == 0, done.stderr.decode()[-2000:]
        line = json.loads(done.stdout.decode().strip().splitlines()[-1])
        assert line["n_gpus"] == 2 and line["rccl_ranks"] == 2
        return
    done = _bench(["--gpus", "2", "--nk", "8192"], {}, timeout=900)
    err = done.stderr.decode()
    assert done.returncode != 0
    assert "RCCL communicator unavailable" in err, err[-2000:]
    assert "launch with" not in err
    assert done.stdout.decode().strip() == ""  # no number that RCCL never produced
    # the launch mechanics themselves (two ranks, rendezvous, max over ranks, one JSON line) with the host gather
    done = _bench(["--gpus", "2", "--nk", "8192"], {"TBK_BENCH_ALLOW_HOST_GATHER": "1"}, timeout=900)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    lines = [ln for ln in done.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["rccl_ranks"] == 0 and "host all-gather" in line["config"]["collective"]


def test_kdotp_model_on_a_device_list():
    """``KdotpModel.devices`` (kdotp.py:51-100 behind several GPUs): ``[0, 0]`` = two staged copies, two host threads; equal to
    the single-device result and to the oracle; pickling keeps the list and drops the handles; one k-point uses one slab."""
    rng = np.random.default_rng(17)
    coeffs = {}
    for key in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (1, 1, 0), (0, 1, 2)]:
        a = rng.normal(size=(6, 6)) + 1j * rng.normal(size=(6, 6))
        coeffs[key] = a + a.conj().T
    single = tbmodels_amd.KdotpModel(coeffs)
    twin = pickle.loads(pickle.dumps(single))
    twin.devices = [0, 0]
    assert twin.devices == [0, 0] and twin.device == 0
    k = rng.uniform(-0.3, 0.3, size=(4001, 3))
    e1, e2 = single.eigenval_array(k), twin.eigenval_array(k)
    assert len(twin._handles) == 2
    assert np.abs(e1 - e2).max() < 1e-12
    powers = np.array(list(coeffs.keys()))
    ref = np.array(oracle.kdotp_eigenval(powers, np.stack([coeffs[tuple(p)] for p in powers]), k[:32]))
    assert np.abs(e2[:32] - ref).max() <= TOL
    assert np.array_equal(twin.hamilton(k[:301]), single.hamilton(k[:301]))
    assert twin.eigenval(k[0]).shape == (6,) and isinstance(twin.eigenval(k[:3]), list)
    again = pickle.loads(pickle.dumps(twin))
    assert again.devices == [0, 0] and again._handles == []
    with pytest.raises(ValueError):
        twin.devices = []
