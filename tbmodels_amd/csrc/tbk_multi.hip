// tbk_multi.hip -- one call, several devices: the k list of a host-buffer call is cut into contiguous slabs, one per
// staged handle, and every slab runs on its handle's device from its own host thread.
//
// The reference evaluates k-points one after the other in ONE process (/root/reference/src/tbmodels/_tb_model.py:1111-1123
// has no cross-k term, :1147-1150 returns rows in caller order); this is the form of the sharded path that keeps that
// surface: Model.eigenval / Model.hamilton stay single calls of a single process, no launcher, no process group.
// With host output there is nothing to exchange -- every device copies its slab straight into its rows of the caller's
// array -- so no collective is issued here (the RCCL all-gather of tbk_comm.hip serves device-resident consumers).
//
// Slabs are the same contiguous ceil(nk / n) rows that tbmodels_amd.sharding.slab_bounds gives the ranks of the
// one-process-per-GPU form, so both forms evaluate a k-point on the same device index and fold mesh slabs alike.

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "tbk_tetra_staged.h"

namespace {

struct SlabResult {
    int status = TBK_OK;
    std::string message;
};

template <class Call>
int run_slabs(int n, int64_t nk, Call&& call) {  // call(i, lo, count): slab i on handle i
    const TetraSlabs cut(nk, n);
    // slabs that hold k-points: a one-k call under TBK_DEVICES=0..7 has ONE, and must not pay seven thread starts
    const int busy = cut.busy();
    if (busy <= 1) return call(0, 0, nk);
    std::vector<SlabResult> results((size_t)busy);
    auto work = [&](int i) {
        const int status = call(i, cut.lo(i), cut.count(i));
        results[(size_t)i].status = status;
        if (status != TBK_OK) results[(size_t)i].message = tbk_last_error();  // this thread's message
    };
    std::vector<std::thread> threads;
    threads.reserve((size_t)busy);
    try {
        for (int i = 1; i < busy; ++i) threads.emplace_back(work, i);
    } catch (...) {
        for (auto& t : threads) t.join();
        tbk_set_error("cannot start a host thread per device");
        return TBK_ERR_DEVICE;
    }
    work(0);  // the caller's thread takes the first slab
    for (auto& t : threads) t.join();
    // the failure of the FIRST failing slab in k order is the call's failure: what a loop over the k list would have hit first
    for (int i = 0; i < busy; ++i) {
        if (results[(size_t)i].status != TBK_OK) {
            tbk_set_error("%s", results[(size_t)i].message.c_str());
            return results[(size_t)i].status;
        }
    }
    return TBK_OK;
}

int check_handles(tbk_model* const* handles, int n) {
    TBK_ARG(handles != nullptr && n >= 1, "no handles");
    for (int i = 0; i < n; ++i) {
        TBK_ARG(handles[i] != nullptr, "a handle is NULL");
        TBK_ARG(handles[i]->dim == handles[0]->dim && handles[i]->n_orb == handles[0]->n_orb,
                "handles of different models (dim / n_orb differ)");
    }
    return TBK_OK;
}

}  // namespace

extern "C" int tbk_eigenval_multi(tbk_model* const* handles, int n_handles, const double* k, int64_t nk, double* E_out) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(nk >= 0, "nk < 0");
    if (nk == 0) return TBK_OK;
    TBK_ARG(k && E_out, "k / E is NULL");
    const int dim = handles[0]->dim, n_orb = handles[0]->n_orb;
    if (n_handles == 1) return tbk_eigenval(handles[0], k, nk, E_out);
    return run_slabs(n_handles, nk, [&](int i, int64_t lo, int64_t count) {
        return tbk_eigenval(handles[i], k + lo * dim, count, E_out + lo * n_orb);
    });
}

extern "C" int tbk_hamilton_multi(tbk_model* const* handles, int n_handles, const double* k, int64_t nk, int convention,
                                  const double* pos, double* H_out) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(convention == 1 || convention == 2, "convention must be 1 or 2");
    TBK_ARG(nk >= 0, "nk < 0");
    if (nk == 0) return TBK_OK;
    TBK_ARG(k && H_out, "k / H is NULL");
    TBK_ARG(convention == 2 || pos != nullptr, "convention 1 needs pos");
    const int dim = handles[0]->dim;
    const int64_t nn2 = (int64_t)handles[0]->n_orb * handles[0]->n_orb * 2;
    if (n_handles == 1) return tbk_hamilton(handles[0], k, nk, convention, pos, H_out);
    return run_slabs(n_handles, nk, [&](int i, int64_t lo, int64_t count) {
        return tbk_hamilton(handles[i], k + lo * dim, count, convention, pos, H_out + lo * nn2);
    });
}

extern "C" int tbk_eigh_multi(tbk_model* const* handles, int n_handles, const double* k, int64_t nk, int convention,
                              const double* pos, double* E_out, double* U_out) {
    TBK_CHECK(tbk_eigh_check_arguments(nk, convention, pos));
    TBK_CHECK(check_handles(handles, n_handles));
    if (nk == 0) return TBK_OK;
    TBK_ARG(k && E_out && U_out, "k / E / U is NULL");
    const int dim = handles[0]->dim, n_orb = handles[0]->n_orb;
    const int64_t nn2 = (int64_t)n_orb * n_orb * 2;
    if (n_handles == 1) return tbk_eigh(handles[0], k, nk, convention, pos, E_out, U_out);
    return run_slabs(n_handles, nk, [&](int i, int64_t lo, int64_t count) {
        return tbk_eigh(handles[i], k + lo * dim, count, convention, pos, E_out + lo * n_orb, U_out + lo * nn2);
    });
}

// The surface Green's function on several devices (tbk_surface.hip): the k list in the slabs of tbk_hamilton_multi, every device writing
// its rows of the results
extern "C" int tbk_surface_green_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int64_t n_z,
                                       const double* z, int max_iterations, int spectral, int32_t* iterations, double* bottom, double* top,
                                       double* bulk) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(nk >= 0, "nk < 0");
    if (n_handles == 1 || nk == 0)
        return tbk_surface_green(handles[0], axis, layers, k, nk, n_z, z, max_iterations, spectral, iterations, bottom, top, bulk);
    TBK_ARG(n_z >= 1 && n_z <= 4096 && layers >= 0 && layers <= 1024, "n_z must be 1 to 4096, layers 0 ... 1024");
    TBK_ARG(iterations != nullptr && bottom != nullptr && top != nullptr && bulk != nullptr, "iterations / bottom / top / bulk is NULL");
    const int dim = handles[0]->dim;
    TBK_ARG(k != nullptr || dim == 1, "k is NULL");
    const int64_t N = (int64_t)handles[0]->n_orb * std::max(layers, 1);
    const int64_t item = n_z * (spectral != 0 ? N : N * N * 2);  // doubles of one k-point in each of the three results
    return run_slabs(n_handles, nk, [&](int i, int64_t lo, int64_t count) {
        return tbk_surface_green_slab(handles[i], lo, axis, layers, k != nullptr ? k + lo * (dim - 1) : nullptr, count, n_z, z, max_iterations, spectral,
                                      iterations + lo * n_z, bottom + lo * item, top + lo * item, bulk + lo * item);
    });
}

// The transmission on several devices (tbk_surface.hip): the slabs of tbk_surface_green_multi; every handle stages the whole V
extern "C" int tbk_transmission_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M, const double* V,
                                      int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T, double* G) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(nk >= 0, "nk < 0");
    if (n_handles == 1 || nk == 0) return tbk_transmission(handles[0], axis, layers, k, nk, M, V, n_z, z, max_iterations, iterations, T, G);
    TBK_ARG(n_z >= 1 && n_z <= 4096 && layers >= 1 && layers <= 1024, "n_z must be 1 to 4096, layers 1 ... 1024");
    TBK_ARG(iterations != nullptr && T != nullptr, "iterations / T is NULL");
    const int dim = handles[0]->dim;
    TBK_ARG(k != nullptr || dim == 1, "k is NULL");
    const int64_t N = (int64_t)handles[0]->n_orb * layers;
    const int64_t item = n_z * N * N * 2;  // doubles of one k-point in G
    return run_slabs(n_handles, nk, [&](int i, int64_t lo, int64_t count) {
        return tbk_transmission_slab(handles[i], lo, axis, layers, k != nullptr ? k + lo * (dim - 1) : nullptr, count, M, V, n_z, z, max_iterations,
                                     iterations + lo * n_z, T + lo * n_z, G != nullptr ? G + lo * item : nullptr);
    });
}

// The transmission of an ensemble on several devices (tbk_ensemble.hip): the slabs of tbk_transmission_multi; every handle stages all the samples
extern "C" int tbk_transmission_ensemble_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M,
                                               int64_t n_s, const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations,
                                               int32_t* iterations, double* T) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(nk >= 0, "nk < 0");
    if (n_handles == 1 || nk == 0)
        return tbk_transmission_ensemble(handles[0], axis, layers, k, nk, M, n_s, V, onsite, n_z, z, max_iterations, iterations, T);
    TBK_ARG(n_z >= 1 && n_z <= 4096 && layers >= 1 && layers <= 1024 && n_s >= 1 && n_s <= 4096, "n_z and n_s must be 1 to 4096, layers 1 ... 1024");
    TBK_ARG(iterations != nullptr && T != nullptr, "iterations / T is NULL");
    const int dim = handles[0]->dim;
    TBK_ARG(k != nullptr || dim == 1, "k is NULL");
    return run_slabs(n_handles, nk, [&](int i, int64_t lo, int64_t count) {
        return tbk_transmission_ensemble_slab(handles[i], lo, axis, layers, k != nullptr ? k + lo * (dim - 1) : nullptr, count, M, n_s, V, onsite, n_z, z,
                                              max_iterations, iterations + lo * n_z, T + lo * n_z * n_s);
    });
}

// The transmission eigenvalues on several devices (tbk_channels.hip): the slabs of tbk_transmission_ensemble_multi
extern "C" int tbk_transmission_channels_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M,
                                               int64_t n_s, const double* V, const double* onsite, int64_t n_z, const double* z, int max_iterations,
                                               int32_t* iterations, double* T, double* channels) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(nk >= 0, "nk < 0");
    if (n_handles == 1 || nk == 0)
        return tbk_transmission_channels(handles[0], axis, layers, k, nk, M, n_s, V, onsite, n_z, z, max_iterations, iterations, T, channels);
    TBK_ARG(n_z >= 1 && n_z <= 4096 && layers >= 1 && layers <= 1024 && n_s >= 1 && n_s <= 4096, "n_z and n_s must be 1 to 4096, layers 1 ... 1024");
    TBK_ARG(iterations != nullptr && T != nullptr && channels != nullptr, "iterations / T / channels is NULL");
    const int dim = handles[0]->dim;
    TBK_ARG(k != nullptr || dim == 1, "k is NULL");
    const int64_t N = (int64_t)handles[0]->n_orb * layers;
    return run_slabs(n_handles, nk, [&](int i, int64_t lo, int64_t count) {
        return tbk_transmission_channels_slab(handles[i], lo, axis, layers, k != nullptr ? k + lo * (dim - 1) : nullptr, count, M, n_s, V, onsite, n_z, z,
                                              max_iterations, iterations + lo * n_z, T + lo * n_z * n_s, channels + lo * n_z * n_s * N);
    });
}

// The device Green's function on several devices (tbk_device_green.hip): the slabs of tbk_transmission_multi; every handle stages the whole V
extern "C" int tbk_device_green_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M, const double* V,
                                      int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T, double* ldos, double* left,
                                      double* right, double* G, double* F, double* C) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(nk >= 0, "nk < 0");
    if (n_handles == 1 || nk == 0)
        return tbk_device_green(handles[0], axis, layers, k, nk, M, V, n_z, z, max_iterations, iterations, T, ldos, left, right, G, F, C);
    TBK_ARG(n_z >= 1 && n_z <= 4096 && layers >= 1 && layers <= 1024 && M >= 1 && M <= 4096, "n_z and M must be 1 to 4096, layers 1 ... 1024");
    TBK_ARG(iterations != nullptr && T != nullptr && ldos != nullptr && left != nullptr && right != nullptr, "iterations / T / ldos / left / right is NULL");
    TBK_ARG((G != nullptr) == (F != nullptr) && (G != nullptr) == (C != nullptr), "G, F and C must all be NULL or none of them");
    const int dim = handles[0]->dim;
    TBK_ARG(k != nullptr || dim == 1, "k is NULL");
    const int64_t N = (int64_t)handles[0]->n_orb * layers;
    const int64_t rows = n_z * M * N, mats = rows * N * 2;  // doubles of one k-point in ldos, left, right and in G, F, C
    return run_slabs(n_handles, nk, [&](int i, int64_t lo, int64_t count) {
        return tbk_device_green_slab(handles[i], lo, axis, layers, k != nullptr ? k + lo * (dim - 1) : nullptr, count, M, V, n_z, z, max_iterations,
                                     iterations + lo * n_z, T + lo * n_z, ldos + lo * rows, left + lo * rows, right + lo * rows,
                                     G != nullptr ? G + lo * mats : nullptr, G != nullptr ? F + lo * mats : nullptr, G != nullptr ? C + lo * mats : nullptr);
    });
}

// The bond currents on several devices (tbk_device_green.hip): the slabs of tbk_device_green_multi
extern "C" int tbk_device_current_multi(tbk_model* const* handles, int n_handles, int axis, int layers, const double* k, int64_t nk, int M, const double* V,
                                        int64_t n_z, const double* z, int max_iterations, int32_t* iterations, double* T, double* ldos, double* left,
                                        double* right, double* current_left, double* current_right, double* inter_left, double* inter_right,
                                        double* intra_left, double* intra_right) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(nk >= 0, "nk < 0");
    if (n_handles == 1 || nk == 0)
        return tbk_device_current(handles[0], axis, layers, k, nk, M, V, n_z, z, max_iterations, iterations, T, ldos, left, right, current_left,
                                  current_right, inter_left, inter_right, intra_left, intra_right);
    TBK_ARG(n_z >= 1 && n_z <= 4096 && layers >= 1 && layers <= 1024 && M >= 1 && M <= 4096, "n_z and M must be 1 to 4096, layers 1 ... 1024");
    TBK_ARG(iterations != nullptr && T != nullptr && ldos != nullptr && left != nullptr && right != nullptr, "iterations / T / ldos / left / right is NULL");
    TBK_ARG(current_left != nullptr && current_right != nullptr, "current_left / current_right is NULL");
    const bool bonds = inter_left != nullptr;
    TBK_ARG((inter_right != nullptr) == bonds && (intra_left != nullptr) == bonds && (intra_right != nullptr) == bonds,
            "inter_left, inter_right, intra_left and intra_right must all be NULL or none of them");
    const int dim = handles[0]->dim;
    TBK_ARG(k != nullptr || dim == 1, "k is NULL");
    const int64_t N = (int64_t)handles[0]->n_orb * layers;
    const int64_t rows = n_z * M * N, krows = n_z * (M - 1) * N;  // doubles of one k-point in ldos ... and in current_left, current_right
    return run_slabs(n_handles, nk, [&](int i, int64_t lo, int64_t count) {
        return tbk_device_current_slab(handles[i], lo, axis, layers, k != nullptr ? k + lo * (dim - 1) : nullptr, count, M, V, n_z, z, max_iterations,
                                       iterations + lo * n_z, T + lo * n_z, ldos + lo * rows, left + lo * rows, right + lo * rows,
                                       current_left + lo * krows, current_right + lo * krows, bonds ? inter_left + lo * krows * N : nullptr,
                                       bonds ? inter_right + lo * krows * N : nullptr, bonds ? intra_left + lo * rows * N : nullptr,
                                       bonds ? intra_right + lo * rows * N : nullptr);
    });
}

// The density of states of a mesh on several devices (tbk_dos.hip): handle i takes a contiguous slab of ceil(n_1 / n) cells along
// axis 0 and evaluates the planes of that slab plus the one periodic neighbour plane its last cells need.  Every handle returns
// its share of nos; the host adds the shares in handle order (slabs that hold no cells are skipped).
extern "C" int tbk_dos_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double e_min, double e_step, int64_t n_e,
                             double* nos_out) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(mesh != nullptr && nos_out != nullptr, "mesh / nos is NULL");
    if (n_handles == 1) return tbk_dos(handles[0], mesh, e_min, e_step, n_e, nos_out);
    TBK_ARG(handles[0]->dim == 2 || handles[0]->dim == 3, "the density of states needs a 2- or 3-dimensional mesh");
    TBK_ARG(mesh[0] >= 1, "a mesh entry is < 1");
    TBK_ARG(n_e >= 2 && n_e <= (int64_t(1) << 20), "the energy grid needs 2 to 2^20 points");
    const int64_t n0 = mesh[0];
    const int busy = TetraSlabs(n0, n_handles).busy();
    std::vector<double> share;
    TBK_CHECK(tetra_shares(&share, (size_t)busy * (size_t)n_e));
    TBK_CHECK(run_slabs(n_handles, n0, [&](int i, int64_t lo, int64_t count) {
        return tbk_dos_slab(handles[i], mesh, lo, count, e_min, e_step, n_e, share.data() + (size_t)i * (size_t)n_e);
    }));
    tetra_add_shares(share, (size_t)busy, (size_t)n_e, nos_out);
    return TBK_OK;
}

// The projected number of states on several devices (tbk_pdos.hip): the slabs of tbk_dos_multi, every handle returning its share of
// nos[n_groups][n_e]; the host adds the shares in handle order.
extern "C" int tbk_pdos_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, const int32_t* group_offsets,
                              const int32_t* group_orbitals, int n_groups, double e_min, double e_step, int64_t n_e, double* nos_out) {
    TBK_CHECK(check_handles(handles, n_handles));
    TBK_ARG(mesh != nullptr && nos_out != nullptr, "mesh / nos is NULL");
    if (n_handles == 1) return tbk_pdos(handles[0], mesh, group_offsets, group_orbitals, n_groups, e_min, e_step, n_e, nos_out);
    TBK_ARG(handles[0]->dim == 2 || handles[0]->dim == 3, "the density of states needs a 2- or 3-dimensional mesh");
    TBK_ARG(mesh[0] >= 1, "a mesh entry is < 1");
    TBK_ARG(n_e >= 2 && n_e <= (int64_t(1) << 20), "the energy grid needs 2 to 2^20 points");
    TBK_CHECK(tbk_pdos_check_groups(handles[0]->n_orb, group_offsets, group_orbitals, n_groups));
    const int64_t n0 = mesh[0];
    const int busy = TetraSlabs(n0, n_handles).busy();
    const size_t n_out = (size_t)n_groups * (size_t)n_e;
    std::vector<double> share;
    TBK_CHECK(tetra_shares(&share, (size_t)busy * n_out));
    TBK_CHECK(run_slabs(n_handles, n0, [&](int i, int64_t lo, int64_t count) {
        return tbk_pdos_slab(handles[i], mesh, lo, count, group_offsets, group_orbitals, n_groups, e_min, e_step, n_e,
                             share.data() + (size_t)i * n_out);
    }));
    tetra_add_shares(share, (size_t)busy, n_out, nos_out);
    return TBK_OK;
}

// The transport distribution on several devices (tbk_tdf.hip): the slabs of tbk_pdos_multi for the expensive half -- every handle
// walks the eigensystem of its own planes and leaves E and the channel weights W at their place in two host arrays of the whole
// mesh -- and then ONE accumulation of the whole mesh on the first handle.  Shares of the channels, each divided and rounded by its
// handle, would add up to other bits than the one launch of a single handle; E and W of a k-point do not know their handle.
extern "C" int tbk_transport_distribution_multi(tbk_model* const* handles, int n_handles, const int32_t* mesh, double e_min, double e_step,
                                                int64_t n_e, double degeneracy, const double* scale, double* cumulative_out) {
    TBK_CHECK(check_handles(handles, n_handles));
    for (int i = 0; i < n_handles; ++i) {
        TBK_ARG(!handles[i]->kdotp, "a k.p model has no Brillouin zone");
        for (int j = 0; j < i; ++j) TBK_ARG(handles[j] != handles[i], "a handle appears twice");
    }
    TBK_ARG(mesh != nullptr && cumulative_out != nullptr, "mesh / cumulative is NULL");
    if (n_handles == 1) return tbk_transport_distribution(handles[0], mesh, e_min, e_step, n_e, degeneracy, scale, cumulative_out);
    const int dim = handles[0]->dim, n = handles[0]->n_orb;
    TBK_CHECK(tbk_tdf_check_arguments(dim, degeneracy, scale));
    int64_t nk_total = 0;
    TBK_CHECK(tbk_dos_check(dim, mesh, e_step, n_e, cumulative_out, &nk_total));
    TBK_ARG(std::isfinite(e_min), "e_min is not finite");
    const int64_t n0 = mesh[0], plane = nk_total / n0;
    const size_t G = (size_t)(dim * (dim + 1) / 2);
    std::vector<double> h_E, h_W;
    TBK_CHECK(tetra_shares(&h_E, (size_t)nk_total * n));
    TBK_CHECK(tetra_shares(&h_W, (size_t)nk_total * n * G));
    TBK_CHECK(run_slabs(n_handles, n0, [&](int i, int64_t lo, int64_t count) {
        const size_t at = (size_t)(lo * plane) * n;
        return tbk_tdf_slab(handles[i], mesh, lo, count, e_min, e_step, n_e, degeneracy, scale, TBK_TDF_WEIGHTS, h_E.data() + at, h_W.data() + at * G,
                            cumulative_out);
    }));
    return tbk_tdf_slab(handles[0], mesh, 0, n0, e_min, e_step, n_e, degeneracy, scale, TBK_TDF_ACCUMULATE, h_E.data(), h_W.data(), cumulative_out);
}

// k.p models on several devices (kdotp.py:51-100 has the same two methods as Model): the same slabs, through the k.p
// entry points of every staged copy
extern "C" int tbk_kdotp_eigenval_multi(tbk_kdotp* const* handles, int n_handles, const double* k, int64_t nk, double* E_out) {
    TBK_ARG(handles != nullptr && n_handles >= 1, "no handles");
    std::vector<tbk_model*> cores((size_t)n_handles);
    for (int i = 0; i < n_handles; ++i) {
        TBK_ARG(handles[i] != nullptr && handles[i]->core != nullptr, "a handle is NULL");
        cores[(size_t)i] = handles[i]->core;
    }
    return tbk_eigenval_multi(cores.data(), n_handles, k, nk, E_out);
}

extern "C" int tbk_kdotp_hamilton_multi(tbk_kdotp* const* handles, int n_handles, const double* k, int64_t nk, double* H_out) {
    TBK_ARG(handles != nullptr && n_handles >= 1, "no handles");
    std::vector<tbk_model*> cores((size_t)n_handles);
    for (int i = 0; i < n_handles; ++i) {
        TBK_ARG(handles[i] != nullptr && handles[i]->core != nullptr, "a handle is NULL");
        cores[(size_t)i] = handles[i]->core;
    }
    return tbk_hamilton_multi(cores.data(), n_handles, k, nk, 2, nullptr, H_out);
}

extern "C" int tbk_kdotp_eigh_multi(tbk_kdotp* const* handles, int n_handles, const double* k, int64_t nk, double* E_out,
                                    double* U_out) {
    TBK_CHECK(tbk_eigh_check_arguments(nk, 2, nullptr));
    TBK_ARG(handles != nullptr && n_handles >= 1, "no handles");
    std::vector<tbk_model*> cores((size_t)n_handles);
    for (int i = 0; i < n_handles; ++i) {
        TBK_ARG(handles[i] != nullptr && handles[i]->core != nullptr, "a handle is NULL");
        cores[(size_t)i] = handles[i]->core;
    }
    return tbk_eigh_multi(cores.data(), n_handles, k, nk, 2, nullptr, E_out, U_out);
}
