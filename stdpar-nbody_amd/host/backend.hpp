// RAII view of the HIP backend (include/nbody_hip.h) for one host System.  Every failure is fatal in
// the reference's style: message on stderr, exit(EXIT_FAILURE).  There is no CPU path behind this.
#pragma once
#include <cstdlib>
#include <iostream>
#include <type_traits>
#include <utility>
#include <vector>

#include "nbody_hip.h"
#include "system.hpp"

namespace nb {

inline void backend_check(int rc, char const* what) {
  if (rc != NBODY_OK) {
    std::cerr << "HIP backend failure in " << what << ": " << nbody_last_error() << std::endl;
    std::exit(EXIT_FAILURE);
  }
}

// One host System on `ngpus` devices.  ngpus == 1: the reference's single device, whole system.  ngpus > 1 (all-pairs only;
// the reference has no counterpart): one context per device, each owning the ABI's contiguous shard of the targets
// (nbody_shard_range) and all N sources; one host thread drives them all, asynchronously, and after every
// accelerate_step the devices exchange their position shards (nbody_allgather_positions, RCCL over xGMI).
template <typename T, int D>
class Device {
 public:
  static constexpr int dtype = std::is_same_v<T, float> ? NBODY_F32 : NBODY_F64;

  // exchange: run the collective even with one device (an explicit `--gpus 1`: the multi-GPU path on a one-GPU box)
  explicit Device(System<T, D>& host, int ngpus = 1, bool exchange = false) : host_(host), sharded_(ngpus > 1 || exchange) {
    ctx_.resize(std::size_t(ngpus), nullptr);
    view_.resize(std::size_t(ngpus));
    for (int g = 0; g < ngpus; ++g) backend_check(nbody_create(&ctx_[std::size_t(g)], dtype, D, host.n, g), "nbody_create");
    if (sharded_) {
      comm_.resize(std::size_t(ngpus), nullptr);
      backend_check(nbody_comm_create_all(comm_.data(), ngpus, nullptr), "nbody_comm_create_all");
      for (int g = 0; g < ngpus; ++g) {
        std::uint32_t first = 0, count = 0;
        nbody_shard_range(host.n, ngpus, g, &first, &count);
        backend_check(nbody_ctx_set_shard(ctx_[std::size_t(g)], first, count), "nbody_ctx_set_shard");
      }
    }
    push();
  }
  ~Device() {
    if (neighbours_) nbody_neighbours_destroy(neighbours_);
    if (knn_) nbody_knn_destroy(knn_);
    if (fof_) nbody_fof_destroy(fof_);
    if (nlist_) nbody_nlist_destroy(nlist_);
    if (hermite_) nbody_hermite_destroy(hermite_);
    if (hermite6_) nbody_hermite6_destroy(hermite6_);
    if (octree_block_) nbody_octree_block_destroy(octree_block_);
    if (octree_) nbody_octree_destroy(octree_);
    if (tree_) nbody_bvh_destroy(tree_);
    for (auto* c : comm_) nbody_comm_destroy(c);
    for (auto* c : ctx_) nbody_destroy(c);
  }
  Device(Device const&)            = delete;
  Device& operator=(Device const&) = delete;

  int ngpus() const { return int(ctx_.size()); }
  bool sharded() const { return sharded_; }
  bool multi() const { return ctx_.size() > 1; }

  // host System -> device mirrors (every device gets everything; it uses all of m and x and its own rows of v, a, ao)
  void push() {
    for (std::size_t g = 0; g < ctx_.size(); ++g) {
      backend_check(nbody_upload(ctx_[g], host_.m.data(), host_.x.data(), host_.v.data(), host_.a.data(), host_.ao.data(),
                                 host_.dt, host_.G),
                    "nbody_upload");
      backend_check(nbody_ctx_state(ctx_[g], &view_[g]), "nbody_ctx_state");
    }
  }
  // device mirrors -> host System (all five arrays: bvh permutes m too); a sharded context writes its own rows
  void pull() {
    for (std::size_t g = 0; g < ctx_.size(); ++g)
      backend_check(nbody_download(ctx_[g], g == 0 ? host_.m.data() : nullptr, host_.x.data(), host_.v.data(), host_.a.data(),
                                   host_.ao.data()),
                    "nbody_download");
  }
  void pull_positions() {
    for (auto* c : ctx_) backend_check(nbody_download(c, nullptr, host_.x.data(), nullptr, nullptr, nullptr), "nbody_download");
  }
  void sync() {
    for (auto* c : ctx_) backend_check(nbody_stream_sync(nbody_ctx_stream(c)), "nbody_stream_sync");
  }
  void* stream(std::size_t g = 0) { return nbody_ctx_stream(ctx_[g]); }

  void all_pairs_force() {
    for (std::size_t g = 0; g < ctx_.size(); ++g) backend_check(nbody_all_pairs_force(&view_[g], stream(g)), "nbody_all_pairs_force");
  }
  void all_pairs_softened_force(double eps) {
    for (std::size_t g = 0; g < ctx_.size(); ++g)
      backend_check(nbody_all_pairs_softened_force(&view_[g], eps, stream(g)), "nbody_all_pairs_softened_force");
  }
  void all_pairs_collapsed_force() {
    single("all-pairs-collapsed");
    backend_check(nbody_all_pairs_collapsed_force(&view_[0], stream()), "nbody_all_pairs_collapsed_force");
  }
  // K3 on every device's shard, then the one exchange of the path
  void accelerate_step() {
    for (std::size_t g = 0; g < ctx_.size(); ++g) backend_check(nbody_accelerate_step(&view_[g], stream(g)), "nbody_accelerate_step");
    if (!sharded_) return;
    if (multi()) backend_check(nbody_comm_group_begin(), "nbody_comm_group_begin");
    for (std::size_t g = 0; g < ctx_.size(); ++g)
      backend_check(nbody_allgather_positions(comm_[g], &view_[g], stream(g)), "nbody_allgather_positions");
    if (multi()) backend_check(nbody_comm_group_end(), "nbody_comm_group_end");
  }

  // --integrator hermite (no reference counterpart): acceleration and jerk of the uploaded state once, then one call per step
  void hermite_start(double eps) {
    single("--integrator hermite");
    if (!hermite_) backend_check(nbody_hermite_create_on(&hermite_, dtype, D, host_.n, 0), "nbody_hermite_create_on");
    backend_check(nbody_hermite_force_jerk(hermite_, &view_[0], eps, stream()), "nbody_hermite_force_jerk");
  }
  void hermite_step(double eps) { backend_check(nbody_hermite_step(hermite_, &view_[0], eps, stream()), "nbody_hermite_step"); }
  // --hermite-order 6: acceleration, jerk and snap of the uploaded state once (two evaluations), then one call per step
  void hermite6_start(double eps) {
    single("--hermite-order 6");
    if (!hermite6_) backend_check(nbody_hermite6_create_on(&hermite6_, dtype, D, host_.n, 0), "nbody_hermite6_create_on");
    backend_check(nbody_hermite6_start(hermite6_, &view_[0], eps, stream()), "nbody_hermite6_start");
  }
  void hermite6_step(double eps) { backend_check(nbody_hermite6_step(hermite6_, &view_[0], eps, stream()), "nbody_hermite6_step"); }
  // --hermite-eta ETA: block time steps; one call advances the system by dt (as many block steps as its levels ask for)
  void hermite_block_start(double eps, double eta_start, int max_level) {
    single("--hermite-eta");
    if (!hermite_) backend_check(nbody_hermite_create_on(&hermite_, dtype, D, host_.n, 0), "nbody_hermite_create_on");
    backend_check(nbody_hermite_block_start(hermite_, &view_[0], eps, eta_start, max_level, stream()), "nbody_hermite_block_start");
  }
  void hermite_block_advance(double eps, double eta) {
    backend_check(nbody_hermite_block_advance(hermite_, &view_[0], eps, eta, stream(), nullptr, nullptr), "nbody_hermite_block_advance");
  }

  // System::calc_energies (src/system.h:62-79) on the device: {kinetic, potential}
  // softening > 0: the potential of the softened force (nbody_calc_energies_softened)
  std::pair<T, T> calc_energies(double softening = 0.0) {
    single("--save energy");
    T ke{}, pe{};
    if (softening > 0.0) backend_check(nbody_calc_energies_softened(&view_[0], softening, &ke, &pe, stream()), "nbody_calc_energies_softened");
    else backend_check(nbody_calc_energies(&view_[0], &ke, &pe, stream()), "nbody_calc_energies");
    return {ke, pe};
  }

  // --save-neighbours: per-body potentials, nearest neighbours and their squared distances of the current (m, x), into the host
  // vectors (nbody_neighbours_*; the reads are blocking)
  void neighbours(double eps, std::vector<T>& phi, std::vector<std::uint32_t>& nn, std::vector<T>& nnd2) {
    single("--save-neighbours");
    if (!neighbours_) backend_check(nbody_neighbours_create_on(&neighbours_, dtype, D, host_.n, 0), "nbody_neighbours_create_on");
    backend_check(nbody_neighbours_compute(neighbours_, &view_[0], eps, stream()), "nbody_neighbours_compute");
    phi.resize(host_.n);
    nn.resize(host_.n);
    nnd2.resize(host_.n);
    backend_check(nbody_neighbours_read(neighbours_, 0, phi.data(), phi.size() * sizeof(T), stream()), "nbody_neighbours_read");
    backend_check(nbody_neighbours_read(neighbours_, 1, nn.data(), nn.size() * sizeof(std::uint32_t), stream()), "nbody_neighbours_read");
    backend_check(nbody_neighbours_read(neighbours_, 2, nnd2.data(), nnd2.size() * sizeof(T), stream()), "nbody_neighbours_read");
  }

  // --save-density K: the local densities from the K-th neighbour of the current (m, x) into rho, and {x_dc[D], r_c, rho_c} into
  // summary (nbody_knn_*; the reads are blocking).  tree (--density-tree): the tree-pruned method, the same bits.
  void density(int k, bool tree, std::vector<T>& rho, T (&summary)[D + 2]) {
    single("--save-density");
    if (!knn_)
      backend_check(nbody_knn_create_method(&knn_, dtype, D, host_.n, k, tree ? NBODY_KNN_TREE : NBODY_KNN_ALL_PAIRS, 0),
                    "nbody_knn_create_method");
    backend_check(nbody_knn_compute(knn_, &view_[0], stream()), "nbody_knn_compute");
    rho.resize(host_.n);
    backend_check(nbody_knn_read(knn_, 2, rho.data(), rho.size() * sizeof(T), stream()), "nbody_knn_read");
    backend_check(nbody_knn_density_centre(knn_, &summary[0], &summary[D], &summary[D + 1], stream()), "nbody_knn_density_centre");
  }

  // --save-groups B: the friends-of-friends groups of the current x for the linking length b (nbody_fof_*; the reads are blocking):
  // the summary, label and size of every body, and the catalogue of the groups of at least min_members bodies
  void groups(double b, std::uint32_t min_members, std::uint32_t (&summary)[4], std::vector<std::uint32_t>& label,
              std::vector<std::uint32_t>& size, std::vector<std::uint32_t>& cat_label, std::vector<std::uint32_t>& cat_size,
              std::vector<T>& cat_mass, std::vector<T>& cat_com) {
    single("--save-groups");
    if (!fof_) backend_check(nbody_fof_create_on(&fof_, dtype, D, host_.n, min_members, 0), "nbody_fof_create_on");
    backend_check(nbody_fof_compute(fof_, &view_[0], b, stream()), "nbody_fof_compute");
    backend_check(nbody_fof_summary(fof_, summary, stream()), "nbody_fof_summary");
    label.resize(host_.n);
    size.resize(host_.n);
    backend_check(nbody_fof_read(fof_, 0, label.data(), label.size() * sizeof(std::uint32_t), stream()), "nbody_fof_read");
    backend_check(nbody_fof_read(fof_, 1, size.data(), size.size() * sizeof(std::uint32_t), stream()), "nbody_fof_read");
    std::size_t const c = summary[1];
    cat_label.resize(c);
    cat_size.resize(c);
    cat_mass.resize(c);
    cat_com.resize(c * D);
    backend_check(nbody_fof_read(fof_, 2, cat_label.data(), c * sizeof(std::uint32_t), stream()), "nbody_fof_read");
    backend_check(nbody_fof_read(fof_, 3, cat_size.data(), c * sizeof(std::uint32_t), stream()), "nbody_fof_read");
    backend_check(nbody_fof_read(fof_, 4, cat_mass.data(), c * sizeof(T), stream()), "nbody_fof_read");
    backend_check(nbody_fof_read(fof_, 5, cat_com.data(), c * D * sizeof(T), stream()), "nbody_fof_read");
  }

  // --save-lists R: the exact fixed-radius neighbour lists of the current x for the radius r (nbody_nlist_*; the reads are blocking):
  // the summary, the count of every body and, when the summary's status is 0, the lists (else `list` comes back empty)
  void lists(double r, std::uint64_t capacity, std::uint64_t (&summary)[4], std::vector<std::uint32_t>& count, std::vector<std::uint32_t>& list) {
    single("--save-lists");
    if (!nlist_) backend_check(nbody_nlist_create_on(&nlist_, dtype, D, host_.n, capacity, 0), "nbody_nlist_create_on");
    backend_check(nbody_nlist_compute(nlist_, &view_[0], r, stream()), "nbody_nlist_compute");
    backend_check(nbody_nlist_summary(nlist_, summary, stream()), "nbody_nlist_summary");
    count.resize(host_.n);
    backend_check(nbody_nlist_read(nlist_, 0, count.data(), count.size() * sizeof(std::uint32_t), stream()), "nbody_nlist_read");
    list.resize(summary[3] == 0 ? std::size_t(summary[0]) : 0);
    if (summary[3] == 0) backend_check(nbody_nlist_read(nlist_, 2, list.data(), list.size() * sizeof(std::uint32_t), stream()), "nbody_nlist_read");
  }

  // Record the phase calls issued by `step` once and return a replayable graph of them (one submission per step).
  template <typename F>
  nbody_graph* record(F&& step) {
    single("step graphs");
    nbody_graph* g = nullptr;
    backend_check(nbody_graph_begin(stream()), "nbody_graph_begin");
    step();
    backend_check(nbody_graph_end(stream(), &g), "nbody_graph_end");
    return g;
  }
  void replay(nbody_graph* g) { backend_check(nbody_graph_launch(g, stream()), "nbody_graph_launch"); }

  void bvh_alloc() {
    single("bvh");
    if (!tree_) backend_check(nbody_bvh_create_on(&tree_, dtype, D, host_.n, 0), "nbody_bvh_create_on");
  }
  void bvh_bounding_box() { backend_check(nbody_bvh_bounding_box(tree_, &view_[0], stream()), "nbody_bvh_bounding_box"); }
  void bvh_hilbert_sort() { backend_check(nbody_bvh_hilbert_sort(tree_, &view_[0], stream()), "nbody_bvh_hilbert_sort"); }
  void bvh_build_tree() { backend_check(nbody_bvh_build_tree(tree_, &view_[0], stream()), "nbody_bvh_build_tree"); }
  void bvh_compute_force(double theta) {
    backend_check(nbody_bvh_compute_force(tree_, &view_[0], theta, stream()), "nbody_bvh_compute_force");
  }
  // octree phases (src/octree.h)
  void octree_alloc() {
    single("octree");
    if (!octree_) backend_check(nbody_octree_create_on(&octree_, dtype, D, host_.n, 0), "nbody_octree_create_on");
  }
  void octree_clear() { backend_check(nbody_octree_clear(octree_, stream()), "nbody_octree_clear"); }
  void octree_compute_bounds() { backend_check(nbody_octree_compute_bounds(octree_, &view_[0], stream()), "nbody_octree_compute_bounds"); }
  void octree_insert() { backend_check(nbody_octree_insert(octree_, &view_[0], stream()), "nbody_octree_insert"); }
  void octree_compute_tree() { backend_check(nbody_octree_compute_tree(octree_, stream()), "nbody_octree_compute_tree"); }
  void octree_compute_quadrupoles() {
    backend_check(nbody_octree_compute_quadrupoles(octree_, stream()), "nbody_octree_compute_quadrupoles");
  }
  void octree_compute_quadrupole_force(double theta) {
    backend_check(nbody_octree_compute_quadrupole_force(octree_, &view_[0], theta, stream()), "nbody_octree_compute_quadrupole_force");
  }
  void octree_compute_force(double theta, double softening = 0.0) {
    if (softening > 0.0)
      backend_check(nbody_octree_compute_softened_force(octree_, &view_[0], theta, softening, stream()),
                    "nbody_octree_compute_softened_force");
    else backend_check(nbody_octree_compute_force(octree_, &view_[0], theta, stream()), "nbody_octree_compute_force");
  }
  // --tree-energy: {kinetic, potential} from a tree built on the current positions (the next step builds its own again), with the
  // potential of the run's force: monopole, softened or quadrupole (nbody_octree_calc_energies; blocking)
  std::pair<T, T> octree_energies(double theta, double softening, bool quadrupole) {
    octree_alloc();
    octree_clear();
    octree_compute_bounds();
    octree_insert();
    octree_compute_tree();
    if (quadrupole) octree_compute_quadrupoles();
    T ke{}, pe{};
    backend_check(nbody_octree_calc_energies(octree_, &view_[0], theta, softening, quadrupole ? 1 : 0, &ke, &pe, stream()),
                  "nbody_octree_calc_energies");
    return {ke, pe};
  }
  // --block-eta ETA: block time steps of the octree leapfrog; one advance moves the system by dt (as many block steps as its levels ask for)
  void octree_block_start(double theta, double eps, double eta, int max_level) {
    octree_alloc();
    if (!octree_block_) backend_check(nbody_octree_block_create_on(&octree_block_, dtype, D, host_.n, 0), "nbody_octree_block_create_on");
    backend_check(nbody_octree_block_start(octree_block_, octree_, &view_[0], theta, eps, eta, max_level, stream()), "nbody_octree_block_start");
  }
  void octree_block_advance(double theta, double eps, double eta) {
    backend_check(nbody_octree_block_advance(octree_block_, octree_, &view_[0], theta, eps, eta, stream(), nullptr, nullptr),
                  "nbody_octree_block_advance");
  }
  // {tree size, total mass}; also where device-side build errors (depth limit, node pool) surface
  std::pair<std::uint32_t, T> octree_info() {
    std::uint32_t size = 0;
    T mass{};
    backend_check(nbody_octree_info(octree_, &size, &mass, stream()), "nbody_octree_info");
    return {size, mass};
  }

  // mass of the root monopole, for --print-info (src/bvh.h:377)
  T bvh_total_mass() {
    std::vector<T> nodes(std::size_t(nbody_bvh_nnodes(tree_)) * (D + 1));
    backend_check(nbody_bvh_read(tree_, 2, nodes.data(), nodes.size() * sizeof(T), stream()), "nbody_bvh_read");
    return nodes[D];
  }

 private:
  // bodies shard over GPUs for all-pairs only (north_star); everything else runs on one device
  void single(char const* what) const {
    if (sharded_) {
      std::cerr << what << " runs on one GPU only (bodies shard over --gpus N for --algorithm all-pairs)" << std::endl;
      std::exit(EXIT_FAILURE);
    }
  }
  System<T, D>& host_;
  bool sharded_ = false;
  std::vector<nbody_ctx*> ctx_;
  std::vector<nbody_comm*> comm_;
  std::vector<nbody_state> view_;
  nbody_bvh* tree_ = nullptr;
  nbody_octree* octree_ = nullptr;
  nbody_hermite* hermite_ = nullptr;
  nbody_hermite6* hermite6_ = nullptr;
  nbody_octree_block* octree_block_ = nullptr;
  nbody_neighbours* neighbours_ = nullptr;
  nbody_knn* knn_               = nullptr;
  nbody_fof* fof_               = nullptr;
  nbody_nlist* nlist_           = nullptr;
};

}  // namespace nb
