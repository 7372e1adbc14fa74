// positions.bin / energy.bin writers in the reference's on-disk format (src/saving.h:85-122):
//   positions.bin: u32 nbodies, u32 steps, u32 sizeof(T), u32 dim, then one frame of x per save_all
//   energy.bin:    u32 steps, u32 sizeof(T), then (kinetic, potential) per save_all
// and, with --save-neighbours (no reference counterpart), in the same style
//   neighbours.bin: u32 nbodies, u32 steps, u32 sizeof(T), u32 dim, then per save_all phi T[n], nn u32[n], nnd2 T[n]
// and, with --save-density K,
//   density.bin:    u32 nbodies, u32 steps, u32 sizeof(T), u32 dim, u32 k, then per save_all rho T[n], x_dc T[dim], r_c T, rho_c T
// and, with --save-groups B (--groups-min M),
//   groups.bin:     u32 nbodies, u32 steps, u32 sizeof(T), u32 dim, f64 b, u32 min_members, then per save_all the u32[4] summary
//                   (groups, catalogued groups c, largest size, its label), label u32[n], size u32[n], then c entries of
//                   {u32 label, u32 size, T mass, T com[dim]}
// and, with --save-lists R (--lists-capacity C),
//   lists.bin:      u32 nbodies, u32 steps, u32 sizeof(T), u32 dim, f64 r, u64 capacity, then per save_all the u64[4] summary (total,
//                   largest count, the lowest index that has it, status), count u32[n], then list u32[total] if the status is 0
#pragma once
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <vector>

#include "backend.hpp"
#include "options.hpp"

namespace nb {

template <typename T, int D>
class Saver {
 public:
  explicit Saver(Options const& o)
   : pos_(o.save_pos), energy_(o.save_energy), tree_energy_(o.tree_energy), quadrupole_(o.quadrupole), softening_(o.softening),
     neighbours_(o.save_neighbours), density_k_(o.save_density), density_tree_(o.density_tree), groups_(o.save_groups), groups_b_(o.groups_b),
     groups_min_(std::uint32_t(o.groups_min)), lists_(o.save_lists), lists_r_(o.lists_r), lists_capacity_(o.lists_capacity), theta_(o.theta), nbodies_(std::uint32_t(o.size)), nsteps_(std::uint32_t(o.steps)) {
    std::uint32_t const tsz = sizeof(T), dim = D;
    if (pos_) {
      pos_file_.open("positions.bin", std::ios::out | std::ios::binary);
      put(pos_file_, nbodies_);
      put(pos_file_, nsteps_);
      put(pos_file_, tsz);
      put(pos_file_, dim);
    }
    if (energy_) {
      energy_file_.open("energy.bin", std::ios::out | std::ios::binary);
      put(energy_file_, nsteps_);
      put(energy_file_, tsz);
    }
    if (neighbours_) {
      neighbours_file_.open("neighbours.bin", std::ios::out | std::ios::binary);
      put(neighbours_file_, nbodies_);
      put(neighbours_file_, nsteps_);
      put(neighbours_file_, tsz);
      put(neighbours_file_, dim);
    }
    if (density_k_ != 0) {
      std::uint32_t const k = std::uint32_t(density_k_);
      density_file_.open("density.bin", std::ios::out | std::ios::binary);
      put(density_file_, nbodies_);
      put(density_file_, nsteps_);
      put(density_file_, tsz);
      put(density_file_, dim);
      put(density_file_, k);
    }
    if (groups_) {
      groups_file_.open("groups.bin", std::ios::out | std::ios::binary);
      put(groups_file_, nbodies_);
      put(groups_file_, nsteps_);
      put(groups_file_, tsz);
      put(groups_file_, dim);
      put(groups_file_, groups_b_);
      put(groups_file_, groups_min_);
    }
    if (lists_) {
      lists_file_.open("lists.bin", std::ios::out | std::ios::binary);
      put(lists_file_, nbodies_);
      put(lists_file_, nsteps_);
      put(lists_file_, tsz);
      put(lists_file_, dim);
      put(lists_file_, lists_r_);
      put(lists_file_, lists_capacity_);
    }
  }

  bool active() const { return pos_ || energy_ || neighbours_ || density_k_ != 0 || groups_ || lists_; }

  // one frame; the device copy is authoritative, so positions are pulled first
  void save_all(System<T, D>& sys, Device<T, D>& dev) {
    if (pos_) {
      dev.pull_positions();
      pos_file_.write(reinterpret_cast<char const*>(sys.x.data()), std::streamsize(std::size_t(nbodies_) * sizeof(T) * D));
    }
    if (energy_) {
      auto [kinetic, potential] = tree_energy_ ? dev.octree_energies(theta_, softening_, quadrupole_) : dev.calc_energies(softening_);
      put(energy_file_, kinetic);
      put(energy_file_, potential);
    }
    if (neighbours_) {
      dev.neighbours(softening_, phi_, nn_, nnd2_);
      neighbours_file_.write(reinterpret_cast<char const*>(phi_.data()), std::streamsize(phi_.size() * sizeof(T)));
      neighbours_file_.write(reinterpret_cast<char const*>(nn_.data()), std::streamsize(nn_.size() * sizeof(std::uint32_t)));
      neighbours_file_.write(reinterpret_cast<char const*>(nnd2_.data()), std::streamsize(nnd2_.size() * sizeof(T)));
    }
    if (density_k_ != 0) {
      T summary[D + 2];  // x_dc, r_c, rho_c
      dev.density(density_k_, density_tree_, rho_, summary);
      density_file_.write(reinterpret_cast<char const*>(rho_.data()), std::streamsize(rho_.size() * sizeof(T)));
      density_file_.write(reinterpret_cast<char const*>(summary), std::streamsize(sizeof summary));
    }
    if (groups_) {
      std::uint32_t summary[4];
      dev.groups(groups_b_, groups_min_, summary, label_, size_, cat_label_, cat_size_, cat_mass_, cat_com_);
      groups_file_.write(reinterpret_cast<char const*>(summary), std::streamsize(sizeof summary));
      groups_file_.write(reinterpret_cast<char const*>(label_.data()), std::streamsize(label_.size() * sizeof(std::uint32_t)));
      groups_file_.write(reinterpret_cast<char const*>(size_.data()), std::streamsize(size_.size() * sizeof(std::uint32_t)));
      for (std::size_t e = 0; e < cat_label_.size(); ++e) {
        put(groups_file_, cat_label_[e]);
        put(groups_file_, cat_size_[e]);
        put(groups_file_, cat_mass_[e]);
        groups_file_.write(reinterpret_cast<char const*>(&cat_com_[e * D]), std::streamsize(sizeof(T) * D));
      }
    }
    if (lists_) {
      std::uint64_t summary[4];
      dev.lists(lists_r_, lists_capacity_, summary, count_, list_);  // list_ is empty when the status is not 0
      lists_file_.write(reinterpret_cast<char const*>(summary), std::streamsize(sizeof summary));
      lists_file_.write(reinterpret_cast<char const*>(count_.data()), std::streamsize(count_.size() * sizeof(std::uint32_t)));
      lists_file_.write(reinterpret_cast<char const*>(list_.data()), std::streamsize(list_.size() * sizeof(std::uint32_t)));
    }
  }

 private:
  template <typename U>
  static void put(std::ofstream& f, U const& v) {
    f.write(reinterpret_cast<char const*>(&v), sizeof v);
  }
  bool pos_, energy_;
  bool tree_energy_, quadrupole_;  // --tree-energy: the octree's energies at theta_, with the --quadrupole term if the run has it
  double softening_;               // --softening: the energies of the softened dynamics
  bool neighbours_;                // --save-neighbours: phi, nn, nnd2 of every recorded frame, softening_ the potential's length
  int density_k_;                  // --save-density K: rho and the density-centre summary of every recorded frame; 0: off
  bool density_tree_;              // --density-tree: by the tree-pruned method (the same bytes)
  bool groups_;                    // --save-groups B: the friends-of-friends groups of every recorded frame
  double groups_b_;                // ... its linking length
  std::uint32_t groups_min_;       // --groups-min M: the smallest group the catalogue lists
  bool lists_;                     // --save-lists R: the fixed-radius neighbour lists of every recorded frame
  double lists_r_;                 // ... its radius
  std::uint64_t lists_capacity_;   // --lists-capacity C: the list entries a frame may hold
  double theta_;
  std::uint32_t nbodies_, nsteps_;
  std::ofstream pos_file_, energy_file_, neighbours_file_, density_file_, groups_file_, lists_file_;
  std::vector<T> phi_, nnd2_, rho_;
  std::vector<std::uint32_t> nn_, label_, size_, cat_label_, cat_size_, count_, list_;
  std::vector<T> cat_mass_, cat_com_;
};

}  // namespace nb
