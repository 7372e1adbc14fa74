// Command line of the reference binary (src/arguments.h): same flags, defaults, help and error text.
#pragma once
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <optional>
#include <limits>
#include <string>
#include <vector>

namespace nb {

enum class Workload { Uniform, Plummer, Galaxy, Load };
enum class Algorithm { AllPairs, AllPairsCollapsed, Octree, Bvh };
enum class Integrator { Leapfrog, Hermite };

struct Options {
  std::size_t size         = 1000;
  std::size_t steps        = 1;
  std::size_t warmup_steps = 10;  // no flag sets it (src/arguments.h:26)
  bool single_precision    = true;
  Workload workload        = Workload::Uniform;
  Algorithm algorithm      = Algorithm::Octree;
  bool print_state         = false;
  bool print_info          = false;
  double theta             = 0.5;
  bool save_pos            = false;
  bool save_energy         = false;
  bool csv_detailed        = false;
  bool csv_total           = false;
  std::optional<std::string> load_input;
  // not in the reference (and therefore not in the --help text, which stays the reference's word for word): --gpus N shards
  // the bodies of --algorithm all-pairs over N devices of this node, one RCCL all-gather of positions per step
  int gpus = 1;
  bool gpus_given = false;  // an explicit --gpus N (any N, also 1) takes the sharded path: communicator, shard windows, exchange
  // not in the reference either (nor in --help): --softening EPS, Plummer softening length for all-pairs (also under --gpus N),
  // octree and --save energy; 0 = off, the same run as without the flag
  double softening = 0.0;
  // not in the reference either (nor in --help): --quadrupole, octree cells also add their quadrupole term (octree only, unsoftened)
  bool quadrupole = false;
  // not in the reference either (nor in --help): --tree-energy, --save energy|all records the octree's energies at the run's --theta,
  // with the potential that matches the run's force (monopole, --softening or --quadrupole), instead of the exact O(N^2) sum
  bool tree_energy = false;
  // not in the reference either (nor in --help): --integrator leapfrog|hermite.  leapfrog (default): the reference's step, the same
  // run as without the flag.  hermite: the fourth-order predictor-corrector with force + jerk (nbody_hermite_*); all-pairs on one
  // GPU with --softening EPS > 0 only
  Integrator integrator = Integrator::Leapfrog;
  // not in the reference either (nor in --help): --hermite-eta ETA (with --integrator hermite only, ETA > 0) switches the Hermite
  // integrator to block time steps with accuracy parameter ETA (nbody_hermite_block_*): every step of the run advances the system by
  // dt in as many block steps as the bodies' levels ask for; --hermite-levels L (0 .. 20, default 12): the smallest step is dt / 2^L
  double hermite_eta = 0.0;  // 0: fixed step
  int hermite_levels = 12;
  bool hermite_levels_given = false;
  // not in the reference either (nor in --help): --hermite-order 4|6 (with --integrator hermite only, default 4).  6: the sixth-order
  // scheme with force + jerk + snap (nbody_hermite6_*), fixed step only (no --hermite-eta)
  int hermite_order = 4;
  bool hermite_order_given = false;
  // not in the reference either (nor in --help): --block-eta ETA (octree with --softening EPS > 0 only, ETA > 0) runs the octree
  // leapfrog with block time steps (nbody_octree_block_*): every step of the run advances the system by dt in as many block steps as
  // the bodies' levels ask for, each body on the power-of-two step its acceleration allows; --block-levels L (0 .. 20, default 12):
  // the smallest step is dt / 2^L
  double block_eta = 0.0;  // 0: one shared step
  int block_levels = 12;
  bool block_levels_given = false;
  // not in the reference either (nor in --help): --save-neighbours, at every frame the run's Saver records, the per-body potentials,
  // nearest neighbours and their squared distances (nbody_neighbours_*) are appended to neighbours.bin; independent of --save; one
  // GPU, with --softening EPS > 0 (the potential's softening length)
  bool save_neighbours = false;
  // not in the reference either (nor in --help): --save-density K (2 .. 16), at every frame the run's Saver records, the local
  // densities from the K-th neighbour, the density centre, the core radius and the core density (nbody_knn_*) are appended to
  // density.bin; independent of --save and of the algorithm (all-pairs kNN whatever --algorithm is, unless --density-tree), needs no
  // --softening; one GPU
  int save_density = 0;  // 0: off
  // not in the reference either (nor in --help): --density-tree, --save-density K uses the tree-pruned exact method
  // (NBODY_KNN_TREE: the same density.bin byte for byte, for the large runs of the tree codes); needs --save-density
  bool density_tree = false;
  // not in the reference either (nor in --help): --save-groups B (a linking length, finite and >= 0), at every frame the run's Saver
  // records, the friends-of-friends groups of the positions (nbody_fof_*: summary, labels, sizes and the catalogue of the groups of
  // at least --groups-min M bodies, default 20) are appended to groups.bin; independent of --save and of the algorithm; one GPU
  bool save_groups     = false;
  double groups_b      = 0.0;
  long groups_min      = 20;
  bool groups_min_given = false;
  // not in the reference either (nor in --help): --save-lists R (a radius, finite and >= 0), at every frame the run's Saver records,
  // the exact fixed-radius neighbour lists of the positions (nbody_nlist_*: summary, counts and, if they fit, the lists) are
  // appended to lists.bin; --lists-capacity C (0 .. 2^32, default 64 n): the list entries a frame may hold; independent of --save and
  // of the algorithm; one GPU
  bool save_lists            = false;
  double lists_r             = 0.0;
  unsigned long long lists_capacity = 0;
  bool lists_capacity_given  = false;
};

namespace detail {
inline constexpr char const* kHelp =
 "Help:\n"
 "-n size\t\tNumber of particles to simulate\n"
 "-s steps\t\tNumber of steps to run simulation for\n"
 "--theta t\t\tTheta threshold parameter to use in Octree\n"
 "--precision double|float(default)\t\tSelects floating-point precision\n"
 "--algorithm all-pairs|all-pairs-collapsed|bvh|octree(default)<algo>\t\tSelects simulation algorithm\n"
 "--workload plummer|galaxy|uniform(default)|load <file.bin>\t\tSelects workload\n"
 "--print-state\t\tPrint the initial and final state of the simulation\n"
 "--print-info\t\tPrint info every timestep\n"
 "--save pos|energy|all|none(default) \t\tSelects what data to save every timestep\n"
 "--help\t\tDisplay this help message and quit\n";

[[noreturn]] inline void reject(char const* what, std::string const& got, char const* choices) {
  std::cerr << "Unknown " << what << ": \"" << got << "\"." << std::endl;
  std::cerr << "Options are: " << choices << "." << std::endl;
  std::exit(EXIT_FAILURE);
}
}  // namespace detail

inline Options parse_options(std::vector<std::string> const& argv) {
  Options o;
  for (std::size_t k = 0; k < argv.size(); ++k) {
    std::string const& f = argv[k];
    auto value           = [&]() -> std::string const& { return argv.at(++k); };  // missing value -> std::out_of_range
    if (f == "-n") {
      o.size = std::stoi(value());
    } else if (f == "-s") {
      o.steps = std::stoi(value());
    } else if (f == "--theta") {
      o.theta = std::stod(value());
    } else if (f == "--csv-detailed") {
      o.csv_detailed = true;
    } else if (f == "--csv-total") {
      o.csv_total = true;
    } else if (f == "--precision") {
      auto const& p = value();
      if (p == "float") o.single_precision = true;
      else if (p == "double") o.single_precision = false;
      else detail::reject("precision", p, "double, float (default)");
    } else if (f == "--algorithm") {
      auto const& a = value();
      if (a == "all-pairs") o.algorithm = Algorithm::AllPairs;
      else if (a == "all-pairs-collapsed") o.algorithm = Algorithm::AllPairsCollapsed;
      else if (a == "octree") o.algorithm = Algorithm::Octree;
      else if (a == "bvh") o.algorithm = Algorithm::Bvh;
      else detail::reject("algorithm", a, "all-pairs, all-pairs-collapsed, octree (default)");
    } else if (f == "--workload") {
      auto const& w = value();
      if (w == "plummer") o.workload = Workload::Plummer;
      else if (w == "galaxy") o.workload = Workload::Galaxy;
      else if (w == "uniform") o.workload = Workload::Uniform;
      else if (w == "load") {
        o.load_input = value();
        o.workload   = Workload::Load;
      } else detail::reject("workload", w, "plummer, galaxy, uniform (default)");
    } else if (f == "--gpus") {
      o.gpus = std::stoi(value());
      o.gpus_given = true;
      if (o.gpus < 1) {
        std::cerr << "--gpus needs a positive device count." << std::endl;
        std::exit(EXIT_FAILURE);
      }
    } else if (f == "--softening") {
      auto const& e = value();
      char* end     = nullptr;
      double const v = std::strtod(e.c_str(), &end);
      if (e.empty() || end != e.c_str() + e.size() || !std::isfinite(v) || v < 0.0) {
        std::cerr << "--softening needs a finite length >= 0 (0 = off), got \"" << e << "\"." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.softening = v;
    } else if (f == "--integrator") {
      auto const& i = value();
      if (i == "leapfrog") o.integrator = Integrator::Leapfrog;
      else if (i == "hermite") o.integrator = Integrator::Hermite;
      else detail::reject("integrator", i, "leapfrog (default), hermite");
    } else if (f == "--hermite-eta") {
      auto const& e = value();
      char* end     = nullptr;
      double const v = std::strtod(e.c_str(), &end);
      if (e.empty() || end != e.c_str() + e.size() || !std::isfinite(v) || !(v > 0.0)) {
        std::cerr << "--hermite-eta needs a finite accuracy parameter > 0, got \"" << e << "\"." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.hermite_eta = v;
    } else if (f == "--hermite-levels") {
      auto const& l = value();
      char* end     = nullptr;
      long const v  = std::strtol(l.c_str(), &end, 10);
      if (l.empty() || end != l.c_str() + l.size() || v < 0 || v > 20) {
        std::cerr << "--hermite-levels needs a level count in 0 .. 20, got \"" << l << "\"." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.hermite_levels       = int(v);
      o.hermite_levels_given = true;
    } else if (f == "--hermite-order") {
      auto const& r = value();
      if (r != "4" && r != "6") {
        std::cerr << "--hermite-order needs 4 or 6, got \"" << r << "\"." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.hermite_order       = r == "6" ? 6 : 4;
      o.hermite_order_given = true;
    } else if (f == "--block-eta") {
      auto const& e = value();
      char* end     = nullptr;
      double const v = std::strtod(e.c_str(), &end);
      if (e.empty() || end != e.c_str() + e.size() || !std::isfinite(v) || !(v > 0.0)) {
        std::cerr << "--block-eta needs a finite accuracy parameter > 0, got \"" << e << "\"." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.block_eta = v;
    } else if (f == "--block-levels") {
      auto const& l = value();
      char* end     = nullptr;
      long const v  = std::strtol(l.c_str(), &end, 10);
      if (l.empty() || end != l.c_str() + l.size() || v < 0 || v > 20) {
        std::cerr << "--block-levels needs a level count in 0 .. 20, got \"" << l << "\"." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.block_levels       = int(v);
      o.block_levels_given = true;
    } else if (f == "--quadrupole") {
      o.quadrupole = true;
    } else if (f == "--tree-energy") {
      o.tree_energy = true;
    } else if (f == "--save-neighbours") {
      o.save_neighbours = true;
    } else if (f == "--save-density") {
      std::string const l = k + 1 < argv.size() ? argv[++k] : std::string();
      char* end           = nullptr;
      long const v        = std::strtol(l.c_str(), &end, 10);
      if (l.empty() || end != l.c_str() + l.size() || v < 2 || v > 16) {
        std::cerr << "--save-density needs a neighbour count K in 2 .. 16." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.save_density = int(v);
    } else if (f == "--density-tree") {
      o.density_tree = true;
    } else if (f == "--save-groups") {
      std::string const l = k + 1 < argv.size() ? argv[++k] : std::string();
      char* end           = nullptr;
      double const v      = std::strtod(l.c_str(), &end);
      if (l.empty() || end != l.c_str() + l.size() || !(v >= 0.0) || !(v <= std::numeric_limits<double>::max())) {
        std::cerr << "--save-groups needs a linking length B, finite and >= 0." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.save_groups = true;
      o.groups_b    = v;
    } else if (f == "--groups-min") {
      std::string const l = k + 1 < argv.size() ? argv[++k] : std::string();
      char* end           = nullptr;
      long const v        = std::strtol(l.c_str(), &end, 10);
      if (l.empty() || end != l.c_str() + l.size() || v < 1) {
        std::cerr << "--groups-min needs a member count M >= 1." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.groups_min       = v;
      o.groups_min_given = true;
    } else if (f == "--save-lists") {
      std::string const l = k + 1 < argv.size() ? argv[++k] : std::string();
      char* end           = nullptr;
      double const v      = std::strtod(l.c_str(), &end);
      if (l.empty() || end != l.c_str() + l.size() || !(v >= 0.0) || !(v <= std::numeric_limits<double>::max())) {
        std::cerr << "--save-lists needs a radius R, finite and >= 0." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.save_lists = true;
      o.lists_r    = v;
    } else if (f == "--lists-capacity") {
      std::string const l = k + 1 < argv.size() ? argv[++k] : std::string();
      char* end           = nullptr;
      unsigned long long const v = std::strtoull(l.c_str(), &end, 10);
      if (l.empty() || l[0] < '0' || l[0] > '9' || end != l.c_str() + l.size() || v > (1ull << 32)) {
        std::cerr << "--lists-capacity needs an entry count C in 0 .. 2^32." << std::endl;
        std::exit(EXIT_FAILURE);
      }
      o.lists_capacity       = v;
      o.lists_capacity_given = true;
    } else if (f == "--print-state") {
      o.print_state = true;
    } else if (f == "--print-info") {
      o.print_info = true;
    } else if (f == "--save") {
      auto const& s = value();
      if (s == "pos") o.save_pos = true;
      else if (s == "energy") o.save_energy = true;
      else if (s == "all") o.save_pos = o.save_energy = true;
      else if (s == "none") o.save_pos = o.save_energy = false;
      else detail::reject("save options", s, "pos, energy, all, none (default)");
    } else if (f == "--help" || f == "-h") {
      std::cout << detail::kHelp;
      std::exit(EXIT_SUCCESS);
    } else {
      std::cout << "Unknown argument: '" << f << "'\n";
      std::exit(EXIT_FAILURE);
    }
  }
  if (o.csv_detailed && o.csv_total) {
    std::cerr << "Cannot capture a CSV detailed and coarse trace in the same run. Specify one or the other." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.save_neighbours) {
    if (!(o.softening > 0.0)) {
      std::cerr << "--save-neighbours needs --softening EPS with EPS > 0." << std::endl;
      std::exit(EXIT_FAILURE);
    }
    if (o.gpus_given) {
      std::cerr << "--save-neighbours runs on one GPU: it cannot be combined with --gpus." << std::endl;
      std::exit(EXIT_FAILURE);
    }
  }
  if (o.save_density != 0 && o.gpus_given) {
    std::cerr << "--save-density runs on one GPU: it cannot be combined with --gpus." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.density_tree && o.save_density == 0) {
    std::cerr << "--density-tree needs --save-density K." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.groups_min_given && !o.save_groups) {
    std::cerr << "--groups-min needs --save-groups B." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.save_groups && o.gpus_given) {
    std::cerr << "--save-groups runs on one GPU: it cannot be combined with --gpus." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.save_groups && (o.size < 1 || o.groups_min > long(o.size))) {
    std::cerr << "--groups-min M must not exceed the number of bodies (M = " << o.groups_min << ")." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.lists_capacity_given && !o.save_lists) {
    std::cerr << "--lists-capacity needs --save-lists R." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.save_lists && o.gpus_given) {
    std::cerr << "--save-lists runs on one GPU: it cannot be combined with --gpus." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.save_lists && !o.lists_capacity_given) o.lists_capacity = 64ull * o.size;
  if (o.save_lists && o.lists_capacity > (1ull << 32)) o.lists_capacity = 1ull << 32;
  if (o.block_levels_given && !(o.block_eta > 0.0)) {
    std::cerr << "--block-levels needs --block-eta ETA." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.block_eta > 0.0) {  // block time steps of the octree leapfrog: softened monopole walk, one GPU
    if (o.algorithm != Algorithm::Octree) {
      std::cerr << "--block-eta is supported by --algorithm octree only." << std::endl;
      std::exit(EXIT_FAILURE);
    }
    if (o.integrator == Integrator::Hermite) {
      std::cerr << "--block-eta steps the octree leapfrog: it cannot be combined with --integrator hermite." << std::endl;
      std::exit(EXIT_FAILURE);
    }
    if (o.quadrupole) {
      std::cerr << "--block-eta takes the softened monopole walk: it cannot be combined with --quadrupole." << std::endl;
      std::exit(EXIT_FAILURE);
    }
    if (!(o.softening > 0.0)) {
      std::cerr << "--block-eta needs --softening EPS with EPS > 0." << std::endl;
      std::exit(EXIT_FAILURE);
    }
    if (o.gpus_given) {
      std::cerr << "--block-eta runs on one GPU: it cannot be combined with --gpus." << std::endl;
      std::exit(EXIT_FAILURE);
    }
  }
  if (o.integrator == Integrator::Hermite) {
    if (o.algorithm != Algorithm::AllPairs) {
      std::cerr << "--integrator hermite is supported by --algorithm all-pairs only." << std::endl;
      std::exit(EXIT_FAILURE);
    }
    if (!(o.softening > 0.0)) {
      std::cerr << "--integrator hermite needs --softening EPS with EPS > 0." << std::endl;
      std::exit(EXIT_FAILURE);
    }
    if (o.gpus_given) {
      std::cerr << "--integrator hermite runs on one GPU: it cannot be combined with --gpus." << std::endl;
      std::exit(EXIT_FAILURE);
    }
  }
  if (o.hermite_eta > 0.0 && o.integrator != Integrator::Hermite) {
    std::cerr << "--hermite-eta needs --integrator hermite." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.hermite_levels_given && !(o.hermite_eta > 0.0)) {
    std::cerr << "--hermite-levels needs --hermite-eta ETA." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.hermite_order_given && o.integrator != Integrator::Hermite) {
    std::cerr << "--hermite-order needs --integrator hermite." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.hermite_order == 6 && o.hermite_eta > 0.0) {
    std::cerr << "--hermite-order 6 takes a fixed step: it cannot be combined with --hermite-eta." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.softening > 0.0 && (o.algorithm == Algorithm::Bvh || o.algorithm == Algorithm::AllPairsCollapsed)) {
    std::cerr << "--softening is supported by --algorithm all-pairs and octree only, not by "
              << (o.algorithm == Algorithm::Bvh ? "bvh" : "all-pairs-collapsed") << "." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.quadrupole && o.algorithm != Algorithm::Octree) {
    std::cerr << "--quadrupole is supported by --algorithm octree only." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.quadrupole && o.softening > 0.0) {
    std::cerr << "--quadrupole and --softening cannot be combined." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.tree_energy && o.algorithm != Algorithm::Octree) {
    std::cerr << "--tree-energy is supported by --algorithm octree only." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  if (o.tree_energy && !o.save_energy) {
    std::cerr << "--tree-energy changes what --save energy|all records: it needs one of them." << std::endl;
    std::exit(EXIT_FAILURE);
  }
  return o;
}

}  // namespace nb
