// Step drivers: the L3 layer of the reference (run_all_pairs src/all_pairs.h:52-106, run_bvh
// src/bvh.h:327-418, run_simulation src/main.cpp:19-40) re-stated over the HIP backend.  They keep
// the reference's observable behaviour: which steps are warm-up and which are timed, the CSV text,
// when frames are saved.  Device work is asynchronous, so every wall-clock bracket ends with a
// stream sync.
#pragma once
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "backend.hpp"
#include "options.hpp"
#include "saver.hpp"

namespace nb {

using wall_clock = std::chrono::steady_clock;
using seconds_t  = std::chrono::duration<double>;

template <typename F>
seconds_t timed(F&& f) {
  auto t0 = wall_clock::now();
  f();
  return seconds_t(wall_clock::now() - t0);
}

inline std::string fixed2(double v) {
  char b[64];
  std::snprintf(b, sizeof b, "%.2f", v);
  return b;
}

inline void csv_total_guard(Options const& o) {  // src/all_pairs.h:58-62, src/bvh.h:334-339
  if (o.csv_total && (o.print_state || o.print_info || o.save_pos || o.save_energy || o.save_neighbours || o.save_density != 0 || o.save_groups || o.save_lists)) std::abort();
}

template <typename T, int D>
void run_all_pairs(System<T, D>& sys, Device<T, D>& dev, Options o, char const* name, bool collapsed) {
  Saver<T, D> saver(o);
  saver.save_all(sys, dev);
  csv_total_guard(o);
  if (o.csv_total) std::cout << "algorithm,dim,precision,nsteps,nbodies,total [s]\n";  // detailed prints no header here

  auto force = [&] {
    if (collapsed) dev.all_pairs_collapsed_force();
    else if (o.softening > 0.0) dev.all_pairs_softened_force(o.softening);
    else dev.all_pairs_force();
  };
  seconds_t t_force(0), t_accel(0), t_total(0);
  // --integrator hermite: acceleration and jerk of the starting state once, then one predictor-corrector call per step; the step has
  // no separate accelerate phase (its time goes to the force column, accel stays 0.00)
  bool const hermite = o.integrator == Integrator::Hermite && !collapsed;
  // --hermite-eta: block time steps.  One step of the run is one advance of dt; it reads the size of every active set back, so it
  // is not recorded: warm-up and timed steps are plain calls (eta_start = ETA / 2 for the first levels, which have no a2, a3 yet)
  bool const block = hermite && o.hermite_eta > 0.0;
  // --hermite-order 6: the sixth-order scheme (force + jerk + snap), driven like the fixed-step fourth-order run
  bool const sixth = hermite && o.hermite_order == 6;
  if (block) {
    dev.hermite_block_start(o.softening, 0.5 * o.hermite_eta, o.hermite_levels);
    dev.sync();
  } else if (hermite) {
    if (sixth) dev.hermite6_start(o.softening);
    else dev.hermite_start(o.softening);
    dev.sync();
  }
  auto hermite_one = [&] {
    if (block) dev.hermite_block_advance(o.softening, o.hermite_eta);
    else if (sixth) dev.hermite6_step(o.softening);
    else dev.hermite_step(o.softening);
  };
  if (block && !o.csv_detailed) {
    for (std::size_t step = 0; step < o.warmup_steps; ++step) hermite_one();
    dev.sync();
    t_total = timed([&] {
      for (std::size_t step = o.warmup_steps; step < o.steps; ++step) hermite_one();
      dev.sync();
    });
    o.steps -= o.warmup_steps;
  } else if (hermite && o.csv_detailed) {
    t_total = timed([&] {
      for (std::size_t step = 0; step < o.steps; ++step) {
        t_force += timed([&] { hermite_one(); dev.sync(); });
        saver.save_all(sys, dev);
      }
    });
  } else if (hermite) {
    nbody_graph* g = dev.record(hermite_one);
    for (std::size_t step = 0; step < o.warmup_steps; ++step) dev.replay(g);
    dev.sync();
    t_total = timed([&] {
      for (std::size_t step = o.warmup_steps; step < o.steps; ++step) dev.replay(g);
      dev.sync();
    });
    nbody_graph_destroy(g);
    o.steps -= o.warmup_steps;
  } else if (o.csv_detailed) {
    t_total = timed([&] {
      for (std::size_t step = 0; step < o.steps; ++step) {
        t_force += timed([&] { force(); dev.sync(); });
        t_accel += timed([&] { dev.accelerate_step(); dev.sync(); });
        saver.save_all(sys, dev);
      }
    });
  } else if (dev.sharded()) {
    // several devices driven by this one thread: plain asynchronous launches (5 per device and step against >= 80 ms of force)
    auto one_step = [&] { force(); dev.accelerate_step(); };
    for (std::size_t step = 0; step < o.warmup_steps; ++step) one_step();
    dev.sync();
    t_total = timed([&] {
      for (std::size_t step = o.warmup_steps; step < o.steps; ++step) one_step();
      dev.sync();
    });
    o.steps -= o.warmup_steps;
  } else {
    // the step is a fixed launch sequence: record it once, replay it (hipGraph)
    nbody_graph* g = dev.record([&] { force(); dev.accelerate_step(); });
    for (std::size_t step = 0; step < o.warmup_steps; ++step) dev.replay(g);
    dev.sync();
    t_total = timed([&] {
      for (std::size_t step = o.warmup_steps; step < o.steps; ++step) dev.replay(g);
      dev.sync();
    });
    nbody_graph_destroy(g);
    o.steps -= o.warmup_steps;  // wraps for steps < 10, as printed by the reference
  }
  if (o.csv_detailed || o.csv_total) {
    std::cout << name << ',' << D << ',' << sizeof(T) * 8 << ',' << o.steps << ',' << sys.n << ',' << fixed2(t_total.count());
    if (o.csv_detailed) std::cout << ',' << fixed2(t_force.count()) << ',' << fixed2(t_accel.count());
    std::cout << "\n";
  }
}

template <typename T, int D>
void run_bvh(System<T, D>& sys, Device<T, D>& dev, Options o) {
  Saver<T, D> saver(o);
  saver.save_all(sys, dev);
  csv_total_guard(o);
  if (o.csv_total || o.csv_detailed) {
    std::cout << "algorithm,dim,precision,nsteps,nbodies,total [s]";
    if (o.csv_detailed) std::cout << ",force [s],accel [s],bbox [s],sort [s],multipoles [s],force approx [s]";
    std::cout << "\n";
  }
  dev.bvh_alloc();
  T const theta = T(o.theta);
  seconds_t t_force(0), t_accel(0), t_bbox(0), t_sort(0), t_tree(0), t_walk(0), t_total(0);
  if (o.csv_detailed) {
    t_total = timed([&] {
      for (std::size_t step = 0; step < o.steps; ++step) {
        t_force += timed([&] {
          t_bbox += timed([&] { dev.bvh_bounding_box(); dev.sync(); });
          t_sort += timed([&] { dev.bvh_hilbert_sort(); dev.sync(); });
          t_tree += timed([&] { dev.bvh_build_tree(); dev.sync(); });
          t_walk += timed([&] { dev.bvh_compute_force(theta); dev.sync(); });
        });
        t_accel += timed([&] { dev.accelerate_step(); dev.sync(); });
        if (o.print_info) {
          char b[64];
          std::snprintf(b, sizeof b, "Total mass: % .5f\n", double(dev.bvh_total_mass()));
          std::cout << b;
        }
        saver.save_all(sys, dev);
      }
    });
  } else {
    auto one_step = [&] {
      dev.bvh_bounding_box();
      dev.bvh_hilbert_sort();
      dev.bvh_build_tree();
      dev.bvh_compute_force(theta);
      dev.accelerate_step();
    };
    nbody_graph* g = dev.record(one_step);  // ~40 launches per step -> one graph submission
    for (std::size_t step = 0; step < o.warmup_steps; ++step) dev.replay(g);
    dev.sync();
    t_total = timed([&] {
      for (std::size_t step = o.warmup_steps; step < o.steps; ++step) dev.replay(g);
      dev.sync();
    });
    nbody_graph_destroy(g);
    o.steps -= o.warmup_steps;
  }
  if (o.csv_detailed || o.csv_total) {
    std::cout << "bvh," << D << ',' << sizeof(T) * 8 << ',' << o.steps << ',' << sys.n << ',' << fixed2(t_total.count());
    if (o.csv_detailed)
      std::cout << ',' << fixed2(t_force.count()) << ',' << fixed2(t_accel.count()) << ',' << fixed2(t_bbox.count()) << ','
                << fixed2(t_sort.count()) << ',' << fixed2(t_tree.count()) << ',' << fixed2(t_walk.count());
    std::cout << "\n";
  }
}

// src/octree.h:266-347
template <typename T, int D>
void run_octree(System<T, D>& sys, Device<T, D>& dev, Options o) {
  Saver<T, D> saver(o);
  saver.save_all(sys, dev);
  csv_total_guard(o);
  if (o.csv_total || o.csv_detailed) {
    std::cout << "algorithm,dim,precision,nsteps,nbodies,total [s]";
    if (o.csv_detailed) std::cout << ",force [s],accel [s],clear [s],bbox [s],insert [s],multipoles [s],force approx [s]";
    std::cout << "\n";
  }
  dev.octree_alloc();  // (with --tree-energy the first save_all has already made the tree: this is then a no-op)
  if (o.print_info) std::cout << "Tree init complete\n";
  T const theta = T(o.theta);
  seconds_t t_force(0), t_accel(0), t_clear(0), t_bbox(0), t_insert(0), t_tree(0), t_walk(0), t_total(0);
  // --block-eta: block time steps.  One step of the run is one advance of dt; it reads the size of every active set back, so it is
  // not recorded: warm-up and timed steps are plain calls.  The advance has no phases of its own to time: with --csv-detailed its
  // time goes to the force column, the others stay 0.00
  bool const block = o.block_eta > 0.0;
  auto block_one   = [&] { dev.octree_block_advance(theta, o.softening, o.block_eta); };
  if (block) {
    dev.octree_block_start(theta, o.softening, o.block_eta, o.block_levels);
    dev.sync();
  }
  if (block && o.csv_detailed) {
    t_total = timed([&] {
      for (std::size_t step = 0; step < o.steps; ++step) {
        t_force += timed([&] { block_one(); dev.sync(); });
        auto [size, mass] = dev.octree_info();  // reports a build of ANY block step that hit the depth limit / node pool
        if (o.print_info) {
          char b[96];
          std::snprintf(b, sizeof b, "Tree size: %u\nTotal mass: % .5f\n", size, double(mass));
          std::cout << b;
        }
        saver.save_all(sys, dev);
      }
    });
  } else if (block) {
    for (std::size_t step = 0; step < o.warmup_steps; ++step) block_one();
    dev.sync();
    (void)dev.octree_info();  // a build flagged on the device stops the run here
    t_total = timed([&] {
      for (std::size_t step = o.warmup_steps; step < o.steps; ++step) block_one();
      dev.sync();
    });
    (void)dev.octree_info();
    o.steps -= o.warmup_steps;
  } else if (o.csv_detailed) {
    t_total = timed([&] {
      for (std::size_t step = 0; step < o.steps; ++step) {
        t_force += timed([&] {
          t_clear += timed([&] { dev.octree_clear(); dev.sync(); });
          t_bbox += timed([&] { dev.octree_compute_bounds(); dev.sync(); });
          t_insert += timed([&] { dev.octree_insert(); dev.sync(); });
          t_tree += timed([&] { dev.octree_compute_tree(); dev.sync(); });
          if (o.quadrupole) t_tree += timed([&] { dev.octree_compute_quadrupoles(); dev.sync(); });  // the multipoles column
          t_walk += timed([&] {
            if (o.quadrupole) dev.octree_compute_quadrupole_force(theta);
            else dev.octree_compute_force(theta, o.softening);
            dev.sync();
          });
        });
        t_accel += timed([&] { dev.accelerate_step(); dev.sync(); });
        auto [size, mass] = dev.octree_info();  // also reports a build that hit the depth limit / node pool
        if (o.print_info) {
          char b[96];
          std::snprintf(b, sizeof b, "Tree size: %u\nTotal mass: % .5f\n", size, double(mass));
          std::cout << b;
        }
        saver.save_all(sys, dev);
      }
    });
  } else {
    auto one_step = [&] {
      dev.octree_clear();
      dev.octree_compute_bounds();
      dev.octree_insert();
      dev.octree_compute_tree();
      if (o.quadrupole) {
        dev.octree_compute_quadrupoles();
        dev.octree_compute_quadrupole_force(theta);
      } else {
        dev.octree_compute_force(theta, o.softening);
      }
      dev.accelerate_step();
    };
    one_step();  // the phase-order checks of the ABI need one direct pass before the sequence is recorded
    (void)dev.octree_info();  // ... and tells the library how deep this system's tree is: the recorded step launches that many levels
    nbody_graph* g = dev.record(one_step);
    for (std::size_t step = 1; step < o.warmup_steps; ++step) dev.replay(g);
    dev.sync();
    (void)dev.octree_info();  // a build flagged on the device (bodies that never separate, node pool) stops the run here
    t_total = timed([&] {
      for (std::size_t step = o.warmup_steps; step < o.steps; ++step) dev.replay(g);
      dev.sync();
    });
    nbody_graph_destroy(g);
    (void)dev.octree_info();
    o.steps -= o.warmup_steps;
  }
  if (o.csv_detailed || o.csv_total) {
    std::cout << "octree," << D << ',' << sizeof(T) * 8 << ',' << o.steps << ',' << sys.n << ',' << fixed2(t_total.count());
    if (o.csv_detailed)
      std::cout << ',' << fixed2(t_force.count()) << ',' << fixed2(t_accel.count()) << ',' << fixed2(t_clear.count()) << ','
                << fixed2(t_bbox.count()) << ',' << fixed2(t_insert.count()) << ',' << fixed2(t_tree.count()) << ','
                << fixed2(t_walk.count());
    std::cout << "\n";
  }
}

// src/main.cpp:19-40
template <typename T, int D>
void run_simulation(Options const& o, System<T, D>& sys) {
  bool const quiet = o.csv_total || o.csv_detailed;
  if (o.print_state) {
    std::cout << "Starting state:" << std::endl;
    sys.print();
  }
  if (!quiet) std::cout << "Starting simulation" << std::endl;
  auto t0 = wall_clock::now();
  {
    if (o.gpus > 1 && o.algorithm != Algorithm::AllPairs) {
      std::cerr << "--gpus " << o.gpus << ": bodies shard over GPUs for --algorithm all-pairs only." << std::endl;
      std::exit(EXIT_FAILURE);
    }
    // an explicit --gpus N with all-pairs goes through the communicator, the shard windows and the exchange for ANY N (N = 1
    // is how a one-GPU box exercises that path); without the flag: the reference's single device, no communicator
    bool const exchange = o.algorithm == Algorithm::AllPairs && o.gpus_given;
    Device<T, D> dev(sys, o.gpus, exchange);
    switch (o.algorithm) {
      case Algorithm::AllPairs: run_all_pairs(sys, dev, o, "all-pairs", false); break;
      case Algorithm::AllPairsCollapsed: run_all_pairs(sys, dev, o, "all-pairs-collapsed", true); break;
      case Algorithm::Bvh: run_bvh(sys, dev, o); break;
      case Algorithm::Octree: run_octree(sys, dev, o); break;
    }
    dev.pull();
  }
  auto t1 = wall_clock::now();
  if (o.print_state) {
    std::cout << "Final state:" << std::endl;
    sys.print();
  }
  if (!quiet) {
    char b[96];
    std::snprintf(b, sizeof b, "Done simulation\nTotal time: %.2f ms\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
    std::cout << b;
  }
}

}  // namespace nb
