/*
 * nbody_hip.h — C ABI of the MI355X (gfx950) N-body force/integration backend.
 *
 * Drop-in boundary for the hot path of UoB-HPC/stdpar-nbody: the reference has no FFI; its seam is
 * the L3 -> L2 edge where a step driver (run_all_pairs, src/all_pairs.h:52; run_bvh, src/bvh.h:327)
 * issues one blocking stdpar algorithm per phase over the raw-pointer view System::state_t
 * (src/system.h:41-50).  Each entry point below replaces exactly one of those stdpar call sites and
 * takes the same view (`nbody_state`, pointers now in device memory), so a reference maintainer
 * swaps `std::for_each(par_unseq, ...)` for one call (see INTEGRATION.md for the stub).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++/torch types.  Every function returns 0 on success
 *    and a non-zero code on failure; nbody_last_error() returns the message (thread-local).
 *    No exception crosses the boundary.
 *  - All phase calls are asynchronous on `stream` (a hipStream_t passed as void*, NULL = default
 *    stream).  Ordering between phases is stream order.  nbody_stream_sync() / nbody_download()
 *    are the blocking points.
 *  - dtype: NBODY_F32 | NBODY_F64.  dim: 2 | 3.  Arrays use the reference layout: m is T[sz];
 *    x, v, a, ao are vec<T,D>[...] = D contiguous T per body (src/vec.h:17-19), no padding.
 *  - Sharding (multi-GPU all-pairs): a state owns target bodies [first, first+count).  m and x
 *    always hold ALL sz bodies (sources); v, a, ao hold `count` records, record k = body first+k.
 *    Single GPU: first = 0, count = sz.
 *  - The library never falls back to a CPU path: without a usable HIP device every call fails.
 *  - Devices: a context, a tree and a communicator remember the device they were created on; a phase call runs on
 *    the device of its `stream` (NULL stream: the calling thread's current device); a tree must be used with a stream
 *    of its own device (NBODY_ERR_ARG otherwise).  Every entry point switches to
 *    that device for the duration of the call and restores the caller's, so one host thread can drive several GPUs.
 */
#ifndef NBODY_HIP_H
#define NBODY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBODY_F32 0
#define NBODY_F64 1

#define NBODY_OK 0
#define NBODY_ERR_ARG 1     /* bad argument (dtype/dim/null pointer/size) */
#define NBODY_ERR_HIP 2     /* HIP runtime error, message has hipGetErrorString */
#define NBODY_ERR_STATE 3   /* call sequence error (e.g. build_tree before hilbert_sort) */

/* Device-pointer mirror of System<T,N>::state_t (src/system.h:41-50) plus the shard window. */
typedef struct nbody_state {
  void* m;         /* T[sz]            masses of all bodies                         */
  void* x;         /* vec<T,D>[sz]     positions of all bodies                      */
  void* v;         /* vec<T,D>[count]  velocities of owned bodies                   */
  void* a;         /* vec<T,D>[count]  accelerations of owned bodies                */
  void* ao;        /* vec<T,D>[count]  previous-step accelerations of owned bodies  */
  double dt;       /* time step   (converted to T inside, as System::dt is T)       */
  double c;        /* constant G  (System::constant)                                */
  uint32_t sz;     /* total number of bodies (System::size, index_t = uint32_t)     */
  uint32_t first;  /* first owned body                                              */
  uint32_t count;  /* number of owned bodies                                        */
  int32_t dtype;   /* NBODY_F32 | NBODY_F64                                         */
  int32_t dim;     /* 2 | 3                                                         */
  uint32_t tuning; /* K1 launch shape for calls with this view: 0 = the library default, else
                      NBODY_TUNING(split, targets_per_thread, source_path); never changes which
                      pairs are summed (see nbody_all_pairs_configure).  A state filled by hand
                      must zero this field: any other value is refused (NBODY_ERR_ARG)       */
} nbody_state;

/* split in bits 0-3, targets per lane in bits 4-5, source path in bits 6-7; each 0 = auto */
#define NBODY_TUNING(split, targets_per_thread, source_path) \
  ((uint32_t)(((split) & 15) | (((targets_per_thread) & 3) << 4) | (((source_path) & 3) << 6) | 0x100u))

/* ABI version of this header/library pair: major * 1000 + minor.  Bindings should refuse a different major.
 * 2.0: nbody_state.tuning; the collective (nbody_comm_*), shard windows on contexts, per-device guards.
 * 2.1: nbody_bvh_create_on / nbody_octree_create_on (explicit device), nbody_octree_set_walk, nbody_octree_set_build, nbody_octree_set_step_budget,
 *      nbody_bvh_set_launch_order;
 *      a tree used with a stream of another device is refused; nbody_state.tuning is validated (0 or NBODY_TUNING(...)).
 * 2.2: nbody_bvh_read what = 6 and nbody_bvh_opening_thresholds (the opening test as one compare), nbody_all_pairs_pair_rule;
 *      the measured forms that are not shipped (traversal 3 / 4 / 6, octree build 2 / 4) are refused by this library.
 * 2.3: nbody_all_pairs_status; nbody_stream_sync / nbody_download return NBODY_ERR_STATE after a failed K1 chunk hand-off;
 *      nbody_all_pairs_pair_rule decides from the positions' variances, not from their bounding box.
 * 2.4: Plummer softening: nbody_all_pairs_softened_force, nbody_calc_energies_softened, nbody_octree_compute_softened_force.
 *      Additive, same version: octree quadrupole moments, nbody_octree_compute_quadrupoles, nbody_octree_compute_quadrupole_force,
 *      nbody_octree_read_root_quadrupole.  Additive, same version: octree potentials and energies, nbody_octree_compute_potential,
 *      nbody_octree_compute_softened_potential, nbody_octree_compute_quadrupole_potential, nbody_octree_calc_energies.
 *      Additive, same version: the fourth-order Hermite integrator for all-pairs, nbody_hermite_create, nbody_hermite_create_on,
 *      nbody_hermite_destroy, nbody_hermite_force_jerk, nbody_hermite_step, nbody_hermite_read.  Additive, same version: block
 *      (individual) time steps for it, nbody_hermite_block_start, nbody_hermite_block_step, nbody_hermite_block_advance,
 *      nbody_hermite_block_read.  Additive, same version: block (individual) time steps for the octree leapfrog,
 *      nbody_octree_block_create, nbody_octree_block_create_on, nbody_octree_block_destroy, nbody_octree_block_start,
 *      nbody_octree_block_step, nbody_octree_block_advance, nbody_octree_block_read.  Additive, same version: the sixth-order
 *      Hermite integrator for all-pairs, nbody_hermite6_create, nbody_hermite6_create_on, nbody_hermite6_destroy,
 *      nbody_hermite6_start, nbody_hermite6_step, nbody_hermite6_read.  Additive, same version: block (individual) time steps
 *      for it, nbody_hermite6_block_start, nbody_hermite6_block_step, nbody_hermite6_block_advance, nbody_hermite6_block_read.
 *      Additive, same version: all-pairs per-body potentials, nearest neighbours and the closest pair, nbody_neighbours_create,
 *      nbody_neighbours_create_on, nbody_neighbours_destroy, nbody_neighbours_compute, nbody_neighbours_read,
 *      nbody_neighbours_closest_pair.  Additive, same version: all-pairs k nearest neighbours, local densities and the density
 *      centre, nbody_knn_create, nbody_knn_create_on, nbody_knn_destroy, nbody_knn_compute, nbody_knn_read,
 *      nbody_knn_density_centre; nbody_knn_create_method and nbody_knn_method (the tree-pruned method of the same handle).
 *      Additive, same version: friends-of-friends groups on the same tree, nbody_fof_create, nbody_fof_create_on,
 *      nbody_fof_destroy, nbody_fof_compute, nbody_fof_read, nbody_fof_summary.  Additive, same version: exact fixed-radius
 *      neighbour lists on the same tree, nbody_nlist_create, nbody_nlist_create_on, nbody_nlist_destroy, nbody_nlist_set_radii,
 *      nbody_nlist_compute, nbody_nlist_read, nbody_nlist_summary. */
#define NBODY_HIP_ABI_VERSION 2004
int nbody_abi_version(void);

/* Last error message of the calling thread ("" if none). */
const char* nbody_last_error(void);

/* Library / device identification: writes e.g. "gfx950:sramecc+:xnack-" and the CU count. */
int nbody_device_info(int device, char* arch_out, size_t arch_len, int* cu_count);

/* ---- all-pairs ---------------------------------------------------------------------------------- */

/* K1. Replaces all_pairs_force (src/all_pairs.h:14-27):
 *   a[i] = c * sum_{j != i} m[j] * (x[j] - x[i]) / (pow(|x[j]-x[i]|^2, 3/2) + eps(T))
 * for owned bodies i; sources j = 0..sz-1 staged through LDS tiles.
 * In double, from 262 144 bodies on, the automatic launch is ORDERED: sources and the window's targets are sorted by a space key
 * (the Morton code of the body's cell of side 1) before the kernel runs and `a` is scattered back afterwards — 11 launches per call
 * (18 for a shard window) and about 48 + 24 + 16 dim bytes of stream scratch per body, reserved with the packed records (so a
 * context's recorded step never allocates).  The sum of a target then runs in key order: a function of all sz positions, so the
 * rows of any shard window equal the whole launch's bit for bit; systems on the dense pair rule keep the index order. */
int nbody_all_pairs_force(const nbody_state* s, void* stream);

/* K1's in-kernel chunk hand-off, and how it fails.  From 2048 bodies on, the source range is cut into >= 16 chunks over grid.y;
 * the block of chunk y adds its sum into `a` after the block of chunk y - 1 has (a turn word per group of targets), which fixes
 * the rounding order without a scratch array or a second launch.  (Launches whose whole grid is resident at once — up to 2048
 * blocks, i.e. up to 8192 targets — collect the chunks' sums instead: whichever chunk arrives last adds them in chunk order; the same
 * bits, no waiting, nothing that can fail.)  A block waits only for blocks of smaller linear index.  That
 * this terminates rests on an ASSUMPTION about the dispatcher (true of every GPU this library targets, stated nowhere in the
 * ISA): the workgroups of a grid are started in linear index order, so the oldest unfinished block never waits.  The reference's
 * loop (src/all_pairs.h:14-27) cannot return garbage silently, and neither does this: a wave that has waited for its turn past
 * the poll budget (minutes) gives up, the group's rows of `a` end as NaN — never as a finite partial sum — and a sticky
 * per-stream status word is set on the device.  nbody_stream_sync, nbody_download and nbody_all_pairs_status on that stream then
 * return NBODY_ERR_STATE with a message naming the target block, the group and the chunk, until the status is cleared.
 *
 * nbody_all_pairs_status waits for `stream` and writes (out may be NULL)
 *   out[0] = 1 if a hand-off has failed, out[1..3] = target block, target group, chunk of the first failure,
 *   out[4] = polls made by waves that had to wait for their turn, out[5] = number of waves that had to wait
 * accumulated over every K1 launch of this stream since the last clear; clear != 0 zeroes them after the read.  A stream that
 * has never run the chunked K1 reports zeros.  In normal operation nobody waits: out[4] = out[5] = 0. */
int nbody_all_pairs_status(void* stream, uint64_t out[6], int clear);

/* K2. Replaces all_pairs_collapsed_force (src/all_pairs.h:29-50) with its INTENDED semantics
 * (64-bit pair space, all D components; the reference wraps the pair count at 2^32 and drops
 * component 2 — SURVEY §0.5):  a[i] <- (a[i] - ao[i]) + sum_{j != i} (c*m[j]) * (x[j]-x[i]) / dist3.
 * Lanes run along the SOURCE axis (one ordered pair per lane and step), the partial sums of 16 (double: 8) targets are
 * reduced across the wavefront together, one atomic add per target, component and wave (tolerance parity).  Float: a wave
 * owns its 16 targets for a whole chunk of the packed source records (streamed from L2, no LDS); double: (target group x
 * LDS source tile) blocks.  Uses the stream's K1 scratch (packed records) like nbody_all_pairs_force.  Single-GPU only
 * (first = 0, count = sz). */
int nbody_all_pairs_collapsed_force(const nbody_state* s, void* stream);

/* K3. Replaces System::accelerate_step (src/system.h:52-60) for owned bodies:
 *   x += dt*v + ((0.5*dt)*dt)*ao;  v += (0.5*dt)*(a + ao);  ao = a          (bit-exact, no FMA) */
int nbody_accelerate_step(const nbody_state* s, void* stream);

/* K10+K11. Replaces System::calc_energies (src/system.h:62-79): kinetic = 0.5*sum m|v|^2 and potential =
 * -0.5*c*sum_i sum_{j!=i} m_i m_j/(|x_i-x_j| + eps).  Writes one T each to the HOST pointers; blocking.
 * Needs the whole system (first = 0, count = sz). */
int nbody_calc_energies(const nbody_state* s, void* kinetic_out, void* potential_out, void* stream);

/* Tuning knob for K1 (does not change which pairs are summed, only the split of the source range
 * over the waves of a block and hence the rounding order).  split in {0 (auto from sz: 8 for sz >= 65536, else 4), 1, 2,
 * 4, 8 (8: scalar-stream form only)}; targets_per_thread in {0 (auto), 1, 2} (no effect on the result).  The auto split
 * depends on sz only — never on first/count — so results are bitwise independent of how bodies are sharded over GPUs. */
int nbody_all_pairs_configure(int split, int targets_per_thread);
/* The two calls here set the PROCESS-WIDE default (atomic; used by every view whose `tuning` is 0).  A context carries its
 * own choice: nbody_ctx_configure_all_pairs stores it and nbody_ctx_state hands it out in nbody_state.tuning. */
/* How K1 brings a source record to the 64 lanes of a wave (same arithmetic, same order, bitwise the same result):
 * 1 = tiles staged in LDS, read as LDS broadcasts; 2 = records packed once per call and streamed through the scalar
 * unit into SGPRs; 0 = auto (2 once the call has several waves per SIMD, about 65 536 targets; 1 below).  Form 2 keeps a packed-source buffer per calling stream (32 B per body, grow-only):
 * contexts from nbody_create reserve theirs, any other stream gets it on its first call, which must not be recorded. */
int nbody_all_pairs_source_path(int mode);

/* ---- Hilbert BVH (src/bvh.h) ---------------------------------------------------------------------- */

/* Tree + scratch storage; replaces bvh<T,N>::alloc / dealloc (src/bvh.h:147-172).
 * nleafs = bit_ceil(n), nlevels = log2(nleafs), nnodes = 2^nlevels - 1.  n >= 2. */
typedef struct nbody_bvh nbody_bvh;
int  nbody_bvh_create(nbody_bvh** out, int dtype, int dim, uint32_t n);               /* on the current device */
int  nbody_bvh_create_on(nbody_bvh** out, int dtype, int dim, uint32_t n, int device); /* device < 0: the current one */
void nbody_bvh_destroy(nbody_bvh* t);

/* K4. Replaces bounding_box (src/bvh.h:17-22): AABB of all x padded by +-10 eps, always containing
 * the origin.  Result stays on the device for K5; nbody_bvh_get_bounding_box copies it out
 * (blocking): xmin_out/xmax_out are T[dim] on the host. */
int nbody_bvh_bounding_box(nbody_bvh* t, const nbody_state* s, void* stream);
int nbody_bvh_get_bounding_box(nbody_bvh* t, void* xmin_out, void* xmax_out, void* stream);

/* K5+K6. Replaces hilbert_sort (src/bvh.h:25-96): 64-bit Hilbert key per body from the K4 box,
 * stable LSD radix sort of (key, index), then one gather that permutes m, x, v, a, ao IN PLACE
 * (caller-visible, exactly like the reference). Requires first = 0, count = sz. */
int nbody_bvh_hilbert_sort(nbody_bvh* t, const nbody_state* s, void* stream);

/* K7+K8. Replaces bvh::build_tree (src/bvh.h:175-244): leaf-parent level from body pairs, then one
 * launch per level upward (monopoles, AABBs, widths; dead nodes have mass 0 and width 0). */
int nbody_bvh_build_tree(nbody_bvh* t, const nbody_state* s, void* stream);

/* K9. Replaces bvh::compute_force (src/bvh.h:246-324): stackless traversal per owned body with the
 * opening test bw^2 < theta^2 * dist2 evaluated exactly as the reference does (no FMA). */
int nbody_bvh_compute_force(nbody_bvh* t, const nbody_state* s, double theta, void* stream);

/* Test/diagnostic read-back of BVH internals (blocking device->host copies).
 * what: 0 keys u64[n] (pre-sort order) | 1 perm u32[n] (new -> old) | 2 node monopoles T[nnodes][D+1]
 * (x..., mass) | 3 node widths T[nnodes] | 4 node boxes T[nnodes][2D] | 5 traversal counters
 * u32[n][4] {node tests, leaf visits, monopole terms, body terms} (filled by
 * nbody_bvh_compute_force only after nbody_bvh_enable_counters(t, 1)) | 6 opening thresholds T[nnodes]: the largest v
 * with width^2 >= fl(theta^2 * d2) for every d2 <= v, i.e. the reference's test width^2 < theta^2 * d2
 * (src/bvh.h:246-248) is v < d2 bit for bit; written by the build for the angle of the last nbody_bvh_compute_force
 * (0.5, the reference's default, before the first) and rewritten by a traversal that asks for another one. */
int nbody_bvh_read(nbody_bvh* t, int what, void* host_out, size_t bytes, void* stream);
/* The thresholds of what = 6 for given width^2 values, computed on the HOST by the same function the build kernels run (no
 * device needed): out[i] = the largest v such that width2[i] < fl(theta^2 * d2) fails for every d2 <= v; -1 for a negative
 * input (body entries), +inf when no distance accepts.  For the tests that hold this form against src/bvh.h:246-248. */
int nbody_bvh_opening_thresholds(int dtype, const void* width2, double theta, size_t n, void* out);
int nbody_bvh_enable_counters(nbody_bvh* t, int on);
/* K9 scheduling form: 0 = auto (by size), 1 = one independent stackless walk per lane — the reference's loop as is, with its
 * product form of the opening test —, 2 (= 5) = wave-cooperative sweep of the union of the wave's walks in DFS key order, the step
 * program written as ISA, the opening test as one compare against the record's threshold (nbody_bvh_read what = 6).  Both make
 * every body perform the same tests in the same order: results and counters are bitwise identical (the tests hold them equal).
 * Forms that were measured and lost (3 / 4 / 6) exist in the -DNBODY_EXPERIMENTS build only; this library refuses them. */
int nbody_bvh_set_traversal(nbody_bvh* t, int mode);
/* Launch order of the sweep: 0 = work items (groups that straddle a jump of the key order are cut in two and start first),
 * 1 = one block per group in index order.  Bitwise identical results; tests and tuning runs compare the two. */
int nbody_bvh_set_launch_order(nbody_bvh* t, int mode);
uint32_t nbody_bvh_nnodes(const nbody_bvh* t);

/* ---- octree Barnes-Hut (src/octree.h, the reference's default --algorithm) ---------------------------------
 * The reference inserts bodies concurrently under per-node spin locks; only node NUMBERS depend on that order.
 * Here the same spatial tree is built without locks (path keys -> radix sort -> breadth-first split), so results,
 * tree size and visit counts equal the reference's.  Whole system only for the build phases; compute_force
 * honours the shard window.  Errors found on the device (coincident bodies / node pool exhausted) surface in nbody_octree_info. */
typedef struct nbody_octree nbody_octree;
/* octree<T,N>::alloc / dealloc (src/octree.h:42-60); capacity = max(2^dim * n, 1000) nodes (src/system.h:30). */
int  nbody_octree_create(nbody_octree** out, int dtype, int dim, uint32_t n);               /* on the current device */
int  nbody_octree_create_on(nbody_octree** out, int dtype, int dim, uint32_t n, int device); /* device < 0: the current one */
void nbody_octree_destroy(nbody_octree* t);
/* Scheduling form of the walk: 0 = auto, 1 = the compiler-scheduled kernel, 2 = the visit round written as ISA (fails where that
 * form does not exist).  Same tests, same arithmetic, same order: bitwise identical accelerations and counters. */
int  nbody_octree_set_walk(nbody_octree* t, int mode);
/* How the tree is built from the sorted path keys and how the multipole pass is launched:
 *   0 = auto (3);
 *   3 = one pass: every cell follows from the common key prefixes of neighbouring bodies, so all cells are numbered by one prefix
 *       sum and built at once (4 launches whatever the depth), and the multipoles take two or three (rank chunks, then the cells
 *       that span chunk boundaries, in two rounds above 2.6e5 bodies);
 *   1 = breadth-first, one launch per tree level for the build and one for the multipoles (21 + 21 in 3D): the cross-check.
 * 1 numbers the sibling groups breadth-first, 3 in pre-order; the cells, their monopoles, the tree size and every force and
 * counter the walk produces are the same bit for bit.  A tree inserted by one form is not the other's to finish: changing the
 * form clears the insert / tree state.  (The grid-barrier forms 2 and 4 — measured slower on MI355X — exist in the
 * -DNBODY_EXPERIMENTS build only.) */
int  nbody_octree_set_build(nbody_octree* t, int mode);
/* Visit rounds one body's walk may make before it is abandoned and nbody_octree_info reports it (never spin on a damaged
 * tree).  0 = the default: the node pool size, which no walk of a well-formed tree reaches. */
int  nbody_octree_set_step_budget(nbody_octree* t, uint32_t steps);
/* octree::clear (src/octree.h:85-89): readies the tree for the next step. */
int nbody_octree_clear(nbody_octree* t, void* stream);
/* octree::compute_bounds (src/octree.h:93-112): root cube from the scalar min/max over all coordinates, +-1. */
int nbody_octree_compute_bounds(nbody_octree* t, const nbody_state* s, void* stream);
/* octree::insert (src/octree.h:114-181). */
int nbody_octree_insert(nbody_octree* t, const nbody_state* s, void* stream);
/* octree::compute_tree (src/octree.h:183-224): masses and centres of mass, children summed in child order. */
int nbody_octree_compute_tree(nbody_octree* t, void* stream);
/* octree::compute_force (src/octree.h:226-263): a[i] = c * sum over the walk with side/dx < theta.  Every body performs
 * the reference's opening tests and accumulates the reference's terms (the per-body counters are identical); the terms
 * are added per child slot and the 2^dim partial sums combined, so sums differ from the reference's at rounding level. */
int nbody_octree_compute_force(nbody_octree* t, const nbody_state* s, double theta, void* stream);
/* Blocking.  tree_size = next_free_child_group (printed by --print-info, src/octree.h:314), root_mass = m[0].mass()
 * as one T; either may be NULL.  Fails if ANY build since the previous call hit the depth limit or exhausted the node
 * pool (the device-side flag is sticky; this call reports and clears it) — a caller that replays recorded steps checks once
 * at the end of the run. */
int nbody_octree_info(nbody_octree* t, uint32_t* tree_size, void* root_mass, void* stream);
/* Test/diagnostic: per-body {nodes examined, terms accumulated} u32[n][2] of the last compute_force. */
int nbody_octree_enable_counters(nbody_octree* t, int on);
int nbody_octree_read_counters(nbody_octree* t, uint32_t* host_out, size_t bytes, void* stream);
/* Quadrupole moments (no reference counterpart): the next term of the expansion of an accepted cell.  For a cell with centre of mass
 * p, Q = sum over its children c (child order, empty ones skipped) of Q_c + m_c (3 d d^T - |d|^2 I), d = p_c - p; a body leaf has
 * Q = 0.  NQ = 6 values in 3D (xx, xy, xz, yy, yz, zz), 3 in 2D (xx, xy, yy: the 3D tensor restricted to the plane, not traceless).
 * A child's stored p is its centre of mass rounded to T, so about p it keeps a dipole P_c of rounding size (a body's is 0); the sum
 * also takes 3 (P_c d^T + d P_c^T) - 2 (P_c . d) I, which keeps Q that of the cell's bodies about p to rounding level wherever the
 * cell lies (without it the error is eps(T) |p| / |d| of Q).  Both build forms give the same Q bit for bit.
 * compute_quadrupoles: after compute_tree; children before parents, on the stream.  The first call allocates the array (NQ + dim
 *   values of T per node of the pool: 576 B per body in double 3D), so it must not be recorded: under stream capture it returns
 *   NBODY_ERR_STATE.
 * compute_quadrupole_force: compute_force whose accepted cells also add -c (Q d) y^5 + (5/2) c (d^T Q d) d y^7, d = p - x[i],
 *   y = 1/|d|.  The opening tests, their order, the monopole terms and the counters are compute_force's bit for bit; honours the
 *   shard window.  The compiler-scheduled walk (form 1) on auto; NBODY_ERR_ARG after nbody_octree_set_walk(t, 2).
 * read_root_quadrupole: blocking; NQ values of T into host_out.
 * The last two return NBODY_ERR_STATE unless compute_quadrupoles ran after the latest clear / insert / compute_tree / set_build
 * (tracked by the host in call order, which a recorded step replays). */
int nbody_octree_compute_quadrupoles(nbody_octree* t, void* stream);
int nbody_octree_compute_quadrupole_force(nbody_octree* t, const nbody_state* s, double theta, void* stream);
int nbody_octree_read_root_quadrupole(nbody_octree* t, void* host_out, void* stream);

/* ---- softening (no reference counterpart: its eps(T) is machine epsilon, a guard against 0 / 0) ------------------------
 * Plummer softening with length eps.  e2 = fl_T(T(eps) * T(eps)); eps must be finite and > 0 and e2 a normal number of T with
 * e2^(-3/2) finite: e2 >= 2^-84 in float (eps >= ~1.5e-13), 2^-680 in double (eps >= ~1.4e-103).  Anything else returns
 * NBODY_ERR_ARG before the device is touched.  "No softening" is the unsoftened entry points, unchanged.
 *   force      a[i] = c * sum_{j != i} m[j] * (x[j] - x[i]) / (|x[j] - x[i]|^2 + e2)^(3/2)
 *              The self term is 0 because its difference is 0; coincident distinct bodies add 0 too.  No branch, no pair rule:
 *              |x[j] - x[i]|^2 + e2 is the FMA chain of the unsoftened K1 seeded with e2, the weight (m y^3)(1 + e(3/2 + 15/8 e)) from
 *              v_rsq_f64 (<= 2.5 ulp) in double, m y^3 from v_rsq_f32 in float.
 *   potential  -0.5 * c * sum_i m_i sum_{j != i} m_j / sqrt(|x_i - x_j|^2 + e2): the self term (m_i / eps, not 0) is excluded by
 *              index; coincident distinct bodies contribute m_i m_j / eps.  The kinetic energy is the unsoftened call's, bit for bit.
 *   octree     opening decisions unchanged (the reference's side / (sqrt(d2) + eps(T)) < theta on the unsoftened distance); only
 *              the accepted term changes, to m_node * d / (|d|^2 + e2)^(3/2).
 * Rounding structure: the unsoftened K1's.  A target's sum follows from sz alone (slices, chunks, chunk-order hand-off or collect),
 * so any shard window sums bitwise like the whole system, and both K1 source paths give the same bits. */

/* K1 softened; honours the shard window and nbody_state.tuning like nbody_all_pairs_force, and uses the stream's packed-source
 * scratch the same way (a context's stream: it may be recorded into a step graph). */
int nbody_all_pairs_softened_force(const nbody_state* s, double eps, void* stream);
/* nbody_calc_energies with the softened potential (whole system; blocking; host outputs, one T each). */
int nbody_calc_energies_softened(const nbody_state* s, double eps, void* kinetic_out, void* potential_out, void* stream);
/* nbody_octree_compute_force with the softened accepted term: the compiler-scheduled walk (form 1) whatever the walk setting
 * says on auto; NBODY_ERR_ARG if nbody_octree_set_walk(t, 2) asked for the ISA visit round, which has no softened form.
 * Counters (nbody_octree_read_counters) are the unsoftened walk's bit for bit. */
int nbody_octree_compute_softened_force(nbody_octree* t, const nbody_state* s, double theta, double eps, void* stream);

/* ---- octree potentials and energies (no reference counterpart) --------------------------------------------------------------
 * The walk that gives the force gives the potential.  For body i, S_i = the sum over its walk of the accepted terms — the same opening
 * tests in the same order as the matching force walk, the same per-child-slot partial sums combined in the same fixed order — and
 *   phi_i = -c * S_i,   PE = -0.5 * c * sum_i m_i * S_i,
 * which is System::calc_energies (src/system.h:62-79) with the inner sum replaced by the tree's.  Accepted terms, d = p - x[i]:
 *   monopole    m / (|d| + eps(T)) (src/vec.h:243-246), evaluated as nbody_calc_energies evaluates a pair, so at theta = 0 every
 *               term is the direct path's to rounding level;
 *   softened    m / sqrt(|d|^2 + e2) (e2 as for the softened force; the same NBODY_ERR_ARG rules for eps);
 *   quadrupole  the monopole term, and for accepted CELLS (never leaves) + 0.5 * (d^T Q d) / |d|^5, Q as stored by
 *               nbody_octree_compute_quadrupoles.
 * The body's own leaf (m / eps(T) unsoftened, m / eps softened, where the force's self term is 0) is left out: in a well-formed tree it
 * is the only leaf at d == 0 in every coordinate.  The compiler-scheduled walk (form 1) on auto; NBODY_ERR_ARG after
 * nbody_octree_set_walk(t, 2).  With counters on, the walks write the matching force walk's counters bit for bit.
 * compute_*potential: phi (device pointer, T[count]): phi[k] = phi of body first + k; honours the shard window.  Phase order as for
 *   the force entries (clear, compute_bounds, insert, compute_tree on this state; NBODY_ERR_STATE otherwise); the quadrupole entry also
 *   needs compute_quadrupoles after the latest build.  They allocate nothing, so a step graph may record them.
 * calc_energies: the whole system (first = 0, count = sz), on a tree built as above; eps = 0 unsoftened, eps > 0 softened,
 *   quadrupole != 0 the quadrupole term (refused together with eps > 0).  Blocking, host outputs of one T each; the kinetic energy is
 *   nbody_calc_energies' bit for bit, the potential goes through the same reduction.  NBODY_ERR_STATE under stream capture.
 * Argument errors (NULL tree, state or output, a bad eps, quadrupole with eps, a shard window for calc_energies) return NBODY_ERR_ARG
 * before the device is touched. */
int nbody_octree_compute_potential(nbody_octree* t, const nbody_state* s, double theta, void* phi, void* stream);
int nbody_octree_compute_softened_potential(nbody_octree* t, const nbody_state* s, double theta, double eps, void* phi, void* stream);
int nbody_octree_compute_quadrupole_potential(nbody_octree* t, const nbody_state* s, double theta, void* phi, void* stream);
int nbody_octree_calc_energies(nbody_octree* t, const nbody_state* s, double theta, double eps, int quadrupole, void* kinetic_out,
                               void* potential_out, void* stream);

/* ---- fourth-order Hermite integrator for all-pairs (no reference counterpart: its only integrator is K3's leapfrog step) ------
 * The predictor-corrector of Makino & Aarseth (1992) with a fixed step dt and Plummer softening: one evaluation of the acceleration
 * AND its time derivative (the jerk) per step.  With e2 = fl_T(T(eps) * T(eps)), d = x_j - x_i, u = v_j - v_i, q = |d|^2 + e2:
 *   a_i = c * sum_j m_j d q^(-3/2),     j_i = c * sum_j m_j (u - 3 (d.u) / q * d) q^(-3/2)
 * The self pair, and coincident bodies at equal velocity, add 0 because d = 0 (and u = 0): no branch, no index test, as in the
 * softened K1.  The weight m q^(-3/2) is the softened K1's, operation for operation; 1 / q comes from the same reciprocal square
 * root (no divide, no second transcendental).  eps obeys the rules of the softening section above; eps = 0 is NOT supported
 * (NBODY_ERR_ARG): the unsoftened pair needs K1's near-pair forms, which have no jerk twin.  One step from (x, v, a0, j0):
 *   predict   xp = x + dt v + dt^2/2 a0 + dt^3/6 j0,   vp = v + dt a0 + dt^2/2 j0
 *   evaluate  (a1, j1) at (xp, vp), all bodies
 *   correct   v1 = v + dt/2 (a0 + a1) + dt^2/12 (j0 - j1),   x1 = x + dt/2 (v + v1) + dt^2/12 (a0 - a1)
 *   then      x <- x1, v <- v1, a <- a1, jerk <- j1
 * (P(EC)^1: the force at the corrected positions is not evaluated again.)  dt is converted to T once, as K3 does.
 * The handle owns the jerk, the packed predicted state and the partial sums; everything is allocated by create, so the phase calls
 * allocate nothing and may be recorded into a step graph.  A body's sums are added in an order that follows from sz alone (no
 * atomics, no waiting between blocks): two runs, an eager step and a replayed recorded one give the same bits.
 *  - Whole system only: first = 0, count = sz, else NBODY_ERR_ARG.  (Sharding would need an exchange of xp AND vp per step.)
 *  - Argument errors are found before the device is touched, in this order: s NULL; the state's dtype, dim, window, tuning; eps
 *    (the message names the softening); h NULL; h made for another dtype, dim or n (all NBODY_ERR_ARG).
 *  - nbody_hermite_step before nbody_hermite_force_jerk on that handle: NBODY_ERR_STATE.  A handle used with a stream of another
 *    device: NBODY_ERR_ARG.  Every entry switches to the handle's device and restores the caller's.
 *  - nbody_hermite_read and nbody_hermite_create(_on) between nbody_graph_begin and nbody_graph_end: NBODY_ERR_STATE. */
typedef struct nbody_hermite nbody_hermite;
int  nbody_hermite_create(nbody_hermite** out, int dtype, int dim, uint32_t n);                /* on the current device */
int  nbody_hermite_create_on(nbody_hermite** out, int dtype, int dim, uint32_t n, int device); /* device < 0: the current one */
void nbody_hermite_destroy(nbody_hermite* h);
/* a = s->a and the handle's jerk at (s->x, s->v): starts a run, or restarts it after an upload.  Asynchronous, recordable. */
int  nbody_hermite_force_jerk(nbody_hermite* h, const nbody_state* s, double eps, void* stream);
/* One step as above: reads s->x, s->v, s->a and the jerk, rewrites them.  s->ao is neither read nor written.  Asynchronous, recordable. */
int  nbody_hermite_step(nbody_hermite* h, const nbody_state* s, double eps, void* stream);
/* Blocking.  what: 0 jerk T[n][D] | 1 predicted x T[n][D] | 2 predicted v T[n][D] of the last step (after force_jerk: x and v as
 * they were evaluated).  bytes must be n * D * sizeof(T) (NBODY_ERR_ARG); NBODY_ERR_STATE before the first force_jerk. */
int  nbody_hermite_read(nbody_hermite* h, int what, void* host_out, size_t bytes, void* stream);

/* ---- block (individual) time steps for the Hermite integrator: the Aarseth criterion on power-of-two steps -------------------
 * dt_max = s->dt is the largest step and the synchronisation interval, L = max_level (0 .. 20), tick = dt_max / 2^L.  Body i has a
 * level l_i in [0, L], a step of 2^(L - l_i) ticks and a last-update time tau_i in ticks since the start of the current interval
 * (integers: time accumulates no rounding); tau_i is always a multiple of the body's step.
 *   start       a and the jerk of all bodies (nbody_hermite_force_jerk); want_i = eta_start |a_i| / |j_i| (|j_i| = 0: level 0);
 *               l_i = the smallest level with dt_max 2^-l <= want_i, clamped to [0, L]; tau_i = 0.
 *   block step  tau_next = min_i(tau_i + step_i); the active set is every i with tau_i + step_i == tau_next, in ascending body
 *               order.  ALL bodies are predicted to tau_next with h_i = T(tau_next - tau_i) * T(tick) (the predictor above); a and
 *               the jerk of the ACTIVE bodies only, against all N predicted bodies; for each active body the corrector above with
 *               h = step_i * tick, then with a0, j0 the old and a1, j1 the new values
 *                 a2 = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2,  a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3,  a2 <- a2 + h a3
 *                 want = sqrt(eta (|a1| |a2| + |j1|^2) / (|j1| |a3| + |a2|^2))            (denominator 0: no limit)
 *               (1 / h is 2^l_i * fl_T(1 / T(dt_max)), an exact scaling).  New level: if want < h, the smallest level deeper than
 *               l_i whose step is <= want, at most L; else if want >= 2 h, l_i > 0 and tau_next is a multiple of twice the body's
 *               step, l_i - 1 (one doubling at most); else unchanged.  tau_i = tau_next.  Inactive bodies are not written.
 *   At tau_next = 2^L every body is active, the system is synchronous at t + dt_max, and tau starts again from 0.
 * With max_level = 0 a block step is nbody_hermite_step, bit for bit.  The active list is a stable compaction (no atomics decide a
 * slot) and the launch shape of the active set's force + jerk follows from (sz, n_active) alone, chunks added in chunk order: two
 * runs from the same state give the same bits.  The schedule arrays are allocated by the first block_start on a handle.
 *  - Argument errors before the device is touched, in this order: the state as for nbody_hermite_step; eps; eta / eta_start (finite,
 *    > 0, also as T); max_level (0 .. 20); h NULL; h made for another dtype, dim or n; s->dt (finite, > 0, tick and 1 / dt normal
 *    numbers of T); for a step, s->dt other than block_start's (all NBODY_ERR_ARG).
 *  - block_start allocates on first use and block_step / block_advance read the size of the active set back (8 bytes, blocking):
 *    all of them, and block_read, return NBODY_ERR_STATE between nbody_graph_begin and nbody_graph_end, and leave the capture usable.
 *  - block_step / block_advance / block_read before block_start on that handle, or after a later nbody_hermite_force_jerk (which
 *    restarts the fixed-step run): NBODY_ERR_STATE.  nbody_hermite_step may follow a block_advance (the system is synchronous). */
int  nbody_hermite_block_start(nbody_hermite* h, const nbody_state* s, double eps, double eta_start, int max_level, void* stream);
/* One block step.  *n_active: the size of its active set, *tau: its tau_next in ticks (2^max_level: the interval is complete);
 * either may be NULL.  Blocking for the schedule, asynchronous for the force + jerk and the corrector. */
int  nbody_hermite_block_step(nbody_hermite* h, const nbody_state* s, double eps, double eta, void* stream, uint32_t* n_active,
                              uint32_t* tau);
/* Block steps until the system is synchronous at t + s->dt.  *block_steps: how many, *body_steps: the sum of their active sets
 * (the force + jerk evaluations made); either may be NULL. */
int  nbody_hermite_block_advance(nbody_hermite* h, const nbody_state* s, double eps, double eta, void* stream, uint64_t* block_steps,
                                 uint64_t* body_steps);
/* Blocking.  what: 0 levels int32[n] | 1 tau_i uint32[n] | 2 the active list of the last block step, uint32[n_active] ascending.
 * bytes must match (NBODY_ERR_ARG). */
int  nbody_hermite_block_read(nbody_hermite* h, int what, void* host_out, size_t bytes, void* stream);

/* ---- sixth-order Hermite integrator for all-pairs (no reference counterpart) ------------------------------------------------------
 * The predictor-corrector of Nitadori & Makino (2008) with a fixed step and Plummer softening: one evaluation of the acceleration,
 * its first time derivative (the jerk) AND its second (the snap) per step, in one pair loop.  With e2 = fl_T(T(eps) * T(eps)),
 * d = x_j - x_i, u = v_j - v_i, b = a_j - a_i, q = |d|^2 + e2, w = m_j q^(-3/2), alpha = (d.u) / q, gamma = (|u|^2 + d.b) / q:
 *   a_i = c * sum_j w d,   j_i = c * sum_j w (u - 3 alpha d),   s_i = c * sum_j w (b - 6 alpha u + (15 alpha^2 - 3 gamma) d)
 * The self pair, and coincident bodies at equal velocity and acceleration, add 0 because d = u = b = 0: no branch, no index test.
 * w is the softened K1's weight, operation for operation; 1 / q comes from the same reciprocal square root (no divide, no second
 * transcendental).  eps obeys the rules of the softening section above; eps = 0 is NOT supported (NBODY_ERR_ARG), as in the
 * fourth-order integrator.  One step of h = T(dt) from (x, v, a0, j0, s0, k0), k0 the crackle kept from the previous step:
 *   predict   xp = x + h v + h^2/2 a0 + h^3/6 j0 + h^4/24 s0 + h^5/120 k0
 *             vp = v + h a0 + h^2/2 j0 + h^3/6 s0 + h^4/24 k0,      ap = a0 + h j0 + h^2/2 s0 + h^3/6 k0
 *   evaluate  (a1, j1, s1) at (xp, vp, ap), all bodies
 *   correct   v1 = v + h/2 (a0 + a1) + h^2/10 (j0 - j1) + h^3/120 (s0 + s1)
 *             x1 = x + h/2 (v + v1)  + h^2/10 (a0 - a1) + h^3/120 (j0 + j1)
 *   crackle   k1 = (60 (a1 - a0) - h (24 j0 + 36 j1) + h^2 (9 s1 - 3 s0)) / h^3     (1 / h^3 is computed once per call, as T)
 *   then      x <- x1, v <- v1, a <- a1, jerk <- j1, snap <- s1, crackle <- k1                                           (P(EC)^1)
 * The crackle term of the predictor is what makes the scheme sixth order.  The start evaluates twice, because the snap needs the
 * accelerations of all bodies: the first pass, with ap = 0, keeps a alone; the second, at (x, v, a), gives a (the same bits: the sum
 * of a does not read ap), the jerk and the snap; the crackle starts as 0, so the first step is one order lower, once.
 * The handle owns the jerk, the snap, the crackle, the packed predicted state and the partial sums; everything is allocated by
 * create, so start and step allocate nothing and may be recorded into a step graph.  A body's sums are added in an order that
 * follows from sz alone (no atomics, no waiting between blocks): two runs, an eager step and a replayed recorded one give the same
 * bits.  s->ao is neither read nor written.
 *  - Whole system only: first = 0, count = sz, else NBODY_ERR_ARG.
 *  - Argument errors are found before the device is touched, in the order of nbody_hermite_step: s NULL; the state's dtype, dim,
 *    window, tuning; eps (the message names the softening); h NULL; h made for another dtype, dim or n (all NBODY_ERR_ARG).
 *  - nbody_hermite6_step before nbody_hermite6_start on that handle: NBODY_ERR_STATE.  A handle used with a stream of another
 *    device: NBODY_ERR_ARG.  Every entry switches to the handle's device and restores the caller's.
 *  - nbody_hermite6_read and nbody_hermite6_create(_on) between nbody_graph_begin and nbody_graph_end: NBODY_ERR_STATE.
 * Block time steps for this scheme: nbody_hermite6_block_* below (nbody_hermite_block_* steps the fourth-order scheme). */
typedef struct nbody_hermite6 nbody_hermite6;
int  nbody_hermite6_create(nbody_hermite6** out, int dtype, int dim, uint32_t n);                /* on the current device */
int  nbody_hermite6_create_on(nbody_hermite6** out, int dtype, int dim, uint32_t n, int device); /* device < 0: the current one */
void nbody_hermite6_destroy(nbody_hermite6* h);                                                  /* NULL: no-op */
/* a = s->a and the handle's jerk and snap at (s->x, s->v), crackle = 0: starts a run, or restarts it after an upload.  Two
 * evaluations.  Asynchronous, recordable. */
int  nbody_hermite6_start(nbody_hermite6* h, const nbody_state* s, double eps, void* stream);
/* One step as above: reads s->x, s->v, s->a, the jerk, the snap and the crackle, rewrites them.  Asynchronous, recordable. */
int  nbody_hermite6_step(nbody_hermite6* h, const nbody_state* s, double eps, void* stream);
/* Blocking.  what: 0 jerk | 1 snap | 2 crackle | 3 predicted x | 4 predicted v | 5 predicted a of the last step (after start: x, v
 * and a as they were evaluated), each T[n][D].  bytes must be n * D * sizeof(T) (NBODY_ERR_ARG); NBODY_ERR_STATE before the first
 * start. */
int  nbody_hermite6_read(nbody_hermite6* h, int what, void* host_out, size_t bytes, void* stream);

/* ---- block (individual) time steps for the sixth-order Hermite integrator: NBODY_F64 only ---------------------------------------
 * Levels, ticks, tau, the active set and the level rule are those of nbody_hermite_block_* above, word for word: dt_max = s->dt,
 * L = max_level (0 .. 20), tick = dt_max / 2^L, a level l_i in [0, L], a step of 2^(L - l_i) ticks and an integer tau_i per body; the
 * active list in ascending body order, built by a stable compaction; deeper if want < h, one doubling at most and only onto the
 * coarser level's grid if want >= 2 h, a zero denominator means no limit.  What differs from the fourth order:
 *   start       nbody_hermite6_start's two evaluations: a, the jerk and the snap of all bodies, crackle = 0;
 *               want_i = eta_start |a_i| / |j_i| (|j_i| = 0: level 0), the fourth order's rule; tau_i = 0.
 *   predict     ALL bodies to tau_next with h_i = T(tau_next - tau_i) * T(tick): the three chains of nbody_hermite6_step's predictor
 *               (x to h^5 with the crackle, v to h^4, a to h^3) with h_i in place of h.
 *   evaluate    (a1, j1, s1) of the ACTIVE bodies only, against all N predicted bodies (a target's own x, v, a are its predicted ones).
 *   correct     per active body with h = step_i * tick: v1, x1 and the crackle k1 by nbody_hermite6_step's expressions, 1 / h^3 =
 *               2^(3 l_i) * fl_T(1 / (dt_max dt_max dt_max)) (an exact scaling); then a <- a1, jerk <- j1, snap <- s1, crackle <- k1,
 *               tau_i = tau_next (0 at 2^L).  Inactive bodies are not written.
 *   criterion   (Nitadori & Makino 2008) the derivatives at the new time of the quintic through (a0, j0, s0) at 0 and (a1, j1, s1) at h:
 *                 a3 = k1 = (60 (a1 - a0) - h (24 j0 + 36 j1) + h^2 (9 s1 - 3 s0)) / h^3
 *                 a4 = (360 (a1 - a0) - h (168 j0 + 192 j1) + h^2 (36 s1 - 24 s0)) / h^4
 *                 a5 = (720 (a1 - a0) - 360 h (j0 + j1) + 60 h^2 (s1 - s0)) / h^5
 *                 want = eta ((|a1| |s1| + |j1|^2) / (|a3| |a5| + |a4|^2))^(1/6), evaluated in T as eta * cbrt(sqrt(num / den))
 *               (1 / h is 2^l_i * fl_T(1 / T(dt_max)), 1 / h^4 and 1 / h^5 products of it with 1 / h^3).
 * float is refused.  a5 is a fifth difference of the force, of size (h / t)^5 |a| for a body whose force changes on the time scale t;
 * float force sums carry about 1e-6 |a| of rounding, which inflates a5, shrinks want, shrinks h and so grows 32-fold per halving: a
 * float run falls to the deepest level within one interval.  Use the fixed step or the fourth-order block steps in float.
 * With max_level = 0 a block step is nbody_hermite6_step: the launch shape of the active set's kernel follows from (sz, n_active)
 * alone by nbody_hermite_block_*'s rule with at least two chunks once there are two source tiles, which with every body active is the
 * fixed step's shape for every sz; chunks are added in chunk order.  Two runs from the same state give the same bits.  The schedule
 * arrays are allocated by the first block_start on a handle.
 *  - Argument errors before the device is touched, in this order: s NULL; the state's dtype, dim, window, tuning; the whole-system
 *    rule; dtype other than NBODY_F64 (the message names the fifth difference and float's rounding); eps; eta / eta_start (finite,
 *    > 0); max_level (0 .. 20); h NULL; h made for another dtype, dim or n; s->dt (finite, > 0; tick, 1 / dt and 2^(3 L) / dt^3
 *    normal and finite); for a step, s->dt other than block_start's (all NBODY_ERR_ARG).
 *  - Then a stream of another device (NBODY_ERR_ARG).  block_start allocates on first use and block_step / block_advance read the
 *    size of the active set back (8 bytes, blocking): all of them, and block_read, return NBODY_ERR_STATE between nbody_graph_begin
 *    and nbody_graph_end, and leave the capture usable.
 *  - block_step / block_advance / block_read before block_start on that handle, or after a later nbody_hermite6_start (which ends the
 *    block run): NBODY_ERR_STATE.  nbody_hermite6_step may follow a completed block_advance (the system is synchronous).
 *  - A schedule read back out of range (n_active, tau_next) ends the block run with NBODY_ERR_STATE. */
int  nbody_hermite6_block_start(nbody_hermite6* h, const nbody_state* s, double eps, double eta_start, int max_level, void* stream);
/* One block step.  *n_active: the size of its active set, *tau: its tau_next in ticks (2^max_level: the interval is complete);
 * either may be NULL.  Blocking for the schedule, asynchronous for the evaluation and the corrector. */
int  nbody_hermite6_block_step(nbody_hermite6* h, const nbody_state* s, double eps, double eta, void* stream, uint32_t* n_active,
                               uint32_t* tau);
/* Block steps until the system is synchronous at t + s->dt.  *block_steps: how many, *body_steps: the sum of their active sets
 * (the force + jerk + snap evaluations made); either may be NULL. */
int  nbody_hermite6_block_advance(nbody_hermite6* h, const nbody_state* s, double eps, double eta, void* stream, uint64_t* block_steps,
                                  uint64_t* body_steps);
/* Blocking.  what: 0 levels int32[n] | 1 tau_i uint32[n] | 2 the active list of the last block step, uint32[n_active] ascending.
 * bytes must match (NBODY_ERR_ARG). */
int  nbody_hermite6_block_read(nbody_hermite6* h, int what, void* host_out, size_t bytes, void* stream);

/* ---- block (individual) time steps for the octree leapfrog (no reference counterpart) ----------------------------------------
 * A per-body velocity-Verlet (kick-drift-kick) step on the level grid of the Hermite block steps above, with the force from the
 * softened monopole walk (nbody_octree_compute_softened_force).  dt_max = s->dt is the largest step and the synchronisation
 * interval, L = max_level (0 .. 20), tick = dt_max / 2^L.  Body i has a level l_i in [0, L], a step of 2^(L - l_i) ticks, a
 * last-update time tau_i in integer ticks since the start of the current interval (always a multiple of the body's step), and its
 * acceleration a_i = s->a[i] at (x_i, tau_i).  eps > 0 is required, as for the Hermite integrator.
 *   criterion   want_i = sqrt(2 eta eps / |a_i|), evaluated in T as sqrt(k / sqrt(|a_i|^2)) with k = T(2) * T(eta) * T(eps) and
 *               |a_i|^2 an FMA chain over the components; |a_i| = 0 means no limit.
 *   start       the tree on x (bounds, insert, multipoles), the softened monopole force of ALL bodies into s->a, then
 *               l_i = the smallest level with dt_max 2^-l <= want_i, clamped to [0, L] (no limit: level 0); tau_i = 0.
 *   block step  1. tau_next = min_i(tau_i + step_i);
 *               2. the active set is every i with tau_i + step_i == tau_next;
 *               3. ALL bodies are predicted: xp_i = x_i + h_i v_i + h_i^2/2 a_i, h_i = T(tau_next - tau_i) * T(tick), evaluated as
 *                  fma(h, fma(h/2, a, v), x);
 *               4. the tree is built on xp: clear, bounds, insert, multipoles, as a fixed step builds it on x;
 *               5. a1 = the softened monopole force of the ACTIVE bodies only, walked from that tree in key order by the kernel of
 *                  nbody_octree_compute_softened_force (so a1_i is bit for bit what that call gives body i on the positions xp);
 *               6. for each active body v_i += h_i/2 (a_i + a1_i) (as fma(h/2, a + a1, v)), x_i = xp_i, a_i = a1_i, the new level,
 *                  tau_i = tau_next.  New level, the Hermite block steps' rule with h = the body's step and want from a1: if
 *                  want < h, the smallest level deeper than l_i whose step is <= want, at most L; else if want >= 2 h (or no
 *                  limit), l_i > 0 and tau_next is a multiple of twice the body's step, l_i - 1 (one doubling at most); else l_i;
 *               7. inactive bodies are not written (x, v, a, level, tau);
 *               8. at tau_next = 2^L every body is active, the system is synchronous at t + dt_max, and tau starts again from 0.
 * s->ao is neither read nor written.  Both active lists (ascending body order for the kick and for block_read, key order for the
 * walk) are stable compactions — no atomic decides a slot — and a body's force is the walk's, which has no cross-body reduction: two
 * runs from the same state give the same bits.
 *  - Scope: monopole and softened only; the whole system only (first = 0, count = sz).  Not recordable into a step graph: a block
 *    step reads (n_active, tau_next) back (8 bytes, blocking).
 *  - The handle owns the levels, tau, the schedule words, both active lists, xp and the scratch for a1; all allocated by create.
 *    The tree is the caller's: any nbody_octree made for the same (dtype, dim, n).  A block step leaves it built on xp, with its phase
 *    flags as after nbody_octree_compute_tree; nbody_octree_info after a step or an advance reports a build that hit the depth limit
 *    or the node pool on ANY block step since the last call (the device-side flag is sticky).
 *  - Argument errors before the device is touched, in this order (all NBODY_ERR_ARG): s NULL; the state's dtype, dim, window, tuning;
 *    the whole-system rule; eps (the message names the softening); eta (finite, > 0, also as T, and 2 eta eps a positive finite T);
 *    max_level (0 .. 20; start only); h NULL; t NULL; h, then t, made for another dtype, dim or n; s->dt (finite, > 0, tick a normal
 *    number of T).  Then: a handle or tree used with a stream of another device (NBODY_ERR_ARG); any of start / step / advance / read
 *    between nbody_graph_begin and nbody_graph_end (NBODY_ERR_STATE; the capture stays usable); a tree after
 *    nbody_octree_set_walk(t, 2) (NBODY_ERR_ARG with the softened walk's message, as nbody_octree_compute_softened_force returns it);
 *    step / advance / read before start on that handle (NBODY_ERR_STATE); for a step, s->dt other than start's (NBODY_ERR_ARG). */
typedef struct nbody_octree_block nbody_octree_block;
int  nbody_octree_block_create(nbody_octree_block** out, int dtype, int dim, uint32_t n);                /* on the current device */
int  nbody_octree_block_create_on(nbody_octree_block** out, int dtype, int dim, uint32_t n, int device); /* device < 0: the current one */
void nbody_octree_block_destroy(nbody_octree_block* h);
/* Starts a run (or restarts it after an upload): the force of all bodies into s->a, the first levels, tau = 0. */
int  nbody_octree_block_start(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, double theta, double eps, double eta,
                              int max_level, void* stream);
/* One block step.  *n_active: the size of its active set, *tau: its tau_next in ticks (2^max_level: the interval is complete);
 * either may be NULL.  Blocking for the schedule, asynchronous for the walk and the kick. */
int  nbody_octree_block_step(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, double theta, double eps, double eta,
                             void* stream, uint32_t* n_active, uint32_t* tau);
/* Block steps until the system is synchronous at t + s->dt.  *block_steps: how many, *body_steps: the sum of their active sets (the
 * force evaluations made); either may be NULL. */
int  nbody_octree_block_advance(nbody_octree_block* h, nbody_octree* t, const nbody_state* s, double theta, double eps, double eta,
                                void* stream, uint64_t* block_steps, uint64_t* body_steps);
/* Blocking.  what: 0 levels int32[n] | 1 tau_i uint32[n] | 2 the active list of the last block step, uint32[n_active] in ascending
 * body order | 3 the predicted positions xp of the last block step, T[n][D].  bytes must match (NBODY_ERR_ARG); 2 and 3 before the
 * first block step: NBODY_ERR_STATE. */
int  nbody_octree_block_read(nbody_octree_block* h, int what, void* host_out, size_t bytes, void* stream);

/* ---- all-pairs per-body potentials, nearest neighbours and the closest pair (no reference counterpart) --------------------------
 * What a direct-sum code reports beside the force: how deep body i sits in the potential, and who its nearest neighbour is.  Reads a
 * state's (m, x) and changes nothing in it, so it works after any algorithm or integrator, also at the synchronous end of a
 * block-step advance.  With T the state's type, D its dimension, e2 = fl_T(T(eps) * T(eps)) and d = x_j - x_i:
 *   d2_ij      the UNSOFTENED squared distance, computed as one FMA chain in component order: t = d_0 * d_0, then t = fma(d_k, d_k, t).
 *              Bitwise symmetric in (i, j), because x_i - x_j is the exact negation of x_j - x_i.
 *   q_ij       d2_ij + e2.
 *   potential  phi_i = -c * S_i, S_i = sum_{j != i} m_j / sqrt(q_ij): the sign and scaling of the octree potentials above and the pair
 *              form of nbody_calc_energies_softened.  The self pair is excluded BY INDEX (its term would be m_i / eps, not 0);
 *              coincident distinct bodies contribute m_j / eps.  One reciprocal square root per pair (v_rsq_f64 polished to third
 *              order in double, the bare v_rsq_f32 in float, as the softened energies take it); no divide, no sqrt.
 *   neighbour  nn_i = the j != i with the smallest computed d2_ij, the LOWEST index among equal computed values; nnd2_i = that d2.
 *              Selection is on the unsoftened d2, so nn and nnd2 do not depend on eps: the same bits for any valid eps.
 *              n = 1: nn_0 = 0xffffffff, nnd2_0 = +inf, phi_0 = 0.
 *   closest    the pair (i, j), i < j, with the smallest d2; ties to the lowest i, then the lowest j.  Because d2 is symmetric this
 *              is the body of lowest index among those with minimal nnd2, together with its nn.  n = 1: (0xffffffff, 0xffffffff, +inf).
 * eps obeys the rules of the softening section above; eps = 0 is NOT supported (NBODY_ERR_ARG): the unsoftened potential's pair is the
 * reference's m / (|d| + eps(T)), a different form.
 * The rounding order of S_i follows from sz alone (the terms of 64 consecutive sources summed by themselves, those sums added per
 * wave, tile by tile, the block's waves in wave order, the chunks of the source range in chunk order): no atomics, no waiting between
 * blocks, nothing read from the device or the CU count; nn has an exact tie rule.  Two runs give the same bits for every output, and
 * so do an eager call and a replayed recorded one, and a handle destroyed and made again.
 *  - create allocates everything (packed records, the chunks' partial arrays, the three result arrays, the closest-pair record); the
 *    handle owns the results.  create(_on) between nbody_graph_begin and nbody_graph_end: NBODY_ERR_STATE.
 *  - compute reads s->m and s->x only: s->v, s->a and s->ao may be NULL or garbage.  Asynchronous, allocates nothing, may be recorded
 *    into a step graph; four launches, the last a small one that produces the closest-pair record.  Whole system only (first = 0,
 *    count = sz).
 *  - Argument errors of compute are found before the device is touched, in the order of nbody_hermite_step: s NULL; the state's
 *    dtype, dim, window, tuning; the whole-system rule; eps (the message names the softening); h NULL; h made for another dtype, dim
 *    or n (all NBODY_ERR_ARG).  Then a stream of another device (NBODY_ERR_ARG).
 *  - read and closest_pair are blocking; NBODY_ERR_STATE before the first compute on that handle and between nbody_graph_begin and
 *    nbody_graph_end (the capture stays usable).  Every entry switches to the handle's device and restores the caller's. */
typedef struct nbody_neighbours nbody_neighbours;
int  nbody_neighbours_create(nbody_neighbours** out, int dtype, int dim, uint32_t n);                /* on the current device */
int  nbody_neighbours_create_on(nbody_neighbours** out, int dtype, int dim, uint32_t n, int device); /* device < 0: the current one */
void nbody_neighbours_destroy(nbody_neighbours* h);                                                  /* NULL: no-op */
/* phi, nn, nnd2 of all bodies and the closest pair at (s->m, s->x), into the handle.  Asynchronous, recordable. */
int  nbody_neighbours_compute(nbody_neighbours* h, const nbody_state* s, double eps, void* stream);
/* Blocking.  what: 0 phi T[n] | 1 nn uint32[n] | 2 nnd2 T[n] of the last compute.  bytes must match (NBODY_ERR_ARG; what and
 * bytes = 0 are refused before the handle is looked at). */
int  nbody_neighbours_read(nbody_neighbours* h, int what, void* host_out, size_t bytes, void* stream);
/* Blocking.  The closest pair of the last compute: *i < *j and its d2 as one T; any of the three may be NULL. */
int  nbody_neighbours_closest_pair(nbody_neighbours* h, uint32_t* i, uint32_t* j, void* d2_out, void* stream);

/* ---- all-pairs k nearest neighbours, local densities, the density centre (no reference counterpart) ------------------------------
 * The Casertano & Hut (1985) diagnostics of a star cluster: each body's local density from its k-th neighbour (conventionally k = 6),
 * the density centre, the core radius and the core density.  Reads a state's (m, x) and changes nothing in it.  Selection is on the
 * UNSOFTENED squared distance, so there is no eps: it works after any algorithm or integrator, also unsoftened.  With T the state's
 * type, D its dimension and d = x_j - x_i:
 *   d2_ij      exactly the d2 of the neighbours section above (one FMA chain in component order, bitwise symmetric in (i, j)).
 *   order      the k neighbours of i are the k smallest (d2_ij, j), j != i, in lexicographic order — equal computed d2 resolve to the
 *              LOWEST index — listed ascending in that order.  The self pair is excluded by index.  A body has min(k, n - 1)
 *              neighbours; unused slots hold index 0xffffffff and d2 +inf.  Column 0 is nn / nnd2 of nbody_neighbours_compute, bit
 *              for bit.
 *   k          fixed at create, 1 <= k <= NBODY_KNN_MAX.  The sweep carries a list of capacity 4, 8 or 16 (the smallest >= k); the
 *              tie rule is exact, so the first k entries do not depend on the capacity: the k neighbours of a handle made for k are
 *              the first k of a handle made for any larger k.
 *   density    rho_i = M_i / V, M_i the masses of neighbours 0 .. k - 2 added in list order (the k-th itself excluded: Casertano &
 *              Hut's unbiased form), d2_k the k-th squared distance: 3D rho_i = M_i / (T(4 pi / 3) * (d2_k * sqrt(d2_k))), 2D rho_i =
 *              M_i / (T(pi) * d2_k); correctly rounded sqrt, true divide.  k = 1, or fewer than k neighbours (n <= k): rho_i = 0.
 *              d2_k = 0 (coincident bodies): what IEEE gives (+inf).
 *   summary    x_dc = sum rho x / sum rho (the density centre); r_c = sqrt(sum rho^2 |x - x_dc|^2 / sum rho^2) (the core radius, the
 *              rho^2-weighted NBODY form); rho_c = sum rho^2 / sum rho (the core density).  Summed in double for both types in a
 *              fixed order, rounded to T.  sum rho = 0 (k = 1, n <= k) or a non-finite rho (coincident bodies) gives NaN by IEEE
 *              rules: that is not an error.
 * No atomics, no waiting between blocks, nothing read from the device or the CU count: the cut of the work follows from sz alone.
 * Two runs give the same bits for every output, and so do an eager call and a replayed recorded one, and a handle destroyed and made
 * again.
 *  - create allocates everything (packed records, the chunks' partial lists uint32/T[chunk][n][capacity], the three result arrays,
 *    the summary record) and frees everything again if one allocation fails; the handle owns the results.  Argument errors in this
 *    order: out NULL, dtype, dim, n = 0 or n > 2^28, k outside 1 .. NBODY_KNN_MAX (all NBODY_ERR_ARG).  create(_on) between
 *    nbody_graph_begin and nbody_graph_end: NBODY_ERR_STATE.
 *  - compute reads s->m and s->x only: s->v, s->a and s->ao may be NULL or garbage.  Asynchronous, allocates nothing, may be recorded
 *    into a step graph; four launches.  Whole system only (first = 0, count = sz).
 *  - Argument errors of compute are found before the device is touched, in this order: s NULL; the state's dtype, dim, window,
 *    tuning; the whole-system rule; h NULL; h made for another dtype, dim or n (all NBODY_ERR_ARG).  Then a stream of another device
 *    (NBODY_ERR_ARG).
 *  - read and density_centre are blocking; NBODY_ERR_STATE before the first compute on that handle and between nbody_graph_begin and
 *    nbody_graph_end (the capture stays usable).  Every entry switches to the handle's device and restores the caller's. */
#define NBODY_KNN_MAX 16
typedef struct nbody_knn nbody_knn;
int  nbody_knn_create(nbody_knn** out, int dtype, int dim, uint32_t n, int k);                /* on the current device */
int  nbody_knn_create_on(nbody_knn** out, int dtype, int dim, uint32_t n, int k, int device); /* device < 0: the current one */
/* The method of a handle.  ALL_PAIRS (what create and create_on make): every body meets every other one, O(n^2).  TREE: an EXACT
 * search that prunes with bounding boxes over a space-sorted copy of the bodies, for large n.
 * Contract of TREE: every output of nbody_knn_read (what = 0, 1, 2) and nbody_knn_density_centre equals, BIT FOR BIT, what an
 * ALL_PAIRS handle of the same (dtype, dim, n, k) gives on the same state, for any finite positions and any order of the bodies in
 * the state: the tie rule above is exact, so the result is a set with one correct answer.  That covers exact ties, coincident bodies,
 * n <= k (unused slots 0xffffffff / +inf, rho = 0) and n = 1.  The state is neither changed nor permuted.  Speed depends on the input
 * (clustering, the order does not matter: the bodies are sorted along a Morton curve by every compute); results do not.  Non-finite
 * positions are outside the contract (the call stays memory-safe; the outputs of the two methods may differ).
 *  - create_method takes the argument checks of create_on in the same order, `method` (NBODY_ERR_ARG outside {0, 1}) after k.  A TREE
 *    handle allocates the packed records, the sorted records, the boxes, the keys, the permutation and the sort's scratch (sized
 *    at create from n), the three result arrays and the summary record — and NOT the chunks' partial lists of ALL_PAIRS.
 *  - compute dispatches on the handle's method; argument errors, state rules, read and density_centre are the same for both.  For
 *    TREE it is still asynchronous, allocates nothing and may be recorded into a step graph; the number of launches (pack, bounds,
 *    keys, the sort, gather, upper levels, walk, finish, summary) is a function of n alone.
 *  - nbody_knn_method: the method the handle was made for; h NULL: -1, and nbody_last_error() says so. */
#define NBODY_KNN_ALL_PAIRS 0
#define NBODY_KNN_TREE      1
int  nbody_knn_create_method(nbody_knn** out, int dtype, int dim, uint32_t n, int k, int method, int device); /* device < 0: current */
int  nbody_knn_method(const nbody_knn* h);
void nbody_knn_destroy(nbody_knn* h);                                                         /* NULL: no-op */
/* The k neighbours, rho of all bodies and the summary at (s->m, s->x), into the handle.  Asynchronous, recordable. */
int  nbody_knn_compute(nbody_knn* h, const nbody_state* s, void* stream);
/* Blocking.  what: 0 idx uint32[n][k] | 1 d2 T[n][k] | 2 rho T[n] of the last compute, row-major.  bytes must match (NBODY_ERR_ARG;
 * what and bytes = 0 are refused before the handle is looked at). */
int  nbody_knn_read(nbody_knn* h, int what, void* host_out, size_t bytes, void* stream);
/* Blocking.  The summary of the last compute: centre_out T[dim], the core radius and the core density one T each; any of the three
 * may be NULL. */
int  nbody_knn_density_centre(nbody_knn* h, void* centre_out, void* core_radius_out, void* core_density_out, void* stream);

/* ---- friends-of-friends groups (no reference counterpart) ---------------------------------------------------------------------------
 * Which bodies belong together: clumps, sub-clusters, escapers, the core against the halo.  Reads a state's (m, x) and changes nothing
 * in it; positions only — no softening, no periodic wrap, no velocities.  With T the state's type and D its dimension:
 *   link       i and j (i != j) are friends iff d2_ij <= b2.  d2_ij is exactly the d2 of the neighbours and kNN sections above (one
 *              FMA chain in component order, contraction off, bitwise symmetric in (i, j)); b2 = T(b) * T(b), rounded once in T on the
 *              host; b is a double argument of compute.  b = 0 is legal and links only bodies whose computed d2 is 0.
 *   group      a connected component of the friend relation.  label[i] is the LOWEST original index among the members of i's group,
 *              so label[i] <= i, and label[i] == i for exactly one member of each group; size[i] is the member count of i's group.
 *              Both uint32_t[n] in the state's body order.  They are integers with one correct answer: neither depends on the order
 *              of the bodies in the state beyond the renaming, nor on how the bodies happen to be scheduled.
 *   summary    uint32_t[4]: the number of groups, the number of catalogued groups c, the largest size, the label of the largest group
 *              (among groups of equal largest size the lowest label).
 *   catalogue  the groups with size >= min_members, in ascending label order; min_members is fixed at create.  Per entry: label
 *              (uint32), size (uint32), mass (T), com[D] (T).  Mass and sum(m x) are accumulated in DOUBLE for both types in an order
 *              that is a fixed function of the group's member list in ascending original index (member t goes to partial t mod 64,
 *              the 64 partials are folded by a fixed tree), com = sum(m x) / sum(m), each converted to T once.
 *              Masses may be zero (tracers): a catalogued group whose masses sum to 0 has mass 0 and com = 0 / 0 = NaN by IEEE
 *              rules, which is not an error (label and size do not look at the masses).
 * The search is exact: the tree of the kNN section's TREE method prunes with a bound that needs no tolerance, and a group is built
 * with a lock-free union-find over integer indices.  No floating-point atomics anywhere: two computes of the same state give the
 * same bits for every output, and so do an eager call and a replayed recorded one, and a handle destroyed and made again.  No loop of
 * any kernel waits for another lane, wave or block.  Non-finite positions are outside the contract (the call stays memory-safe; a NaN
 * distance links nothing).
 *  - create allocates everything (packed and sorted records, boxes, keys, the sort's scratch, the union-find arrays, label, size, a
 *    catalogue of n / min_members entries, the summary) and frees everything again if one allocation fails.  Argument errors in this
 *    order: out NULL, dtype, dim, n = 0 or n > 2^28, min_members outside 1 .. n (all NBODY_ERR_ARG).  create(_on) between
 *    nbody_graph_begin and nbody_graph_end: NBODY_ERR_STATE.
 *  - compute reads s->m and s->x only: s->v, s->a and s->ao may be NULL or garbage.  Asynchronous, allocates nothing, reads nothing
 *    back, may be recorded into a step graph; the number of launches is a function of n alone.  Whole system only.
 *  - Argument errors of compute are found before the device is touched, in this order: s NULL; the state's dtype, dim, window,
 *    tuning; the whole-system rule; h NULL; h made for another dtype, dim or n; b negative, NaN or infinite; b2 not finite in T (all
 *    NBODY_ERR_ARG).  Then a stream of another device (NBODY_ERR_ARG).
 *  - read and summary are blocking; NBODY_ERR_STATE before the first compute on that handle and between nbody_graph_begin and
 *    nbody_graph_end (the capture stays usable).  Every entry switches to the handle's device and restores the caller's. */
typedef struct nbody_fof nbody_fof;
int  nbody_fof_create(nbody_fof** out, int dtype, int dim, uint32_t n, uint32_t min_members);                /* on the current device */
int  nbody_fof_create_on(nbody_fof** out, int dtype, int dim, uint32_t n, uint32_t min_members, int device); /* device < 0: the current one */
void nbody_fof_destroy(nbody_fof* h);                                                                        /* NULL: no-op */
/* label, size, the summary and the catalogue at (s->m, s->x) for the linking length b, into the handle.  Asynchronous, recordable. */
int  nbody_fof_compute(nbody_fof* h, const nbody_state* s, double b, void* stream);
/* Blocking.  what: 0 label uint32[n] | 1 size uint32[n]: bytes must be n * 4.  2 label uint32[c] | 3 size uint32[c] | 4 mass T[c] |
 * 5 com T[c][dim] of the catalogue: bytes must be c * the element's size; the call reads c back itself, so nbody_fof_summary need not
 * have been called (c = 0: bytes = 0, nothing is written, host_out may be NULL).  Order of the argument errors: what, h NULL, then for
 * 0 / 1 host_out NULL and bytes; the state rules; then for 2 .. 5 bytes and host_out NULL. */
int  nbody_fof_read(nbody_fof* h, int what, void* host_out, size_t bytes, void* stream);
/* Blocking.  out4: the summary of the last compute. */
int  nbody_fof_summary(nbody_fof* h, uint32_t* out4, void* stream);

/* ---- exact fixed-radius neighbour lists on the same tree (no reference counterpart) ----------------------------------------------
 * Every neighbour of every body within a radius, as a variable-length list per body.  T the state's type, D its dimension:
 *   neighbour  j is a neighbour of i iff j != i and d2_ij <= r2_i, d2 the unsoftened squared distance of the kNN section (one FMA
 *              chain in component order, bitwise symmetric in (i, j)).
 *   radius     scalar (the default): r2_i = T(r) * T(r), rounded once in T on the host; r is compute's argument, r = 0 is legal and
 *              finds the bodies whose computed d2 is 0.  The relation is then symmetric.  Per-body radii (nbody_nlist_set_radii):
 *              r2_i = v_i * v_i, one multiply in T, or r2_i = v_i with squared = 1.  That is a gather: i's own radius decides, so i
 *              may list j without j listing i.
 *   count      uint32_t[n]: the number of neighbours of every body, in the state's body order.
 *   offset     uint64_t[n + 1]: the exclusive prefix sum of count in body order; offset[n] is the total.
 *   list       uint32_t[total]: the neighbours of i are list[offset[i] .. offset[i + 1]), in ascending index.
 *   summary    uint64_t[4]: the total, the largest count, the lowest index that has it, status.
 *   status     NBODY_NLIST_OVER_CAPACITY: total > capacity; NBODY_NLIST_OVER_PER_BODY: the largest count exceeds
 *              NBODY_NLIST_MAX_PER_BODY.  Either means that the list was NOT produced by this compute (nbody_nlist_read of the list
 *              returns NBODY_ERR_STATE); count, offset and summary are always valid, and a later compute that fits clears the status.
 *   capacity   the number of list entries the handle can hold, 0 .. 2^32, fixed at create.  capacity = 0 makes a counts-only handle:
 *              it skips the two passes that produce the list.
 * The lists are sets with one correct answer: they do not depend on the order of the bodies in the state beyond the renaming, on
 * scheduling, or on how the tree was built.  The search is exact: the tree of the kNN section's TREE method prunes with a bound that
 * needs no tolerance, and a body at exactly r2_i is listed.  No atomics anywhere: two computes of the same state give the same bits
 * for every output, and so do an eager call and a replayed recorded one, and a handle destroyed and made again.  No loop of any kernel
 * waits for another lane, wave or block.  Non-finite positions are outside the contract (the call stays memory-safe; a NaN distance is
 * within no radius).
 *  - create allocates everything (packed and sorted records, boxes, keys, the sort's scratch, the radii, count, offset, the scan's
 *    strips, two arrays of capacity entries, the summary) and frees everything again if one allocation fails.  Argument errors in
 *    this order: out NULL, dtype, dim, n = 0 or n > 2^28, capacity > 2^32 (all NBODY_ERR_ARG).  create(_on) between
 *    nbody_graph_begin and nbody_graph_end: NBODY_ERR_STATE.
 *  - set_radii is blocking.  host_values: T[n] on the host, bytes = n * sizeof(T); NULL with bytes = 0 returns the handle to the
 *    scalar radius.  Every r2_i must be finite and >= 0 and every v_i >= 0: checked on the host before anything is copied; a bad
 *    value is NBODY_ERR_ARG with a message that names the first offending index, and the handle keeps the radii it had.  Order: h
 *    NULL, host_values NULL, bytes, squared not 0 or 1 (NBODY_ERR_ARG); the stream's device; between nbody_graph_begin and
 *    nbody_graph_end NBODY_ERR_STATE; then the values.  It may be called before the first compute.
 *  - compute reads s->m and s->x only: s->v, s->a and s->ao may be NULL or garbage.  Asynchronous, allocates nothing, reads nothing
 *    back, may be recorded into a step graph (a recording keeps the radius, or the use of the per-body radii, it was made with); the
 *    number of launches is fixed at create (it follows from n, and from whether capacity is 0).  Whole system only.
 *  - Argument errors of compute are found before the device is touched, in this order: s NULL; the state's dtype, dim, window,
 *    tuning; the whole-system rule; h NULL; h made for another dtype, dim or n; and when the handle holds no radii: r negative, NaN
 *    or infinite; r2 not finite in T (all NBODY_ERR_ARG).  With radii set r is ignored.  Then a stream of another device
 *    (NBODY_ERR_ARG).
 *  - read and summary are blocking; NBODY_ERR_STATE before the first compute on that handle and between nbody_graph_begin and
 *    nbody_graph_end (the capture stays usable).  Every entry switches to the handle's device and restores the caller's. */
#define NBODY_NLIST_MAX_PER_BODY 4096
#define NBODY_NLIST_OVER_CAPACITY 1u
#define NBODY_NLIST_OVER_PER_BODY 2u
typedef struct nbody_nlist nbody_nlist;
int  nbody_nlist_create(nbody_nlist** out, int dtype, int dim, uint32_t n, uint64_t capacity);                /* on the current device */
int  nbody_nlist_create_on(nbody_nlist** out, int dtype, int dim, uint32_t n, uint64_t capacity, int device); /* device < 0: the current one */
void nbody_nlist_destroy(nbody_nlist* h);                                                                     /* NULL: no-op */
/* Blocking.  Per-body radii (squared = 0) or squared radii (squared = 1) for every later compute; NULL, 0: the scalar radius again. */
int  nbody_nlist_set_radii(nbody_nlist* h, const void* host_values, size_t bytes, int squared, void* stream);
/* count, offset, the summary and (if it fits) the list at (s->m, s->x) for the radius r, into the handle.  Asynchronous, recordable. */
int  nbody_nlist_compute(nbody_nlist* h, const nbody_state* s, double r, void* stream);
/* Blocking.  what: 0 count uint32[n]: bytes must be n * 4 | 1 offset uint64[n + 1]: bytes must be (n + 1) * 8 | 2 list uint32[total]:
 * bytes must be total * 4; the call reads the total back itself, so nbody_nlist_summary need not have been called (total = 0: bytes =
 * 0, nothing is written, host_out may be NULL).  A list read after a compute whose status is not 0 returns NBODY_ERR_STATE with a
 * message that says which limit was hit: the needed total and the capacity, or the largest count.  Order of the argument errors:
 * what, h NULL, then for 0 / 1 host_out NULL and bytes; the state rules; then for 2 the status, bytes and host_out NULL. */
int  nbody_nlist_read(nbody_nlist* h, int what, void* host_out, size_t bytes, void* stream);
/* Blocking.  out4: the summary of the last compute. */
int  nbody_nlist_summary(nbody_nlist* h, uint64_t* out4, void* stream);

/* ---- owning context (device mirrors of a host System), used by the C++ CLI host ------------------ */

typedef struct nbody_ctx nbody_ctx;
/* Allocates device arrays for n bodies on `device` and a private stream. */
int  nbody_create(nbody_ctx** out, int dtype, int dim, uint32_t n, int device);
void nbody_destroy(nbody_ctx* ctx);
/* Host -> device copy of the System arrays (T[n], vec<T,D>[n] x4) and the scalars dt, c. Blocking. */
int  nbody_upload(nbody_ctx* ctx, const void* m, const void* x, const void* v, const void* a, const void* ao, double dt,
                  double c);
/* Device -> host; any pointer may be NULL to skip that array.  m too: bvh permutes it. Blocking. */
int  nbody_download(nbody_ctx* ctx, void* m, void* x, void* v, void* a, void* ao);
/* The device view and stream of the context, to pass to the phase calls above. */
int  nbody_ctx_state(nbody_ctx* ctx, nbody_state* out);
void* nbody_ctx_stream(nbody_ctx* ctx);
/* Blocks until all work queued on `stream` has completed (so wall-clock phase timers are honest). */
int  nbody_stream_sync(void* stream);
/* K1 launch shape of THIS context (0 = auto for each; see nbody_all_pairs_configure / nbody_all_pairs_source_path). */
int  nbody_ctx_configure_all_pairs(nbody_ctx* ctx, int split, int targets_per_thread, int source_path);
/* Multi-GPU all-pairs: this context owns target bodies [first, first+count) of the n it was created for.  m and x stay
 * whole (sources); nbody_ctx_state then returns the window with v/a/ao pointing at the owned rows, and nbody_download
 * writes only the owned rows of x, v, a, ao (at their place in the full-size host arrays) plus all of m. */
int  nbody_ctx_set_shard(nbody_ctx* ctx, uint32_t first, uint32_t count);
/* What K1 will launch for this view, e.g. "all_pairs_force_sgpr_kernel<double,3,R=2,JS=8> tile=512 pair=far3/near2"
 * (bench.py stamps its profiles with it). */
int  nbody_all_pairs_describe(const nbody_state* s, char* out, size_t len);
/* What K2 (nbody_all_pairs_collapsed_force) will launch for this state: the kernel and its launch shape on one line, e.g.
 * "all_pairs_collapsed_stream_kernel<8> hand float 3 padded=33792 nbatches=66 bpc=4 chunks=17" (float: the streamed form; bpc =
 * batches per source chunk) or "all_pairs_collapsed_kernel<double,3,NT=8,KS=8,NB=1> tile=1024 iblocks=129 ntiles=33 tpb=2
 * ysplit=17" (double: the tile form; tpb = source tiles per block row).  Host arithmetic only: no stream, no GPU work. */
int  nbody_all_pairs_collapsed_describe(const nbody_state* s, char* out, size_t len);
/* Which per-pair rounding form K1 (sz >= 32768) takes for this state — a property of ALL sz positions, the same on every rank
 * and for every shard window: *sparse_out = 1 when the volume (area in 2D; through *volume_out if not NULL) of the uniformly
 * filled box that has the positions' variances, prod_k sqrt(12 var_k), is at least 1.7e5 (6.4e4 in 2D); pairs at r^2 >= 4 then
 * drop the eps term of m / (r^3 + eps), which is below an eighth of an ulp there (float: they take m r^-3 from the reciprocal
 * square root alone).  0: the dense rule (always below 32768 bodies).  The moments are summed in a fixed order (same bits on
 * every rank and in every run).  Until ABI 2.2 the volume was the bounding box's, which a single escaping body inflates at
 * will: config 2 as written took the sparse rule from its 36th step on with every batch of pairs holding a close one (+ 8.5 %).
 * Either form is within 2.5 ulp per term, but a system that spreads out moves from one to the other between two steps; tests
 * and bitwise A/B runs query the rule in force with this call.  Blocking (one reduction + a 16-byte copy). */
int  nbody_all_pairs_pair_rule(const nbody_state* s, void* stream, int* sparse_out, double* volume_out);

/* ---- the collective: per-step all-gather of position shards (multi-GPU all-pairs; no reference counterpart) ------
 * RCCL over xGMI.  Partition fixed by the ABI: rank r of W owns bodies [sz*r/W, sz*(r+1)/W) (nbody_shard_range).
 * Every rank holds all of x; nbody_allgather_positions fills in the other ranks' rows in place, asynchronously on
 * `stream` (stream-ordered after the K3 that moved the owned rows): one in-place ncclAllGather when W divides sz,
 * else one grouped ncclSend/ncclRecv per peer.  RCCL is loaded on first use (dlopen), never at library load.
 *  - one process per GPU: rank 0 calls nbody_comm_get_unique_id, the launcher hands the NBODY_COMM_ID_BYTES to every
 *    rank (bench.py: torch.distributed broadcast), each rank calls nbody_comm_create;
 *  - one process, several GPUs (the CLI's --gpus N): nbody_comm_create_all (ncclCommInitAll); the host thread brackets
 *    the per-device nbody_allgather_positions calls of a step with nbody_comm_group_begin/end. */
typedef struct nbody_comm nbody_comm;
#define NBODY_COMM_ID_BYTES 128
int  nbody_comm_get_unique_id(void* id_out);
int  nbody_comm_create(nbody_comm** out, int world, int rank, const void* unique_id, int device);
int  nbody_comm_create_all(nbody_comm** out /* [ndev] */, int ndev, const int* devices /* NULL = 0..ndev-1 */);
void nbody_comm_destroy(nbody_comm* comm);
int  nbody_comm_world(const nbody_comm* comm);
int  nbody_comm_rank(const nbody_comm* comm);
int  nbody_comm_rccl_version(void); /* ncclGetVersion code, 0 if RCCL cannot be loaded */
void nbody_shard_range(uint32_t sz, int world, int rank, uint32_t* first, uint32_t* count);
int  nbody_comm_group_begin(void);
int  nbody_comm_group_end(void);
int  nbody_allgather_positions(nbody_comm* comm, const nbody_state* s, void* stream);

/* ---- step graphs ----------------------------------------------------------------------------------------
 * A simulation step is a fixed sequence of phase calls (5 launches for all-pairs, ~40 for bvh).  Between
 * nbody_graph_begin and nbody_graph_end the phase calls made on `stream` are recorded instead of executed
 * (HIP stream capture); nbody_graph_launch replays the whole step with one submission.  Only the asynchronous
 * phase calls may be recorded (no upload/download/read/get/sync/calc_energies inside a capture). */
typedef struct nbody_graph nbody_graph;
int  nbody_graph_begin(void* stream);
int  nbody_graph_end(void* stream, nbody_graph** out);
int  nbody_graph_launch(nbody_graph* g, void* stream);
void nbody_graph_destroy(nbody_graph* g);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_H */
