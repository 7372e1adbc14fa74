"""GPU: the octree walks per body against the oracle's wide walk (oracle.octree_walk_wide, validated on the CPU by
tests/test_oracle_octree_wide.py, which also owns the systems): the monopole, softened and quadrupole force, the three potentials,
the tree energies and one block step of the octree leapfrog, at theta 0.5 and 1.0, where cells are accepted — down to the
quadrupoles of cells below the key depth (the deep system) and the index by which a walk fetches a cell's Q.

The oracle makes the reference's opening decisions and the GPU's per-body counters are held to them bit for bit, so body i of the GPU
and of the wide walk accumulate the same nodes and no body is left out.  Bounds, per body and component, against the body's own sum of
term magnitudes: |a - a_wide| <= FORCE_TOL * scale_a (the project's force bound: 1e-12 double, 2e-5 float) and
|phi + c s_wide| <= THETA0_TOL * c * scale_s (tests/test_gpu_tree_energy.py's: 1e-13, 3e-5).

The figures an MI355X gave are in profiles/tests_octree_wide/new_tests_figures.txt."""
import numpy as np
import pytest

from test_oracle_octree_wide import (CASE_DIMS, CASE_IDS, FORCE_TOL, SOFTENING, THETA0_TOL, THETAS, make_state, per_body, state_of,
                                     wide_of)

pytestmark = pytest.mark.gpu


def host_of(nb, s):
    hs = nb.HostSystem(s.dtype, s.dim, s.n)
    hs.m[:], hs.x[:], hs.v[:] = s.m, s.x, s.v
    hs.c, hs.dt = s.c, s.dt
    return hs


def check_walks(nb, s, w, theta, build=0, tag=""):
    """Every walk of one system against its wide walk `w`; prints the six force / potential figures and the three energy figures."""
    dtype, c = s.dtype, float(s.c)
    dev = nb.DeviceSystem.from_host(host_of(nb, s))
    t = dev.octree
    if build:
        t.set_build(build)
    t.enable_counters(True)
    fig = {}

    def counters(what):
        assert np.array_equal(t.read_counters(dev.stream), w.counts), (what, "counters")

    for what, kw, want, scale in (("a_mono", {}, w.a_mono, w.scale_a_mono),
                                  ("a_soft", {"softening": SOFTENING}, w.a_soft, w.scale_a_soft),
                                  ("a_quad", {"quadrupole": True}, w.a_quad, w.scale_a_quad)):
        dev.octree_force(theta, **kw)
        a = dev.download().a.copy()
        counters(what)
        assert np.isfinite(a).all(), what
        fig[what] = per_body(a, want, scale)
    for what, kw, want, scale in (("s_mono", {}, w.s_mono, w.scale_s_mono),
                                  ("s_soft", {"softening": SOFTENING}, w.s_soft, w.scale_s_soft),
                                  ("s_quad", {"quadrupole": True}, w.s_quad, w.scale_s_quad)):
        phi = dev.octree_potential(theta, **kw).astype(np.float64)
        counters(what)
        assert np.isfinite(phi).all(), what
        fig[what] = per_body(phi, -c * want, c * scale)
        _, pe = dev.octree_energies(theta, **kw)
        m = s.m.astype(np.longdouble)
        ref = -0.5 * c * float((m * want.astype(np.longdouble)).sum())
        fig["pe_" + what[2:]] = abs(float(pe) - ref) / (0.5 * c * float((np.abs(m) * scale.astype(np.longdouble)).sum()))
    t.info(dev.stream)  # raises if a build or a walk flagged anything
    dev.close()
    print(f"{tag} dtype {dtype} theta {theta}: " + " ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v <= (FORCE_TOL if k.startswith("a_") else THETA0_TOL)[dtype], (k, v)


@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("name, n, dim", CASE_DIMS, ids=CASE_IDS)
def test_walks_against_the_wide_walk(nb, oracle, name, n, dim, dtype, theta):
    """The monopole, softened (0.05) and quadrupole force, the three potentials and the three tree energies of every case of
    tests/test_oracle_octree_wide.py, default build form, counters equal to the wide walk's for each of the nine calls.
    measured on an MI355X, max over cases of the per-body figure: forces 1.7e-15 of scale in double and 1.1e-6 in float, potentials
    1.8e-15 and 7.8e-7, energies 3.9e-16 and 1.4e-7 (galaxy 20000 gives nearly all of them).  The deep system first gave a_quad
    2.99e-5 in float 2D at theta 1.0 (1.1e-5 in 3D, 4e-14 in double), over the bound: the quadrupole pass shifted Q child to parent as
    if the stored centres of mass were exact; since each cell carries its residual dipole (octree.hip) it gives 3.3e-7 and 8e-16."""
    check_walks(nb, state_of(name, n, dtype, dim), wide_of(name, n, dtype, dim, theta), theta, tag=f"{name} {n} {dim}D")


@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_walks_against_the_wide_walk_breadth_first_build(nb, oracle, dim, dtype, theta):
    """galaxy 4099 through build form 1 (one launch per level for the cells, the monopoles and the quadrupoles)."""
    check_walks(nb, state_of("galaxy", 4099, dtype, dim), wide_of("galaxy", 4099, dtype, dim, theta), theta, build=1,
                tag=f"galaxy 4099 {dim}D build 1")


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("dim", [3, 2])
def test_block_step_leaves_the_softened_force_of_the_predicted_positions(nb, oracle, dtype, dim):
    """tests/test_gpu_octree_block.py's smallest interesting case (n = 257, max_level = 0: every body active, one step of dt): the
    accelerations octree_block_start leaves against a_soft on the positions, and those one block step leaves against a_soft on the
    predicted positions it reports — that file pins them bitwise to the public softened force, this one pins that force's value."""
    from test_gpu_octree_block import random_system
    theta, eps, eta = 0.5, SOFTENING, 0.05
    hs = random_system(nb, dtype, dim, 257, seed=200 + 257, dt=0.125)
    dev = nb.DeviceSystem.from_host(hs)
    dev.octree_block_start(theta, eps, eta, 0)
    a0 = dev.download().a.copy()
    n_act, nxt = dev.octree_block_step(theta, eps, eta)
    assert (n_act, nxt) == (hs.n, 1)
    xp = dev.octree_block_predicted()
    a1 = dev.download().a.copy()
    dev.octree.info(dev.stream)
    dev.close()
    fig = []
    for x, a in ((hs.x, a0), (xp, a1)):
        w = oracle.octree_walk_wide(make_state(dtype, dim, x, hs.m, c=hs.c, dt=hs.dt), theta, eps)
        fig.append(per_body(a, w.a_soft, w.scale_a_soft))
    print(f"block step n 257 {dim}D dtype {dtype}: start {fig[0]:.3g} step {fig[1]:.3g}")
    assert max(fig) <= FORCE_TOL[dtype], fig
