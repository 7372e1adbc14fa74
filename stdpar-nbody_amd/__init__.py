"""Python host-side mirror of the reference's step-driver interface over the gfx950 backend.

This module is PLUMBING: it binds the C ABI of libnbody_hip.so (include/nbody_hip.h) with ctypes and
exposes the same phase calls the reference's drivers make (run_all_pairs, src/all_pairs.h:52-106;
run_bvh, src/bvh.h:327-418).  All arithmetic happens in the HIP kernels; there is NO CPU fallback —
if the shared library or a HIP device is missing every entry point raises.

The directory name contains a hyphen, so import it with the loader in `tests/conftest.py`,
`bench.py` or `__graft_entry__.py` (importlib by path, module name `stdpar_nbody_amd`).
"""
import ctypes as C
import os
import sys
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnbody_hip.so")
HOST_LIB_PATH = os.path.join(HERE, "libnbody_host.so")

F32, F64 = 0, 1
UNIFORM, PLUMMER, GALAXY = 0, 1, 2
WORKLOADS = {"uniform": UNIFORM, "plummer": PLUMMER, "galaxy": GALAXY}


class NbodyError(RuntimeError):
    pass


class nbody_state(C.Structure):
    """include/nbody_hip.h: device-pointer mirror of System<T,N>::state_t (src/system.h:41-50)."""
    _fields_ = [("m", C.c_void_p), ("x", C.c_void_p), ("v", C.c_void_p), ("a", C.c_void_p), ("ao", C.c_void_p),
                ("dt", C.c_double), ("c", C.c_double), ("sz", C.c_uint32), ("first", C.c_uint32), ("count", C.c_uint32),
                ("dtype", C.c_int32), ("dim", C.c_int32), ("tuning", C.c_uint32)]


def build(verbose=False):
    """Compile libnbody_hip.so (hipcc --offload-arch=gfx950), libnbody_host.so and the CLI, in-tree."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", HERE, "all"], stdout=out)


# every symbol include/nbody_hip.h declares (tests/test_abi.py checks the .so exports them all)
ABI_SYMBOLS = [
    "nbody_abi_version", "nbody_last_error", "nbody_device_info", "nbody_all_pairs_force", "nbody_all_pairs_collapsed_force",
    "nbody_accelerate_step", "nbody_calc_energies", "nbody_all_pairs_configure", "nbody_all_pairs_source_path", "nbody_bvh_create", "nbody_bvh_destroy",
    "nbody_bvh_bounding_box", "nbody_bvh_get_bounding_box", "nbody_bvh_hilbert_sort", "nbody_bvh_build_tree",
    "nbody_octree_create", "nbody_octree_destroy", "nbody_octree_clear", "nbody_octree_compute_bounds", "nbody_octree_insert",
    "nbody_octree_compute_tree", "nbody_octree_compute_force", "nbody_octree_info", "nbody_octree_enable_counters",
    "nbody_octree_read_counters", "nbody_bvh_compute_force", "nbody_bvh_read", "nbody_bvh_enable_counters", "nbody_bvh_set_traversal", "nbody_bvh_nnodes", "nbody_create",
    "nbody_bvh_create_on", "nbody_octree_create_on", "nbody_octree_set_walk", "nbody_octree_set_build", "nbody_octree_set_step_budget", "nbody_bvh_set_launch_order",
    "nbody_destroy", "nbody_upload", "nbody_download", "nbody_ctx_state", "nbody_ctx_stream", "nbody_stream_sync",
    "nbody_graph_begin", "nbody_graph_end", "nbody_graph_launch", "nbody_graph_destroy",
    "nbody_ctx_configure_all_pairs", "nbody_ctx_set_shard", "nbody_all_pairs_describe", "nbody_all_pairs_collapsed_describe",
    "nbody_comm_get_unique_id", "nbody_comm_create", "nbody_comm_create_all", "nbody_comm_destroy", "nbody_comm_world",
    "nbody_comm_rank", "nbody_comm_rccl_version", "nbody_shard_range", "nbody_comm_group_begin", "nbody_comm_group_end",
    "nbody_allgather_positions", "nbody_bvh_opening_thresholds", "nbody_all_pairs_pair_rule", "nbody_all_pairs_status",
    "nbody_all_pairs_softened_force", "nbody_calc_energies_softened", "nbody_octree_compute_softened_force",
    "nbody_octree_compute_quadrupoles", "nbody_octree_compute_quadrupole_force", "nbody_octree_read_root_quadrupole",
    "nbody_octree_compute_potential", "nbody_octree_compute_softened_potential", "nbody_octree_compute_quadrupole_potential",
    "nbody_octree_calc_energies",
    "nbody_hermite_create", "nbody_hermite_create_on", "nbody_hermite_destroy", "nbody_hermite_force_jerk", "nbody_hermite_step",
    "nbody_hermite_read",
    "nbody_hermite_block_start", "nbody_hermite_block_step", "nbody_hermite_block_advance", "nbody_hermite_block_read",
    "nbody_octree_block_create", "nbody_octree_block_create_on", "nbody_octree_block_destroy", "nbody_octree_block_start",
    "nbody_octree_block_step", "nbody_octree_block_advance", "nbody_octree_block_read",
    "nbody_hermite6_create", "nbody_hermite6_create_on", "nbody_hermite6_destroy", "nbody_hermite6_start", "nbody_hermite6_step",
    "nbody_hermite6_read",
    "nbody_hermite6_block_start", "nbody_hermite6_block_step", "nbody_hermite6_block_advance", "nbody_hermite6_block_read",
    "nbody_neighbours_create", "nbody_neighbours_create_on", "nbody_neighbours_destroy", "nbody_neighbours_compute",
    "nbody_neighbours_read", "nbody_neighbours_closest_pair",
    "nbody_knn_create", "nbody_knn_create_on", "nbody_knn_destroy", "nbody_knn_compute", "nbody_knn_read", "nbody_knn_density_centre",
    "nbody_knn_create_method", "nbody_knn_method",
    "nbody_fof_create", "nbody_fof_create_on", "nbody_fof_destroy", "nbody_fof_compute", "nbody_fof_read", "nbody_fof_summary",
    "nbody_nlist_create", "nbody_nlist_create_on", "nbody_nlist_destroy", "nbody_nlist_set_radii", "nbody_nlist_compute",
    "nbody_nlist_read", "nbody_nlist_summary",
]
ABI_MAJOR = 2
COMM_ID_BYTES = 128

_lib = None
_host = None


def lib():
    """Load libnbody_hip.so; raises NbodyError when it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NbodyError(f"{LIB_PATH} is missing: run `make -C stdpar-nbody_amd` (or __graft_entry__.build())")
        # One HIP runtime per process.  The PyTorch wheel bundles its own libamdhip64; if this library pulled in /opt/rocm's
        # first, a later `import torch` (sharded.py, bench.py) would bring a second runtime that finds no devices
        # ("No HIP GPUs are available").  Loaded in this order, both resolve to the copy torch brought.
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        L = C.CDLL(LIB_PATH)
        if L.nbody_abi_version() // 1000 != ABI_MAJOR:
            raise NbodyError(f"{LIB_PATH} has ABI version {L.nbody_abi_version()}, this binding needs major version {ABI_MAJOR}")
        L.nbody_last_error.restype = C.c_char_p
        L.nbody_ctx_stream.restype = C.c_void_p
        L.nbody_bvh_nnodes.restype = C.c_uint32
        L.nbody_shard_range.restype = None
        vp, d = C.c_void_p, C.c_double
        L.nbody_octree_compute_potential.argtypes = [vp, vp, d, vp, vp]
        L.nbody_octree_compute_softened_potential.argtypes = [vp, vp, d, d, vp, vp]
        L.nbody_octree_compute_quadrupole_potential.argtypes = [vp, vp, d, vp, vp]
        L.nbody_octree_calc_energies.argtypes = [vp, vp, d, d, C.c_int, vp, vp, vp]
        L.nbody_hermite_force_jerk.argtypes = [vp, vp, d, vp]
        L.nbody_hermite_step.argtypes = [vp, vp, d, vp]
        L.nbody_hermite_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.nbody_hermite_block_start.argtypes = [vp, vp, d, d, C.c_int, vp]
        L.nbody_hermite_block_step.argtypes = [vp, vp, d, d, vp, vp, vp]
        L.nbody_hermite_block_advance.argtypes = [vp, vp, d, d, vp, vp, vp]
        L.nbody_hermite_block_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.nbody_hermite6_destroy.restype = None
        L.nbody_hermite6_destroy.argtypes = [vp]
        L.nbody_hermite6_start.argtypes = [vp, vp, d, vp]
        L.nbody_hermite6_step.argtypes = [vp, vp, d, vp]
        L.nbody_hermite6_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.nbody_hermite6_block_start.argtypes = [vp, vp, d, d, C.c_int, vp]
        L.nbody_hermite6_block_step.argtypes = [vp, vp, d, d, vp, vp, vp]
        L.nbody_hermite6_block_advance.argtypes = [vp, vp, d, d, vp, vp, vp]
        L.nbody_hermite6_block_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.nbody_octree_block_destroy.restype = None
        L.nbody_octree_block_destroy.argtypes = [vp]
        L.nbody_octree_block_start.argtypes = [vp, vp, vp, d, d, d, C.c_int, vp]
        L.nbody_octree_block_step.argtypes = [vp, vp, vp, d, d, d, vp, vp, vp]
        L.nbody_octree_block_advance.argtypes = [vp, vp, vp, d, d, d, vp, vp, vp]
        L.nbody_octree_block_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.nbody_neighbours_create.argtypes = [vp, C.c_int, C.c_int, C.c_uint32]
        L.nbody_neighbours_create_on.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int]
        L.nbody_neighbours_destroy.restype = None
        L.nbody_neighbours_destroy.argtypes = [vp]
        L.nbody_neighbours_compute.argtypes = [vp, vp, d, vp]
        L.nbody_neighbours_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.nbody_neighbours_closest_pair.argtypes = [vp, vp, vp, vp, vp]
        L.nbody_knn_create.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int]
        L.nbody_knn_create_on.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int]
        L.nbody_knn_create_method.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_int]
        L.nbody_knn_method.argtypes = [vp]
        L.nbody_knn_destroy.restype = None
        L.nbody_knn_destroy.argtypes = [vp]
        L.nbody_knn_compute.argtypes = [vp, vp, vp]
        L.nbody_knn_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.nbody_knn_density_centre.argtypes = [vp, vp, vp, vp, vp]
        L.nbody_fof_create.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32]
        L.nbody_fof_create_on.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_int]
        L.nbody_fof_destroy.restype = None
        L.nbody_fof_destroy.argtypes = [vp]
        L.nbody_fof_compute.argtypes = [vp, vp, d, vp]
        L.nbody_fof_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.nbody_fof_summary.argtypes = [vp, vp, vp]
        L.nbody_nlist_create.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint64]
        L.nbody_nlist_create_on.argtypes = [vp, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.c_int]
        L.nbody_nlist_destroy.restype = None
        L.nbody_nlist_destroy.argtypes = [vp]
        L.nbody_nlist_set_radii.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
        L.nbody_nlist_compute.argtypes = [vp, vp, d, vp]
        L.nbody_nlist_read.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.nbody_nlist_summary.argtypes = [vp, vp, vp]
        _lib = L
    return _lib


def host_lib():
    """libnbody_host.so: the product's ISO-C++ workload generators (host/models.hpp) behind a C entry."""
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise NbodyError(f"{HOST_LIB_PATH} is missing: run `make -C stdpar-nbody_amd host`")
        H = C.CDLL(HOST_LIB_PATH)
        H.nbody_host_build_model.restype = C.c_int64
        _host = H
    return _host


def _check(rc):
    if rc != 0:
        raise NbodyError(f"nbody backend error {rc}: {lib().nbody_last_error().decode()}")


def np_dtype(dtype):
    return np.float32 if dtype == F32 else np.float64


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def bvh_opening_thresholds(dtype, width2, theta):
    """The opening thresholds nbody_bvh_build_tree stores (nbody_bvh_read what = 6) for given width^2 values, computed on the
    host by the same function (no device needed)."""
    w2 = np.ascontiguousarray(width2, np_dtype(dtype))
    out = np.empty_like(w2)
    _check(lib().nbody_bvh_opening_thresholds(dtype, _p(w2), C.c_double(theta), C.c_size_t(w2.size), _p(out)))
    return out


def device_info(device=0):
    arch = C.create_string_buffer(128)
    cus = C.c_int()
    _check(lib().nbody_device_info(device, arch, C.c_size_t(128), C.byref(cus)))
    return arch.value.decode(), cus.value


def configure_all_pairs(split=0, targets_per_thread=0, source_path=None):
    """K1 knobs (include/nbody_hip.h): source split, targets per lane, and — when given — how a source record reaches
    the lanes (0 auto, 1 LDS tiles, 2 scalar stream)."""
    _check(lib().nbody_all_pairs_configure(split, targets_per_thread))
    if source_path is not None:
        _check(lib().nbody_all_pairs_source_path(int(source_path)))


def tuning(split=0, targets_per_thread=0, source_path=0):
    """NBODY_TUNING(split, targets_per_thread, source_path) of include/nbody_hip.h; 0 = the library default."""
    if not (split or targets_per_thread or source_path):
        return 0
    return (split & 15) | ((targets_per_thread & 3) << 4) | ((source_path & 3) << 6) | 0x100


def describe_all_pairs(st):
    """The K1 launch the library will make for this view (kernel template arguments, tile, chunks, pair math)."""
    buf = C.create_string_buffer(256)
    _check(lib().nbody_all_pairs_describe(C.byref(st), buf, C.c_size_t(256)))
    return buf.value.decode()


def describe_all_pairs_collapsed(st):
    """The K2 launch the library will make for this state (kernel, and padded / nbatches / bpc / chunks of the streamed form or
    iblocks / ntiles / tpb / ysplit of the tile form).  Host arithmetic only: no GPU needed."""
    buf = C.create_string_buffer(256)
    _check(lib().nbody_all_pairs_collapsed_describe(C.byref(st), buf, C.c_size_t(256)))
    return buf.value.decode()


def all_pairs_pair_rule(st, stream=None):
    """(sparse, volume): the per-pair rounding form K1 takes for this state (nbody_all_pairs_pair_rule)."""
    sparse, vol = C.c_int(), C.c_double()
    _check(lib().nbody_all_pairs_pair_rule(C.byref(st), C.c_void_p(stream), C.byref(sparse), C.byref(vol)))
    return bool(sparse.value), vol.value


def all_pairs_status(stream=None, clear=False, check=True):
    """K1's chunk hand-off status of a stream (nbody_all_pairs_status; waits for the stream): a dict with `failed`, the
    (block, group, chunk) of the first failure, and `polls` / `waits` — how often waves had to wait for their turn.  Raises
    NbodyError while a failure is recorded, unless check is False."""
    out = (C.c_uint64 * 6)()
    rc = lib().nbody_all_pairs_status(C.c_void_p(stream), out, 1 if clear else 0)
    if check:
        _check(rc)
    return {"failed": bool(out[0]), "block": int(out[1]), "group": int(out[2]), "chunk": int(out[3]), "polls": int(out[4]),
            "waits": int(out[5]), "rc": rc}


def shard_range(n, rank, world):
    """nbody_shard_range: rank r of W owns bodies [n*r//W, n*(r+1)//W) — the partition the collective assumes."""
    f, c = C.c_uint32(), C.c_uint32()
    lib().nbody_shard_range(C.c_uint32(n), world, rank, C.byref(f), C.byref(c))
    return f.value, f.value + c.value


class _Handle:
    """An opaque handle of the library: self.h, closed by the symbol the class names in _destroy."""

    _destroy = None

    def close(self):
        if self.h:
            getattr(lib(), self._destroy)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm(_Handle):
    """nbody_comm: the RCCL communicator of the per-step all-gather of positions (one process per GPU form)."""

    _destroy = "nbody_comm_destroy"

    def __init__(self, world, rank, unique_id, device):
        self.h = C.c_void_p()
        assert len(unique_id) == COMM_ID_BYTES
        _check(lib().nbody_comm_create(C.byref(self.h), world, rank, C.c_char_p(bytes(unique_id)), device))
        self.world, self.rank = world, rank

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check(lib().nbody_comm_get_unique_id(buf))
        return buf.raw

    @staticmethod
    def rccl_version():
        return int(lib().nbody_comm_rccl_version())

    def allgather_positions(self, st, stream=None):
        _check(lib().nbody_allgather_positions(self.h, C.byref(st), C.c_void_p(stream)))


class HostSystem:
    """Host arrays of the reference's System<T,N> (src/system.h:13-19)."""

    def __init__(self, dtype, dim, n):
        t = np_dtype(dtype)
        self.dtype, self.dim, self.n = dtype, dim, n
        self.m = np.zeros(n, t)
        self.x = np.zeros((n, dim), t)
        self.v = np.zeros((n, dim), t)
        self.a = np.zeros((n, dim), t)
        self.ao = np.zeros((n, dim), t)
        self.dt = 0.0
        self.c = 0.0


def build_model(dtype, dim, workload, n):
    """Product workload generators (host/models.hpp, mirrors src/models.h). Returns a HostSystem."""
    wl = WORKLOADS[workload] if isinstance(workload, str) else workload
    s = HostSystem(dtype, dim, n)
    dt, c = C.c_double(), C.c_double()
    sz = host_lib().nbody_host_build_model(dtype, dim, wl, C.c_uint32(n), _p(s.m), _p(s.x), _p(s.v), C.byref(dt), C.byref(c))
    if sz < 0:
        raise NbodyError(f"nbody_host_build_model failed ({sz})")
    if sz != n:
        t = HostSystem(dtype, dim, int(sz))
        t.m[:], t.x[:], t.v[:] = s.m[:sz], s.x[:sz], s.v[:sz]
        s = t
    s.dt, s.c = dt.value, c.value
    return s


class Bvh(_Handle):
    """bvh<T,N> (src/bvh.h:98-325) on the device."""

    _destroy = "nbody_bvh_destroy"

    def __init__(self, dtype, dim, n, device=-1):
        """device: where the tree's buffers live (-1: the calling thread's current device)."""
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n = dtype, dim, n
        _check(lib().nbody_bvh_create_on(C.byref(self.h), dtype, dim, C.c_uint32(n), device))
        self.nnodes = int(lib().nbody_bvh_nnodes(self.h))

    def bounding_box(self, st, stream=None):
        _check(lib().nbody_bvh_bounding_box(self.h, C.byref(st), C.c_void_p(stream)))

    def get_bounding_box(self, stream=None):
        t = np_dtype(self.dtype)
        lo, hi = np.zeros(self.dim, t), np.zeros(self.dim, t)
        _check(lib().nbody_bvh_get_bounding_box(self.h, _p(lo), _p(hi), C.c_void_p(stream)))
        return lo, hi

    def hilbert_sort(self, st, stream=None):
        _check(lib().nbody_bvh_hilbert_sort(self.h, C.byref(st), C.c_void_p(stream)))

    def build_tree(self, st, stream=None):
        _check(lib().nbody_bvh_build_tree(self.h, C.byref(st), C.c_void_p(stream)))

    def compute_force(self, st, theta, stream=None):
        _check(lib().nbody_bvh_compute_force(self.h, C.byref(st), C.c_double(theta), C.c_void_p(stream)))

    def set_traversal(self, mode):
        """0 auto, 1 per-lane walks, 2 wave-cooperative sweep (bitwise identical results)."""
        _check(lib().nbody_bvh_set_traversal(self.h, mode))

    def set_launch_order(self, mode):
        """Sweep: 0 work items (cut groups first), 1 one block per group in index order (bitwise identical results)."""
        _check(lib().nbody_bvh_set_launch_order(self.h, mode))

    def enable_counters(self, on=True):
        _check(lib().nbody_bvh_enable_counters(self.h, 1 if on else 0))

    def read(self, what, stream=None):
        t = np_dtype(self.dtype)
        shapes = {0: ((self.n,), np.uint64), 1: ((self.n,), np.uint32), 2: ((self.nnodes, self.dim + 1), t),
                  3: ((self.nnodes,), t), 4: ((self.nnodes, 2 * self.dim), t), 5: ((self.n, 4), np.uint32),
                  6: ((self.nnodes,), t)}
        shape, dt = shapes[what]
        out = np.zeros(shape, dt)
        _check(lib().nbody_bvh_read(self.h, what, _p(out), C.c_size_t(out.nbytes), C.c_void_p(stream)))
        return out


class Octree(_Handle):
    """octree<T,N> (src/octree.h) on the device."""

    _destroy = "nbody_octree_destroy"

    def __init__(self, dtype, dim, n, device=-1):
        """device: where the tree's buffers live (-1: the calling thread's current device)."""
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n = dtype, dim, n
        _check(lib().nbody_octree_create_on(C.byref(self.h), dtype, dim, C.c_uint32(n), device))

    def set_build(self, mode):
        """0 auto (= 3), 1 one launch per tree level, 2 all levels behind a grid barrier, 3 one pass over the sorted keys, 4 per-level
        for the levels of the last info + one launch for the rest.  Same cells, monopoles, forces and counters bit for bit."""
        _check(lib().nbody_octree_set_build(self.h, mode))

    def set_step_budget(self, steps):
        """Visit rounds a body's walk may make before it is abandoned and info() raises (0 = the node pool size)."""
        _check(lib().nbody_octree_set_step_budget(self.h, C.c_uint32(steps)))

    def set_walk(self, mode):
        """0 auto, 1 the compiler-scheduled walk kernel, 2 the visit round as ISA (bitwise identical results)."""
        _check(lib().nbody_octree_set_walk(self.h, mode))

    def clear(self, stream=None):
        _check(lib().nbody_octree_clear(self.h, C.c_void_p(stream)))

    def compute_bounds(self, st, stream=None):
        _check(lib().nbody_octree_compute_bounds(self.h, C.byref(st), C.c_void_p(stream)))

    def insert(self, st, stream=None):
        _check(lib().nbody_octree_insert(self.h, C.byref(st), C.c_void_p(stream)))

    def compute_tree(self, stream=None):
        _check(lib().nbody_octree_compute_tree(self.h, C.c_void_p(stream)))

    def compute_force(self, st, theta, stream=None):
        _check(lib().nbody_octree_compute_force(self.h, C.byref(st), C.c_double(theta), C.c_void_p(stream)))

    def compute_softened_force(self, st, theta, eps, stream=None):
        """compute_force with Plummer softening eps > 0 (nbody_octree_compute_softened_force): the same opening decisions, the
        accepted term m d / (|d|^2 + eps^2)^(3/2); the compiler-scheduled walk (refused after set_walk(2))."""
        _check(lib().nbody_octree_compute_softened_force(self.h, C.byref(st), C.c_double(theta), C.c_double(eps), C.c_void_p(stream)))

    def compute_quadrupoles(self, stream=None):
        """Quadrupole moments of every cell (nbody_octree_compute_quadrupoles); after compute_tree."""
        _check(lib().nbody_octree_compute_quadrupoles(self.h, C.c_void_p(stream)))

    def compute_quadrupole_force(self, st, theta, stream=None):
        """compute_force with the quadrupole term of every accepted cell (nbody_octree_compute_quadrupole_force)."""
        _check(lib().nbody_octree_compute_quadrupole_force(self.h, C.byref(st), C.c_double(theta), C.c_void_p(stream)))

    def read_root_quadrupole(self, stream=None):
        """The root's quadrupole: xx, xy, xz, yy, yz, zz in 3D, xx, xy, yy in 2D (blocking)."""
        out = np.zeros(6 if self.dim == 3 else 3, dtype=np_dtype(self.dtype))
        _check(lib().nbody_octree_read_root_quadrupole(self.h, _p(out), C.c_void_p(stream)))
        return out

    def compute_potential(self, st, theta, phi, stream=None):
        """phi[k] = -c S of body st.first + k (nbody_octree_compute_potential): the force walk's tests, the accepted term
        m / (|d| + eps(T)), the body's own leaf left out.  phi: a device pointer (int) to count values of T, e.g. a torch tensor's
        data_ptr(); nothing is allocated, so this may be recorded."""
        _check(lib().nbody_octree_compute_potential(self.h, C.byref(st), theta, phi, stream))

    def compute_softened_potential(self, st, theta, eps, phi, stream=None):
        """compute_potential with the softened term m / sqrt(|d|^2 + eps^2) (nbody_octree_compute_softened_potential)."""
        _check(lib().nbody_octree_compute_softened_potential(self.h, C.byref(st), theta, eps, phi, stream))

    def compute_quadrupole_potential(self, st, theta, phi, stream=None):
        """compute_potential whose accepted cells also add 1/2 (d^T Q d) / |d|^5 (after compute_quadrupoles)."""
        _check(lib().nbody_octree_compute_quadrupole_potential(self.h, C.byref(st), theta, phi, stream))

    def calc_energies(self, st, theta, eps=0.0, quadrupole=False, stream=None):
        """(kinetic, potential) with the potential from the tree (nbody_octree_calc_energies; blocking, whole system, on a built
        tree): -c/2 sum_i m_i S_i.  eps > 0 softened, quadrupole=True the quadrupole term (after compute_quadrupoles)."""
        t = np_dtype(self.dtype)
        ke, pe = np.zeros(1, t), np.zeros(1, t)
        _check(lib().nbody_octree_calc_energies(self.h, C.byref(st), theta, eps, 1 if quadrupole else 0, _p(ke), _p(pe), stream))
        return ke[0], pe[0]

    def info(self, stream=None):
        """(tree size = next_free_child_group, root mass); raises if the build hit the depth limit / node pool."""
        size = C.c_uint32()
        mass = np.zeros(1, np_dtype(self.dtype))
        _check(lib().nbody_octree_info(self.h, C.byref(size), _p(mass), C.c_void_p(stream)))
        return size.value, mass[0]

    def enable_counters(self, on=True):
        _check(lib().nbody_octree_enable_counters(self.h, 1 if on else 0))

    def read_counters(self, stream=None):
        out = np.zeros((self.n, 2), np.uint32)
        _check(lib().nbody_octree_read_counters(self.h, _p(out), C.c_size_t(out.nbytes), C.c_void_p(stream)))
        return out


class Hermite(_Handle):
    """Fourth-order Hermite integrator for all-pairs (nbody_hermite_*): owns the jerk, the packed predicted state and the partial sums."""

    _destroy = "nbody_hermite_destroy"

    def __init__(self, dtype, dim, n, device=-1):
        """device: where the handle's buffers live (-1: the calling thread's current device)."""
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n = dtype, dim, n
        _check(lib().nbody_hermite_create_on(C.byref(self.h), dtype, dim, C.c_uint32(n), device))

    def force_jerk(self, st, eps, stream=None):
        """a = st.a and the handle's jerk at (st.x, st.v), Plummer softening eps > 0: starts (or restarts) a run."""
        _check(lib().nbody_hermite_force_jerk(self.h, C.byref(st), eps, stream))

    def step(self, st, eps, stream=None):
        """One predictor-corrector step of st.dt: rewrites st.x, st.v, st.a and the jerk; st.ao is untouched.  Recordable."""
        _check(lib().nbody_hermite_step(self.h, C.byref(st), eps, stream))

    def read(self, what, stream=None):
        """0 the jerk, 1 the predicted positions, 2 the predicted velocities of the last step: (n, dim) of T (blocking)."""
        out = np.zeros((self.n, self.dim), np_dtype(self.dtype))
        _check(lib().nbody_hermite_read(self.h, what, _p(out), out.nbytes, stream))
        return out

    # block (individual) time steps
    def block_start(self, st, eps, eta_start, max_level, stream=None):
        """a, the jerk and the first levels (nbody_hermite_block_start): st.dt is the largest step, st.dt / 2^max_level the smallest."""
        _check(lib().nbody_hermite_block_start(self.h, C.byref(st), eps, eta_start, max_level, stream))

    def block_step(self, st, eps, eta, stream=None):
        """One block step: (n_active, tau_next in ticks).  Blocking for the schedule."""
        na, tau = C.c_uint32(), C.c_uint32()
        _check(lib().nbody_hermite_block_step(self.h, C.byref(st), eps, eta, stream, C.byref(na), C.byref(tau)))
        return na.value, tau.value

    def block_advance(self, st, eps, eta, stream=None):
        """Block steps until the system is synchronous at t + st.dt: (block steps, body steps)."""
        bs, bod = C.c_uint64(), C.c_uint64()
        _check(lib().nbody_hermite_block_advance(self.h, C.byref(st), eps, eta, stream, C.byref(bs), C.byref(bod)))
        return bs.value, bod.value

    def block_read(self, what, stream=None, count=None):
        """0 the levels (int32), 1 tau_i in ticks (uint32), 2 the active list of the last block step (uint32, `count` of them)."""
        out = np.zeros(self.n if what != 2 else count, np.int32 if what == 0 else np.uint32)
        _check(lib().nbody_hermite_block_read(self.h, what, _p(out), out.nbytes, stream))
        return out


class Hermite6(_Handle):
    """Sixth-order Hermite integrator for all-pairs (nbody_hermite6_*): owns the jerk, the snap, the crackle, the packed predicted
    state and the partial sums."""

    _destroy = "nbody_hermite6_destroy"

    def __init__(self, dtype, dim, n, device=-1):
        """device: where the handle's buffers live (-1: the calling thread's current device)."""
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n = dtype, dim, n
        _check(lib().nbody_hermite6_create_on(C.byref(self.h), dtype, dim, C.c_uint32(n), device))

    def start(self, st, eps, stream=None):
        """a = st.a, the jerk and the snap at (st.x, st.v), crackle = 0, Plummer softening eps > 0: starts (or restarts) a run."""
        _check(lib().nbody_hermite6_start(self.h, C.byref(st), eps, stream))

    def step(self, st, eps, stream=None):
        """One predictor-corrector step of st.dt: rewrites st.x, st.v, st.a, the jerk, the snap and the crackle; st.ao is untouched.
        Recordable."""
        _check(lib().nbody_hermite6_step(self.h, C.byref(st), eps, stream))

    def read(self, what, stream=None):
        """0 the jerk, 1 the snap, 2 the crackle, 3 / 4 / 5 the predicted positions / velocities / accelerations of the last step:
        (n, dim) of T (blocking)."""
        out = np.zeros((self.n, self.dim), np_dtype(self.dtype))
        _check(lib().nbody_hermite6_read(self.h, what, _p(out), out.nbytes, stream))
        return out

    # block (individual) time steps: double only
    def block_start(self, st, eps, eta_start, max_level, stream=None):
        """a, the jerk, the snap, crackle = 0 and the first levels (nbody_hermite6_block_start): st.dt is the largest step,
        st.dt / 2^max_level the smallest.  A float handle is refused."""
        _check(lib().nbody_hermite6_block_start(self.h, C.byref(st), eps, eta_start, max_level, stream))

    def block_step(self, st, eps, eta, stream=None):
        """One block step: (n_active, tau_next in ticks).  Blocking for the schedule."""
        na, tau = C.c_uint32(), C.c_uint32()
        _check(lib().nbody_hermite6_block_step(self.h, C.byref(st), eps, eta, stream, C.byref(na), C.byref(tau)))
        return na.value, tau.value

    def block_advance(self, st, eps, eta, stream=None):
        """Block steps until the system is synchronous at t + st.dt: (block steps, body steps)."""
        bs, bod = C.c_uint64(), C.c_uint64()
        _check(lib().nbody_hermite6_block_advance(self.h, C.byref(st), eps, eta, stream, C.byref(bs), C.byref(bod)))
        return bs.value, bod.value

    def block_read(self, what, stream=None, count=None):
        """0 the levels (int32), 1 tau_i in ticks (uint32), 2 the active list of the last block step (uint32, `count` of them)."""
        out = np.zeros(self.n if what != 2 else count, np.int32 if what == 0 else np.uint32)
        _check(lib().nbody_hermite6_block_read(self.h, what, _p(out), out.nbytes, stream))
        return out


class Neighbours(_Handle):
    """All-pairs per-body potentials, nearest neighbours and the closest pair (nbody_neighbours_*): owns the packed records, the
    chunks' partial arrays and the results."""

    _destroy = "nbody_neighbours_destroy"

    def __init__(self, dtype, dim, n, device=-1):
        """device: where the handle's buffers live (-1: the calling thread's current device)."""
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n = dtype, dim, n
        _check(lib().nbody_neighbours_create_on(C.byref(self.h), dtype, dim, C.c_uint32(n), device))

    def compute(self, st, eps, stream=None):
        """phi, nn, nnd2 and the closest pair at (st.m, st.x), Plummer softening eps > 0, into the handle.  Asynchronous, recordable."""
        _check(lib().nbody_neighbours_compute(self.h, C.byref(st), eps, stream))

    def read(self, what, stream=None):
        """0 phi (n,) of T, 1 nn (n,) uint32, 2 nnd2 (n,) of T of the last compute (blocking)."""
        out = np.zeros(self.n, np.uint32 if what == 1 else np_dtype(self.dtype))
        _check(lib().nbody_neighbours_read(self.h, what, _p(out), out.nbytes, stream))
        return out

    def closest_pair(self, stream=None):
        """(i, j, d2) of the last compute: i < j, d2 of T (blocking)."""
        i, j = C.c_uint32(), C.c_uint32()
        d2 = np.zeros(1, np_dtype(self.dtype))
        _check(lib().nbody_neighbours_closest_pair(self.h, C.byref(i), C.byref(j), _p(d2), stream))
        return i.value, j.value, d2[0]


class Knn(_Handle):
    """k nearest neighbours, local densities and the density centre (nbody_knn_*): owns the packed records, the method's work
    arrays and the results.  k is fixed here, 1 <= k <= 16.  method: "all-pairs" (every pair, O(n^2)) or "tree" (exact, pruned with
    bounding boxes over a space-sorted copy, for large n): the same outputs bit for bit."""

    _destroy = "nbody_knn_destroy"

    METHODS = {"all-pairs": 0, "tree": 1}

    def __init__(self, dtype, dim, n, k, device=-1, method="all-pairs"):
        """device: where the handle's buffers live (-1: the calling thread's current device)."""
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n, self.k = dtype, dim, n, k
        if method not in self.METHODS:
            raise ValueError(f"Knn method must be one of {sorted(self.METHODS)}, got {method!r}")
        _check(lib().nbody_knn_create_method(C.byref(self.h), dtype, dim, C.c_uint32(n), k, self.METHODS[method], device))

    @property
    def method(self):
        """The method the handle was made for: "all-pairs" or "tree" (nbody_knn_method)."""
        m = lib().nbody_knn_method(self.h)
        for name, v in self.METHODS.items():
            if v == m:
                return name
        raise RuntimeError(lib().nbody_last_error().decode())

    def compute(self, st, stream=None):
        """idx, d2, rho and the summary at (st.m, st.x), into the handle.  Asynchronous, recordable."""
        _check(lib().nbody_knn_compute(self.h, C.byref(st), stream))

    def read(self, what, stream=None):
        """0 idx (n, k) uint32, 1 d2 (n, k) of T, 2 rho (n,) of T of the last compute (blocking)."""
        t = np_dtype(self.dtype)
        out = np.zeros(self.n, t) if what == 2 else np.zeros((self.n, self.k), np.uint32 if what == 0 else t)
        _check(lib().nbody_knn_read(self.h, what, _p(out), out.nbytes, stream))
        return out

    def density_centre(self, stream=None):
        """(x_dc (dim,), r_c, rho_c) of the last compute, of T (blocking).  NaN where sum rho is 0 or a rho is not finite."""
        t = np_dtype(self.dtype)
        x, rc, rhoc = np.zeros(self.dim, t), np.zeros(1, t), np.zeros(1, t)
        _check(lib().nbody_knn_density_centre(self.h, _p(x), _p(rc), _p(rhoc), stream))
        return x, rc[0], rhoc[0]


class Fof(_Handle):
    """Friends-of-friends groups (nbody_fof_*): bodies no farther apart than a linking length b are friends, a group is a connected
    component.  Exact, on the tree of the kNN "tree" method.  min_members (fixed here, 1 .. n) is the smallest group the catalogue
    lists; label and size cover every body whatever it is."""

    _destroy = "nbody_fof_destroy"

    def __init__(self, dtype, dim, n, min_members=1, device=-1):
        """device: where the handle's buffers live (-1: the calling thread's current device)."""
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n, self.min_members = dtype, dim, n, min_members
        _check(lib().nbody_fof_create_on(C.byref(self.h), dtype, dim, C.c_uint32(n), C.c_uint32(min_members), device))

    def compute(self, st, b, stream=None):
        """label, size, the summary and the catalogue at (st.m, st.x) for the linking length b >= 0, into the handle.  Asynchronous,
        recordable."""
        _check(lib().nbody_fof_compute(self.h, C.byref(st), C.c_double(b), stream))

    def summary(self, stream=None):
        """(groups, catalogued groups, largest size, label of the largest group) of the last compute, uint32 (4,) (blocking)."""
        out = np.zeros(4, np.uint32)
        _check(lib().nbody_fof_summary(self.h, _p(out), stream))
        return out

    def read(self, what, stream=None):
        """0 label (n,) uint32, 1 size (n,) uint32; the catalogue's 2 label (c,) uint32, 3 size (c,) uint32, 4 mass (c,) of T,
        5 com (c, dim) of T of the last compute (blocking)."""
        t = np_dtype(self.dtype)
        if what <= 1:
            out = np.zeros(self.n, np.uint32)
        else:
            c = int(self.summary(stream)[1])
            out = np.zeros((c, self.dim), t) if what == 5 else np.zeros(c, np.uint32 if what <= 3 else t)
        _check(lib().nbody_fof_read(self.h, what, _p(out) if out.size else None, out.nbytes, stream))
        return out

    def catalogue(self, stream=None):
        """{"label", "size", "mass", "com"}: the groups of at least min_members bodies, in ascending label order (blocking)."""
        return {name: self.read(what, stream) for what, name in ((2, "label"), (3, "size"), (4, "mass"), (5, "com"))}


class NeighbourLists(_Handle):
    """Exact fixed-radius neighbour lists (nbody_nlist_*): every j != i with d2_ij <= r2_i, as count (n,), offset (n + 1,) and a list
    in ascending index per body.  On the tree of the kNN "tree" method.  capacity (fixed here, 0 .. 2^32) is the number of list
    entries the handle can hold; 0 makes a counts-only handle."""

    _destroy = "nbody_nlist_destroy"

    MAX_PER_BODY = 4096
    OVER_CAPACITY, OVER_PER_BODY = 1, 2  # the summary's status bits: no list was produced by that compute

    def __init__(self, dtype, dim, n, capacity, device=-1):
        """device: where the handle's buffers live (-1: the calling thread's current device)."""
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n, self.capacity = dtype, dim, n, int(capacity)
        _check(lib().nbody_nlist_create_on(C.byref(self.h), dtype, dim, C.c_uint32(n), C.c_uint64(self.capacity), device))

    def set_radii(self, values, squared=False, stream=None):
        """Per-body radii (n,), or squared radii with squared=True, for every later compute: r2_i = v_i * v_i (or v_i), each >= 0 and
        finite (blocking)."""
        v = np.ascontiguousarray(values, np_dtype(self.dtype))
        _check(lib().nbody_nlist_set_radii(self.h, _p(v), v.nbytes, 1 if squared else 0, stream))

    def clear_radii(self, stream=None):
        """Back to the scalar radius of compute."""
        _check(lib().nbody_nlist_set_radii(self.h, None, 0, 0, stream))

    def compute(self, st, r=0.0, stream=None):
        """count, offset, the summary and (if it fits) the list at (st.m, st.x) for the radius r >= 0 (ignored once radii are set),
        into the handle.  Asynchronous, recordable."""
        _check(lib().nbody_nlist_compute(self.h, C.byref(st), C.c_double(r), stream))

    def summary(self, stream=None):
        """(total, largest count, lowest index that has it, status) of the last compute, uint64 (4,) (blocking)."""
        out = np.zeros(4, np.uint64)
        _check(lib().nbody_nlist_summary(self.h, _p(out), stream))
        return out

    def read(self, what, stream=None):
        """0 count (n,) uint32, 1 offset (n + 1,) uint64, 2 list (total,) uint32 of the last compute (blocking).  The list of a compute
        whose status is not 0 does not exist: NbodyError."""
        if what == 0:
            out = np.zeros(self.n, np.uint32)
        elif what == 1:
            out = np.zeros(self.n + 1, np.uint64)
        else:
            total, _, _, status = self.summary(stream)
            out = np.zeros(int(total) if status == 0 else 0, np.uint32)  # no list: the call below says which limit was hit
        _check(lib().nbody_nlist_read(self.h, what, _p(out) if out.size else None, out.nbytes, stream))
        return out

    def lists(self, stream=None):
        """(count, offset, idx) of the last compute (blocking)."""
        return self.read(0, stream), self.read(1, stream), self.read(2, stream)


class OctreeBlock(_Handle):
    """Block (individual) time steps for the octree leapfrog (nbody_octree_block_*): owns the levels, tau, the active lists, the
    predicted positions and the scratch of the active set's forces; the tree is the caller's Octree."""

    _destroy = "nbody_octree_block_destroy"

    def __init__(self, dtype, dim, n, device=-1):
        """device: where the handle's buffers live (-1: the calling thread's current device)."""
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n = dtype, dim, n
        _check(lib().nbody_octree_block_create_on(C.byref(self.h), dtype, dim, C.c_uint32(n), device))

    def start(self, tree, st, theta, eps, eta, max_level, stream=None):
        """The softened force of all bodies into st.a and the first levels: st.dt is the largest step, st.dt / 2^max_level the smallest."""
        _check(lib().nbody_octree_block_start(self.h, tree.h, C.byref(st), theta, eps, eta, max_level, stream))

    def step(self, tree, st, theta, eps, eta, stream=None):
        """One block step: (n_active, tau_next in ticks).  Blocking for the schedule."""
        na, tau = C.c_uint32(), C.c_uint32()
        _check(lib().nbody_octree_block_step(self.h, tree.h, C.byref(st), theta, eps, eta, stream, C.byref(na), C.byref(tau)))
        return na.value, tau.value

    def advance(self, tree, st, theta, eps, eta, stream=None):
        """Block steps until the system is synchronous at t + st.dt: (block steps, body steps)."""
        bs, bod = C.c_uint64(), C.c_uint64()
        _check(lib().nbody_octree_block_advance(self.h, tree.h, C.byref(st), theta, eps, eta, stream, C.byref(bs), C.byref(bod)))
        return bs.value, bod.value

    def read(self, what, stream=None, count=None):
        """0 the levels (int32), 1 tau_i in ticks (uint32), 2 the active list of the last block step (uint32, `count` of them,
        ascending), 3 its predicted positions, (n, dim) of T."""
        if what == 3:
            out = np.zeros((self.n, self.dim), np_dtype(self.dtype))
        else:
            out = np.zeros(self.n if what != 2 else count, np.int32 if what == 0 else np.uint32)
        _check(lib().nbody_octree_block_read(self.h, what, _p(out), out.nbytes, stream))
        return out


class DeviceSystem(_Handle):
    """Owning device mirror of a System<T,N>; phase methods mirror the calls of the reference drivers."""

    _destroy = "nbody_destroy"
    _CACHED = ("_bvh", "_octree", "_hermite", "_octree_block", "_hermite6", "_neighbours")  # one handle each, made on first use

    def __init__(self, dtype, dim, n, device=0):
        self.h = C.c_void_p()
        self.dtype, self.dim, self.n, self.device = dtype, dim, n, device
        _check(lib().nbody_create(C.byref(self.h), dtype, dim, C.c_uint32(n), device))
        self.stream = lib().nbody_ctx_stream(self.h)
        for a in self._CACHED:
            setattr(self, a, None)
        self._knn = {}
        self._knn_other = {}
        self._fof = {}
        self._nlist = {}

    @classmethod
    def from_host(cls, hs, device=0):
        d = cls(hs.dtype, hs.dim, hs.n, device)
        d.upload(hs)
        return d

    def close(self):
        cached = [getattr(self, a) for a in self._CACHED] + list(self._knn.values()) + list(self._knn_other.values())
        cached += list(self._fof.values()) + list(self._nlist.values())
        for h in cached:
            if h is not None:
                h.close()
        for a in self._CACHED:
            setattr(self, a, None)
        self._knn = {}
        self._knn_other = {}
        self._fof = {}
        self._nlist = {}
        super().close()  # the context last

    def upload(self, hs):
        for k in ("m", "x", "v", "a", "ao"):
            arr = getattr(hs, k)
            assert arr.flags["C_CONTIGUOUS"] and arr.dtype == np_dtype(self.dtype)
        _check(lib().nbody_upload(self.h, _p(hs.m), _p(hs.x), _p(hs.v), _p(hs.a), _p(hs.ao), C.c_double(hs.dt), C.c_double(hs.c)))

    def download(self, hs=None):
        hs = hs or HostSystem(self.dtype, self.dim, self.n)
        _check(lib().nbody_download(self.h, _p(hs.m), _p(hs.x), _p(hs.v), _p(hs.a), _p(hs.ao)))
        st = self.state()
        hs.dt, hs.c = st.dt, st.c
        return hs

    def state(self, first=0, count=None):
        """Device view; (first, count) selects a shard of targets (v/a/ao pointers are offset to it)."""
        st = nbody_state()
        _check(lib().nbody_ctx_state(self.h, C.byref(st)))
        if first or (count is not None and count != self.n):
            count = self.n - first if count is None else count
            esz = (4 if self.dtype == F32 else 8) * self.dim
            st.first, st.count = first, count
            st.v, st.a, st.ao = st.v + first * esz, st.a + first * esz, st.ao + first * esz
        return st

    def sync(self):
        _check(lib().nbody_stream_sync(C.c_void_p(self.stream)))

    def configure_all_pairs(self, split=0, targets_per_thread=0, source_path=0):
        """K1 launch shape of THIS context (nbody_ctx_configure_all_pairs); state() then carries it in `tuning`."""
        _check(lib().nbody_ctx_configure_all_pairs(self.h, split, targets_per_thread, source_path))

    def set_shard(self, first, count):
        """nbody_ctx_set_shard: this context owns targets [first, first+count) (multi-GPU all-pairs)."""
        _check(lib().nbody_ctx_set_shard(self.h, C.c_uint32(first), C.c_uint32(count)))

    # K1/K2/K3
    def all_pairs_force(self, first=0, count=None):
        st = self.state(first, count)
        _check(lib().nbody_all_pairs_force(C.byref(st), C.c_void_p(self.stream)))

    def all_pairs_softened_force(self, eps, first=0, count=None):
        """K1 with Plummer softening eps > 0 (nbody_all_pairs_softened_force); (first, count) is a shard window as in all_pairs_force."""
        st = self.state(first, count)
        _check(lib().nbody_all_pairs_softened_force(C.byref(st), C.c_double(eps), C.c_void_p(self.stream)))

    def all_pairs_collapsed_force(self):
        st = self.state()
        _check(lib().nbody_all_pairs_collapsed_force(C.byref(st), C.c_void_p(self.stream)))

    def accelerate_step(self, first=0, count=None):
        st = self.state(first, count)
        _check(lib().nbody_accelerate_step(C.byref(st), C.c_void_p(self.stream)))

    # fourth-order Hermite (no reference counterpart)
    @property
    def hermite(self):
        if self._hermite is None:
            self._hermite = Hermite(self.dtype, self.dim, self.n, self.device)
        return self._hermite

    def hermite_start(self, eps):
        """Acceleration and jerk of the state as it is (nbody_hermite_force_jerk): before the first hermite_step and after an upload."""
        self.hermite.force_jerk(self.state(), eps, self.stream)

    def hermite_step(self, eps):
        """One Hermite step of dt (nbody_hermite_step); a StepGraph may record it (after hermite_start has been called)."""
        self.hermite.step(self.state(), eps, self.stream)

    def hermite_jerk(self):
        """The jerk of the last hermite_start / hermite_step, (n, dim) of T (blocking)."""
        return self.hermite.read(0, self.stream)

    def hermite_block_start(self, eps, eta_start=0.01, max_level=12):
        """Starts a run with block time steps (nbody_hermite_block_start): dt is the largest step, dt / 2^max_level the smallest."""
        self.hermite.block_start(self.state(), eps, eta_start, max_level, self.stream)

    def hermite_block_step(self, eps, eta):
        """One block step: (n_active, tau_next in ticks); tau_next == 2^max_level completes the interval of dt."""
        return self.hermite.block_step(self.state(), eps, eta, self.stream)

    def hermite_block_advance(self, eps, eta):
        """Block steps until the system is synchronous at t + dt: (block steps, body steps)."""
        return self.hermite.block_advance(self.state(), eps, eta, self.stream)

    def hermite_block_levels(self):
        """(levels, tau) of the bodies, int32 and uint32 (blocking)."""
        return self.hermite.block_read(0, self.stream), self.hermite.block_read(1, self.stream)

    def hermite_block_active(self, n_active):
        """The active list of the last block step (ascending body indices); n_active as hermite_block_step returned it."""
        return self.hermite.block_read(2, self.stream, n_active)

    # sixth-order Hermite (no reference counterpart)
    @property
    def hermite6(self):
        if self._hermite6 is None:
            self._hermite6 = Hermite6(self.dtype, self.dim, self.n, self.device)
        return self._hermite6

    def hermite6_start(self, eps):
        """Acceleration, jerk and snap of the state as it is, crackle = 0 (nbody_hermite6_start): before the first hermite6_step and
        after an upload."""
        self.hermite6.start(self.state(), eps, self.stream)

    def hermite6_step(self, eps):
        """One sixth-order Hermite step of dt (nbody_hermite6_step); a StepGraph may record it (after hermite6_start has been called)."""
        self.hermite6.step(self.state(), eps, self.stream)

    def hermite6_read(self, what):
        """0 the jerk, 1 the snap, 2 the crackle, 3 / 4 / 5 the predicted x / v / a of the last hermite6_start / hermite6_step,
        (n, dim) of T (blocking)."""
        return self.hermite6.read(what, self.stream)

    def hermite6_block_start(self, eps, eta_start=0.01, max_level=12):
        """Starts a sixth-order run with block time steps (nbody_hermite6_block_start): dt is the largest step, dt / 2^max_level the
        smallest.  Double only."""
        self.hermite6.block_start(self.state(), eps, eta_start, max_level, self.stream)

    def hermite6_block_step(self, eps, eta):
        """One block step (nbody_hermite6_block_step): (n_active, tau_next in ticks)."""
        return self.hermite6.block_step(self.state(), eps, eta, self.stream)

    def hermite6_block_advance(self, eps, eta):
        """Block steps until the system is synchronous at t + dt (nbody_hermite6_block_advance): (block steps, body steps)."""
        return self.hermite6.block_advance(self.state(), eps, eta, self.stream)

    def hermite6_block_levels(self):
        """The levels (int32) and tau_i in ticks (uint32) of all bodies (blocking)."""
        return self.hermite6.block_read(0, self.stream), self.hermite6.block_read(1, self.stream)

    def hermite6_block_active(self, n_active):
        """The active list of the last block step (ascending body indices); n_active as hermite6_block_step returned it."""
        return self.hermite6.block_read(2, self.stream, n_active)

    # block time steps for the octree leapfrog (no reference counterpart)
    @property
    def octree_block(self):
        if self._octree_block is None:
            self._octree_block = OctreeBlock(self.dtype, self.dim, self.n, self.device)
        return self._octree_block

    def octree_block_start(self, theta, eps, eta, max_level=12):
        """Starts a run of the octree leapfrog with block time steps (nbody_octree_block_start): the softened force of all bodies and
        the first levels; dt is the largest step, dt / 2^max_level the smallest."""
        self.octree_block.start(self.octree, self.state(), theta, eps, eta, max_level, self.stream)

    def octree_block_step(self, theta, eps, eta):
        """One block step: (n_active, tau_next in ticks); tau_next == 2^max_level completes the interval of dt."""
        return self.octree_block.step(self.octree, self.state(), theta, eps, eta, self.stream)

    def octree_block_advance(self, theta, eps, eta):
        """Block steps until the system is synchronous at t + dt: (block steps, body steps)."""
        return self.octree_block.advance(self.octree, self.state(), theta, eps, eta, self.stream)

    def octree_block_levels(self):
        """(levels, tau) of the bodies, int32 and uint32 (blocking)."""
        return self.octree_block.read(0, self.stream), self.octree_block.read(1, self.stream)

    def octree_block_active(self, n_active):
        """The active list of the last block step (ascending body indices); n_active as octree_block_step returned it."""
        return self.octree_block.read(2, self.stream, n_active)

    def octree_block_predicted(self):
        """The predicted positions of the last block step, (n, dim) of T (blocking)."""
        return self.octree_block.read(3, self.stream)

    # per-body potentials, nearest neighbours, closest pair (no reference counterpart)
    @property
    def neighbours_handle(self):
        if self._neighbours is None:
            self._neighbours = Neighbours(self.dtype, self.dim, self.n, self.device)
        return self._neighbours

    def neighbours_compute(self, eps):
        """nbody_neighbours_compute on the state as it is; a StepGraph may record it."""
        self.neighbours_handle.compute(self.state(), eps, self.stream)

    def neighbours(self, eps):
        """(phi, nn, nnd2) of the state as it is: phi_i = -c sum_{j != i} m_j / sqrt(|x_i - x_j|^2 + eps^2) (n,) of T, nn_i the nearest
        neighbour (n,) uint32, nnd2_i its unsoftened squared distance (n,) of T (blocking)."""
        h = self.neighbours_handle
        h.compute(self.state(), eps, self.stream)
        return h.read(0, self.stream), h.read(1, self.stream), h.read(2, self.stream)

    def closest_pair(self, eps):
        """(i, j, d2), i < j: the closest pair of the state as it is (blocking)."""
        h = self.neighbours_handle
        h.compute(self.state(), eps, self.stream)
        return h.closest_pair(self.stream)

    # k nearest neighbours, local densities, density centre (no reference counterpart)
    def knn_handle(self, k, method="all-pairs"):
        """The Knn handle of this system for (k, method), made at the first use and closed with the system."""
        handles = self._knn if method == "all-pairs" else self._knn_other  # _knn: the all-pairs handles, by k
        key = k if method == "all-pairs" else (k, method)
        if key not in handles:
            handles[key] = Knn(self.dtype, self.dim, self.n, k, self.device, method)
        return handles[key]

    def knn_compute(self, k, method="all-pairs"):
        """nbody_knn_compute on the state as it is; a StepGraph may record it (the handle for (k, method) is made before the
        recording)."""
        self.knn_handle(k, method).compute(self.state(), self.stream)

    def knn(self, k, method="all-pairs"):
        """(idx (n, k) uint32, d2 (n, k) of T): the k nearest neighbours of every body, ascending in (d2, index), and their unsoftened
        squared distances; unused slots (n <= k) hold (0xffffffff, +inf) (blocking)."""
        h = self.knn_handle(k, method)
        h.compute(self.state(), self.stream)
        return h.read(0, self.stream), h.read(1, self.stream)

    def local_density(self, k=6, method="all-pairs"):
        """rho (n,) of T: Casertano & Hut's local density from the k-th neighbour (blocking)."""
        h = self.knn_handle(k, method)
        h.compute(self.state(), self.stream)
        return h.read(2, self.stream)

    def density_centre(self, k=6, method="all-pairs"):
        """(x_dc (dim,), r_c, rho_c): the density centre, core radius and core density from the k-th-neighbour densities (blocking)."""
        h = self.knn_handle(k, method)
        h.compute(self.state(), self.stream)
        return h.density_centre(self.stream)

    # friends-of-friends groups (no reference counterpart)
    def fof_handle(self, min_members=1):
        """The Fof handle of this system for min_members, made at the first use and closed with the system."""
        if min_members not in self._fof:
            self._fof[min_members] = Fof(self.dtype, self.dim, self.n, min_members, self.device)
        return self._fof[min_members]

    def fof_compute(self, b, min_members=1):
        """nbody_fof_compute on the state as it is; a StepGraph may record it (the handle for min_members is made before the
        recording)."""
        self.fof_handle(min_members).compute(self.state(), b, self.stream)

    def fof(self, b, min_members=1):
        """(label (n,) uint32, size (n,) uint32) of the state as it is for the linking length b: the lowest index in every body's
        group and the group's member count (blocking)."""
        h = self.fof_handle(min_members)
        h.compute(self.state(), b, self.stream)
        return h.read(0, self.stream), h.read(1, self.stream)

    def fof_groups(self, b, min_members=20):
        """(catalogue, summary): the groups of at least min_members bodies ({"label", "size", "mass", "com"}, ascending label) and
        (groups, catalogued groups, largest size, its label) (blocking)."""
        h = self.fof_handle(min_members)
        h.compute(self.state(), b, self.stream)
        return h.catalogue(self.stream), h.summary(self.stream)

    # exact fixed-radius neighbour lists (no reference counterpart)
    def nlist_handle(self, capacity=0):
        """The NeighbourLists handle of this system for `capacity` list entries (0: counts only), made at the first use and closed
        with the system."""
        capacity = int(capacity)
        if capacity not in self._nlist:
            self._nlist[capacity] = NeighbourLists(self.dtype, self.dim, self.n, capacity, self.device)
        return self._nlist[capacity]

    def nlist_compute(self, r, capacity=0):
        """nbody_nlist_compute on the state as it is; a StepGraph may record it (the handle for `capacity` is made before the
        recording).  The radius is r unless that handle holds per-body radii (nlist_handle(capacity).set_radii)."""
        self.nlist_handle(capacity).compute(self.state(), r, self.stream)

    def _nlist_run(self, h, r, radii, squared):
        if (r is None) == (radii is None):
            raise ValueError("give either a radius r or per-body radii")
        if radii is None:
            h.clear_radii(self.stream)
        else:
            h.set_radii(radii, squared, self.stream)
        h.compute(self.state(), 0.0 if r is None else r, self.stream)

    def radius_counts(self, r=None, radii=None, squared=False):
        """count (n,) uint32: the number of bodies j != i with d2_ij <= r2_i, for one radius r or per-body radii (squared=True: the
        values are r2_i) (blocking)."""
        h = self.nlist_handle(0)
        self._nlist_run(h, r, radii, squared)
        return h.read(0, self.stream)

    def radius_neighbours(self, r=None, radii=None, squared=False, capacity=None):
        """(offset (n + 1,) uint64, idx (total,) uint32): the neighbours of body i within its radius are idx[offset[i]:offset[i + 1]],
        ascending (blocking).  capacity=None: the counts-only handle gives the total and a handle of exactly that capacity the list;
        with a capacity that turns out too small, or a body with more than NeighbourLists.MAX_PER_BODY neighbours, NbodyError."""
        if capacity is None:
            h0 = self.nlist_handle(0)
            self._nlist_run(h0, r, radii, squared)
            capacity = int(h0.summary(self.stream)[0])
        h = self.nlist_handle(capacity)
        self._nlist_run(h, r, radii, squared)
        return h.read(1, self.stream), h.read(2, self.stream)

    def calc_energies(self, softening=0.0):
        """(kinetic, potential) as in System::calc_energies (src/system.h:62-79); blocking.  softening > 0: the potential of the
        softened force, -c/2 sum_i m_i sum_{j != i} m_j / sqrt(|x_i - x_j|^2 + softening^2) (nbody_calc_energies_softened)."""
        t = np_dtype(self.dtype)
        ke, pe = np.zeros(1, t), np.zeros(1, t)
        st = self.state()
        if softening:
            _check(lib().nbody_calc_energies_softened(C.byref(st), C.c_double(softening), _p(ke), _p(pe), C.c_void_p(self.stream)))
        else:
            _check(lib().nbody_calc_energies(C.byref(st), _p(ke), _p(pe), C.c_void_p(self.stream)))
        return ke[0], pe[0]

    # K4..K9
    @property
    def bvh(self):
        if self._bvh is None:
            self._bvh = Bvh(self.dtype, self.dim, self.n, self.device)
        return self._bvh

    @property
    def octree(self):
        if self._octree is None:
            self._octree = Octree(self.dtype, self.dim, self.n, self.device)
        return self._octree

    def _octree_build(self, quadrupole=False):
        st, t = self.state(), self.octree
        t.clear(self.stream)
        t.compute_bounds(st, self.stream)
        t.insert(st, self.stream)
        t.compute_tree(self.stream)
        if quadrupole:
            t.compute_quadrupoles(self.stream)
        return st, t

    def octree_potential(self, theta, softening=0.0, quadrupole=False):
        """Per-body potentials phi_i = -c S_i from the tree, built like octree_force; returns a NumPy array (n,) of T."""
        if softening and quadrupole:
            raise ValueError("octree_potential: softening and quadrupole cannot be combined")
        import torch
        st, t = self._octree_build(quadrupole)
        phi = torch.empty(self.n, dtype=torch.float32 if self.dtype == F32 else torch.float64, device=f"cuda:{self.device}")
        if quadrupole:
            t.compute_quadrupole_potential(st, theta, phi.data_ptr(), self.stream)
        elif softening:
            t.compute_softened_potential(st, theta, softening, phi.data_ptr(), self.stream)
        else:
            t.compute_potential(st, theta, phi.data_ptr(), self.stream)
        self.sync()
        return phi.cpu().numpy()

    def octree_energies(self, theta, softening=0.0, quadrupole=False):
        """(kinetic, potential) with the potential from the tree, built like octree_force (nbody_octree_calc_energies)."""
        if softening and quadrupole:
            raise ValueError("octree_energies: softening and quadrupole cannot be combined")
        st, t = self._octree_build(quadrupole)
        return t.calc_energies(st, theta, softening, quadrupole, self.stream)

    def octree_force(self, theta, softening=0.0, quadrupole=False):
        """One force phase of run_octree (src/octree.h:321-326); softening > 0 takes the softened walk, quadrupole=True the
        quadrupole pass and walk (the two do not combine)."""
        if softening and quadrupole:
            raise ValueError("octree_force: softening and quadrupole cannot be combined")
        st, t = self.state(), self.octree
        t.clear(self.stream)
        t.compute_bounds(st, self.stream)
        t.insert(st, self.stream)
        t.compute_tree(self.stream)
        if quadrupole:
            t.compute_quadrupoles(self.stream)
            t.compute_quadrupole_force(st, theta, self.stream)
        elif softening:
            t.compute_softened_force(st, theta, softening, self.stream)
        else:
            t.compute_force(st, theta, self.stream)

    def bvh_force(self, theta):
        """One force phase of run_bvh (src/bvh.h:382-393)."""
        st, b = self.state(), self.bvh
        b.bounding_box(st, self.stream)
        b.hilbert_sort(st, self.stream)
        b.build_tree(st, self.stream)
        b.compute_force(st, theta, self.stream)


def _load_sharded():
    import importlib.util
    import sys
    name = __name__ + ".sharded"
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "sharded.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


parallel = _load_sharded()


class StepGraph(_Handle):
    """Records the phase calls of one step on the device's stream (HIP stream capture) and replays them."""

    _destroy = "nbody_graph_destroy"

    def __init__(self, dev, record):
        self.dev, self.h = dev, C.c_void_p()
        _check(lib().nbody_graph_begin(C.c_void_p(dev.stream)))
        try:
            record()
        finally:
            _check(lib().nbody_graph_end(C.c_void_p(dev.stream), C.byref(self.h)))

    def launch(self):
        _check(lib().nbody_graph_launch(self.h, C.c_void_p(self.dev.stream)))


def executed_steps(steps, csv_detailed, warmup=10):
    """Step-count semantics of the reference drivers."""
    return steps if csv_detailed else max(steps, warmup)


OCTREE_CHECK_EVERY = 64


def run(dev, algorithm, nsteps, theta=0.5):
    """The step loop of run_all_pairs / run_bvh / run_octree on the device.  Octree builds report trouble (bodies that
    never separate, node pool, walk stack or step budget exhausted) through a sticky device-side flag: it is read every
    OCTREE_CHECK_EVERY steps and after the last one, and raises — a flagged build drops mass, never integrate on."""
    for k in range(nsteps):
        if algorithm == "all-pairs":
            dev.all_pairs_force()
        elif algorithm == "all-pairs-collapsed":
            dev.all_pairs_collapsed_force()
        elif algorithm == "bvh":
            dev.bvh_force(theta)
        elif algorithm == "octree":
            dev.octree_force(theta)
            if (k + 1) % OCTREE_CHECK_EVERY == 0:
                dev.octree.info(dev.stream)
        else:
            raise ValueError(algorithm)
        dev.accelerate_step()
    if algorithm == "octree" and nsteps > 0:
        dev.octree.info(dev.stream)
    dev.sync()
