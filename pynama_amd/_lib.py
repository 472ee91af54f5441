"""ctypes binding of libpynama_hip.so (include/pynama_hip.h).

There is NO CPU fallback: if the library is missing or no MI355X is visible, every compute
entry raises.  Loading the library and checking its symbols works without a GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_LIB_PATH = os.path.join(_HERE, "libpynama_hip.so")
LIB_PATH = os.environ.get("PYNAMA_LIB_PATH") or _DEFAULT_LIB_PATH   # (the override: A/B of two builds, tools/)
_NEWER_SYMBOLS = ("pyn_assemble_last_rows", "pyn_ho3_geometry")   # diagnostics an older build under PYNAMA_LIB_PATH may lack (never the in-tree library)
CSRC = os.path.join(_HERE, "csrc")

# enums of include/pynama_hip.h
Q_FULL, Q_RED, Q_NODAL = 0, 1, 2
FORM_LAPLACE, FORM_MASS_NODAL, FORM_MASS_FULL, FORM_KLE, FORM_OPERATOR = 0, 1, 2, 3, 4
KSP_CG, KSP_GMRES = 0, 1
MATFREE_OFF, MATFREE_LAPLACE, MATFREE_KLE, MATFREE_KLE_GENERAL, MATFREE_KLE_NGL3_GENERAL = 0, 1, 2, 3, 4
PC_NONE, PC_JACOBI, PC_MG = 0, 1, 2
MG_MAX_LEVELS = 16
TS_MAX_STAGES = 8
NORM_PRECONDITIONED, NORM_UNPRECONDITIONED, NORM_NATURAL = 0, 1, 2
T_SYMBOLIC, T_ASSEMBLE, T_SPMV, T_SOLVE, T_INTEGRATE = 0, 1, 2, 3, 4
RULE_NODAL, RULE_GAUSS = 0, 1
# PYN_FIELD_*: the closed-form fields of cases/custom_func.py that pyn_field_eval evaluates on the device
(FIELD_TG2D_VEL, FIELD_TG2D_VORT, FIELD_TG3D_VEL, FIELD_TG3D_VORT, FIELD_TG3D_CONV, FIELD_TG3D_DIFF,
 FIELD_SEN2D_VEL, FIELD_SEN2D_VORT, FIELD_SEN2D_CONV, FIELD_SEN2D_DIFF) = range(10)
FIELD_COUNT, FIELD_MAX_PARAMS = 10, 4


class PynamaHipError(RuntimeError):
    pass


class SolveOpts(C.Structure):
    _fields_ = [("method", C.c_int), ("pc", C.c_int), ("norm_type", C.c_int), ("maxit", C.c_int),
                ("restart", C.c_int), ("fixed_iters", C.c_int), ("profile", C.c_int), ("cg_variant", C.c_int),
                ("gmres_orthog", C.c_int), ("matfree", C.c_int), ("rtol", C.c_double), ("atol", C.c_double), ("dtol", C.c_double)]


class MgOpts(C.Structure):
    """pyn_mg_opts: a zero field takes the library's default"""
    _fields_ = [("max_levels", C.c_int), ("smooth_degree", C.c_int), ("coarse_max_rows", C.c_int), ("esteig_its", C.c_int),
                ("esteig_min", C.c_double), ("esteig_max", C.c_double)]


class SolveInfo(C.Structure):
    _fields_ = [("iters", C.c_int), ("reason", C.c_int), ("rnorm", C.c_double), ("rnorm0", C.c_double),
                ("true_resid", C.c_double), ("solve_ms", C.c_double), ("spmv_ms", C.c_double),
                ("spmv_launches", C.c_int), ("reduce_ms", C.c_double), ("halo_ms", C.c_double)]


_P = C.c_void_p
_I, _L, _D = C.c_int, C.c_int64, C.c_double
_pi32 = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_pi64 = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
_pf64 = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_pu8 = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")

# name -> argtypes ; every function returns int except pyn_last_error
SIGNATURES = {
    "pyn_version": [],
    "pyn_device_count": [C.POINTER(_I)],
    "pyn_alloc_live": [C.POINTER(_L), C.POINTER(_L)],
    "pyn_ctx_create": [_I, C.POINTER(_P)],
    "pyn_ctx_destroy": [_P],
    "pyn_sync": [_P],
    "pyn_comm_unique_id": [C.c_char_p, _I],
    "pyn_comm_init": [_P, _I, _I, C.c_char_p, _I],
    "pyn_comm_init_shm": [_P, _I, _I, C.c_char_p, _L],
    "pyn_comm_barrier": [_P],
    "pyn_comm_allreduce_f64": [_P, _pf64, _I, _I],
    "pyn_comm_selftest": [_P, _pf64, _I],
    "pyn_halo_set": [_P, _L, _L, _I, _pi32, _pi64, _pi32, _pi64],
    "pyn_mesh_set": [_P, _I, _I, _L, _L, _pi32, _pf64],
    "pyn_mesh_topology": [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)],
    "pyn_mesh_ho_lattice": [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)],
    "pyn_ho_matfree_max_ngl": [_I],
    "pyn_ho_tables_1d": [_I, _pf64, _pf64, _pf64, _pf64, _pf64, _pf64, _pf64],
    "pyn_ho_local_lattice": [_I, _I, _pi32],
    "pyn_elem_tables_set": [_P, _I, _I, _pf64, _pf64, _pf64, _pf64],
    "pyn_bc_set": [_P, _I, _P],
    "pyn_csr_symbolic": [_P],
    "pyn_csr_info": [_P, C.POINTER(_L), C.POINTER(_L)],
    "pyn_csr_get": [_P, C.c_void_p, C.c_void_p],
    "pyn_patch_plan_set": [_P, _I, _P, _P],
    "pyn_patch_plan_set_kind": [_P, _I, _I, _P, _P],
    "pyn_patch_plan_info": [_P, _I, _P],
    "pyn_mesh_box": [_P, _I, _I, _P, _L, _P, _P, _L, _P, _P],
    "pyn_mesh_get": [_P, _P, _P],
    "pyn_mat_create": [_P, _I, _I, C.POINTER(_I)],
    "pyn_mat_create_rhs": [_P, _I, _I, C.POINTER(_I)],
    "pyn_mat_stored_blocks": [_P, _I, C.POINTER(_L), C.POINTER(_L)],
    "pyn_mat_destroy": [_P, _I],
    "pyn_mat_zero": [_P, _I],
    "pyn_mat_add_values": [_P, _I, _I, _pi32, _I, _pi32, _pf64, _I],
    "pyn_mat_get_values": [_P, _I, _pf64],
    "pyn_mat_get_diagonal": [_P, _I, _I],
    "pyn_mat_axpy": [_P, _I, _D, _I],
    "pyn_mat_row_scale": [_P, _I, _I],
    "pyn_vec_create": [_P, _I, C.POINTER(_I)],
    "pyn_vec_destroy": [_P, _I],
    "pyn_vec_set_host": [_P, _I, _pf64],
    "pyn_vec_set_local_host": [_P, _I, _pf64],
    "pyn_vec_get_host": [_P, _I, _pf64],
    "pyn_vec_fill": [_P, _I, _D],
    "pyn_vec_scatter_host": [_P, _I, _L, _pi32, _pf64, _I],
    "pyn_vec_axpby": [_P, _I, _D, _I, _D, _I],
    "pyn_vec_pointwise_mult": [_P, _I, _I, _I],
    "pyn_vec_reciprocal": [_P, _I],
    "pyn_vec_vtensv": [_P, _I, _I],
    "pyn_vec_dot": [_P, _I, _I, C.POINTER(_D)],
    "pyn_vec_norm": [_P, _I, _I, C.POINTER(_D)],
    "pyn_vec_maxpy": [_P, _I, _I, _I, _pi32, _pf64],
    "pyn_ts_step_finish": [_P, _I, _I, _pi32, _pf64, _P, _D, _D, C.POINTER(_D)],
    "pyn_nodeset_create": [_P, _L, _P, C.POINTER(_I)],
    "pyn_nodeset_destroy": [_P, _I],
    "pyn_field_info": [_I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)],
    "pyn_field_eval": [_P, _I, _pf64, _I, _I, _I],
    "pyn_vec_set_nodes": [_P, _I, _I, _pf64, _I, _P],
    "pyn_assemble_kle": [_P, _D, _D, _I, _I, _I, _I, _I],
    "pyn_assemble_kle_noslip": [_P, _D, _D, C.POINTER(_I)],
    "pyn_assemble_scalar": [_P, _I, _I, _I, _I],
    "pyn_elem_local": [_P, _I, _D, _D, _pf64, _P, _P, _P],
    "pyn_assemble_operator": [_P, _I, _I, _pi32, _pf64, _I],
    "pyn_elem_operator_local": [_P, _I, _I, _I, _I, _pi32, _pf64, _pf64, _pf64],
    "pyn_spmv": [_P, _I, _I, _I],
    "pyn_product_last": [_P, _pi64],
    "pyn_product_choose": [_I] * 4 + [_L, _L] + [_I] * 7 + [_D, _I, _I] + [C.POINTER(_I)] * 4,
    "pyn_assemble_last": [_P, _pi64],
    "pyn_assemble_last_rows": [_P, _pi64],
    "pyn_ho3_geometry": [_P, _pi64],
    "pyn_assemble_choose": [_pi64, _pi64, _pi64, _pi64],
    "pyn_assemble_choose_layout": [C.c_char_p, _I],
    "pyn_matfree_apply": [_P, _I, _I, _I],
    "pyn_matfree_set": [_P, _I, _D, _D],
    "pyn_solve": [_P, _I, _I, _I, C.POINTER(SolveOpts), C.POINTER(SolveInfo)],
    "pyn_direct_max_rows": [],
    "pyn_solve_direct": [_P, _I, _I, _I, C.POINTER(SolveInfo)],
    "pyn_direct_band_info": [_P, _I, C.POINTER(_L), C.POINTER(_L), C.POINTER(_L)],
    "pyn_solve_direct_band": [_P, _I, _I, _I, _L, C.POINTER(SolveInfo)],
    "pyn_mg_setup": [_P, _I, C.POINTER(MgOpts)],
    "pyn_mg_info": [_P, _I, C.POINTER(_I), _pi64, _pf64, C.POINTER(_D), C.POINTER(_I)],
    "pyn_mg_apply": [_P, _I, _I, _I],
    "pyn_mg_level_get": [_P, _I, _I, _pf64],
    "pyn_ibm_set": [_P, _I, _I, _L, _pf64, _pf64, _pf64, _pf64],
    "pyn_ibm_interp": [_P, _I, _pf64],
    "pyn_ibm_spread": [_P, _pf64, _I],
    "pyn_ibm_correct": [_P, _I, _pf64, _pf64],
    "pyn_ibm_matrix_get": [_P, _pf64],
    "pyn_ibm_info": [_P, _pi64],
    "pyn_ibm_clear": [_P],
    "pyn_probe_create": [_P, _L, _pf64, C.POINTER(_I)],
    "pyn_probe_info": [_P, _I, _pi64],
    "pyn_probe_get": [_P, _I, _pi32, _pf64],
    "pyn_probe_sample": [_P, _I, _I, _pf64],
    "pyn_probe_destroy": [_P, _I],
    "pyn_integrate": [_P, _I, _I, _I, _I, _pf64, C.POINTER(_I)],
    "pyn_integrate_len": [_I, _I, _I],
    "pyn_timers_get": [_P, _pf64, _I],
}

_lib = None


def build_library(force=False):
    """Compile libpynama_hip.so for gfx950 with hipcc (in-tree)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-j4"])
    return LIB_PATH


def load_library():
    """dlopen the library and bind every symbol of the header.  No GPU needed."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PynamaHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C pynama_amd/csrc`). pynama_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        if name in _NEWER_SYMBOLS and LIB_PATH != _DEFAULT_LIB_PATH and not hasattr(lib, name):
            continue                     # an older build loaded for an A/B: the diagnostics it predates report "unknown"
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.argtypes = args
        fn.restype = C.c_int
    for name in ("pyn_last_error", "pyn_source_hash"):
        getattr(lib, name).argtypes = []
        getattr(lib, name).restype = C.c_char_p
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise PynamaHipError(f"[{rc}] {_lib.pyn_last_error().decode(errors='replace')}")


def source_hash() -> str:
    """identity of the kernel sources the loaded library was built from (profiles/*.json record it)"""
    return load_library().pyn_source_hash().decode()


def alloc_live():
    """(buffers, bytes) of device and pinned-host memory the library holds right now, over all contexts of the process"""
    n, b = _L(0), _L(0)
    _check(load_library().pyn_alloc_live(C.byref(n), C.byref(b)))
    return n.value, b.value


def device_count() -> int:
    lib = load_library()
    n = _I(0)
    _check(lib.pyn_device_count(C.byref(n)))
    return n.value


def ho_matfree_max_ngl(dim) -> int:
    """largest order (ngl) the matrix-free KLE operator of high-order box lattices has a kernel for"""
    return load_library().pyn_ho_matfree_max_ngl(int(dim))


def integrate_len(dim, bs, grad=False) -> int:
    """entries of Context.integrate for a vector of block size bs on a dim-D mesh (pyn_integrate_len; 0: no such dim or bs)"""
    return load_library().pyn_integrate_len(int(dim), int(bs), 1 if grad else 0)


def ho_tables_1d(ngl):
    """The 1-D tables the matrix-free KLE operator of order ngl >= 4 recomputes on the host (no device needed): dict with xl, wl
    (Lobatto nodes / weights), Dl [ngl, ngl] (Dl[i, a] = h_a'(xl_i)), xr, wr (Gauss(ngl-1)), Br, Gr [ngl-1, ngl] (values and
    derivatives of the Lagrange functions at the Gauss points)."""
    n = int(ngl)
    if n < 2:
        raise PynamaHipError(f"ho_tables_1d: ngl {n} out of range")
    t = dict(xl=np.zeros(n), wl=np.zeros(n), Dl=np.zeros((n, n)), xr=np.zeros(n - 1), wr=np.zeros(n - 1),
             Br=np.zeros((n - 1, n)), Gr=np.zeros((n - 1, n)))
    _check(load_library().pyn_ho_tables_1d(n, *(t[k] for k in ("xl", "wl", "Dl", "xr", "wr", "Br", "Gr"))))
    return t


def ho_local_lattice(ngl, dim):
    """[ngl^dim, dim] lattice offset of every local node of a box-mesh cell as the library's lattice check assumes it"""
    loc = np.zeros((int(ngl) ** int(dim), int(dim)), np.int32)
    _check(load_library().pyn_ho_local_lattice(int(ngl), int(dim), loc))
    return loc


def field_info(field):
    """(dim, block size, number of parameters) of a PYN_FIELD_* id as the library holds them (no device needed)"""
    d, b, n = _I(0), _I(0), _I(0)
    _check(load_library().pyn_field_info(int(field), C.byref(d), C.byref(b), C.byref(n)))
    return d.value, b.value, n.value


def product_choose(br, bc, npat, maxw, nnzb, n_owned, rhs_compact=False, solver=False, image=False, sell_image=False,
                   block_sell=False, no_csrlb=False, no_sell=False, bcsr_min_avg=None, bcsr_lanes=None, bcsr_unroll=None):
    """The product kernel the library would resolve for a matrix with these facts under these knobs (no device needed; None = knob
    not set): (kind, W, lanes, unroll), kind as slot 0 of Context.product_last()."""
    out = [_I(0) for _ in range(4)]
    _check(load_library().pyn_product_choose(
        int(br), int(bc), int(npat), int(maxw), int(nnzb), int(n_owned), int(rhs_compact), int(solver), int(image), int(sell_image),
        int(block_sell), int(no_csrlb), int(no_sell), -1.0 if bcsr_min_avg is None else float(bcsr_min_avg),
        -1 if bcsr_lanes is None else int(bcsr_lanes), -1 if bcsr_unroll is None else int(bcsr_unroll), *(C.byref(o) for o in out)))
    return tuple(o.value for o in out)


ASSEMBLY_KINDS = ("none", "generic", "p1", "patch", "lattice", "march", "kle_lattice", "rowrun")
AK_NONE, AK_GENERIC, AK_P1, AK_PATCH, AK_LATTICE, AK_MARCH, AK_KLE_LATTICE, AK_ROWRUN = range(8)
_ASM_LAST_KEYS = ("kind", "shape", "k_closed", "rw_closed", "generic", "krhs_completed", "dinv", "count")


def assemble_choose_layout():
    """{'request': names, 'facts': names, 'knobs': names}: the order of the three integer arrays of pyn_assemble_choose"""
    buf = C.create_string_buffer(4096)
    _check(load_library().pyn_assemble_choose_layout(buf, len(buf)))
    return {part.split(":")[0]: tuple(n for n in part.split(":")[1].split(",") if n) for part in buf.value.decode().split(";")}


def assemble_choose(request, facts, knobs=None):
    """The kernel family the library would resolve for an assembly request (dict: form, variant, K, Krhs, Rw, Rd, krhs_compact,
    op_rule, op_nterms; variant defaults to 1, the rest to 0) on a context with these facts (dict, missing = 0) under these knobs
    (dict, missing = not set; flags True / 1).  No device needed.  Returns the slots 'kind' .. 'dinv' of Context.assemble_last()
    ('krhs_completed': left to the completion pass) + 'rowrun_candidate'."""
    layout = assemble_choose_layout()
    given = {"request": dict({"variant": 1}, **request), "facts": dict(facts), "knobs": dict(knobs or {})}
    arrays = {}
    for part, names in layout.items():
        unknown = set(given[part]) - set(names)
        if unknown:
            raise PynamaHipError(f"assemble_choose: unknown {part} {sorted(unknown)}")
        arrays[part] = np.array([int(given[part].get(n, -1 if part == "knobs" else 0)) for n in names], np.int64)
    out = np.zeros(8, np.int64)
    _check(load_library().pyn_assemble_choose(arrays["request"], arrays["facts"], arrays["knobs"], out))
    return dict({k: int(v) for k, v in zip(_ASM_LAST_KEYS[:7], out)}, rowrun_candidate=int(out[7]))


class _stdout_to_stderr:
    """File descriptor 1 points at stderr inside the block: keeps C-level chatter of third-party libraries (RCCL's version
    banner) out of a program's stdout, which callers such as bench.py reserve for their own output."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        try:
            C.CDLL(None).fflush(None)       # C stdio buffers of the library must drain while fd 1 is still redirected
        except OSError:
            pass
        os.dup2(self._saved, 1)
        os.close(self._saved)
        return False


def default_device() -> int:
    """GPU of this process: LOCAL_RANK under a one-process-per-GPU launcher, else 0."""
    n = device_count()
    if n <= 0:
        raise PynamaHipError("no MI355X visible: pynama_amd has no CPU fallback")
    return int(os.environ.get("LOCAL_RANK", "0")) % n


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class Context:
    """One GPU, one process.  Thin, explicit wrapper: every method is one C-ABI call."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = _P()
        _check(self.lib.pyn_ctx_create(device, C.byref(h)))
        self.h = h
        self.rank, self.nranks = 0, 1
        self.dim = self.nn = 0
        self.n_owned = self.n_ghost = 0
        self._vec_bs = {}               # block size of every vector made by vec_create (probe_sample sizes its result by it)

    def close(self):
        if getattr(self, "h", None):
            self.lib.pyn_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- communicator
    @staticmethod
    def unique_id() -> bytes:
        lib = load_library()
        buf = C.create_string_buffer(128)
        with _stdout_to_stderr():
            _check(lib.pyn_comm_unique_id(buf, 128))
        return buf.raw

    def comm_init(self, rank, nranks, uid: bytes | None):
        with _stdout_to_stderr():       # RCCL prints a version banner on stdout when a communicator comes up
            _check(self.lib.pyn_comm_init(self.h, rank, nranks, uid, len(uid) if uid else 0))
        self.rank, self.nranks = rank, nranks

    @staticmethod
    def shm_size(nranks, cap_bytes):
        return 4096 + nranks * 512 + nranks * nranks * 16 + nranks * cap_bytes

    def comm_init_shm(self, rank, nranks, path, cap_bytes):
        """TEST transport (several ranks on one GPU): collectives staged through the shared-memory file `path`"""
        _check(self.lib.pyn_comm_init_shm(self.h, rank, nranks, path.encode(), cap_bytes))
        self.rank, self.nranks = rank, nranks

    def barrier(self):
        _check(self.lib.pyn_comm_barrier(self.h))

    def allreduce(self, values, op="sum"):
        a = _f64(np.atleast_1d(values)).copy()
        _check(self.lib.pyn_comm_allreduce_f64(self.h, a, a.size, 1 if op == "max" else 0))
        return a

    def comm_selftest(self):
        """rank count seen by RCCL, all-reduce of 1 / of the rank, rank-stamped halo exchange on both streams (raises on a mismatch)"""
        info = np.zeros(8)
        _check(self.lib.pyn_comm_selftest(self.h, info, info.size))
        out = {"transport": "rccl" if info[0] > 0 else "shm (test transport: ranks share one GPU, no RCCL)",
               "allreduce_sum_ones": info[1], "allreduce_sum_ranks": info[2],
               "halo_ghosts_checked_main_stream": int(info[3]), "halo_ghosts_checked_comm_stream": int(info[4]),
               "allreduce_beside_exchange_sum_ranks_plus_1": info[5]}
        if info[0] > 0:
            out["nranks_seen_by_rccl"] = int(info[0])      # counted by RCCL itself (ncclCommCount of both communicators)
            out["halo_communicator"] = "own (ncclCommSplit)" if info[6] == 1 else "shared with the all-reduces (split refused)"
        return out

    def halo_set(self, n_owned, n_ghost, neigh, send_ptr, send_idx, recv_ptr):
        neigh = _i32(neigh)
        _check(self.lib.pyn_halo_set(self.h, n_owned, n_ghost, len(neigh), neigh if len(neigh) else np.zeros(1, np.int32),
                                     np.ascontiguousarray(send_ptr, np.int64),
                                     _i32(send_idx) if len(send_idx) else np.zeros(1, np.int32),
                                     np.ascontiguousarray(recv_ptr, np.int64)))
        self._halo = True
        self.n_owned, self.n_ghost = int(n_owned), int(n_ghost)

    def sync(self):
        _check(self.lib.pyn_sync(self.h))

    # -- mesh / tables / bc
    def mesh_set(self, dim, conn, xyz):
        conn = _i32(conn)
        xyz = _f64(xyz)
        n_elem, nn = conn.shape
        n_node = xyz.shape[0]
        assert xyz.shape[1] == dim
        _check(self.lib.pyn_mesh_set(self.h, dim, nn, n_elem, n_node, conn, xyz))
        self.dim, self.nn, self.n_elem, self.n_node = dim, nn, n_elem, n_node
        self._bc_last = None
        if not getattr(self, "_halo", False):
            self.n_owned, self.n_ghost = n_node, 0

    def mesh_box(self, dim, ngl, nel_local, layer0, lattice, loc, planes, axes):
        """this rank's block of a structured box mesh, generated on the device (pyn_mesh_box): no host conn / xyz"""
        nel = np.ascontiguousarray(nel_local, dtype=np.int64)
        lat = np.ascontiguousarray(lattice, dtype=np.int64)
        loc = _i32(loc)
        planes = np.ascontiguousarray(planes, dtype=np.int64)
        axes = _f64(np.concatenate([np.asarray(a, dtype=np.float64) for a in axes]))
        assert loc.shape == (ngl ** dim, dim) and nel.size == dim and lat.size == dim and axes.size == int(lat.sum())
        _check(self.lib.pyn_mesh_box(self.h, dim, ngl, nel.ctypes.data_as(_P), int(layer0), lat.ctypes.data_as(_P),
                                     loc.ctypes.data_as(_P), planes.size, planes.ctypes.data_as(_P), axes.ctypes.data_as(_P)))
        per = int(np.prod(lat[:-1]))
        self.dim, self.nn, self.n_elem, self.n_node = dim, ngl ** dim, int(np.prod(nel)), per * planes.size
        self._bc_last = None
        if not getattr(self, "_halo", False):
            self.n_owned, self.n_ghost = self.n_node, 0

    def mesh_get(self, conn=True, xyz=True):
        """host copies of the local mesh as the device holds it"""
        cn = np.empty((self.n_elem, self.nn), np.int32) if conn else None
        xy = np.empty((self.n_node, self.dim), np.float64) if xyz else None
        _check(self.lib.pyn_mesh_get(self.h, cn.ctypes.data_as(_P) if conn else None, xy.ctypes.data_as(_P) if xyz else None))
        return cn, xy

    def patch_plan_info(self, kind=0):
        """(patches, longest patch in rows, longest row in entries, patch-element pairs) of the plan in use"""
        info = np.zeros(4, np.int64)
        _check(self.lib.pyn_patch_plan_info(self.h, kind, info.ctypes.data_as(_P)))
        return tuple(int(v) for v in info)

    def mesh_topology(self):
        """('lattice', nx, ny, nz) for structured Q1 hex meshes, ('general', 0, 0, 0) otherwise"""
        k, a, b, c = _I(0), _I(0), _I(0), _I(0)
        _check(self.lib.pyn_mesh_topology(self.h, C.byref(k), C.byref(a), C.byref(b), C.byref(c)))
        return (("general", "lattice", "lattice-ngl3", "lattice-q1-2d")[k.value], a.value, b.value, c.value)

    def tables_set(self, which, w, H, Hrs, HrsCoo):
        w = _f64(w)
        _check(self.lib.pyn_elem_tables_set(self.h, which, w.size, w, _f64(H), _f64(Hrs), _f64(HrsCoo)))

    def bc_set(self, ndof, mask):
        """Dirichlet mask per local DOF.  A mask identical to the one on the device is not sent again: the library stamps every
        pyn_bc_set as a new Dirichlet set (compact Krhs layouts, skipped zero blocks and cached element lists are tied to the stamp)."""
        if mask is None:
            self._bc_last = None
            _check(self.lib.pyn_bc_set(self.h, 0, None))
            return
        m = np.ascontiguousarray(mask, dtype=np.uint8)
        assert m.size == self.n_node * ndof
        last = getattr(self, "_bc_last", None)
        if last is not None and last[0] == ndof and last[1].shape == m.shape and np.array_equal(last[1], m):
            return
        _check(self.lib.pyn_bc_set(self.h, ndof, m.ctypes.data_as(_P)))
        self._bc_last = (ndof, m.copy())

    # -- graph
    def csr_symbolic(self):
        _check(self.lib.pyn_csr_symbolic(self.h))
        self.graph_gen = getattr(self, "graph_gen", 0) + 1     # every matrix handle of the previous graph is dead now
        nr, nz = _L(0), _L(0)
        _check(self.lib.pyn_csr_info(self.h, C.byref(nr), C.byref(nz)))
        self.n_rows, self.nnzb = nr.value, nz.value
        return nr.value, nz.value

    def csr_get(self, cols=True):
        """node graph on the host; cols=False copies the row offsets only (the column array is 27 x larger)"""
        rp = np.empty(self.n_rows + 1, np.int32)
        ci = np.empty(self.nnzb, np.int32) if cols else None
        _check(self.lib.pyn_csr_get(self.h, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p) if cols else None))
        return rp, ci

    def patch_plan_set(self, patch_ptr, patch_rows, kind=0):
        """kind 0: scalar forms (tiles of <= 352 rows), kind 1: tiled KLE assembly (<= 36 rows)"""
        if patch_ptr is None:
            _check(self.lib.pyn_patch_plan_set_kind(self.h, kind, 0, None, None))
            return
        pp = _i32(patch_ptr)
        pr = _i32(patch_rows)
        _check(self.lib.pyn_patch_plan_set_kind(self.h, kind, len(pp) - 1, pp.ctypes.data_as(_P), pr.ctypes.data_as(_P)))

    # -- matrices
    def mat_create(self, br, bc) -> int:
        i = _I(-1)
        _check(self.lib.pyn_mat_create(self.h, br, bc, C.byref(i)))
        return i.value

    def mat_create_rhs(self, br, bc) -> int:
        """compact imposed-column matrix (Krhs / Krhsfs / Arhs): only the node rows next to an imposed node are stored"""
        i = _I(-1)
        _check(self.lib.pyn_mat_create_rhs(self.h, br, bc, C.byref(i)))
        return i.value

    def mat_stored(self, mid):
        """(graph blocks, node rows) the matrix stores: the whole graph, or the boundary layer of a compact imposed-column matrix"""
        b, r = _L(0), _L(0)
        _check(self.lib.pyn_mat_stored_blocks(self.h, mid, C.byref(b), C.byref(r)))
        return b.value, r.value

    def mat_values(self, mid, br, bc):
        v = np.empty(self.nnzb * br * bc, np.float64)
        _check(self.lib.pyn_mat_get_values(self.h, mid, v))
        return v

    def mat_zero(self, mid):
        _check(self.lib.pyn_mat_zero(self.h, mid))

    def mat_axpy(self, y, a, x):
        _check(self.lib.pyn_mat_axpy(self.h, y, a, x))

    def mat_row_scale(self, mid, vid):
        _check(self.lib.pyn_mat_row_scale(self.h, mid, vid))

    def mat_add_values(self, mid, rows, cols, vals, insert=False):
        """dense block into the matrix at scalar DOF indices (Mat.setValues); a scalar `vals` fills the block"""
        rows, cols = _i32(np.atleast_1d(rows)), _i32(np.atleast_1d(cols))
        v = np.asarray(vals, dtype=np.float64)
        if v.size == 1:
            v = np.full(rows.size * cols.size, float(v.reshape(-1)[0]))
        v = np.ascontiguousarray(v.reshape(-1))
        assert v.size == rows.size * cols.size, "vals must hold len(rows) x len(cols) entries"
        _check(self.lib.pyn_mat_add_values(self.h, mid, rows.size, rows, cols.size, cols, v, 1 if insert else 0))

    def mat_destroy(self, mid):
        if self.h:
            _check(self.lib.pyn_mat_destroy(self.h, mid))

    def mat_diagonal(self, mid, vid):
        _check(self.lib.pyn_mat_get_diagonal(self.h, mid, vid))

    # -- vectors
    def vec_create(self, bs) -> int:
        i = _I(-1)
        _check(self.lib.pyn_vec_create(self.h, bs, C.byref(i)))
        self._vec_bs[i.value] = int(bs)
        return i.value

    def vec_destroy(self, vid):
        if self.h:
            _check(self.lib.pyn_vec_destroy(self.h, vid))

    def vec_set(self, vid, arr):
        _check(self.lib.pyn_vec_set_host(self.h, vid, _f64(arr)))

    def vec_set_local(self, vid, arr):
        a = _f64(arr)
        assert a.size % (self.n_owned + self.n_ghost) == 0
        _check(self.lib.pyn_vec_set_local_host(self.h, vid, a))

    def vec_get(self, vid, bs):
        out = np.empty(self.n_owned * bs, np.float64)
        _check(self.lib.pyn_vec_get_host(self.h, vid, out))
        return out

    def vec_fill(self, vid, value):
        _check(self.lib.pyn_vec_fill(self.h, vid, float(value)))

    def vec_scatter(self, vid, idx, vals, add=False):
        idx = _i32(idx)
        vals = _f64(vals)
        assert idx.size == vals.size
        _check(self.lib.pyn_vec_scatter_host(self.h, vid, idx.size, idx, vals, 1 if add else 0))

    def vec_axpby(self, w, a, x, b, y):
        _check(self.lib.pyn_vec_axpby(self.h, w, float(a), x, float(b), y))

    def vec_pointwise_mult(self, w, x, y):
        _check(self.lib.pyn_vec_pointwise_mult(self.h, w, x, y))

    def vec_reciprocal(self, x):
        _check(self.lib.pyn_vec_reciprocal(self.h, x))

    def vec_vtensv(self, v, out):
        _check(self.lib.pyn_vec_vtensv(self.h, v, out))

    def vec_dot(self, x, y) -> float:
        d = _D(0)
        _check(self.lib.pyn_vec_dot(self.h, x, y, C.byref(d)))
        return d.value

    def vec_maxpy(self, y, x, ids, w):
        """y = x + sum_j w[j] * vec ids[j] (at most TS_MAX_STAGES terms; y may be x)"""
        ids, w = _i32(ids), _f64(w)
        assert ids.size == w.size
        _check(self.lib.pyn_vec_maxpy(self.h, y, x, ids.size, ids, w))

    def ts_step_finish(self, x, ids, hb, hd=None, atol=0.0, rtol=0.0):
        """x += sum_j hb[j] * vec ids[j]; with hd, the weighted RMS norm of sum_j hd[j] * vec ids[j] (else None)"""
        ids, hb = _i32(ids), _f64(hb)
        assert ids.size == hb.size
        if hd is None:
            _check(self.lib.pyn_ts_step_finish(self.h, x, ids.size, ids, hb, None, float(atol), float(rtol), None))
            return None
        hd, out = _f64(hd), _D(0.0)
        assert hd.size == ids.size
        _check(self.lib.pyn_ts_step_finish(self.h, x, ids.size, ids, hb, hd.ctypes.data, float(atol), float(rtol), C.byref(out)))
        return out.value

    # -- node sets, analytic fields and constant values on them
    def nodeset_create(self, nodes) -> int:
        """device copy of a set of OWNED local nodes (strictly increasing, each in [0, n_owned); may be empty); the id dies with the
        mesh"""
        nodes = np.asarray(nodes).ravel()
        if nodes.size and (nodes.min() < -2 ** 31 or nodes.max() >= 2 ** 31):
            raise PynamaHipError("nodeset_create: a node id does not fit 32 bits")
        nodes = _i32(nodes)
        i = _I(-1)
        _check(self.lib.pyn_nodeset_create(self.h, nodes.size, nodes.ctypes.data_as(_P) if nodes.size else None, C.byref(i)))
        return i.value

    def nodeset_destroy(self, set_id):
        if self.h:
            _check(self.lib.pyn_nodeset_destroy(self.h, int(set_id)))

    def field_eval(self, field, params, set_id, vid):
        """vec[node*bs + k] = field_k(xyz[node]) over the node set (-1: every owned node), stream-ordered; params: the field's
        coordinate-independent factors, computed by the caller (include/pynama_hip.h lists them per field)"""
        params = _f64(np.atleast_1d(params)).ravel()
        _check(self.lib.pyn_field_eval(self.h, int(field), params if params.size else np.zeros(1), params.size, int(set_id), int(vid)))

    def vec_set_nodes(self, vid, set_id, values, dofs=None):
        """vec[node*bs + k] = values[k] over the node set (-1: every owned node) for the components with dofs[k] != 0 (None: all)"""
        values = _f64(np.atleast_1d(values)).ravel()
        d = None
        if dofs is not None:
            d = np.ascontiguousarray(dofs, dtype=np.uint8).ravel()
            if d.size != values.size:
                raise PynamaHipError(f"vec_set_nodes: {d.size} component flags for {values.size} values")
        _check(self.lib.pyn_vec_set_nodes(self.h, int(vid), int(set_id), values if values.size else np.zeros(1), values.size,
                                          d.ctypes.data_as(_P) if d is not None else None))

    def vec_norm(self, x, norm_type=2) -> float:
        d = _D(0)
        _check(self.lib.pyn_vec_norm(self.h, x, norm_type, C.byref(d)))
        return d.value

    # -- hot loops
    def assemble_kle(self, alpha_d, alpha_w, K=-1, Krhs=-1, Rw=-1, Rd=-1, variant=1):
        _check(self.lib.pyn_assemble_kle(self.h, alpha_d, alpha_w, K, Krhs, Rw, Rd, variant))

    def assemble_kle_noslip(self, alpha_d, alpha_w, mat_ids):
        ids = (_I * 8)(*[int(m) for m in mat_ids])
        _check(self.lib.pyn_assemble_kle_noslip(self.h, alpha_d, alpha_w, ids))

    def assemble_scalar(self, form, A=-1, Arhs=-1, variant=1):
        _check(self.lib.pyn_assemble_scalar(self.h, form, A, Arhs, variant))

    def elem_local(self, form, corners, alpha_d=1e3, alpha_w=1e2):
        dim, nn = self.dim, self.nn
        dw = 1 if dim == 2 else 3
        c = _f64(corners).ravel()
        assert c.size == (nn if nn == dim + 1 else 2 ** dim) * dim
        if form == FORM_KLE:
            o0 = np.empty((dim * nn, dim * nn))
            o1 = np.empty((dim * nn, dw * nn))
            o2 = np.empty((dim * nn, nn))
            _check(self.lib.pyn_elem_local(self.h, form, alpha_d, alpha_w, c, o0.ctypes.data_as(_P),
                                           o1.ctypes.data_as(_P), o2.ctypes.data_as(_P)))
            return o0, o1, o2
        o0 = np.empty((nn, nn))
        _check(self.lib.pyn_elem_local(self.h, form, 0.0, 0.0, c, o0.ctypes.data_as(_P), None, None))
        return o0

    def assemble_operator(self, rule, terms, coef, mid):
        t = _i32(terms).reshape(-1, 3)
        _check(self.lib.pyn_assemble_operator(self.h, rule, t.shape[0], t, _f64(coef), mid))

    def elem_operator_local(self, rule, br, bc, terms, coef, corners):
        t = _i32(terms).reshape(-1, 3)
        out = np.empty((br * self.nn, bc * self.nn))
        _check(self.lib.pyn_elem_operator_local(self.h, rule, br, bc, t.shape[0], t, _f64(coef), _f64(corners).ravel(), out))
        return out

    def spmv(self, mid, x, y):
        _check(self.lib.pyn_spmv(self.h, mid, x, y))

    def product_last(self):
        """the most recent product launch of this context: {'family' (0 none, 1 raw, 2 sell, 3 sellp, 4 sellb explicit, 5 sellb
        dictionary, 6 csrl, 7 csrlb, 8 bcsr), 'param' (W / lanes per node row / BC), 'unroll', 'dot', 'grid', 'npat', 'maxw',
        'launches' (running count)}"""
        info = np.zeros(8, np.int64)
        _check(self.lib.pyn_product_last(self.h, info))
        keys = ("family", "param", "unroll", "dot", "grid", "npat", "maxw", "launches")
        return {k: int(v) for k, v in zip(keys, info)}

    def assemble_last(self):
        """what the most recent numeric assembly of this context launched: {'kind' (index into ASSEMBLY_KINDS), 'shape' (tile id, or
        rows per run), 'k_closed', 'rw_closed', 'generic' (sub-variant), 'krhs_completed', 'dinv', 'count' (running count),
        'rows_form' (the rows kernel of rectilinear Q1 lattices: 0 did not run, 1 one workgroup per x-line, 2 persistent),
        'rows_grid' (its workgroups); both -1 from an older build under PYNAMA_LIB_PATH that does not record them}"""
        info, rows = np.zeros(8, np.int64), np.zeros(2, np.int64)
        _check(self.lib.pyn_assemble_last(self.h, info))
        if hasattr(self.lib, "pyn_assemble_last_rows"):
            _check(self.lib.pyn_assemble_last_rows(self.h, rows))
        else:                                # (an older build under PYNAMA_LIB_PATH)
            rows[:] = -1
        return dict({k: int(v) for k, v in zip(_ASM_LAST_KEYS, info)}, rows_form=int(rows[0]), rows_grid=int(rows[1]))

    def ho3_geometry(self):
        """what the row-run geometry pre-pass found on this mesh: {'affine', 'diag' (1 / 0; -1: the pass has not run), 'matfree_diag'
        (form of the matrix-free KLE operator set on a second-order lattice; -1: none set)}; all -1 from an older build under
        PYNAMA_LIB_PATH"""
        info = np.full(3, -1, np.int64)
        if hasattr(self.lib, "pyn_ho3_geometry"):
            _check(self.lib.pyn_ho3_geometry(self.h, info))
        return dict(zip(("affine", "diag", "matfree_diag"), (int(v) for v in info)))

    def mesh_ho_lattice(self):
        """(ngl, nx, ny, nz) when the mesh is a box lattice of order ngl >= 4 that the matrix-free KLE operator accepts
        (mesh_topology() says 'general' for these), (0, 0, 0, 0) otherwise"""
        g, a, b, c = _I(0), _I(0), _I(0), _I(0)
        _check(self.lib.pyn_mesh_ho_lattice(self.h, C.byref(g), C.byref(a), C.byref(b), C.byref(c)))
        return g.value, a.value, b.value, c.value

    def matfree_apply(self, x, y, op=1):
        """y = A x without an assembled matrix (op: MATFREE_LAPLACE scalar, structured Q1 hex meshes; MATFREE_KLE dim DOFs per
        node: structured Q1 hex meshes, second-order lattices of affine cells, box lattices of affine cells of order ngl 4..12
        in 2-D / 4..8 in 3-D; MATFREE_KLE_GENERAL the same K on any quadrilateral / hexahedral mesh of those orders, one rank;
        MATFREE_KLE_NGL3_GENERAL the same K on any quadrilateral / hexahedral mesh of order ngl 3 -- bent cells, imported meshes --
        on one rank)"""
        _check(self.lib.pyn_matfree_apply(self.h, op, x, y))

    def matfree_set(self, op=1, alpha_d=0.0, alpha_w=0.0):
        """define the matrix-free operator (a MATFREE_* id; each id keeps its own snapshot) from the mesh, the tables and a snapshot
        of the CURRENT Dirichlet mask"""
        _check(self.lib.pyn_matfree_set(self.h, op, alpha_d, alpha_w))

    def matfree_kle_set(self, alpha_d, alpha_w):
        self.matfree_set(MATFREE_KLE, alpha_d, alpha_w)

    def solve(self, mid, b, x, method=KSP_CG, pc=PC_JACOBI, rtol=1e-5, atol=1e-50, dtol=1e5, maxit=10000,
              restart=30, norm_type=NORM_PRECONDITIONED, fixed_iters=0, profile=0, cg_variant=0, gmres_orthog=0,
              matfree=0) -> SolveInfo:
        o = SolveOpts(method, pc, norm_type, maxit, restart, fixed_iters, profile, cg_variant, gmres_orthog, matfree,
                      rtol, atol, dtol)
        info = SolveInfo()
        _check(self.lib.pyn_solve(self.h, mid, b, x, C.byref(o), C.byref(info)))
        return info

    def direct_max_rows(self):
        return int(self.lib.pyn_direct_max_rows())

    def solve_direct(self, mid, b, x) -> SolveInfo:
        """dense LU with partial pivoting (small systems, one rank); the factors stay cached until the matrix changes"""
        info = SolveInfo()
        _check(self.lib.pyn_solve_direct(self.h, mid, b, x, C.byref(info)))
        return info

    def direct_band_info(self, mid):
        """(kl, ku, bytes): half-bandwidths of the matrix in the current numbering and the bytes of its banded LU factors"""
        kl, ku, nb = _L(0), _L(0), _L(0)
        _check(self.lib.pyn_direct_band_info(self.h, mid, C.byref(kl), C.byref(ku), C.byref(nb)))
        return kl.value, ku.value, nb.value

    def solve_direct_band(self, mid, b, x, max_bytes=16 << 30) -> SolveInfo:
        """banded LU with partial pivoting (one rank, factors of at most max_bytes); cached until the matrix changes"""
        info = SolveInfo()
        _check(self.lib.pyn_solve_direct_band(self.h, mid, b, x, int(max_bytes), C.byref(info)))
        return info

    def mg_setup(self, mid, max_levels=0, smooth_degree=0, coarse_max_rows=0, esteig_its=0, esteig_min=0.0, esteig_max=0.0):
        """geometric multigrid hierarchy of the matrix (PC_MG; lattice meshes of kinds 1, 2, 3 and box lattices of order ngl >= 4);
        rebuilt only when the options or the values changed.  0 = default"""
        o = MgOpts(max_levels, smooth_degree, coarse_max_rows, esteig_its, esteig_min, esteig_max)
        _check(self.lib.pyn_mg_setup(self.h, mid, C.byref(o)))

    def mg_info(self, mid):
        """{'levels', 'rows' (per level), 'lambda' (lambda_max(D^-1 A) estimate per smoothed level), 'setup_ms', 'builds'}"""
        n, ms, nb = _I(0), _D(0), _I(0)
        rows, lam = np.zeros(MG_MAX_LEVELS, np.int64), np.zeros(MG_MAX_LEVELS)
        _check(self.lib.pyn_mg_info(self.h, mid, C.byref(n), rows, lam, C.byref(ms), C.byref(nb)))
        k = n.value
        return {"levels": k, "rows": [int(r) for r in rows[:k]], "lambda": [float(v) for v in lam[:k]], "setup_ms": ms.value,
                "builds": nb.value}

    def mg_apply(self, mid, r, z):
        """z = M^-1 r: one V-cycle (assembled matrix at level 0)"""
        _check(self.lib.pyn_mg_apply(self.h, mid, r, z))

    def mg_level_get(self, mid, level, b):
        """stencil of coarse level `level`: [node][3^dim][b][b] (nodes lexicographic, offsets x fastest)"""
        rows = self.mg_info(mid)["rows"][level]
        out = np.empty(rows * 3 ** self.dim * b)
        _check(self.lib.pyn_mg_level_get(self.h, mid, level, out))
        return out.reshape(rows // b, 3 ** self.dim, b, b)

    # -- immersed boundary
    def ibm_set(self, kernel, X, dl, lower, h):
        """marker set X [n, dim] with weights dl [n] on the uniform node lattice lower + i h: stencils, node-major spreading lists,
        A = H S and its LU factors for this position (kernel 0: 4-point delta, 1: 3-point)"""
        X = _f64(X)
        dim = self.dim
        if X.ndim == 1:
            X = X.reshape(-1, dim) if dim else X.reshape(0, 1)
        dl, lower, h = _f64(dl).ravel(), _f64(lower).ravel(), _f64(h).ravel()
        n = X.shape[0]
        if dl.size != n or lower.size != dim or h.size != dim or (n and X.shape[1] != dim):
            raise PynamaHipError(f"ibm_set: X {X.shape}, dl {dl.shape}, lower {lower.shape}, h {h.shape} do not fit {n} markers in {dim}-D")
        pad = np.zeros(1)
        _check(self.lib.pyn_ibm_set(self.h, int(kernel), dim, n, X if n else pad, dl if n else pad, lower, h))

    def _ibm_count(self):
        return int(self.ibm_info()["markers"])

    def ibm_interp(self, u):
        """H u at the markers, [n, dim]"""
        out = np.empty((self._ibm_count(), self.dim))
        _check(self.lib.pyn_ibm_interp(self.h, u, out))
        return out

    def ibm_spread(self, q, u):
        """u += S q, q [n, dim]"""
        q = _f64(q)
        n = self._ibm_count()
        if q.size != n * self.dim:
            raise PynamaHipError(f"ibm_spread: q has {q.size} entries, the marker set needs {n} x {self.dim}")
        _check(self.lib.pyn_ibm_spread(self.h, q, u))

    def ibm_correct(self, u, ub):
        """solve A q = ub - H u per component and u += S q on the device; returns q [n, dim]"""
        ub = _f64(ub)
        n = self._ibm_count()
        if ub.size != n * self.dim:
            raise PynamaHipError(f"ibm_correct: ub has {ub.size} entries, the marker set needs {n} x {self.dim}")
        q = np.empty((n, self.dim))
        _check(self.lib.pyn_ibm_correct(self.h, u, ub, q))
        return q

    def ibm_matrix(self):
        """A = H S, [n, n]"""
        n = self._ibm_count()
        A = np.empty((n, n))
        _check(self.lib.pyn_ibm_matrix_get(self.h, A))
        return A

    def ibm_info(self):
        """{'markers', 'width' (stencil lines per axis), 'affected_nodes', 'builds'}"""
        info = np.zeros(4, np.int64)
        _check(self.lib.pyn_ibm_info(self.h, info))
        return {"markers": int(info[0]), "width": int(info[1]), "affected_nodes": int(info[2]), "builds": int(info[3])}

    def ibm_clear(self):
        _check(self.lib.pyn_ibm_clear(self.h))

    # -- point probes
    def probe_create(self, X) -> int:
        """locates the points X [n, dim] in the mesh on the device (pyn_probe_create); the id dies with the mesh"""
        X = _f64(X)
        dim = self.dim
        if X.ndim == 1 and dim:
            X = X.reshape(-1, dim)
        if X.ndim != 2 or (X.shape[0] and X.shape[1] != dim):
            raise PynamaHipError(f"probe_create: points {X.shape} are not [n, {dim}]")
        i = _I(-1)
        _check(self.lib.pyn_probe_create(self.h, X.shape[0], X if X.size else np.zeros(1), C.byref(i)))
        return i.value

    def probe_info(self, pid):
        """{'n', 'found', 'path' (0 rectilinear, 1 search), 'max_newton', 'max_candidates'}"""
        info = np.zeros(5, np.int64)
        _check(self.lib.pyn_probe_info(self.h, int(pid), info))
        return dict(zip(("n", "found", "path", "max_newton", "max_candidates"), (int(v) for v in info)))

    def probe_get(self, pid):
        """(cell [n] int32, -1 where the point is in no cell; xi [n, dim], NaN there)"""
        n = self.probe_info(pid)["n"]
        cell, xi = np.empty(n, np.int32), np.empty((n, self.dim))
        _check(self.lib.pyn_probe_get(self.h, int(pid), cell, xi))
        return cell, xi

    def probe_sample(self, pid, vid, bs=None):
        """the vector's interpolant at the points, [n, bs] (NaN where a point was not found); bs: the vector's block size (known for
        vectors of vec_create)"""
        if bs is None:
            bs = self._vec_bs.get(vid)
            if bs is None:
                raise PynamaHipError(f"probe_sample: the block size of vector {vid} is not known here, pass bs")
        elif self._vec_bs.get(vid, bs) != bs:
            raise PynamaHipError(f"probe_sample: vector {vid} has block size {self._vec_bs[vid]}, not {bs}")
        out = np.empty((self.probe_info(pid)["n"], int(bs)))
        _check(self.lib.pyn_probe_sample(self.h, int(pid), int(vid), out))
        return out

    def probe_destroy(self, pid):
        if self.h:
            _check(self.lib.pyn_probe_destroy(self.h, int(pid)))

    # -- mesh integrals
    def integrate(self, vec_a, vec_b=None, rule=RULE_GAUSS, grad=False):
        """the moments of u = vec_a (- vec_b) over the mesh (pyn_integrate), flat: volume, value[bs], square[bs] and, with grad,
        grad2[bs] and, for bs == dim, div2, curl2[dim_w]; pynama_amd.domain.integrals.Moments names them"""
        out, n = np.zeros(24), _I(0)
        _check(self.lib.pyn_integrate(self.h, int(rule), 1 if grad else 0, int(vec_a), -1 if vec_b is None else int(vec_b), out, C.byref(n)))
        return out[:n.value].copy()

    def timers(self):
        t = np.zeros(8)
        _check(self.lib.pyn_timers_get(self.h, t, 8))
        return {"symbolic_ms": t[0], "assemble_ms": t[1], "spmv_ms": t[2], "solve_ms": t[3], "integrate_ms": t[4]}
