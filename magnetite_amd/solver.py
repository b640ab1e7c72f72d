"""Host-side mirror of Magnetite's solver interface over the C ABI.

Same names, argument meaning and error behaviour as the reference:
  datatypes.rs:1-29   Vertex, Node, Element, ModelMetadata
  error.rs:3-22       MagnetiteError, displayed as "<Kind> error: <msg>"
  solver.rs:543-547   run(nodes, elements, model_metadata) mutates in place; afterwards every
                      node.ux/uy/fx/fy and element.stress is set (solver.rs:476-482,532-533)
  solver.rs:17-19     DOF, MAX_CG_ITER, TARGET_CG_COST
  solver.rs:187-193   compute_element_area (pub; the mesher imports it)

The arithmetic happens in libmagnetite_hip.so (hand-written HIP for gfx950); this module only
flattens the AoS-with-Options model into the SoA arrays of include/magnetite_hip.h and back.
The C++ twin for compiled callers is include/magnetite_solver.hpp; the Rust shim is in INTEGRATION.md.
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _lib
from ._lib import (MAG_ERR_NOT_CONVERGED, MAG_MEM_HOST, MAG_OK, MAG_OP_CSR, MAG_OP_MATRIX_FREE, MAG_STOP_REL,
                   MAG_STOP_RNORM, MAG_STOP_RNORM_SQ)

DOF = 2
MAX_CG_ITER = int(1e7)
TARGET_CG_COST = 1e-4


class MagnetiteError(Exception):
    """error.rs:3-22"""

    def __init__(self, kind, message, code=None):
        super().__init__(f"{kind} error: {message}")
        self.kind, self.message, self.code = kind, message, code


@dataclass
class Vertex:
    x: float
    y: float


@dataclass
class Node:
    vertex: Vertex
    ux: Optional[float] = None
    uy: Optional[float] = None
    fx: Optional[float] = 0.0  # mesher.rs:615-624 defaults
    fy: Optional[float] = 0.0


@dataclass
class Element:
    nodes: List[int]
    stress: Optional[float] = None


@dataclass
class ModelMetadata:
    youngs_modulus: float
    poisson_ratio: float
    part_thickness: float
    characteristic_length_min: float = 0.0
    characteristic_length_max: float = 0.0


def compute_element_area(element, nodes):
    """solver.rs:187-193 (signed)."""
    xy = np.array([[nodes[i].vertex.x, nodes[i].vertex.y] for i in element.nodes], dtype=np.float64).reshape(-1)
    tri = np.arange(3, dtype=np.int32)
    return _lib.lib().mag_compute_element_area(xy.ctypes.data_as(C.POINTER(C.c_double)),
                                               tri.ctypes.data_as(C.POINTER(C.c_int32)))


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Context:
    """Owns one mag_ctx (one GPU, one stream)."""

    def __init__(self, **opts):
        L = _lib.lib()
        o = _lib.Options()
        L.mag_default_options(C.byref(o))
        known = {name for name, _ in _lib.Options._fields_}
        for k, v in opts.items():
            if k not in known:  # (setattr on a ctypes structure takes any name: only mag_options' own fields are options)
                raise TypeError(f"unknown option {k}")
            setattr(o, k, v)
        self.options = o
        self._L = L
        self._h = L.mag_create(C.byref(o))
        if not self._h:
            raise MagnetiteError("Solver", "mag_create returned NULL")
        self._keep = None
        self.N = self.E = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.mag_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, allow=()):
        if rc != MAG_OK and rc not in allow:
            raise MagnetiteError("Solver", self._L.mag_last_error(self._h).decode(), rc)
        return rc

    # -- multi-GPU: one process per GPU ------------------------------------------
    def init_rccl_from_torch(self, dist, rank, world):
        """RCCL communicator for the library's own stream; torch.distributed only carries the 128-byte id."""
        import torch
        ident = (C.c_uint8 * _lib.MAG_UNIQUE_ID_BYTES)()
        if rank == 0:
            rc = self._L.mag_comm_get_unique_id(C.cast(ident, C.c_void_p))
            if rc != MAG_OK:
                raise MagnetiteError("Solver", "mag_comm_get_unique_id failed (librccl not loadable?)", rc)
        t = torch.tensor(list(bytes(ident)), dtype=torch.uint8, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.broadcast(t, src=0)
        raw = bytes(t.cpu().tolist())
        buf = (C.c_uint8 * _lib.MAG_UNIQUE_ID_BYTES).from_buffer_copy(raw)
        self._check(self._L.mag_comm_init_rccl(self._h, C.cast(buf, C.c_void_p), world, rank))

    def comm_info(self):
        """dict(ranks, rank, transport, rccl_ranks) of the context's communicator (mag_comm_query)."""
        info = (C.c_int32 * 4)()
        self._check(self._L.mag_comm_query(self._h, info))
        return dict(ranks=info[0], rank=info[1], transport={0: "none", 1: "rccl", 2: "callback"}[info[2]],
                    rccl_ranks=info[3])

    def set_window(self, shm):
        """Multi-GPU on-chip CG: `shm` is a multiprocessing.shared_memory.SharedMemory (or None to remove the window)
        that EVERY rank of the node has opened under the same name; see mag_comm_set_window in the header."""
        if shm is None:
            self._check(self._L.mag_comm_set_window(self._h, None, 0))
            self._window = None
            return
        addr = C.addressof(C.c_uint8.from_buffer(shm.buf))  # the temporary export ends here: shm.close() stays possible
        self._check(self._L.mag_comm_set_window(self._h, C.c_void_p(addr), shm.size))
        self._window = shm  # keep the mapping alive as long as the library uses it

    def create_inbox(self, nbytes=8 << 20):
        """Multi-GPU on-chip CG, peer-memory form: allocates this rank's inbox in device memory and returns its HIP IPC
        handle (bytes); exchange the handles of all ranks and pass them, in rank order, to open_inboxes()."""
        h = (C.c_uint8 * _lib.MAG_IPC_HANDLE_BYTES)()
        self._check(self._L.mag_comm_inbox_create(self._h, nbytes, C.cast(h, C.c_void_p)))
        return bytes(h)

    def open_inboxes(self, handles):
        raw = b"".join(handles)
        buf = (C.c_uint8 * len(raw)).from_buffer_copy(raw)
        self._check(self._L.mag_comm_inbox_open(self._h, C.cast(buf, C.c_void_p)))

    def close_inboxes(self):
        self._check(self._L.mag_comm_inbox_create(self._h, 0, None))

    def init_callback(self, fn, rank, world):
        """Test transport: fn(numpy_view) must sum the array over ranks in place (e.g. gloo all_reduce)."""
        import numpy as _np

        def _cb(user, ptr, count):
            try:
                fn(_np.ctypeslib.as_array(ptr, shape=(count,)))
                return 0
            except Exception as exc:  # pragma: no cover - surfaced as MAG_ERR_RCCL
                print("allreduce callback failed:", exc, flush=True)
                return 1

        self._cb = _lib.ALLREDUCE_FN(_cb)  # keep alive
        self._check(self._L.mag_comm_init_callback(self._h, world, rank, self._cb, None))

    # -- problem ---------------------------------------------------------------
    def upload(self, xy, conn, u_known, u_in, f_in, youngs_modulus, poisson_ratio, part_thickness):
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
        conn = np.ascontiguousarray(conn, dtype=np.int32).reshape(-1)
        u_known = np.ascontiguousarray(u_known, dtype=np.uint8).reshape(-1)
        u_in = np.ascontiguousarray(u_in, dtype=np.float64).reshape(-1)
        f_in = np.ascontiguousarray(f_in, dtype=np.float64).reshape(-1)
        N, E = xy.size // 2, conn.size // 3
        if not (u_known.size == u_in.size == f_in.size == 2 * N) or xy.size != 2 * N or conn.size != 3 * E:
            raise MagnetiteError("Solver", "array sizes do not match num_nodes/num_elements")
        p = _lib.Problem(N, E, xy.ctypes.data, conn.ctypes.data, u_known.ctypes.data, u_in.ctypes.data,
                         f_in.ctypes.data, float(youngs_modulus), float(poisson_ratio), float(part_thickness),
                         MAG_MEM_HOST, 0)
        self._check(self._L.mag_upload(self._h, C.byref(p)))
        self.N, self.E = N, E

    def upload_problem(self, prob):
        """prob: magnetite_amd.meshgen.Problem"""
        self.upload(prob.xy_flat, prob.conn_flat, prob.u_known, prob.u_in, prob.f_in, prob.youngs_modulus,
                    prob.poisson_ratio, prob.part_thickness)

    def run(self, allow_not_converged=False):
        """mag_run.  Stopping at the iteration cap is a normal termination, as in the reference (solver.rs:149-176
        returns Ok(best_param)): no error, stats()["converged"] == 0, the best iterate is returned.
        allow_not_converged only tolerates a numerical breakdown (MAG_ERR_NOT_CONVERGED: non-finite residual)."""
        allow = (MAG_ERR_NOT_CONVERGED,) if allow_not_converged else ()
        return self._check(self._L.mag_run(self._h), allow)

    def download(self):
        u, f, s = np.empty(2 * self.N), np.empty(2 * self.N), np.empty(self.E)
        r = _lib.Result(u.ctypes.data, f.ctypes.data, s.ctypes.data, MAG_MEM_HOST, 0)
        self._check(self._L.mag_download(self._h, C.byref(r)))
        return u, f, s

    def stats(self):
        st = _lib.Stats()
        self._L.mag_get_stats(self._h, C.byref(st))
        return st.as_dict()

    def history(self, n):
        h = np.empty(max(n, 1))
        self._check(self._L.mag_get_history(self._h, _p(h, C.c_double), n))
        return h[:n]

    def solve(self, prob, allow_not_converged=False):
        """mag_solve on a meshgen.Problem: dict(u, f, stress, **stats)."""
        self.upload_problem(prob)
        self.run(allow_not_converged)
        u, f, s = self.download()
        out = dict(u=u, f=f, stress=s)
        out.update(self.stats())
        return out

    # -- member sets (load cases, design variants): what their getters share ------
    def _download_at(self, fn, i):
        u, f, s = np.empty(2 * self.N), np.empty(2 * self.N), np.empty(self.E)
        r = _lib.Result(u.ctypes.data, f.ctypes.data, s.ctypes.data, MAG_MEM_HOST, 0)
        self._check(fn(self._h, i, C.byref(r)))
        return u, f, s

    def _stats_at(self, fn, i):
        st = _lib.Stats()
        self._check(fn(self._h, i, C.byref(st)))
        return st.as_dict()

    def _info(self, fn, keys):
        info = (C.c_int32 * 4)()
        self._check(fn(self._h, info))
        return dict(zip(keys, info))

    def _collect(self, n, download, stats):
        """A list of dicts shaped like solve()'s, one per member."""
        outs = []
        for i in range(n):
            u, f, s = download(i)
            outs.append(dict(u=u, f=f, stress=s, **stats(i)))
        return outs

    # -- load cases: several sets of prescribed values on the uploaded mesh ------
    def set_load_cases(self, u_in, f_in):
        """mag_set_load_cases: u_in, f_in of shape (L, 2N) -- prescribed displacements / forces per case, read where the
        uploaded u_known mask says so."""
        u_in = np.ascontiguousarray(u_in, dtype=np.float64)
        f_in = np.ascontiguousarray(f_in, dtype=np.float64)
        if u_in.ndim != 2 or u_in.shape != f_in.shape or u_in.shape[1] != 2 * self.N:
            raise MagnetiteError("Solver", "load cases: u_in and f_in must both have shape (num_cases, 2 * num_nodes)")
        self._check(self._L.mag_set_load_cases(self._h, u_in.shape[0], _p(u_in, C.c_double), _p(f_in, C.c_double),
                                               MAG_MEM_HOST))
        self.num_cases = u_in.shape[0]

    def run_cases(self, allow_not_converged=False):
        """mag_run_cases: order, symbolic work and K once, the cases' CG solves side by side on the chip where they fit."""
        allow = (MAG_ERR_NOT_CONVERGED,) if allow_not_converged else ()
        return self._check(self._L.mag_run_cases(self._h), allow)

    def download_case(self, i):
        return self._download_at(self._L.mag_download_case, i)

    def case_stats(self, i):
        return self._stats_at(self._L.mag_get_case_stats, i)

    def cases_info(self):
        """dict(cases, cases_per_launch (0: one after another through the single-case CG phases), launches, redone)."""
        return self._info(self._L.mag_get_cases_info, ("cases", "cases_per_launch", "launches", "redone"))

    def solve_cases(self, prob, u_in, f_in, allow_not_converged=False):
        """Upload prob's mesh, material and mask, solve the (L, 2N) load sets: a list of dicts shaped like solve()'s."""
        self.upload_problem(prob)
        self.set_load_cases(u_in, f_in)
        self.run_cases(allow_not_converged)
        return self._collect(self.num_cases, self.download_case, self.case_stats)

    # -- design variants: several shapes / materials / value sets of the uploaded mesh ------
    def set_variants(self, xy=None, material=None, u_in=None, f_in=None):
        """mag_set_variants: xy (V, 2N) or (V, N, 2), material (V, 3) = E, nu, thickness, u_in / f_in (V, 2N) -- each optional
        (None: every variant keeps what was uploaded), at least one given, all with the same V."""
        N = self.N

        def arr(a, width, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.ndim == 3 and what == "xy":
                a = a.reshape(a.shape[0], -1)
            if a.ndim != 2 or a.shape[1] != width:
                raise MagnetiteError("Solver", f"variants: {what} must have shape (num_variants, {width})")
            return a

        xy, material = arr(xy, 2 * N, "xy"), arr(material, 3, "material")
        u_in, f_in = arr(u_in, 2 * N, "u_in"), arr(f_in, 2 * N, "f_in")
        if (u_in is None) != (f_in is None):
            raise MagnetiteError("Solver", "variants: u_in and f_in come together")
        given = [a for a in (xy, material, u_in, f_in) if a is not None]
        if len({a.shape[0] for a in given}) > 1:
            raise MagnetiteError("Solver", "variants: xy, material, u_in and f_in must agree on num_variants")
        V = given[0].shape[0] if given else 1  # (nothing given: the library answers)
        ptr = lambda a: None if a is None else _p(a, C.c_double)
        self._check(self._L.mag_set_variants(self._h, V, ptr(xy), ptr(material), ptr(u_in), ptr(f_in), MAG_MEM_HOST))
        self.num_variants = V

    def run_variants(self, allow_not_converged=False):
        """mag_run_variants: order, tables and CSR pattern once; per variant coordinates, K, right-hand side, blocks, CG, post --
        the CG solves side by side on the chip where they fit."""
        allow = (MAG_ERR_NOT_CONVERGED,) if allow_not_converged else ()
        return self._check(self._L.mag_run_variants(self._h), allow)

    def download_variant(self, i):
        return self._download_at(self._L.mag_download_variant, i)

    def variant_stats(self, i):
        return self._stats_at(self._L.mag_get_variant_stats, i)

    def variants_info(self):
        """dict(variants, variants_per_launch (0: one after another through the single-case phases), launches, redone)."""
        return self._info(self._L.mag_get_variants_info, ("variants", "variants_per_launch", "launches", "redone"))

    def solve_variants(self, prob, xy=None, material=None, u_in=None, f_in=None, allow_not_converged=False):
        """Upload prob (its coordinates give the ordering every variant shares), solve the variants: a list of dicts shaped
        like solve()'s."""
        self.upload_problem(prob)
        self.set_variants(xy, material, u_in, f_in)
        self.run_variants(allow_not_converged)
        return self._collect(self.num_variants, self.download_variant, self.variant_stats)

    def assemble_csr_variant(self, i):
        """K of variant i in the uploaded mesh's pattern (test entry point mag_assemble_csr_variant)."""
        nnz = C.c_int64(0)
        self._check(self._L.mag_assemble_csr_variant(self._h, i, C.byref(nnz), None, None, None))
        rowptr = np.empty(2 * self.N + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value)
        self._check(self._L.mag_assemble_csr_variant(self._h, i, C.byref(nnz), _p(rowptr, C.c_int32), _p(col, C.c_int32),
                                                     _p(val, C.c_double)))
        return rowptr, col, val

    # -- energy and design sensitivities of the solved members of a set ------------
    SENSITIVITY_SETS = {"run": _lib.MAG_SET_RUN, "cases": _lib.MAG_SET_CASES, "variants": _lib.MAG_SET_VARIANTS}
    SENSITIVITY_SCALARS = ("strain_energy", "potential_energy", "external_work", "reaction_work", "dPi_dE", "dPi_dnu",
                           "dPi_dt")

    def _sensitivity_set(self, set):
        if set not in self.SENSITIVITY_SETS:
            raise MagnetiteError("Solver", f"sensitivities: set must be one of {sorted(self.SENSITIVITY_SETS)}")
        return self.SENSITIVITY_SETS[set]

    def run_sensitivities(self, set="run"):
        """mag_run_sensitivities on the last completed run() / run_cases() / run_variants(): solves nothing."""
        self._check(self._L.mag_run_sensitivities(self._h, self._sensitivity_set(set)))

    def download_sensitivity(self, set, i):
        """dict(energy (E), dxy (2N), strain_energy, potential_energy, external_work, reaction_work, dPi_dE, dPi_dnu, dPi_dt)
        of member i of the set."""
        which = self._sensitivity_set(set)
        energy, dxy = np.empty(self.E), np.empty(2 * self.N)
        o = _lib.Sensitivity(energy.ctypes.data, dxy.ctypes.data, (C.c_double * 8)(), MAG_MEM_HOST, 0)
        self._check(self._L.mag_download_sensitivity(self._h, which, i, C.byref(o)))
        return dict(energy=energy, dxy=dxy, **dict(zip(self.SENSITIVITY_SCALARS, o.scalars)))

    def sensitivities(self, set="run"):
        """Energy and design gradient of every solved member of the set ("run": the one of run(); "cases"; "variants"): a list
        of dicts as download_sensitivity returns them.  dxy, dPi_dE, dPi_dnu, dPi_dt are the total derivatives of the potential
        energy with respect to the node coordinates and the material (include/magnetite_hip.h)."""
        self.run_sensitivities(set)
        n = 1 if set == "run" else (self.num_cases if set == "cases" else self.num_variants)
        return [self.download_sensitivity(set, i) for i in range(n)]

    # -- adjoint sensitivities: the gradient of any objective of the solved members of a set ------------
    ADJOINT_SCALARS = ("a", "dJ_dE", "dJ_dnu", "dJ_dt")

    def _members(self, set):
        """Members of the set; 0 where none was given yet (the library then answers with its state error)."""
        return 1 if set == "run" else getattr(self, "num_cases" if set == "cases" else "num_variants", 0)

    def run_adjoint(self, dJ_du, set="run", allow_not_converged=False):
        """mag_run_adjoint on the last completed run() / run_cases() / run_variants(): dJ_du of shape (members, 2N), or (2N,)
        for "run" -- one adjoint solve per member with its own K, then the bilinear pass."""
        which = self._sensitivity_set(set)
        g = np.ascontiguousarray(dJ_du, dtype=np.float64)
        if set == "run" and g.ndim == 1:
            g = g.reshape(1, -1)
        members = self._members(set)
        if g.ndim != 2 or (self.N and g.shape[1] != 2 * self.N) or (members and g.shape[0] != members):
            raise MagnetiteError("Solver", "adjoint: dJ_du must have shape (members of the set, 2 * num_nodes)")
        allow = (MAG_ERR_NOT_CONVERGED,) if allow_not_converged else ()
        return self._check(self._L.mag_run_adjoint(self._h, which, _p(g, C.c_double), MAG_MEM_HOST), allow)

    def download_adjoint(self, set, i):
        """dict(lambda (2N), dloads (2N), delem (E), dxy (2N), a, dJ_dE, dJ_dnu, dJ_dt) of member i of the set."""
        which = self._sensitivity_set(set)
        lam, dloads, delem, dxy = np.empty(2 * self.N), np.empty(2 * self.N), np.empty(self.E), np.empty(2 * self.N)
        o = _lib.Adjoint(lam.ctypes.data, dloads.ctypes.data, delem.ctypes.data, dxy.ctypes.data, (C.c_double * 8)(), MAG_MEM_HOST, 0)
        self._check(self._L.mag_download_adjoint(self._h, which, i, C.byref(o)))
        out = {"lambda": lam, "dloads": dloads, "delem": delem, "dxy": dxy}
        out.update(zip(self.ADJOINT_SCALARS, o.scalars))
        return out

    def adjoint_stats(self, set, i):
        """The statistics of member i's adjoint solve (mag_get_adjoint_stats)."""
        st = _lib.Stats()
        self._check(self._L.mag_get_adjoint_stats(self._h, self._sensitivity_set(set), i, C.byref(st)))
        return st.as_dict()

    def adjoint_info(self, set):
        """mag_get_adjoint_info: the four words of cases_info() for the adjoint solves of the set, as a list."""
        info = (C.c_int32 * 4)()
        self._check(self._L.mag_get_adjoint_info(self._h, self._sensitivity_set(set), info))
        return list(info)

    def adjoint(self, dJ_du, set="run", allow_not_converged=False):
        """The gradient of an objective J of every solved member of the set, given dJ/du at the member's u: a list of dicts as
        download_adjoint returns them.  dxy, dJ_dE, dJ_dnu, dJ_dt, delem and dloads are total derivatives at fixed prescribed
        values, without J's explicit dependence on the design (include/magnetite_hip.h)."""
        self.run_adjoint(dJ_du, set, allow_not_converged)
        return [self.download_adjoint(set, i) for i in range(self._members(set))]

    # -- objectives on the device: J, dJ/du, explicit partials and, through the adjoint, the total design gradient ------------
    OBJECTIVE_KINDS = {"disp_lsq": _lib.MAG_OBJ_DISP_LSQ, "stress_pnorm": _lib.MAG_OBJ_STRESS_PNORM}
    OBJECTIVE_SCALARS = ("J", "pJ_pE", "pJ_pnu", "pJ_pt", "dJ_dE", "dJ_dnu", "dJ_dt")

    def run_objective(self, kind, set="run", weights=None, target=None, p=8.0, scale=1.0, adjoint=False, allow_not_converged=False):
        """mag_run_objective on the last completed run() / run_cases() / run_variants().  kind: "disp_lsq" (weights (2N,) or
        (members, 2N), target likewise or None) or "stress_pnorm" (weights (E,) or (members, E) or None, p, scale)."""
        which = self._sensitivity_set(set)
        if kind not in self.OBJECTIVE_KINDS:
            raise MagnetiteError("Solver", f"objective: kind must be one of {sorted(self.OBJECTIVE_KINDS)}")
        width = 2 * self.N if kind == "disp_lsq" else self.E
        members = self._members(set)

        def rows(a, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.ndim not in (1, 2) or (width and a.shape[-1] != width) or (a.ndim == 2 and members and a.shape[0] != members):
                raise MagnetiteError("Solver", f"objective: {what} must have shape ({width},) or (members of the set, {width})")
            return a

        w, tg = rows(weights, "weights"), rows(target if kind == "disp_lsq" else None, "target")
        given = [a for a in (w, tg) if a is not None]
        if len({a.ndim for a in given}) > 1:
            raise MagnetiteError("Solver", "objective: weights and target are both one row or both a row per member")
        per_member = 1 if given and given[0].ndim == 2 else 0
        ptr = lambda a: None if a is None else a.ctypes.data
        o = _lib.Objective(self.OBJECTIVE_KINDS[kind], per_member, float(p), float(scale), ptr(w), ptr(tg), MAG_MEM_HOST, 0)
        allow = (MAG_ERR_NOT_CONVERGED,) if allow_not_converged else ()
        return self._check(self._L.mag_run_objective(self._h, which, C.byref(o), 1 if adjoint else 0), allow)

    def download_objective(self, set, i, total=False):
        """dict(J, g (2N), pxy (2N), pJ_pE, pJ_pnu, pJ_pt: the explicit partials) of member i of the set; with total (the
        objective ran with adjoint=True) also dxy (2N), dJ_dE, dJ_dnu, dJ_dt: the total derivatives."""
        which = self._sensitivity_set(set)
        g, pxy, dxy = np.empty(2 * self.N), np.empty(2 * self.N), np.empty(2 * self.N) if total else None
        o = _lib.ObjectiveResult(g.ctypes.data, pxy.ctypes.data, dxy.ctypes.data if total else None, (C.c_double * 8)(), MAG_MEM_HOST, 0)
        self._check(self._L.mag_download_objective(self._h, which, i, C.byref(o)))
        out = dict(g=g, pxy=pxy)
        out.update(zip(self.OBJECTIVE_SCALARS[:4], o.scalars))
        if total:
            out["dxy"] = dxy
            out.update(zip(self.OBJECTIVE_SCALARS[4:], o.scalars[4:7]))
        return out

    def objective(self, kind, set="run", weights=None, target=None, p=8.0, scale=1.0, adjoint=False, allow_not_converged=False):
        """An objective of every solved member of the set, evaluated on the device: a list of dicts as download_objective
        returns them.  adjoint=True also runs the adjoint pass on the device-resident dJ/du (its results are then those of
        adjoint(g, set)) and returns the total derivatives (include/magnetite_hip.h)."""
        self.run_objective(kind, set, weights, target, p, scale, adjoint, allow_not_converged)
        return [self.download_objective(set, i, total=adjoint) for i in range(self._members(set))]

    # -- stress recovery: the tensor per element, the nodal field and the ZZ error estimate of the solved members of a set ---
    STRESS_SCALARS = ("eta", "energy_norm", "eta_rel", "vm_max", "vm_node_max")

    def run_stress(self, set="run"):
        """mag_run_stress on the last completed run() / run_cases() / run_variants(): solves nothing."""
        self._check(self._L.mag_run_stress(self._h, self._sensitivity_set(set)))

    def download_stress(self, set, i):
        """dict(elem (E, 4): sx, sy, txy, vm; node (N, 4): the averaged tensor and its vm; eta2 (E); eta, energy_norm: the
        square roots of the library's eta^2 and U^2; eta_rel, vm_max, vm_node_max) of member i of the set."""
        which = self._sensitivity_set(set)
        elem, node, eta2 = np.empty((self.E, 4)), np.empty((self.N, 4)), np.empty(self.E)
        o = _lib.StressField(elem.ctypes.data, node.ctypes.data, eta2.ctypes.data, (C.c_double * 8)(), MAG_MEM_HOST, 0)
        self._check(self._L.mag_download_stress(self._h, which, i, C.byref(o)))
        sc = list(o.scalars)
        return dict(elem=elem, node=node, eta2=eta2, **dict(zip(self.STRESS_SCALARS, [np.sqrt(sc[0]), np.sqrt(sc[1])] + sc[2:5])))

    def stress_recovery(self, set="run"):
        """The stress field of every solved member of the set ("run": the one of run(); "cases"; "variants"): a list of dicts
        as download_stress returns them -- the tensor and von Mises value per element, the area-weighted nodal field, the ZZ
        error indicator eta2 per element with its norm eta, the energy norm of the solution and their ratio eta_rel
        (include/magnetite_hip.h)."""
        self.run_stress(set)
        return [self.download_stress(set, i) for i in range(self._members(set))]

    # -- adaptive mesh refinement: longest-edge bisection with conformity closure of the uploaded mesh -----------------
    REFINE_RULES = {"marks": _lib.MAG_REFINE_MARKS, "max_fraction": _lib.MAG_REFINE_MAX_FRACTION, "top_fraction": _lib.MAG_REFINE_TOP_FRACTION}
    REFINE_INFO = ("nodes", "elements", "marked", "marked_edges", "sweeps", "split2", "split3", "split4")

    def run_refine(self, marks=None, indicator=None, rule="top_fraction", theta=0.2, split=1):
        """mag_run_refine on the uploaded mesh: solves nothing.  marks (E, nonzero: marked) selects rule "marks" whatever
        `rule` says; otherwise `rule` is "top_fraction" or "max_fraction" of `indicator` (E values, finite and >= 0), or of the
        device-resident eta2 of the last run_stress("run") when indicator is None."""
        if marks is not None:
            rule = "marks"
        if rule not in self.REFINE_RULES:
            raise MagnetiteError("Solver", f"refine: rule must be one of {sorted(self.REFINE_RULES)}")
        keep = []
        o = _lib.RefineOptions(self.REFINE_RULES[rule], int(split), float(theta), None, None, MAG_MEM_HOST, 0)
        for name, a, dtype in (("marks", marks, np.uint8), ("indicator", indicator, np.float64)):
            if a is None:
                continue
            a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
            if a.size != self.E:
                raise MagnetiteError("Solver", f"refine: {name} must have num_elements entries")
            keep.append(a)
            setattr(o, name, a.ctypes.data)
        self._check(self._L.mag_run_refine(self._h, C.byref(o)))

    def refine_info(self):
        """dict(nodes, elements: N', E' of the refined mesh; marked: elements marked before the closure; marked_edges = N' - N;
        sweeps of the closure; split2, split3, split4: elements split in two, three, four)."""
        info = (C.c_int64 * 8)()
        self._check(self._L.mag_get_refine_info(self._h, info))
        return dict(zip(self.REFINE_INFO, info))

    def download_refine(self):
        """dict(xy (N', 2), conn (E', 3), u_known, u_in, f_in (2N'), node_parents (N' - N, 2): lo, hi of the edge a new node
        halves; elem_parent (E')) of the last run_refine()."""
        info = self.refine_info()
        Nn, En, added = info["nodes"], info["elements"], info["marked_edges"]
        xy, conn = np.empty((Nn, 2)), np.empty((En, 3), dtype=np.int32)
        known, u_in, f_in = np.empty(2 * Nn, dtype=np.uint8), np.empty(2 * Nn), np.empty(2 * Nn)
        nparents, eparent = np.empty((added, 2), dtype=np.int32), np.empty(En, dtype=np.int32)
        o = _lib.Refined(xy.ctypes.data, conn.ctypes.data, known.ctypes.data, u_in.ctypes.data, f_in.ctypes.data,
                         nparents.ctypes.data if added else None, eparent.ctypes.data, MAG_MEM_HOST, 0)
        self._check(self._L.mag_download_refine(self._h, C.byref(o)))
        return dict(xy=xy, conn=conn, u_known=known, u_in=u_in, f_in=f_in, node_parents=nparents, elem_parent=eparent)

    def upload_refined(self):
        """mag_upload_refined: the refined mesh becomes the uploaded problem, device to device, with the same material -- bit
        for bit download_refine() followed by upload().  Runs, sets and modes are dropped as upload() drops them."""
        info = self.refine_info()
        self._check(self._L.mag_upload_refined(self._h))
        self.N, self.E = info["nodes"], info["elements"]

    def refine(self, marks=None, indicator=None, rule="top_fraction", theta=0.2, split=1):
        """run_refine + download_refine: the arrays of the refined mesh and the words of refine_info() by name."""
        self.run_refine(marks, indicator, rule, theta, split)
        out = self.download_refine()
        out.update(self.refine_info())
        return out

    def adapt(self, prob, rounds=3, theta=0.2, rule="top_fraction", split=1, target_eta_rel=None):
        """The adaptive loop on a meshgen.Problem with the mesh staying on the device: per round solve -> stress_recovery("run")
        -> record -> run_refine on the device's eta2 -> upload_refined; after the last refinement a final solve and recovery.
        Stops early once eta_rel <= target_eta_rel.  Returns dict(history: per solve dict(nodes, elements, eta, eta_rel,
        iterations), rounds + 1 entries unless stopped early; problem: the final mesh and boundary data as a meshgen.Problem;
        result: solve()'s dict for it; recovery: its stress_recovery("run")[0])."""
        from .meshgen import Mesh, Problem
        self.upload_problem(prob)
        history = []
        for r in range(int(rounds) + 1):
            self.run()
            field = self.stress_recovery("run")[0]
            history.append(dict(nodes=self.N, elements=self.E, eta=field["eta"], eta_rel=field["eta_rel"], iterations=self.stats()["iterations"]))
            if r == rounds or (target_eta_rel is not None and field["eta_rel"] <= target_eta_rel):
                break
            self.run_refine(rule=rule, theta=theta, split=split)
            self.upload_refined()
        u, f, s = self.download()
        result = dict(u=u, f=f, stress=s)
        result.update(self.stats())
        if len(history) > 1:
            m = self.download_refine()
            name = getattr(prob.mesh, "name", "mesh") + "_adapted"
            final = Problem(Mesh(m["xy"], m["conn"], name), m["u_known"], m["u_in"], m["f_in"], prob.youngs_modulus,
                            prob.poisson_ratio, prob.part_thickness)
        else:
            final = prob
        return dict(history=history, problem=final, result=result, recovery=field)

    # -- element stiffness field and the density design update on it --------------------------------------------------
    DESIGN_INFO = ("volume_fraction", "lagrange", "change", "greyness", "reachable", "steps", "J")

    def set_element_scale(self, scale):
        """mag_set_element_scale: a relative stiffness scale per element (E values, finite and > 0), K = sum_e s_e K_e; None
        clears the field.  Drops the results of run() and run_cases(); ends a design."""
        if scale is None:
            return self._check(self._L.mag_set_element_scale(self._h, None, MAG_MEM_HOST))
        scale = np.ascontiguousarray(scale, dtype=np.float64).reshape(-1)
        if self.E and scale.size != self.E:
            raise MagnetiteError("Solver", "element scale: num_elements entries are needed")
        return self._check(self._L.mag_set_element_scale(self._h, _p(scale, C.c_double), MAG_MEM_HOST))

    def design_init(self, volume_fraction=0.5, penal=3, scale_min=1e-3, rho_min=1e-3, move=0.2, filter_passes=1, rho0=None):
        """mag_design_init on the uploaded problem: the densities rho0 (E values in (0, 1]; None: volume_fraction everywhere),
        their filtered field and its SIMP scale, installed as the element scale."""
        o = _lib.DesignOptions(float(volume_fraction), float(scale_min), float(rho_min), float(move), int(penal), int(filter_passes))
        if rho0 is not None:
            rho0 = np.ascontiguousarray(rho0, dtype=np.float64).reshape(-1)
            if self.E and rho0.size != self.E:
                raise MagnetiteError("Solver", "design: rho0 needs num_elements entries")
        return self._check(self._L.mag_design_init(self._h, C.byref(o), None if rho0 is None else _p(rho0, C.c_double), MAG_MEM_HOST))

    def design_step(self, dJ_ds=None):
        """mag_design_step after run(): the optimality-criteria update under the volume constraint.  dJ_ds None: the stiffest
        design (J = -2 Pi) from the device-resident energies of run_sensitivities("run"); otherwise E values dJ/ds_e of any
        objective, e.g. adjoint delem / scale.  Installs the new scale: the next run() solves the updated design."""
        if dJ_ds is not None:
            dJ_ds = np.ascontiguousarray(dJ_ds, dtype=np.float64).reshape(-1)
            if self.E and dJ_ds.size != self.E:
                raise MagnetiteError("Solver", "design: dJ_ds needs num_elements entries")
        return self._check(self._L.mag_design_step(self._h, None if dJ_ds is None else _p(dJ_ds, C.c_double), MAG_MEM_HOST))

    def design_info(self):
        """dict(volume_fraction reached, lagrange: the multiplier L, change: max |rho_new - rho|, greyness: mean(4 rho~ (1 - rho~)),
        reachable: 1 if the volume target lay within the move limits, steps since design_init, J of the step)."""
        info = (C.c_double * 8)()
        self._check(self._L.mag_get_design_info(self._h, info))
        out = dict(zip(self.DESIGN_INFO, info))
        out["reachable"], out["steps"] = int(out["reachable"]), int(out["steps"])
        return out

    def download_design(self):
        """dict(rho, rho_filtered, scale, dJ_drho: E values each) of the design as it stands."""
        rho, rhof, scale, g = (np.empty(self.E) for _ in range(4))
        o = _lib.Design(rho.ctypes.data, rhof.ctypes.data, scale.ctypes.data, g.ctypes.data, MAG_MEM_HOST, 0)
        self._check(self._L.mag_download_design(self._h, C.byref(o)))
        return dict(rho=rho, rho_filtered=rhof, scale=scale, dJ_drho=g)

    def topopt(self, prob, iters=30, volume_fraction=0.5, penal=3, scale_min=1e-3, rho_min=1e-3, move=0.2, filter_passes=1, rho0=None):
        """Density topology optimisation of the stiffest design (J = -2 Pi) on a meshgen.Problem, the design staying on the
        device: upload, design_init, then `iters` times run + run_sensitivities + design_step.  Returns dict(history: per
        iteration dict(J, volume_fraction, change, greyness, reachable, lagrange, iterations, cg_kernel, ms_order,
        ms_csr_symbolic), J being that of the design the iteration SOLVED and the rest of the update that followed; rho,
        rho_filtered, scale: the final design, which no run has solved yet)."""
        self.upload_problem(prob)
        self.design_init(volume_fraction, penal, scale_min, rho_min, move, filter_passes, rho0)
        history = []
        for _ in range(int(iters)):
            self.run()
            st = self.stats()
            self.run_sensitivities("run")
            self.design_step()
            info = self.design_info()
            info.pop("steps")
            history.append(dict(info, **{k: st[k] for k in ("iterations", "cg_kernel", "ms_order", "ms_csr_symbolic")}))
        final = self.download_design()
        return dict(history=history, rho=final["rho"], rho_filtered=final["rho_filtered"], scale=final["scale"])

    # -- modal analysis: the lowest natural frequencies and mode shapes of the uploaded part ------------
    MODAL_INFO =("modes", "subspace", "outer", "converged", "vectors_per_launch", "launches", "redone")

    def run_modal(self, modes=6, density=None, subspace=0, tol=0.0, cg_tol=0.0, max_outer=0, lumped=False, allow_not_converged=False):
        """mag_run_modal on the uploaded problem (no run needed): subspace iteration for the `modes` lowest pairs of
        K_FF phi = lambda M_FF phi, prescribed DOFs as supports.  Reaching max_outer is no error (modal_info()["converged"] == 0)."""
        if density is None:
            raise MagnetiteError("Solver", "modal: a density is needed (the model has none)")
        o = _lib.ModalOptions(int(modes), int(subspace), int(max_outer), 1 if lumped else 0, float(density), float(tol), float(cg_tol))
        allow = (MAG_ERR_NOT_CONVERGED,) if allow_not_converged else ()
        return self._check(self._L.mag_run_modal(self._h, C.byref(o)), allow)

    def modal_info(self):
        """dict(modes, subspace, outer, converged, vectors_per_launch (0: one after another), launches, redone)."""
        info = (C.c_int32 * 8)()
        self._check(self._L.mag_get_modal_info(self._h, info))
        return dict(zip(self.MODAL_INFO, info))

    def modal_stats(self, j):
        """The statistics of inner solve j of the last outer step (mag_get_modal_stats)."""
        return self._stats_at(self._L.mag_get_modal_stats, j)

    def download_modal(self):
        """dict(lambda (p), frequency (p), residual (p), shapes (p, 2N)) of the last run_modal()."""
        p = self.modal_info()["modes"]
        lam, freq, res, shapes = np.empty(p), np.empty(p), np.empty(p), np.empty((p, 2 * self.N))
        o = _lib.ModalResult(lam.ctypes.data, freq.ctypes.data, res.ctypes.data, shapes.ctypes.data, MAG_MEM_HOST, 0)
        self._check(self._L.mag_download_modal(self._h, C.byref(o)))
        return {"lambda": lam, "frequency": freq, "residual": res, "shapes": shapes}

    def modal(self, prob=None, modes=6, density=None, subspace=0, tol=0.0, cg_tol=0.0, max_outer=0, lumped=False):
        """The `modes` lowest natural frequencies (Hz) and mode shapes of prob (uploaded when given; otherwise of what is
        uploaded): dict(lambda, frequency, residual, shapes (modes, 2N), and the words of modal_info() by name).  shapes are
        mass-normalised, phi_k^T M phi_l = delta_kl, and 0 on prescribed DOFs, which act as supports (include/magnetite_hip.h)."""
        if prob is not None:
            self.upload_problem(prob)
        self.run_modal(modes, density, subspace, tol, cg_tol, max_outer, lumped)
        out = self.download_modal()
        out.update(self.modal_info())
        return out

    def apply_mass(self, x, density, lumped=False, masked=False):
        """y = M x with the mass operator of run_modal (test entry point mag_apply_mass)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(2 * self.N)
        self._check(self._L.mag_apply_mass(self._h, float(density), 1 if lumped else 0, _p(x, C.c_double), _p(y, C.c_double),
                                           1 if masked else 0))
        return y

    # -- linearised buckling: the critical load factors and buckling shapes of a solved member ------------
    BUCKLING_INFO = ("modes", "subspace", "outer", "converged", "vectors_per_launch", "launches", "redone", "positive")
    BUCKLING_SETS = {"run": _lib.MAG_SET_RUN, "cases": _lib.MAG_SET_CASES}

    def _prestress(self, what, set, member):
        if set not in self.BUCKLING_SETS:
            raise MagnetiteError("Solver", f"{what}: set must be one of {sorted(self.BUCKLING_SETS)} (the prestress is a solved run or load case)")
        if int(member) != member or member < 0:
            raise MagnetiteError("Solver", f"{what}: member {member!r} is no index of a solved member")
        return self.BUCKLING_SETS[set], int(member)

    def run_buckling(self, modes=4, set="run", member=0, subspace=0, tol=0.0, cg_tol=0.0, max_outer=0, allow_not_converged=False):
        """mag_run_buckling under the prestress of a solved member (the last run(), or case `member` of the last run_cases()):
        the `modes` pairs of smallest |lambda| of (K_FF + lambda K_G,FF) phi = 0.  Reaching max_outer is no error
        (buckling_info()["converged"] == 0)."""
        sid, member = self._prestress("buckling", set, member)
        o = _lib.BucklingOptions(int(modes), int(subspace), int(max_outer), sid, member, 0, float(tol), float(cg_tol))
        allow = (MAG_ERR_NOT_CONVERGED,) if allow_not_converged else ()
        return self._check(self._L.mag_run_buckling(self._h, C.byref(o)), allow)

    def buckling_info(self):
        """dict(modes, subspace, outer, converged, vectors_per_launch (0: one after another), launches, redone, positive)."""
        info = (C.c_int32 * 8)()
        self._check(self._L.mag_get_buckling_info(self._h, info))
        return dict(zip(self.BUCKLING_INFO, info))

    def buckling_stats(self, j):
        """The statistics of inner solve j of the last outer step (mag_get_buckling_stats)."""
        return self._stats_at(self._L.mag_get_buckling_stats, j)

    def download_buckling(self):
        """dict(load_factor (p), residual (p), shapes (p, 2N)) of the last run_buckling()."""
        p = self.buckling_info()["modes"]
        lam, res, shapes = np.empty(p), np.empty(p), np.empty((p, 2 * self.N))
        o = _lib.BucklingResult(lam.ctypes.data, res.ctypes.data, shapes.ctypes.data, MAG_MEM_HOST, 0)
        self._check(self._L.mag_download_buckling(self._h, C.byref(o)))
        return {"load_factor": lam, "residual": res, "shapes": shapes}

    def buckling(self, prob=None, modes=4, set="run", member=0, subspace=0, tol=0.0, cg_tol=0.0, max_outer=0):
        """The `modes` load factors of smallest magnitude, signed and ordered by magnitude, and the buckling shapes under the
        prestress of a solved member (prob, when given, is uploaded and run first): dict(load_factor, residual, shapes (modes,
        2N), critical -- the smallest positive factor, or None -- and the words of buckling_info() by name).  A negative factor
        is buckling under the reversed load.  shapes are K-normalised, phi_k^T K phi_l = delta_kl, and 0 on prescribed DOFs,
        which act as supports (include/magnetite_hip.h)."""
        self._prestress("buckling", set, member)
        if prob is not None:
            self.upload_problem(prob)
            self.run()
        self.run_buckling(modes, set, member, subspace, tol, cg_tol, max_outer)
        out = self.download_buckling()
        out.update(self.buckling_info())
        positive = out["load_factor"][out["load_factor"] > 0.0]
        out["critical"] = float(positive.min()) if positive.size else None
        return out

    def apply_geometric(self, x, set="run", member=0, masked=False):
        """y = K_G(sigma(u0)) x with the geometric stiffness operator of run_buckling, u0 the solution of the solved member
        (test entry point mag_apply_geometric)."""
        sid, member = self._prestress("apply_geometric", set, member)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        if x.size != 2 * self.N:
            raise MagnetiteError("Solver", f"apply_geometric: an array of {x.size} entries where {2 * self.N} are expected")
        y = np.empty(2 * self.N)
        self._check(self._L.mag_apply_geometric(self._h, sid, member, _p(x, C.c_double), _p(y, C.c_double), 1 if masked else 0))
        return y

    def assemble_geometric(self, set="run", member=0):
        """The values of K_G(sigma(u0)) in the layout of assemble_csr() (mag_assemble_geometric)."""
        sid, member = self._prestress("assemble_geometric", set, member)
        nnz = C.c_int64(0)
        self._check(self._L.mag_assemble_csr(self._h, C.byref(nnz), None, None, None))
        val = np.empty(nnz.value)
        self._check(self._L.mag_assemble_geometric(self._h, sid, member, _p(val, C.c_double), MAG_MEM_HOST))
        return val

    # -- transient dynamics: Newmark time stepping of the uploaded part ----------------------------------
    TRANSIENT_INFO = ("steps", "cg_kernel", "preconditioner", "cg_iterations", "max_step_iterations", "snapshots_kept", "resumed", "converged")

    def run_transient(self, steps, dt, density=None, beta=0.25, gamma=0.5, rayleigh=(0.0, 0.0), amplitude=None, u0=None, v0=None,
                      probes=(), energies=False, snapshot_every=0, cg=0, cg_tol=0.0, lumped=False, resume=False):
        """mag_run_transient on the uploaded problem (no run needed): `steps` steps of Newmark's method (include/magnetite_hip.h)."""
        if density is None:
            raise MagnetiteError("Solver", "transient: a density is needed (the model has none)")
        o = _lib.TransientOptions()
        self._L.mag_default_transient_options(C.byref(o))
        o.lumped, o.cg = 1 if lumped else 0, int(cg)
        o.dt, o.beta, o.gamma, o.density = float(dt), float(beta), float(gamma), float(density)
        o.rayleigh_mass, o.rayleigh_stiffness, o.cg_tol = float(rayleigh[0]), float(rayleigh[1]), float(cg_tol)
        return self._run_steps("transient", self._L.mag_run_transient, o, steps, amplitude, u0, v0, probes, energies, snapshot_every, resume)

    def _run_steps(self, name, run, o, steps, amplitude, u0, v0, probes, energies, snapshot_every, resume):
        """What run_transient and run_explicit share: the options both passes have, the call, what download_transient sizes."""
        keep = []  # (the arrays the options point to, until the call returns)

        def vec(x, n):
            if x is None:
                return None
            a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
            if a.size != n:
                raise MagnetiteError("Solver", f"{name}: an array of {a.size} entries where {n} are expected")
            keep.append(a)
            return a.ctypes.data

        probes = np.ascontiguousarray(probes, dtype=np.int32).reshape(-1)
        o.steps, o.resume, o.energies = int(steps), 1 if resume else 0, 1 if energies else 0
        o.snapshot_every, o.num_probes, o.memory = int(snapshot_every), int(probes.size), MAG_MEM_HOST
        o.amplitude = vec(amplitude, max(int(steps), 0) + 1)
        o.u0, o.v0 = vec(u0, 2 * self.N), vec(v0, 2 * self.N)
        o.probes = probes.ctypes.data if probes.size else None
        rc = self._check(run(self._h, C.byref(o)))
        self._transient_probes, self._transient_energies = int(probes.size), bool(energies)  # (what download_transient sizes)
        return rc

    def transient_info(self):
        """The words of mag_get_transient_info by name (TRANSIENT_INFO)."""
        info = (C.c_int32 * 8)()
        self._check(self._L.mag_get_transient_info(self._h, info))
        return dict(zip(self.TRANSIENT_INFO, (int(v) for v in info)))

    def download_transient(self, num_probes=None, energies=None):
        """dict(u, v, a, f (2N: the final state and its reactions), iterations (steps + 1), t_start, t_end, and what the run
        recorded: probe_u / probe_v / probe_a (steps + 1, probes), energies (steps + 1, 3 = T, W, P), snapshots (rows, 2N))."""
        info = self.transient_info()
        # (after an explicit run -- cg_kernel 6, or 7 with total-Lagrangian kinematics -- the rows are those of steps 0,
        # record_every, ...: word 4)
        explicit = info["cg_kernel"] in (6, 7)
        rows, n2 = (info["steps"] // info["max_step_iterations"] if explicit else info["steps"]) + 1, 2 * self.N
        num_probes = self._transient_probes if num_probes is None else num_probes
        energies = self._transient_energies if energies is None else energies
        out = {k: np.empty(n2) for k in ("u", "v", "a", "f")}
        out["iterations"] = np.empty(rows, dtype=np.int32)
        if num_probes:
            for k in ("probe_u", "probe_v", "probe_a"):
                out[k] = np.empty((rows, num_probes))
        if energies:
            out["energies"] = np.empty((rows, 3))
        if info["snapshots_kept"]:
            out["snapshots"] = np.empty((info["snapshots_kept"], n2))
        o = _lib.TransientResult()
        o.u_out, o.v_out, o.a_out, o.f_out = (out[k].ctypes.data for k in ("u", "v", "a", "f"))
        o.iterations = out["iterations"].ctypes.data
        for k in ("probe_u", "probe_v", "probe_a", "energies", "snapshots"):
            if k in out:
                setattr(o, k, out[k].ctypes.data)
        o.memory = MAG_MEM_HOST
        self._check(self._L.mag_download_transient(self._h, C.byref(o)))
        out["t_start"], out["t_end"] = float(o.scalars[0]), float(o.scalars[1])
        if explicit:
            out["dt"], out["dt_bound"] = float(o.scalars[2]), float(o.scalars[3])
        return out

    _transient_probes = 0
    _transient_energies = False

    def transient(self, prob=None, steps=None, dt=None, density=None, beta=0.25, gamma=0.5, rayleigh=(0.0, 0.0), amplitude=None,
                  u0=None, v0=None, probes=(), energies=False, snapshot_every=0, cg=0, cg_tol=0.0, lumped=False, resume=False,
                  kinematics="linear", newton_tol=0.0, max_newton=0):
        """The response of prob (uploaded when given; otherwise of what is uploaded) over `steps` steps of dt: the arrays of
        download_transient() and the words of transient_info() by name.  kinematics="tl": mag_run_transient_tl, Newton's method
        on the total-Lagrangian tangent in every step (rayleigh[1] must be 0) -- the dict gains newton_iterations (steps done + 1),
        newton_residuals and newton_cg (one entry per Newton iteration of the run), elements (E, 8), inverted, the words of
        mag_get_transient_tl_info by name (TRANSIENT_TL_INFO; `steps` is the steps done) and, when a step did not converge
        (converged == 0), `message`."""
        if kinematics not in self.KINEMATICS:
            raise ValueError(f"transient: kinematics {kinematics!r} is none of {sorted(self.KINEMATICS)}")
        if prob is not None:
            self.upload_problem(prob)
        if steps is None or dt is None:
            raise MagnetiteError("Solver", "transient: steps and dt are needed")
        if kinematics == "tl":
            self.run_transient_tl(steps, dt, density, beta, gamma, rayleigh, amplitude, u0, v0, probes, energies, snapshot_every, cg,
                                  cg_tol, lumped, resume, newton_tol, max_newton)
            out = self.download_transient()
            out.update(self.transient_info())
            out.update(self.download_transient_tl())
            out.update(self.transient_tl_info())
            out["inverted"] = bool(out["inverted"])
            out["material"] = self.material_law()
            if not out["converged"]:
                out["message"] = self._L.mag_last_error(self._h).decode()
            return out
        self.run_transient(steps, dt, density, beta, gamma, rayleigh, amplitude, u0, v0, probes, energies, snapshot_every, cg, cg_tol,
                           lumped, resume)
        out = self.download_transient()
        out.update(self.transient_info())
        return out

    # -- nonlinear transient dynamics: Newmark steps, Newton's method on the total-Lagrangian tangent ------
    TRANSIENT_TL_INFO = ("steps", "cg_kernel", "preconditioner", "newton_iterations_total", "max_step_newton", "cg_iterations_total",
                         "inverted", "converged")

    def run_transient_tl(self, steps, dt, density=None, beta=0.25, gamma=0.5, rayleigh=(0.0, 0.0), amplitude=None, u0=None, v0=None,
                         probes=(), energies=False, snapshot_every=0, cg=0, cg_tol=0.0, lumped=False, resume=False, newton_tol=0.0,
                         max_newton=0):
        """mag_run_transient_tl on the uploaded problem (no run needed): `steps` Newmark steps on the total-Lagrangian internal
        force, each by Newton's method (include/magnetite_hip.h)."""
        if density is None:
            raise MagnetiteError("Solver", "transient: a density is needed (the model has none)")
        if float(rayleigh[1]) != 0.0:
            raise MagnetiteError("Solver", "transient: kinematics 'tl' has no stiffness-proportional damping: rayleigh[1] must be 0")
        o = _lib.TransientTlOptions()
        self._L.mag_default_transient_tl_options(C.byref(o))
        o.lumped, o.cg, o.max_newton = 1 if lumped else 0, int(cg), int(max_newton)
        o.dt, o.beta, o.gamma, o.density = float(dt), float(beta), float(gamma), float(density)
        o.rayleigh_mass, o.cg_tol, o.newton_tol = float(rayleigh[0]), float(cg_tol), float(newton_tol)
        return self._run_steps("transient", self._L.mag_run_transient_tl, o, steps, amplitude, u0, v0, probes, energies, snapshot_every, resume)

    def transient_tl_info(self):
        """The words of mag_get_transient_tl_info by name (TRANSIENT_TL_INFO)."""
        info = (C.c_int32 * 8)()
        self._check(self._L.mag_get_transient_tl_info(self._h, info))
        return dict(zip(self.TRANSIENT_TL_INFO, (int(v) for v in info)))

    def download_transient_tl(self):
        """dict(newton_iterations (steps done + 1), newton_residuals, newton_cg (one entry per Newton iteration of the run),
        elements (E, 8: mag_run_newton's element rows of the final state))."""
        info = self.transient_tl_info()
        its = info["newton_iterations_total"]
        out = dict(newton_iterations=np.empty(info["steps"] + 1, dtype=np.int32), newton_residuals=np.empty(its),
                   newton_cg=np.empty(its, dtype=np.int32), elements=np.empty((self.E, 8)))
        o = _lib.TransientTlResult()
        o.newton_iterations, o.elem = out["newton_iterations"].ctypes.data, out["elements"].ctypes.data
        if its:
            o.residuals, o.cg_iterations = out["newton_residuals"].ctypes.data, out["newton_cg"].ctypes.data
        o.memory = MAG_MEM_HOST
        self._check(self._L.mag_download_transient_tl(self._h, C.byref(o)))
        return out

    def assemble_effective_tangent(self, u, c_K, c_M, density, lumped=False):
        """The values of c_K K_T(u) + c_M M in the layout of assemble_csr() (mag_assemble_effective_tangent)."""
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        if u.size != 2 * self.N:
            raise MagnetiteError("Solver", f"assemble_effective_tangent: an array of {u.size} entries where {2 * self.N} are expected")
        nnz = C.c_int64(0)
        self._check(self._L.mag_assemble_csr(self._h, C.byref(nnz), None, None, None))
        val = np.empty(nnz.value)
        self._check(self._L.mag_assemble_effective_tangent(self._h, _p(u, C.c_double), float(c_K), float(c_M), float(density),
                                                           1 if lumped else 0, _p(val, C.c_double), MAG_MEM_HOST))
        return val

    # -- explicit dynamics: central differences on the lumped mass, one fused launch a step --------------
    EXPLICIT_INFO = ("steps", "method", "fused", "step_launches", "record_every", "snapshots_kept", "resumed", "finite")

    def explicit_dt(self, density, rayleigh_stiffness=0.0):
        """mag_explicit_dt on the uploaded problem: dict(lambda_bound, dt_bound_undamped, dt_bound, min_mass)."""
        out = np.empty(4)
        self._check(self._L.mag_explicit_dt(self._h, float(density), float(rayleigh_stiffness), _p(out, C.c_double)))
        return dict(zip(("lambda_bound", "dt_bound_undamped", "dt_bound", "min_mass"), (float(v) for v in out)))

    KINEMATICS = {"linear": _lib.MAG_KIN_LINEAR, "tl": _lib.MAG_KIN_TOTAL_LAGRANGIAN}

    def run_explicit(self, steps, dt=None, dt_scale=0.9, density=None, rayleigh=(0.0, 0.0), amplitude=None, u0=None, v0=None, probes=(),
                     energies=False, record_every=1, snapshot_every=0, resume=False, kinematics="linear"):
        """mag_run_explicit on the uploaded problem (no run needed): `steps` central-difference steps (include/magnetite_hip.h);
        dt None: dt_scale times the device's bound.  kinematics: "linear", or "tl" for the total-Lagrangian internal force (large
        rotations)."""
        if kinematics not in self.KINEMATICS:
            raise ValueError(f"explicit: kinematics {kinematics!r} is none of {sorted(self.KINEMATICS)}")
        if density is None:
            raise MagnetiteError("Solver", "explicit: a density is needed (the model has none)")
        o = _lib.ExplicitOptions()
        self._L.mag_default_explicit_options(C.byref(o))
        o.record_every, o.kinematics = int(record_every), self.KINEMATICS[kinematics]
        o.dt, o.dt_scale, o.density = 0.0 if dt is None else float(dt), float(dt_scale), float(density)
        o.rayleigh_mass, o.rayleigh_stiffness = float(rayleigh[0]), float(rayleigh[1])
        return self._run_steps("explicit", self._L.mag_run_explicit, o, steps, amplitude, u0, v0, probes, energies, snapshot_every, resume)

    def explicit(self, prob=None, steps=None, dt=None, dt_scale=0.9, density=None, rayleigh=(0.0, 0.0), amplitude=None, u0=None, v0=None,
                 probes=(), energies=False, record_every=1, snapshot_every=0, resume=False, kinematics="linear"):
        """The response of prob (uploaded when given; otherwise of what is uploaded) over `steps` explicit steps: the arrays of
        download_transient() (rows at steps 0, record_every, ...), the words of mag_get_transient_info by name (EXPLICIT_INFO),
        dt (the step used), dt_bound and time (the rows' times).  kinematics="tl": method is 7, and the dict gains inverted
        (True when an element had det F <= 0 in some evaluation of the force; `finite` is then 0)."""
        if kinematics not in self.KINEMATICS:
            raise ValueError(f"explicit: kinematics {kinematics!r} is none of {sorted(self.KINEMATICS)}")
        if prob is not None:
            self.upload_problem(prob)
        if steps is None:
            raise MagnetiteError("Solver", "explicit: steps are needed")
        self.run_explicit(steps, dt, dt_scale, density, rayleigh, amplitude, u0, v0, probes, energies, record_every, snapshot_every, resume,
                          kinematics)
        out = self.download_transient()
        info = (C.c_int32 * 8)()
        self._check(self._L.mag_get_transient_info(self._h, info))
        out.update(zip(self.EXPLICIT_INFO, (int(v) for v in info)))
        if kinematics == "tl":
            out["inverted"] = info[7] == 0
            out["material"] = self.material_law()
        out["time"] = out["t_start"] + out["dt"] * (out["record_every"] * np.arange(len(out["iterations"])))
        return out

    def internal_force(self, u):
        """(f, W, inverted) of mag_internal_force: the total-Lagrangian internal force f_int(u) (2N, caller numbering), the strain
        energy W(u), and whether some element has det F <= 0."""
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        if u.size != 2 * self.N:
            raise MagnetiteError("Solver", f"internal_force: an array of {u.size} entries where {2 * self.N} are expected")
        f, scalars = np.empty(2 * self.N), np.empty(2)
        self._check(self._L.mag_internal_force(self._h, _p(u, C.c_double), _p(f, C.c_double), _p(scalars, C.c_double), MAG_MEM_HOST))
        return f, float(scalars[0]), bool(scalars[1] != 0.0)

    # -- the material of the total-Lagrangian passes -----------------------------------------------------
    MATERIAL_LAWS = {"svk": _lib.MAG_LAW_SVK, "neo_hooke": _lib.MAG_LAW_NEO_HOOKE}

    def set_material_law(self, law):
        """mag_set_material_law: "svk" (St. Venant-Kirchhoff, the default) or "neo_hooke" (compressible neo-Hooke, plane stress
        enforced per element) for explicit(kinematics="tl"), internal_force, newton, assemble_tangent, transient(kinematics="tl")
        and assemble_effective_tangent.  Context state: kept across uploads; no stored result changes."""
        if law not in self.MATERIAL_LAWS:
            raise ValueError(f"set_material_law: law {law!r} is none of {sorted(self.MATERIAL_LAWS)}")
        self._check(self._L.mag_set_material_law(self._h, self.MATERIAL_LAWS[law]))

    def material_law(self):
        """The law of mag_get_material_law by name."""
        law = C.c_int32(-1)
        self._check(self._L.mag_get_material_law(self._h, C.byref(law)))
        return {v: k for k, v in self.MATERIAL_LAWS.items()}[law.value]

    # -- nonlinear statics: Newton's method on the total-Lagrangian tangent, in load increments ----------
    NEWTON_INFO = ("increments_converged", "cg_kernel", "preconditioner", "newton_iterations_total", "cg_iterations_total", "halvings",
                   "inverted", "converged")

    def run_newton(self, increments=1, load_factors=None, newton_tol=0.0, max_newton=0, line_search=0, cg=0, cg_tol=0.0, u0=None,
                   probes=(), snapshots=False):
        """mag_run_newton on the uploaded problem (no run needed): the large-deflection equilibrium in `increments` load increments
        (include/magnetite_hip.h)."""
        o = _lib.NewtonOptions()
        self._L.mag_default_newton_options(C.byref(o))
        keep = []  # (the arrays the options point to, until the call returns)

        def vec(x, n, what):
            if x is None:
                return None
            a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
            if a.size != n:
                raise MagnetiteError("Solver", f"newton: {what} has {a.size} entries where {n} are expected")
            keep.append(a)
            return a.ctypes.data

        probes = np.ascontiguousarray(probes, dtype=np.int32).reshape(-1)
        o.increments, o.max_newton, o.line_search, o.cg = int(increments), int(max_newton), int(line_search), int(cg)
        o.snapshots, o.num_probes, o.memory = 1 if snapshots else 0, int(probes.size), MAG_MEM_HOST
        o.newton_tol, o.cg_tol = float(newton_tol), float(cg_tol)
        o.load_factors = vec(load_factors, max(int(increments), 0), "load_factors")
        o.u0 = vec(u0, 2 * self.N, "u0")
        o.probes = probes.ctypes.data if probes.size else None
        rc = self._check(self._L.mag_run_newton(self._h, C.byref(o)))
        self._newton_shape = (int(increments), int(probes.size), bool(snapshots))  # (what download_newton sizes)
        return rc

    def newton_info(self):
        """The words of mag_get_newton_info by name (NEWTON_INFO)."""
        info = (C.c_int32 * 8)()
        self._check(self._L.mag_get_newton_info(self._h, info))
        return dict(zip(self.NEWTON_INFO, (int(v) for v in info)))

    def download_newton(self):
        """dict(u, f (2N), elem (E, 8), load, newton_iterations (increments + 1), energies (increments + 1, 2 = W, Pi), residuals,
        cg_iterations, step_lengths (one entry per Newton iteration of the run), and what the run recorded: probe_u (increments + 1,
        probes), snapshots (increments + 1, 2N))."""
        increments, num_probes, snapshots = self._newton_shape
        rows, n2, its = increments + 1, 2 * self.N, self.newton_info()["newton_iterations_total"]
        out = dict(u=np.empty(n2), f=np.empty(n2), elem=np.empty((self.E, 8)), load=np.empty(rows), energies=np.empty((rows, 2)),
                   newton_iterations=np.empty(rows, dtype=np.int32), residuals=np.empty(its), cg_iterations=np.empty(its, dtype=np.int32),
                   step_lengths=np.empty(its))
        if num_probes:
            out["probe_u"] = np.empty((rows, num_probes))
        if snapshots:
            out["snapshots"] = np.empty((rows, n2))
        o = _lib.NewtonResult()
        o.u_out, o.f_out = out["u"].ctypes.data, out["f"].ctypes.data
        for k in ("elem", "load", "energies", "newton_iterations", "residuals", "cg_iterations", "step_lengths", "probe_u", "snapshots"):
            if k in out and out[k].size:
                setattr(o, k, out[k].ctypes.data)
        o.memory = MAG_MEM_HOST
        self._check(self._L.mag_download_newton(self._h, C.byref(o)))
        return out

    _newton_shape = (0, 0, False)

    def newton(self, prob=None, increments=1, load_factors=None, newton_tol=0.0, max_newton=0, line_search=0, cg=0, cg_tol=0.0, u0=None,
               probes=(), snapshots=False):
        """The large-deflection equilibrium of prob (uploaded when given; otherwise of what is uploaded): the arrays of
        download_newton() and the words of newton_info() by name; `message` is mag_last_error's text when an increment did not
        converge (converged == 0: the state and the records are the last converged increment's)."""
        if prob is not None:
            self.upload_problem(prob)
        self.run_newton(increments, load_factors, newton_tol, max_newton, line_search, cg, cg_tol, u0, probes, snapshots)
        out = self.download_newton()
        info = self.newton_info()
        out["newton_iterations_total"] = info.pop("newton_iterations_total")
        out["cg_iterations_total"] = info.pop("cg_iterations_total")
        out.update(info)
        out["material"] = self.material_law()
        if not out["converged"]:
            out["message"] = self._L.mag_last_error(self._h).decode()
        return out

    def assemble_tangent(self, u):
        """The values of the consistent tangent K_T(u) in the layout of assemble_csr() (mag_assemble_tangent)."""
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        if u.size != 2 * self.N:
            raise MagnetiteError("Solver", f"assemble_tangent: an array of {u.size} entries where {2 * self.N} are expected")
        nnz = C.c_int64(0)
        self._check(self._L.mag_assemble_csr(self._h, C.byref(nnz), None, None, None))
        val = np.empty(nnz.value)
        self._check(self._L.mag_assemble_tangent(self._h, _p(u, C.c_double), _p(val, C.c_double), MAG_MEM_HOST))
        return val

    def assemble_effective(self, c_K, c_M, density, lumped=False):
        """The values of c_K K + c_M M in the layout of assemble_csr() (mag_assemble_effective)."""
        nnz = C.c_int64(0)
        self._check(self._L.mag_assemble_csr(self._h, C.byref(nnz), None, None, None))
        val = np.empty(nnz.value)
        self._check(self._L.mag_assemble_effective(self._h, float(c_K), float(c_M), float(density), 1 if lumped else 0,
                                                   _p(val, C.c_double), MAG_MEM_HOST))
        return val

    # -- pieces, for parity tests ----------------------------------------------
    def element_stiffness(self):
        ke = np.empty(36 * self.E)
        self._check(self._L.mag_element_stiffness(self._h, _p(ke, C.c_double)))
        return ke.reshape(self.E, 6, 6)

    def assemble_csr(self):
        nnz = C.c_int64(0)
        self._check(self._L.mag_assemble_csr(self._h, C.byref(nnz), None, None, None))
        rowptr = np.empty(2 * self.N + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value)
        self._check(self._L.mag_assemble_csr(self._h, C.byref(nnz), _p(rowptr, C.c_int32), _p(col, C.c_int32),
                                             _p(val, C.c_double)))
        return rowptr, col, val

    def reduce_system(self):
        nf, nz = C.c_int64(0), C.c_int64(0)
        self._check(self._L.mag_reduce_system(self._h, C.byref(nf), C.byref(nz), None, None, None, None))
        rowptr = np.empty(nf.value + 1, dtype=np.int32)
        col = np.empty(max(nz.value, 1), dtype=np.int32)
        val = np.empty(max(nz.value, 1))
        b = np.empty(nf.value)
        self._check(self._L.mag_reduce_system(self._h, C.byref(nf), C.byref(nz), _p(rowptr, C.c_int32),
                                              _p(col, C.c_int32), _p(val, C.c_double), _p(b, C.c_double)))
        return rowptr, col[:nz.value], val[:nz.value], b

    def apply_operator(self, x, masked=False):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty(2 * self.N)
        self._check(self._L.mag_apply_operator(self._h, _p(x, C.c_double), _p(y, C.c_double), 1 if masked else 0))
        return y

    def time_operator(self, reps=200):
        ms = C.c_double(0.0)
        self._check(self._L.mag_time_operator(self._h, reps, C.byref(ms)))
        return ms.value

    def time_spmv(self, reps=200):
        ms = C.c_double(0.0)
        self._check(self._L.mag_time_spmv(self._h, reps, C.byref(ms)))
        return ms.value


def flatten(nodes, elements):
    """Vec<Node>/Vec<Element> -> SoA (what the Rust shim does before the extern "C" call).

    A DOF with both or neither of (u, f) set cannot be expressed across the ABI; the reference
    panics on it (solver.rs:431), here it is a Solver error.
    """
    N, E = len(nodes), len(elements)
    xy = np.empty(2 * N)
    u_known = np.zeros(2 * N, dtype=np.uint8)
    u_in = np.zeros(2 * N)
    f_in = np.zeros(2 * N)
    for i, nd in enumerate(nodes):
        xy[2 * i], xy[2 * i + 1] = nd.vertex.x, nd.vertex.y
        for a, (u, f) in enumerate(((nd.ux, nd.fx), (nd.uy, nd.fy))):
            if (u is None) == (f is None):
                raise MagnetiteError("Solver", f"node {i} axis {'xy'[a]}: exactly one of displacement/force "
                                               "must be prescribed")
            if u is not None:
                u_known[2 * i + a], u_in[2 * i + a] = 1, u
            else:
                f_in[2 * i + a] = f
    conn = np.empty(3 * E, dtype=np.int32)
    for e, el in enumerate(elements):
        if len(el.nodes) != 3:
            raise MagnetiteError("Solver", f"element {e} does not have 3 nodes")
        conn[3 * e:3 * e + 3] = el.nodes
    return xy, conn, u_known, u_in, f_in


def run(nodes, elements, model_metadata, **options):
    """solver.rs:543-586: updates values on the nodes and elements lists in place."""
    xy, conn, u_known, u_in, f_in = flatten(nodes, elements)
    with Context(**options) as ctx:
        ctx.upload(xy, conn, u_known, u_in, f_in, model_metadata.youngs_modulus, model_metadata.poisson_ratio,
                   model_metadata.part_thickness)
        ctx.run()
        u, f, s = ctx.download()
    for i, nd in enumerate(nodes):
        nd.ux, nd.uy = float(u[2 * i]), float(u[2 * i + 1])
        nd.fx, nd.fy = float(f[2 * i]), float(f[2 * i + 1])
    for e, el in enumerate(elements):
        el.stress = float(s[e])
    return None
