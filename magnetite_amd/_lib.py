"""ctypes binding of include/magnetite_hip.h (libmagnetite_hip.so).

Plumbing only: structs and prototypes mirror the header one to one.  There is
no fallback -- if the shared library is missing or no HIP device is usable the
calls raise MagnetiteError with the library's message.
"""
import ctypes as C
import os
import subprocess

_DIR = os.path.dirname(os.path.abspath(__file__))
# MAG_LIB_PATH: load another build of the same library (A/B of compiler flags or kernel variants in one GPU session)
SO_PATH = os.environ.get("MAG_LIB_PATH") or os.path.join(_DIR, "libmagnetite_hip.so")
CSRC = os.path.join(_DIR, "csrc")

MAG_OK, MAG_ERR_BAD_ARGS, MAG_ERR_BC_MISMATCH, MAG_ERR_NOT_CONVERGED = 0, 1, 2, 3
MAG_ERR_HIP, MAG_ERR_RCCL, MAG_ERR_TOO_LARGE, MAG_ERR_STATE = 4, 5, 6, 7
MAG_STOP_RNORM, MAG_STOP_RNORM_SQ, MAG_STOP_REL = 0, 1, 2
MAG_OP_MATRIX_FREE, MAG_OP_CSR = 0, 1
MAG_FIELD_CG_PLAIN, MAG_FIELD_CG_JACOBI, MAG_FIELD_CG_BLOCK_JACOBI = 1, 2, 3
MAG_TERM_NONE, MAG_TERM_TARGET_COST, MAG_TERM_MAX_ITERS, MAG_TERM_BREAKDOWN = 0, 1, 2, 3
MAG_MEM_HOST, MAG_MEM_DEVICE = 0, 1
MAG_KIN_LINEAR, MAG_KIN_TOTAL_LAGRANGIAN = 0, 1
MAG_LAW_SVK, MAG_LAW_NEO_HOOKE = 0, 1
MAG_SET_RUN, MAG_SET_CASES, MAG_SET_VARIANTS = 0, 1, 2
MAG_OBJ_DISP_LSQ, MAG_OBJ_STRESS_PNORM = 0, 1
MAG_REFINE_MARKS, MAG_REFINE_MAX_FRACTION, MAG_REFINE_TOP_FRACTION = 0, 1, 2
MAG_UNIQUE_ID_BYTES = 128
MAG_IPC_HANDLE_BYTES = 64

# every symbol include/magnetite_hip.h declares (tests/test_abi.py checks the .so exports them all)
SYMBOLS = [
    "mag_version", "mag_default_options", "mag_create", "mag_destroy", "mag_last_error", "mag_solve",
    "mag_upload", "mag_run", "mag_download", "mag_get_stats", "mag_get_history", "mag_compute_element_area",
    "mag_compute_strain_displacement_matrix", "mag_compute_stress_strain_matrix",
    "mag_element_stiffness", "mag_assemble_csr", "mag_reduce_system", "mag_apply_operator", "mag_time_operator", "mag_time_spmv",
    "mag_set_load_cases", "mag_run_cases", "mag_download_case", "mag_get_case_stats", "mag_get_cases_info",
    "mag_set_variants", "mag_run_variants", "mag_download_variant", "mag_get_variant_stats", "mag_get_variants_info",
    "mag_assemble_csr_variant",
    "mag_run_sensitivities", "mag_download_sensitivity",
    "mag_run_adjoint", "mag_download_adjoint", "mag_get_adjoint_stats", "mag_get_adjoint_info",
    "mag_run_objective", "mag_download_objective",
    "mag_run_stress", "mag_download_stress",
    "mag_run_modal", "mag_download_modal", "mag_get_modal_info", "mag_get_modal_stats", "mag_apply_mass",
    "mag_run_buckling", "mag_download_buckling", "mag_get_buckling_info", "mag_get_buckling_stats", "mag_apply_geometric",
    "mag_assemble_geometric",
    "mag_default_transient_options", "mag_run_transient", "mag_download_transient", "mag_get_transient_info", "mag_assemble_effective",
    "mag_default_explicit_options", "mag_run_explicit", "mag_explicit_dt", "mag_internal_force",
    "mag_default_newton_options", "mag_run_newton", "mag_download_newton", "mag_get_newton_info", "mag_assemble_tangent",
    "mag_default_transient_tl_options", "mag_run_transient_tl", "mag_download_transient_tl", "mag_get_transient_tl_info",
    "mag_assemble_effective_tangent",
    "mag_set_material_law", "mag_get_material_law",
    "mag_run_refine", "mag_get_refine_info", "mag_download_refine", "mag_upload_refined",
    "mag_set_element_scale", "mag_design_init", "mag_design_step", "mag_get_design_info", "mag_download_design",
    "mag_comm_get_unique_id", "mag_comm_init_rccl", "mag_comm_query", "mag_comm_init_callback", "mag_comm_set_window", "mag_comm_inbox_create", "mag_comm_inbox_open",
]


class Options(C.Structure):
    _fields_ = [("device", C.c_int32), ("stop_mode", C.c_int32), ("tol", C.c_double), ("max_iter", C.c_int64),
                ("cg_operator", C.c_int32), ("assemble_csr", C.c_int32), ("check_every", C.c_int32),
                ("use_graph", C.c_int32), ("tile_nodes", C.c_int32), ("history_len", C.c_int32),
                ("verbose", C.c_int32), ("op_variant", C.c_int32), ("cg_variant", C.c_int32), ("precision", C.c_int32),
                ("preconditioner", C.c_int32), ("field_cg", C.c_int32)]


class Problem(C.Structure):
    _fields_ = [("num_nodes", C.c_int64), ("num_elements", C.c_int64), ("xy", C.c_void_p), ("conn", C.c_void_p),
                ("u_known", C.c_void_p), ("u_in", C.c_void_p), ("f_in", C.c_void_p),
                ("youngs_modulus", C.c_double), ("poisson_ratio", C.c_double), ("part_thickness", C.c_double),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("u_out", C.c_void_p), ("f_out", C.c_void_p), ("stress_out", C.c_void_p),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("iterations", C.c_int64), ("final_cost", C.c_double), ("rhs_norm", C.c_double),
                ("converged", C.c_int32), ("breakdown", C.c_int32), ("n_free", C.c_int64), ("nnz", C.c_int64),
                ("num_tiles", C.c_int64), ("ell_entries", C.c_int64), ("halo_nodes", C.c_int64),
                ("max_tile_halo", C.c_int32), ("lds_operator", C.c_int32), ("cg_kernel", C.c_int32),
                ("exchange", C.c_int32), ("ms_order", C.c_double),
                ("ms_csr_symbolic", C.c_double), ("ms_element", C.c_double), ("ms_assemble", C.c_double),
                ("ms_bc", C.c_double), ("ms_cg", C.c_double), ("ms_post", C.c_double), ("ms_total", C.c_double),
                ("best_iteration", C.c_int64), ("termination", C.c_int32), ("persist_timeout", C.c_int32),
                ("exchange_timeout", C.c_int32), ("best_param_mismatch", C.c_int32),
                ("edge_blocks", C.c_int32), ("tiles_per_workgroup", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Sensitivity(C.Structure):
    _fields_ = [("energy_out", C.c_void_p), ("dxy_out", C.c_void_p), ("scalars", C.c_double * 8),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class Adjoint(C.Structure):
    _fields_ = [("lambda_out", C.c_void_p), ("dloads_out", C.c_void_p), ("delem_out", C.c_void_p), ("dxy_out", C.c_void_p),
                ("scalars", C.c_double * 8), ("memory", C.c_int32), ("reserved", C.c_int32)]


class Objective(C.Structure):
    _fields_ = [("kind", C.c_int32), ("per_member", C.c_int32), ("p", C.c_double), ("scale", C.c_double),
                ("weights", C.c_void_p), ("target", C.c_void_p), ("memory", C.c_int32), ("reserved", C.c_int32)]


class ObjectiveResult(C.Structure):
    _fields_ = [("g_out", C.c_void_p), ("pxy_out", C.c_void_p), ("dxy_out", C.c_void_p), ("scalars", C.c_double * 8),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class StressField(C.Structure):
    _fields_ = [("elem_out", C.c_void_p), ("node_out", C.c_void_p), ("eta2_out", C.c_void_p), ("scalars", C.c_double * 8),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class ModalOptions(C.Structure):
    _fields_ = [("modes", C.c_int32), ("subspace", C.c_int32), ("max_outer", C.c_int32), ("lumped", C.c_int32),
                ("density", C.c_double), ("tol", C.c_double), ("cg_tol", C.c_double)]


class ModalResult(C.Structure):
    _fields_ = [("lambda_out", C.c_void_p), ("frequency_out", C.c_void_p), ("residual_out", C.c_void_p), ("shapes_out", C.c_void_p),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class BucklingOptions(C.Structure):
    _fields_ = [("modes", C.c_int32), ("subspace", C.c_int32), ("max_outer", C.c_int32), ("set", C.c_int32),
                ("member", C.c_int32), ("reserved", C.c_int32), ("tol", C.c_double), ("cg_tol", C.c_double)]


class BucklingResult(C.Structure):
    _fields_ = [("load_factor_out", C.c_void_p), ("residual_out", C.c_void_p), ("shapes_out", C.c_void_p),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class TransientOptions(C.Structure):
    _fields_ = [("steps", C.c_int32), ("resume", C.c_int32), ("lumped", C.c_int32), ("cg", C.c_int32), ("energies", C.c_int32),
                ("snapshot_every", C.c_int32), ("num_probes", C.c_int32), ("memory", C.c_int32),
                ("dt", C.c_double), ("beta", C.c_double), ("gamma", C.c_double), ("density", C.c_double),
                ("rayleigh_mass", C.c_double), ("rayleigh_stiffness", C.c_double), ("cg_tol", C.c_double),
                ("amplitude", C.c_void_p), ("u0", C.c_void_p), ("v0", C.c_void_p), ("probes", C.c_void_p)]


class ExplicitOptions(C.Structure):
    _fields_ = [("steps", C.c_int32), ("resume", C.c_int32), ("energies", C.c_int32), ("record_every", C.c_int32),
                ("snapshot_every", C.c_int32), ("num_probes", C.c_int32), ("memory", C.c_int32), ("kinematics", C.c_int32),
                ("dt", C.c_double), ("dt_scale", C.c_double), ("density", C.c_double), ("rayleigh_mass", C.c_double),
                ("rayleigh_stiffness", C.c_double),
                ("amplitude", C.c_void_p), ("u0", C.c_void_p), ("v0", C.c_void_p), ("probes", C.c_void_p)]


class TransientResult(C.Structure):
    _fields_ = [("u_out", C.c_void_p), ("v_out", C.c_void_p), ("a_out", C.c_void_p), ("f_out", C.c_void_p),
                ("probe_u", C.c_void_p), ("probe_v", C.c_void_p), ("probe_a", C.c_void_p), ("energies", C.c_void_p),
                ("snapshots", C.c_void_p), ("iterations", C.c_void_p), ("scalars", C.c_double * 4),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class NewtonOptions(C.Structure):
    _fields_ = [("increments", C.c_int32), ("max_newton", C.c_int32), ("line_search", C.c_int32), ("cg", C.c_int32),
                ("snapshots", C.c_int32), ("num_probes", C.c_int32), ("memory", C.c_int32), ("reserved", C.c_int32),
                ("newton_tol", C.c_double), ("cg_tol", C.c_double),
                ("load_factors", C.c_void_p), ("u0", C.c_void_p), ("probes", C.c_void_p)]


class NewtonResult(C.Structure):
    _fields_ = [("u_out", C.c_void_p), ("f_out", C.c_void_p), ("elem", C.c_void_p), ("probe_u", C.c_void_p), ("snapshots", C.c_void_p),
                ("load", C.c_void_p), ("energies", C.c_void_p), ("newton_iterations", C.c_void_p), ("residuals", C.c_void_p),
                ("cg_iterations", C.c_void_p), ("step_lengths", C.c_void_p), ("memory", C.c_int32), ("reserved", C.c_int32)]


class TransientTlOptions(C.Structure):
    _fields_ = [("steps", C.c_int32), ("resume", C.c_int32), ("lumped", C.c_int32), ("cg", C.c_int32), ("energies", C.c_int32),
                ("snapshot_every", C.c_int32), ("num_probes", C.c_int32), ("memory", C.c_int32), ("max_newton", C.c_int32),
                ("reserved", C.c_int32),
                ("dt", C.c_double), ("beta", C.c_double), ("gamma", C.c_double), ("density", C.c_double),
                ("rayleigh_mass", C.c_double), ("cg_tol", C.c_double), ("newton_tol", C.c_double),
                ("amplitude", C.c_void_p), ("u0", C.c_void_p), ("v0", C.c_void_p), ("probes", C.c_void_p)]


class TransientTlResult(C.Structure):
    _fields_ = [("newton_iterations", C.c_void_p), ("cg_iterations", C.c_void_p), ("residuals", C.c_void_p), ("elem", C.c_void_p),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class RefineOptions(C.Structure):
    _fields_ = [("rule", C.c_int32), ("split", C.c_int32), ("theta", C.c_double), ("marks", C.c_void_p), ("indicator", C.c_void_p),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


class Refined(C.Structure):
    _fields_ = [("xy", C.c_void_p), ("conn", C.c_void_p), ("u_known", C.c_void_p), ("u_in", C.c_void_p), ("f_in", C.c_void_p),
                ("node_parents", C.c_void_p), ("elem_parent", C.c_void_p), ("memory", C.c_int32), ("reserved", C.c_int32)]


class DesignOptions(C.Structure):
    _fields_ = [("volume_fraction", C.c_double), ("scale_min", C.c_double), ("rho_min", C.c_double), ("move", C.c_double),
                ("penal", C.c_int32), ("filter_passes", C.c_int32), ("reserved", C.c_int32 * 2)]


class Design(C.Structure):
    _fields_ = [("rho_out", C.c_void_p), ("rho_filtered_out", C.c_void_p), ("scale_out", C.c_void_p), ("dJ_drho_out", C.c_void_p),
                ("memory", C.c_int32), ("reserved", C.c_int32)]


HASHED_SOURCES = ("persist.hip", "persist_kernel.h", "persist_shapes.h", "persist_inst.hip", "cg.hip", "cg_device.h", "exact.hip", "symbolic.hip", "kernels.h")


def kernel_source_hash():
    """sha256 (first 16 hex digits) over the kernel sources as they are in the tree now -- the digest csrc/Makefile
    writes next to the library when it links it."""
    import hashlib
    h = hashlib.sha256()
    for name in HASHED_SOURCES:
        with open(os.path.join(CSRC, name), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def built_source_hash():
    """The digest recorded when the loaded library was linked (None for a library built by other means)."""
    path = os.path.splitext(SO_PATH)[0] + ".srchash"
    try:
        with open(path) as f:
            return f.read().strip() or None
    except OSError:
        return None


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int64)


def build(force=False):
    """hipcc --offload-arch=gfx950 build of the shared library (cross-compiles without a GPU), and of its diagnostic twin with
    the in-kernel phase stamps (libmagnetite_hip_stamps.so: scripts/persist_phases*.py load it; the product never does)."""
    cmd = ["make", "-C", CSRC, "-j6", "all", "stamps"] + (["-B"] if force else [])
    subprocess.check_call(cmd, stdout=subprocess.DEVNULL)
    return SO_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise OSError(f"{SO_PATH} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(there is no CPU fallback)")
    L = C.CDLL(SO_PATH)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.mag_version.restype = C.c_int
    L.mag_default_options.argtypes = [C.POINTER(Options)]
    L.mag_default_options.restype = None
    L.mag_create.argtypes = [C.POINTER(Options)]
    L.mag_create.restype = vp
    L.mag_destroy.argtypes = [vp]
    L.mag_destroy.restype = None
    L.mag_last_error.argtypes = [vp]
    L.mag_last_error.restype = C.c_char_p
    L.mag_solve.argtypes = [vp, C.POINTER(Problem), C.POINTER(Result)]
    L.mag_upload.argtypes = [vp, C.POINTER(Problem)]
    L.mag_run.argtypes = [vp]
    L.mag_download.argtypes = [vp, C.POINTER(Result)]
    L.mag_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.mag_get_history.argtypes = [vp, dp, C.c_int64]
    L.mag_set_load_cases.argtypes = [vp, C.c_int32, dp, dp, C.c_int32]
    L.mag_run_cases.argtypes = [vp]
    L.mag_download_case.argtypes = [vp, C.c_int32, C.POINTER(Result)]
    L.mag_get_case_stats.argtypes = [vp, C.c_int32, C.POINTER(Stats)]
    L.mag_get_cases_info.argtypes = [vp, ip]
    L.mag_set_variants.argtypes = [vp, C.c_int32, dp, dp, dp, dp, C.c_int32]
    L.mag_run_variants.argtypes = [vp]
    L.mag_download_variant.argtypes = [vp, C.c_int32, C.POINTER(Result)]
    L.mag_get_variant_stats.argtypes = [vp, C.c_int32, C.POINTER(Stats)]
    L.mag_get_variants_info.argtypes = [vp, ip]
    L.mag_assemble_csr_variant.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), ip, ip, dp]
    L.mag_run_sensitivities.argtypes = [vp, C.c_int32]
    L.mag_download_sensitivity.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(Sensitivity)]
    if hasattr(L, "mag_run_adjoint"):  # (an earlier build loaded through MAG_LIB_PATH has none: scripts/adjoint_probe.py)
        L.mag_run_adjoint.argtypes = [vp, C.c_int32, dp, C.c_int32]
        L.mag_download_adjoint.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(Adjoint)]
        L.mag_get_adjoint_stats.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(Stats)]
        L.mag_get_adjoint_info.argtypes = [vp, C.c_int32, ip]
    if hasattr(L, "mag_run_objective"):  # (likewise: scripts/objective_probe.py)
        L.mag_run_objective.argtypes = [vp, C.c_int32, C.POINTER(Objective), C.c_int32]
        L.mag_download_objective.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(ObjectiveResult)]
    if hasattr(L, "mag_run_stress"):  # (likewise: scripts/stress_recovery_probe.py)
        L.mag_run_stress.argtypes = [vp, C.c_int32]
        L.mag_download_stress.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(StressField)]
    if hasattr(L, "mag_run_modal"):  # (likewise: scripts/modal_probe.py)
        L.mag_run_modal.argtypes = [vp, C.POINTER(ModalOptions)]
        L.mag_download_modal.argtypes = [vp, C.POINTER(ModalResult)]
        L.mag_get_modal_info.argtypes = [vp, ip]
        L.mag_get_modal_stats.argtypes = [vp, C.c_int32, C.POINTER(Stats)]
        L.mag_apply_mass.argtypes = [vp, C.c_double, C.c_int32, dp, dp, C.c_int32]
    if hasattr(L, "mag_run_buckling"):  # (likewise: scripts/buckling_probe.py)
        L.mag_run_buckling.argtypes = [vp, C.POINTER(BucklingOptions)]
        L.mag_download_buckling.argtypes = [vp, C.POINTER(BucklingResult)]
        L.mag_get_buckling_info.argtypes = [vp, ip]
        L.mag_get_buckling_stats.argtypes = [vp, C.c_int32, C.POINTER(Stats)]
        L.mag_apply_geometric.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, C.c_int32]
        L.mag_assemble_geometric.argtypes = [vp, C.c_int32, C.c_int32, dp, C.c_int32]
    if hasattr(L, "mag_run_transient"):  # (likewise: scripts/transient_probe.py)
        L.mag_default_transient_options.argtypes = [C.POINTER(TransientOptions)]
        L.mag_default_transient_options.restype = None
        L.mag_run_transient.argtypes = [vp, C.POINTER(TransientOptions)]
        L.mag_download_transient.argtypes = [vp, C.POINTER(TransientResult)]
        L.mag_get_transient_info.argtypes = [vp, ip]
        L.mag_assemble_effective.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_int32, dp, C.c_int32]
    if hasattr(L, "mag_run_explicit"):  # (likewise: scripts/explicit_probe.py)
        L.mag_default_explicit_options.argtypes = [C.POINTER(ExplicitOptions)]
        L.mag_default_explicit_options.restype = None
        L.mag_run_explicit.argtypes = [vp, C.POINTER(ExplicitOptions)]
        L.mag_explicit_dt.argtypes = [vp, C.c_double, C.c_double, dp]
    if hasattr(L, "mag_internal_force"):  # (likewise: scripts/explicit_tl_probe.py)
        L.mag_internal_force.argtypes = [vp, dp, dp, dp, C.c_int32]
    if hasattr(L, "mag_run_newton"):  # (likewise: scripts/newton_probe.py)
        L.mag_default_newton_options.argtypes = [C.POINTER(NewtonOptions)]
        L.mag_default_newton_options.restype = None
        L.mag_run_newton.argtypes = [vp, C.POINTER(NewtonOptions)]
        L.mag_download_newton.argtypes = [vp, C.POINTER(NewtonResult)]
        L.mag_get_newton_info.argtypes = [vp, ip]
        L.mag_assemble_tangent.argtypes = [vp, dp, dp, C.c_int32]
    if hasattr(L, "mag_run_transient_tl"):  # (likewise: scripts/transient_tl_probe.py)
        L.mag_default_transient_tl_options.argtypes = [C.POINTER(TransientTlOptions)]
        L.mag_default_transient_tl_options.restype = None
        L.mag_run_transient_tl.argtypes = [vp, C.POINTER(TransientTlOptions)]
        L.mag_download_transient_tl.argtypes = [vp, C.POINTER(TransientTlResult)]
        L.mag_get_transient_tl_info.argtypes = [vp, ip]
        L.mag_assemble_effective_tangent.argtypes = [vp, dp, C.c_double, C.c_double, C.c_double, C.c_int32, dp, C.c_int32]
    if hasattr(L, "mag_set_material_law"):  # (likewise: scripts/hyper_probe.py)
        L.mag_set_material_law.argtypes = [vp, C.c_int32]
        L.mag_get_material_law.argtypes = [vp, ip]
    if hasattr(L, "mag_run_refine"):  # (likewise: scripts/refine_probe.py)
        L.mag_run_refine.argtypes = [vp, C.POINTER(RefineOptions)]
        L.mag_get_refine_info.argtypes = [vp, C.POINTER(C.c_int64)]
        L.mag_download_refine.argtypes = [vp, C.POINTER(Refined)]
        L.mag_upload_refined.argtypes = [vp]
    if hasattr(L, "mag_set_element_scale"):  # (likewise: scripts/design_probe.py)
        L.mag_set_element_scale.argtypes = [vp, dp, C.c_int32]
        L.mag_design_init.argtypes = [vp, C.POINTER(DesignOptions), dp, C.c_int32]
        L.mag_design_step.argtypes = [vp, dp, C.c_int32]
        L.mag_get_design_info.argtypes = [vp, dp]
        L.mag_download_design.argtypes = [vp, C.POINTER(Design)]
    L.mag_compute_element_area.argtypes = [dp, ip]
    L.mag_compute_element_area.restype = C.c_double
    L.mag_compute_strain_displacement_matrix.argtypes = [dp, ip, C.c_double, dp]
    L.mag_compute_strain_displacement_matrix.restype = None
    L.mag_compute_stress_strain_matrix.argtypes = [C.c_double, C.c_double, dp]
    L.mag_compute_stress_strain_matrix.restype = None
    L.mag_element_stiffness.argtypes = [vp, dp]
    L.mag_assemble_csr.argtypes = [vp, C.POINTER(C.c_int64), ip, ip, dp]
    L.mag_reduce_system.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), ip, ip, dp, dp]
    L.mag_apply_operator.argtypes = [vp, dp, dp, C.c_int32]
    L.mag_time_operator.argtypes = [vp, C.c_int32, dp]
    L.mag_time_spmv.argtypes = [vp, C.c_int32, dp]
    L.mag_comm_get_unique_id.argtypes = [vp]
    L.mag_comm_init_rccl.argtypes = [vp, vp, C.c_int32, C.c_int32]
    L.mag_comm_query.argtypes = [vp, ip]
    L.mag_comm_init_callback.argtypes = [vp, C.c_int32, C.c_int32, ALLREDUCE_FN, vp]
    L.mag_comm_set_window.argtypes = [vp, vp, C.c_uint64]
    L.mag_comm_inbox_create.argtypes = [vp, C.c_uint64, vp]
    L.mag_comm_inbox_open.argtypes = [vp, vp]
    for name in SYMBOLS:
        fn = getattr(L, name, None)
        if fn is not None and fn.restype is C.c_int and name not in ("mag_version",):
            fn.restype = C.c_int
    _lib = L
    return L
