"""No GPU: one rule for every `memory` of the ABI (include/magnetite_hip.h, at enum mag_memory).  A value that is none of the enum
is refused with MAG_ERR_BAD_ARGS, the message naming the function and mag_memory, among the checks that precede any HIP call and
ahead of the MAG_ERR_STATE of a missing upload; where nothing would be read through it, it is not looked at; the two values of
the enum still reach the state check.  (mag_set_element_scale, mag_design_init, mag_design_step and mag_download_design:
tests/test_design.py::test_errors_before_any_hip_call.)"""
import ctypes as C

import numpy as np

from magnetite_amd import _lib
from magnetite_amd._lib import MAG_ERR_BAD_ARGS, MAG_ERR_HIP, MAG_ERR_STATE

UNKNOWN = (-1, 2, 7)
KNOWN = (_lib.MAG_MEM_HOST, _lib.MAG_MEM_DEVICE)


def entry_points(L, h):
    """name -> call(memory): every entry point and struct of the header that carries a `memory`, with pointers that are not NULL
    (host arrays of a 2-node, 1-element problem: no call here gets as far as reading them)."""
    N, E, M = 2, 1, 1
    d = np.ones(4 * max(2 * N, E) * M)
    i32, u8 = np.zeros(16, dtype=np.int32), np.zeros(16, dtype=np.uint8)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    a = d.ctypes.data
    keep = [d, i32, u8]
    mat = np.array([1.0, 0.3, 1.0])
    keep.append(mat)
    mp = mat.ctypes.data_as(C.POINTER(C.c_double))

    def problem(memory):  # (a value of the enum comes with NULL arrays: on a machine with a GPU nothing may be uploaded or solved)
        if memory in KNOWN:
            return _lib.Problem(N, E, None, None, None, None, None, 1.0, 0.3, 1.0, memory, 0)
        return _lib.Problem(N, E, a, i32.ctypes.data, u8.ctypes.data, a, a, 1.0, 0.3, 1.0, memory, 0)

    def result(memory):
        return _lib.Result(a, a, a, memory, 0)

    scalars = lambda: (C.c_double * 8)()
    calls = {
        "mag_upload": lambda m: L.mag_upload(h, C.byref(problem(m))),
        "mag_solve": lambda m: L.mag_solve(h, C.byref(problem(m)), C.byref(result(0))),
        "mag_solve (result)": lambda m: L.mag_solve(h, C.byref(problem(_lib.MAG_MEM_HOST)), C.byref(result(m))),
        "mag_download": lambda m: L.mag_download(h, C.byref(result(m))),
        "mag_set_load_cases": lambda m: L.mag_set_load_cases(h, M, dp, dp, m),
        "mag_download_case": lambda m: L.mag_download_case(h, 0, C.byref(result(m))),
        "mag_set_variants": lambda m: L.mag_set_variants(h, M, dp, mp, dp, dp, m),
        "mag_set_variants (xy)": lambda m: L.mag_set_variants(h, M, dp, None, None, None, m),
        "mag_set_variants (material)": lambda m: L.mag_set_variants(h, M, None, mp, None, None, m),
        "mag_download_variant": lambda m: L.mag_download_variant(h, 0, C.byref(result(m))),
        "mag_download_sensitivity": lambda m: L.mag_download_sensitivity(h, 0, 0, C.byref(_lib.Sensitivity(a, a, scalars(), m, 0))),
        "mag_run_adjoint": lambda m: L.mag_run_adjoint(h, 0, dp, m),
        "mag_download_adjoint": lambda m: L.mag_download_adjoint(h, 0, 0, C.byref(_lib.Adjoint(a, a, a, a, scalars(), m, 0))),
        "mag_run_objective": lambda m: L.mag_run_objective(h, 0, C.byref(_lib.Objective(_lib.MAG_OBJ_DISP_LSQ, 0, 2.0, 1.0, a, a, m, 0)), 0),
        "mag_run_objective (weights)": lambda m: L.mag_run_objective(h, 0, C.byref(_lib.Objective(_lib.MAG_OBJ_STRESS_PNORM, 0, 2.0, 1.0, a, None, m, 0)), 0),
        "mag_download_objective": lambda m: L.mag_download_objective(h, 0, 0, C.byref(_lib.ObjectiveResult(a, a, None, scalars(), m, 0))),
        "mag_download_stress": lambda m: L.mag_download_stress(h, 0, 0, C.byref(_lib.StressField(a, a, a, scalars(), m, 0))),
        "mag_download_modal": lambda m: L.mag_download_modal(h, C.byref(_lib.ModalResult(a, a, a, a, m, 0))),
        "mag_run_refine": lambda m: L.mag_run_refine(h, C.byref(_lib.RefineOptions(_lib.MAG_REFINE_MARKS, 1, 0.5, u8.ctypes.data, None, m, 0))),
        "mag_run_refine (indicator)": lambda m: L.mag_run_refine(h, C.byref(_lib.RefineOptions(_lib.MAG_REFINE_TOP_FRACTION, 1, 0.5, None, a, m, 0))),
        "mag_download_refine": lambda m: L.mag_download_refine(h, C.byref(_lib.Refined(a, i32.ctypes.data, u8.ctypes.data, a, a, i32.ctypes.data, i32.ctypes.data, m, 0))),
    }
    return calls, keep


# with a value of the enum these get as far as the context's HIP state (mag_upload, mag_solve) or, in mag_download, past it: what
# they answer then depends on whether the machine has a GPU, but it is never about `memory`
PAST_THE_ARGUMENT_CHECKS = ("mag_upload", "mag_solve", "mag_solve (result)", "mag_download")


def test_an_unknown_memory_is_refused_by_every_entry_point_before_any_hip_call(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    try:
        calls, keep = entry_points(L, h)
        for name, call in calls.items():
            fn = name.split()[0].encode()
            for memory in UNKNOWN:
                assert call(memory) == MAG_ERR_BAD_ARGS, (name, memory)
                msg = L.mag_last_error(h)
                assert fn in msg and b"mag_memory" in msg and str(memory).encode() in msg, (name, memory, msg)
            for memory in KNOWN:  # a value of the enum: the missing upload, run or pass is what is noticed
                rc = call(memory)
                msg = L.mag_last_error(h)
                if name in PAST_THE_ARGUMENT_CHECKS:  # (without a GPU: MAG_ERR_HIP with mag_create's message left as it was)
                    assert rc == MAG_ERR_HIP or (rc != 0 and b"mag_memory" not in msg), (name, memory, rc, msg)
                else:
                    assert rc == MAG_ERR_STATE and b"mag_memory" not in msg, (name, memory, rc, msg)
        # nothing would be read: `memory` is not looked at
        for memory in UNKNOWN:
            by_eta2 = _lib.RefineOptions(_lib.MAG_REFINE_TOP_FRACTION, 1, 0.5, None, None, memory, 0)
            assert L.mag_run_refine(h, C.byref(by_eta2)) == MAG_ERR_STATE and b"before mag_upload" in L.mag_last_error(h)
            ones = _lib.Objective(_lib.MAG_OBJ_STRESS_PNORM, 0, 2.0, 1.0, None, None, memory, 0)
            assert L.mag_run_objective(h, 0, C.byref(ones), 0) == MAG_ERR_STATE and b"mag_memory" not in L.mag_last_error(h)
            assert L.mag_run_adjoint(h, 0, None, memory) == MAG_ERR_BAD_ARGS and b"null dJ_du" in L.mag_last_error(h)
        # the other argument checks are where they were: a NULL struct is reported as such
        assert L.mag_download(h, None) in (MAG_ERR_HIP, MAG_ERR_BAD_ARGS)
        assert L.mag_download_case(h, 0, None) == MAG_ERR_BAD_ARGS and b"null result" in L.mag_last_error(h)
        assert L.mag_download_modal(h, None) == MAG_ERR_BAD_ARGS and b"null modal result" in L.mag_last_error(h)
        assert L.mag_download_refine(h, None) == MAG_ERR_BAD_ARGS and b"null refined mesh" in L.mag_last_error(h)
        assert L.mag_download_stress(h, 0, 0, None) == MAG_ERR_BAD_ARGS and b"null stress field" in L.mag_last_error(h)
        for memory in UNKNOWN:  # without a context there is nothing to name the function in
            assert L.mag_upload(None, C.byref(_lib.Problem(memory=memory))) == MAG_ERR_BAD_ARGS
            assert L.mag_download(None, C.byref(_lib.Result(memory=memory))) == MAG_ERR_BAD_ARGS
            assert L.mag_set_load_cases(None, 1, None, None, memory) == MAG_ERR_BAD_ARGS
        del keep
    finally:
        L.mag_destroy(h)
