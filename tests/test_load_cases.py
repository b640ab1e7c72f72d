"""CPU: the load-case entry points (mag_set_load_cases ... mag_get_cases_info) exist in header, binding and library, and
their call-order and argument errors come back before any HIP call -- on a context that has no GPU at all."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from magnetite_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "magnetite_amd", "csrc")
NAMES = ("mag_set_load_cases", "mag_run_cases", "mag_download_case", "mag_get_case_stats", "mag_get_cases_info")
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7


def test_symbols_in_header_binding_and_library(built):
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.mag_version() == 4  # new entry points only: the version and every struct stay


@pytest.fixture()
def ctx(built):
    L = _lib.lib()
    h = L.mag_create(None)
    assert h
    yield L, h
    L.mag_destroy(h)


def test_argument_errors_before_any_hip_call(ctx):
    L, h = ctx
    v = np.zeros(8)
    p = v.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mag_set_load_cases(h, 0, p, p, 0) == MAG_ERR_BAD_ARGS
    assert L.mag_set_load_cases(h, -3, p, p, 0) == MAG_ERR_BAD_ARGS
    assert b"num_cases" in L.mag_last_error(h)
    assert L.mag_set_load_cases(h, 2, None, p, 0) == MAG_ERR_BAD_ARGS
    assert L.mag_set_load_cases(h, 2, p, None, 0) == MAG_ERR_BAD_ARGS
    assert L.mag_set_load_cases(None, 2, p, p, 0) == MAG_ERR_BAD_ARGS
    assert L.mag_run_cases(None) == MAG_ERR_BAD_ARGS
    r, st = _lib.Result(), _lib.Stats()
    assert L.mag_download_case(h, 0, None) == MAG_ERR_BAD_ARGS
    assert L.mag_download_case(h, -1, C.byref(r)) == MAG_ERR_BAD_ARGS
    assert L.mag_get_case_stats(h, 0, None) == MAG_ERR_BAD_ARGS
    assert L.mag_get_case_stats(h, -1, C.byref(st)) == MAG_ERR_BAD_ARGS
    assert L.mag_get_cases_info(h, None) == MAG_ERR_BAD_ARGS


def test_call_order_errors_before_any_hip_call(ctx):
    L, h = ctx
    v = np.zeros(8)
    p = v.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mag_set_load_cases(h, 2, p, p, 0) == MAG_ERR_STATE  # before mag_upload
    assert b"mag_upload" in L.mag_last_error(h)
    assert L.mag_run_cases(h) == MAG_ERR_STATE  # before mag_set_load_cases
    assert b"mag_set_load_cases" in L.mag_last_error(h)
    r, st, info = _lib.Result(), _lib.Stats(), (C.c_int32 * 4)()
    assert L.mag_download_case(h, 0, C.byref(r)) == MAG_ERR_STATE  # before a completed mag_run_cases
    assert L.mag_get_case_stats(h, 0, C.byref(st)) == MAG_ERR_STATE
    assert L.mag_get_cases_info(h, info) == MAG_ERR_STATE


def test_python_mirror_checks_shapes(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        c.N = 4
        with pytest.raises(MagnetiteError):
            c.set_load_cases(np.zeros((2, 7)), np.zeros((2, 7)))
        with pytest.raises(MagnetiteError):
            c.set_load_cases(np.zeros(8), np.zeros(8))
        with pytest.raises(MagnetiteError) as e:
            c.set_load_cases(np.zeros((2, 8)), np.zeros((2, 8)))  # shapes fine: the library answers (no upload yet)
        assert e.value.args and "mag_upload" in str(e.value)


def _kernel_meta(path):
    """{kernel symbol: (vgprs, sgpr spills, vgpr spills, scratch bytes)} from the metadata of an ISA listing."""
    txt = open(path).read()
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", txt)[1:]:
        g = lambda k: int(re.search(r"\." + k + r":\s*(\d+)", blk).group(1))
        name = re.search(r"\.name:\s*(\S+)", blk).group(1)
        out[name] = (g("vgpr_count"), g("sgpr_spill_count"), g("vgpr_spill_count"), g("private_segment_fixed_size"))
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to emit the ISA")
def test_load_case_instantiations_exist_and_pass_the_isa_lint(built):
    """The load-case code objects: one per shape (triangle walk; edge blocks with and without overflow: the single-workgroup
    kernel with one to four tiles, and one tile per workgroup), hazard-free in the emitted ISA like the others."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_lint
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "build/persist_cases.s"], stdout=subprocess.DEVNULL)
    path = os.path.join(CSRC, "build", "persist_cases.s")
    meta = _kernel_meta(path)
    # k_cg_persist<512, false, 512, EBM, ONE, NPTX, LC = true>: the load-case flag is the last template argument
    lc = [k for k in meta if "k_cg_persist" in k and k.endswith("ELb1EEEvNS_13PersistParamsE")]
    assert len(lc) == 11, sorted(meta)
    assert len(meta) == 11  # ... and nothing else in that object
    assert isa_lint.count_asm_stores(path) >= 11 * 4
    problems = isa_lint.lint(path)
    assert problems == [], "\n".join(problems[:20])
    for k in lc:
        assert meta[k][0] <= 256, (k, meta[k])
