"""CPU: the design-variant entry points (mag_set_variants ... mag_get_variants_info, mag_assemble_csr_variant) exist in header,
binding and library; their argument and call-order errors come back before any HIP call -- on a context that has no GPU at
all --; the Python mirror checks shapes; the variant form of the on-chip kernel has its own code objects."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from magnetite_amd import _lib
from test_load_cases import _kernel_meta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "magnetite_amd", "csrc")
NAMES = ("mag_set_variants", "mag_run_variants", "mag_download_variant", "mag_get_variant_stats", "mag_get_variants_info",
         "mag_assemble_csr_variant")
MAG_ERR_BAD_ARGS, MAG_ERR_STATE = 1, 7


def test_symbols_in_header_binding_and_library(built):
    header = open(os.path.join(ROOT, "include", "magnetite_hip.h")).read()
    L = _lib.lib()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.SYMBOLS
        assert getattr(L, name).argtypes is not None
    assert L.mag_version() == 4  # new entry points only: the version and every struct stay
    assert "MAG_ABI_VERSION 4" in header


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
    m = np.array([[7e10, 0.3, 0.01], [7e10, 1.0, 0.01]])
    pm = m.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mag_set_variants(h, 0, p, None, None, None, 0) == MAG_ERR_BAD_ARGS
    assert L.mag_set_variants(h, -2, p, None, None, None, 0) == MAG_ERR_BAD_ARGS
    assert b"num_variants" in L.mag_last_error(h)
    assert L.mag_set_variants(h, 2, None, None, None, None, 0) == MAG_ERR_BAD_ARGS  # everything NULL
    assert b"at least one" in L.mag_last_error(h)
    assert L.mag_set_variants(h, 2, p, None, p, None, 0) == MAG_ERR_BAD_ARGS  # the value pair comes together
    assert L.mag_set_variants(h, 2, p, None, None, p, 0) == MAG_ERR_BAD_ARGS
    assert L.mag_set_variants(h, 2, None, pm, None, None, 0) == MAG_ERR_BAD_ARGS  # nu = 1 in variant 1: mag_upload's check
    assert b"variant 1" in L.mag_last_error(h) and b"poisson" in L.mag_last_error(h)
    assert L.mag_set_variants(None, 2, p, None, None, None, 0) == MAG_ERR_BAD_ARGS
    assert L.mag_run_variants(None) == MAG_ERR_BAD_ARGS
    r, st = _lib.Result(), _lib.Stats()
    assert L.mag_download_variant(h, 0, None) == MAG_ERR_BAD_ARGS
    assert L.mag_download_variant(h, -1, C.byref(r)) == MAG_ERR_BAD_ARGS
    assert L.mag_get_variant_stats(h, 0, None) == MAG_ERR_BAD_ARGS
    assert L.mag_get_variant_stats(h, -1, C.byref(st)) == MAG_ERR_BAD_ARGS
    assert L.mag_get_variants_info(h, None) == MAG_ERR_BAD_ARGS


def test_call_order_errors_before_any_hip_call(ctx):
    L, h = ctx
    v = np.zeros(8)
    p = v.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mag_set_variants(h, 2, p, None, None, None, 0) == MAG_ERR_STATE  # before mag_upload
    assert b"mag_upload" in L.mag_last_error(h)
    assert L.mag_run_variants(h) == MAG_ERR_STATE  # before mag_set_variants
    assert b"mag_set_variants" in L.mag_last_error(h)
    r, st, info, nnz = _lib.Result(), _lib.Stats(), (C.c_int32 * 4)(), C.c_int64(0)
    assert L.mag_download_variant(h, 0, C.byref(r)) == MAG_ERR_STATE  # before a completed mag_run_variants
    assert L.mag_get_variant_stats(h, 0, C.byref(st)) == MAG_ERR_STATE
    assert L.mag_get_variants_info(h, info) == MAG_ERR_STATE
    assert L.mag_assemble_csr_variant(h, 0, C.byref(nnz), None, None, None) == MAG_ERR_STATE
    assert L.mag_run_cases(h) == MAG_ERR_STATE  # the load-case entry points answer as before


def test_python_mirror_checks_shapes(built):
    from magnetite_amd import Context
    from magnetite_amd.solver import MagnetiteError
    with Context() as c:
        c.N = 4
        with pytest.raises(MagnetiteError):
            c.set_variants(xy=np.zeros((2, 7)))
        with pytest.raises(MagnetiteError):
            c.set_variants(material=np.zeros((2, 2)))
        with pytest.raises(MagnetiteError):
            c.set_variants(u_in=np.zeros((2, 8)))  # without f_in
        with pytest.raises(MagnetiteError):
            c.set_variants(xy=np.zeros((2, 8)), material=np.ones((3, 3)) * 0.3)  # two counts
        with pytest.raises(MagnetiteError) as e:
            c.set_variants()  # nothing given: the library answers
        assert e.value.code == MAG_ERR_BAD_ARGS
        with pytest.raises(MagnetiteError) as e:
            c.set_variants(xy=np.zeros((2, 4, 2)), material=np.full((2, 3), 0.3))  # shapes fine (no upload yet)
        assert e.value.code == MAG_ERR_STATE and "mag_upload" in str(e.value)
        for call in (c.run_variants, c.variants_info, lambda: c.variant_stats(0), lambda: c.download_variant(0)):
            with pytest.raises(MagnetiteError) as e:
                call()
            assert e.value.code == MAG_ERR_STATE


def test_variant_helpers_keep_orientation_and_ranges():
    from magnetite_amd import meshgen
    from variants_util import keeps_orientation, make_variants, shortest_edge
    prob = meshgen.config_fixed_left_pull_right(meshgen.shuffle(meshgen.plate_with_holes(24), 3))
    xy, mat, u, f = make_variants(prob, 9, seed=1)
    h = shortest_edge(prob.mesh.xy, prob.mesh.conn)
    assert np.array_equal(xy[0], prob.xy_flat)
    assert np.abs(xy - prob.xy_flat).max() <= 0.2 * h * (1 + 1e-12)
    assert all(keeps_orientation(prob, x) for x in xy)
    assert (mat[:, 1] >= 0.2).all() and (mat[:, 1] <= 0.4).all()
    assert (mat[:, 0] >= 0.5 * prob.youngs_modulus).all() and (mat[:, 0] <= 2 * prob.youngs_modulus).all()
    turned = xy[3].reshape(-1, 2).copy()
    a, b, c = prob.mesh.conn[5]
    turned[a] = turned[b] + turned[c] - turned[a]
    assert not keeps_orientation(prob, turned.reshape(-1))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to emit the ISA")
def test_variant_instantiations_exist_spill_free_and_pass_the_isa_lint(built):
    """One variant code object per load-case shape, in an object of their own; no VGPR spill, no scratch; hazard-free stores."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import isa_lint
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC, "build/persist_variants.s"], stdout=subprocess.DEVNULL)
    path = os.path.join(CSRC, "build", "persist_variants.s")
    meta = _kernel_meta(path)
    # k_cg_persist<512, false, 512, EBM, ONE, NPTX, VAR = true, LC = true>
    var = [k for k in meta if "k_cg_persist" in k and k.endswith("ELb1ELb1EEEvNS_13PersistParamsE")]
    assert len(var) == 11 and len(meta) == 11, sorted(meta)
    for k in var:
        vgprs, _, vgpr_spills, scratch = meta[k]
        assert vgprs <= 256 and vgpr_spills == 0 and scratch == 0, (k, meta[k])
    assert isa_lint.count_asm_stores(path) >= 11 * 4
    problems = isa_lint.lint(path)
    assert problems == [], "\n".join(problems[:20])
