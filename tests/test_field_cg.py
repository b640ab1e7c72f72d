"""mag_options.field_cg without a GPU: the numpy twin of the fused block-row CG stands on its own feet (it lands on the direct
solve, its plain form starts on textbook CG's residual history, its inverse blocks invert the masked diagonal blocks, its row
order is what it says), and the option sits where the header puts it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import field_cg_ref as fref
from magnetite_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "magnetite_hip.h")

CASES = [
    ("plate_6x5", "pull", "random"), ("plate_6x5", "rollers", "two-phase"), ("frontal16", "rollers", "random"),
    ("frontal16", "pull", "two-phase"), ("frontal32s", "pull", "two-phase"), ("plate_40x24", "cantilever", "random"),
]


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


@pytest.mark.parametrize("kind", [1, 2, 3])
@pytest.mark.parametrize("name,bc,which", CASES)
def test_the_twin_lands_on_the_direct_solve(name, bc, which, kind):
    """the bars of the device's solve: true residual <= 10 tol |b|, u in rel-L2 <= cond(K_ff) 10 tol"""
    tol = 1e-12
    prob, sol = fref.problem(name, bc), fref.direct(name, bc, which)
    out = fref.twin_run(name, bc, which, kind, tol)
    assert out["converged"] == 1
    x = out["x"][sol["free"]]
    assert np.linalg.norm(sol["Kff"] @ x - sol["b"]) <= 10 * tol * np.linalg.norm(sol["b"])
    assert rel(x, sol["u"][sol["free"]]) <= sol["cond"] * 10 * tol
    assert np.all(out["x"][prob.u_known == 1] == 0.0)  # nothing moves on a prescribed DOF


@pytest.mark.parametrize("name,bc,which", CASES[:4])
def test_the_plain_form_starts_on_textbook_cg(name, bc, which):
    """the expanded numerator of beta restarts from the true r.r every launch: the first 15 costs are textbook CG's to 1e-9"""
    sol = fref.direct(name, bc, which)
    out = fref.twin_run(name, bc, which, 1, 1e-12, hist_len=15)
    want = fref.textbook_cg_history(sol["Kff"], sol["b"], 15)
    assert np.allclose(out["history"][:15], want, rtol=1e-9), np.max(np.abs(out["history"][:15] / want - 1))


@pytest.mark.parametrize("kind", [2, 3])
@pytest.mark.parametrize("name,bc,which", CASES[:4])
def test_the_inverse_blocks_invert_the_masked_diagonal_blocks(name, bc, which, kind):
    """fp32 rounding of three entries of a 2x2 inverse: M Minv = I within 4 * 2^-24 * cond(block) on the free DOFs; a prescribed
    DOF has neither row nor column in Minv"""
    prob, sol = fref.problem(name, bc), fref.direct(name, bc, which)
    minv = fref.inverse_blocks(sol["K"], prob.u_known, kind).astype(np.float64)
    for g in range(len(minv)):
        free = [d for d in (0, 1) if not prob.u_known[2 * g + d]]
        M = sol["K"][2 * g:2 * g + 2, 2 * g:2 * g + 2]
        if kind == 2:
            M = np.diag(np.diag(M))
        Mi = np.array([[minv[g, 0], minv[g, 1]], [minv[g, 1], minv[g, 2]]])
        for d in (0, 1):
            if d not in free:
                assert Mi[d, 0] == 0.0 and Mi[0, d] == 0.0 and Mi[d, 1] == 0.0 and Mi[1, d] == 0.0
        if len(free) < 2 or kind == 2:
            for d in free:
                assert abs(M[d, d] * Mi[d, d] - 1.0) <= 2.0 ** -23
            if free and kind == 3:
                assert Mi[0, 1] == 0.0
        else:
            assert np.abs(M @ Mi - np.eye(2)).max() <= 4 * 2.0 ** -24 * np.linalg.cond(M)


def test_the_row_order_is_the_diagonal_then_ascending_position():
    prob, sol = fref.problem("frontal16", "pull"), fref.direct("frontal16", "pull", "random")
    N = prob.mesh.num_nodes
    rowptr, col = fref.block_pattern(prob.mesh.conn, N)
    position = np.random.default_rng(11).permutation(N)
    rows = fref.row_order(rowptr, col, position)
    assert max(len(r) for r in rows) == 9
    for i, r in enumerate(rows):
        assert r[0] == i and sorted(r) == sorted(int(c) for c in col[rowptr[i]:rowptr[i + 1]])
        assert all(position[a] < position[b] for a, b in zip(r[1:], r[2:]))
    v = np.random.default_rng(12).standard_normal(2 * N)
    q = fref.row_sum_in_table_order(sol["K"], rows, v)
    assert rel(q, sol["K"] @ v) <= 1e-13  # the pattern holds all of K's row, in whatever order


def test_the_option_defaults_to_off():
    o = _lib.Options()
    _lib.lib().mag_default_options(C.byref(o))
    assert o.field_cg == 0
    assert (_lib.MAG_FIELD_CG_PLAIN, _lib.MAG_FIELD_CG_JACOBI, _lib.MAG_FIELD_CG_BLOCK_JACOBI) == (1, 2, 3)


def test_the_option_sits_at_the_headers_offset():
    """mag_options in include/magnetite_hip.h: fifteen 4-byte words, one double and one int64 -- field_cg is the last word, where
    `reserved` was"""
    text = open(HEADER).read()
    body = re.search(r"typedef struct mag_options \{(.*?)\} mag_options;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"\b(int32_t|int64_t|double)\s+(\w+)\s*;", body)]
    size = {"int32_t": 4, "int64_t": 8, "double": 8}
    off, offsets = 0, {}
    for t, n in fields:
        off = (off + size[t] - 1) // size[t] * size[t]
        offsets[n] = off
        off += size[t]
    assert "reserved" not in offsets and fields[-1] == ("int32_t", "field_cg")
    assert [n for n, _ in _lib.Options._fields_] == [n for _, n in fields]
    assert _lib.Options.field_cg.offset == offsets["field_cg"] == 68 and _lib.Options.field_cg.size == 4
    assert C.sizeof(_lib.Options) == 72


def test_an_unknown_option_is_refused_before_anything_is_created():
    from magnetite_amd import Context
    for bad in ("field_gc", "_fields_", "reserved"):
        with pytest.raises(TypeError):
            Context(**{bad: 1})
