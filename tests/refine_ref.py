"""The numpy twin of mag_run_refine, written from the specification in include/magnetite_hip.h: longest-edge refinement with
conformity closure (Rivara) with the header's numbering of edges, new nodes and children, so that every array can be compared
with the device's exactly.  Vectorised; the closure is swept Jacobi-wise (every sweep reads the flags the previous one left),
which is the largest number of sweeps any order of a sweep can need.  Also the mesh checks the tests share."""
import math

import numpy as np

from magnetite_amd.meshgen import Mesh

RULES = ("marks", "max_fraction", "top_fraction")
INFO = ("nodes", "elements", "marked", "marked_edges", "sweeps", "split2", "split3", "split4")


def edge_table(conn, N):
    """eid (E, 3): the id of local edge k = (conn[e, k], conn[e, (k + 1) % 3]); lo, hi of every edge id."""
    a = conn.astype(np.int64)
    b = np.roll(a, -1, axis=1)
    key = (np.minimum(a, b) << 32) | np.maximum(a, b)
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    return inv.reshape(-1, 3), uniq >> 32, uniq & 0xFFFFFFFF


def longest_edges(xy, eid, lo, hi):
    """L (E): the local edge of largest len2, on a tie the smaller edge id."""
    dx, dy = xy[hi, 0] - xy[lo, 0], xy[hi, 1] - xy[lo, 1]
    len2 = dx * dx + dy * dy
    rows = np.arange(len(eid))
    L = np.zeros(len(eid), dtype=np.int64)
    for k in (1, 2):
        lk, lL = len2[eid[:, k]], len2[eid[rows, L]]
        L = np.where((lk > lL) | ((lk == lL) & (eid[:, k] < eid[rows, L])), k, L)
    return L


def mark_elements(E, marks=None, indicator=None, rule="top_fraction", theta=0.2):
    if marks is not None:
        return np.asarray(marks).reshape(-1) != 0
    ind = np.asarray(indicator, dtype=np.float64).reshape(-1)
    if not (np.isfinite(ind) & (ind >= 0)).all():
        raise ValueError("indicator[%d] is not finite and >= 0" % int(np.flatnonzero(~(np.isfinite(ind) & (ind >= 0)))[0]))
    out = np.zeros(E, dtype=bool)
    if rule == "max_fraction":
        top = ind.max()
        return ind >= theta * top if top > 0 else out
    assert rule == "top_fraction"
    k = min(max(int(math.ceil(theta * float(E))), 1), E)
    key = ~(ind + 0.0).view(np.uint64)
    out[np.argsort(key, kind="stable")[:k]] = True
    return out


def refine(xy, conn, u_known, u_in, f_in, marks=None, indicator=None, rule="top_fraction", theta=0.2, split=1):
    """dict(xy, conn, u_known, u_in, f_in, node_parents, elem_parent and the info words by name; sweeps: the Jacobi count)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    conn = np.asarray(conn, dtype=np.int32).reshape(-1, 3)
    u_known = np.asarray(u_known, dtype=np.uint8).reshape(-1)
    u_in, f_in = np.asarray(u_in, dtype=np.float64).reshape(-1), np.asarray(f_in, dtype=np.float64).reshape(-1)
    N, E = len(xy), len(conn)
    rows = np.arange(E)
    eid, lo, hi = edge_table(conn, N)
    L = longest_edges(xy, eid, lo, hi)
    longest = eid[rows, L]
    marked = mark_elements(E, marks, indicator, rule, theta)
    flag = np.zeros(len(lo), dtype=bool)
    flag[longest[marked]] = True
    if split == 3:
        flag[eid[marked].reshape(-1)] = True
    sweeps = 0
    while True:
        sweeps += 1
        new = flag[eid].any(axis=1) & ~flag[longest]
        if not new.any():
            break
        flag[longest[new]] = True
    # new nodes: marked edge number r in edge-id order is node N + r
    mid = np.where(flag, N + np.cumsum(flag) - 1, -1)
    plo, phi = lo[flag], hi[flag]
    added = len(plo)
    new_xy = np.vstack([xy, np.column_stack([0.5 * (xy[plo, 0] + xy[phi, 0]), 0.5 * (xy[plo, 1] + xy[phi, 1])])])
    known = np.zeros((N + added, 2), dtype=np.uint8)
    nu_in, nf_in = np.zeros((N + added, 2)), np.zeros((N + added, 2))
    known[:N], nu_in[:N], nf_in[:N] = u_known.reshape(-1, 2), u_in.reshape(-1, 2), f_in.reshape(-1, 2)
    k2, u2 = u_known.reshape(-1, 2), u_in.reshape(-1, 2)
    both = (k2[plo] != 0) & (k2[phi] != 0)
    known[N:] = both
    nu_in[N:] = np.where(both, 0.5 * (u2[plo] + u2[phi]), 0.0)
    # new elements: rotated so that the longest edge comes first
    k1, k2_ = (L + 1) % 3, (L + 2) % 3
    p, q, r = conn[rows, L], conn[rows, k1], conn[rows, k2_]
    M, A, B = mid[eid[rows, L]], mid[eid[rows, k1]], mid[eid[rows, k2_]]
    assert ((M >= 0) | ((A < 0) & (B < 0))).all()  # the closure: a marked edge implies a marked longest edge
    cnt = 1 + (M >= 0) + (A >= 0) + (B >= 0)
    off = np.concatenate([[0], np.cumsum(cnt)])
    new_conn = np.empty((off[-1], 3), dtype=np.int32)

    def put(mask, at, a, b, c):
        new_conn[at[mask]] = np.column_stack([a[mask], b[mask], c[mask]])

    at = off[:-1].copy()
    whole = M < 0
    put(whole, at, conn[:, 0], conn[:, 1], conn[:, 2])
    put(~whole & (B >= 0), at, p, M, B)
    put(~whole & (B >= 0), at + 1, B, M, r)
    put(~whole & (B < 0), at, p, M, r)
    at = at + np.where(B >= 0, 2, 1)
    put(~whole & (A >= 0), at, M, q, A)
    put(~whole & (A >= 0), at + 1, M, A, r)
    put(~whole & (A < 0), at, M, q, r)
    out = dict(xy=new_xy, conn=new_conn, u_known=known.reshape(-1), u_in=nu_in.reshape(-1), f_in=nf_in.reshape(-1),
               node_parents=np.column_stack([plo, phi]).astype(np.int32).reshape(-1, 2), elem_parent=np.repeat(rows, cnt).astype(np.int32))
    out.update(zip(INFO, (N + added, int(off[-1]), int(marked.sum()), added, sweeps, int((cnt == 2).sum()), int((cnt == 3).sum()),
                          int((cnt == 4).sum()))))
    return out


def of_problem(prob, **kw):
    return refine(prob.mesh.xy, prob.mesh.conn, prob.u_known, prob.u_in, prob.f_in, **kw)


def free_mesh(mesh, **kw):
    """The twin on a mesh without boundary data."""
    n = 2 * len(mesh.xy)
    return refine(mesh.xy, mesh.conn, np.zeros(n, dtype=np.uint8), np.zeros(n), np.zeros(n), **kw)


# ---- meshes and checks the tests share
def tie_strip(n):
    """Bottom nodes (i, 0), top nodes (i + 0.5, 2), i = 0..n; triangles (b_i, b_i+1, t_i) and (b_i+1, t_i+1, t_i): every slanted
    edge has len2 = 4.25 exactly, so only the tie rule orders them -- and the closure runs the length of the strip."""
    i = np.arange(n + 1, dtype=np.float64)
    xy = np.vstack([np.column_stack([i, 0 * i]), np.column_stack([i + 0.5, 0 * i + 2.0])])
    b, t = np.arange(n), np.arange(n) + n + 1
    conn = np.empty((2 * n, 3), dtype=np.int32)
    conn[0::2] = np.column_stack([b, b + 1, t])
    conn[1::2] = np.column_stack([b + 1, t + 1, t])
    return Mesh(xy, conn, f"tie_strip{n}")


def signed_area2(xy, conn):
    p, q, r = xy[conn[:, 0]], xy[conn[:, 1]], xy[conn[:, 2]]
    return (q[:, 0] - p[:, 0]) * (r[:, 1] - p[:, 1]) - (r[:, 0] - p[:, 0]) * (q[:, 1] - p[:, 1])


def min_angle_deg(xy, conn):
    m = np.pi
    for k in range(3):
        p, q, r = xy[conn[:, k]], xy[conn[:, (k + 1) % 3]], xy[conn[:, (k + 2) % 3]]
        u, v = q - p, r - p
        c = (u * v).sum(1) / np.sqrt((u * u).sum(1) * (v * v).sum(1))
        m = min(m, np.arccos(np.clip(c, -1, 1)).min())
    return np.degrees(m)


def once_used_edges(conn):
    """The undirected edges (keys lo << 32 | hi) that one element only has."""
    a = conn.astype(np.int64)
    b = np.roll(a, -1, axis=1)
    key, count = np.unique(((np.minimum(a, b) << 32) | np.maximum(a, b)).reshape(-1), return_counts=True)
    return key[count == 1]


def assert_conforming(conn, coarse=None, node_parents=None):
    """Every directed edge is unique and every undirected edge occurs at most twice.  With the coarse mesh and the parents of
    the new nodes: no hanging node -- a new node on an edge that one coarse element had adds one once-used edge, a new node on
    a shared edge none; a node hanging on an element that was not split would leave that element's whole edge and the two
    halves once-used, three more."""
    a = conn.astype(np.int64)
    b = np.roll(a, -1, axis=1)
    directed = ((a << 32) | b).reshape(-1)
    assert len(np.unique(directed)) == len(directed)
    _, count = np.unique(((np.minimum(a, b) << 32) | np.maximum(a, b)).reshape(-1), return_counts=True)
    assert count.max() <= 2
    if coarse is not None:
        before = once_used_edges(coarse)
        par = node_parents.astype(np.int64)
        on_boundary = np.isin((par[:, 0] << 32) | par[:, 1], before)
        assert len(once_used_edges(conn)) == len(before) + int(on_boundary.sum())
