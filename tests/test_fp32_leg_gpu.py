"""-m gpu: the fp32 CG leg (mag_options.precision = 1, cg_kernel == 4: k_cg_fused32, k_coords32, k_fused32_init,
k_x32_to_f64) against its float32 twin (tests/fp32_twin.py).

Operator probe.  The fp32 operator exists only fused inside the iteration kernel, so it is extracted through the ABI: on a
problem with zero prescribed displacements and a float32-exact load b, max_iter = 1 returns x1 = fl(alpha1 b) and max_iter = 2
returns x2 = x1 + alpha2 p2 with p2 in span{b, K b}.  d = x2 - x1 is fitted on {b, q_ref = K b (fp64)} by two global
coefficients, and what is left is measured entry by entry in units of float32 rounding (fp32_twin.probe_ratio).  Every bar is
4 x the spread of the twin's own float32 realisations (element order permuted, origin anywhere in the bounding box), computed
here on the CPU; test_fp32_twin.py asserts that seeded 1e-4 errors stand at least twice above that bar for every case.
"""
import numpy as np
import pytest

import fp32_cases as fc
import fp32_twin as tw
from magnetite_amd import Context, MagnetiteError, _lib
from magnetite_amd._lib import MAG_ERR_BAD_ARGS, MAG_STOP_REL, MAG_STOP_RNORM_SQ

pytestmark = pytest.mark.gpu

REFUSAL = "precision fp32 needs the LDS-halo operator and tile_nodes 256|512"


def fp32_solve(p, hist=0, **opts):
    with Context(device=0, precision=1, history_len=max(hist, 1), **opts) as c:
        out = c.solve(p)
        if hist:
            out["history"] = c.history(min(hist, out["iterations"]))
    assert out["cg_kernel"] == 4 and out["lds_operator"] == 1
    return out


def gpu_probe(name, tile):
    """(ratio, alpha deviation, stats of the two-iteration solve) of the kernel on one case of the matrix"""
    p = fc.problem(name)
    one = fp32_solve(p, tile_nodes=tile, max_iter=1)
    two = fp32_solve(p, tile_nodes=tile, max_iter=2)
    assert one["iterations"] == 1 and two["iterations"] == 2 and two["best_iteration"] == 2  # d = alpha2 p2
    assert two["termination"] == _lib.MAG_TERM_MAX_ITERS and two["best_param_mismatch"] == 0
    known = p.u_known == 1
    assert not one["u"][known].any() and not two["u"][known].any()
    return fc.probe(name, one["u"], two["u"]) + (two,)


@pytest.mark.parametrize("name,tile", fc.matrix())
def test_operator_probe(built, name, tile, monkeypatch):
    if name in fc.GRID_CAP:
        monkeypatch.setenv("MAG_TUNE_GRID", str(fc.GRID_CAP[name]))  # every workgroup walks two or three tiles
    fam = fc.family_probe(name)
    assert all(f[2] == 2 for f in fam)
    bar, alpha_bar = fc.bars(name)
    ratio, alpha_dev, st = gpu_probe(name, tile)
    print(f"[fp32 probe] {name} tile {tile}: ratio {ratio:.2f} (family max {bar / 4:.2f}), alpha1 deviation {alpha_dev:.2e} "
          f"(family max {alpha_bar / 4:.2e}); tiles {st['num_tiles']}, max halo {st['max_tile_halo']}")
    if name in fc.GRID_CAP:
        assert st["num_tiles"] >= 2 * fc.GRID_CAP[name]
    if name in fc.HALO_OVER_TILE:
        assert st["max_tile_halo"] > tile  # the hh >= B branch: more halo nodes than threads
    if name == "plate24_shuffled":
        assert st["num_tiles"] * tile > fc.problem(name).mesh.num_nodes > (st["num_tiles"] - 1) * tile  # ragged last tile
    assert ratio <= bar, (ratio, bar)
    assert alpha_dev <= alpha_bar, (alpha_dev, alpha_bar)


@pytest.mark.parametrize("tile", fc.TILES)
@pytest.mark.parametrize("name", ["hole_perturbed", "plate24_shuffled"])
def test_history_follows_fp64_within_the_family_spread(built, name, tile):
    p, ref = fc.full_problem(name), fc.full_reference(name)
    bar, spread = fc.history_bar(name)
    out = fp32_solve(p, hist=fc.HISTORY, tile_nodes=tile, max_iter=fc.HISTORY)
    assert out["iterations"] == fc.HISTORY
    dev = tw.history_dev(out["history"], ref["history"][:fc.HISTORY])
    print(f"[fp32 history] {name} tile {tile}: largest deviation {dev.max():.2e} (family {spread.max():.2e}), "
          f"largest deviation / bar {np.max(dev / bar):.2f}")
    assert len(dev) == fc.HISTORY and np.all(dev <= bar), (dev, bar)


@pytest.mark.parametrize("tile", fc.TILES)
def test_end_to_end_error_is_the_family_s(built, tile):
    name = "plate24_shuffled"
    p, ref = fc.full_problem(name), fc.full_reference(name)
    fam = fc.family_solves(name, tw.STOP_REL, 1e-7)
    assert all(s["converged"] for s in fam)
    worst = max(fc.rel(s["u"], ref["u"]) for s in fam)
    out = fp32_solve(p, tile_nodes=tile, stop_mode=MAG_STOP_REL, tol=1e-7)
    err = fc.rel(out["u"], ref["u"])
    print(f"[fp32 end to end] {name} tile {tile}: rel(u, u64) {err:.2e} (family max {worst:.2e}), {out['iterations']} iterations "
          f"(family {min(s['iterations'] for s in fam)}-{max(s['iterations'] for s in fam)})")
    assert out["converged"] == 1
    assert err <= 4.0 * worst, (err, worst)
    k = p.u_known == 1
    assert np.array_equal(out["u"][k], p.u_in[k])


def test_repeated_solves_and_host_options_give_the_same_bits(built):
    """two solves on one context; check_every = 2 and use_graph = 0: the stop test is in the kernel, so the host's polling
    interval and the graph replay change neither the bits nor the history"""
    p = fc.full_problem("plate24_shuffled")
    n = 64
    with Context(device=0, precision=1, stop_mode=MAG_STOP_REL, tol=1e-7, history_len=n) as c:
        a = c.solve(p)
        ha = c.history(n)
        b = c.solve(p)
        hb = c.history(n)
    assert a["cg_kernel"] == b["cg_kernel"] == 4 and a["converged"] == 1 and a["iterations"] == b["iterations"] > n
    assert np.array_equal(a["u"], b["u"]) and np.array_equal(a["f"], b["f"]) and np.array_equal(ha, hb)
    for kw in (dict(check_every=2), dict(use_graph=0)):
        with Context(device=0, precision=1, stop_mode=MAG_STOP_REL, tol=1e-7, history_len=n, **kw) as c:
            o = c.solve(p)
            ho = c.history(n)
        assert o["cg_kernel"] == 4 and o["iterations"] == a["iterations"] and o["final_cost"] == a["final_cost"], kw
        assert np.array_equal(o["u"], a["u"]) and np.array_equal(ho, ha), kw


def test_iteration_cap_returns_best_param_in_fp32(built):
    """as test_iteration_cap_returns_best_param_like_argmin: the repeat up to best_iteration must reproduce the fp32 kernel's
    own bits"""
    p = fc.full_problem("plate_shuffled")
    cap = 50
    with Context(device=0, precision=1, max_iter=cap, history_len=cap) as c:
        out = c.solve(p)
        hist = c.history(cap)
    assert out["cg_kernel"] == 4
    assert out["converged"] == 0 and out["termination"] == _lib.MAG_TERM_MAX_ITERS and out["iterations"] == cap
    assert out["best_iteration"] == int(np.argmin(hist)) + 1
    assert out["best_param_mismatch"] == 0
    assert out["final_cost"] == hist[out["best_iteration"] - 1]
    fam = fc.family_solves("plate_shuffled", tw.STOP_RNORM, 1e-4, cap)
    assert out["best_iteration"] in {s["best_iteration"] for s in fam}


def test_zero_rhs_returns_zero_in_fp32(built):
    from magnetite_amd import meshgen
    p = meshgen.apply_boundary_rules(meshgen.plate(6), [meshgen.BoundaryRule("r", x_max=1e-9, ux=0.0, uy=0.0)])
    out = fp32_solve(p)
    assert out["iterations"] == 0 and np.all(out["u"] == 0.0)


@pytest.mark.parametrize("mode,twin_mode", [(MAG_STOP_RNORM_SQ, tw.STOP_RNORM_SQ), (_lib.MAG_STOP_RNORM, tw.STOP_RNORM)])
def test_stop_rules_stop_where_the_family_does(built, mode, twin_mode):
    name = "plate24_shuffled"
    fam = fc.family_solves(name, twin_mode, 1e-4)
    assert all(s["converged"] for s in fam)
    lo, hi = min(s["iterations"] for s in fam), max(s["iterations"] for s in fam)
    out = fp32_solve(fc.full_problem(name), stop_mode=mode)
    print(f"[fp32 stop rule {mode}] {out['iterations']} iterations, family {lo}-{hi}")
    assert out["converged"] == 1
    assert lo - max(3, lo // 50) <= out["iterations"] <= hi + max(3, hi // 50)


def test_refusals_leave_the_context_usable(built):
    """tile 1024, the gather operator (asked for, or forced by a hub whose halo does not fit the LDS image) have no fp32
    kernel: MAG_ERR_BAD_ARGS, and the context goes on working"""
    from magnetite_amd import meshgen
    small, ref = fc.full_problem("plate12"), fc.full_reference("plate12")
    worst = max(fc.rel(s["u"], ref["u"]) for s in fc.family_solves("plate12", tw.STOP_REL, 1e-7))
    hub = meshgen.apply_boundary_rules(fc.hub_mesh(3000, 1), [meshgen.BoundaryRule("hold", x_max=-1.2, ux=0.0, uy=0.0),
                                                              meshgen.BoundaryRule("pull", x_min=1.2, ux=0.01, fy=0.0)])
    for kw, prob in ((dict(tile_nodes=1024), small), (dict(op_variant=1), small), (dict(), hub)):
        with Context(device=0, precision=1, stop_mode=MAG_STOP_REL, tol=1e-7, **kw) as c:
            with pytest.raises(MagnetiteError) as ei:
                c.solve(prob)
            assert ei.value.code == MAG_ERR_BAD_ARGS and REFUSAL in str(ei.value), kw
            if kw:  # the options are the context's: it refuses again, and everything but the fp32 CG still works
                with pytest.raises(MagnetiteError) as again:
                    c.solve(small)
                assert again.value.code == MAG_ERR_BAD_ARGS and REFUSAL in str(again.value), kw
                x = np.random.default_rng(1).standard_normal(2 * small.mesh.num_nodes)
                assert fc.rel(c.apply_operator(x, masked=False), fc.Csr64(small).matvec(x)) < 1e-12
            else:   # refused for the mesh: the same context then solves plate(12)
                out = c.solve(small)
                assert out["cg_kernel"] == 4 and out["converged"] == 1
                assert fc.rel(out["u"], ref["u"]) <= 4.0 * worst
