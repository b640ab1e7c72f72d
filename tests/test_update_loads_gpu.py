"""-m gpu: the four-slot structured on-chip CG kernel with its update loads in flight under the scalars (persist_kernel.h,
persist_update_loads; tests/test_update_loads_isa.py looks at the ISA) on small meshes.

MAG_TUNE_PERSIST_K=4 with MAG_TUNE_PERSIST_MIN_K=1 puts a mesh of a few 512-node tiles on the four-slot instantiation
k_cg_persist<512, false, 512, 1>, which otherwise only meshes of 769 tiles and more run:

  plate-4-live  plate(63, 63): 4096 nodes = 8 tiles, two workgroups, every node slot live
  holes-4       plate_with_holes(96): a tile count that is no multiple of four -- the last workgroup has dead slots, which the
                kernel now updates like live ones, on zeros
  capped        holes-4 with max_iter = 25: the loop is left with loads in flight; against the same build's streaming kernels
                (cg_variant = 1) at the same cap

(The overflow kernel k_cg_persist<512, false, 512, 2> keeps its update phase -- DESIGN UB -- and has no case here.)

Against the oracle with the bars of tests/test_walk_gathers_gpu.py: u, f and stress to 1e-8 relative L2, the iteration count
within max(3, it // 50); each case twice for the same bits."""
import numpy as np
import pytest

import oracle
from magnetite_amd import Context, _lib, meshgen

pytestmark = pytest.mark.gpu

TOL = 1e-8  # north_star: relative L2 on nodal displacements
CAP = 25


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _problem(case):
    mesh = meshgen.plate(63, 63) if case == "plate-4-live" else meshgen.plate_with_holes(96)
    return meshgen.config_fixed_left_pull_right(mesh)


@pytest.fixture(scope="module")
def reference():
    refs = {}

    def get(case):
        if case not in refs:
            p = _problem(case)
            refs[case] = (p, oracle.run(p.xy_flat, p.conn_flat, p.u_known, p.u_in, p.f_in, p.youngs_modulus, p.poisson_ratio,
                                        p.part_thickness, path="sparse"))
        return refs[case]
    return get


def _four_slots(st):
    return st["cg_kernel"] == 2 and st["persist_timeout"] == 0 and st["tiles_per_workgroup"] == 4 and st["edge_blocks"] == 1


@pytest.mark.parametrize("case", ["plate-4-live", "holes-4"])
def test_four_slot_kernel_with_update_loads_in_flight(built, case, reference, monkeypatch):
    p, ref = reference(case)
    tiles = (p.mesh.num_nodes + 511) // 512
    if case == "plate-4-live":
        assert p.mesh.num_nodes == 4096 and tiles == 8
    else:
        assert tiles % 4 != 0, tiles
    monkeypatch.setenv("MAG_TUNE_PERSIST_MIN_K", "1")
    monkeypatch.setenv("MAG_TUNE_PERSIST_K", "4")
    with Context(device=0, tile_nodes=512) as c:
        out = c.solve(p)
        st = c.stats()
        again = c.solve(p)
        st_again = c.stats()
    assert _four_slots(st) and _four_slots(st_again), (case, st, st_again)
    assert out["converged"] == 1 and abs(out["iterations"] - ref["iterations"]) <= max(3, ref["iterations"] // 50), case
    for key in ("u", "f", "stress"):
        print(case, key, rel(out[key], ref[key]))
        assert rel(out[key], ref[key]) <= TOL, (case, key)
    assert np.array_equal(out["u"], again["u"])  # bitwise reproducible


def test_capped_solve_leaves_the_loop_with_loads_in_flight(built, monkeypatch):
    p = _problem("holes-4")
    monkeypatch.setenv("MAG_TUNE_PERSIST_MIN_K", "1")
    monkeypatch.setenv("MAG_TUNE_PERSIST_K", "4")
    with Context(device=0, tile_nodes=512, max_iter=CAP) as c:
        out = c.solve(p)
        st = c.stats()
        again = c.solve(p)
        st_again = c.stats()
    with Context(device=0, tile_nodes=512, max_iter=CAP, cg_variant=1) as c:
        streaming = c.solve(p)
    assert _four_slots(st) and _four_slots(st_again), (st, st_again)
    assert streaming["cg_kernel"] != 2, streaming["cg_kernel"]
    assert out["converged"] == 0 and out["termination"] == _lib.MAG_TERM_MAX_ITERS
    assert streaming["termination"] == _lib.MAG_TERM_MAX_ITERS and out["iterations"] == streaming["iterations"] == CAP
    print("capped u", rel(out["u"], streaming["u"]))
    assert rel(out["u"], streaming["u"]) <= TOL
    assert np.array_equal(out["u"], again["u"])
