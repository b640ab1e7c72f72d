"""-m gpu: the four-slot edge-block kernels with their walks' gathers pinned in groups (cg_device.h, ring_walk_blocks;
tests/test_walk_gathers_isa.py looks at the ISA) on small meshes.

MAG_TUNE_PERSIST_K=4 with MAG_TUNE_PERSIST_MIN_K=1 puts a mesh of a few tiles on the four-slot instantiations, which
otherwise only meshes of 769 tiles and more run:

  structured  plate_with_holes(96): about 18 tiles, so five workgroups, the last one with two live slots -- the path that
              runs all four slots as one block and the path with a test per slot; k_cg_persist<512, false, 512, 1>
  overflow    frontal_like(100, 0.4, 3): rows of seven and more entries, the blocks beyond six in the LDS pool;
              k_cg_persist<512, false, 512, 2>

Against the oracle with the bars of test_gpu_parity.py's
test_on_chip_edge_blocks_with_overflow_match_the_oracle_and_the_triangle_walk, against the one-slot kernel (the same solve
without MAG_TUNE_PERSIST_K) to 1e-9, and twice for the same bits."""
import numpy as np
import pytest

import oracle
from magnetite_amd import Context, meshgen

pytestmark = pytest.mark.gpu

TOL_U = 1e-8  # north_star: relative L2 on nodal displacements


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("case,edge_blocks", [("structured", 1), ("overflow", 2)])
def test_four_slot_kernels_with_grouped_gathers(built, case, edge_blocks, monkeypatch):
    mesh = meshgen.plate_with_holes(96) if case == "structured" else meshgen.frontal_like(100, 0.4, 3)
    p = meshgen.config_fixed_left_pull_right(mesh)
    ref = oracle.run(p.xy_flat, p.conn_flat, p.u_known, p.u_in, p.f_in, p.youngs_modulus, p.poisson_ratio, p.part_thickness,
                     path="sparse")
    monkeypatch.setenv("MAG_TUNE_PERSIST_MIN_K", "1")
    with Context(device=0, tile_nodes=512) as c:
        one = c.solve(p)
        st_one = c.stats()
        monkeypatch.setenv("MAG_TUNE_PERSIST_K", "4")
        out = c.solve(p)
        st = c.stats()
        again = c.solve(p)
    assert st["cg_kernel"] == 2 and st["edge_blocks"] == edge_blocks and st["tiles_per_workgroup"] == 4, (case, st)
    assert st_one["cg_kernel"] == 2 and st_one["edge_blocks"] == edge_blocks and st_one["tiles_per_workgroup"] == 1, (case, st_one)
    if case == "structured":  # five workgroups, the last one with live and dead slots
        tiles = (p.mesh.num_nodes + 511) // 512
        assert tiles > 16 and tiles % 4 != 0, tiles
    assert out["converged"] == 1 and abs(out["iterations"] - ref["iterations"]) <= max(3, ref["iterations"] // 50), case
    for key in ("u", "f", "stress"):
        assert rel(out[key], ref[key]) <= TOL_U, (case, key)
    assert rel(out["u"], one["u"]) <= 1e-9, case
    assert np.array_equal(out["u"], again["u"])  # bitwise reproducible
