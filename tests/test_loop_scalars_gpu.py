"""-m gpu: the four-slot structured on-chip CG kernel with its loop's bookkeeping at compile time and in one scalar word
(persist_kernel.h, persist_loop_scalars, DESIGN LS: a slot's tile and position are s and tid, and what a wave needs to know of
its slots' flags -- a live tile, a lane whose q is zeroed, a lane that publishes -- are bits the loop branches on;
tests/test_loop_scalars_isa.py looks at the ISA), MAG_TUNE_PERSIST_MIN_K=1, tile_nodes=512:

  holes-4     plate_with_holes(96), MAG_TUNE_PERSIST_K=4: 18 tiles in 5 workgroups, dead slots in the last -- the scalar branch
              over a slot without a tile, and the x update that runs on its zeros
  plate130-4  plate(130, 130), K=4: 34 tiles in 9 workgroups, the last one with dead slots
  holes-1     holes-4's mesh with one slot per lane: the predicate is off, the kernel is the one it was

config_fixed_left_pull_right fixes the left edge and pulls on the right one: a few wave-slots hold prescribed nodes and most hold
none, the tiles' rims publish their q and their interiors do not, the last tile ends inside a wave -- both arms of every scalar
branch run.  Each case against the oracle's sparse path at the bars of test_exchange_reduction_gpu.py (u, f, stress <= 1e-8
relative L2, iterations within max(3, it // 50)), solved twice for the same bits, on the on-chip kernel without a timeout."""
import numpy as np
import pytest

import oracle
from magnetite_amd import Context, meshgen

pytestmark = pytest.mark.gpu

TOL = 1e-8  # relative L2 on u, f and stress (test_exchange_reduction_gpu.py)

# case -> (mesh, MAG_TUNE_PERSIST_K, tiles per workgroup, tiles, workgroups)
CASES = {
    "holes-4": (lambda: meshgen.plate_with_holes(96), "4", 4, 18, 5),
    "plate130-4": (lambda: meshgen.plate(130, 130), "4", 4, 34, 9),
    "holes-1": (lambda: meshgen.plate_with_holes(96), None, 1, 18, 18),
}


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("case", list(CASES))
def test_loop_scalars_match_the_oracle_bit_for_bit_twice(built, case, monkeypatch):
    make, k, tiles_per_workgroup, tiles_expected, workgroups_expected = CASES[case]
    p = meshgen.config_fixed_left_pull_right(make())
    ref = oracle.run(p.xy_flat, p.conn_flat, p.u_known, p.u_in, p.f_in, p.youngs_modulus, p.poisson_ratio, p.part_thickness,
                     path="sparse")
    monkeypatch.setenv("MAG_TUNE_PERSIST_MIN_K", "1")
    if k:
        monkeypatch.setenv("MAG_TUNE_PERSIST_K", k)
    with Context(device=0, tile_nodes=512) as c:
        out = c.solve(p)
        st = c.stats()
        again = c.solve(p)
        st_again = c.stats()
    # the shapes the cases are about: a change of meshgen must not move a case off them silently
    tiles = (p.mesh.num_nodes + 511) // 512
    workgroups = -(-tiles // tiles_per_workgroup)
    assert (tiles, workgroups) == (tiles_expected, workgroups_expected), (case, tiles, workgroups)
    assert st["num_tiles"] == tiles, (case, st["num_tiles"])
    if k:
        assert tiles % 4 != 0, tiles  # the last workgroup has dead slots
    assert 0 < np.count_nonzero(p.u_known) < p.u_known.size  # prescribed DOFs, and not everywhere
    for s in (st, st_again):
        assert s["cg_kernel"] == 2 and s["persist_timeout"] == 0 and s["tiles_per_workgroup"] == tiles_per_workgroup, (case, s)
    print(case, "tiles", tiles, "workgroups", workgroups, "iterations", out["iterations"], ref["iterations"],
          {key: rel(out[key], ref[key]) for key in ("u", "f", "stress")})
    assert out["converged"] == 1 and abs(out["iterations"] - ref["iterations"]) <= max(3, ref["iterations"] // 50), case
    for key in ("u", "f", "stress"):
        assert rel(out[key], ref[key]) <= TOL, (case, key)
    assert again["iterations"] == out["iterations"]
    for key in ("u", "f", "stress"):
        assert np.array_equal(out[key], again[key]), (case, key)  # the same bits
