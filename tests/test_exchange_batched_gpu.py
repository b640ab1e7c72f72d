"""-m gpu: the on-chip CG kernel's exchange with its loads issued in batches (persist_kernel.h, persist_exchange: the halo
loads in front of the first wait, the record loads behind it, every further pass all of them in front of its first wait;
tests/test_exchange_batched_isa.py looks at the ISA) on meshes of 512-node tiles, MAG_TUNE_PERSIST_MIN_K=1:

  holes-1     plate_with_holes(96), one slot per lane: about 18 workgroups -- most lanes have no record piece (36 of 512 do),
              and the halo entries sit in the first waves only
  holes-4     the same mesh with MAG_TUNE_PERSIST_K=4: four slots, structured, the last workgroup with dead slots
  frontal-4   frontal_like(100, 0.4, 3) with MAG_TUNE_PERSIST_K=4: four slots with overflow
  plate-1     plate(130, 130), one slot: 34 workgroups -- the record pieces span more than one wave (68 lanes), and lanes
              >= 2 * grid share wave 1 with live ones

Each against the oracle's sparse path with the bars of test_walk_gathers_gpu.py (u, f, stress <= 1e-8 relative L2, iterations
within max(3, it // 50)), solved twice for the same bits, on the on-chip kernel without a timeout.

A lane's SECOND halo entry is live in none of these cases: a workgroup of at most 2048 nodes of a plane mesh has a few hundred
halo nodes after compaction, entry 1 starts at the 513th.  No small single-GPU mesh gets there, and the product has no knob for
it; the second entry's loads are issued with the extent as their offset in every case here, which is the path they take on
the benchmark meshes as well."""
import numpy as np
import pytest

import oracle
from magnetite_amd import Context, meshgen

pytestmark = pytest.mark.gpu

TOL = 1e-8  # relative L2 on u, f and stress (test_walk_gathers_gpu.py)

CASES = {
    "holes-1": (lambda: meshgen.plate_with_holes(96), None, 1),
    "holes-4": (lambda: meshgen.plate_with_holes(96), "4", 4),
    "frontal-4": (lambda: meshgen.frontal_like(100, 0.4, 3), "4", 4),
    "plate-1": (lambda: meshgen.plate(130, 130), None, 1),
}


def rel(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


@pytest.mark.parametrize("case", list(CASES))
def test_batched_exchange_matches_the_oracle_bit_for_bit_twice(built, case, monkeypatch):
    make, k, tiles_per_workgroup = CASES[case]
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
    tiles = (p.mesh.num_nodes + 511) // 512
    if case == "holes-1":
        assert 12 <= tiles <= 24, tiles
    if case == "holes-4":
        assert tiles % 4 != 0, tiles  # the last workgroup has dead slots
    if case == "plate-1":
        assert tiles > 32 and (2 * tiles) % 64 != 0, tiles  # record pieces in more than one wave, the last one mixed
    for s in (st, st_again):
        assert s["cg_kernel"] == 2 and s["persist_timeout"] == 0 and s["tiles_per_workgroup"] == tiles_per_workgroup, (case, s)
    print(case, "tiles", tiles, "iterations", out["iterations"], ref["iterations"],
          {key: rel(out[key], ref[key]) for key in ("u", "f", "stress")})
    assert out["converged"] == 1 and abs(out["iterations"] - ref["iterations"]) <= max(3, ref["iterations"] // 50), case
    for key in ("u", "f", "stress"):
        assert rel(out[key], ref[key]) <= TOL, (case, key)
    assert again["iterations"] == out["iterations"]
    for key in ("u", "f", "stress"):
        assert np.array_equal(out[key], again[key]), (case, key)  # the same bits
