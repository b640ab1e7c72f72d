"""GPU: load cases and design variants on ONE context, in turns.  Both sets run through the same host driver, so what can go
wrong is cross-talk: a set's results, counters or the lent problem leaking into the other set or into the context's own solve."""
import os

import numpy as np
import pytest

from load_cases_util import make_cases
from magnetite_amd import Context, meshgen
from variants_util import make_variants

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RESULTS = ("u", "f", "stress")


def tensile():
    g = np.load(os.path.join(GOLD, "tensile.npz"))
    return meshgen.Problem(meshgen.Mesh(g["xy"], g["conn"].astype(np.int32), "tensile"), g["u_known"].astype(np.uint8), g["u_in"],
                           g["f_in"], *[float(v) for v in g["material"]])


def assert_rounds_equal(first, second, what):
    assert len(first) == len(second) == 3
    for i, (a, b) in enumerate(zip(first, second)):
        for key, x, y in zip(RESULTS, a, b):
            assert np.array_equal(x, y), (what, i, key)


# cg_variant=1: no on-chip kernel, so every member runs alone with the uploaded problem lent to it
@pytest.mark.parametrize("opts,side_by_side", [(dict(), True), (dict(cg_variant=1), False)])
def test_cases_and_variants_in_turns_on_one_context(built, opts, side_by_side):
    prob = tensile()
    assert prob.mesh.num_nodes < 600
    cu, cf = make_cases(prob, 3, seed=5)
    xy, mat, vu, vf = make_variants(prob, 3, seed=9)
    assert not np.array_equal(cu, vu) or not np.array_equal(cf, vf)  # (the sets differ in their loads as well)
    with Context(device=0, **opts) as c:
        c.upload_problem(prob)
        c.set_load_cases(cu, cf)
        c.set_variants(xy, mat, vu, vf)
        rounds = []
        for _ in range(2):
            c.run_cases()
            cases = [c.download_case(i) for i in range(3)]
            cases_info = c.cases_info()
            c.run_variants()
            variants = [c.download_variant(i) for i in range(3)]
            rounds.append((cases, cases_info, variants, c.variants_info()))
        (cases1, cinfo1, variants1, vinfo1), (cases2, cinfo2, variants2, vinfo2) = rounds
        print(opts, cinfo1, vinfo1)
        assert_rounds_equal(cases1, cases2, "load cases")
        assert_rounds_equal(variants1, variants2, "variants")
        # counters start over with every run and are each set's own
        assert cinfo2 == cinfo1 and vinfo2 == vinfo1
        assert cinfo1["cases"] == 3 and vinfo1["variants"] == 3 and cinfo1["redone"] == 0 and vinfo1["redone"] == 0
        for info, per_launch in ((cinfo1, "cases_per_launch"), (vinfo1, "variants_per_launch")):
            assert (info[per_launch] >= 3 and info["launches"] == 1) if side_by_side else (info[per_launch] == 0 and info["launches"] == 0), info
        # the sets are not each other's: variant 2 has other loads, another shape and another material than load case 2
        assert not np.array_equal(cases1[2][0], variants1[2][0])
        # the uploaded problem came back from every loan: a run of what the context holds, then a plain solve
        c.run()
        held = dict(zip(RESULTS, c.download()), **c.stats())
        after = c.solve(prob)
    with Context(device=0, **opts) as fresh:
        ref = fresh.solve(prob)
    for out in (held, after):
        for key in RESULTS:
            assert np.array_equal(out[key], ref[key]), key
        assert out["iterations"] == ref["iterations"] and out["cg_kernel"] == ref["cg_kernel"]
