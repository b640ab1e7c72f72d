"""GPU: the passes on the assembled pattern do not disturb one another through the scratch they share (the block-row table, the
device checks' words and probe list, the state and words of the single evaluations).

Leg A, on one context: mag_run_transient (6 steps, probes, energies, snapshots), mag_run_newton (one increment, probes at other
indices), mag_assemble_tangent, mag_assemble_effective_tangent and mag_internal_force at a non-zero state, mag_run_explicit
(linear) resumed for 5 steps, mag_run_transient_tl resumed for 4 steps.  Leg B: the stepping runs alone.  Every array of
download_transient() and download_transient_tl() after the last run and the info words have the same bytes in both legs, and in
leg A download_newton() right after the Newton run is download_newton() at the end.  On plate16 and holes3k, at cg 0 and 4."""
import numpy as np
import pytest

import transient_tl_cases as cases
from magnetite_amd import Context
from test_transient_tl_gpu import RHO, SET, same_bits

pytestmark = pytest.mark.gpu


def one_leg(p, s, cg, between):
    """the stepping runs of a leg on one context; `between` runs behind the linear implicit pass"""
    n2 = 2 * p.mesh.num_nodes
    rec = dict(density=RHO, probes=[0, 7, n2 - 1], energies=True, snapshot_every=2)
    with Context(device=0) as c:
        c.upload_problem(p)
        lin = c.transient(steps=6, dt=s["dt"], rayleigh=(s["alpha"], 0.0), u0=s["u0"], cg=cg, cg_tol=cases.CG_TOL, **rec)
        kept = between(c, lin["u"])
        ex = c.explicit(steps=5, resume=True, **rec)
        tl = c.transient(steps=4, dt=s["dt"], rayleigh=(s["alpha"], 0.0), resume=True, kinematics="tl", cg=cg, **SET, **rec)
        last = dict(c.download_transient(), **{"tl_" + k: v for k, v in c.download_transient_tl().items()})
        last["info"] = np.array(list(c.transient_info().values()) + list(c.transient_tl_info().values()))
        newton_at_the_end = c.download_newton() if kept is not None else None
    assert lin["converged"] == 1 and tl["converged"] == 1 and tl["resumed"] == 1 and ex["resumed"] == 1
    assert lin["u"].any() and np.isfinite(last["u"]).all()
    return last, kept, newton_at_the_end


@pytest.mark.parametrize("cg", [0, 4])
@pytest.mark.parametrize("name", ["plate16", "holes3k"])
def test_the_passes_leave_one_anothers_results_alone(built, name, cg):
    s = cases.setup(name, "pull5d")
    p = s["prob"]
    n2 = 2 * p.mesh.num_nodes

    def newton_and_the_evaluations(c, u):
        out = c.newton(increments=1, probes=[3, n2 - 2, 5, 11], cg=cg, **SET)
        assert out["probe_u"].shape == (2, 4)
        newton = c.download_newton()
        kt = c.assemble_tangent(u)
        at = c.assemble_effective_tangent(u, 0.25 * s["dt"] ** 2, 1.0, RHO)
        f, W, inverted = c.internal_force(u)
        assert np.isfinite(kt).all() and np.isfinite(at).all() and np.isfinite(f).all() and W > 0.0 and not inverted
        return newton

    a, newton, newton_at_the_end = one_leg(p, s, cg, newton_and_the_evaluations)
    b, _, _ = one_leg(p, s, cg, lambda c, u: None)
    print(name, "cg", cg, "arrays", sorted(a), "info", a["info"].tolist())
    same_bits(a, b, "with and without the Newton run and the evaluations between the stepping runs")
    same_bits(newton, newton_at_the_end, "mag_download_newton right after its run and at the end")
