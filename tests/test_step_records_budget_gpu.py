"""GPU: the record budget of the time-stepping passes (mag_run_transient, mag_run_explicit with either kinematics), the one path
through their shared host set-up that no other suite takes.  A run of 2^31 - 1 steps with a snapshot a step asks for 2^31 x 400
bytes of snapshots alone (25 nodes: a state vector is 400 bytes), about 859 GB, more than the card has whatever is free: the
pass refuses with MAG_ERR_TOO_LARGE before it allocates anything for the run, leaves no results behind, and the next run gives
the bits of the run before the refusal."""
import numpy as np
import pytest

from magnetite_amd import Context, meshgen
from magnetite_amd._lib import MAG_ERR_STATE, MAG_ERR_TOO_LARGE
from magnetite_amd.solver import MagnetiteError

pytestmark = pytest.mark.gpu

RHO = 2700.0
RECORDS = dict(probes=(0, 7, 49), energies=True, snapshot_every=2)
PASSES = {
    "transient": ("mag_run_transient", lambda c, **kw: c.run_transient(dt=1e-6, density=RHO, **kw)),
    "explicit": ("mag_run_explicit", lambda c, **kw: c.run_explicit(density=RHO, **kw)),
    "explicit_tl": ("mag_run_explicit", lambda c, **kw: c.run_explicit(density=RHO, kinematics="tl", **kw)),
}


@pytest.mark.parametrize("name", list(PASSES))
def test_records_beyond_the_card_are_refused_and_leave_nothing(built, name):
    fn, run = PASSES[name]
    prob = meshgen.config_fixed_left_point_load(meshgen.plate(4))
    assert prob.mesh.num_nodes == 25
    with Context(device=0) as c:
        c.upload_problem(prob)
        run(c, steps=4, **RECORDS)
        good = c.download_transient()

        with pytest.raises(MagnetiteError) as e:
            run(c, steps=2**31 - 1, snapshot_every=1)
        text = str(e.value)
        print(name, text)
        assert e.value.code == MAG_ERR_TOO_LARGE, text
        assert fn in text and "the records of 2147483647 steps need" in text and "are free" in text, text

        with pytest.raises(MagnetiteError) as e:
            c.download_transient()
        assert e.value.code == MAG_ERR_STATE, str(e.value)
        with pytest.raises(MagnetiteError) as e:
            run(c, steps=4, resume=True, **RECORDS)
        assert e.value.code == MAG_ERR_STATE and "resume" in str(e.value), str(e.value)

        run(c, steps=4, **RECORDS)
        again = c.download_transient()
    assert sorted(again) == sorted(good)
    for k, v in good.items():
        assert np.asarray(again[k]).tobytes() == np.asarray(v).tobytes(), k
