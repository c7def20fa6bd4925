"""GPU: the engine's automatic sharded plan over the grid of tests/test_plan_grid.py equals
tests/golden/plan_grid.json, recorded from the engine of the commit before the planner moved into
csrc/plan.h: every kind and plan letter, and the modelled ms / link ms that gossip_plan_model reports.
No kernel of a round runs: plan, commit, plan, reset per point.

The modelled times must agree to a relative 1e-9: a double carries 2.2e-16 and the longest expression
of the model has about 20 operations, so the same formula in another order stays below 1e-14, while the
smallest meaningful change to a fitted constant is above 1e-3.  With link_gbps 0 the model divides by a
zero bandwidth: inf must equal inf and NaN must equal NaN."""
import math

import pytest

from test_plan_grid import SHAPES, recorded, shape_engines, walk  # noqa: F401  (recorded: the fixture)

pytestmark = pytest.mark.gpu


def same_ms(got, want):
    if math.isnan(want) or math.isinf(want):
        return math.isnan(got) if math.isnan(want) else got == want
    return abs(got - want) <= 1e-9 * abs(want)


@pytest.mark.parametrize("N,G", SHAPES, ids=[f"{N}-{G}" for N, G in SHAPES])
def test_engine_plans_recorded_kinds_and_costs(recorded, N, G):  # noqa: F811
    from gossip_hip import Engine
    for name, e in shape_engines(Engine, N, G):
        want = recorded["engine"][name]
        assert want["kinds"] == recorded["oracle"][name], name  # (the grid stays where both planners can run every kind)
        kinds, letters, ms = walk(e, N)
        assert kinds == want["kinds"], name
        assert letters == want["letters"], name
        rows = [recorded["model_rows"][i] for i in want["model_ms"]]
        assert len(ms) == len(rows)
        for i, (g, w) in enumerate(zip(ms, rows)):
            assert all(same_ms(a, b) for a, b in zip(g, w)), (name, i, g, w)
