"""Of R passes in flight, the slots the library keeps resident under a queue budget (nxhip_resident_slots_for): the rule alone, a pure
function of (passes, budget) — no device."""
import pytest

from nexus_amd import capi

PASSES = range(1, 9)
BUDGETS = range(1, 33)


@pytest.mark.parametrize("passes", PASSES)
def test_the_rule(passes):
    values = [capi.resident_slots_for(passes, budget) for budget in BUDGETS]
    for budget, resident in zip(BUDGETS, values):
        assert 1 <= resident <= passes, (passes, budget, resident)
        if 2 * passes + 1 <= budget:  # the parallel shape fits: every slot is served
            assert resident == passes, (passes, budget, resident)
        if passes == 1:
            assert resident == 1, (budget, resident)
    assert all(b >= a for a, b in zip(values, values[1:])), "falls as the budget grows: %s" % (values,)


def test_the_default_budget():
    """four queues: the context's stream takes one, the slots share the chip as if the other three served one slot each"""
    assert [capi.resident_slots_for(passes, 4) for passes in PASSES] == [1, 2, 3, 3, 3, 3, 3, 3]
