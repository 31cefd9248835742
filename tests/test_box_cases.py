"""The shared box cases (box_cases.py) on the oracle alone: the precondition of the parity claim (2 h_max < L/2 on every
periodic axis after the h iteration) and the code paths each case is sized to reach.  If a share moves because a kernel
constant changed, the case is re-sized; the assertion stays."""
import pytest

import box_cases as bc
import pyoracle as po


@pytest.fixture(scope="module")
def ora():
    return po.load_oracle()


@pytest.mark.parametrize("name", list(bc.CASES))
def test_regime(ora, name):
    """the preconditions and the intent of every case hold on the oracle alone"""
    st, box = bc.state(name)
    rule, waves = bc.check_regime(st, box, ora)
    print(name, f"rule-path clusters {rule:.3f}, search waves off the prefilter {waves:.3f}")
    if name in ("thin_z", "gresho"):
        assert rule >= 0.9
    elif name in ("windshock", "far_pbc"):
        assert rule == 0.0 and waves == 0.0
    elif name in ("mixed", "far_mixed"):
        assert 0.0 < rule < 1.0 and 0.0 < waves < 1.0
