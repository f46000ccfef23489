"""The candidate loop of the fused kernel's 1-NN search (process_points, pcore_fused.hip) on the segment of
tests/csr_rows_cases.py, certified on the CPU by tests/test_csr_rows_cases.py: queries whose four CSR rows have the
lengths {0, 1, 5, 0}, {3, 0, 0, 2} and {7, 7, 7, 7}, with the one candidate within r at every position of the flattened
sequence in turn, and exact ties across a row boundary.  Cost types 2 and 0, whole windows and a 64-sample tile, bit for
bit against the oracle's brute force."""
import pytest

torch = pytest.importorskip("torch")

from tests import csr_rows_cases as cr
from tests.test_gpu_nn_adversarial import _assert_costs, _evaluate, _setup

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _want(cost_type):
    """The oracle's costs, computed once and left unchanged."""
    if cost_type not in _ORACLE:
        _ORACLE[cost_type] = cr.case().oracle_costs(cost_type)
    return _ORACLE[cost_type]


@pytest.mark.parametrize("tile", ["auto", "tcap64"])
def test_costs_match_the_brute_force(tile, monkeypatch):
    if tile == "tcap64":
        monkeypatch.setenv("PCORE_FUSED_TCAP", "64")
    case = cr.case()
    core, t = _setup(case)
    want2, want0 = _want(2), _want(0)
    for call in range(2):
        _assert_costs(_evaluate(core, t, case, 2), want2, f"csr rows 6-DoF, tile {tile}, call {call}")
        _assert_costs(_evaluate(core, t, case, 0), want0, f"csr rows 3-DoF, tile {tile}, call {call}")
    core.close()
