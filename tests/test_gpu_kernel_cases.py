"""Every built ladder / wave / colour / statistics / shortest-chain kernel, run bit for bit against the CPU oracle: one case per kernel from the registry
(tests/kernel_cases.py, tests/kernel_cases.json).  Each case runs its call, asserts that the library launched the kernel the case is keyed by
(qecmc._lib.last_kernel(): the case ran that kernel and not a neighbour), that the oracle's run of the same inputs is not vacuous (conditions on the
reference alone, kernel_cases.vacuous), and that every compared field equals the oracle's on the same Philox streams -- counts, samples, tops0,
steps_done, converged; the final state of every rung of a fixed-length run; swap_accepts / nerr_sums of the statistics kernels; shortest / shortest_n /
unique_n / overflow of the shortest-chain kernels; N(n) / m(n) of the unique-chain estimators' kernels.  No tolerances.

tests/test_kernel_cases_cpu.py holds the registry complete against the build, so the labels seen here are the built kernels."""
import numpy as np
import pytest

import kernel_cases as KC

pytestmark = pytest.mark.gpu

CASES = KC.load_cases()
SEEN = set()


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.mark.parametrize("case", CASES, ids=[c["label"] for c in CASES])
def test_kernel_bit_exact_against_the_oracle(q, case):
    init = KC.make_init(case)
    ref = KC.run_oracle(case, init)
    assert not KC.vacuous(case, init, ref)
    got = KC.run_gpu(q, case, np.array(init))
    ran = q._lib.last_kernel()
    assert ran == case["label"]
    SEEN.add(ran)
    assert KC.differences(case, got, ref) == []


def test_the_cases_ran_every_built_kernel():
    built = set(KC.built_labels())
    assert SEEN <= built
    if len(SEEN) == len(CASES):          # (a session that ran the whole registry; a selection of cases, `-k`, has seen its own only)
        assert SEEN == built
