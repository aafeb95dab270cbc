"""The sampler kernels at the ends of their parameter range, bit for bit against the CPU oracle on the same Philox streams: every row of tests/range_cases.py
-- coinciding and nearly coinciding rungs (swap_fast_ok off: the ladder kernels' 64-bit compare against the plan's table, the colour kernels' two-word
thresholds), each side of the single-precision bound of the biased and alpha rules (bias_f32ok on, off, and on for the hot rungs only; the unique-chain
alpha kernel), and p down to the smallest positive double (thresholds saturated at 1 and at 0, flat swap rows, swap_inv_log2 = 0), scan = wave in both
forms of its cascade.  Everything the entry point returns is compared: the states of every rung, counts, samples, tops0, steps_done, converged; flags and
(n_z, n_x + n_y) of the step entry points; swap_accepts / nerr_sums where asked; N(n), m(n) and the (n_x, n_y, n_z) sets of ptdc_batch.  No tolerances.
A row either equals the oracle or is refused by name when its plan is made -- the same refusal tests/test_sampler_range_cpu.py reads from plan_host().
That file holds the premises (the plan's flags, the tables' saturation) and the conditions under which the oracle's run proves something; the oracle's
result of a row is computed once and shared by the forms."""
import re

import numpy as np
import pytest

import range_cases as R

pytestmark = pytest.mark.gpu

CASES = [pytest.param(r, f, id=r["id"] + (", replay" if f else "")) for r in R.ROWS for f in r["forms"]]
_REF = {}


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _ref(orc, row):
    """the oracle's result of a row: computed by the first form that asks, read (never written) by the second"""
    if row["id"] not in _REF:
        init = R.make_init(row)
        _REF[row["id"]] = (init, R.run_oracle(orc, row, init))
    return _REF[row["id"]]


@pytest.mark.parametrize("row,flags", CASES)
def test_row_equals_the_oracle_or_is_refused_by_name(q, orc, row, flags):
    if "refusal" in row:
        with pytest.raises(q.QecmcError) as e:
            R.run_gpu(q, row, R.make_init(row), flags)
        assert re.search(row["refusal"], str(e.value)), str(e.value)
        return
    init, ref = _ref(orc, row)
    got = R.run_gpu(q, row, init, flags)
    print("%-52s %s" % (row["id"], q._lib.last_kernel() if row["entry"] != "chain" else "chain_update"))
    assert R.differences(row, got, ref) == []
