"""The kernels whose hot arguments now lead their argument lists (so that they arrive in SGPRs with the wavefront instead of
through a load of the argument struct) compute what they computed before: only where a value comes from changed, so every
weight, both Adam moments, every cost and every score must have the same BITS as at the parent commit.

tests/golden/arg_preload_parent.json was recorded on an MI355X at that commit by scripts/record_arg_preload_golden.py, whose
cases() this test runs again: the DIN step at T = 50 and T = 3 (wide weight-gradient launch, NCH0 = 9, partial last batch, a
4-step and a 1-step graph, then a second call on the carried start), the YouTube kind at D = 64 (NCH0 = 15, the <8,5>
weight-gradient launch), predict of 33 / 8192 + 33 / 16384 + 33 rows (ctr_fwd16, the forward-only chain, ctr_fwd4) and the
float64 MLP [281, 100, 1] with a short last batch.  Compared for equality: CRC32s of the exact bytes, the costs as a list.

(B = 256 as the smallest batch that surely keeps the wide weight-gradient launch: tn_schedule_wide's `ok` does not depend on the
batch at all, so any batch would, and 256 gives the chain launch eight tiles and the last batch a single partial one.)"""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(_HERE), "scripts"))
import record_arg_preload_golden as rec  # noqa: E402

with open(os.path.join(_HERE, "golden", "arg_preload_parent.json")) as _f:
    GOLDEN = json.load(_f)

CASES = sorted(rec.cases())


def test_golden_holds_every_case():
    assert sorted(GOLDEN) == CASES


@pytest.mark.parametrize("name", CASES)
def test_same_bits_as_the_parent_commit(name):
    from goctr_amd import capi
    capi.init(0)
    got = rec.cases()[name]()
    want = GOLDEN[name]
    print(f"{name}: got {got}")
    assert got == want
