"""The recorded programs of hipnet.engine.Plan, op by op and slot by slot, against tests/plan_fingerprints.json.

The fixture holds, per configuration and per program, the SHA-256 of the canonical text of tests/plan_fingerprint.py
(every op's kind, lane, integer slots, float bits and pointers by NAME, tables and host structs decoded), the op count
and a histogram of kinds, and the side data (bucket marks, late cuts, counters) in clear. It was written by
`python tests/plan_fingerprint.py` on the commit before the backward recorder was split into a driver and one method
per tape-entry kind; a change to the recorder that is meant to leave the programs alone leaves every digest alone.

Plans are recorded at (2, 64, 64) and never run. Two processes: one without HRNET_MEASURE (the product switches), one
with HRNET_MEASURE=1 from the start, which flips one measurement switch per plan. On a mismatch the full canonical
texts go to pytest's tmp_path: record the same file on the reference commit and diff the two.
"""
import json
import os

import pytest

from spawned import spawned

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'plan_fingerprints.json')
REQUIRED = {
    'product': ['w32_bf16_train', 'w32_fp32_train', 'w48_bf16_train', 'softmax_bf16_train', 'w32_bf16_eval',
                'deterministic', 'deterministic_wgrad_atomic', 'dp_plan'],
    'measure': ['fused_bwd_0', 'fused_pw_0', 'fused_maxc_32', 'fuse_sum_0', 'batch_sumbwd_0', 'batch_sumfwd_0'],
}


def _check(which, tmp_path):
    import plan_fingerprint as F
    with open(FIXTURE) as f:
        fixture = json.load(f)
    want = fixture['configs'][which]
    names = [name for name, _ in want]
    assert set(REQUIRED[which]) <= set(names)
    # every configuration is in the fixture, or is listed with the error the reference commit raised for it
    assert set(names) | set(fixture['not_recorded']) >= {c[0] for c in F.CONFIGS[which]}
    got = F.record(which, only=set(names))
    assert [name for name, _ in got] == names
    bad = []
    for (name, fp), (_, ref) in zip(got, want):
        assert 'error' not in fp, (name, fp)
        if F.summary(fp) != ref:
            for prog in ('fwd', 'bwd'):
                path = os.path.join(str(tmp_path), '{}.{}.txt'.format(name, prog))
                with open(path, 'w') as f:
                    f.write(fp[prog]['text'])
            diff = [k for k in ('fwd', 'bwd', 'side') if F.summary(fp)[k] != ref[k]]
            print(name, 'differs in', diff, {k: (F.summary(fp)[k], ref[k]) for k in diff})
            bad.append((name, diff))
    assert not bad, 'recorded programs changed: {} (canonical texts in {})'.format(bad, tmp_path)


@spawned
def test_product_configurations_record_the_reference_programs(tmp_path):
    _check('product', tmp_path)


@spawned
def test_measurement_switches_record_the_reference_programs(tmp_path):
    _check('measure', tmp_path)
