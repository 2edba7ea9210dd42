"""The d > 16 proposal-regime rule decides which kernel a step runs, with thresholds fitted on the hardware.  CPU only: every scripted
run of oracle/make_regime_traces.py -- every band edge, debugging switch, mode count and script -- gives the
records in tests/golden/regime_traces.json, taken on the commit before the rule became a function of its own (tempest_amd/regime.py)."""
import json

from oracle import make_regime_traces as M


def test_regime_traces_match_the_record():
    with open(M.GOLDEN) as f:
        golden = json.load(f)
    assert golden["recorded_at"] == M.RECORDED_AT and tuple(golden["n"]) == M.NS
    now = M.record()
    # the runs written out first: a difference there names the reading
    assert set(now["full"]) == set(golden["full"]) and len(golden["full"]) >= 12
    for rid, runs in golden["full"].items():
        assert now["full"][rid] == runs, rid
    assert len(golden["groups"]) == len(M.N_DIMS) * len(M.ENVS)
    assert now["groups"] == golden["groups"]
