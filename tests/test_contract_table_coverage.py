"""CPU test: the contract table of tests/test_gpu_api_contract.py (host form equals _dev form, every argument error, every empty batch) covers the
C ABI.  Every c12381_*_dev name that include/c12381_hip.h declares, and every host entry without a _dev twin, is a row of the table or is
listed here with the reason why it is not."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NOT_IN_TABLE = {
    "fp_mulchain_dev": "benchmark kernel of the Fp leaf: no host form, no bytes anyone relies on",
    "g1_msm_multi": "takes an array of contexts; tests/test_gpu_distributed.py",
    "create": "life cycle", "destroy": "life cycle", "last_error": "life cycle", "trim": "life cycle", "version": "life cycle",
    "set_stream": "stream call", "sync": "stream call", "wait_event": "stream call", "record_event": "stream call",
    "profile": "event timing, no batch", "profile_read": "event timing, no batch",
}


def test_every_entry_is_in_the_contract_table_or_listed():
    from test_gpu_api_contract import _entries
    text = open(os.path.join(ROOT, "include", "c12381_hip.h")).read()
    declared = set(re.findall(r"\bc12381_([a-z0-9_]+)\s*\(", text))
    assert len(declared) > 100
    rows = _entries(3)
    hosts, devs = {h for h, _, _, _ in rows}, {d for _, d, _, _ in rows if d}
    assert hosts | devs <= declared, sorted((hosts | devs) - declared)
    for name in sorted(declared):
        if name.endswith("_dev"):
            assert name in devs or name in NOT_IN_TABLE, name
        elif name + "_dev" in declared:
            assert name in hosts or name + "_dev" in NOT_IN_TABLE, name
        else:
            assert name in hosts or name in NOT_IN_TABLE, name
    for name in NOT_IN_TABLE:
        assert name in declared and name not in hosts | devs, name
