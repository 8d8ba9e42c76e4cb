"""The device loader's intern table and string pool kept in HBM between loads (csrc/append_gpu.hip
intern_carry / intern_compact): a session built by device loads and appends reports what a one-shot
session of the same documents loaded by the host loader reports, and what the oracle reports."""
import json

import pytest

import guard_amd
import synth
from guard_oracle import validate_structured as oracle_validate

pytestmark = pytest.mark.gpu
RULES = [("iam.guard", synth.IAM_RULES), ("ebs.guard", synth.EBS_RULES)]
PARAMS = [("p.yaml", "Parameters:\n  Port: 5432\n  Team: a\n")]
ANCHORED = "Resources:\n  b:\n    Type: AWS::S3::Bucket\n    Metadata: &a x\n"   # refused by the device, built on the host
CFN = synth.cfn_corpus(80, 0, 8)


def _fresh(k, tag="q"):
    """CFN[0] with k strings no other document holds, in a list under a key the pool holds already"""
    d = json.loads(CFN[0])
    d["Type"] = ["fresh-%s-%d" % (tag, i) for i in range(k)]
    return json.dumps(d)


def _lists(ndocs, k):
    """ndocs small documents of k strings each, all distinct"""
    return [json.dumps({"Resources": {"b": {"Type": "AWS::S3::Bucket"}}, "L": ["s%d-%d" % (d, i) for i in range(k)]}) for d in range(ndocs)]


# name -> (steps, environment); a step is (loader, documents, the load's seeded_strings is zero, its
# index_strings or None): the first step's figures are not checked (nothing to seed, every string is new)
D, H = "device", "host"
CASES = {
    "no_new_string": ([(D, CFN[:20], None, None), (D, CFN[:20], True, 0)], {}),
    **{"adds_%d" % k: ([(D, CFN[:20], None, None), (D, [_fresh(k)], True, k)], {}) for k in (1, 63, 64, 65)},
    # more than 32768 occurrences: sized for them the working table is larger than the resident 2^16 slots
    # (with the starting size capped at 2^16 as well, it grows by the retry instead)
    "grow_at_start": ([(D, CFN[:4], None, None), (D, _lists(8, 5000), True, 40001)], {}),
    "grow_at_start_log16": ([(D, CFN[:4], None, None), (D, _lists(8, 5000), True, 40001)], {"GG_JSON_TABLE_LOG": "16"}),
    # more than 65536 distinct strings: BAD_TABLE doubles the table after a polluted run
    "retry_mid_load": ([(D, CFN[:4], None, None), (D, _lists(16, 5000), True, 80001)], {"GG_JSON_TABLE_LOG": "16"}),
    "three_appends": ([(D, CFN[:20], None, None), (D, CFN[20:40], True, None), (D, CFN[40:60], True, None),
                       (D, CFN[60:80] + [_fresh(3)], True, None)], {}),
    "host_add_docs": ([(D, CFN[:20], None, None), (H, CFN[20:30]), (D, CFN[30:40], False, None), (D, CFN[40:50], True, None)], {}),
    "host_built_document": ([(D, CFN[:20] + [ANCHORED], None, None), (D, CFN[20:40], False, None), (D, CFN[40:60], True, None)], {}),
    "collisions": ([(D, CFN[:10], None, None), (D, CFN[10:20] + [_fresh(5)], None, None)], {"GG_JSON_FP_MASK": "0xF"}),
}


def _session(params=None):
    s = guard_amd.Session()
    s.configure(0, 0)
    for name, text in RULES:
        s.add_rules(text, name)
    if params:
        s.set_params(params)
    return s


def _host_report(data, params=None):
    """the JSON report of a one-shot session of `data` loaded by the host loader, checked against the oracle's"""
    one = _session(params)
    one.add_docs([t for _, t in data], [n for n, _ in data])
    one.eval(1)
    want = one.report()
    one.close()
    assert want == oracle_validate(RULES, data, params=params)[:2]
    return want


@pytest.mark.parametrize("name", list(CASES))
def test_appends_report_as_the_host_loaded_session(name, monkeypatch):
    steps, env = CASES[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, data = _session(), []
    for loader, docs, *expect in steps:
        names = ["d%04d" % (len(data) + i) for i in range(len(docs))]
        data += list(zip(names, docs))
        if loader == H:
            s.add_docs(docs, names)
            continue
        st = s.add_docs_device(docs, names)
        assert st is not None
        carried, added = expect
        if carried is not None:
            assert (s.stat(s.STAT["seeded_strings"]) == 0) == carried
        if added is not None:
            assert s.stat(s.STAT["index_strings"]) == added == st["distinct_strings"]
        if name == "retry_mid_load" and len(data) > 4:
            assert st["table_retries"] > 0
        if name == "three_appends":   # the state an append left serves the next one
            s.eval(1)
            assert s.report() == _host_report(data)
    s.eval(1)
    got = s.report()
    s.close()
    assert got == _host_report(data)


def test_failed_append_leaves_the_resident_table_as_it_was():
    late = CFN[30:35] + ['{"Parameters": 1, "z": 2}'] + CFN[35:40]   # a root key the parameters hold: the merge fails
    s = _session(PARAMS)
    data = [("d%04d" % i, t) for i, t in enumerate(CFN[:30])]
    s.add_docs_device(CFN[:20], [n for n, _ in data[:20]])    # the parameters' strings join the pool on the host
    s.add_docs_device(CFN[20:30], [n for n, _ in data[20:]])  # seeded with them: the device holds every string now
    s.eval(1)
    before = s.report()
    with pytest.raises(guard_amd.GuardError):
        s.add_docs_device(late, ["d%04d" % i for i in range(30, 41)])
    assert s.stat(s.STAT["ndocs"]) == 30 and s.report() == before
    more = [("d%04d" % (30 + i), t) for i, t in enumerate(CFN[40:50] + [_fresh(7)])]
    s.add_docs_device([t for _, t in more], [n for n, _ in more])
    assert s.stat(s.STAT["seeded_strings"]) == 0 and s.stat(s.STAT["index_strings"]) >= 7
    s.eval(1)
    got = s.report()
    s.close()
    assert got == _host_report(data + more, PARAMS)
