"""Device loads appended to a session that already holds documents (csrc/append_gpu.hip): the session
equals a one-shot session of the concatenated input, and its reports equal the oracle's."""
import json

import pytest

import guard_amd
import synth
from guard_oracle import validate_structured as oracle_validate

pytestmark = pytest.mark.gpu
RULES = [("iam.guard", synth.IAM_RULES), ("ebs.guard", synth.EBS_RULES)]
FORMATS = ("json", "yaml", "sarif")
ANCHORED = "Resources:\n  b:\n    Type: AWS::S3::Bucket\n    Metadata: &a x\n"   # refused by the device, built on the host
HUGE_FLOAT = '{"Resources": {"v": {"Type": "AWS::S3::Bucket", "Properties": {"Weight": 1e400}}}}'   # likewise
CFN = synth.cfn_corpus(68, 0, 8)
# 16 documents of 5000 strings each, all distinct: more than a 2^16-slot table holds
MANY = [json.dumps({"Resources": {"b": {"Type": "AWS::S3::Bucket"}}, "L": ["s%d-%d" % (d, k) for k in range(5000)]}) for d in range(16)]
# name -> (batches, environment, refused documents per load, first batch through the host loader)
SPLITS = {
    "1+1": ([CFN[:1], CFN[1:2]], {}, 0),
    "3+65": ([CFN[:3], CFN[3:]], {}, 0),
    "20+20+20": ([CFN[:20], CFN[20:40], CFN[40:60]], {}, 0),
    "40+10+10": ([CFN[:40], CFN[40:50], CFN[50:60]], {}, 0),   # the third load fits the blocks the second grew
    "host_columns": ([CFN[:20], CFN[20:40]], {"GG_RESIDENT_ARENA": "0"}, 0),
    "host_loader_first": ([CFN[:20], CFN[20:40]], {}, 0, True),
    "json+yaml": ([CFN[:30], synth.cfn_yaml_corpus(30, 30, 8)], {}, 0),
    "refused": ([CFN[:9] + [ANCHORED] + CFN[9:20], CFN[20:25] + [HUGE_FLOAT] + CFN[25:40]], {}, 1),
    "coop": ([CFN[:20], CFN[20:40]], {"GG_JSON_COOP_MIN": "64"}, 0),
    "table": ([CFN[:20], MANY], {"GG_JSON_TABLE_LOG": "16"}, 0),
}


def _session(batches, params=None, mode=0, host_first=False):
    """a session with RULES that device-loads each batch in turn (host_first: the first one through
    add_docs); returns it, the loads' statistics and the (name, text) list the oracle takes"""
    s = guard_amd.Session()
    s.configure(mode, 0)
    for name, text in RULES:
        s.add_rules(text, name)
    if params:
        s.set_params(params)
    first, stats = 0, []
    for b in batches:
        names = ["d%04d" % (first + i) for i in range(len(b))]
        stats.append(s.add_docs(b, names) if host_first and not first else s.add_docs_device(b, names))
        first += len(b)
    return s, stats, [("d%04d" % i, t) for i, t in enumerate(t for b in batches for t in b)]


@pytest.mark.parametrize("name", list(SPLITS))
def test_split_loads_equal_the_one_shot_session(name, monkeypatch):
    batches, env, refused, host_first = (SPLITS[name] + (False,))[:4]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s, stats, data = _session(batches, host_first=host_first)
    one, ostats, _ = _session([[t for b in batches for t in b]])
    assert all(st is not None and st["refused_docs"] == refused for st in stats[host_first:])
    for what in ("ndocs", "nodes", "bytes"):
        assert s.stat(s.STAT[what]) == one.stat(one.STAT[what])
    for what in ("distinct_strings", "pool_bytes") if not host_first else ():   # a shared string is held once
        assert sum(st[what] for st in stats) == ostats[0][what]
    if name == "table":
        assert stats[1]["table_retries"] >= 1
    if name == "coop":
        assert s.stat(s.STAT["coop_docs"]) == 40
    s.eval(1)
    got = {f: s.report(f) for f in FORMATS}
    s.close()
    one.close()
    assert got == {f: oracle_validate(RULES, data, output=f)[:2] for f in FORMATS}


@pytest.mark.parametrize("mode,device_report", [(0, "1"), (1, "1"), (0, "0")])   # "0": a host writer runs before the append
def test_append_after_an_evaluation(mode, device_report, monkeypatch):
    monkeypatch.setenv("GG_DEVICE_REPORT", device_report)
    s, _, data = _session([CFN[:30]], mode=mode)
    s.eval(1)
    assert s.report() == oracle_validate(RULES, data)[:2]
    for lo, hi in ((30, 67), (67, 68)):   # the second upload grows the packed buffers, the third fits them
        data += [("d%04d" % i, CFN[i]) for i in range(lo, hi)]
        s.add_docs_device(CFN[lo:hi], [n for n, _ in data[lo:hi]])
        s.eval(1)
        assert s.report() == oracle_validate(RULES, data)[:2]
    s.close()


PARAMS = [("p.yaml", "Parameters:\n  Port: 5432\n  Team: a\n")]


def test_parameters_merge_into_both_loads():
    batches = [CFN[:20] + [ANCHORED], CFN[20:60]]
    s, _, data = _session(batches, params=PARAMS)
    s.eval(1)
    got = s.report()
    s.close()
    assert got == oracle_validate(RULES, data, params=PARAMS)[:2]


def test_failed_append_leaves_the_session_as_it_was():
    late = CFN[20:30] + ['{"Parameters": 1, "z": 2}'] + CFN[30:40]   # a root key the parameters hold
    s, _, data = _session([CFN[:20]], params=PARAMS)
    _, ecode, err = oracle_validate(RULES, data + [("d%04d" % (20 + i), t) for i, t in enumerate(late)], params=PARAMS)
    assert ecode == -1
    s.eval(1)
    before = s.report()
    with pytest.raises(guard_amd.GuardError) as ei:
        s.add_docs_device(late, ["d%04d" % i for i in range(20, 41)])
    assert ei.value.code == -1 and err == "Error occurred " + ei.value.message
    assert s.stat(s.STAT["ndocs"]) == 20 and s.report() == before
    s.close()
