"""`validate -i` on the device loader (csrc/merge_gpu.hip): a session with input parameters loads its
documents on the MI355X and merges the parameters there; reports, merge errors and the batch entries
equal the oracle's (and a host-loaded session's)."""
import functools
import json
import os

import pytest

import guard_amd
import synth
from guard_oracle import validate_structured as oracle_validate

pytestmark = pytest.mark.gpu
P = os.path.join(os.path.dirname(__file__), "golden", "params")
FORMATS = ("json", "yaml", "sarif", "junit")
ANCHORED = "Resources:\n  b:\n    Type: AWS::S3::Bucket\n    Metadata: &a x\n"   # refused: built and merged on the host


def _pfile(rel):
    return (os.path.basename(rel), open(os.path.join(P, rel)).read())


def _map_docs(n=130):
    """db_resource.yaml and synthetic templates as JSON and block YAML (4 waves a workgroup: 33 workgroups),
    a {} root and a root of 70 keys (the conflict check's second round of 64 lanes)"""
    db = _pfile("db_resource.yaml")[1]
    docs = [(db, synth.cfn_corpus(1, i, 2)[0], synth.cfn_yaml_doc(i, 2))[i % 3] for i in range(n)]
    docs[5] = "{}"
    docs[77 % n] = json.dumps({"k%d" % j: j for j in range(70)})
    return docs


def _list_docs(n=130):
    docs = [("[%d, 2]" % i, "- %d\n- 9\n- 1\n" % i)[i % 2] for i in range(n)]
    docs[5] = "[]"
    docs[77] = json.dumps(list(range(70)))
    return docs


WIDE = "\n".join("P%d: %d" % (j, j) for j in range(4000)) + "\n"   # 4001 nodes: past the LDS staging limit
# (parameter files, rules, documents, the refused document)
SETS = {
    "db": ([_pfile("input-parameters-dir/db_params.yaml"), _pfile("input-parameters-dir/db_metadata.yaml")],
           [_pfile("params_keys.guard")], _map_docs, ANCHORED),
    "keyblock": ([_pfile("dup_params.yaml")], [_pfile("params_keys.guard")], _map_docs, ANCHORED),
    "list": ([("p.yaml", "- 7\n- 3\n")], [("l.guard", "this[*] > 5\nthis[3] == 1\n")], _list_docs, "- &a 1\n- 2\n"),
    # rules that print single values: a failure that shows the merged root would print 4000 entries a document
    "wide": ([("wide.yaml", WIDE)], [("w.guard", "rule last { P3999 == 0 }\nrule has { this[ keys == 'P2000' ] exists }\n"
                                                 "rule deep { Resources.*.Properties.Tags[*].Key == 'bar' }\n")],
             _map_docs, ANCHORED),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    params, rules, make, refused = SETS[name]
    docs = make(40 if name == "wide" else 130)   # the oracle merges 4000 keys a document in seconds: 10 workgroups
    docs[60 % len(docs)] = refused
    data = [("d%03d" % i, t) for i, t in enumerate(docs)]
    return params, rules, data, {f: oracle_validate(rules, data, output=f, params=params)[:2] for f in FORMATS}


def _session(rules, params, data):
    s = guard_amd.Session()
    for name, text in rules:
        s.add_rules(text, name)
    s.set_params(params)
    return s, [t for _, t in data], [n for n, _ in data]


@pytest.mark.parametrize("resident", ["1", "0"])
@pytest.mark.parametrize("name", list(SETS))
def test_merged_batch_equals_the_oracle(name, resident, monkeypatch):
    monkeypatch.setenv("GG_RESIDENT_ARENA", resident)
    params, rules, data, exp = _case(name)
    s, texts, names = _session(rules, params, data)
    st = s.add_docs_device(texts, names)
    assert st is not None and st["refused_docs"] == 1
    s.eval(1)
    got = {f: s.report(f) for f in FORMATS}
    s.close()
    assert got == exp
    h, texts, names = _session(rules, params, data)
    h.add_docs(texts, names)
    h.eval(1)
    assert h.report() == got["json"]
    h.close()


CONFLICTS = {
    # two device-loaded documents hold a root key the parameters hold: the earlier one's error
    "device": (SETS["db"][0], {37: '{"Parameters": 1, "z": 2}', 90: "Metadata: 1\n"}),
    # the host-built refused document comes first
    "host_first": (SETS["db"][0], {20: "Metadata: &a 1\n", 37: '{"Parameters": 1}', 90: '{"Parameters": 2}'}),
    "device_first": (SETS["db"][0], {37: '{"a": 0, "Metadata": {}}', 90: "Parameters: &a 1\n"}),
    "incompatible": ([("p.yaml", "- 1\n")], {}),
}


@pytest.mark.parametrize("name", list(CONFLICTS))
def test_merge_errors_are_the_first_failing_documents(name):
    params, bad = CONFLICTS[name]
    rules = [_pfile("db_param_port_rule.guard")]
    docs = _map_docs()
    for i, t in bad.items():
        docs[i] = t
    data = [("d%03d" % i, t) for i, t in enumerate(docs)]
    _, ecode, err = oracle_validate(rules, data, params=params)
    assert ecode == -1
    s, texts, names = _session(rules, params, data)
    with pytest.raises(guard_amd.GuardError) as ei:
        s.add_docs_device(texts, names)
    s.close()
    assert ei.value.code == -1 and err == "Error occurred " + ei.value.message
    with pytest.raises(guard_amd.GuardError) as ei:
        guard_amd.validate_structured(rules, data, params=params)
    assert ei.value.code == -1 and err == "Error occurred " + ei.value.message


@pytest.mark.parametrize("fmt", FORMATS)
def test_batch_entries_with_parameters(fmt):
    params, rules, data, _ = _case("db")
    data = data[:60] + data[61:]   # every document on the device: the arena stays resident
    exp = oracle_validate(rules, data, output=fmt, params=params)[:2]
    assert guard_amd.validate_structured(rules, data, output=fmt, params=params) == exp
    assert guard_amd.validate_structured_devices(rules, data, devices=[0, 0], output=fmt, params=params) == exp
