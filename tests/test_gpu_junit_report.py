"""The structured JUnit report rendered on the MI355X (csrc/report_junit_gpu.hip: one <testsuite> per document
through the XML writer, a FAILed tile's records walked twice) against the host writer and the oracle: the same
bytes whichever writer took a document."""
import json
import os

import pytest

import guard_amd
import synth
from guard_oracle import validate_structured as oracle_validate
from rulepack import rule_pack

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
FRAME = ('<?xml version="1.0" encoding="UTF-8"?>\n<testsuites name="cfn-guard validate report" tests="0" failures="0" '
         'errors="0" time="0">\n</testsuites>\n')


def _session(rules, data):
    s = guard_amd.Session()
    for name, text in rules:
        s.add_rules(text, name)
    s.add_docs([d for _, d in data], [n for n, _ in data])
    s.eval(1)
    return s


@pytest.mark.parametrize("pack,corpus", [
    ("cfg2", lambda: synth.cfn_corpus(300, start=177, n_resources=30)),
    ("cfg3", lambda: synth.cfn_corpus(120, start=5100, n_resources=20)),
    ("cfg4", lambda: synth.tf_corpus(8, start=19, n_resources=50)),
    ("cfg5", lambda: synth.config_corpus(100, start=60)),
])
def test_device_junit_equals_host_and_oracle(pack, corpus):
    rules = rule_pack(pack)
    data = [("%s-%d.json" % (pack, i), d) for i, d in enumerate(corpus())]
    s = _session(rules, data)
    s.set_device_report(True)
    dev = s.report("junit")
    s.set_device_report(False)
    host = s.report("junit")
    n, code, st = s.report_junit_device()
    s.close()
    exp, ecode, _ = oracle_validate(rules, data, output="junit")
    assert dev == host == (exp, ecode)
    assert (n, code) == (len(exp.encode()), ecode)
    assert st["device_docs"] > 0


SPECIAL = "a&<b>'q'\"d\"é中"


def _edge_corpus():
    """XML specials and non-ASCII in a document name, a rules file name, a custom message and a compared string
    (a rule name is an identifier: it cannot hold them, the file-name part of a failure's name can); an empty
    `<<>>` message (Some("")), a multi-line one, a top-level clause outside any rule (failure "default"), an IN
    failure, files that PASS and SKIP, an empty document name, a float and a 50-deep value for the host writer.
    (A FAILed file without any message needs a REC_CMP whose `to` is absent; no rule constructs one.)"""
    rules = [("dir.guard/edge & <pack> 'q' \"d\" é.guard",
              "let allowed = ['x', 'y.[z', [1, 2]]\n"
              "rule cmp_str when Resources exists { Resources.*.Properties.V == 'plain' <<custom & <msg> 'q' \"d\" é>> }\n"
              "rule empty_msg when Resources exists { Resources.*.Properties.E exists <<>> }\n"
              "rule multi when Resources exists { Resources.*.Properties.M == 1\n  <<\n    line one\n    line <two>\n  >> }\n"
              "rule in_list when Resources exists { Resources.*.Properties.I IN %allowed }\n"
              "rule deep when Resources exists { Resources.*.Properties.D == 1 }\n"),
             ("top.guard",
              "when Resources exists { Resources.*.Properties.T == 'top' <<top-level>> }\n"
              "rule flt when Resources exists { Resources.*.Properties.F == 2 or Resources.*.Properties.F !exists }\n")]
    good = {"V": "plain", "E": 0, "M": 1, "I": "x", "D": 1, "T": "top", "F": 2}
    data = []
    for i in range(36):
        p = dict(good)
        if i % 9 == 1:
            data.append(("skip %d.json" % i, json.dumps({"Other": i})))   # every file SKIPs
            continue
        if i % 9 != 2:   # (i % 9 == 2: every file PASSes)
            p["V"] = SPECIAL if i % 2 else "other"
            if i % 3 == 0:
                del p["E"]
            if i % 4 == 0:
                p["M"] = [i, {"k&": "<v>"}]
            if i % 5 == 0:
                p["I"] = "q.r" if i % 2 else {"a.b": [3]}
            if i % 6 == 1:
                p["T"] = "not"
            if i == 13:
                p["F"] = 2.5
            if i == 22:
                deep = "leaf"
                for _ in range(50):
                    deep = {"n": [deep]}
                p["D"] = deep
        name = "" if i == 4 else "dir/doc %d & <%s> '\"é.json" % (i, "x" * (i % 3))
        data.append((name, json.dumps({"Resources": {"r%d" % i: {"Properties": p}}}, ensure_ascii=False)))
    return rules, data


def test_xml_edges_and_host_fallback():
    rules, data = _edge_corpus()
    exp, ecode, _ = oracle_validate(rules, data, output="junit")
    assert 'message="default"' in exp and "&apos;q&apos;" in exp and 'status="skip"' in exp and "y[z" in exp
    s = _session(rules, data)
    assert s.report("junit") == (exp, ecode)
    n, code, st = s.report_junit_device()
    assert (n, code) == (len(exp.encode()), ecode)
    assert st["host_docs"] > 0 and st["device_docs"] > 0
    # a middle slice and an empty range are reports of their own
    mid = oracle_validate(rules, data[10:27], output="junit")
    assert s.report_range("junit", 10, 17) == (mid[0], mid[1])
    assert s.report_range("junit", 10, 0)[0] == FRAME
    s.close()
    assert guard_amd.validate_structured_devices(rules, data, devices=[0, 0], output="junit") == (exp, ecode)
    # JunitReporter keeps a rules-file parse error's 5 over a FAIL's 19
    broken = rules + [("broken.guard", "rule r { Resources.*.Properties.X == }")]
    out, code = guard_amd.validate_structured(broken, data[:6], output="junit")
    assert (out, code) == oracle_validate(broken, data[:6], output="junit")[:2]
    assert code == 5 and "<failure" in out


def test_device_junit_golden():
    gdir = os.path.join(G, "validate")
    rules = [(f, open(os.path.join(gdir, "rules-dir", f)).read())
             for f in sorted(os.listdir(os.path.join(gdir, "rules-dir"))) if f.endswith(".guard")]
    dn = "s3-public-read-prohibited-template-non-compliant.yaml"
    s = _session(rules, [(dn, open(os.path.join(gdir, "data-dir", dn)).read())])
    out, code = s.report("junit")
    n, _, st = s.report_junit_device()
    s.close()
    assert code == 19
    assert out == open(os.path.join(gdir, "structured.junit")).read()
    assert n == len(out.encode()) and st["device_docs"] == 1


def test_streamed_junit_equals_one_session():
    rules, data = _edge_corpus()
    one = guard_amd.validate_structured(rules, data, output="junit")
    assert guard_amd.validate_structured_stream(rules, data, chunk_docs=11, output="junit") == one   # 4 chunks
