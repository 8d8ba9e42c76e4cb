"""The structured YAML report rendered on the MI355X (csrc/report_yaml_gpu.hip: report_gpu.hip's record walk
through the block-YAML writer, scalars styled by csrc/yaml_scalar.h) against the host libyaml writer and the
oracle: the same bytes whichever writer took a document."""
import json
import os

import pytest

import guard_amd
import synth
from guard_oracle import validate_structured as oracle_validate
from rulepack import rule_pack
from test_yaml_scalar_cpu import STRINGS

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


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
def test_device_yaml_equals_host_and_oracle(pack, corpus):
    rules = rule_pack(pack)
    data = [("%s-%d.json" % (pack, i), d) for i, d in enumerate(corpus())]
    s = _session(rules, data)
    s.set_device_report(True)
    dev = s.report("yaml")
    s.set_device_report(False)
    host = s.report("yaml")
    n, code, st = s.report_yaml_device()
    s.close()
    exp, ecode, _ = oracle_validate(rules, data, output="yaml")
    assert dev == host == (exp, ecode)
    assert (n, code) == (len(exp.encode()), ecode)
    assert st["device_docs"] > 0


def _style_corpus():
    """documents whose keys and values carry every scalar style, floats, a 129-byte key, a "|+" value and
    nesting past the device writer's depth; rules whose custom messages are multi-line with leading and
    trailing spaces, and whose failures print keys and values in messages and as values"""
    rules = [("style.guard",
              "rule v { Resources.*.Properties.V == 'no such value'\n  <<\n    Violation: V differs\n  >> }\n"
              "rule w { Resources.*.Properties.W exists << trailing space >> }\n"
              "rule m { Resources.*.Properties.M.Missing exists <<true>> }\n"
              "rule d { Resources.*.Properties.D == 1 }\n")]
    strings = STRINGS + [1.5, 7, -3, None, True, ["x", ["y", []], {}], {"a": {"b": [{"c": "p\nq"}]}}]
    data = []
    for i, v in enumerate(strings):
        k = v if isinstance(v, str) and v else "key%d" % i
        deep = "leaf"
        for _ in range(50 if i % 23 == 5 else i % 4):
            deep = {"n": [deep]}
        props = {"V": v, "M": {k: v, "other": [v]}, "D": deep}
        # (escaped: raw U+0085 / U+2028 would be breaks to the YAML loader; it takes no surrogate-pair escapes)
        text = json.dumps({"Resources": {"r%d" % i: {"Properties": props}}}).replace("\\ud83d\\ude00", "\U0001F600")
        data.append(("dir/style %d.json" % i if i % 2 else "", text))
    return rules, data


def test_styles_and_host_fallback():
    rules, data = _style_corpus()
    exp, ecode, _ = oracle_validate(rules, data, output="yaml")
    s = _session(rules, data)
    assert s.report("yaml") == (exp, ecode)
    n, code, st = s.report_yaml_device()
    assert (n, code) == (len(exp.encode()), ecode)
    assert st["host_docs"] > 0 and st["device_docs"] > 0
    # a middle slice and an empty range are reports of their own
    mid = oracle_validate(rules, data[20:45], output="yaml")
    assert s.report_range("yaml", 20, 25) == (mid[0], mid[1])
    assert s.report_range("yaml", 20, 0)[0] == "[]\n"
    s.close()
    assert guard_amd.validate_structured_devices(rules, data, devices=[0, 0], output="yaml") == (exp, ecode)


def test_device_yaml_golden():
    gdir = os.path.join(G, "validate")
    rules = [(f, open(os.path.join(gdir, "rules-dir", f)).read())
             for f in sorted(os.listdir(os.path.join(gdir, "rules-dir"))) if f.endswith(".guard")]
    dn = "s3-public-read-prohibited-template-non-compliant.yaml"
    s = _session(rules, [(dn, open(os.path.join(gdir, "data-dir", dn)).read())])
    out, code = s.report("yaml")
    n, _, st = s.report_yaml_device()
    s.close()
    assert code == 19
    assert out == open(os.path.join(gdir, "structured.yaml")).read()
    assert n == len(out.encode()) and st["device_docs"] == 1
