"""The cooperative JSON parse (csrc/json_coop.inc, a workgroup per large document) builds the host loader's
arena: every feature shifted byte by byte across a lane's 16-byte window, a wave's 1 KB and the workgroup's
4 KB tile; the shapes at its limits; and Terraform plans through the session, against the oracle's report."""
import functools
import json
import os

import pytest

import guard_amd
import synth
from guard_oracle import validate_structured as oracle_validate

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
HEAD = '{"p":"'
PRETTY = '{\n  "p": "'
# the text after the padded string `"p":"xxx",` -- its first bytes are what crosses the boundary
FEATURES = {
    "string": '"s":"abcdefghijklmnopqrstuvwx","t":1}',
    "bs1_quote": '"a":"\\"","k":[1]}',
    "bs2_quote": '"a":"\\\\","k":[1]}',
    "bs3_quote": '"a":"\\\\\\"","k":[1]}',
    "bs4_quote": '"a":"\\\\\\\\","k":[1]}',
    "bs1_letter": '"a":"\\n","k":[1]}',
    "bs2_letter": '"a":"\\\\n","k":[1]}',
    "bs3_letter": '"a":"\\\\\\n","k":[1]}',
    "bs4_letter": '"a":"\\\\\\\\n","k":[1]}',
    "u_escape": '"a":"\\u00e9","k":{"b":"\\u00e9"}}',
    "utf8_2": '"a":"é","k":{"é":1}}',
    "utf8_3": '"a":"€","k":{"€":1}}',
    "utf8_4": '"a":"\U0001F600","k":{"\U0001F600":1}}',
    "newline": (PRETTY, '\n  "k": {"a": 1},\n  "é": [\n    2\n  ]\n}'),
    "empty_map": '"a":{},"b":{ }}',
    "empty_list": '"a":[],"b":[\n]}',
    "close_open": '"a":[{"b":1},{"c":2}]}',
    "number": '"a":-12.5e+3,"b":1234567890123}',
    "true": '"a":true,"b":false}',
    "null": '"a":null,"b":null}',
    "colon": '"abc":1,"d":2}',   # shift -5 puts the colon on the boundary
    "comma": '"a":1,"b":2}',     # shift -5: the comma
}


def _shifted(feature, boundary, shifts=range(-14, 7)):
    """a batch in which the feature starts at `boundary + shift` bytes past its document's first aligned tile
    (documents are packed back to back, and the tiles are aligned in the packed text)"""
    head, tail = feature if isinstance(feature, tuple) else (HEAD, feature)
    docs, at = [], 0
    for s in shifts:
        pad = boundary + s - at % 16 - len(head.encode()) - 2
        pad %= 16 if pad < 0 else pad + 1   # (the 16-byte boundary: a later window's)
        docs.append(head + "x" * pad + '",' + tail)
        at += len(docs[-1].encode())
    return docs


@pytest.mark.parametrize("boundary", [16, 1024, 4096])
@pytest.mark.parametrize("name", list(FEATURES))
def test_features_across_tile_boundaries(name, boundary, monkeypatch):
    monkeypatch.setenv("GG_JSON_COOP_MIN", "0")
    assert guard_amd.loader_device_check(_shifted(FEATURES[name], boundary)) == (1, "")


@functools.lru_cache(maxsize=None)
def _plans(n, start, n_resources):
    return synth.tf_corpus(n, start=start, n_resources=n_resources)


ACCEPTED = {
    "depth64": lambda: ["[" * 64 + "]" * 64, '{"a":' * 63 + "{}" + "}" * 63],
    "list65535": lambda: [json.dumps(list(range(65535)), separators=(",", ":"))],
    "empty": lambda: ["[]", "{}"],
    "whitespace": lambda: ['\n \n {"a": [1, "b"]} \n\n', "  [\n]\n"],
    "plans": lambda: list(_plans(3, 0, 150)),
    "plans_indent": lambda: [json.dumps(json.loads(t), indent=2) for t in _plans(3, 0, 150)],
}


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_shapes_accepted(name, monkeypatch):
    monkeypatch.setenv("GG_JSON_COOP_MIN", "0")
    assert guard_amd.loader_device_check(ACCEPTED[name]()) == (1, "")


REFUSED = {
    "depth65": ("[" * 65 + "]" * 65, "nesting deeper than 64"),
    "trailing_comma": ('{"a":1,}', "strict-JSON subset"),
    "missing_colon": ('{"a" 1}', "strict-JSON subset"),
    "unterminated": ('{"a":"b}', "strict-JSON subset"),
    "after_root": ('{"a":1} x', "strict-JSON subset"),
    "leading_zero": ("[01]", "strict-JSON subset"),
    "control_byte": ('{"a":"b\x01c"}', "strict-JSON subset"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_shapes_refused(name, monkeypatch):
    monkeypatch.setenv("GG_JSON_COOP_MIN", "0")
    text, word = REFUSED[name]
    verdict, message = guard_amd.loader_device_check(['{"ok":[1,2]}', text])
    assert verdict == -1 and word in message


def _pack(d):
    p = os.path.join(G, d)
    return [(f, open(os.path.join(p, f)).read()) for f in sorted(os.listdir(p)) if f.endswith(".guard")]


def _load_and_report(data, params=None):
    s = guard_amd.Session()
    for name, text in _pack("tf_rulepack"):
        s.add_rules(text, name)
    if params:
        s.set_params(params)
    st = s.add_docs_device([t for _, t in data], [n for n, _ in data])
    coop = s.stat(s.STAT["coop_docs"])
    if st is not None:
        s.eval(1)
        st["report"] = s.report()
    s.close()
    return st, coop


def test_plans_load_on_the_device_at_the_default_threshold():
    data = [("plan-%d.json" % i, t) for i, t in enumerate(_plans(6, 11, 600))]
    assert sum(len(t) for _, t in data) / 6 > 65536
    st, coop = _load_and_report(data)
    assert st is not None   # the lane-per-document loader refused this batch as too few, too large
    assert st["refused_docs"] == 0 and coop == 6
    assert st["report"] == oracle_validate(_pack("tf_rulepack"), data)[:2]


@pytest.mark.parametrize("params", [None, [("p.yaml", "ExtraParameter: 1\n")]])
def test_mixed_batch(params):
    plans = _plans(6, 11, 600)
    docs = list(plans[:2]) + synth.cfn_corpus(70, 0, 2) + [synth.cfn_yaml_doc(i, 2) for i in range(3)]
    docs.append('{"format_version":"0",' + plans[2][1:])   # a duplicate key: refused, built on the host
    data = [("d%03d" % i, t) for i, t in enumerate(docs)]
    st, coop = _load_and_report(data, params)
    assert st is not None and st["refused_docs"] == 1 and coop == 2
    assert st["report"] == oracle_validate(_pack("tf_rulepack"), data, params=params)[:2]
