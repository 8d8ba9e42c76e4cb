"""The cooperative YAML parse (csrc/yaml_coop.inc: a workgroup's line index and segmentation, a lane per
segment) builds the host loader's arena, marks included: every feature shifted byte by byte across a lane's
16-byte window, a wave's 1 KB and the workgroup's 4 KB tile; the segment shapes; documents a split could
mis-build are refused, never built differently; and large templates load through the session."""
import os

import pytest

import guard_amd
import synth
import test_gpu_yaml as lane
from guard_oracle import validate_structured as oracle_validate
from rulepack import rule_pack

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _coop_on(monkeypatch):
    monkeypatch.setenv("GG_YAML_COOP", "1")


def _indent(n):
    return "a:\n" + " " * n + "b: 1\n" + " " * n + "c: é\nd: 2\n"


# the text after a padding comment line: its first bytes are what crosses the boundary
FEATURES = {
    "indent2": _indent(2), "indent8": _indent(8), "indent17": _indent(17),
    "comment": "a:\n  # note: - x\n  b: 1\n# top\nc: 2\n",
    "dash": "a:\n- x\n- k: 1\n  z: 2\nb:\n  - p\n  - q\n",
    "colon": "abc: 1\nd:\n  efg: 2\n",
    "quoted": "a: \"x # y: z\"\nb:\n  c: 'q: # r'\n",
    "literal": "a: |\n  one\n  two\nb:\n  c: |\n    three\n  d: 1\n",
    "utf8_2": "é: 1\nb:\n  éé: x\n  c: 2\n",
    "utf8_3": "€: 1\nb:\n  €€: x\n  c: 2\n",
    "utf8_4": "\U0001F600: 1\nb:\n  \U0001F600\U0001F600: x\n  c: 2\n",
    "blank": "a: 1\n\nb:\n  c: 1\n\n  d: 2\n",
    "no_eol": "a: 1\nb:\n  c: 2\n  d: 3",
}


def _shifted(tail, boundary, shifts=range(-14, 7)):
    """a batch in which the feature starts at `boundary + shift` bytes past its document's first aligned tile
    (documents are packed back to back, and the tiles are aligned in the packed text)"""
    docs, at = [], 0
    for s in shifts:
        pad = boundary + s - at % 16 - 2
        if pad < 0:
            pad %= 16   # (the 16-byte boundary: a later window's)
        docs.append("#" + "x" * pad + "\n" + tail)
        at += len(docs[-1].encode())
    return docs


def _coop_docs(docs):
    """how many of `docs` the cooperative kernels parsed: the arena cases below must not pass on the lane path"""
    s = guard_amd.Session()
    st = s.add_docs_device(docs)
    coop = s.stat(s.STAT["coop_docs"])
    s.close()
    assert st is not None
    return coop


@pytest.mark.parametrize("boundary", [16, 1024, 4096])
@pytest.mark.parametrize("name", list(FEATURES))
def test_features_across_tile_boundaries(name, boundary, monkeypatch):
    monkeypatch.setenv("GG_JSON_COOP_MIN", "0")
    docs = _shifted(FEATURES[name], boundary)
    assert guard_amd.loader_device_check(docs) == (1, "")
    assert _coop_docs(docs) == len(docs)


def _roots(n):
    return "".join("k%d:\n  a: %d\n  b: x\n" % (i, i) for i in range(n))


SHAPES = {
    "one_entry": lambda: ["a: 1\n", "a:\n  b: 1\n"],
    "empty_values": lambda: ["a: 1\nb:\nc: 2\nd:\n", "r:\n  a:\n  b: 1\n  c:\n"],
    "literal_at_child_indent": lambda: ["Description: |\n  text\n  more: text\nResources:\n  A:\n    T: 1\n  B:\n    T: 2\n"],
    "tagged_literal": lambda: ["K: !Sub |\n  x ${y}\n  z\nL: 1\n"],
    "tagged_sequence": lambda: ["K: !Join\n  - ''\n  - - a\n    - b\nL: 1\n"],
    "indentless": lambda: ["K:\n- a\n- b: 1\n  c: 2\n- d\nL: 1\n"],
    "sequence300": lambda: ["K:\n" + "".join("  - i: %d\n    v: x\n" % i for i in range(300)) + "L: 1\n"],
    "roots65": lambda: [_roots(65)],
    "roots129": lambda: [_roots(129)],
    "root_sequence": lambda: ["- a\n- b: 1\n  c:\n    - x\n- - 1\n  - 2\n"],
    "quoted_headers": lambda: ["\"K\":\n  a: 1\n  b: 2\n'L''s':\n  - x\n  - z\n\"M\\\"\": 1\n"],
    "marker": lambda: ["# head\n---\n# c\na:\n  b: 1\n  c: 2\n"],
    "comments_between": lambda: ["a: 1\n# top\n\nb:\n  # child\n  c: 1\n\n  # another\n  d: 2\n# end\ne: 3\n"],
    "corpus": lambda: synth.cfn_yaml_corpus(3, start=11, n_resources=20),
    "edge": lambda: lane.EDGE,
}
SHAPES.update({"edge%d" % i: (lambda d=d: [d]) for i, d in enumerate(lane.EDGE)})


@pytest.mark.parametrize("name", list(SHAPES))
def test_segment_shapes(name, monkeypatch):
    monkeypatch.setenv("GG_JSON_COOP_MIN", "0")
    docs = SHAPES[name]()
    assert guard_amd.loader_device_check(docs) == (1, "")
    assert _coop_docs(docs) == len(docs)


HAZARDS = ['a: "x\ny"\nb: 1\n', "a: b\nc\nd: 1\n", "a: [1,\n2]\n", "a:\n    b: 1\n  c: 2\n", "a: |\nb: 1\n", "a:\n  b: 1\n\tc: 2\n"]
REFUSED = [(d, "YAML subset") for d in HAZARDS] + list(lane.test_yaml_refusals.pytestmark[0].args[1])


@pytest.mark.parametrize("doc,why", REFUSED)
def test_mis_splits_and_subset_refusals(doc, why, monkeypatch):
    monkeypatch.setenv("GG_JSON_COOP_MIN", "0")
    good = synth.cfn_yaml_corpus(2, n_resources=4)
    verdict, message = guard_amd.loader_device_check([good[0], doc, good[1]])
    assert verdict == -1 and why in message
    assert _coop_docs(good) == 2   # (the session rejects a batch whose refused document the host rejects too)


def _load_and_report(rules, data, params=None):
    s = guard_amd.Session()
    for name, text in rules:
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


def test_templates_load_on_the_device_at_the_default_threshold():
    # (the corpus has no unquoted yes / no / on / off, which the oracle types as strings)
    data = [("t-%d.yaml" % i, synth.cfn_yaml_doc(i, 240)) for i in range(6)]
    assert sum(len(t) for _, t in data) / 6 > 65536
    st, coop = _load_and_report(rule_pack("cfg2"), data)
    assert st is not None   # the lane-per-document loader refused this batch as too few, too large
    assert st["refused_docs"] == 0 and coop == 6
    assert st["report"] == oracle_validate(rule_pack("cfg2"), data)[:2]


@pytest.mark.parametrize("params", [None, [("p.yaml", "ExtraParameter: 1\n")]])
def test_mixed_batch(params):
    docs = [synth.cfn_yaml_doc(i, 240) for i in range(2)] + synth.tf_corpus(1, start=11, n_resources=600)
    docs += synth.cfn_corpus(70, 0, 2) + [synth.cfn_yaml_doc(i, 2) for i in range(3)]
    docs.append(docs[1].replace("\nResources:", "\nDescription: &d x\nResources:", 1))   # an anchor: host-loaded
    assert "&d" in docs[-1]
    data = [("d%03d" % i, t) for i, t in enumerate(docs)]
    # the Terraform rule pack, not cfg2: cfg2's type blocks raise on a Terraform plan, in the oracle too,
    # and this pack evaluates plans and templates alike (as test_gpu_json_coop's mixed batch uses it)
    pack = os.path.join(os.path.dirname(__file__), "golden", "tf_rulepack")
    rules = [(f, open(os.path.join(pack, f)).read()) for f in sorted(os.listdir(pack)) if f.endswith(".guard")]
    st, coop = _load_and_report(rules, data, params)
    assert st is not None and st["refused_docs"] == 1 and coop == 3
    assert st["report"] == oracle_validate(rules, data, params=params)[:2]
