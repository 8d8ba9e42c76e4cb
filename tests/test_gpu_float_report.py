"""Floats in the device report writers (csrc/shortest_f64.h through report_gpu.hip's write_value / value_only):
documents whose failing clauses report floats -- compared, inside a reported struct and list, under an
unresolved traversed_to, as rule literals -- are written on the MI355X in all four structured formats, with the
bytes of the host writer and the oracle.  (A non-finite float still sends its document to the host writer, which
raises its IncompatibleError: test_gpu_errors.py, float-inf.)"""
import json

import pytest
import yaml

import guard_amd
from guard_oracle import validate_structured as oracle_validate
from test_float_format_cpu import EDGES

pytestmark = pytest.mark.gpu
FORMATS = ("json", "yaml", "sarif", "junit")

RULES = [("floats.guard",
          "rule cmp when Resources exists { Resources.*.Properties.F == 10 }\n"
          "rule whole when Resources.*.Properties.M exists { Resources.*.Properties.M == 1 }\n"
          "rule trav when Resources.*.Properties.M exists { Resources.*.Properties.M.Missing exists }\n"
          "rule lit when Resources exists { Resources.*.Properties.S == 2.5 <<S is not 2.5>> }\n"
          "rule inl when Resources exists { Resources.*.Properties.T IN [1.5, 0.25] }\n")]


def _docs():
    """64 one-resource documents.  i % 8 == 6 PASSes; i % 8 == 7 FAILs without reporting a float; the rest take
    the edge floats in turn: F compared, M reported whole and as the value traversed to, S and T against the
    float literals (which every such failure reports too)."""
    docs = []
    for i in range(64):
        x, y = EDGES[i % len(EDGES)], EDGES[(3 * i + 1) % len(EDGES)]
        if i % 8 == 6:
            p = {"F": 10, "S": 2.5, "T": 1.5}
        elif i % 8 == 7:
            p = {"F": "ten", "M": {"a": "s", "l": [1, {"b": None}]}, "S": 2.5, "T": 0.25}
        else:
            p = {"F": x, "M": {"a": x, "l": [y, -x, {"b": y}, "s"]}, "S": y if i % 2 else 2.5, "T": x if i % 3 else 1.5}
        docs.append(("doc%d" % i, {"Resources": {"r%d" % i: {"Properties": p}}}))
    return docs


FLOAT_DOCS = sum(1 for i in range(64) if i % 8 < 6)   # the documents the parent's writers left to the host


def _data(kind):
    if kind == "yaml-text":
        return [(n + ".yaml", yaml.safe_dump(d, default_flow_style=False)) for n, d in _docs()]
    return [(n + ".json", json.dumps(d)) for n, d in _docs()]


@pytest.fixture(scope="module")
def sessions():
    made = {}

    def get(kind):
        if kind not in made:
            data = _data(kind)
            s = guard_amd.Session()
            s.add_rules(RULES[0][1], RULES[0][0])
            if kind == "device-loaded":   # the arena stays in HBM: the writers need no copy-down
                st = s.add_docs_device([d for _, d in data], [n for n, _ in data])
                assert st is not None and st["refused_docs"] == 0
            else:
                s.add_docs([d for _, d in data], [n for n, _ in data])
            s.eval(1)
            made[kind] = (s, data)
        return made[kind]

    yield get
    for s, _ in made.values():
        s.close()


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", ["host-loaded", "device-loaded", "yaml-text"])
def test_float_documents_are_written_on_the_device(sessions, kind, fmt):
    s, data = sessions(kind)
    exp, ecode, _ = oracle_validate(RULES, data, output=fmt)
    s.set_device_report(True)
    dev = s.report(fmt)
    s.set_device_report(False)
    host = s.report(fmt)
    s.set_device_report(None)
    assert dev == host == (exp, ecode)
    n, code, st = getattr(s, "report_%s_device" % fmt)()
    assert (n, code) == (len(exp.encode()), ecode)
    assert (st["host_docs"], st["device_docs"]) == (0, len(data))


def test_report_range_slice(sessions):
    s, data = sessions("host-loaded")
    exp, ecode, _ = oracle_validate(RULES, data[10:40], output="yaml")
    assert s.report_range("yaml", 10, 30) == (exp, ecode)

