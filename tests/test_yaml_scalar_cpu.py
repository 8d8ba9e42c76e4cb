"""The device YAML writer's scalar machine (csrc/yaml_scalar.h: style selection and emission as a streaming
scan / emit pair) run on the host through gg_yaml_scalar, against libyaml itself (PyYAML's CDumper, fed the
events serde_yaml produces): every string as a mapping value and as a mapping key, at indents 0 and 4."""
import io

import pytest
import yaml

import guard_amd
from guard_oracle import formats

STRINGS = [
    "a\tb", "a: b", "a:b", "- x", "-x", "a #b", "a#b", "x ", " x", "", "it's",
    "a\nb", "a\nb\n", " a\nb", "a\nb ", "a\n b", "a \nb", "a\rb", "a\n\nb", "\nq",
    "é\u0085  z", "\x07\x1b\x7f﻿", "\U0001F600", "café 中",
    "?x", "? x", "[a", "a,b", "a]", "%a", "@a", "`a", "---", "--- a", "...", "-", "?", ":", "a:", "a: ",
    "!a", "&a", "*a", "|a", ">a", "\"a", "'a", "a\"b", "{a", "a}", "a\\b", "#a",
    "true", "True", "1", "-1", "+1", "1.5", "1.", ".5", "1e5", "~", "null", "NULL", "0x1F", "0o17", "0b2", ".inf", "-.INF",
    ".nan", "1e400", "+", "++1", "0x", "1_0", "12345678901234567890123", "Check was not compliant: /Resources/a[L:1,C:2] #x",
    "abcdefghijklmnopqrstuvwxyz0123456789/path: tail", "k" * 128, "k" * 129,
    "a\nb\n\n", "\n",
]
# the only strings the device writer may hand to the host writer (-1): "|+" scalars, complex keys, 1e400
KEEP = {"a\nb\n\n", "\n"}


def _libyaml(text, key, indent):
    def sc(v):
        return yaml.ScalarEvent(None, None, (True, True), v, style=formats._str_style(v))
    ms, me = yaml.MappingStartEvent(None, None, True, flow_style=False), yaml.MappingEndEvent()
    depth = indent // 2
    ev = [yaml.StreamStartEvent(), yaml.DocumentStartEvent(explicit=False)]
    for _ in range(depth):
        ev += [ms, sc("p")]
    ev += [ms] + ([sc(text), sc("v")] if key else [sc("k"), sc(text)]) + [me] * (depth + 1)
    ev += [yaml.DocumentEndEvent(explicit=False), yaml.StreamEndEvent()]
    buf = io.StringIO()
    yaml.emit(ev, buf, Dumper=yaml.CDumper, width=-1, allow_unicode=True)
    body = "\n".join(buf.getvalue().split("\n")[depth:])[indent:]
    return body[:-len(": v\n")] if key else body[len("k:"):-1]


@pytest.mark.parametrize("indent", [0, 4])
@pytest.mark.parametrize("key", [False, True])
@pytest.mark.parametrize("text", STRINGS, ids=[repr(s)[:24] for s in STRINGS])
def test_scalar_equals_libyaml(text, key, indent):
    got = guard_amd.yaml_scalar(text, indent, key)
    multiline = any(c in text for c in "\n\r\u0085\u2028\u2029")   # libyaml's breaks: not a simple key
    may_host = text in KEEP or text == "1e400" or (key and (multiline or len(text.encode()) > 128))
    if got is None:
        assert may_host, "handed to the host writer"
        return
    assert got.decode("utf-8") == _libyaml(text, key, indent)
