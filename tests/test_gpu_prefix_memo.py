"""Prefix memo of the lane evaluator (eval_core.inc "Prefix memo"; compiler.cpp mark_prefix_slots): clauses that walk
the same run of key steps after the same `%var` head reuse the node the first walk reached.  Results must not
change: for every case the structured JSON report and the per-tile statuses equal the oracle's, byte for byte, with
one tile per lane (where the memo runs) and with one tile per wave (where it does not)."""
import json
import os

import pytest

import guard_amd
from guard_oracle import validate_structured as oracle_validate

pytestmark = pytest.mark.gpu

CAP = 16   # eval_core.inc PM_CAP: values of a variable the memo holds

PABC = ["BlockPublicAcls", "BlockPublicPolicy", "IgnorePublicAcls", "RestrictPublicBuckets"]

SHARED = """let buckets = Resources.*[ Type == 'AWS::S3::Bucket' ]
rule public_read when %buckets !empty {
  %buckets.Properties.PublicAccessBlockConfiguration exists
  %buckets.Properties.PublicAccessBlockConfiguration.BlockPublicAcls == true
  %buckets.Properties.PublicAccessBlockConfiguration.BlockPublicPolicy == true
  %buckets.Properties.PublicAccessBlockConfiguration.IgnorePublicAcls == true
  %buckets.Properties.PublicAccessBlockConfiguration.RestrictPublicBuckets == true
}
"""

TWO_VARS = """let a = Resources.*[ Type == 'T::A' ]
let b = Resources.*[ Type == 'T::B' ]
rule ra when %a !empty {
  %a.Properties.Cfg.X == true
  %a.Properties.Cfg.Y == true
}
rule rb when %b !empty {
  %b.Properties.Cfg.X == true
  %b.Properties.Cfg.Y == true
  %b.Properties.Cfg.Z exists
}
rule rc when %a !empty {
  %a.Properties.Cfg.Z exists
  %a.Properties.Other.W exists
  %a.Properties.Other.V == 1
}
"""

NOT_EVALUATED = """let a = Resources.*[ Type == 'T::A' ]
rule first_in_or when %a !empty {
  %a.Type exists or %a.Properties.Cfg.X == true
  %a.Properties.Cfg.X == true
}
rule first_in_when when %a !empty {
  when %a.Nope exists {
    %a.Properties.Other.W exists
  }
  %a.Properties.Other.W exists
  %a.Properties.Other.V == 1
}
"""
# first_in_or: `%a.Type exists` passes for every value, so the second clause of the disjunction -- the first
# user of the run Properties.Cfg.X -- never walks; the next clause is the run's first walk.  first_in_when: no
# value has `Nope`, so the block is skipped; its clause is the first user of the run Properties.Other.W, which
# neither the condition nor anything before it walks; the clause after the block is the run's first walk.

# Block values: clauses of a type block and of a nested block that share `Properties.Cfg`.  A memo for these
# (a start-node-tagged entry at the driver's query site) was built, passed this case, measured slower and was
# removed: the case stays as a guard that block-value walks are left alone -- a type
# block with three clauses over several resources, one value after another, and a nested block on a child value.
BLOCKS = """rule typed {
  T::A {
    Properties.Cfg exists
    Properties.Cfg.X == true
    Properties.Cfg.Y == true
  }
}
rule typed_b {
  T::B {
    Properties.Cfg.X == true
    Properties.Cfg.Y == true
    Properties.Cfg {
      X exists
      Y == true
      Inner.K exists
      Inner.K == 1
    }
  }
}
"""

KEY_CASE = """let a = Resources.*[ Type == 'T::A' ]
rule exact when %a !empty {
  %a.Properties.Cfg.X == true
  %a.Properties.Cfg.Y == true
}
rule converted when %a !empty {
  %a.properties.cfg.X == true
  %a.properties.cfg.Y == true
  %a.Properties.cfg.X == true
  %a.Properties.cfg.Y == true
}
"""


def _bucket(k):
    """bucket k of a document: complete, partly false, or broken at each step of the shared prefix"""
    full = {"Type": "AWS::S3::Bucket", "Properties": {"BucketName": "b%d" % k, "PublicAccessBlockConfiguration": {p: True for p in PABC}}}
    m = k % 7
    if m == 1:
        full["Properties"]["PublicAccessBlockConfiguration"]["IgnorePublicAcls"] = False
    elif m == 2:
        del full["Properties"]["PublicAccessBlockConfiguration"]["BlockPublicPolicy"]
    return full


def _broken(k):
    m = k % 6
    if m == 0:
        return {"Type": "AWS::S3::Bucket"}
    if m == 1:
        return {"Type": "AWS::S3::Bucket", "Properties": "none"}
    if m == 2:
        return {"Type": "AWS::S3::Bucket", "Properties": [{"PublicAccessBlockConfiguration": {}}]}
    if m == 3:
        return {"Type": "AWS::S3::Bucket", "Properties": {"BucketName": "x"}}
    if m == 4:
        return {"Type": "AWS::S3::Bucket", "Properties": {"PublicAccessBlockConfiguration": "off"}}
    return _bucket(k)


def _doc(resources):
    return json.dumps({"Resources": {"r%02d" % i: r for i, r in enumerate(resources)}})


def _other(k):
    return {"Type": "AWS::EC2::Volume", "Properties": {"Size": 10 + k, "Encrypted": k % 2 == 0}}


def _t(kind, k):
    """resource of the T::A / T::B cases: resolved, converted-case and broken prefixes by k"""
    cfg = {"X": k % 2 == 0, "Y": k % 3 != 0, "Inner": {"K": k % 2}}
    if k % 5 == 1:
        cfg["Z"] = "z"
    props = {"Cfg": cfg, "Other": {"W": 1, "V": k % 2}}
    m = k % 8
    if m == 3:
        props = {"Other": {"W": 1}}
    elif m == 4:
        props = {"cfg": cfg}            # reached through a converter only
    elif m == 5:
        return {"Type": kind, "properties": {"Cfg": cfg}}
    elif m == 6:
        return {"Type": kind, "Properties": ["Cfg"]}
    elif m == 7:
        del cfg["Y"]
    return {"Type": kind, "Properties": props}


def _shared_docs():
    return [_doc([_bucket(3 * d + k) if k % 3 else _other(k) for k in range(2 + d % 9)]) for d in range(24)]


def _break_docs():
    return [_doc([_broken(d + k) if k % 4 else _bucket(d + k) for k in range(1 + d % 11)]) for d in range(24)]


def _capacity_docs():
    docs = []
    for n in (CAP + 3, CAP, 1, 0, CAP + 3, CAP - 1, CAP + 1):
        docs.append(_doc([_other(0)] + [_broken(k) if k % 5 == 4 else _bucket(k) for k in range(n)]))
    return docs


def _t_docs(n=24):
    return [_doc([_t("T::A" if (k + d) % 3 else "T::B", d + k) for k in range(1 + d % 10)] + [_other(d)]) for d in range(n)]


def _batch_docs():
    # 200 documents in one launch.  In lane mode the test launches it as 400 one-document batches on 256 waves
    # (BATCH_ENV), so a lane evaluates a second and a third tile -- of another document, or of the other rules
    # file -- and an entry or a valid bit left from the tile before would show.
    return [_doc([_broken(d + k) if (d + k) % 3 == 0 else _bucket(d + k) for k in range(d % 5)] + [_t("T::A", d), _other(d)])
            for d in range(200)]


# the launch shape knobs of the library (capi.cpp session_upload): one document per batch, one wave per CU
BATCH_ENV = {"GG_LANE_DOCS": "1", "GG_LANE_WAVES_PER_CU": "1"}


CASES = {
    "shared": ([("shared.guard", SHARED)], _shared_docs),
    "breaks": ([("shared.guard", SHARED)], _break_docs),
    "capacity": ([("shared.guard", SHARED)], _capacity_docs),
    "two_vars": ([("two_vars.guard", TWO_VARS)], _t_docs),
    "not_evaluated": ([("not_evaluated.guard", NOT_EVALUATED)], _t_docs),
    "blocks": ([("blocks.guard", BLOCKS)], _t_docs),
    "key_case": ([("key_case.guard", KEY_CASE)], _t_docs),
    "batches": ([("shared.guard", SHARED), ("key_case.guard", KEY_CASE)], _batch_docs),
}

_expected = {}


def _oracle(case):
    """the oracle's report, exit code and per-tile statuses of a case, computed once"""
    if case not in _expected:
        from guard_oracle import evaluator as E
        from guard_oracle.loader import load_document
        from guard_oracle.parser import parse_rules
        rules, mk = CASES[case]
        docs = mk()
        names = ["m-%d.json" % i for i in range(len(docs))]
        exp, ecode, _ = oracle_validate(rules, list(zip(names, docs)))
        parsed = [parse_rules(t, n) for n, t in rules]
        want = {"PASS": 0, "FAIL": 1, "SKIP": 2}
        st = []
        for n, d in zip(names, docs):
            doc = load_document(d, n)
            for rf in parsed:
                st.append(want[E.eval_rules_file(rf, E.RootScope(rf, doc), n)])
        _expected[case] = (docs, names, exp, ecode, bytes(st))
    return _expected[case]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_prefix_memo_vs_oracle(case, mode):
    rules = CASES[case][0]
    docs, names, exp, ecode, statuses = _oracle(case)
    env = BATCH_ENV if case == "batches" and mode == 0 else {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    s = guard_amd.Session()
    try:
        s.configure(mode)
        for name, text in rules:
            s.add_rules(text, name)
        s.add_docs(docs, names)
        s.eval(1)
        assert s.stat(s.STAT["mode"]) == mode
        if mode == 0:
            assert s.stat(s.STAT["lane_group"]) == 1   # one lane per tile: the walker with the memo
            assert s.stat(s.STAT["retried"]) == 0      # and no tile handed to the wave kernel
        assert s.stat(s.STAT["errors"]) == 0
        assert s.tile_status(len(docs) * len(rules)) == statuses
        assert s.report() == (exp, ecode)
        if env:
            # more batches than waves in the grid: some wave took a second batch
            assert s.stat(s.STAT["lane_docs"]) == 1 and len(docs) * len(rules) > s.stat(s.STAT["lane_slots"]) > 0
    finally:
        s.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
