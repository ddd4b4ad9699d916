"""Every plan the suite can reach, pinned by its digest (tsg_ruleset_plan_digest: a hash of
every member of the compiled plan).  tests/golden/plan_digests.json was recorded before
build_plan was split into passes, from a library that differed from that commit's parent by
the digest hook alone (`python -m tests.test_plan_digest` writes it); a refactor of the plan
construction must leave every digest as it is.  Each entry also holds the rule set's info(),
so that a mismatch reads as more than two numbers.

The cases: the builtin rules at every group size the suite uses, the rule sets of
tests/cover_common.py, the user rule sets of trivy_amd/configs.py at every K1X step, and with
the no_k1x knob the K1 fallback that leaves keywords out of the automaton."""
import json
import os

import pytest

from tests import cover_common as CC
from tests.conftest import GOLDEN
from trivy_amd import _native as N
from trivy_amd import configs
from trivy_amd import secret as S

GOLDEN_FILE = os.path.join(GOLDEN, "plan_digests.json")

# case id -> (rule set, knobs set around the compile)
CASES = {}
for g in CC.GROUP_STATES:
    CASES[CC.set_id(("builtin", g))] = ("builtin", {} if g is None else {"group_states": g})
CASES["builtin-table32"] = ("builtin", {"group_table_kib": 32})
CASES["builtin-1024-table48"] = ("builtin", {"group_states": 1024, "group_table_kib": 48})
COVER_SETS = ("blob", "foldcut", "k2", "hostonly", "user40", "assert", ("assert", 24), "group64")
for name in COVER_SETS:
    CASES[CC.set_id(name)] = (name, {})
CASES["user100"] = ("user100", {})
CASES["user100-no_k1x"] = ("user100", {"no_k1x": 1})
CASES["user1000"] = ("user1000", {})
for step in (4, 2, 1):
    CASES["user1000-x_step%d" % step] = ("user1000", {"x_step": step})
CASES["user1000-no_k1x"] = ("user1000", {"no_k1x": 1})
CASES["allow-exclude"] = ("allow-exclude", {})


def compile_case(case):
    rules, knobs = CASES[case]
    if rules in COVER_SETS:
        return CC.rule_set(rules)[0]   # (they set their own knobs, and are shared with other tests)
    doc = {"builtin": lambda: None, "user100": lambda: configs.user_rules_doc(100, seed=4),
           "user1000": lambda: configs.user_rules_doc(1000, seed=4),
           "allow-exclude": configs.allow_exclude_doc}[rules]()
    for k, v in knobs.items():
        N.knob(k, v)
    try:
        return S.NewScanner(None if doc is None else S.config_from_dict(doc))
    finally:
        for k in knobs:
            N.knob(k, None)


def entry(case):
    sc = compile_case(case)
    return {"digest": "%016x" % sc.plan_digest(), "info": sc.info()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_golden_holds_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", list(CASES))
def test_plan_digest(golden, case):
    got = entry(case)
    print(case, got)
    assert got == golden[case]


if __name__ == "__main__":
    import sys
    out = {case: entry(case) for case in CASES}
    if "--print" in sys.argv:   # the stability check: compare the output of several processes
        print(json.dumps(out, indent=1, sort_keys=True))
    else:
        with open(GOLDEN_FILE, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote %s: %d cases" % (GOLDEN_FILE, len(out)))
