"""The product's rule data (trivy_amd/rules/builtin_rules.json) against the reference's
Go source, re-read here with a parser independent of tools/gen_builtin_rules.py.

gen_builtin_rules.py splits the rule table with regexes; this test tokenizes the Go
source (string literals, identifiers, punctuation), walks the composite literal
`var builtinRules = []Rule{ ... }` by brace depth, and evaluates the only expression forms
the table uses: string literals, the pattern constants, `MustCompile(x)` and
`fmt.Sprintf(fmt, args...)` with `%s` verbs.  Every field of every rule and allow rule is
compared, so a transcription error in any of the 83 rules fails here, not only in the
dozen rules the reference fixtures exercise.

The Go source is not part of this repository.  What that parse found is recorded in
tests/golden/builtin_rules_go_digest.json: per rule and allow rule, in table order, its ID
and the sha256 of its canonical field record (every field of the table, absent ones with
Go's zero value).  The tests compare the product's rule data with that record, so they
need nothing outside the tree.  Where a checkout of the reference is at hand,

    TSG_REFERENCE_SRC=<reference>/pkg/fanal/secret python -m pytest tests/test_rules_data.py

also re-parses the Go source, compares it field by field as well, and checks that the
record is that parse's; `python -m tests.test_rules_data --record` rewrites the record from
it."""
import hashlib
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("TSG_REFERENCE_SRC", "")
RULES_JSON = os.path.join(os.path.dirname(HERE), "trivy_amd", "rules", "builtin_rules.json")
DIGESTS = os.path.join(HERE, "golden", "builtin_rules_go_digest.json")


def tokenize(src):
    """Go tokens: ('str', value) | ('id', name) | ('p', char).  Comments are dropped."""
    toks, i, n = [], 0, len(src)
    esc = {"n": "\n", "t": "\t", "r": "\r", '"': '"', "\\": "\\", "'": "'"}
    while i < n:
        c = src[i]
        if c.isspace():
            i += 1
        elif src.startswith("//", i):
            i = src.index("\n", i)
        elif src.startswith("/*", i):
            i = src.index("*/", i) + 2
        elif c == "`":
            j = src.index("`", i + 1)
            toks.append(("str", src[i + 1:j]))
            i = j + 1
        elif c == '"':
            out, j = [], i + 1
            while src[j] != '"':
                if src[j] == "\\":
                    out.append(esc[src[j + 1]])
                    j += 2
                else:
                    out.append(src[j])
                    j += 1
            toks.append(("str", "".join(out)))
            i = j + 1
        elif c.isalnum() or c == "_":
            j = i
            while j < n and (src[j].isalnum() or src[j] == "_"):
                j += 1
            toks.append(("id", src[i:j]))
            i = j
        else:
            toks.append(("p", c))
            i += 1
    return toks


class Walker:
    def __init__(self, toks, consts):
        self.t, self.k, self.consts = toks, 0, consts

    def peek(self, o=0):
        return self.t[self.k + o]

    def take(self, kind=None, val=None):
        tok = self.t[self.k]
        assert kind is None or tok[0] == kind, tok
        assert val is None or tok[1] == val, tok
        self.k += 1
        return tok

    def expr(self):
        kind, v = self.take()
        if kind == "str":
            return v
        if kind == "id" and v == "MustCompile":
            self.take("p", "(")
            x = self.expr()
            self.take("p", ")")
            return x
        if kind == "id" and v == "fmt":
            self.take("p", ".")
            self.take("id", "Sprintf")
            self.take("p", "(")
            args = [self.expr()]
            while self.peek() == ("p", ","):
                self.take()
                args.append(self.expr())
            self.take("p", ")")
            fmt, rest = args[0], args[1:]
            assert fmt.count("%s") == len(rest) and "%" not in fmt.replace("%s", "")
            for a in rest:
                fmt = fmt.replace("%s", a, 1)
            return fmt
        if kind == "id" and v == "types":  # types.SecretRuleCategory("X")
            self.take("p", ".")
            self.take("id")
            self.take("p", "(")
            x = self.expr()
            self.take("p", ")")
            return x
        if kind == "id" and v == "nil":
            return None
        if kind == "id" and v == "[":
            raise AssertionError
        if kind == "id":
            return self.consts[v]
        if (kind, v) == ("p", "["):  # []string{...}
            self.take("p", "]")
            self.take("id", "string")
            self.take("p", "{")
            out = []
            while self.peek() != ("p", "}"):
                out.append(self.expr())
                if self.peek() == ("p", ","):
                    self.take()
            self.take("p", "}")
            return out
        raise AssertionError((kind, v))

    def struct(self):
        """{ Field: expr, ... } -> dict"""
        self.take("p", "{")
        d = {}
        while self.peek() != ("p", "}"):
            name = self.take("id")[1]
            self.take("p", ":")
            d[name] = self.expr()
            if self.peek() == ("p", ","):
                self.take()
        self.take("p", "}")
        return d

    def slice_of_structs(self, var):
        while not (self.peek() == ("id", var) and self.peek(1) == ("p", "=")):
            self.k += 1
        self.k += 2
        self.take("p", "[")
        self.take("p", "]")
        self.take("id")
        self.take("p", "{")
        out = []
        while self.peek() != ("p", "}"):
            out.append(self.struct())
            if self.peek() == ("p", ","):
                self.take()
        return out


def consts_of(toks):
    """Every `Name = "lit"` / `Name = types.SecretRuleCategory("lit")` in const blocks."""
    consts = {}
    w = Walker(toks, consts)
    for i in range(len(toks) - 2):
        if toks[i][0] == "id" and toks[i + 1] == ("p", "=") and i > 0 and toks[i - 1][1] != "var":
            if toks[i + 2][0] == "str" or toks[i + 2] == ("id", "types"):
                w.k = i + 2
                consts[toks[i][1]] = w.expr()
    return consts


RULE_KEYS = ("id", "category", "title", "severity", "regex", "secret_group_name", "keywords")
ALLOW_KEYS = ("id", "description", "regex", "path")


def digest(record):
    return hashlib.sha256(json.dumps(record, sort_keys=True, ensure_ascii=True).encode()).hexdigest()


def go_rules():
    """The rule table of the Go source as canonical field records."""
    src = open(os.path.join(REF, "builtin-rules.go")).read()
    toks = tokenize(src)
    consts = consts_of(toks)
    rules = Walker(toks, consts).slice_of_structs("builtinRules")
    for go in rules:
        assert set(go) <= {"ID", "Category", "Title", "Severity", "Regex", "SecretGroupName",
                           "Keywords"}, go["ID"]
    return [{"id": go["ID"], "category": go["Category"], "title": go["Title"],
             "severity": go.get("Severity", ""), "regex": go["Regex"],
             "secret_group_name": go.get("SecretGroupName", ""),
             "keywords": go.get("Keywords", [])} for go in rules]


def go_allow_rules():
    src = open(os.path.join(REF, "builtin-allow-rules.go")).read()
    allow = Walker(tokenize(src), {}).slice_of_structs("builtinAllowRules")
    return [{"id": go["ID"], "description": go.get("Description", ""), "regex": go.get("Regex"),
             "path": go.get("Path")} for go in allow]


def _recorded(records):
    return [{"id": r["id"], "sha256": digest(r)} for r in records]


def _check(mine, keys, recorded, parse):
    assert len(mine) == len(recorded)
    for j, rec in zip(mine, recorded):
        assert j["id"] == rec["id"]
        assert digest({k: j[k] for k in keys}) == rec["sha256"], rec["id"]
    if REF:  # a checkout of the reference: every field by name, and the record itself
        go = parse()
        assert _recorded(go) == recorded
        for g, j in zip(go, mine):
            for k in keys:
                assert j[k] == g[k], (g["id"], k)


def test_builtin_rules_match_go_source():
    mine = json.load(open(RULES_JSON))["rules"]
    recorded = json.load(open(DIGESTS))["rules"]
    assert len(recorded) == 83
    _check(mine, RULE_KEYS, recorded, go_rules)


def test_builtin_allow_rules_match_go_source():
    mine = json.load(open(RULES_JSON))["allow_rules"]
    recorded = json.load(open(DIGESTS))["allow_rules"]
    assert len(recorded) == 12
    _check(mine, ALLOW_KEYS, recorded, go_allow_rules)


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv and REF:
        with open(DIGESTS, "w") as f:
            json.dump({"rules": _recorded(go_rules()), "allow_rules": _recorded(go_allow_rules())}, f, indent=1)
            f.write("\n")
    else:
        raise SystemExit("usage: TSG_REFERENCE_SRC=<reference>/pkg/fanal/secret python -m tests.test_rules_data --record")
