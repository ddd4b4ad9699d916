"""The rule sets, batches and cover predicate shared by tests/test_candidate_cover.py (the
emulation) and tests/test_gpu_candidate_cover.py (the device's own records).

DESIGN.md 3.5 claims that K2's candidates cover every true match end.  Here the true matches
come from the oracle's regexp over files made by tests/match_gen.py, and `cover` checks the
claim match by match against a set of (file, rule, end) candidates."""
import ctypes as C
import functools
import gzip
import json
import os
from dataclasses import dataclass

import numpy as np

from tests import helpers as H
from tests import match_gen as G
from tests.conftest import GOLDEN
from trivy_amd import _native as N
from trivy_amd import configs
from trivy_amd import secret as S

WHOLE = 0xFFFFFFFF
CHUNKS = (16, 64, 256)
GROUP_STATES = (None, 256, 64, 48, 24)

# The rule whose finding the resolver lost (its plan: a suffix program from the anchor
# ' secretblob', relaxed, cut to a prefix) and its twin without the unbounded prefix, whose
# program starts at the first atom.
BLOB_TAIL = r" SECRETBLOB\s*?-----(?P<secret>[a-z0-9]*k" + "[a-z0-9]" * 12 + ")-----END"
BLOB_RULES = [
    {"id": "blob", "category": "t", "title": "blob", "severity": "LOW", "secret-group-name": "secret",
     "regex": r"(?i)-----\s*?BEGIN[ A-Z0-9_-]*?" + BLOB_TAIL, "keywords": ["secretblob"]},
    {"id": "blob-twin", "category": "t", "title": "blob twin", "severity": "LOW", "secret-group-name": "secret",
     "regex": r"(?i)-----BEGIN" + BLOB_TAIL, "keywords": ["secretblob"]},
]

# A prefix-cut rule whose program starts at the first atom and whose prefix is bounded while
# the rule is not (group_states 24: relax 8, 10 atoms kept, rule_winback 14, maxlen -1), with
# a (?i)k in the prefix: in a file with U+212A the resolver takes its full-match ends from the
# fold-rune DFA, and those must not get the window of a prefix end.  Its findings were lost.
FOLDCUT_RULES = [
    {"id": "fold-cut", "category": "t", "title": "fold cut", "severity": "LOW",
     "regex": r"(?i)qqtoken=kabcdefghij[a-j]+END", "keywords": ["qqtoken"]},
]

# Empty-width assertions: every operation (^ $ \A \z (?m)^ (?m)$ \b \B) leading and trailing,
# \b and a line anchor inside an alternation or between atoms, beside a rule without any.
# (id, regex, keyword or None, the core string that tests/match_gen.py's context matrix puts
# between every `before` and `after` context.)  Each keyword is its rule's literal.
ASSERT_RULES = (
    ("mla", r"(?m)^mla=[a-f0-9]{8}$", "mla=", b"mla=0123abcd"),
    ("mlb", r"(?m)^mlb=[a-f0-9]{8}", "mlb=", b"mlb=0123abcd"),
    ("mlc", r"mlc=[a-f0-9]{8}(?m:$)", "mlc=", b"mlc=0123abcd"),
    ("wbd", r"\bwbd[0-9]{4}\b", "wbd", b"wbd1234"),
    ("wbe", r"wbe[0-9]{4}\b", "wbe", b"wbe1234"),
    ("nwf", r"\Bnwf[0-9]{4}\B", "nwf", b"nwf1234"),
    ("atg", r"\Aatg=[a-z]{4,9}", "atg=", b"atg=abcde"),
    ("zth", r"zth=[a-z]{4,9}\z", "zth=", b"zth=abcde"),
    ("csi", r"(?:^|,)csi=[a-z]{6}(?:,|$)", "csi=", b"csi=abcdef"),
    ("mlj", r"(?m)(?:^|\s)mlj\s*=\s*(?P<secret>[A-Za-z0-9]{12})\r?$", "mlj", b"mlj = Ab3dEf6hIj9l"),
    ("kwk", r"(?i)\bkwk_[a-z0-9]{10}\b", "kwk_", b"KwK_a1B2c3D4e5"),
    ("bgl", r"(?s)(?m)^bgl\{.*?\}$", "bgl{", b"bgl{ab\ncd}"),
    ("lzm", r"(?U)lzm=[a-z]+;", "lzm=", b"lzm=abc;"),
    ("wbn", r"wbn\b.\b[a-z]{3}", "wbn", b"wbn-abc"),
    ("up24", r"\b[A-Z0-9]{24}\b", None, b"AB12CD34EF56GH78IJ90KL12"),
    ("hex32", r"(?m)^[a-f0-9]{32}$", None, b"0123456789abcdef0123456789abcdef"),
    ("rud", r"(?m)^\s*rud\s*[:=]\s*[A-Za-z0-9+/]{20,}={0,2}$", "rud", b"rud: QWxhZGRpbjpvcGVuIHNlc2FtZQ=="),
    ("rue", r"(?i)(?:^|[^a-z0-9])rue[a-z0-9]{16}(?:[^a-z0-9]|$)", "rue", b"rueabcdefgh12345678"),
    ("ruf", r"(?m)^ruf-[a-z]+-[0-9]+\r?$", "ruf-", b"ruf-abc-123"),
    ("rug", r"(?s)\Arug.*zz\z", "rug", b"rug middle zz"),
)
ASSERT_CORE = {r[0]: r[3] for r in ASSERT_RULES}

# One DFA of max_rules_per_group = 64 rules: 70 rules gq<xy>_[0-9]{4} whose tails rotate through
# \b, nothing and $ in pairs (rule i: tail i // 2 % 3), so that the rules with local index 0, 31,
# 32 and 63 of the full group can all match in the middle of a file, and a rule without a
# length bound.
GROUP64_TAILS = (r"\b", "", "$")
GROUP64_N = 70
GROUP64_UNB = "gqzz"


def _gq(i):
    return "gq" + "abcdefghij"[i // 10] + "klmnopqrst"[i % 10]


def _rule(rid, regex, keyword):
    d = {"id": rid, "category": "t", "title": rid, "severity": "LOW", "regex": regex}
    if keyword:
        d["keywords"] = [keyword]
    return d


def assert_doc():
    return {"enable-builtin-rules": [H.AKIA_GROUP_RULE], "rules": [_rule(i, rx, kw) for i, rx, kw, _ in ASSERT_RULES]}


def group64_doc():
    rules = [_rule(_gq(i), _gq(i) + "_[0-9]{4}" + GROUP64_TAILS[i // 2 % 3], _gq(i) + "_") for i in range(GROUP64_N)]
    rules.append(_rule(GROUP64_UNB, r"(?s)gqzz\{.*\}", "gqzz{"))
    return {"enable-builtin-rules": [H.AKIA_GROUP_RULE], "rules": rules}



def _scanner(doc, group_states=None):
    if group_states is not None:
        N.knob("group_states", group_states)
    try:
        return S.NewScanner(None if doc is None else S.config_from_dict(doc))
    finally:
        if group_states is not None:
            N.knob("group_states", None)


def _user40_doc():
    rules = configs.user_rules_doc(1000, 4)["rules"]
    return {"enable-builtin-rules": [H.AKIA_GROUP_RULE],
            "rules": [rules[int(i)] for i in np.linspace(0, len(rules) - 1, 40).round()]}


@functools.lru_cache(maxsize=None)
def rule_set(name):
    """(scanner, the indices of the rules that the set's batch has files for).  Names:
    ("builtin", group_states), "blob", "foldcut", "k2", "hostonly", "user40", "assert",
    ("assert", 24), "group64"."""
    if isinstance(name, tuple) and name[0] == "builtin":
        sc = _scanner(None, name[1])
        return sc, tuple(range(len(sc.Rules)))
    if name == "blob":
        sc = _scanner({"enable-builtin-rules": [H.AKIA_GROUP_RULE], "rules": BLOB_RULES})
    elif name == "foldcut":
        sc = _scanner({"enable-builtin-rules": [H.AKIA_GROUP_RULE], "rules": FOLDCUT_RULES}, 24)
    elif name == "k2":
        sc = H.k2_scanner()
    elif name == "hostonly":
        sc = H.hostonly_scanner()
    elif name == "user40":
        sc = _scanner(_user40_doc())
    elif name == "assert":
        sc = _scanner(assert_doc())
    elif name == ("assert", 24):
        sc = _scanner(assert_doc(), 24)
    elif name == "group64":
        sc = _scanner(group64_doc())
    else:
        raise ValueError(name)
    builtin = {r.ID for r in S.builtin_rules()[0]}
    return sc, tuple(i for i, r in enumerate(sc.Rules) if r.ID not in builtin)


def set_id(name):
    return name if isinstance(name, str) else "%s-%s" % (name[0], "default" if name[1] is None else name[1])


ALL_SETS = tuple(("builtin", g) for g in GROUP_STATES) + ("blob", "foldcut", "k2", "hostonly", "user40",
                                                           "assert", ("assert", 24), "group64")
# the sets whose batches keep the files in which the oracle finds nothing: what catches a
# spurious finding
KEEP_UNMATCHED = ("assert", "group64")


@dataclass
class CoverBatch:
    batch: object      # S.Batch
    meta: list         # GenFile per file
    rule: list         # rule index per file
    truth: list        # per file: [(start, end)] of its rule, keyword gate applied (oracle)


def _batch_of(meta, rule, truth):
    args = [S.ScanArgs("g/%s/%d.txt" % (m.rule, i), m.body) for i, m in enumerate(meta)]
    return CoverBatch(S.Batch.from_args(args), meta, rule, truth)


# The device tests take their batches from committed fixtures (the oracle's modules are
# imported with tests/match_gen.py, but beside a GPU none of its regexps is compiled or
# run): tests/golden/candidate_cover/<set>.json.gz, written by
# `python -m tests.cover_common`; tests/test_candidate_cover.py checks that they are what the
# generator and the oracle give today.
FIXTURE_SETS = {"builtin": ("builtin", None), "user40": "user40", "foldcut": "foldcut", "assert": "assert",
                "group64": "group64"}


def _fixture_path(key):
    return os.path.join(GOLDEN, "candidate_cover", key + ".json.gz")


def fixture_rows(cb):
    return [[m.rule, m.cls, m.variant, m.placement, m.body.decode("latin-1"), m.fold, m.aux,
             [list(x) for x in t]] for m, t in zip(cb.meta, cb.truth)]


@functools.lru_cache(maxsize=None)
def fixture_batch(key):
    """The committed batch of FIXTURE_SETS[key]."""
    with gzip.open(_fixture_path(key), "rt", encoding="ascii") as f:
        rows = json.load(f)["files"]
    sc, _ = rule_set(FIXTURE_SETS[key])
    ids = {r.ID: i for i, r in enumerate(sc.Rules)}
    meta = [G.GenFile(r[0], r[1], r[2], r[3], r[4].encode("latin-1"), r[5], r[6]) for r in rows]
    return _batch_of(meta, [ids[m.rule] for m in meta], [[tuple(x) for x in r[7]] for r in rows])


def write_fixtures():
    os.makedirs(os.path.dirname(_fixture_path("x")), exist_ok=True)
    for key, name in FIXTURE_SETS.items():
        cb = cover_batch(name)
        with gzip.GzipFile(_fixture_path(key), "wb", mtime=0) as z:
            z.write(json.dumps({"generator": "python -m tests.cover_common (tests/match_gen.py, oracle/goregex.py)",
                                "files": fixture_rows(cb)}).encode("ascii"))
        print("%s: %d files, %d bytes" % (_fixture_path(key), len(cb.meta), os.path.getsize(_fixture_path(key))))


def _context_files(ru, take):
    """The "assert" set's files of one rule: the full (before, after) product wherever it
    falls, then every single context on the scan's geometry and the file-boundary pairs
    (tests/match_gen.py), the partner context of a single one being the first with which the
    oracle found a match in the product."""
    core = ASSERT_CORE[ru.ID]
    hit = [gf.variant.split("|") for gf in G.context_product(ru.ID, core) if take(gf)]
    before = next((b for b in G.BEFORE if any(h[0] == b[0] for h in hit)), G.BEFORE[1])
    after = next((a for a in G.AFTER if any(h[1] == a[0] for h in hit)), G.AFTER[1])
    for gf in G.context_geometry(ru.ID, core, before, after):
        take(gf)


def _group64_files(sc, r, own):
    """The "group64" set's files of rule r: the rule's shortest match at the end of a file
    and in the middle of one before a word character; for two rules the file with every
    rule's match on a line of its own; for the unbounded rule a body of 40,000 bytes (most of
    the batch: at chunk 128 the full group has fewer items than half the chunks and is
    listed); and, with the first rule of a group's upper half (local index 32), a file in
    which one 16-byte word of the batch holds the ends of two matches of rules with local
    index >= 32."""
    ru = sc.Rules[r]
    k = own.index(r)
    if ru.ID == GROUP64_UNB:
        return [G.GenFile(ru.ID, "g64", "unbounded", "long", b"qz gqzz{" + G.filler(40000) + b"} qz\n", False)]
    m = ("%s_%04d" % (ru.ID, k)).encode()
    out = [G.GenFile(ru.ID, "g64", "eof", "word/eof", b"qz " + m, False),
           G.GenFile(ru.ID, "g64", "mid", "mid/word", b"qz " + m + b"x qz\n", False)]
    if k % 35 == 0:
        lines = b"".join(("%s_%04d\n" % (sc.Rules[q].ID, j)).encode() for j, q in enumerate(own)
                         if sc.Rules[q].ID != GROUP64_UNB)
        out.append(G.GenFile(ru.ID, "g64", "all", "lines", lines, False))
    local = sc.group_table(sc.rule_group(r))["rules"]
    if len(local) > 32 and local[32] == r:
        # two rules of the upper half whose match may end before a space; the first match
        # ends at byte 17 of a file that starts a chunk, the second at byte 27
        two = [q for q in local[32:] if not sc.Rules[q].Regex.endswith("$")]
        a, b = (("%s_%04d" % (sc.Rules[q].ID, 7)).encode() for q in (two[0], two[-1]))
        for q in (two[0], two[-1]):
            out.append(G.GenFile(sc.Rules[q].ID, "g64", "two-ends", "word16@0", b"qz vx qz" + a + b" " + b + b" qz\n", False))
    return out


@functools.lru_cache(maxsize=None)
def cover_batch(name, reduced=True):
    """The generated files of a rule set in which the oracle finds a match of the file's
    rule (neighbour files are kept as they are; in the KEEP_UNMATCHED sets every file is
    kept).  It depends on the rules only: the builtin sets share one batch, and so do the
    plans of "assert"."""
    from oracle import goregex
    if isinstance(name, tuple) and name[1] is not None:
        return cover_batch((name[0], None) if name[0] == "builtin" else name[0], reduced)
    sc, own = rule_set(name)
    keep_all = name in KEEP_UNMATCHED
    meta, rule, truth = [], [], []
    for r in own:
        ru = sc.Rules[r]
        if not ru.Regex:
            continue
        rx = goregex.MustCompile(ru.Regex)
        kws = [k.lower().encode() for k in ru.Keywords]
        kept = set()

        def take(gf, r=r):
            gated = not kws or any(k in gf.body.lower() for k in kws)
            found = [tuple(m) for m in rx.FindAllIndex(gf.body)] if gated else []
            if not found and not gf.aux and not keep_all:
                return False
            meta.append(gf)
            rule.append(r)
            truth.append(found)
            if found:
                kept.add(gf.cls)
            return bool(found)

        if name == "assert":
            _context_files(ru, take)
            continue
        if name == "group64":
            ids = {x.ID: i for i, x in enumerate(sc.Rules)}
            for gf in _group64_files(sc, r, list(own)):
                if gf.rule == ru.ID:
                    take(gf)
                else:   # (the second rule of the two-ends file)
                    rx2 = goregex.MustCompile(sc.Rules[ids[gf.rule]].Regex)
                    meta.append(gf)
                    rule.append(ids[gf.rule])
                    truth.append([tuple(m) for m in rx2.FindAllIndex(gf.body)])
            continue
        for gf in G.files_for(ru.ID, ru.Regex, list(ru.Keywords), seed=r, reduced=reduced):
            take(gf)
        # a class whose variants matched at none of their rotating placements (a rule that
        # ends in $, say): its first file that matches among all placements
        for cls in G.CLASSES if reduced else ():
            if cls not in kept:
                any(take(gf) for gf in G.files_for(ru.ID, ru.Regex, list(ru.Keywords), seed=r, reduced=False,
                                                   only=(cls,)) if not gf.aux)
    # The chunks and words are the batch's, not the file's: a file whose placement aims at a
    # chunk or word boundary starts on a multiple of 256 bytes of the batch (a context file:
    # at its own offset modulo 256, G.phase_of), behind a filler file of the bytes that takes.
    meta0, rule0, truth0 = meta, rule, truth
    meta, rule, truth = [], [], []
    at = 0
    for m, r, t in zip(meta0, rule0, truth0):
        ph = G.phase_of(m)
        if ph is not None and at % 256 != ph:
            pad = G.GenFile(m.rule, m.cls, m.variant, "filler", G.filler((ph - at) % 256), False, True)
            meta.append(pad)
            rule.append(r)
            truth.append([])
            at += len(pad.body)
        meta.append(m)
        rule.append(r)
        truth.append(t)
        at += len(m.body)
    # the batch's last bytes are a match: the first kept file that ends in one, again
    k = next(i for i, m in enumerate(meta) if truth[i] and truth[i][-1][1] == len(m.body))
    meta.append(meta[k])
    rule.append(rule[k])
    truth.append(truth[k])
    return _batch_of(meta, rule, truth)


ANCHOR_KINDS = {1: "run U", 2: "run D", 1 << 31: "none"}   # any other event bit: a literal class


def plan_of(sc, r):
    """Everything the plan says about rule r (rule_plan, rule_program, rule_anchor)."""
    ev, d = C.c_uint32(), C.c_int64()
    desc = C.create_string_buffer(128)
    N.check(N.lib().tsg_ruleset_rule_anchor(sc.handle, r, C.byref(ev), C.byref(d), desc, 128))
    p = dict(sc.rule_plan(r))
    p.update(sc.rule_program(r))
    p.update(event=ev.value, evdist=d.value, anchor=desc.value.decode("utf-8", "replace"),
             kind=ANCHOR_KINDS.get(ev.value, "literal"))
    return p


def plan_line(sc, r):
    p = plan_of(sc, r)
    return ("%s: group %d relax %d maxlen %d first_atom %d rule_atoms %d winback %d rev %d anchor %s (%s) evdist %d" % (
        sc.Rules[r].ID, p["group"], p["relax"], p["maxlen"], p["first_atom"], p["rule_atoms"], p["rule_winback"],
        p["rule_rev"], p["kind"], p["anchor"], p["evdist"]))


def shapes_of(sc, rules):
    """The plan shapes among `rules` of a scanner, as a set of names."""
    out = set()
    for r in rules:
        if not sc.Rules[r].Regex:
            continue
        p = plan_of(sc, r)
        if p["group"] < 0:
            out.add("host-only")
            continue
        out.add("relax %d" % p["relax"])
        out.add("anchor " + p["kind"])
        if p["rule_atoms"] >= 0:
            out.add("prefix-cut, first_atom == 0" if p["first_atom"] == 0 else "prefix-cut, first_atom > 0")
            if p["rule_winback"] >= 0 and p["maxlen"] < 0:
                out.add("prefix-cut, bounded prefix of an unbounded rule")
        elif p["first_atom"] > 0:
            out.add("suffix without a cut")
    return out


ALL_SHAPES = {"relax %d" % k for k in (-1, 32, 16, 8, 4, 2, 1, 0)} | {
    "prefix-cut, first_atom == 0", "prefix-cut, first_atom > 0", "suffix without a cut",
    "prefix-cut, bounded prefix of an unbounded rule", "anchor run U", "anchor run D", "anchor literal", "anchor none", "host-only"}


def cover(sc, cb, triples, flags, chunk, ext_cap=S.DEFAULT_EXT_CAP):
    """Every true match [s, e) of a file's rule against the candidate set `triples`
    ((file, rule, end) rows, WHOLE ends kept) and the per-file flags (bits 0-1: overflow,
    folding runes: the resolver takes the file whole):
      an uncut rule needs the candidate (f, r, e); a prefix-cut rule one with s <= e' <= e;
      (f, r, WHOLE) excuses a match only of a rule without a length bound, or one longer
        than ext_cap;
      a host-only rule is excused; a flag excuses only in a file the generator marked fold.
    Raises on the first match that is neither covered nor excused, naming rule, variant,
    placement, chunk and plan.  Returns counts: ends, explicit, whole, host, flag, and
    `bounded` / `bounded_explicit` over the uncut rules with a length bound."""
    tri = np.asarray(triples, dtype=np.uint32).reshape(-1, 3)
    ends = {}
    for f, r, e in tri.tolist():
        ends.setdefault((f, r), set()).add(e)
    plans = {}
    n = dict(ends=0, explicit=0, whole=0, host=0, flag=0, bounded=0, bounded_explicit=0)
    for f, found in enumerate(cb.truth):
        r = cb.rule[f]
        if r not in plans:
            plans[r] = plan_of(sc, r)
        p = plans[r]
        have = ends.get((f, r), ())
        for s, e in found:
            n["ends"] += 1
            if p["group"] < 0:
                n["host"] += 1
                continue
            cut = p["rule_atoms"] >= 0
            bounded = not cut and p["maxlen"] >= 0
            n["bounded"] += bounded
            if (any(s <= x <= e for x in have if x != WHOLE) if cut else e in have):
                n["explicit"] += 1
                n["bounded_explicit"] += bounded
            elif WHOLE in have and (p["maxlen"] < 0 or e - s > ext_cap):
                n["whole"] += 1
            elif (int(flags[f]) & 3) and cb.meta[f].fold:
                n["flag"] += 1
            else:
                m = cb.meta[f]
                raise AssertionError(
                    "match [%d, %d) of file %d is not covered: rule %s, variant %s %s, placement %s, chunk %d, "
                    "flags %d, candidates %s\n  plan: %s" % (
                        s, e, f, m.rule, m.cls, m.variant, m.placement, chunk, int(flags[f]),
                        sorted(have)[:12], plan_line(sc, r)))
    return n


if __name__ == "__main__":
    write_fixtures()
