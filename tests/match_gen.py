"""Boundary-match generator: for one Go regexp, strings that match it at the edges of its
structure, placed into files at the edges of the scan's geometry.

The structure comes from the oracle's own Go-syntax parser (oracle.goregex.parse), not from
the product: repetitions at their bounds and far past their lower bound, every alternation
branch, the lowest / highest / multi-byte members of every set, both cases of a (?i) letter
and, as a class of their own, the runes U+017F / U+212A that (?i) folds onto s / k.  The
generator does not decide what matches: the oracle's FindAllIndex does, and a file in which
it finds nothing is dropped (tests/test_candidate_cover.py).

The context matrix (below) is the other way round: the string stays, the bytes around it
change.  It is for empty-width assertions, and there the files without a match are kept.

variants(src)          -> [(variant class, variant name, str)]
files_for(rule, ...)   -> [GenFile]: the variants of one rule at their placements
context_product(..)    -> [GenFile]: one core string between every before / after pair
context_geometry(..)   -> [GenFile]: every single context on chunk, word and file boundaries
"""
import random
from dataclasses import dataclass

from oracle import gounicode as U
from oracle import goregex

LONG = (700, 5000)            # an unbounded repetition runs lo + these: many chunks, > 4 KiB
MAX_CHARS = 24000             # a variant longer than this is not generated (nested repetitions)
FOLD_RUNES = (0x17F, 0x212A)  # (?i)s and (?i)k fold onto them
CLASSES = ("lo", "hi", "alt", "long", "nonascii", "case", "fold", "random")
_ASSERT = ("bot", "eot", "bol", "eol", "wb", "nwb", "empty")
_SURR = (0xD800, 0xDFFF)
BAD_BYTE = 0xDCFF             # the byte FF under surrogateescape: invalid UTF-8
_QUIET = "qz vx "             # filler: letters of no builtin keyword or anchor literal


def _width(cp):
    return 1 if cp < 0x80 else 2 if cp < 0x800 else 3 if cp < 0x10000 else 4


def _members(ranges, lo, hi):
    """The first code point of `ranges` within [lo, hi] that is no surrogate, or None."""
    for a, b in ranges:
        a, b = max(a, lo), min(b, hi)
        while a <= b and _SURR[0] <= a <= _SURR[1]:
            a = _SURR[1] + 1
        if a <= b:
            return a
    return None


def _lowest(ranges):
    return _members(ranges, 0, U.MAX_RUNE)


def _highest(ranges):
    for a, b in reversed(ranges):
        while b >= a and _SURR[0] <= b <= _SURR[1]:
            b = _SURR[0] - 1
        if b >= a:
            return b
    return None


def _plain(ranges):
    """A tame member: a lower-case letter, a digit, an upper-case letter, printable ASCII,
    else the lowest code point."""
    for lo, hi in ((0x61, 0x7A), (0x30, 0x39), (0x41, 0x5A), (0x21, 0x7E), (0x20, 0x20)):
        cp = _members(ranges, lo, hi)
        if cp is not None:
            return cp
    return _lowest(ranges)


_ANY = [(0, U.MAX_RUNE)]
_ANYNOTNL = [(0, 9), (11, U.MAX_RUNE)]


class _Chooser:
    """One variant's decisions: repetition counts, alternation branches, set members."""

    def __init__(self, reps="lo", alt=0, chars="plain", long_rep=None, long_by=0, rng=None):
        self.reps, self.alt, self.chars = reps, alt, chars
        self.long_rep, self.long_by = long_rep, long_by
        self.rng = rng
        self.n_unbounded = 0    # unbounded repetitions met, in generation order
        self.n_alts = 0         # the widest alternation met
        self.budget = MAX_CHARS

    def count(self, lo, hi):
        if hi < 0:
            k = self.n_unbounded
            self.n_unbounded += 1
            if self.long_rep is not None:
                return lo + (self.long_by if k == self.long_rep else 0)
            if self.reps == "random":
                return lo + int(self.rng.choice((0, 1, 2, 3, 7, 17, 40)))
            return lo if self.reps == "lo" else lo + 3
        if self.reps == "random":
            return self.rng.choice((lo, hi, self.rng.randint(lo, hi)))
        return lo if self.reps == "lo" or self.long_rep is not None else hi

    def branch(self, n):
        self.n_alts = max(self.n_alts, n)
        if self.alt == "random":
            return self.rng.randrange(n)
        return n - 1 if self.alt == "last" else self.alt % n

    def member(self, ranges, orbit=None):
        how = self.chars
        if how == "random":
            how = self.rng.choice(("plain", "plain", "any", "any", "upper", "u2", "u3", "u4", "nl", "low", "high"))
        cp = None
        if how != "fold":
            # the folding runes sit in a (?i) set beside its letters: they are the "fold"
            # variants' alone, so that the other classes' files stay free of them
            kept = [r for r in ranges if not (r[0] == r[1] and r[0] in FOLD_RUNES)]
            ranges = kept or ranges
        if how == "bad":      # an invalid byte decodes as U+FFFD, one byte wide
            return BAD_BYTE if _members(ranges, 0xFFFD, 0xFFFD) is not None else _plain(ranges)
        if how == "low":
            cp = _lowest(ranges)
        elif how == "high":
            cp = _highest(ranges)
        elif how == "u2":
            cp = _members(ranges, 0x80, 0x7FF)
        elif how == "u3":
            cp = _members(ranges, 0x800, 0xFFFF)
        elif how == "u4":
            cp = _members(ranges, 0x10000, U.MAX_RUNE)
        elif how == "nl":
            cp = _members(ranges, 10, 10)
        elif how == "upper":
            cp = _members(ranges, 0x41, 0x5A)
        elif how == "lower":
            cp = _members(ranges, 0x61, 0x7A)
        elif how == "fold":
            # a folding rune where it is in the set through an orbit (its neighbours are not)
            for f in FOLD_RUNES:
                if _members(ranges, f, f) is not None and _members(ranges, f + 1, f + 1) is None:
                    cp = f
        elif how == "any":
            a, b = self.rng.choice(ranges)
            cp = _members([(a, b)], self.rng.randint(a, b), b)
        return _plain(ranges) if cp is None else cp


def _gen(node, ch, out):
    k = node[0]
    if ch.budget < 0:
        return
    if k == "lit":
        r = node[1]
        if node[2]:
            orb = U.fold_orbit(r)
            if len(orb) > 1:
                r = ch.member([(o, o) for o in sorted(orb)])
        out.append(chr(r))
        ch.budget -= 1
    elif k == "class":
        if not node[1]:
            ch.budget = -1   # the empty set matches nothing
            return
        out.append(chr(ch.member(node[1])))
        ch.budget -= 1
    elif k == "any":
        out.append(chr(ch.member(_ANY)))
        ch.budget -= 1
    elif k == "anynotnl":
        out.append(chr(ch.member(_ANYNOTNL)))
        ch.budget -= 1
    elif k == "cat":
        for x in node[1]:
            _gen(x, ch, out)
    elif k == "alt" and ch.alt == "longest":
        # the branch that generates the most bytes
        ch.n_alts = max(ch.n_alts, len(node[1]))
        best = None
        for x in node[1]:
            sub = []
            _gen(x, ch, sub)
            if best is None or len(_enc("".join(sub))) > len(_enc("".join(best))):
                best = sub
        out.extend(best)
    elif k == "alt":
        _gen(node[1][ch.branch(len(node[1]))], ch, out)
    elif k == "rep":
        for _ in range(ch.count(node[1], node[2])):
            _gen(node[4], ch, out)
            if ch.budget < 0:
                return
    elif k == "cap":
        _gen(node[2], ch, out)
    elif k == "group":
        _gen(node[1], ch, out)
    else:
        assert k in _ASSERT, node


def _one(ast, **kw):
    ch = _Chooser(**kw)
    out = []
    _gen(ast, ch, out)
    return (None if ch.budget < 0 else "".join(out)), ch


def variants(src, seed=0, nrandom=3):
    """[(variant class, name, string)] of one regexp, without duplicates of a string within
    a class.  Classes: lo, hi, alt, long, nonascii, case, fold, random."""
    ast = goregex.parse(src)
    got = []
    seen = set()

    def add(cls, name, s):
        if s is None or s == "" or (cls, s) in seen:
            return
        if cls == "nonascii" and s.isascii():
            return
        if cls == "fold" and not any(chr(f) in s for f in FOLD_RUNES):
            return
        seen.add((cls, s))
        got.append((cls, name, s))

    s, probe = _one(ast, reps="lo", alt=0, chars="plain")
    add("lo", "lo/first/plain", s)
    add("lo", "lo/last/low", _one(ast, reps="lo", alt="last", chars="low")[0])
    add("hi", "hi/last/plain", _one(ast, reps="hi", alt="last", chars="plain")[0])
    add("hi", "hi/first/high", _one(ast, reps="hi", alt=0, chars="high")[0])
    # the longest match in bytes: where the planner's byte distances are met exactly
    add("hi", "hi/longest/high", _one(ast, reps="hi", alt="longest", chars="high")[0])
    add("hi", "hi/longest/plain", _one(ast, reps="hi", alt="longest", chars="plain")[0])
    for b in range(probe.n_alts):
        add("alt", "branch%d/lo" % b, _one(ast, reps="lo", alt=b, chars="plain")[0])
        add("alt", "branch%d/hi" % b, _one(ast, reps="hi", alt=b, chars="plain")[0])
    # which unbounded repetitions there are depends on the branch taken: both ends
    for alt in (0, "last"):
        n = _one(ast, reps="lo", alt=alt, chars="plain")[1].n_unbounded
        for k in range(n):
            for by in LONG:
                add("long", "rep%d+%d/%s" % (k, by, alt), _one(ast, alt=alt, long_rep=k, long_by=by)[0])
    for how in ("u2", "u3", "u4", "nl"):
        add("nonascii" if how != "nl" else "hi", "hi/first/" + how, _one(ast, reps="hi", alt=0, chars=how)[0])
        add("nonascii" if how != "nl" else "hi", "hi/last/" + how, _one(ast, reps="hi", alt="last", chars=how)[0])
    add("nonascii", "hi/last/high", _one(ast, reps="hi", alt="last", chars="high")[0])
    add("nonascii", "hi/first/bad", _one(ast, reps="hi", alt=0, chars="bad")[0])
    for how in ("upper", "lower"):
        add("case", "lo/first/" + how, _one(ast, reps="lo", alt=0, chars=how)[0])
        add("case", "hi/last/" + how, _one(ast, reps="hi", alt="last", chars=how)[0])
    add("fold", "lo/first/fold", _one(ast, reps="lo", alt=0, chars="fold")[0])
    add("fold", "hi/last/fold", _one(ast, reps="hi", alt="last", chars="fold")[0])
    rng = random.Random("%d:%s" % (seed, src))
    for k in range(nrandom):
        add("random", "random%d" % k, _one(ast, reps="random", alt="random", chars="random", rng=rng)[0])
    return got


# ------------------------------------------------------------------------------ placements
@dataclass
class GenFile:
    rule: str          # rule id
    cls: str           # variant class
    variant: str       # variant name
    placement: str
    body: bytes
    fold: bool         # holds U+017F / U+212A: the resolver may take the file whole
    aux: bool = False  # a neighbour file, kept whether or not anything matches in it


def filler(n):
    """n bytes of quiet words ending in a newline."""
    if n <= 0:
        return b""
    s = (_QUIET * (n // len(_QUIET) + 1))[:n - 1] + "\n"
    return s.encode()


def _pad_to(pre_len, at, mod):
    """Filler length so that offset pre_len + filler + at is a multiple of mod."""
    return (-(pre_len + at)) % mod


def _enc(s):
    return s.encode("utf-8", "surrogateescape")


ALIGNED = ("straddle16", "straddle256", "end16", "chunk-end")   # aim at offsets of the batch
PLACEMENTS = ("start", "word/eof", "space/nl", "nl/word", "straddle16", "straddle256", "end16", "twice",
              "truncated", "behind-keyword", "behind-prefix", "chunk-end")


def place(s, keywords, placement):
    """[(body, aux)] of string s at one placement; the keywords stand on a first line of their
    own (for "start": on a last one, the match begins the file)."""
    kw = (" ".join(keywords) + "\n").encode() if keywords else b""
    m = _enc(s)
    if placement == "start":
        return [(m + b"\n" + kw, False)]
    if placement == "word/eof":      # after a word character; the match ends the file
        return [(kw + b"a" + m, False)]
    if placement == "space/nl":
        return [(kw + b"qz " + m + b"\n", False)]
    if placement == "nl/word":
        return [(kw + m + b"z", False)]
    if placement in ("straddle16", "straddle256"):
        mod = 16 if placement == "straddle16" else 256
        if len(m) < 2:
            return []
        pad = _pad_to(len(kw), len(m) // 2, mod)   # a chunk boundary in the middle of the match
        return [(kw + filler(pad) + m + b"\n", False)]
    if placement == "chunk-end":
        # the match starts at the last byte of a chunk of 16, 64 and 256 bytes: with a
        # longest variant its anchor lies as many chunks behind its start as it ever can
        pad = _pad_to(len(kw), 1, 256)
        return [(kw + filler(pad) + m + b"\n", False)]
    if placement == "end16":         # the match ends on a 16-byte word boundary
        pad = _pad_to(len(kw), len(m), 16)
        return [(kw + filler(pad) + m + b" qz\n", False)]
    if placement == "twice":
        return [(kw + m + m + b"\n", False)]
    if placement == "truncated":
        cut = _enc(s[:max(1, (2 * len(s)) // 3)])
        return [(kw + m + cut, False)]
    if placement == "behind-keyword":
        # the batch is one byte stream: the file before ends in the rule's keyword
        if not keywords:
            return []
        return [(b"qz " + keywords[0].encode(), True), (m + b"\n" + kw, False)]
    if placement == "behind-prefix":
        return [(kw + b"qz " + _enc(s[:max(1, len(s) // 2)]), True), (m + b"\n" + kw, False)]
    raise ValueError(placement)


def features(src):
    """What the regexp's structure admits: {"unbounded": it has a repetition without an upper
    bound, "nonascii": one of its sets holds a rune past ASCII that is no folding rune}."""
    out = {"unbounded": False, "nonascii": False}

    def walk(node):
        k = node[0]
        if k in ("any", "anynotnl"):
            out["nonascii"] = True
        elif k == "class":
            out["nonascii"] |= any(b >= 0x80 and not (a == b and a in FOLD_RUNES) for a, b in node[1])
        elif k == "lit" and node[2]:
            out["nonascii"] |= any(o >= 0x80 and o not in FOLD_RUNES for o in U.fold_orbit(node[1]))
        elif k == "lit":
            out["nonascii"] |= node[1] >= 0x80
        elif k in ("cat", "alt"):
            for x in node[1]:
                walk(x)
        elif k == "rep":
            out["unbounded"] |= node[2] < 0
            walk(node[4])
        elif k == "cap":
            walk(node[2])
        elif k == "group":
            walk(node[1])
    walk(goregex.parse(src))
    return out


def files_for(rule_id, src, keywords, seed=0, reduced=True, only=None):
    """The files of one rule.  reduced: each variant at two placements that rotate through
    the list (a long-repetition or folding-rune variant at one), instead of at every
    placement.  only: the variant classes wanted."""
    out = []
    k = 0
    for cls, name, s in variants(src, seed):
        if only is not None and cls not in only:
            continue
        if reduced:
            n = 1 if cls in ("long", "fold") else 2
            pls = [PLACEMENTS[(k + j * 5) % len(PLACEMENTS)] for j in range(n)]
            k += 1
            # the variants with every repetition at its upper bound are the longest: where
            # the planner's distances (anchor behind the start, window before the end) are
            # met exactly, so they always get the placement that tests those
            if cls in ("hi", "alt", "nonascii") and "hi" in name.split("/") and "chunk-end" not in pls:
                pls.append("chunk-end")
        else:
            pls = PLACEMENTS if cls != "long" else PLACEMENTS[:7] + PLACEMENTS[-1:]
        for pl in pls:
            for body, aux in place(s, keywords, pl):
                fold = b"\xc5\xbf" in body or b"\xe2\x84\xaa" in body
                out.append(GenFile(rule_id, cls, name, pl, body, fold, aux))
    return out


# ------------------------------------------------------------------------ context matrix
# Empty-width assertions are decided by the bytes around a match, not by the match: one core
# string per rule between every `before` and every `after` context.  "bot" / "eot": the core
# begins / ends the file.
BEFORE = (("bot", b""), ("nl", b"\n"), ("crlf", b"\r\n"), ("a", b"a"), ("_", b"_"), ("9", b"9"), ("sp", b" "),
          ("comma", b","), ("e-acute", "é".encode()), ("ff", b"\xff"))
AFTER = (("eot", b""), ("nl", b"\n"), ("crlf", b"\r\n"), ("cr", b"\r"), ("a", b"a"), ("_", b"_"), ("0", b"0"),
         ("sp", b" "), ("comma", b","), ("e-acute", "é".encode()), ("ff", b"\xff"))
# where a single context is put on the scan's geometry: the core starts on a 256-byte multiple
# of the batch (its context byte is the previous chunk's last byte), ends on one (the
# look-ahead byte is the next chunk's first), ends on a 16-byte word end that is no end of a
# 64- or 256-byte chunk, and has a 256-byte multiple in its middle
GEOMETRY = ("start256", "end256", "end16", "mid256")
PAIR_AT = 100   # a file boundary in the middle of a chunk of 256 bytes, and of a 16-byte word


def phase_of(gf):
    """The offset modulo 256 of the batch at which a file wants to start (None: anywhere): 0
    for the ALIGNED placements, the number behind '@' for a context file."""
    if gf.placement in ALIGNED:
        return 0
    return int(gf.placement.split("@")[1]) if "@" in gf.placement else None


def _ctx(rule_id, before, core, after, placement, at=None, aux=False):
    body = before[1] + core + after[1]
    if at is not None:
        placement = "%s@%d" % (placement, at % 256)
    return GenFile(rule_id, "ctx", before[0] + "|" + after[0], placement, body, False, aux)


def context_product(rule_id, core):
    """One file per (before, after) pair, wherever it falls in the batch."""
    return [_ctx(rule_id, b, core, a, "product") for b in BEFORE for a in AFTER]


def context_geometry(rule_id, core, before, after):
    """Every single context at the four GEOMETRY placements -- each `before` with the partner
    `after`, each `after` with the partner `before` -- and the file-boundary pairs: a file that
    ends in a word character without a newline before one that begins with the core (the
    file's start must win over the neighbour's byte), and a file that ends with the core
    before one that begins with a word character (the file's end must win), each with the
    boundary inside a chunk and on a 256-byte multiple of the batch."""
    out = []
    nc = len(core)
    singles = [(b, after) for b in BEFORE] + [(before, a) for a in AFTER]
    for b, a in singles:
        nb = len(b[1])
        for pl, at in (("start256", -nb), ("end256", -(nb + nc)), ("end16", 48 - (nb + nc)),
                       ("mid256", -(nb + nc // 2))):
            out.append(_ctx(rule_id, b, core, a, pl, at))
    word = (("word", b"qz vxa"), ("", b""))
    for pl, at in (("bot-pair", PAIR_AT), ("bot-pair256", 0)):
        out.append(_ctx(rule_id, word[0], b"", word[1], pl, at - len(word[0][1]), aux=True))
        out.append(_ctx(rule_id, BEFORE[0], core, after, pl))
    for pl, at in (("eot-pair", PAIR_AT), ("eot-pair256", 0)):
        out.append(_ctx(rule_id, before, core, AFTER[0], pl, at - len(before[1]) - nc))
        out.append(GenFile(rule_id, "ctx", "|word", pl, b"a qz\n", False, True))
    return out
