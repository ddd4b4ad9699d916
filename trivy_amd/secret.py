"""Host-side mirror of trivy's `pkg/fanal/secret` API over the native engine.

Same names, argument meaning and error behaviour as the reference:
  Config / Rule / AllowRule / ExcludeBlock / Global      scanner.go:23-94, 186-225
  ParseConfig(path) -> Config | None                      scanner.go:267-291
  NewScanner(config) -> Scanner                           scanner.go:293-329
  Scanner.Scan(ScanArgs) -> Secret                        scanner.go:341-416 (exact, CPU)
  Scanner.AllowPath(path)                                 scanner.go:55-57
and the batching boundary the GPU needs:
  Scanner.ScanBatch([ScanArgs], device=...) -> [Secret]   (K1 + K2 on the MI355X, exact
                                                          host resolution of candidates)

`Secret` values are dicts shaped like Go's types.Secret:
  {"FilePath": str, "Findings": None | [SecretFinding]}
with SecretFinding = {"RuleID", "Category", "Severity", "Title", "StartLine", "EndLine",
"Code": {"Lines": [Line]}, "Match"}; Match and line Content/Highlighted are `bytes`
(Go strings are byte strings; content need not be valid UTF-8).
"""
import ctypes as C
import json
import os
import struct
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import yaml

from . import _native as N

_RULES_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rules",
                           "builtin_rules.json")


class ConfigError(ValueError):
    """secrets config decode / regexp compile error (scanner.go:74-77, 286-288)."""


def _check_regex(src):
    """regexp.Compile on the native engine; raises ConfigError like UnmarshalYAML."""
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = N.lib().tsg_regex_compile(src.encode("utf-8", "surrogateescape"), C.byref(h), err, 512)
    if rc != N.TSG_OK:
        raise ConfigError("regexp compile error: %s" % err.value.decode("utf-8", "replace"))
    N.lib().tsg_regex_free(h)
    return src


@dataclass
class AllowRule:
    ID: str = ""
    Description: str = ""
    Regex: Optional[str] = None
    Path: Optional[str] = None


@dataclass
class ExcludeBlock:
    Description: str = ""
    Regexes: List[str] = field(default_factory=list)


@dataclass
class Rule:
    ID: str = ""
    Category: str = ""
    Title: str = ""
    Severity: str = ""
    Regex: Optional[str] = None
    Keywords: List[str] = field(default_factory=list)
    Path: Optional[str] = None
    AllowRules: List[AllowRule] = field(default_factory=list)
    ExcludeBlock: ExcludeBlock = field(default_factory=ExcludeBlock)
    SecretGroupName: str = ""


@dataclass
class Config:
    EnableBuiltinRuleIDs: List[str] = field(default_factory=list)
    DisableRuleIDs: List[str] = field(default_factory=list)
    DisableAllowRuleIDs: List[str] = field(default_factory=list)
    CustomRules: List[Rule] = field(default_factory=list)
    CustomAllowRules: List[AllowRule] = field(default_factory=list)
    ExcludeBlock: ExcludeBlock = field(default_factory=ExcludeBlock)


@dataclass
class ScanArgs:
    FilePath: str
    Content: bytes


def _s(v):
    return "" if v is None else str(v)


def _rx(v):
    return None if v is None else _check_regex(str(v))


def _allow(lst):
    return [AllowRule(_s(a.get("id")), _s(a.get("description")), _rx(a.get("regex")),
                      _rx(a.get("path"))) for a in (lst or [])]


def _exclude(d):
    d = d or {}
    return ExcludeBlock(_s(d.get("description")), [_rx(x) for x in (d.get("regexes") or [])])


def config_from_dict(doc):
    if not isinstance(doc, dict):
        raise ConfigError("secrets config decode error")
    c = Config()
    c.EnableBuiltinRuleIDs = [str(x) for x in (doc.get("enable-builtin-rules") or [])]
    c.DisableRuleIDs = [str(x) for x in (doc.get("disable-rules") or [])]
    c.DisableAllowRuleIDs = [str(x) for x in (doc.get("disable-allow-rules") or [])]
    for r in doc.get("rules") or []:
        c.CustomRules.append(Rule(
            ID=_s(r.get("id")), Category=_s(r.get("category")), Title=_s(r.get("title")),
            Severity=_s(r.get("severity")), Regex=_rx(r.get("regex")),
            Keywords=[str(k) for k in (r.get("keywords") or [])], Path=_rx(r.get("path")),
            AllowRules=_allow(r.get("allow-rules")), ExcludeBlock=_exclude(r.get("exclude-block")),
            SecretGroupName=_s(r.get("secret-group-name"))))
    c.CustomAllowRules = _allow(doc.get("allow-rules"))
    c.ExcludeBlock = _exclude(doc.get("exclude-block"))
    return c


def ParseConfig(config_path):
    """scanner.go:267-291: "" or a missing file -> None (builtins only)."""
    if not config_path:
        return None
    if not os.path.exists(config_path):
        return None
    with open(config_path, "rb") as f:
        doc = yaml.safe_load(f)
    if doc is None:
        raise ConfigError("secrets config decode error: EOF")
    return config_from_dict(doc)


_BUILTINS = None


def builtin_rules():
    """The 83 builtin rules and 12 builtin allow rules (builtin-rules.go, builtin-allow-rules.go)."""
    global _BUILTINS
    if _BUILTINS is None:
        d = json.load(open(_RULES_JSON))
        rules = [Rule(ID=r["id"], Category=r["category"], Title=r["title"],
                      Severity=r["severity"], Regex=r["regex"], Keywords=list(r["keywords"]),
                      SecretGroupName=r["secret_group_name"]) for r in d["rules"]]
        allow = [AllowRule(a["id"], a["description"], a["regex"], a["path"])
                 for a in d["allow_rules"]]
        _BUILTINS = (rules, allow)
    return _BUILTINS


def NewScanner(config=None):
    """scanner.go:293-329"""
    b_rules, b_allow = builtin_rules()
    if config is None:
        return Scanner(list(b_rules), list(b_allow), ExcludeBlock())
    enabled = list(b_rules)
    if config.EnableBuiltinRuleIDs:
        enabled = [r for r in b_rules if r.ID in config.EnableBuiltinRuleIDs]
    enabled = enabled + list(config.CustomRules)
    rules = [r for r in enabled if r.ID not in config.DisableRuleIDs]
    allow = [a for a in list(b_allow) + list(config.CustomAllowRules)
             if a.ID not in config.DisableAllowRuleIDs]
    return Scanner(rules, allow, config.ExcludeBlock)


def _b(s):
    return None if s is None else s.encode("utf-8", "surrogateescape")


class _Keep:
    """Keeps ctypes buffers alive for the duration of a native call."""

    def __init__(self):
        self.refs = []

    def cstr(self, s):
        b = _b(s)
        self.refs.append(b)
        return b

    def arr(self, ctype, items):
        a = (ctype * max(1, len(items)))(*items)
        self.refs.append(a)
        return a


class Batch:
    """Files packed for the engine: one contiguous byte stream + u64 offsets (+ paths)."""

    def __init__(self, data, offsets, paths, path_offsets):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.paths = np.ascontiguousarray(paths, dtype=np.uint8)
        self.path_offsets = np.ascontiguousarray(path_offsets, dtype=np.uint64)
        self.nfiles = len(self.offsets) - 1

    @classmethod
    def from_args(cls, args):
        lens = np.array([len(a.Content) for a in args], dtype=np.uint64)
        offs = np.zeros(len(args) + 1, dtype=np.uint64)
        np.cumsum(lens, out=offs[1:])
        data = np.frombuffer(b"".join(a.Content for a in args) or b"\0", dtype=np.uint8)
        pb = [a.FilePath.encode("utf-8", "surrogateescape") for a in args]
        plens = np.array([len(p) for p in pb], dtype=np.uint64)
        poffs = np.zeros(len(args) + 1, dtype=np.uint64)
        np.cumsum(plens, out=poffs[1:])
        paths = np.frombuffer(b"".join(pb) or b"\0", dtype=np.uint8)
        return cls(data, offs, paths, poffs)

    def ptrs(self):
        u64p = C.POINTER(C.c_uint64)
        return (C.c_void_p(self.data.ctypes.data), self.offsets.ctypes.data_as(u64p),
                C.c_uint32(self.nfiles), C.c_void_p(self.paths.ctypes.data),
                self.path_offsets.ctypes.data_as(u64p))

    def path(self, i):
        return bytes(self.paths[int(self.path_offsets[i]):int(self.path_offsets[i + 1])]).decode(
            "utf-8", "surrogateescape")


DEFAULT_EXT_CAP, DEFAULT_CAND_CAPACITY = 1 << 16, 1 << 22  # tsg_ctx_options' defaults
# K2 record forms (include/trivy_secret.h, tsg_emulate_candidates)
CAND_WHOLE, CAND_TRANS, CAND_WORD = 0xFFFFFFFF, 0x80000000, 0x40000000


class Scanner:
    """secret.Scanner{Global}: compiled once, shared read-only (thread-safe natively)."""

    def __init__(self, rules, allow_rules, exclude_block):
        self.Rules = list(rules)
        self.AllowRules = list(allow_rules)
        self.ExcludeBlock = exclude_block
        self._h = None
        self._compile()

    def _compile(self):
        L = N.lib()
        keep = _Keep()
        descs = []
        for r in self.Rules:
            kws = keep.arr(C.c_char_p, [keep.cstr(k) for k in r.Keywords])
            ars = keep.arr(N.AllowRuleDesc, [N.AllowRuleDesc(keep.cstr(a.ID),
                                                              keep.cstr(a.Description),
                                                              keep.cstr(a.Regex), keep.cstr(a.Path))
                                              for a in r.AllowRules])
            exc = keep.arr(C.c_char_p, [keep.cstr(x) for x in r.ExcludeBlock.Regexes])
            descs.append(N.RuleDesc(keep.cstr(r.ID), keep.cstr(r.Category), keep.cstr(r.Title),
                                    keep.cstr(r.Severity), keep.cstr(r.Regex), kws,
                                    len(r.Keywords), keep.cstr(r.Path), ars, len(r.AllowRules),
                                    exc, len(r.ExcludeBlock.Regexes),
                                    keep.cstr(r.SecretGroupName)))
        rd = keep.arr(N.RuleDesc, descs)
        ad = keep.arr(N.AllowRuleDesc, [N.AllowRuleDesc(keep.cstr(a.ID), keep.cstr(a.Description),
                                                        keep.cstr(a.Regex), keep.cstr(a.Path))
                                        for a in self.AllowRules])
        ex = keep.arr(C.c_char_p, [keep.cstr(x) for x in self.ExcludeBlock.Regexes])
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        rc = L.tsg_ruleset_compile(rd, len(descs), ad, len(self.AllowRules), ex,
                                   len(self.ExcludeBlock.Regexes), C.byref(h), err, 1024)
        if rc == N.TSG_ERR_CONFIG:
            raise ConfigError(err.value.decode("utf-8", "replace"))
        N.check(rc)
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            N.lib().tsg_ruleset_destroy(self._h)
            self._h = None

    @property
    def handle(self):
        return self._h

    def info(self):
        i = N.RulesetInfo()
        N.check(N.lib().tsg_ruleset_get_info(self._h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in N.RulesetInfo._fields_}

    def plan_digest(self):
        """Test hook (tsg_ruleset_plan_digest): a 64-bit hash of every member of the compiled
        plan; two plans with the same digest are the same plan."""
        d = C.c_uint64()
        N.check(N.lib().tsg_ruleset_plan_digest(self._h, C.byref(d)))
        return d.value

    def k1_reference(self, batch, chunk):
        """K1 semantics on the CPU (same layout as GpuContext.k1_output)."""
        import numpy as np
        W = (self.info()["n_keywords"] + 31) // 32
        kw = np.zeros(batch.nfiles * W, dtype=np.uint32)
        ev = np.zeros((int(batch.offsets[-1]) + chunk - 1) // chunk, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        N.check(N.lib().tsg_emulate_k1(self.handle, C.c_void_p(batch.data.ctypes.data),
                                       batch.offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       batch.nfiles, chunk, kw.ctypes.data_as(u32p), kw.size,
                                       ev.ctypes.data_as(u32p), ev.size))
        return kw.reshape(batch.nfiles, W), ev

    def emulate_items(self, batch, chunk, max_back=16):
        """The item set K2 scans (tsg_emulate_items): sorted (group, file, chunk) triples
        [n, 3] and the items per group.  max_back 16 is the device's every-chunk rule,
        0xFFFFFFFF the emulation's."""
        G = self.info()["n_groups"]
        counts = np.zeros(max(G, 1), dtype=np.uint64)
        n = C.c_uint64()
        u64p = C.POINTER(C.c_uint64)
        args = (self.handle, C.c_void_p(batch.data.ctypes.data), batch.offsets.ctypes.data_as(u64p),
                batch.nfiles, chunk, max_back)
        N.check(N.lib().tsg_emulate_items(*args, None, 0, counts.ctypes.data_as(u64p), C.byref(n)))
        tri = np.zeros((max(n.value, 1), 3), dtype=np.uint32)
        N.check(N.lib().tsg_emulate_items(*args, tri.ctypes.data_as(C.POINTER(C.c_uint32)), n.value,
                                          None, None))
        return tri[:n.value], counts[:G]

    def emulate_candidates(self, batch, chunk, ext_cap=DEFAULT_EXT_CAP, items_cap=None, max_dense=16,
                           word_recs=True):
        """What K2 should write for the batch (tsg_emulate_candidates): raw records [n, 3]
        {file, rule, end} in the device's form, no capacity applied.  items_cap None is the
        default capacity of the batch's chunk count."""
        if items_cap is None:
            items_cap = default_items_cap((int(batch.offsets[-1]) + chunk - 1) // chunk)
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        args = (self.handle, C.c_void_p(batch.data.ctypes.data), batch.offsets.ctypes.data_as(u64p),
                batch.nfiles, chunk, int(ext_cap), int(items_cap), int(max_dense), 1 if word_recs else 0)
        n = C.c_uint64()
        N.check(N.lib().tsg_emulate_candidates(*args, None, 0, C.byref(n)))
        rec = np.zeros((max(n.value, 1), 3), dtype=np.uint32)
        N.check(N.lib().tsg_emulate_candidates(*args, rec.ctypes.data_as(u32p), n.value, None))
        return rec[:n.value]

    def emulate_item_candidates(self, batch, chunk, ext_cap=DEFAULT_EXT_CAP):
        """(file, rule, end) triples [n, 3] of the emulation's per-item form
        (tsg_emulate_item_candidates), in item order."""
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        args = (self.handle, C.c_void_p(batch.data.ctypes.data), batch.offsets.ctypes.data_as(u64p),
                batch.nfiles, chunk, int(ext_cap))
        n = C.c_uint64()
        N.check(N.lib().tsg_emulate_item_candidates(*args, None, 0, C.byref(n)))
        tri = np.zeros((max(n.value, 1), 3), dtype=np.uint32)
        N.check(N.lib().tsg_emulate_item_candidates(*args, tri.ctypes.data_as(u32p), n.value, None))
        return tri[:n.value]

    def expand_candidates(self, batch, records):
        """K2 records -> (file, rule, end) triples [n, 3] as the resolver expands them
        (tsg_expand_candidates), in record order, CAND_WHOLE ends kept."""
        rec = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, 3)
        u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
        args = (self.handle, C.c_void_p(batch.data.ctypes.data), batch.offsets.ctypes.data_as(u64p),
                batch.nfiles, rec.ctypes.data_as(u32p), len(rec))
        n = C.c_uint64()
        N.check(N.lib().tsg_expand_candidates(*args, None, 0, C.byref(n)))
        tri = np.zeros((max(n.value, 1), 3), dtype=np.uint32)
        N.check(N.lib().tsg_expand_candidates(*args, tri.ctypes.data_as(u32p), n.value, None))
        return tri[:n.value]

    def candidate_stats(self, batch, chunk):
        """tsg_emulate_candidate_stats: (candidate ends per rule, K2 item bytes per group)."""
        per_rule = np.zeros(max(len(self.Rules), 1), dtype=np.uint64)
        per_group = np.zeros(max(self.info()["n_groups"], 1), dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        N.check(N.lib().tsg_emulate_candidate_stats(
            self.handle, C.c_void_p(batch.data.ctypes.data), batch.offsets.ctypes.data_as(u64p),
            batch.nfiles, chunk, per_rule.ctypes.data_as(u64p), per_group.ctypes.data_as(u64p)))
        return per_rule[:len(self.Rules)], per_group[:self.info()["n_groups"]]

    def rule_group(self, rule):
        """Plan introspection: the K2 group of rule index `rule` (-1: host only)."""
        g, relax, ml = C.c_int32(), C.c_int32(), C.c_int64()
        N.check(N.lib().tsg_ruleset_rule_plan(self.handle, rule, C.byref(g), C.byref(relax), C.byref(ml)))
        return g.value

    def rule_plan(self, rule):
        """Plan introspection (tsg_ruleset_rule_plan): the rule's K2 group (-1: host only),
        relaxation (-1: exact) and longest match in bytes (-1: unbounded)."""
        g, relax, ml = C.c_int32(), C.c_int32(), C.c_int64()
        N.check(N.lib().tsg_ruleset_rule_plan(self.handle, rule, C.byref(g), C.byref(relax), C.byref(ml)))
        return {"group": g.value, "relax": relax.value, "maxlen": ml.value}

    def rule_program(self, rule):
        """Plan introspection (tsg_ruleset_rule_program): the rule's GPU program: first_atom
        (> 0: a suffix program), rule_atoms (>= 0: a prefix-cut program), the resolver's
        rule_winback and whether it has a reverse DFA (rule_rev)."""
        fa, at, wb, rev = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        N.check(N.lib().tsg_ruleset_rule_program(self.handle, rule, C.byref(fa), C.byref(at), C.byref(wb),
                                                 C.byref(rev)))
        return {"first_atom": fa.value, "rule_atoms": at.value, "rule_winback": wb.value,
                "rule_rev": bool(rev.value)}

    def group_table(self, group):
        """Test hook (tsg_ruleset_group_table): K2 group `group`'s rules in local order (a
        rule's position is its bit in the group's accept masks) and the accept layout of its
        device table, as the upload decides it: per_state True (accepts per state, staged in
        LDS) or False (look-ahead: accepts per transition)."""
        n, ps = C.c_uint32(), C.c_int32()
        rules = (C.c_uint32 * 64)()
        N.check(N.lib().tsg_ruleset_group_table(self.handle, group, C.byref(n), C.byref(ps), rules, 64))
        return {"rules": list(rules[:n.value]), "per_state": bool(ps.value)}

    def k1_literals(self):
        """K1's literals as (bytes, event bits); ids below n_keywords are keywords."""
        out = []
        buf = C.create_string_buffer(1 << 16)
        n, ev = C.c_uint32(), C.c_uint32()
        while N.lib().tsg_ruleset_k1_literal(self._h, len(out), buf, len(buf), C.byref(n), C.byref(ev)) == 0:
            out.append((buf.raw[:n.value], ev.value))
        return out

    def k1f_emulate(self, batch, chunk, quiet=(), sample_kib=0):
        """K1F's algorithm on the CPU (k1f.hpp): (keyword bits, chunk events, stats); with
        sample_kib the filter is priced on the batch's first sample_kib KiB."""
        import numpy as np
        W = (self.info()["n_keywords"] + 31) // 32
        kw = np.zeros(batch.nfiles * W, dtype=np.uint32)
        ev = np.zeros((int(batch.offsets[-1]) + chunk - 1) // chunk, dtype=np.uint32)
        q = np.array(list(quiet) or [0], dtype=np.uint32)
        st = np.zeros(4, dtype=np.uint64)
        u32p = C.POINTER(C.c_uint32)
        N.check(N.lib().tsg_emulate_k1f(self.handle, C.c_void_p(batch.data.ctypes.data),
                                        batch.offsets.ctypes.data_as(C.POINTER(C.c_uint64)),
                                        batch.nfiles, chunk, q.ctypes.data_as(u32p), len(quiet),
                                        sample_kib, kw.ctypes.data_as(u32p), kw.size, ev.ctypes.data_as(u32p),
                                        ev.size, st.ctypes.data_as(C.POINTER(C.c_uint64))))
        return kw.reshape(batch.nfiles, W), ev, {"groups": int(st[0]), "arrivals": int(st[1]),
                                                 "records": int(st[2])}

    def AllowPath(self, path):
        b = _b(path)
        rc = N.lib().tsg_ruleset_allow_path(self._h, b, len(b))
        if rc < 0:
            N.check(rc)
        return rc == 1

    def Scan(self, args):
        """scanner.go:341-416 on the exact CPU path."""
        p = _b(args.FilePath)
        out = C.c_void_p()
        N.check(N.lib().tsg_scan_cpu(self._h, p, len(p), bytes(args.Content), len(args.Content),
                                     C.byref(out)))
        return self.decode(out, [args.FilePath])[0]

    def ScanBatch(self, args, device=None, ctx=None, emulate_chunk=0, nthreads=0):
        """Scan many files.  device=int -> MI355X kernels; emulate_chunk>0 -> the kernels'
        algorithm emulated on the CPU (tests); otherwise the exact CPU batch path."""
        batch = args if isinstance(args, Batch) else Batch.from_args(args)
        paths = [batch.path(i) for i in range(batch.nfiles)]
        out = C.c_void_p()
        L = N.lib()
        if device is not None or ctx is not None:
            own = ctx is None
            if own:
                ctx = GpuContext(self, device)
            try:
                N.check(L.tsg_scan_batch(ctx.handle, *batch.ptrs(), C.byref(out)))
            finally:
                if own:
                    ctx.close()
        elif emulate_chunk:
            N.check(L.tsg_scan_batch_emulated(self._h, *batch.ptrs(), emulate_chunk, C.byref(out)))
        else:
            N.check(L.tsg_scan_cpu_batch(self._h, *batch.ptrs(), nthreads, C.byref(out)))
        return self.decode(out, paths)

    def decode(self, out, paths):
        L = N.lib()
        n = C.c_size_t()
        ptr = L.tsg_result_data(out, C.byref(n))
        buf = C.string_at(ptr, n.value)
        L.tsg_result_free(out)
        return decode_results(buf, paths, self.Rules)


GROUP_NONE, GROUP_LIST, GROUP_DENSE, GROUP_SKIP = 0, 1, 2, 3
ENTRY_ITEMS, ENTRY_CHUNKS = 512, 1024  # a K2 list entry's items, a dense entry's chunks
# The kernels' block shapes (kernels.hip), for the tests that count a capped grid's rounds
# (knob grid_cap): threads of the 256-thread kernels (kBlock; a wave per unit: four units per
# block), chunks a compaction thread tests (kEvPer), k1x_kernel's lanes per block and 16-B
# words per lane and round (kK1XBlock, kXWords), the largest K1X verify image staged in LDS
# (kXImgLds), outputs_kernel's fixed grid
BLOCK_THREADS, EV_PER, K1X_BLOCK, K1X_WORDS, K1X_IMG_LDS, OUT_BLOCKS = 256, 32, 1024, 4, 128 << 10, 128


def default_items_cap(nchunks):
    """K2's item capacity for a batch of nchunks chunks without the k2_items_cap knob."""
    return max(2 * nchunks, 1 << 16)


def layout_reference(counts, nchunks, items_cap, max_dense=16):
    """tsg_layout_reference: (kind per group, totals) of the device's item layout."""
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    kind = np.zeros(max(len(counts), 1), dtype=np.uint8)
    tot = np.zeros(4, dtype=np.uint64)
    u64p = C.POINTER(C.c_uint64)
    N.check(N.lib().tsg_layout_reference(counts.ctypes.data_as(u64p), len(counts), int(nchunks),
                                         int(items_cap), int(max_dense),
                                         kind.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         tot.ctypes.data_as(u64p)))
    return kind[:len(counts)], {"items": int(tot[0]), "entries": int(tot[1]),
                                "dense_entries": int(tot[2]), "skipped": int(tot[3])}


K1_LAYOUT_OF_KEYS = tuple(k for k, _ in N.K1Layout._fields_ if k not in ("kw_words", "k1_filter", "reserved"))


def k1_layout_of(states, classes):
    """tsg_test_k1_layout_of: the layout the automaton K1 gives a keyword automaton of
    `states` x `classes` (Scanner.info()'s kw_states and kw_classes), as a dict of
    tsg_k1_layout's fields.  Raises NativeError where no device tables can be made of it."""
    v = N.K1Layout()
    N.check(N.lib().tsg_test_k1_layout_of(int(states), int(classes), C.byref(v)))
    return {k: int(getattr(v, k)) for k in K1_LAYOUT_OF_KEYS}


def decode_results(buf, paths, rules):
    magic, nfiles = struct.unpack_from("<II", buf, 0)
    assert magic == 0x31475354 and nfiles == len(paths)
    pos = 8
    out = []
    for i in range(nfiles):
        status = buf[pos]
        (nf,) = struct.unpack_from("<I", buf, pos + 1)
        pos += 5
        findings = []
        for _ in range(nf):
            ri, sl, el, ml = struct.unpack_from("<IiiI", buf, pos)
            pos += 16
            match = buf[pos:pos + ml]
            pos += ml
            (nl,) = struct.unpack_from("<I", buf, pos)
            pos += 4
            lines = []
            for _ in range(nl):
                num, fl, cl = struct.unpack_from("<iBI", buf, pos)
                pos += 9
                content = buf[pos:pos + cl]
                pos += cl
                lines.append({"Number": num, "Content": content, "IsCause": bool(fl & 1),
                              "Annotation": "", "Truncated": False, "Highlighted": content,
                              "FirstCause": bool(fl & 2), "LastCause": bool(fl & 4)})
            r = rules[ri]
            findings.append({"RuleID": r.ID, "Category": r.Category,
                             "Severity": r.Severity if r.Severity != "" else "UNKNOWN",
                             "Title": r.Title, "StartLine": sl, "EndLine": el,
                             "Code": {"Lines": lines or None}, "Match": match})
        if status == 0:
            out.append({"FilePath": "", "Findings": None})
        elif status == 1:
            out.append({"FilePath": paths[i], "Findings": None})
        else:
            out.append({"FilePath": paths[i], "Findings": findings})
    return out


class GpuContext:
    """One device context (tsg_ctx): rule tables replicated in HBM, two lanes, pinned slots.

    upload() copies a batch into a pinned slot that this object then holds (the library
    keeps no pointer to the caller's buffers); submit() / submit_slot() return the native
    ticket of the submission and collect(ticket) decodes its results with the paths it was
    submitted with (collect() with no ticket takes this object's oldest submission).
    scan_batch() is the one-call, thread-safe Scan of a batch.  emulate=True runs the
    kernels' algorithm on the CPU over the same pipeline (tests without a GPU)."""

    def __init__(self, scanner, device=0, chunk_bytes=0, ext_cap=0, cand_capacity=0,
                 host_threads=0, adapt_mib=0, emulate=False, slot_mib=0, max_slots=0):
        import threading
        self._h = None
        self._owned = True
        self.scanner = scanner
        self.chunk = chunk_bytes or 256
        self.ext_cap = ext_cap or DEFAULT_EXT_CAP                    # (tsg_ctx_options' defaults)
        self.cand_capacity = cand_capacity or DEFAULT_CAND_CAPACITY
        opt = N.CtxOptions(chunk_bytes, ext_cap, cand_capacity, host_threads, adapt_mib,
                           N.TSG_CTX_EMULATE if emulate else 0, slot_mib, max_slots)
        h = C.c_void_p()
        N.check(N.lib().tsg_ctx_create(int(device), scanner.handle, C.byref(opt), C.byref(h)))
        self._h = h
        self._upload = None     # (slot id, Batch) of the last upload
        self._k1 = None
        self._lock = threading.Lock()
        self._fifo = []         # (ticket, paths) of this object's uncollected submissions
        self._paths = {}        # ticket -> paths
        self._tensors = {}      # ticket -> the tensor of a submit_tensor, alive until collect
        self._kept = {}         # ticket -> the kept mask of a submit_spans, until collect
        self._device = int(device)
        self._emulate = bool(emulate)

    @classmethod
    def borrowed(cls, scanner, handle, chunk_bytes=0):
        """A view of a context owned elsewhere (a device of a MultiGpu): same methods, and
        close() leaves the context itself alone."""
        import threading
        self = cls.__new__(cls)
        self._h = handle
        self._owned = False
        self.scanner = scanner
        self.chunk = chunk_bytes or 256
        self.ext_cap = self.cand_capacity = None   # (the owner's options: not known here)
        self._upload = None
        self._k1 = None
        self._lock = threading.Lock()
        self._fifo = []
        self._paths = {}
        self._tensors = {}
        self._kept = {}
        self._device = None     # (the owner knows; submit_tensor then only asks for a GPU tensor)
        self._emulate = False
        return self

    @property
    def handle(self):
        return self._h

    def upload(self, batch):
        """Copy the batch into a pinned slot held by this object (the previous upload's slot
        is given back)."""
        sid = C.c_uint32()
        N.check(N.lib().tsg_batch_upload(self._h, *batch.ptrs(), C.byref(sid)))
        with self._lock:
            prev, self._upload = self._upload, (sid.value, batch)
        if prev is not None:
            N.check(N.lib().tsg_slot_release(self._h, prev[0]))

    def kernels(self):
        """The device part of a scan of the uploaded batch, synchronously (test hook);
        k1_output() then returns its keyword bits and chunk events."""
        sid, b = self._upload
        W = (self.scanner.info()["n_keywords"] + 31) // 32
        kw = np.zeros(b.nfiles * W, dtype=np.uint32)
        ev = np.zeros((int(b.offsets[-1]) + self.chunk - 1) // self.chunk, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        N.check(N.lib().tsg_batch_kernels(self._h, sid, b.nfiles, kw.ctypes.data_as(u32p), kw.size,
                                          ev.ctypes.data_as(u32p), ev.size))
        self._k1 = (kw.reshape(b.nfiles, W), ev)

    def batch_items(self):
        """K2's work lists of the last kernels() call (tsg_batch_items): list entries [n, 4]
        {group, first item, items, kind}, dense entries [n, 4] {group, first chunk, chunks,
        kind}, the item array [n, 2] (file, chunk) and the skip flag of every group."""
        sid, _ = self._upload
        G = self.scanner.info()["n_groups"]
        n = (C.c_uint64 * 3)()
        u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        N.check(N.lib().tsg_batch_items(self._h, sid, None, 0, None, 0, None, 0, None, 0, n))
        ent = np.zeros((max(n[0], 1), 4), dtype=np.uint32)
        dent = np.zeros((max(n[1], 1), 4), dtype=np.uint32)
        items = np.zeros((max(n[2], 1), 2), dtype=np.uint32)
        gskip = np.zeros(max(G, 1), dtype=np.uint8)
        m = (C.c_uint64 * 3)()
        N.check(N.lib().tsg_batch_items(self._h, sid, ent.ctypes.data_as(u32p), n[0],
                                        dent.ctypes.data_as(u32p), n[1], items.ctypes.data_as(u32p), n[2],
                                        gskip.ctypes.data_as(u8p), G, m))
        assert list(m) == list(n)
        return ent[:n[0]], dent[:n[1]], items[:n[2]], gskip[:G]

    def batch_candidates(self):
        """What K2 and the outputs kernel of the last kernels() call handed to the host
        (tsg_batch_candidates): {"count": records K2 reserved, "cand_cap": the capacity,
        "records": [min(count, cand_cap), 3] raw {file, rule, end}, "flags": [nfiles] (1
        overflow, 2 folding runes, 4 row written), "kw": [nfiles, kw_words] the rows of the
        files with flag 4, zero elsewhere}."""
        sid, b = self._upload
        W = (self.scanner.info()["n_keywords"] + 31) // 32
        n = (C.c_uint64 * 4)()
        u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        N.check(N.lib().tsg_batch_candidates(self._h, sid, None, 0, None, 0, None, 0, n))
        assert n[2] == b.nfiles
        rec = np.zeros((max(n[1], 1), 3), dtype=np.uint32)
        flags = np.zeros(max(b.nfiles, 1), dtype=np.uint8)
        kw = np.zeros(max(b.nfiles * W, 1), dtype=np.uint32)
        m = (C.c_uint64 * 4)()
        N.check(N.lib().tsg_batch_candidates(self._h, sid, rec.ctypes.data_as(u32p), n[1],
                                             flags.ctypes.data_as(u8p), b.nfiles,
                                             kw.ctypes.data_as(u32p), b.nfiles * W, m))
        assert list(m) == list(n)
        return {"count": int(n[0]), "cand_cap": int(n[3]), "records": rec[:n[1]],
                "flags": flags[:b.nfiles], "kw": kw[:b.nfiles * W].reshape(b.nfiles, W)}

    def adaptation(self):
        """What the context's K1 adaptation decided (tsg_test_adaptation): {"adapted",
        "k1_filter", "hot_states", "ev_hot", "sample_bytes", "kw_unknown": [n_keywords],
        "gate_open": [n_groups], "event_everywhere": [n_groups], "hits": [n_literals] u32 and
        "quiet": [n_literals] after a K1F adaptation, else None}."""
        info = N.AdaptationInfo()
        u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        N.check(N.lib().tsg_test_adaptation(self._h, C.byref(info), None, 0, None, 0, None, 0, None, 0, None, 0))
        nk, ng, nl = info.n_keywords, info.n_groups, info.n_literals
        kwu = np.zeros(max(nk, 1), dtype=np.uint8)
        gate = np.zeros(max(ng, 1), dtype=np.uint8)
        evw = np.zeros(max(ng, 1), dtype=np.uint8)
        hits = np.zeros(max(nl, 1), dtype=np.uint32)
        quiet = np.zeros(max(nl, 1), dtype=np.uint8)
        N.check(N.lib().tsg_test_adaptation(self._h, C.byref(info), kwu.ctypes.data_as(u8p), nk,
                                            gate.ctypes.data_as(u8p), ng, evw.ctypes.data_as(u8p), ng,
                                            hits.ctypes.data_as(u32p), nl, quiet.ctypes.data_as(u8p), nl))
        assert (info.n_keywords, info.n_groups, info.n_literals) == (nk, ng, nl)
        return {"adapted": int(info.adapted), "k1_filter": int(info.k1_filter),
                "hot_states": int(info.hot_states), "ev_hot": int(info.ev_hot),
                "sample_bytes": int(info.sample_bytes), "kw_unknown": kwu[:nk], "gate_open": gate[:ng],
                "event_everywhere": evw[:ng], "hits": hits[:nl] if nl else None,
                "quiet": quiet[:nl] if nl else None}

    def lane_buffers(self):
        """The HBM buffers of the context's lanes (tsg_test_lane_buffers): ([{name: (bytes,
        allocs)} per lane], the lane the last batch was enqueued on or None).  allocs
        unchanged between two calls: the batches in between ran in the same memory."""
        n = (C.c_uint32 * 3)()
        N.check(N.lib().tsg_test_lane_buffers(self._h, None, 0, n))
        bufs = (N.LaneBuffer * max(n[0] * n[1], 1))()
        m = (C.c_uint32 * 3)()
        N.check(N.lib().tsg_test_lane_buffers(self._h, bufs, n[0] * n[1], m))
        assert list(m) == list(n)
        lanes = [{bufs[k * n[1] + i].name.decode(): (int(bufs[k * n[1] + i].bytes), int(bufs[k * n[1] + i].allocs))
                  for i in range(n[1])} for k in range(n[0])]
        return lanes, (None if n[2] == 0xFFFFFFFF else int(n[2]))

    def k1_layout(self):
        """The layout of the context's automaton K1 (tsg_test_k1_layout): k1_layout_of's record
        read from the device tables, with "kw_words" and "k1_filter" (1: batches under 4 GiB
        run K1F, and the automaton only stands by)."""
        v = N.K1Layout()
        N.check(N.lib().tsg_test_k1_layout(self._h, C.byref(v)))
        return {k: int(getattr(v, k)) for k, _ in N.K1Layout._fields_ if k != "reserved"}

    def k1_output(self, chunk):
        """(keyword bits [nfiles, kw_words], chunk event bits) of the last kernels() call."""
        assert chunk == self.chunk, "the context's chunk is %d" % self.chunk
        return self._k1

    @staticmethod
    def _paths_of(batch):
        if isinstance(batch, Batch):
            return [batch.path(i) for i in range(batch.nfiles)]
        return list(batch)

    def _track(self, ticket, paths_of):
        with self._lock:
            self._fifo.append(ticket)
            self._paths[ticket] = paths_of
        return ticket

    def submit(self):
        """Device part of a scan of the uploaded batch, asynchronously; its host resolution
        follows it in the background.  Returns the ticket."""
        sid, b = self._upload
        t = C.c_uint64()
        N.check(N.lib().tsg_slot_submit(self._h, sid, b.nfiles, C.byref(t)))
        return self._track(t.value, b)

    def submit_slot(self, slot_id, nfiles, paths_of):
        """Submit the first nfiles files of an acquired slot (see acquire_slot); paths_of is
        the Batch or the list of paths they were packed from.  Returns the ticket."""
        if paths_of is None:
            raise ValueError("submit_slot needs the submitted files' paths (a Batch or a list)")
        t = C.c_uint64()
        N.check(N.lib().tsg_slot_submit(self._h, int(slot_id), int(nfiles), C.byref(t)))
        return self._track(t.value, paths_of)

    def acquire_slot(self, data_bytes, nfiles, path_bytes):
        """A pinned slot to fill directly: (id, data, offsets, paths, path_offsets) as
        numpy views of the library's pinned memory."""
        v = N.SlotView()
        N.check(N.lib().tsg_slot_acquire(self._h, int(data_bytes), int(nfiles),
                                         int(path_bytes), C.byref(v)))
        data = np.ctypeslib.as_array((C.c_uint8 * v.data_cap).from_address(v.data))
        offs = np.ctypeslib.as_array(v.offsets, shape=(v.files_cap + 1,))
        paths = np.ctypeslib.as_array((C.c_uint8 * v.paths_cap).from_address(v.paths))
        poffs = np.ctypeslib.as_array(v.path_offsets, shape=(v.files_cap + 1,))
        return v.id, data, offs, paths, poffs

    def release_slot(self, slot_id):
        N.check(N.lib().tsg_slot_release(self._h, int(slot_id)))

    def _take(self, ticket):
        with self._lock:
            if ticket is None:
                if not self._fifo:
                    raise N.NativeError(N.TSG_ERR_ARG, "no submitted batch")
                ticket = self._fifo.pop(0)
            elif ticket in self._paths:
                self._fifo.remove(ticket)
            return ticket, self._paths.pop(ticket, None)

    def collect_raw(self, ticket=None):
        """Results of one submission (default: this object's oldest) as a raw tsg_result
        handle; the caller frees it."""
        ticket, _ = self._take(ticket)
        out = C.c_void_p()
        try:
            N.check(N.lib().tsg_batch_collect(self._h, ticket, C.byref(out)))
        finally:
            self._tensors.pop(ticket, None)
            self._kept.pop(ticket, None)
        return out

    def collect(self, ticket=None):
        ticket, paths = self._take(ticket)
        out = C.c_void_p()
        try:
            N.check(N.lib().tsg_batch_collect(self._h, ticket, C.byref(out)))
        finally:
            self._tensors.pop(ticket, None)  # (a submit_tensor's tensor: the batch is done)
            self._kept.pop(ticket, None)
        return self.scanner.decode(out, self._paths_of(paths))

    def pending(self):
        """Uncollected submissions of the context (every caller)."""
        return N.lib().tsg_batch_pending(self._h)

    def scan(self):
        return self.collect(self.submit())

    def scan_batch(self, batch):
        """tsg_scan_batch: copy, scan and resolve one batch in a slot of its own
        (thread-safe: any number of threads may call it on one context)."""
        out = C.c_void_p()
        N.check(N.lib().tsg_scan_batch(self._h, *batch.ptrs(), C.byref(out)))
        return self.scanner.decode(out, self._paths_of(batch))

    def _check_tensor(self, data):
        """The tensor checks of the device-resident entry points (raise before any native call)."""
        import torch
        if not isinstance(data, torch.Tensor):
            raise TypeError("data must be a torch.Tensor, not %s" % type(data).__name__)
        if data.dtype != torch.uint8:
            raise TypeError("data must be a torch.uint8 tensor, not %s" % data.dtype)
        if data.dim() != 1 or not data.is_contiguous():
            raise ValueError("data must be 1-D and contiguous")
        if self._emulate:
            if data.device.type != "cpu":
                raise ValueError("an emulated context scans host tensors, not %s" % data.device)
        elif data.device.type != "cuda" or (self._device is not None and data.device.index != self._device):
            raise ValueError("data is on %s, the context on device %s" % (data.device, self._device))

    @staticmethod
    def _path_arrays(paths, nfiles):
        paths = list(paths)
        if len(paths) != nfiles:
            raise ValueError("%d paths for %d files" % (len(paths), nfiles))
        pb = [_b(p) for p in paths]
        poffs = np.zeros(len(pb) + 1, dtype=np.uint64)
        np.cumsum(np.array([len(p) for p in pb], dtype=np.uint64), out=poffs[1:])
        blob = np.frombuffer(b"".join(pb) or b"\0", dtype=np.uint8)
        return paths, blob, poffs

    @staticmethod
    def _sync_tensor(data):
        import torch
        if data.device.type == "cuda":
            # the bytes must be written when the library's own streams read them
            torch.cuda.current_stream(data.device).synchronize()

    def _tensor_args(self, data, offsets, paths):
        """Checked arguments of tsg_device_submit for a tensor: raises before any native
        call.  Returns (pointer, offsets, nfiles, path bytes, path offsets, paths)."""
        self._check_tensor(data)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        if offs.ndim != 1 or len(offs) < 1 or int(offs[0]) != 0:
            raise ValueError("offsets must be 1-D and start at 0")
        if (offs[1:] < offs[:-1]).any():
            raise ValueError("offsets must be non-decreasing")
        if int(offs[-1]) > data.numel():
            raise ValueError("offsets cover %d bytes, the tensor holds %d" % (int(offs[-1]), data.numel()))
        paths, blob, poffs = self._path_arrays(paths, len(offs) - 1)
        self._sync_tensor(data)
        u64p = C.POINTER(C.c_uint64)
        return (C.c_void_p(data.data_ptr() if data.numel() else None), offs.ctypes.data_as(u64p),
                C.c_uint32(len(paths)), C.c_void_p(blob.ctypes.data), poffs.ctypes.data_as(u64p)), (offs, blob, poffs), paths

    def _spans_args(self, data, starts, lengths, paths, binary_gate):
        """Checked arguments of tsg_device_spans_submit (raises before any native call):
        (arguments up to `kept`, arrays to keep alive, paths, kept mask)."""
        self._check_tensor(data)

        def u64(a, what):
            a = np.asarray(a)
            if a.ndim != 1:
                raise ValueError("%s must be 1-D" % what)
            if a.size and (a.dtype.kind not in "iu" or (a.dtype.kind == "i" and (a < 0).any())):
                raise ValueError("%s must be non-negative integers" % what)
            return np.ascontiguousarray(a, dtype=np.uint64)
        st, ln = u64(starts, "starts"), u64(lengths, "lengths")
        if len(st) != len(ln):
            raise ValueError("%d starts for %d lengths" % (len(st), len(ln)))
        n = data.numel()
        n64 = np.uint64(n)
        if ((st > n64) | (ln > n64 - np.minimum(st, n64))).any():
            raise ValueError("a span lies outside the tensor's %d bytes" % n)
        paths, blob, poffs = self._path_arrays(paths, len(st))
        self._sync_tensor(data)
        kept = np.zeros(max(len(st), 1), dtype=np.uint8)
        u64p = C.POINTER(C.c_uint64)
        args = (C.c_void_p(data.data_ptr() if n else None), C.c_uint64(n), st.ctypes.data_as(u64p),
                ln.ctypes.data_as(u64p), C.c_uint32(len(st)), C.c_void_p(blob.ctypes.data), poffs.ctypes.data_as(u64p),
                C.c_uint32(N.TSG_SPANS_BINARY_GATE if binary_gate else 0), kept.ctypes.data_as(C.POINTER(C.c_uint8)))
        return args, (st, ln, blob, poffs), paths, kept[:len(st)]

    def submit_tensor(self, data, offsets, paths):
        """tsg_device_submit: scan files that already live in this device's memory.  data is a
        1-D contiguous torch.uint8 tensor on the context's device (a slice with a storage
        offset is fine: any byte alignment), file i = data[offsets[i]:offsets[i + 1]], paths
        the files' names.  The current torch stream is synchronized first; the tensor is kept
        alive, and must stay unchanged, until collect(ticket).  Returns the ticket."""
        args, keep, paths = self._tensor_args(data, offsets, paths)
        t = C.c_uint64()
        N.check(N.lib().tsg_device_submit(self._h, *args, C.byref(t)))
        del keep  # (host arrays: copied by the call)
        with self._lock:
            self._tensors[t.value] = data
        return self._track(t.value, paths)

    def scan_tensor(self, data, offsets, paths):
        """tsg_scan_device: submit_tensor + collect in one thread-safe call; the findings are
        scan_batch's for the same bytes."""
        args, keep, paths = self._tensor_args(data, offsets, paths)
        out = C.c_void_p()
        N.check(N.lib().tsg_scan_device(self._h, *args, C.byref(out)))
        del keep
        return self.scanner.decode(out, paths)

    def submit_spans(self, data, starts, lengths, paths, binary_gate=True):
        """tsg_device_spans_submit: scan files given as spans of one tensor on the context's
        device: file i = data[starts[i]:starts[i] + lengths[i]], in any order, with gaps (a
        layer tar as a GPU decompressor leaves it).  With binary_gate the files
        utils.IsBinary calls binary are dropped on the device.  The tensor is kept alive, and
        must stay unchanged, until collect(ticket), which returns the KEPT files' findings in
        input order.  Returns the ticket; spans_kept(ticket) is the kept mask over the input
        files, final as soon as this returns."""
        args, keep, paths, kept = self._spans_args(data, starts, lengths, paths, binary_gate)
        t = C.c_uint64()
        N.check(N.lib().tsg_device_spans_submit(self._h, *args, C.byref(t)))
        del keep
        kept = kept.astype(bool)
        with self._lock:
            self._tensors[t.value] = data
            self._kept[t.value] = kept
        return self._track(t.value, [p for p, k in zip(paths, kept) if k])

    def spans_kept(self, ticket):
        """The kept mask of a submit_spans that is not collected yet (True = scanned)."""
        with self._lock:
            return self._kept[ticket]

    def scan_spans(self, data, starts, lengths, paths, binary_gate=True):
        """tsg_scan_device_spans: submit_spans + collect in one thread-safe call.  Returns
        (results of the kept files in input order, kept mask over the input files)."""
        args, keep, paths, kept = self._spans_args(data, starts, lengths, paths, binary_gate)
        out = C.c_void_p()
        N.check(N.lib().tsg_scan_device_spans(self._h, *args, C.byref(out)))
        del keep
        kept = kept.astype(bool)
        return self.scanner.decode(out, [p for p, k in zip(paths, kept) if k]), kept

    def device_spans_stats(self):
        """tsg_device_spans_stats of the context's spans batches."""
        s = N.DeviceSpansStats()
        N.check(N.lib().tsg_ctx_get_device_spans_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in N.DeviceSpansStats._fields_}

    def device_layer_stats(self):
        """tsg_device_layer_stats of the context's scan_layer_tensor calls."""
        s = N.DeviceLayerStats()
        N.check(N.lib().tsg_ctx_get_device_layer_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in N.DeviceLayerStats._fields_}

    def tar_marks(self, data):
        """Test hook (tsg_test_device_tar_marks): what tar_mark_kernel, or its emulation,
        says of every whole 512-byte block of the tensor `data` (as scan_layer_tensor takes
        it): (header, zero), two bool arrays of data.numel() // 512 entries."""
        self._check_tensor(data)
        self._sync_tensor(data)
        n = data.numel()
        nblocks = n // 512
        words = (nblocks + 63) // 64
        hdr = np.zeros(words + 1, dtype=np.uint64)
        zero = np.zeros(words + 1, dtype=np.uint64)
        u64p = C.POINTER(C.c_uint64)
        N.check(N.lib().tsg_test_device_tar_marks(self._h, C.c_void_p(data.data_ptr() if n else None), C.c_uint64(n),
                                                  hdr.ctypes.data_as(u64p), zero.ctypes.data_as(u64p),
                                                  C.c_uint64(words)))

        def bits(a):
            return np.unpackbits(a[:words].view(np.uint8), bitorder="little")[:nblocks].astype(bool)
        return bits(hdr), bits(zero)

    def stats(self):
        s = N.Stats()
        N.check(N.lib().tsg_ctx_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in N.Stats._fields_}

    def device_input_stats(self):
        """tsg_device_input_stats of the context's device-resident batches."""
        s = N.DeviceInputStats()
        N.check(N.lib().tsg_ctx_get_device_input_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in N.DeviceInputStats._fields_}

    def device_mirror(self):
        """Test hook (tsg_test_device_mirror): the pinned mirror of the last finished
        device-resident batch as (bytes [total], segments [n, 2] of (offset, length))."""
        n = (C.c_uint64 * 2)()
        N.check(N.lib().tsg_test_device_mirror(self._h, None, 0, None, 0, n))
        data = np.zeros(max(int(n[0]), 1), dtype=np.uint8)
        segs = np.zeros((max(int(n[1]), 1), 2), dtype=np.uint64)
        m = (C.c_uint64 * 2)()
        N.check(N.lib().tsg_test_device_mirror(self._h, C.c_void_p(data.ctypes.data), int(n[0]),
                                               segs.ctypes.data_as(C.POINTER(C.c_uint64)), int(n[1]), m))
        assert list(m) == list(n)
        return data[:int(n[0])], segs[:int(n[1])]

    def close(self):
        if self._h:
            if self._upload is not None:
                N.lib().tsg_slot_release(self._h, self._upload[0])
                self._upload = None
            if self._owned:
                N.lib().tsg_ctx_destroy(self._h)  # (waits for the batches in flight)
                self._tensors.clear()
            self._h = None

    def __del__(self):
        self.close()


class MultiGpu:
    """tsg_multi: one process driving several devices (trivy's per-layer goroutines over a
    node's GPUs, pkg/fanal/artifact/image/image.go:210-234).  scan_batch() shards a batch's
    files LPT by bytes over the devices and returns the results in input order."""

    def __init__(self, scanner, devices, slot_mib=0, host_threads=0, emulate=False, max_slots=0,
                 chunk_bytes=0):
        self._h = None
        self.scanner = scanner
        self.chunk = chunk_bytes or 256
        opt = N.CtxOptions(chunk_bytes, 0, 0, host_threads, 0, N.TSG_CTX_EMULATE if emulate else 0,
                           slot_mib, max_slots)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        N.check(N.lib().tsg_multi_create(devs, len(devices), scanner.handle, C.byref(opt),
                                         C.byref(h)))
        self._h = h
        self.n = len(devices)

    def scan_batch(self, batch):
        out = C.c_void_p()
        N.check(N.lib().tsg_multi_scan_batch(self._h, *batch.ptrs(), C.byref(out)))
        return self.scanner.decode(out, GpuContext._paths_of(batch))

    def context(self, i):
        """The i-th device's context (owned by this object) as a GpuContext view."""
        h = C.c_void_p()
        N.check(N.lib().tsg_multi_ctx(self._h, int(i), C.byref(h)))
        return GpuContext.borrowed(self.scanner, h, self.chunk)

    def stats(self, i):
        s = N.Stats()
        N.check(N.lib().tsg_multi_get_stats(self._h, int(i), C.byref(s)))
        return {k: getattr(s, k) for k, _ in N.Stats._fields_}

    def close(self):
        if self._h:
            N.lib().tsg_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


class ScanQueue:
    """tsg_queue: Scan(ScanArgs) for many concurrent callers sharing one context; their
    files are coalesced into pinned batches (the analyzer's per-file goroutines,
    pkg/fanal/analyzer/analyzer.go:419-443)."""

    def __init__(self, ctx, flush_us=2000):
        self.ctx = ctx
        h = C.c_void_p()
        N.check(N.lib().tsg_queue_create(ctx.handle, int(flush_us), C.byref(h)))
        self._h = h

    def Scan(self, args):
        p = _b(args.FilePath)
        out = C.c_void_p()
        N.check(N.lib().tsg_queue_scan(self._h, p, len(p), bytes(args.Content),
                                       len(args.Content), C.byref(out)))
        return self.ctx.scanner.decode(out, [args.FilePath])[0]

    def flush(self):
        N.check(N.lib().tsg_queue_flush(self._h))

    def close(self):
        if self._h:
            N.lib().tsg_queue_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()
