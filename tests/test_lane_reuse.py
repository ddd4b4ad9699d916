"""The CPU twin of tests/test_gpu_lane_reuse.py: from the emulation alone, every sequence meets
the conditions it is run for (a quantity that stops satisfying its condition after a change to
the inputs fails here, without a GPU); each sequence's steps through one emulated context give
the exact path's findings batch by batch; and the harness the device tests run
(gpu_common.check_batch under lane_reuse_common.Lanes) accepts a context built from the
references and rejects one that keeps, as a lane whose prep_kernel skipped a zero fill would,
the previous batch's keyword bits, events, overflow bytes, hascand bytes, skip flags or the
bytes behind the batch."""
import numpy as np
import pytest

from tests import gpu_common as GC
from tests import helpers as H
from tests import lane_reuse_common as LR
from trivy_amd import secret as S


@pytest.fixture(scope="module")
def sc():
    return LR.scanner()


# ---------------------------------------------------------------- a context made of references
class ReferenceContext:
    """What the tests ask of a GpuContext, answered from the references in the device's forms
    (reference_work_lists, reference_output), on two lanes whose buffers are sized like
    LaneState's.  stale: names of per-batch state this context does not clear -- it ORs in what
    the lane's previous batch left there, as the device would without the zero fill ("tail": the
    predecessor's bytes behind the batch, as the automaton K1 would read them)."""

    def __init__(self, sc, chunk=256, cand_capacity=0, stale=(), items_cap=None):
        self.scanner, self.chunk = sc, chunk
        self.ext_cap, self.cand_capacity = S.DEFAULT_EXT_CAP, cand_capacity or S.DEFAULT_CAND_CAPACITY
        self.items_cap = items_cap   # (the knob, which the reference context cannot read)
        self.stale = set(stale)
        self.seq, self.last = 0, None
        self.lanes = [{k: [0, 0] for k in ("data_alloc", "meta", "ev_bits", "kw", "ggate", "ovf", "hascand", "cand")}
                      for _ in range(2)]
        self.left = [None, None]
        self._lock = None

    def upload(self, b):
        self.batch = b

    def _ensure(self, lane, name, n):
        buf = self.lanes[lane][name]
        if buf[0] < n or not buf[1]:
            buf[0], buf[1] = n + n // 8, buf[1] + 1

    def kernels(self):
        b, sc = self.batch, self.scanner
        r = GC.BatchRef(sc, b, self.chunk, items_cap=self.items_cap)
        lane = self.last = self.seq % 2
        self.seq += 1
        F, W = b.nfiles, r.k1[0].shape[1]
        for name, n in (("data_alloc", int(b.offsets[-1]) + 8192), ("ev_bits", 4 * r.n + 16), ("kw", 4 * F * W + 4),
                        ("ggate", 8 * F + 8), ("ovf", F + 1), ("hascand", F + 1), ("cand", 12 * self.cand_capacity)):
            self._ensure(lane, name, n)
        kw, ev = r.k1[0].copy(), r.k1[1].copy()
        tot = r.layout[1]
        out = H.reference_output(sc, b, self.chunk, r.records, self.cand_capacity, skipped=tot["skipped"] > 0)
        lists = list(H.reference_work_lists(r.items[0], r.items[1], r.n, r.items_cap))
        prev = self.left[lane]
        if prev is not None:   # what the previous batch left in the buffers this one does not clear
            f, n = min(F, len(prev["kw"])), min(len(ev), len(prev["ev"]))
            if "kw" in self.stale:
                kw[:f] |= prev["kw"][:f]
                rows = (out["flags"][:f] & 4) != 0
                out["kw"][:f][rows] |= prev["kw"][:f][rows]
            if "ev_bits" in self.stale:
                ev[:n] |= prev["ev"][:n]
            if "ovf" in self.stale:   # outputs_kernel: flag 1 from the overflow byte, and the row with it
                was = (prev["flags"][:f] & 1) != 0
                out["flags"][:f][was] |= 5
                out["kw"][:f][was] = kw[:f][was]
            if "hascand" in self.stale:
                was = (prev["hascand"][:f]) != 0
                out["flags"][:f][was] |= 4
                out["kw"][:f][was] = kw[:f][was]
            if "gskip" in self.stale:
                lists[3] = lists[3] | prev["gskip"]
            total = int(b.offsets[-1])
            if "tail" in self.stale and total % 16 and len(prev["data"]) > total:
                # the automaton K1 replays the batch's last 16-byte word whole and takes the event
                # bits of an arrival behind the last byte (k1_accept): with the predecessor's bytes
                # there instead of zeroes, the events of the word's chunk are those of the batch
                # continued to the word's end
                end = min(-(-total // 16) * 16, len(prev["data"]))
                longer = S.Batch.from_args([S.ScanArgs("t", bytes(b.data[:total]) + bytes(prev["data"][total:end]))])
                ev[(total - 1) // self.chunk] |= sc.k1_reference(longer, self.chunk)[1][(total - 1) // self.chunk]
        self.left[lane] = {"data": b.data[:int(b.offsets[-1])], "kw": r.k1[0], "ev": r.k1[1], "flags": out["flags"].copy(), "gskip": lists[3].copy(),
                           "hascand": np.bincount(r.records[:, 0], minlength=F)[:F] if len(r.records) else np.zeros(F, int)}
        self._k1 = (kw, ev)
        self._lists, self._cand = tuple(lists), out
        self._stats = {"k2_items": tot["items"], "k2_launches": tot["entries"], "k2_dense_entries": tot["dense_entries"],
                       "groups_skipped": tot["skipped"], "candidates": len(r.records),
                       "overflow": int(len(r.records) > self.cand_capacity), "event_chunks": r.event_chunks}

    def k1_output(self, chunk):
        return self._k1

    def stats(self):
        return dict(self._stats)

    def batch_items(self):
        return self._lists

    def batch_candidates(self):
        return self._cand

    def lane_buffers(self):
        return [{k: tuple(v) for k, v in lane.items()} for lane in self.lanes], self.last

    def close(self):
        pass


def _lanes(sc, chunk=256, **kw):
    L = LR.Lanes.__new__(LR.Lanes)
    L.sc, L.ctx, L.seen, L.ran, L.log = sc, ReferenceContext(sc, chunk, **kw), None, [], []
    return L


# ---------------------------------------------------------------- the conditions, from the emulation
@pytest.mark.parametrize("chunk", LR.CHUNKS)
def test_shrink_conditions(chunk):
    """(a) `small files` then `corpus 64k`: strictly fewer files, bytes, chunks, entries and
    records (the items are not fewer at chunk 256, so they are not a condition); then `k1
    edges`: fewer bytes and chunks, many more files."""
    big, small, edges = (LR.shape(LR.ref(n, chunk)) for n in ("small files", "corpus 64k", "k1 edges"))
    print(chunk, big, small, edges)
    for k in ("files", "bytes", "chunks", "entries", "records"):
        assert 0 < small[k] < big[k], k
    assert edges["bytes"] < big["bytes"] and edges["chunks"] < big["chunks"]
    assert edges["files"] > 10 * big["files"]
    # the per-file buffers must grow: an eighth of slack over the predecessor's files is not enough
    assert edges["files"] + 1 > (big["files"] + 1) * 9 // 8 + 16
    for s in (big, small, edges):
        assert s["skipped"] == 0 and s["items"] > 0


def test_issue_table():
    """The batches' measures at chunk 256 (files, bytes, chunks, items, list entries, records; dense
    entries for the dense batch), as the sequences' docstrings quote them."""
    want = {"small files": (114, 1049104, 4099, 3001, 55, 273), "corpus 256k": (23, 262144, 1024, 1002, 55, 113),
            "corpus 64k": (7, 65536, 256, 1367, 50, 105), "k1 edges": (1910, 80434, 315, 81, 20, 0),
            "back windows": (143, 97920, 383, 435, 10, 29)}
    for name, w in want.items():
        s = LR.shape(LR.ref(name, 256))
        assert (s["files"], s["bytes"], s["chunks"], s["items"], s["entries"], s["records"]) == w, (name, s)
    s = LR.shape(LR.ref("dense", 256))
    assert (s["files"], s["bytes"], s["chunks"], s["items"], s["entries"], s["dense_entries"], s["records"]) == (
        67, 262145, 1025, 27, 7, 4, 6008), s


def test_empty_batch_reference(sc):
    """(b) three files of no bytes: no chunk, no bit, no item, no record, no flag."""
    r = LR.ref("empty", 256)
    assert r.n == 0 and r.batch.nfiles == 3 and not r.k1[0].any() and len(r.k1[1]) == 0
    assert LR.shape(r)["items"] == 0 and len(r.records) == 0
    out = H.reference_output(sc, r.batch, 256, r.records)
    assert not out["flags"].any()
    assert len(r.exact) == 3 and all(not x["Findings"] for x in r.exact)


@pytest.mark.parametrize("kind", LR.CUT_KINDS)
@pytest.mark.parametrize("chunk", LR.CHUNKS)
def test_cut_secret_truth(sc, chunk, kind):
    """(c) the exact path finds the secret in the predecessor, in the line at that offset, and
    nothing of that rule in the subject; the reference has a record of the rule for the
    predecessor's file and none for the subject; N falls where the kind says; the keyword is
    whole in the subject (kind "keyword": cut, and its bit is not set)."""
    pred, subj, n, at = LR.cut_case(chunk, kind)
    rp, rs = LR.cut_refs(chunk, kind)
    data = bytes(pred.data[:int(pred.offsets[-1])])
    assert int(subj.offsets[-1]) == n and bytes(subj.data[:n]) == data[:n] and subj.nfiles == 1
    assert int(pred.offsets[1]) < at < int(pred.offsets[2])
    line = data[:at].count(b"\n", int(pred.offsets[1])) + 1
    assert len(rs.k1[1]) == -(-n // chunk) > 3
    head = (0, data[:data.index(b"glpat-")].count(b"\n") + 1)
    if kind == "anchor":
        # the cut goes through the anchor literal `glpat-`: its last byte lies behind the subject, in
        # the subject's last 16-byte word and chunk, where the predecessor has the literal's event
        assert data[at:at + 6] == b"glpat-" and n == at + 2 and (at + 5) // 16 == (n - 1) // 16
        assert LR.findings_of(rp.exact, "gitlab-pat")[:2] == [head, (1, line)]
        assert LR.findings_of(rs.exact, "gitlab-pat") == [head]
        last = (n - 1) // chunk
        assert int(rp.k1[1][last]) & ~int(rs.k1[1][last]), "the stale literal would add no event"
        if chunk == 256:   # ... and the chunk has no event of its own: event_chunks would count it
            assert int(rs.k1[1][last]) & 0x7FFFFFFF == 0
    else:
        assert data[at:at + len(H.AKIA)] == H.AKIA
        assert (1, line) in LR.findings_of(rp.exact, LR.AWS_RULE)
        assert 1 in LR.rule_records(sc, rp, LR.AWS_RULE)[:, 0].tolist()
        assert LR.keyword_bit(sc, rp.k1[0], 1, b"AKIA") == 1
        assert LR.findings_of(rs.exact, "gitlab-pat") == [head]
    assert LR.findings_of(rs.exact, LR.AWS_RULE) == []
    assert len(LR.rule_records(sc, rs, LR.AWS_RULE)) == 0
    if kind == "keyword":
        assert at < n < at + 4 and LR.keyword_bit(sc, rs.k1[0], 0, b"AKIA") == 0
    elif kind != "anchor":
        assert at + 4 < n < at + len(H.AKIA) and LR.keyword_bit(sc, rs.k1[0], 0, b"AKIA") == 1
    want = {"word+0": n % 16 == 0, "word+1": n % 16 == 1, "word+15": n % 16 == 15, "chunk end": n % chunk == 0,
            "chunk end+1": n % chunk == 1, "keyword": True, "anchor": n % 16 == 3}[kind]
    assert want, (kind, n)
    # the subject has work of its own in front of the cut: events, items and another rule's records
    assert rs.event_chunks > 0 and LR.shape(rs)["items"] > 0 and len(rs.records) > 0


def test_overflow_conditions(sc):
    """(d) at a capacity of 64 records `corpus 256k` overflows and `back windows` fits."""
    big, small = LR.ref("corpus 256k", 256), LR.ref("back windows", 256)
    assert len(big.records) == 113 > 64 > len(small.records) == 29 > 0
    out = H.reference_output(sc, big.batch, 256, big.records, cand_cap=64)
    assert (out["flags"] & 1).any() and len(out["records"]) == 64
    assert not (H.reference_output(sc, small.batch, 256, small.records, cand_cap=64)["flags"] & 1).any()
    # files that overflow in the predecessor exist in the subject too (a stale overflow byte shows)
    assert np.flatnonzero(out["flags"] & 1).min() < small.batch.nfiles


def test_skip_conditions(sc):
    """(e) under the middle item capacity `corpus 256k` skips groups and gets every row back;
    without it `small files` skips none and gets sparse rows."""
    cap = LR.middle_cap("corpus 256k", 256)
    skip, none = LR.ref("corpus 256k", 256, cap), LR.ref("small files", 256)
    assert skip.layout[1]["skipped"] > 0 and (skip.layout[0] == S.GROUP_LIST).any()
    assert none.layout[1]["skipped"] == 0
    every = H.reference_output(sc, skip.batch, 256, skip.records, skipped=True)
    sparse = H.reference_output(sc, none.batch, 256, none.records)
    assert (every["flags"] & 4).all() and 0 < ((sparse["flags"] & 4) != 0).sum() < none.batch.nfiles
    # a file without a row in the subject has a row in the predecessor (a stale row flag shows)
    assert ((sparse["flags"][:skip.batch.nfiles] & 4) == 0).any()
    # ... and under the default capacity the predecessor skips nothing either
    assert LR.ref("corpus 256k", 256).layout[1]["skipped"] == 0


def test_dense_conditions():
    """(f) the dense batch has 4 dense entries, `corpus 64k` none."""
    assert LR.shape(LR.ref("dense", 256))["dense_entries"] == 4
    assert LR.shape(LR.ref("corpus 64k", 256))["dense_entries"] == 0
    assert LR.shape(LR.ref("corpus 64k", 256))["entries"] > 0


# ---------------------------------------------------------------- the sequences, emulated
@pytest.mark.parametrize("chunk", LR.CHUNKS)
def test_sequences_emulated(sc, chunk):
    """(a), (b), (c) batch by batch through one emulated context: scan() == the exact path and
    the per-batch stats == the references."""
    R = lambda n: (LR.ref(n, chunk), None)
    LR.emulated_sequence(sc, chunk, [R("small files"), R("filler"), R("corpus 64k"), R("filler"), R("small files"),
                                     R("filler"), R("k1 edges")])
    LR.emulated_sequence(sc, chunk, [R("corpus 256k"), R("filler"), R("corpus 256k"), R("filler"), R("empty"),
                                     R("filler"), R("corpus 256k")])
    for kind in LR.CUT_KINDS:
        rp, rs = LR.cut_refs(chunk, kind)
        LR.emulated_sequence(sc, chunk, [(rp, None), R("filler"), (rs, None)])


def test_sequences_emulated_k2_paths(sc):
    """(d), (e), (f) through one emulated context each."""
    R = lambda n, cap=None: (LR.ref(n, 256, cap), cap)
    for order in ((R("corpus 256k"), R("back windows")), (R("back windows"), R("corpus 256k"))):
        LR.emulated_sequence(sc, 256, [order[0], R("filler"), order[1]], cand_capacity=64)
    cap = LR.middle_cap("corpus 256k", 256)
    LR.emulated_sequence(sc, 256, [R("corpus 256k", cap), R("filler"), R("small files"), R("filler"), R("corpus 256k", cap)])
    LR.emulated_sequence(sc, 256, [R("dense"), R("filler"), R("corpus 64k"), R("filler"), R("dense")])


# ---------------------------------------------------------------- the harness itself
def _shrink(L, chunk):
    for lane in (0, 1):
        L.pair(lane, ("small files", LR.ref("small files", chunk)), ("corpus 64k", LR.ref("corpus 64k", chunk)),
               reuse="all")
        L.step(lane, "k1 edges", LR.ref("k1 edges", chunk), grow=LR.PER_FILE, reuse=("data_alloc", "ev_bits"))


def test_harness_accepts_the_references(sc, capsys):
    """Lanes + check_batch on a context made of the references: every step passes, runs on the
    lane it names, and the log says which buffers were allocated again."""
    L = _lanes(sc, 256)
    _shrink(L, 256)
    assert [l for l in L.log if "k1 edges" in l] == [
        "lane %d batch %d: k1 edges: allocs kw +1, ggate +1, ovf +1, hascand +1" % (lane, 3 + 2 * lane) for lane in (0, 1)]
    assert any("corpus 64k: allocs unchanged" in l for l in L.log)
    assert "lane 1 batch 1: filler" in capsys.readouterr().out


def test_harness_conditions_fail(sc):
    """A step on the wrong lane, a `reuse` of a buffer that grew and a `grow` of one that did not
    fail the sequence."""
    small, big = LR.ref("corpus 64k", 256), LR.ref("small files", 256)
    L = _lanes(sc, 256)
    L.step(0, "small", small)
    with pytest.raises(AssertionError, match="first batch on lane 1"):
        L.step(1, "small", small, reuse="all")
    with pytest.raises(AssertionError, match="allocated again"):
        L.step(0, "big", big, reuse=("data_alloc",))
    with pytest.raises(AssertionError, match="did not grow"):
        L.step(0, "small", small, grow=("kw",))
    L.ctx.seq += 1   # a batch the driver has not seen: the next one runs on the other lane
    with pytest.raises(AssertionError, match="not on lane"):
        L.step(L.next_lane(), "small", small)


STALE = {
    "kw": lambda L: L.pair(0, ("small files", LR.ref("small files", 256)), ("corpus 64k", LR.ref("corpus 64k", 256))),
    "ev_bits": lambda L: L.pair(0, ("small files", LR.ref("small files", 256)), ("corpus 64k", LR.ref("corpus 64k", 256))),
    "ovf": lambda L: L.pair(0, ("corpus 256k", LR.ref("corpus 256k", 256)), ("back windows", LR.ref("back windows", 256))),
    "hascand": lambda L: L.pair(0, ("corpus 256k", LR.ref("corpus 256k", 256)), ("small files", LR.ref("small files", 256))),
}


@pytest.mark.parametrize("what", sorted(STALE))
def test_harness_rejects_stale_lane_state(sc, what):
    """A context that keeps the previous batch's keyword bits, events, overflow bytes or hascand
    bytes on the lane fails the sequence made for it, in the subject's step, and passes it when
    it clears them."""
    kw = {"cand_capacity": 64} if what == "ovf" else {}
    STALE[what](_lanes(sc, 256, **kw))
    L = _lanes(sc, 256, stale=(what,), **kw)
    with pytest.raises(AssertionError):
        STALE[what](L)
    assert L.ran[0] == 1 and "filler" in L.log[-1]   # the predecessor passed; the subject failed


def test_harness_rejects_stale_bytes_behind_the_batch(sc):
    """A context whose lane keeps the predecessor's bytes behind the batch fails the subject cut
    through the anchor literal (the rest of the literal completes it inside the subject's last
    word: an event the subject's own bytes do not give) and passes the one cut through the
    secret, where the bytes behind the batch end no literal."""
    for chunk in LR.CHUNKS:
        for kind, fails in (("anchor", True), ("word+1", False)):
            rp, rs = LR.cut_refs(chunk, kind)
            L = _lanes(sc, chunk)
            L.step(0, "predecessor", rp)
            L.step(0, "cut", rs, reuse="all")
            L = _lanes(sc, chunk, stale=("tail",))
            L.step(0, "predecessor", rp)
            if fails:
                with pytest.raises(AssertionError, match="events differ in chunks"):
                    L.step(0, "cut", rs, reuse="all")
            else:
                L.step(0, "cut", rs, reuse="all")


def test_harness_rejects_stale_skip_flags(sc):
    cap = LR.middle_cap("corpus 256k", 256)
    for stale, ok in (((), True), (("gskip",), False)):
        L = _lanes(sc, 256, stale=stale, items_cap=cap)
        L.step(0, "skipping", LR.ref("corpus 256k", 256, cap), items_cap=cap)
        L.ctx.items_cap = None
        if ok:
            L.step(0, "none skipped", LR.ref("small files", 256))
        else:
            with pytest.raises(AssertionError):
                L.step(0, "none skipped", LR.ref("small files", 256))


def test_same_readback_rejects_a_difference(sc):
    r = LR.ref("corpus 64k", 256)
    c = ReferenceContext(sc, 256)
    a = GC.read_batch(c, r.batch)
    b = GC.read_batch(c, r.batch)
    LR.same_readback(a, b)
    b["cand"] = dict(b["cand"], flags=b["cand"]["flags"] ^ 4)
    with pytest.raises(AssertionError):
        LR.same_readback(a, b)
    b = GC.read_batch(c, r.batch)
    b["lists"][2][0] = b["lists"][2][1]
    with pytest.raises(AssertionError):
        LR.same_readback(a, b)
