"""Every kernel output on lanes that earlier batches have used.  The other device tests compare
a batch on a fresh context (or on the lane a context has not used yet); production runs
thousands of batches per context, each in a LaneState whose HBM buffers still hold the lane's
previous batch.  That rests on prep_kernel's zero list (kPad, the tail behind the batch, kw,
ovf, hascand, counts, gcount, cursor, gskip, and for K1F ev_bits and zclaim) and on every other
lane buffer being written before it is read ("Lane buffers across batches").  A
fresh allocation very often reads as zero, and the host resolver re-scans exactly, so neither a
fresh context nor a comparison of findings sees a missing fill.

Here one context runs a sequence (tests/lane_reuse_common.py): a predecessor and its subject on
the same lane, a small filler on the other lane between them, the subject on lane 0 and on
lane 1.  Every subject goes through gpu_common.check_batch: K1 bits and events, entries, dense
entries, items and skip flags, records, flags and rows, and the per-batch stats, all equal to
the CPU references.  GpuContext.lane_buffers() proves that the reuse happened: a step fails
unless it ran on the lane it names and found the named buffers allocated (or grown) as the
sequence claims.  tests/test_lane_reuse.py proves on the CPU that each pair of batches has the
relation it is run for.  Each test prints the lane of every batch and the buffers allocated
for it."""
import numpy as np
import pytest
import torch   # (before the library initialises the GPU: torch finds no device afterwards)

from tests import device_input_common as DI
from tests import grid_rounds_common as R
from tests import gpu_common as GC
from tests import helpers as H
from tests import k1_adapted_common as AC
from tests import lane_reuse_common as LR
from trivy_amd import _native as N

pytestmark = pytest.mark.gpu

LANES = pytest.mark.parametrize("lane", [0, 1])
CHUNK = pytest.mark.parametrize("chunk", LR.CHUNKS)


@pytest.fixture
def sc():
    return LR.scanner()


@pytest.fixture(params=LR.K1S)
def k1(request, knob):
    """K1 as K1F (ev_bits and zclaim are zeroed by prep, events are ORed in) and as the
    automaton (ev_bits is not zeroed: every word is stored)."""
    if request.param == "automaton":
        knob("k1_automaton", 1)
    return request.param


def _named(name, chunk, cap=None):
    return name, LR.ref(name, chunk, cap)


def _k1_ran(L, k1):
    assert L.ctx.stats()["k1_filter"] == (1 if k1 == "k1f" else 0)


# ---------------------------------------------------------------- a. shrink
@LANES
@CHUNK
def test_shrink(sc, k1, chunk, lane):
    """`small files` then `corpus 64k` (fewer files, bytes, chunks, entries, records: every
    buffer is reused, and all of them hold more of the predecessor than the subject writes),
    then `k1 edges` (fewer bytes and chunks, 17 times the files: kw, ovf, hascand and ggate are
    allocated again, data_alloc and ev_bits still hold the first batch)."""
    with LR.Lanes(sc, chunk) as L:
        L.pair(lane, _named("small files", chunk), _named("corpus 64k", chunk), reuse="all")
        L.step(lane, *_named("k1 edges", chunk), grow=LR.PER_FILE, reuse=("data_alloc", "ev_bits", "evlist", "cf"))
        _k1_ran(L, k1)


# ---------------------------------------------------------------- b. the same batch again
@LANES
@CHUNK
def test_same_batch_twice_then_after_an_empty_one(sc, k1, chunk, lane):
    """The same batch twice on one lane and once more after a batch of three empty files, for
    which enqueue_scan launches prep and the outputs kernel only: three identical readbacks,
    equal to the reference; the empty batch itself has no bit, no record and no flag."""
    r = LR.ref("corpus 256k", chunk)
    with LR.Lanes(sc, chunk) as L:
        a, _ = L.step(lane, "corpus 256k", r)
        b, _ = L.step(lane, "corpus 256k again", r, reuse="all")
        e, tot = L.step(lane, "empty", LR.ref("empty", chunk), reuse="all")
        assert not e["kw"].any() and len(e["ev"]) == 0 and e["cand"]["count"] == 0 and not e["cand"]["flags"].any()
        assert tot["items"] == 0 and not e["lists"][3].any() and e["stats"]["event_chunks"] == 0
        c, _ = L.step(lane, "corpus 256k after empty", r, reuse="all")
        LR.same_readback(a, b)
        LR.same_readback(a, c)
        _k1_ran(L, k1)


# ---------------------------------------------------------------- c. stale bytes behind the batch
@pytest.mark.parametrize("upload", sorted(LR.UPLOADS))
@pytest.mark.parametrize("kind", LR.CUT_KINDS)
@CHUNK
def test_stale_bytes_behind_the_batch(sc, k1, chunk, kind, upload):
    """The subject is the predecessor's first N bytes, cut inside a secret (or its keyword, or an
    anchor literal whose event the automaton K1 would take from the word it replays): the
    lane buffer holds the rest right behind the batch.  No record of the rule, no keyword bit
    the subject's own bytes do not give, and no event the bytes behind the batch give: the
    events of the last chunk equal the reference's, and event_chunks, the length of the device's
    own event list, equals the reference's count (an event in a chunk past the last would be
    listed and counted there; the readback itself stops at the last chunk).  Both copies: "uploaded"
    is a slot the library filled (one H2D carries batch, zero tail and offsets: the tail's
    zeroes come from the host), "acquired" a slot the caller filled (two H2Ds, LaneState::meta,
    the tail zeroed by prep_kernel)."""
    rp, rs = LR.cut_refs(chunk, kind)
    up = LR.UPLOADS[upload]
    with LR.Lanes(sc, chunk) as L:
        for lane in (0, 1):
            L.step(lane, "predecessor", rp, upload=up)
            rb, _ = L.step(lane, "cut at %d" % LR.cut_case(chunk, kind)[2], rs, reuse="all", upload=up)
            assert len(LR.rule_records(sc, rs, LR.AWS_RULE)) == 0   # (and the device's equal the reference's)
            tri = sc.expand_candidates(rs.batch, rb["cand"]["records"])
            assert not (tri[:, 1] == H.rule_index(sc, LR.AWS_RULE)).any()
            meta = L.seen[lane]["meta"][1]
            assert (meta >= 1) == (upload == "acquired"), "the %s slot took the other copy (meta allocs %d)" % (upload, meta)
        _k1_ran(L, k1)


# ---------------------------------------------------------------- d. overflow, then fits
@LANES
def test_overflow_then_fits_then_overflow(sc, lane):
    """cand_capacity = 64: `back windows` (29 records) fits, `corpus 256k` (113) overflows --
    exactly 64 records back, the files of the dropped ones flagged -- and `back windows` fits
    again: overflow 0, count 29, no file with flag 1, although the lane's ovf bytes and its
    candidate buffer hold the overflowing batch's.  Both orders in one sequence (the first batch
    has the most files, so the per-file buffers stay where they are)."""
    big, small = LR.ref("corpus 256k", 256), LR.ref("back windows", 256)
    with LR.Lanes(sc, 256, cand_capacity=64) as L:
        a, _ = L.step(lane, "back windows", small)
        b, _ = L.step(lane, "corpus 256k", big, reuse=("cand", "counts") + LR.PER_FILE)
        c, _ = L.step(lane, "back windows again", small, reuse="all")
        assert b["stats"]["overflow"] == 1 and b["cand"]["count"] == 113 and len(b["cand"]["records"]) == 64
        assert (b["cand"]["flags"] & 1).any()
        for fits in (a, c):
            assert fits["stats"]["overflow"] == 0 and fits["cand"]["count"] == 29 == len(fits["cand"]["records"])
            assert not (fits["cand"]["flags"] & 1).any()
        LR.same_readback(a, c)


# ---------------------------------------------------------------- e. skipped groups, then none
@LANES
def test_skipped_groups_then_none_then_skipped(sc, knob, lane):
    """`small files` without the knob skips no group: gskip all zero, sparse rows.  `corpus
    256k` under knob k2_items_cap at its middle list group skips groups and gets every row
    back.  `small files` again: gskip all zero, groups_skipped 0 and sparse rows, on the lane
    whose gskip, hascand and kw hold the skipping batch's; between them a batch of three empty
    files, for which no kernel but prep touches gskip.  Both orders in one sequence."""
    cap = LR.middle_cap("corpus 256k", 256)
    skip, none = LR.ref("corpus 256k", 256, cap), LR.ref("small files", 256)
    with LR.Lanes(sc, 256) as L:
        a, ta = L.step(lane, "small files", none)
        knob("k2_items_cap", cap)
        b, tb = L.step(lane, "corpus 256k, k2_items_cap %d" % cap, skip, items_cap=cap, reuse="all")
        N.knob("k2_items_cap", None)
        # (the emit pass writes every group's skip flag when it runs; a batch without work
        # leaves gskip to prep's zero fill alone)
        e, te = L.step(lane, "empty", LR.ref("empty", 256), reuse="all")
        assert te["skipped"] == 0 and e["stats"]["groups_skipped"] == 0 and not e["lists"][3].any()
        assert not e["cand"]["flags"].any()
        c, tc = L.step(lane, "small files again", none, reuse="all")
        assert tb["skipped"] > 0 and b["stats"]["groups_skipped"] == tb["skipped"] and b["lists"][3].any()
        assert (b["cand"]["flags"] & 4).all()
        for rb, tot in ((a, ta), (c, tc)):
            assert tot["skipped"] == 0 and rb["stats"]["groups_skipped"] == 0 and not rb["lists"][3].any()
            assert not (rb["cand"]["flags"] & 4).all() and (rb["cand"]["flags"] & 4).any()
        LR.same_readback(a, c)


# ---------------------------------------------------------------- f. dense, then list
@LANES
def test_dense_then_list_then_dense(sc, lane):
    """The dense batch (4 dense entries, 6,008 records), `corpus 64k` (none), the dense batch
    again: dentries and the dense entry counter after the other kind of batch, in both orders."""
    dense, lists = LR.ref("dense", 256), LR.ref("corpus 64k", 256)
    with LR.Lanes(sc, 256) as L:
        a, _ = L.step(lane, "dense", dense)
        b, _ = L.step(lane, "corpus 64k", lists, reuse="all")
        c, _ = L.step(lane, "dense again", dense, reuse="all")
        assert [x["stats"]["k2_dense_entries"] for x in (a, b, c)] == [4, 0, 4]
        assert [len(x["lists"][1]) for x in (a, b, c)] == [4, 0, 4]
        LR.same_readback(a, c)


# ---------------------------------------------------------------- g. K1X
@LANES
def test_k1x_lists_after_an_overflowing_batch(lane):
    """The 1,000-rule scanner: after the 2 MiB batch whose hit words overflow the blocks' list
    slices (k1x_inline > 0), a batch of the smallest total of the grid-round tests: its xlist
    slices and xcount come from a smaller grid.  Bits and events == k1_reference."""
    sc, big = R.k1x_overflow_case()
    small = R.k1x_batch(min(R.k1x_totals(1)))
    assert int(small.offsets[-1]) < int(big.offsets[-1]) // 4
    with LR.Lanes(sc, 256) as L:
        st = L.run(lane, "k1x overflow", lambda c: GC.k1_on(sc, c, big)[2])
        assert st["k1x_inline"] > 0 and st["k1x_records"] > 0
        st = L.run(lane, "k1x small", lambda c: GC.k1_on(sc, c, small)[2], reuse=("xlist", "xcount", "ev_bits", "kw"))
        assert st["k1x_records"] > 0 and st["bytes"] == int(small.offsets[-1])
        assert "filler" in L.log[-2]


# ---------------------------------------------------------------- h. the adapted context
@pytest.mark.parametrize("chunk", [256])
def test_adapted_context_reuses_lane_0(chunk):
    """Adapt on lane 0 (adapt_mib = 1, the adapting batch of tests/helpers.py), a filler on lane
    1, then `corpus 256k` on lane 0 in the adapting batch's buffers: K1's bits and events and the
    adapted comparison of the item lists and K2's records, as tests/test_gpu_k1_adapted.py runs
    them on the adapting batch itself."""
    sc = AC.scanner()
    big = AC.case(False)[0]
    subj = LR.batch("corpus 256k")
    tri, counts, cand_ref, want = AC.item_refs(sc, subj, chunk)
    with LR.Lanes(sc, chunk, adapt_mib=1) as L:
        def adapt(c):
            c.upload(big)
            c.kernels()
            return c.adaptation()
        a = L.run(0, "adapting batch", adapt)
        assert a["adapted"] == 1 and a["hot_states"] > 0
        AC.check_bits(sc, L.ctx, big, chunk, a, scanned=True)

        def subject(c):
            AC.check_bits(sc, c, subj, chunk, a)
            AC.check_lists_and_records(sc, subj, chunk, a, c.stats(), c.k1_output(chunk)[0], c.batch_items(),
                                       c.batch_candidates(), tri, counts, cand_ref, dense_full=False)
        L.run(0, "corpus 256k", subject, reuse="all")
        assert "filler" in L.log[-2]
        assert L.ctx.scan() == want
        b = L.ctx.adaptation()
        assert b["hot_states"] == a["hot_states"] and np.array_equal(b["kw_unknown"], a["kw_unknown"])


# ---------------------------------------------------------------- i. production paths in between
def _tensor(b):
    return torch.from_numpy(np.array(b.data[:int(b.offsets[-1])])).to("cuda:0")


def _paths(b):
    return [b.path(i) for i in range(b.nfiles)]


def _by_scan(r):
    def fn(c):
        c.upload(r.batch)
        assert c.scan() == r.exact
    return fn


def _by_tensor(r):
    def fn(c):
        assert c.scan_tensor(_tensor(r.batch), r.batch.offsets, _paths(r.batch)) == r.exact
    return fn


def _by_spans(r):
    def fn(c):
        b = r.batch
        got, kept = c.scan_spans(_tensor(b), b.offsets[:-1], np.diff(b.offsets.astype(np.int64)), _paths(b),
                                 binary_gate=False)
        assert kept.all() and got == r.exact
    return fn


@LANES
@pytest.mark.parametrize("path", ["scan", "scan_tensor", "scan_spans"])
def test_subject_after_a_production_batch(sc, lane, path):
    """The predecessor (`small files`) goes through submit / resolve / collect, through
    tsg_scan_device (stage_kernel) or through tsg_scan_device_spans (gather_kernel) on the
    subject's lane; the subject (`corpus 64k`) is then compared at kernel level."""
    pred = LR.ref("small files", 256)
    by = {"scan": _by_scan, "scan_tensor": _by_tensor, "scan_spans": _by_spans}[path]
    with LR.Lanes(sc, 256) as L:
        L.run(lane, "small files by %s" % path, by(pred))
        L.step(lane, *_named("corpus 64k", 256), reuse="all")
        assert "filler" in L.log[-2]


# (the cut through the anchor literal under the automaton K1: the one kernel that lets a byte
# behind the batch into an output, k1_accept's event bits of the word it replays)
CUT_K1 = [("word+15", "k1f"), ("chunk end", "k1f"), ("keyword", "k1f"), ("anchor", "automaton")]


@LANES
@pytest.mark.parametrize("kind,k1", CUT_K1)
def test_device_resident_subject_after_a_host_batch(sc, knob, lane, kind, k1):
    """The converse: the cut-secret subject of (c) comes from device memory (stage_kernel writes
    the lane buffer, prep the tail) after its predecessor came from the host.  No hook reads the
    lane of this path back, so the integers that would show a superset are compared: candidates
    == the reference's records, event_chunks == the reference's chunks with an event (the
    subject's last chunk has none of its own in the anchor cut, tests/test_lane_reuse.py), k2_items
    == the layout's items; and the findings, and the mirror: exactly the files the reference's
    output flags are fetched."""
    knob("device_poison", 1)
    if k1 == "automaton":
        knob("k1_automaton", 1)
    rp, rs = LR.cut_refs(256, kind)
    with LR.Lanes(sc, 256) as L:
        L.step(lane, "predecessor", rp)
        L.run(lane, "cut subject by scan_tensor", _by_tensor(rs),
              reuse=("data_alloc", "ev_bits", "evlist", "cf", "items", "entries", "cand") + LR.PER_FILE)
        assert "filler" in L.log[-2]
        st = L.ctx.stats()
        assert st["k1_filter"] == (1 if k1 == "k1f" else 0)
        assert st["candidates"] == len(rs.records) and st["event_chunks"] == rs.event_chunks
        assert st["k2_items"] == rs.layout[1]["items"] and st["groups_skipped"] == 0 and st["overflow"] == 0
        full = DI.check_mirror(L.ctx, rs.batch, L.ctx.device_input_stats())
        out = H.reference_output(sc, rs.batch, 256, rs.records)
        assert full == np.flatnonzero(out["flags"] & 4).tolist()


# ---------------------------------------------------------------- j. under the knob grid_cap
@pytest.fixture(params=R.CAPS, ids=["cap1", "cap3"])
def cap(request, knob):
    knob("grid_cap", request.param)
    return request.param


@LANES
@CHUNK
def test_shrink_capped(sc, cap, chunk, lane):
    """(a) with every device-sized grid at 1 and 3 blocks: prep_kernel's fills stride."""
    with LR.Lanes(sc, chunk) as L:
        L.pair(lane, _named("small files", chunk), _named("corpus 64k", chunk), reuse="all")


@pytest.mark.parametrize("upload", sorted(LR.UPLOADS))
@pytest.mark.parametrize("kind,k1", [("word+1", "k1f"), ("chunk end+1", "k1f"), ("keyword", "k1f"), ("anchor", "automaton")])
def test_stale_bytes_capped(sc, cap, knob, kind, k1, upload):
    """(c) under the cap, at chunk 256, on both lanes: prep's tail fill strides."""
    if k1 == "automaton":
        knob("k1_automaton", 1)
    rp, rs = LR.cut_refs(256, kind)
    with LR.Lanes(sc, 256) as L:
        for lane in (0, 1):
            L.step(lane, "predecessor", rp, upload=LR.UPLOADS[upload])
            L.step(lane, "cut", rs, reuse="all", upload=LR.UPLOADS[upload])
        _k1_ran(L, k1)
