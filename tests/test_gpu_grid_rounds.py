"""Every device-sized grid at 1 and 3 blocks (knob grid_cap): the kernel-level comparisons of
the other device tests -- bits and events, work lists, candidate records, flags and rows,
marks, gate flags and poisoned mirrors -- on batches small enough for a test and large enough
that every block of the capped grid runs its loop several times, with a partial last round
(tests/test_grid_rounds.py proves that from the references alone, input by input).  Uncapped,
a test batch gives each of these loops one round at most: the state a block carries from
round to round (k1x_kernel's pipelined loads, ev_compact_block's LDS counters behind their
barrier, the item passes' per-block counts, k2_run's staged DFA, the strides of prep, stage,
gather, fetch, gate, marks and outputs) runs only here and in the benchmark.

Nothing in a reference changes: the cap changes how the device computes, never what.  Every
comparison is exact and is the one of the file it comes from (tests/gpu_common.py and the
device-input harnesses), run through the same code."""
import functools
import tarfile

import numpy as np
import pytest

from tests import device_spans_common as XS
from tests import grid_rounds_common as R
from tests import helpers as H
from tests import test_gpu as T
from tests import test_gpu_configs as TC
from tests import test_gpu_device_input as DI
from tests import test_gpu_device_layer as DL
from tests import test_gpu_device_spans as DS
from tests import test_gpu_k2_records as TR
from tests.device_input_common import big_file_batch
from tests.gpu_common import (check_stats, dense_case, item_case, k1_vs_reference, k2_exact, k2_scanner_for,
                              run_lists, run_records)
from trivy_amd import _native as N
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

NEVER = 0xFFFFFFFF
KERNELS = TR.KERNELS


@pytest.fixture(scope="module")
def builtin():
    return S.NewScanner(None)


@pytest.fixture(params=R.CAPS, ids=["cap1", "cap3"])
def cap(request, knob):
    knob("grid_cap", request.param)
    return request.param


@pytest.fixture
def poisoned(knob):
    knob("device_poison", 1)


@pytest.fixture
def ctx(builtin):
    c = S.GpuContext(builtin, 0, adapt_mib=NEVER)
    yield c
    c.close()


# ---------------------------------------------------------------- K1X
@functools.lru_cache(maxsize=None)
def _user_scanner(step):
    """The 1,000-rule scanner compiled with K1X window step `step`."""
    N.knob("x_step", step)
    try:
        return S.NewScanner(S.config_from_dict(R.user_doc()))
    finally:
        N.knob("x_step", None)


# (index into k1x_totals, x_step): every step at the first and the last total
K1X_CASES = [(0, "1"), (0, "2"), (0, "4"), (3, "1"), (3, "2"), (3, "4"), (1, "4"), (2, "1")]


@pytest.mark.parametrize("which,step", K1X_CASES)
def test_k1x_rounds(cap, which, step):
    """k1x_kernel's software-pipelined loop (four words per lane per round, the next round's
    loads issued while this one is hashed) over batches that end exactly on its third round,
    one byte into a fourth, on the third round's first word per lane, and mid-word inside its
    third word: K1 + K1X keyword bits and events == k1_reference at chunks 16 and 256.

    Which k1x_verify_kernel ran is asserted from tsg_stats.k1x_img_bytes.  Measured on the
    device for the 1,000-rule set (979 hashed literals): x_step 1: 62,976 bytes, x_step 2:
    99,584 bytes, both staged in LDS (<= 131,072: k1x_verify_kernel<true>); x_step 4: 167,328
    bytes, read from global memory (k1x_verify_kernel<false>)."""
    sc = _user_scanner(step)
    total = R.k1x_totals(cap)[which]
    st = k1_vs_reference(sc, R.k1x_batch(total), chunks=(16, 256))
    assert st["k1x_records"] > 0 and st["bytes"] == total
    print("x_step %s: k1x_img_bytes %d" % (step, st["k1x_img_bytes"]))
    if step == "1":
        assert 0 < st["k1x_img_bytes"] <= S.K1X_IMG_LDS
    if step == "4":
        assert st["k1x_img_bytes"] > S.K1X_IMG_LDS


def test_k1x_every_alignment_capped(cap, knob):
    TC.test_k1x_every_alignment("2", knob)


def test_k1x_list_overflow_inline_verify_capped(cap):
    """At a grid of one the single slice is the whole list (total / 256 + 65,536 records) and
    the batch's 131,072 hit words still overflow it (k1x_inline > 0 and k1x_records > 0)."""
    TC.test_k1x_list_overflow_inline_verify()


# ---------------------------------------------------------------- compaction and item passes
@functools.lru_cache(maxsize=None)
def _rounds_case():
    sc = k2_scanner_for("builtin", "default")
    b, chunk = R.rounds_corpus(), R.ROUNDS_CHUNK
    tri, counts = sc.emulate_items(b, chunk, 16)
    return b, tri, counts, H.nchunks_of(b, chunk), sc.ScanBatch(b, nthreads=16)


def _lists_vs_reference(sc, case, chunk):
    batch, tri, counts, n, want = case
    lists, st, got, _ = run_lists(sc, batch, chunk)
    kind, tot = H.check_work_lists(lists, tri, counts, n, S.default_items_cap(n))
    check_stats(st, tot)
    assert tot["skipped"] == 0 and got == want
    return st, tot


@pytest.mark.parametrize("listing", ["gates", "k1f_list"])
def test_compaction_and_item_rounds(builtin, cap, knob, listing):
    """65,555 chunks of 16 bytes: ev_compact_block's outer loop (nine rounds of the one block;
    three per block at three, block 2's last one of 19 chunks) with s_wave / s_base reused
    behind the trailing barrier, and both item passes over nev + F units in many rounds with
    s_count accumulating: the work lists == emulate_items / layout_reference, scan() == exact."""
    if listing == "k1f_list":
        knob("k1f_list", 1)
    st, tot = _lists_vs_reference(builtin, _rounds_case(), R.ROUNDS_CHUNK)
    assert st["event_chunks"] == R.event_chunks(builtin, R.rounds_corpus(), R.ROUNDS_CHUNK)


@pytest.mark.parametrize("listing", ["gates", "k1f_list"])
@pytest.mark.parametrize("chunk", [16, 256])
def test_item_inputs_capped(builtin, cap, knob, chunk, listing):
    if listing == "k1f_list":
        knob("k1f_list", 1)
    for name in ("small files", "k1 edges", "back windows"):
        _lists_vs_reference(builtin, item_case(chunk, name), chunk)


@functools.lru_cache(maxsize=None)
def _user_items_case():
    sc = k2_scanner_for("user", "default")
    b, chunk = R.user_items_batch(), R.ROUNDS_CHUNK
    tri, counts = sc.emulate_items(b, chunk, 16)
    return b, tri, counts, H.nchunks_of(b, chunk), sc.ScanBatch(b, nthreads=16)


def test_layout_of_hundreds_of_groups(cap):
    """965 groups, 220 of them listed: one block (or each of three) lays out the entries of
    many list groups (g % gridDim.x) in the emit pass."""
    st, tot = _lists_vs_reference(k2_scanner_for("user", "default"), _user_items_case(), R.ROUNDS_CHUNK)
    assert tot["entries"] >= 200


def test_dense_layout_capped(builtin, cap):
    chunk, total = H.DENSE_SHAPES[0]
    batch, plants, tri, counts, n, want = dense_case(chunk, total)
    st, tot = _lists_vs_reference(builtin, (batch, tri, counts, n, want), chunk)
    assert st["k2_dense_entries"] == 2 * -(-n // S.ENTRY_CHUNKS) == tot["dense_entries"]


# ---------------------------------------------------------------- K2
@pytest.mark.parametrize("kernel", KERNELS)
def test_k2_records_capped(cap, kernel):
    """k2_run's persistent claim loop with one block (the entries in list order: a restage at
    every change of group, the staged tables reused over a group's run of entries) and with
    three: the candidate records == emulate_candidates, record by record, for the rounds
    corpus, the many-groups corpora, a list group of three entries and the dense batch."""
    sc = k2_scanner_for("builtin", kernel)
    b, _, _, _, want = _rounds_case()
    st, nref, _ = run_records(sc, b, want, R.ROUNDS_CHUNK, kernel)
    assert st["k2_launches"] > 100 and nref > 1000
    for rules, key in (("user", ("corpus", 128 << 10, 9)), ("builtin", ("corpus", 256 << 10, 7))):
        batch, want = k2_exact(rules, key)
        run_records(k2_scanner_for(rules, kernel), batch, want, 256, kernel, rich=0 if rules == "user" else None)
    chunk, n = R.ENTRY_SHAPE
    batch, want = k2_exact("k2", ("entry", chunk, n))
    st, nref, ntri = run_records(k2_scanner_for("k2", kernel), batch, want, chunk, kernel)
    assert nref == ntri == n and st["k2_items"] == n and st["k2_launches"] == 3
    chunk, total = H.DENSE_SHAPES[0]
    batch, want = k2_exact("builtin", ("dense", chunk, total, False))
    st, _, _ = run_records(sc, batch, want, chunk, kernel)
    assert st["k2_dense_entries"] == 2 * -(-H.nchunks_of(batch, chunk) // S.ENTRY_CHUNKS)


def test_assertion_contexts_capped(cap):
    """The "assert" batch of tests/cover_common.py (look-ahead tables, every start row, the
    end-of-text emit) with the entries claimed by one block and by three."""
    batch, want = k2_exact("assert", ("cover", "assert"))
    st, nref, _ = run_records(k2_scanner_for("assert", "default"), batch, want, 256, rich="either")
    assert nref > 1000 and st["k2_launches"] > 1 and st["k2_dense_entries"] > 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_k2_overflow_records_capped(cap, kernel):
    sc = k2_scanner_for("builtin", kernel)
    batch, want = k2_exact("builtin", ("corpus", 256 << 10, 7))
    st, nref, _ = run_records(sc, batch, want, 256, kernel, cand_capacity=63)
    assert st["overflow"] == 1 and nref > 63


def test_skipped_groups_hand_back_every_row_capped(cap, knob):
    TR.test_skipped_groups_hand_back_every_row(knob)


def test_host_only_rule_hands_back_every_row_capped(cap):
    TR.test_host_only_rule_hands_back_every_row()


# ---------------------------------------------------------------- outputs_kernel
def test_outputs_rounds(builtin, cap):
    """2,500 files and 3,522 candidate records (42,264 bytes: 2,641 16-B words and a tail of 8
    bytes): copy_range and the per-file loop of outputs_kernel stride, at 256 and 768 threads.
    The records, the flags and the sparse keyword rows == reference_output."""
    b = R.outputs_batch()
    want = builtin.ScanBatch(b, nthreads=16)
    ref = builtin.emulate_candidates(b, 256)
    out = H.reference_output(builtin, b, 256, ref)
    c = S.GpuContext(builtin, 0, chunk_bytes=256, adapt_mib=NEVER)
    try:
        c.upload(b)
        c.kernels()
        dev = c.batch_candidates()
        H.check_candidates(dev, ref, b, builtin, 256)
        assert dev["count"] == out["count"] == len(dev["records"])
        key = lambda r: r[np.lexsort((r[:, 2], r[:, 1], r[:, 0]))]
        assert np.array_equal(key(dev["records"]), key(out["records"]))
        assert np.array_equal(dev["flags"], out["flags"])
        assert np.array_equal(dev["kw"], out["kw"])
        assert c.scan() == want
    finally:
        c.close()


# ---------------------------------------------------------------- K1 automaton and prep
@pytest.mark.parametrize("chunk", [16, 256])
def test_k1_automaton_capped(builtin, cap, knob, chunk):
    T.test_k1_matches_reference(builtin, chunk, "automaton", knob)


def test_lane_buffers_grow_shrink_grow_capped(builtin, cap):
    """The stale bytes of the larger batch are zeroed by a prep_kernel that strides."""
    T.test_lane_buffers_grow_shrink_grow_gpu(builtin)


# ---------------------------------------------------------------- device-resident input
@pytest.mark.parametrize("k", [0, 7])
def test_stage_alignments_capped(builtin, cap, poisoned, k):
    DI.test_equals_scan_batch_at_every_source_alignment(builtin, None, k)


def test_nothing_outside_the_tensor_is_read_capped(builtin, cap, poisoned):
    DI.test_nothing_outside_the_tensor_is_read(builtin, None, 9)


def test_fetch_writes_only_its_segments_capped(builtin, cap, poisoned):
    DI.fetch_writes_only_its_segments(builtin, big_file_batch(48), 10)


def test_gate_edges_capped(ctx, cap, poisoned):
    assert len(XS.gate_layout().contents) >= 40
    DS.test_gate_edges(ctx, None)


@pytest.mark.parametrize("kind", ["shuffled", "big file"])
def test_gather_edges_capped(ctx, cap, poisoned, kind):
    DS.test_gather_edges(ctx, None, kind)
    assert ctx.device_spans_stats()["files_kept"] >= 10


@pytest.mark.parametrize("nblocks", [63, 65, 4097])
def test_marks_block_counts_capped(ctx, cap, nblocks):
    DL.test_marks_block_counts(ctx, nblocks)


def test_marks_alignment_and_guards_capped(ctx, cap):
    DL.test_marks_alignment_and_guards(ctx, 7)


def test_layer_equals_host_call_capped(ctx, cap):
    DL.test_layer_equals_host_call(ctx, tarfile.PAX_FORMAT, True)
