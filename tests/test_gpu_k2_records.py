"""K2's candidate records, record by record: what k2_kernel, k2_kernel_rich and
k2_dense_kernel wrote and outputs_kernel copied to the host (tsg_batch_candidates: the raw
records, the per-file flags, the sparse keyword rows, the record count) against
tsg_emulate_candidates, on inputs built for the kernels' edges (tests/helpers.py;
tests/test_k2_paths.py proves on the CPU that each input covers its edges and that its
reference stays under the default candidate capacity).  The comparison is of the expanded
(file, rule, end) triples as multisets, so a spurious, lost or doubled record fails here with
its file, chunk, offset in its word, group and rule, even where the resolver's findings would
not move.  Every comparison is exact; then scan() must equal the exact CPU path."""
import pytest

from tests import helpers as H
from tests.gpu_common import k2_exact as _exact, k2_scanner_for as _scanner, run_records as _run
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

KERNELS = ("default", "small tables")


@pytest.fixture
def words(request, knob):
    if not request.param:
        knob("k2_no_word_recs", 1)
    return request.param


WORDS = pytest.mark.parametrize("words", [True, False], indirect=True, ids=["word records", "transition records"])


@WORDS
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("chunk", H.K2_CHUNKS)
def test_word_masks_and_chain_starts(chunk, kernel, words):
    """k2_list_pair's lo / hi word masks and start states (Lane::piece at chunk 48): files
    that start and end inside words, secrets split by file boundaries, accepts at every
    position of a body word and of a tail word, the three start contexts of an item that
    starts mid-file, chunk 0 and the last, partial chunk."""
    sc = _scanner("k2", kernel)
    batch, want = _exact("k2", ("mask", chunk))
    st, nref, ntri = _run(sc, batch, want, chunk, kernel, words)
    assert ntri == len(H.word_mask_batch(chunk)[1])


@WORDS
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ext_cap", [0, 64, 40])
@pytest.mark.parametrize("chunk", H.K2_CHUNKS)
def test_tails(chunk, ext_cap, kernel, words):
    """Lane::tail / tail_ni: ends in the next chunk and behind a whole chunk, fe on the
    chunk's end, inside a tail word and at a state that accepts at end of text, a tail that
    dies on the last byte before the cut (ext_cap 64; 40 cuts at 48), one alive at the cut
    and an immortal state (kCandWhole for every rule of the group, once)."""
    sc = _scanner("k2", kernel)
    batch, want = _exact("k2", ("tail", chunk, ext_cap or S.DEFAULT_EXT_CAP))
    st, nref, ntri = _run(sc, batch, want, chunk, kernel, words, ext_cap=ext_cap)
    assert ntri == len(H.with_group_mates(sc, H.tail_batch(chunk, ext_cap or S.DEFAULT_EXT_CAP)[1]))


@WORDS
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("chunk", H.K2_CHUNKS)
def test_entry_shapes(chunk, kernel, words):
    """A list group of 1, 2, 3, 5, 257, 512 and 513 items: a quad that is not full, lane 0's
    second chain alone, ghost lanes, and the entry boundary -- one record per item, none
    twice."""
    sc = _scanner("k2", kernel)
    for n in H.ENTRY_COUNTS:
        batch, want = _exact("k2", ("entry", chunk, n))
        st, nref, ntri = _run(sc, batch, want, chunk, kernel, words)
        assert nref == ntri == n and st["k2_items"] == n and st["k2_launches"] == -(-n // S.ENTRY_ITEMS)


@WORDS
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("ext_cap,long_tokens", [(0, False), (64, False), (64, True)])
@pytest.mark.parametrize("chunk,total", H.DENSE_SHAPES)
def test_dense_records(chunk, total, ext_cap, long_tokens, kernel, words):
    """k2_dense_kernel (Lane::streams and Lane::piece) beside the list groups of the dense
    batch, at the default ext_cap and at 64; with the long tokens its tails then reach
    kCandWhole in a lane range inside one file and in one shared by files."""
    sc = _scanner("builtin", kernel)
    batch, want = _exact("builtin", ("dense", chunk, total, long_tokens))
    st, nref, ntri = _run(sc, batch, want, chunk, kernel, words, ext_cap=ext_cap)
    assert st["k2_dense_entries"] == 2 * -(-H.nchunks_of(batch, chunk) // S.ENTRY_CHUNKS)


@WORDS
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("rules", ["assert", "group64"])
def test_assertion_contexts_and_a_full_group(rules, kernel, words):
    """The committed batches of tests/cover_common.py at chunk 128: every empty-width assertion
    between every pair of context bytes and on the scan's geometry, files without a match kept
    (four start rows, look-ahead tables, the end-of-text emit), and a group DFA of 64 rules
    (accept-mask bits 32..63).  (Their tables are small: the device's occupancy query picks
    the list kernel under either setting.)"""
    sc = _scanner(rules, kernel)
    batch, want = _exact(rules, ("cover", rules))
    st, nref, _ = _run(sc, batch, want, 128, kernel, words, rich="either")
    print("%s, %s: %d records, k2_rich %d" % (rules, kernel, nref, st["k2_rich"]))
    assert nref > 100 and st["groups_skipped"] == 0


@WORDS
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("chunk,total", H.DENSE_SHAPES)
def test_line_anchored_rule_through_the_dense_kernel(chunk, total, kernel, words):
    """k2_dense_kernel on a look-ahead table: a file of 32-hex-digit lines sends the group of
    (?m)^[a-f0-9]{32}$ through the dense pass (tests/test_k2_paths.py proves that on the CPU),
    where every line start and line end is decided across lane ranges and chunk segments."""
    sc = _scanner("assert", kernel)
    batch, want = _exact("assert", ("hex lines", total))
    st, nref, _ = _run(sc, batch, want, chunk, kernel, words, rich="either")
    assert st["k2_dense_entries"] > 0 and nref >= total // 33


@WORDS
@pytest.mark.parametrize("kernel", KERNELS)
def test_many_groups(kernel, words):
    """Seeded corpora: 128 KiB under 1,000 user rules (many small groups) and the 256 KiB
    corpus under the builtin rules, where words with several accepting transitions make the
    two record forms differ in count."""
    for rules, key in (("user", ("corpus", 128 << 10, 9)), ("builtin", ("corpus", 256 << 10, 7))):
        sc = _scanner(rules, kernel)
        batch, want = _exact(rules, key)
        # (the 1,000-rule set's groups are small: k2_kernel runs for it either way)
        _run(sc, batch, want, 256, kernel, words, rich=0 if rules == "user" else None)


@WORDS
@pytest.mark.parametrize("kernel", KERNELS)
def test_item_pass_inputs_once(kernel, words):
    """The item-pass inputs at chunk 256: the comparison also holds where the work lists were
    already checked."""
    sc = _scanner("builtin", kernel)
    for name in ("small files", "k1 edges", "back windows"):
        batch, want = _exact("builtin", ("items", 256, name))
        _run(sc, batch, want, 256, kernel, words)


@WORDS
@pytest.mark.parametrize("kernel", KERNELS)
def test_overflow_records(kernel, words):
    """cand_capacity below the record count on the 256 KiB corpus: exactly the capacity's
    records come back (outputs_kernel's clamp), all of them the reference's, and exactly the
    files that lost a record, or may have, carry the overflow flag."""
    sc = _scanner("builtin", kernel)
    batch, want = _exact("builtin", ("corpus", 256 << 10, 7))
    st, r0, _ = _run(sc, batch, want, 256, kernel, words)
    assert st["overflow"] == 0 and r0 > 64
    for cap in (r0 - 1, 63, 1):
        st, nref, _ = _run(sc, batch, want, 256, kernel, words, cand_capacity=cap)
        assert st["overflow"] == 1 and nref == r0


def test_skipped_groups_hand_back_every_row(knob):
    """k2_items_cap behind the middle list group of the 256 KiB corpus: the skipped groups
    have no records, the listed ones all of theirs, and outputs_kernel writes every file's
    keyword row (the host resolves the skipped groups' rules over every file)."""
    sc = _scanner("builtin", "default")
    batch, want = _exact("builtin", ("corpus", 256 << 10, 7))
    n = H.nchunks_of(batch, 256)
    _, counts = sc.emulate_items(batch, 256, 16)
    cap = H.middle_items_cap(counts, n)
    knob("k2_items_cap", cap)
    st, nref, _ = _run(sc, batch, want, 256, items_cap=cap)
    full = len(sc.emulate_candidates(batch, 256))
    assert st["groups_skipped"] > 0 and 0 < nref < full


def test_host_only_rule_hands_back_every_row():
    """A rule set with a host-only rule on the tail batch: the records are the reference's and
    every file's keyword row comes back."""
    sc = H.hostonly_scanner()
    batch = H.tail_batch(128, 64)[0]
    _run(sc, batch, sc.ScanBatch(batch, nthreads=16), 128, ext_cap=64, rich=0)
