"""What the device does after K1, compared directly: the work lists the item passes leave
on the lane (tsg_batch_items) against tsg_emulate_items and layout_reference, and K2's
dense, skip, overflow and transition-record paths through the findings of batches built
to reach them (tests/helpers.py; tests/test_k2_paths.py checks on the CPU that each input
covers its edges).  Every comparison is exact; the references are the hooks and the exact
CPU path."""
import numpy as np
import pytest

from tests import helpers as H
from tests.gpu_common import check_stats as _check_stats, dense_case as _dense_case, item_case as _item_case
from tests.gpu_common import run_lists as _run
from trivy_amd import corpus
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def builtin():
    return S.NewScanner(None)


@pytest.mark.parametrize("listing", ["gates", "k1f_list"])
@pytest.mark.parametrize("chunk", H.ITEM_CHUNKS)
def test_item_passes_match_reference(builtin, knob, chunk, listing):
    """gates_kernel / items_count_kernel / items_emit_kernel with layout_block == the
    reference item set and layout, on the tiny/empty-files batch, the K1 edge batch and the
    back-window batch; with the gates pass and with K1F's own event list."""
    if listing == "k1f_list":
        knob("k1f_list", 1)
    for name in ("small files", "k1 edges", "back windows"):
        batch, tri, counts, n, want = _item_case(chunk, name)
        lists, st, got, _ = _run(builtin, batch, chunk)
        kind, tot = H.check_work_lists(lists, tri, counts, n, S.default_items_cap(n))
        _check_stats(st, tot)
        assert tot["skipped"] == 0 and st["k1_filter"] == 1, name
        assert got == want, name


@pytest.mark.parametrize("chunk,total", H.DENSE_SHAPES)
def test_dense_entries(builtin, chunk, total):
    """k2_dense_kernel: two groups want the dense pass (every chunk of their gated files),
    the entries tile [0, nchunks) with a partial last one, and the findings -- true matches
    across lane ranges, entry boundaries, at a file's end before an ungated file and at the
    batch's last byte -- are the exact path's."""
    batch, plants, tri, counts, n, want = _dense_case(chunk, total)
    lists, st, got, _ = _run(builtin, batch, chunk)
    kind, tot = H.check_work_lists(lists, tri, counts, n, S.default_items_cap(n))
    _check_stats(st, tot)
    assert st["k2_dense_entries"] == 2 * -(-n // S.ENTRY_CHUNKS) and tot["skipped"] == 0
    assert got == want
    assert sum(f["RuleID"] == H.AKIA_GROUP_RULE for r in got for f in r["Findings"] or []) == len(plants)


@pytest.mark.parametrize("chunk,total", H.DENSE_SHAPES)
def test_skip_second_dense_group(builtin, knob, chunk, total):
    """k2_max_dense = 1: the second dense-wanting group is skipped (gskip, groups_skipped),
    outputs_kernel hands every keyword row to the host, which resolves the group's rule in
    the files with its keyword and in no other; the other groups' lists are unchanged."""
    batch, plants, tri, counts, n, want = _dense_case(chunk, total)
    knob("k2_max_dense", 1)
    lists, st, got, _ = _run(builtin, batch, chunk)
    kind, tot = H.check_work_lists(lists, tri, counts, n, S.default_items_cap(n), max_dense=1)
    _check_stats(st, tot)
    g = builtin.rule_group([r.ID for r in builtin.Rules].index(H.AKIA_GROUP_RULE))
    assert tot["skipped"] == 1 and kind[g] == S.GROUP_SKIP and lists[3][g] == 1
    assert got == want


@pytest.mark.parametrize("chunk", [16, 256])
def test_skip_over_item_capacity(builtin, knob, chunk):
    """k2_items_cap ending behind the middle list group: the groups up to it are listed as
    before, the later ones skipped (a skipped group keeps its region, so no list group
    behind it fits), and on the dense batch the dense groups behind them still run."""
    cases = [_item_case(chunk, name) for name in ("back windows", "small files")]
    cases += [(b, t, c, n, w) for b, _, t, c, n, w in (_dense_case(*s) for s in H.DENSE_SHAPES if s[0] == chunk)]
    for batch, tri, counts, n, want in cases:
        cap = H.middle_items_cap(counts, n)
        knob("k2_items_cap", cap)
        lists, st, got, _ = _run(builtin, batch, chunk)
        kind, tot = H.check_work_lists(lists, tri, counts, n, cap)
        _check_stats(st, tot)
        assert tot["skipped"] > 0 and (kind == S.GROUP_LIST).any()
        assert got == want


def test_candidate_overflow(builtin):
    """cand_capacity is the capacity the device uses: exactly the batch's records fit; one
    less, 63 and 1 overflow (emit_cand / Lane::put drop the record and flag its file,
    outputs_kernel clamps the copy), and the findings stay the exact path's."""
    batch, _ = corpus.make_corpus(256 << 10, seed=7, plants_per_mib=300)
    want = builtin.ScanBatch(batch, nthreads=16)
    _, _, got, st = _run(builtin, batch, 256)
    r0 = st["candidates"]
    assert got == want and st["overflow"] == 0 and r0 > 64
    for cap, ovf in ((r0, 0), (r0 - 1, 1), (63, 1), (1, 1)):
        _, _, got, st = _run(builtin, batch, 256, cand_capacity=cap)
        assert st["overflow"] == ovf and (st["candidates"] > cap) == bool(ovf), (cap, st["candidates"])
        assert st["candidates"] == r0, (cap, st["candidates"], r0)
        assert got == want, cap


def test_transition_records_and_plain_list_kernel(builtin, knob):
    """k2_no_word_recs (replay_emit's transition records, the form of rule sets with 16,384
    groups and more) and group_table_kib = 32 (smaller DFAs: the occupancy API then picks
    the other list kernel) on the 4 MiB corpus: findings == the exact path."""
    batch, _ = corpus.make_corpus(4 << 20, seed=21 + 64, plants_per_mib=50)
    want = builtin.ScanBatch(batch, nthreads=16)
    _, _, got, st = _run(builtin, batch, 64)
    assert got == want
    knob("k2_no_word_recs", 1)
    _, _, got, st_t = _run(builtin, batch, 64)
    assert got == want
    # a record per accepting transition, not per accepting word: never fewer
    assert st_t["candidates"] >= st["candidates"] and st_t["k2_items"] == st["k2_items"]
    knob("group_table_kib", 32)
    small = S.NewScanner(None)
    want_s = small.ScanBatch(batch, nthreads=16)
    _, _, got, st_s = _run(small, batch, 64)
    assert got == want_s == want
    print("k2_rich: default %d, group_table_kib=32 %d" % (st["k2_rich"], st_s["k2_rich"]))
    assert st_s["k2_rich"] == 0
    assert st["k2_rich"] != st_s["k2_rich"]
