"""The adapted K1 on the device, compared at kernel level.  Every production context adapts
K1 once (adapt_k1f / adapt_k1 on the first batch of adapt_mib MiB): a sampling launch counts
arrivals, the hottest literals leave K1F (the hottest accepting states of the automaton stop
reporting), the tables are rebuilt and rewritten in place, the gates of the groups with an
unknown keyword open and hot anchor events fire in every chunk.  Here that state is read back
(tsg_test_adaptation, tsg_batch_kernels / _items / _candidates) and compared, integer for
integer, with plain restatements on the CPU: the sampling counters with occurrence counts in
Python, the selection with hottest_over_budget restated (helpers.predict_quiet), the rebuilt
tables' bits and events with tsg_emulate_k1f and k1_reference, the opened gates and
everywhere-events with a derivation from the rules, the item lists and K2's records with the
unadapted emulation (equal where the adaptation touched nothing, supersets elsewhere), and the
findings with the exact CPU path.  The inputs come from helpers.adapted_batch;
tests/test_k1_adapted.py checks on the CPU that they meet their conditions.  There are no
tolerances."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import k1_adapted_common as AC
from trivy_amd import configs
from trivy_amd import corpus
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

K1S = ("k1f", "automaton")
FOLD = pytest.mark.parametrize("fold_hot", [True, False], ids=["fold hot", "fold rare"])


_scanner, _case, _big_case, _item_case = AC.scanner, AC.case, AC.big_case, AC.item_case
_adapted_context, _check_bits = AC.adapted_context, AC.check_bits


@FOLD
def test_sampling_counters(fold_hot):
    """k1f_kernel's report() with A.hits: for every literal, the sampling launch's counter
    equals the plain count of the literal's occurrences in the batch -- the batch one byte
    stream, ASCII letters folded, overlapping occurrences counted, ending inside the batch,
    file boundaries ignored (report() counts before its file check; k1f.hpp, k1_reference).
    The sample is the whole batch; the batch's own K1F counters are those of its real launch
    with the rebuilt tables: the arrivals of the literals still in the filter."""
    sc = _scanner()
    batch, picks, counts, _ = _case(fold_hot)
    lits = sc.k1_literals()
    assert sc.k1f_emulate(batch, 256)[2]["records"] == len(lits)   # every literal has a record
    ctx = _adapted_context(sc, batch)
    st, a = ctx.stats(), ctx.adaptation()
    ctx.close()
    assert a["adapted"] == 1 and a["k1_filter"] == 1 and st["k1_filter"] == 1
    assert a["sample_bytes"] == int(batch.offsets[-1])
    bad = np.flatnonzero(a["hits"].astype(np.int64) != counts)
    assert len(bad) == 0, [(int(i), lits[i][0], int(a["hits"][i]), int(counts[i])) for i in bad[:8]]
    stay = a["quiet"] == 0
    assert st["k1f_arrivals"] == int(counts[stay].sum()), (st["k1f_arrivals"], int(counts.sum()))
    assert st["k1f_arrivals"] < int(counts.sum()) and st["k1f_listed"] > 0


@FOLD
def test_selection(fold_hot):
    """hottest_over_budget, the folding-rune exemption and apply_unknown: the literals that
    left the filter are the predicted ones, no folding rune among them; the unknown keywords
    are the quiet literals below n_keywords, ev_hot the OR of the quiet literals' events; and
    the opened gates and everywhere-events are those derived from the rules."""
    sc = _scanner()
    batch, picks, counts, want = _case(fold_hot)
    lits = sc.k1_literals()
    nkw = sc.info()["n_keywords"]
    ctx = _adapted_context(sc, batch)
    st, a = ctx.stats(), ctx.adaptation()
    ctx.close()
    quiet = set(np.flatnonzero(a["quiet"]).tolist())
    assert quiet == want, (sorted(quiet - want), sorted(want - quiet))
    assert {picks["a"], picks["b"], picks["d"]} <= quiet and picks["c"] not in quiet
    assert not a["quiet"][nkw - 3:nkw].any()
    assert np.array_equal(a["kw_unknown"], a["quiet"][:nkw])
    ev_hot = 0
    for i in quiet:
        ev_hot |= lits[i][1]
    assert a["ev_hot"] == ev_hot and ev_hot != 0
    assert a["hot_states"] == len(quiet) == int(a["quiet"].sum()) == st["k1_hot_states"]
    gate, evw = H.gates_after_adaptation(sc, a["kw_unknown"], a["ev_hot"])
    assert np.array_equal(a["gate_open"], gate), np.flatnonzero(a["gate_open"] != gate)
    assert np.array_equal(a["event_everywhere"], evw), np.flatnonzero(a["event_everywhere"] != evw)
    gate0, evw0 = H.gates_after_adaptation(sc, np.zeros(nkw, np.uint8), 0)
    assert (gate != gate0).any() and (evw != evw0).any()


@FOLD
@pytest.mark.parametrize("k1", K1S)
@pytest.mark.parametrize("chunk", [16, 256, 1024])
def test_bits_and_events_after_adaptation(knob, chunk, k1, fold_hot):
    """The rebuilt tables (k1f_build without the quiet literals + upload_k1f; k1_tables with
    the hot states) on the adapting batch itself, then on the K1 edge batch and a folding-rune
    batch, which the same context scans with the tables it keeps."""
    if k1 == "automaton":
        knob("k1_automaton", 1)
    sc = _scanner()
    batch = _case(fold_hot)[0]
    nkw = sc.info()["n_keywords"]
    ctx = _adapted_context(sc, batch, chunk)
    try:
        a = ctx.adaptation()
        assert a["adapted"] == 1 and a["k1_filter"] == (k1 == "k1f") and a["hot_states"] > 0
        assert (a["hits"] is None) == (k1 == "automaton") and (a["quiet"] is None) == (k1 == "automaton")
        assert not a["kw_unknown"][nkw - 3:].any()
        assert 0 < int(a["kw_unknown"].sum()) < nkw / 4
        _check_bits(sc, ctx, batch, chunk, a, scanned=True)
        _check_bits(sc, ctx, corpus.k1_edge_batch(sc.k1_literals(), 7 + chunk % 5), chunk, a)
        _check_bits(sc, ctx, corpus.fold_runes_batch(11, nbytes=512 << 10, plants=300, frac=0.3), chunk, a)
        b = ctx.adaptation()  # one adaptation per context: later batches change nothing
        assert b["hot_states"] == a["hot_states"] and np.array_equal(b["kw_unknown"], a["kw_unknown"])
    finally:
        ctx.close()


@pytest.mark.parametrize("k1", K1S)
def test_batch_larger_than_the_sample(knob, k1):
    """16 MiB + 3 KiB + 5 bytes: the sampling launch stops at its 16 MiB cap, the real launch
    of the same batch covers all of it with the rebuilt tables (the sample's tiles and bytes
    are not the batch's)."""
    if k1 == "automaton":
        knob("k1_automaton", 1)
    sc = _scanner()
    batch = _big_case()
    assert int(batch.offsets[-1]) == H.ADAPT_BIG_TOTAL
    ctx = _adapted_context(sc, batch, 256)
    try:
        a = ctx.adaptation()
        assert a["adapted"] == 1 and a["k1_filter"] == (k1 == "k1f") and a["hot_states"] > 0
        assert not a["kw_unknown"][sc.info()["n_keywords"] - 3:].any()   # folding runes stay exact
        if k1 == "k1f":
            assert a["sample_bytes"] == 16 << 20
        else:  # (a whole number of the automaton's sampled items)
            assert a["sample_bytes"] > 0
        _check_bits(sc, ctx, batch, 256, a, scanned=True)
    finally:
        ctx.close()


@FOLD
@pytest.mark.parametrize("chunk", [16, 256])
def test_gates_items_and_k2_after_adaptation(chunk, fold_hot):
    """gates_kernel, the item passes and K2 with opened gates (galways, d_galw) and
    everywhere-events (kEvAlways, gofbit row 31) on the adapting batch."""
    sc = _scanner()
    batch, picks, _, _ = _case(fold_hot)
    tri, counts, cand_ref, want = _item_case(fold_hot, chunk)
    ctx = _adapted_context(sc, batch, chunk)
    try:
        st, a = ctx.stats(), ctx.adaptation()
        kw_dev, _ = ctx.k1_output(chunk)
        lists = ctx.batch_items()
        dev = ctx.batch_candidates()
        got = ctx.scan()
    finally:
        ctx.close()
    AC.check_lists_and_records(sc, batch, chunk, a, st, kw_dev, lists, dev, tri, counts, cand_ref, mixed=not fold_hot)
    # a file whose only keyword is a quiet one is still resolved
    assert got == want
    found_a, found_b, _ = H.adapted_findings(sc, batch, picks, got)
    assert found_a and found_b


@functools.lru_cache(maxsize=None)
def _user1000():
    doc = configs.user_rules_doc(1000, seed=4)
    sc = S.NewScanner(S.config_from_dict(doc))
    # a K1F-resident keyword made hot, as in adapted_batch: a keyword without events that
    # holds no other literal
    lits = sc.k1_literals()
    fb0 = sc.info()["n_keywords"] - 3
    real = [i for i, (s, _) in enumerate(lits) if s and b"\xff" not in s]
    hot = next(i for i in real if i < fb0 and lits[i][1] == 0 and len(lits[i][0]) >= 5 and
               not any(j != i and lits[j][0] in lits[i][0] for j in real))
    rng = np.random.default_rng(8)
    args = configs.mixed_batch(doc, 2 << 20, seed=67)
    per = -(-H.ADAPT_HOT // len(args))
    args = [S.ScanArgs(x.FilePath, bytes(x.Content) + b"".join(
        b" " + lits[hot][0] + (b"\n" if rng.random() < 0.2 else b"")for _ in range(per))) for x in args]
    batch = S.Batch.from_args(args)
    return sc, batch, hot, sc.ScanBatch(batch, nthreads=16)


def test_large_rule_set_adapts():
    """1,000 user rules: K1F, K1X (the hashed literals) and the adaptation together.  The
    combined bits and events equal k1_reference outside the unknown keywords and hot event
    classes and are subsets inside; the findings are the exact path's."""
    sc, batch, hot, want = _user1000()
    assert sc.info()["k1x_literals"] > 800 and int(batch.offsets[-1]) >= 1 << 20
    ctx = _adapted_context(sc, batch, 256)
    try:
        st, a = ctx.stats(), ctx.adaptation()
        assert a["adapted"] == 1 and a["k1_filter"] == 1 and st["k1x_records"] + st["k1x_inline"] > 0
        assert a["hot_states"] > 0 and a["quiet"][hot] == 1 and a["kw_unknown"][hot] == 1
        assert a["sample_bytes"] == int(batch.offsets[-1])
        _check_bits(sc, ctx, batch, 256, a, scanned=True)
        got = ctx.scan()
    finally:
        ctx.close()
    assert got == want
    assert sum(len(x["Findings"] or []) for x in want) > 10


def test_adaptation_while_the_other_lane_is_busy():
    """A small batch, the adapting batch and another small batch submitted before any is
    collected: the adaptation rewrites the shared tables between the kernels of two lanes.
    Every result, and that of a batch scanned afterwards, is the exact path's."""
    sc = _scanner()
    batch = _case(True)[0]
    small = [corpus.make_corpus(256 << 10, seed=90 + k, plants_per_mib=200)[0] for k in range(3)]
    order = [small[0], batch, small[1]]
    ctx = S.GpuContext(sc, 0, adapt_mib=1)
    try:
        tickets = []
        for b in order:
            ctx.upload(b)
            tickets.append(ctx.submit())
        got = [ctx.collect(t) for t in tickets]
        a = ctx.adaptation()
        ctx.upload(small[2])
        later = ctx.scan()
    finally:
        ctx.close()
    assert a["adapted"] == 1 and a["hot_states"] > 0
    for b, g in zip(order, got):
        assert g == sc.ScanBatch(b, nthreads=16)
    assert later == sc.ScanBatch(small[2], nthreads=16)
