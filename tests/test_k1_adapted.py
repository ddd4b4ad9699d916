"""The inputs of the adapted-K1 device tests (tests/test_gpu_k1_adapted.py), checked on the
CPU: hottest_over_budget restated in Python (helpers.predict_quiet) over plain occurrence
counts of the batch silences the literals the batch makes hot, keeps the folding rune, leaves
most literals exact and does not depend on the sort's order among equals; the batch holds the
findings the device tests look for; and the adaptation hook answers on an emulated context."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from trivy_amd import secret as S


@functools.lru_cache(maxsize=None)
def _scanner():
    return S.NewScanner(None)


@functools.lru_cache(maxsize=None)
def _case(fold_hot):
    sc = _scanner()
    batch, picks = H.adapted_batch(sc, fold_hot=fold_hot)
    return batch, picks, H.literal_counts(sc, batch)


@pytest.mark.parametrize("fold_hot", [True, False])
def test_predicted_hot_set(fold_hot):
    sc = _scanner()
    batch, picks, counts = _case(fold_hot)
    lits = sc.k1_literals()
    nkw = sc.info()["n_keywords"]
    fb0 = nkw - 3
    total = int(batch.offsets[-1])
    assert (1 << 20) <= total < (16 << 20)          # adapts at adapt_mib = 1, the whole batch is the sample
    a, b, c, d = (picks[k] for k in "abcd")
    assert a < fb0 and lits[a][1] == 0              # only a keyword
    assert b >= nkw and lits[b][1] != 0             # an anchor literal with an event class
    assert fb0 <= c < nkw
    assert d is not None and d < fb0 and lits[d][1] != 0   # (the builtin rules have one)
    budget = total // 4096
    hot = [a, b, d] + ([c] if fold_hot else [])
    assert all(counts[i] > 4 * budget for i in hot), [int(counts[i]) for i in hot]
    quiet, tied = H.predict_quiet(counts, total, set(range(fb0, nkw)))
    assert {a, b, d} <= quiet
    assert c not in quiet and not any(fb0 <= i < nkw for i in quiet)
    assert len(lits) - len(quiet) >= 3 * len(lits) / 4, len(quiet)
    assert not tied
    if not fold_hot:  # nothing but the planted literals (and what they hold) is over the budget
        assert quiet == {a, b, d}


@pytest.mark.parametrize("fold_hot", [True, False])
def test_batch_holds_the_findings(fold_hot):
    """A finding of a rule behind (a) in a file whose only keyword is (a), and a finding of a
    rule behind (b); without the hot folding rune also findings of rules whose groups the
    adaptation does not touch."""
    sc = _scanner()
    batch, picks, counts = _case(fold_hot)
    nkw = sc.info()["n_keywords"]
    found_a, found_b, groups = H.adapted_findings(sc, batch, picks, sc.ScanBatch(batch, nthreads=16))
    assert found_a and found_b
    quiet, _ = H.predict_quiet(counts, int(batch.offsets[-1]), set(range(nkw - 3, nkw)))
    kwu = [1 if k in quiet else 0 for k in range(nkw)]
    ev_hot = 0
    for i in quiet:
        ev_hot |= sc.k1_literals()[i][1]
    gate0, evw0 = H.gates_after_adaptation(sc, [0] * nkw, 0)
    gate, evw = H.gates_after_adaptation(sc, kwu, ev_hot)
    touched = {g for g in range(len(gate)) if gate[g] != gate0[g] or evw[g] != evw0[g]}
    assert groups & touched
    # an open gate with events everywhere (d's event class holds a group it is a keyword of)
    assert any(gate[g] and evw[g] and not gate0[g] for g in range(len(gate)))
    if not fold_hot:
        assert len(groups - touched) >= 20, sorted(groups - touched)


def test_hook_on_an_emulated_context():
    sc = _scanner()
    ctx = S.GpuContext(sc, 0, emulate=True, adapt_mib=1)
    batch, _, _ = _case(True)
    ctx.upload(batch)
    ctx.scan()
    a = ctx.adaptation()
    ctx.close()
    info = sc.info()
    assert a["adapted"] == 0 and a["k1_filter"] == 0 and a["hot_states"] == 0 and a["ev_hot"] == 0
    assert a["sample_bytes"] == 0
    assert a["kw_unknown"].shape == (info["n_keywords"],) and not a["kw_unknown"].any()
    gate0, evw0 = H.gates_after_adaptation(sc, [0] * info["n_keywords"], 0)
    assert np.array_equal(a["gate_open"], gate0) and np.array_equal(a["event_everywhere"], evw0)
    assert a["hits"] is None and a["quiet"] is None
