"""DESIGN.md 3.5's exactness argument on the device: the batches of
tests/test_candidate_cover.py (committed under tests/golden/candidate_cover/, where the
oracle's matches are stored with the files) through K1 and K2.  gpu_common.run_records
compares the device's records with emulate_candidates, the flags and keyword rows, and scan()
with the exact path; then the cover predicate is computed from the device's own records.

These batches hold what no other device test has: 2-, 3- and 4-byte runes and invalid bytes
inside K2 items, matches thousands of bytes long, and, under group_states 24, relax-0 and
prefix-cut DFAs.  The "assert" batch is the context matrix of every empty-width assertion
(all four start rows, look-ahead and per-state tables, the end-of-text emit, files back to
back); "group64" fills a group DFA's 64 accept bits.  Their files without a match are kept: a
spurious record shows in the record comparison, a spurious finding in scan() == exact."""
import functools

import numpy as np
import pytest

from tests import cover_common as CC
from tests.gpu_common import run_records
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

# scanner -> the committed batch it scans
SETS = {("builtin", None): "builtin", ("builtin", 24): "builtin", "user40": "user40", "foldcut": "foldcut",
        "assert": "assert", ("assert", 24): "assert", "group64": "group64"}


@functools.lru_cache(maxsize=None)
def _exact(name):
    """(scanner, batch with its truth, exact CPU findings), once per rule set."""
    sc, _ = CC.rule_set(name)
    cb = CC.fixture_batch(SETS[name])
    return sc, cb, sc.ScanBatch(cb.batch, nthreads=16)


def _run(name, chunk, ext_cap=0, dev_rec=None):
    sc, cb, want = _exact(name)
    dev = {}
    # (the default builtin plan's 64 KiB groups run k2_kernel_rich; for the smaller tables of
    # the other two plans the device's occupancy query decides)
    st, nref, ntri = run_records(sc, cb.batch, want, chunk, ext_cap=ext_cap,
                                 rich=None if name == ("builtin", None) else "either", dev_out=dev)
    assert st["overflow"] == 0 and dev["count"] == len(dev["records"])
    tri = sc.expand_candidates(cb.batch, dev["records"])
    n = CC.cover(sc, cb, tri, dev["flags"], chunk, ext_cap or S.DEFAULT_EXT_CAP)
    print("%s chunk %d ext_cap %d: %d records, %s, k2_rich %d, items %d, dense entries %d" % (
        name, chunk, ext_cap, nref, n, st["k2_rich"], st["k2_items"], st["k2_dense_entries"]))
    assert n["ends"] >= sum(1 for t in cb.truth if t) > 0   # every kept file has a match
    assert n["bounded_explicit"] * 10 >= n["bounded"] * 9, n
    if dev_rec is not None:
        dev_rec.update(dev)
    return n


@pytest.mark.parametrize("chunk", [16, 256])
@pytest.mark.parametrize("name", list(SETS), ids=CC.set_id)
def test_device_records_cover_every_match(name, chunk):
    _run(name, chunk)


def test_long_matches_end_in_whole_file_records():
    """ext_cap 256: the tails of the long-repetition variants stop at the cut, so their rules
    come back as whole-file records; only matches longer than the cut (or of a rule without
    a length bound) may lean on them."""
    name = ("builtin", None)
    n = _run(name, 256, ext_cap=256)
    assert n["whole"] > 0   # (none at the default ext_cap: tests/test_candidate_cover.py)


def test_assert_batch_through_lane_piece():
    """Chunk 48 (helpers.K2_CHUNKS): no multiple of 128, so the list kernel runs Lane::piece,
    whose start rows and end-of-text path are its own."""
    _run("assert", 48)


def _eot_locals(sc, cb, dev, group):
    """Local indices in `group` of the rules with a plain record (the device expanded an
    accept mask itself: Lane::emit) that ends its file."""
    local = {r: k for k, r in enumerate(sc.group_table(group)["rules"])}
    rec = dev["records"]
    size = np.diff(cb.batch.offsets.astype(np.int64))
    plain = rec[((rec[:, 1] & S.CAND_TRANS) == 0) & (rec[:, 2] != S.CAND_WHOLE)]
    assert (plain[:, 2] == size[plain[:, 0]]).all()   # nothing else writes a plain end
    return {local[int(r)] for r in plain[:, 1] if int(r) in local}


@pytest.mark.parametrize("chunk", [16, 256])
def test_group64_end_of_text_emit_reaches_the_upper_mask_half(chunk):
    """The device's own expansion of an end-of-text accept mask names rules with local index
    0, 31, 32 and 63 of the full group (d.rules[w * 64 + ctz] with ctz >= 32)."""
    sc, cb, _ = _exact("group64")
    dev = {}
    _run("group64", chunk, dev_rec=dev)
    g = next(g for g in range(sc.info()["n_groups"]) if len(sc.group_table(g)["rules"]) == 64)
    assert not sc.group_table(g)["per_state"]
    assert {0, 31, 32, 63} <= _eot_locals(sc, cb, dev, g)


def test_group64_immortal_tail_returns_its_group_whole_once():
    """ext_cap 256 at chunk 16 (at chunk 256 the file lies inside one lane range of its dense
    group and has no tail): the unbounded rule's tail ends in one whole-file record for every
    rule of its group, once.  The planner does not put that rule into the 64-rule group (the states
    of gqzz{.* times 63 literals do not fit: tests/test_candidate_cover.py), so the burst is
    of its own group's seven rules."""
    sc, cb, _ = _exact("group64")
    dev = {}
    n = _run("group64", 16, ext_cap=256, dev_rec=dev)
    assert n["whole"] > 0
    r = [x.ID for x in sc.Rules].index(CC.GROUP64_UNB)
    mates = sc.group_table(sc.rule_group(r))["rules"]
    f = next(f for f, m in enumerate(cb.meta) if m.variant == "unbounded")
    rec = dev["records"]
    whole = rec[(rec[:, 2] == S.CAND_WHOLE)]
    assert sorted(whole[:, 1].tolist()) == sorted(mates) and set(whole[:, 0].tolist()) == {f}
