"""DESIGN.md 3.5's exactness argument on the device: the batches of
tests/test_candidate_cover.py (committed under tests/golden/candidate_cover/, where the
oracle's matches are stored with the files) through K1 and K2.  gpu_common.run_records
compares the device's records with emulate_candidates, the flags and keyword rows, and scan()
with the exact path; then the cover predicate is computed from the device's own records.

These batches hold what no other device test has: 2-, 3- and 4-byte runes and invalid bytes
inside K2 items, matches thousands of bytes long, and, under group_states 24, relax-0 and
prefix-cut DFAs."""
import functools

import pytest

from tests import cover_common as CC
from tests.gpu_common import run_records
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

# scanner -> the committed batch it scans
SETS = {("builtin", None): "builtin", ("builtin", 24): "builtin", "user40": "user40", "foldcut": "foldcut"}


@functools.lru_cache(maxsize=None)
def _exact(name):
    """(scanner, batch with its truth, exact CPU findings), once per rule set."""
    sc, _ = CC.rule_set(name)
    cb = CC.fixture_batch(SETS[name])
    return sc, cb, sc.ScanBatch(cb.batch, nthreads=16)


def _run(name, chunk, ext_cap=0):
    sc, cb, want = _exact(name)
    dev = {}
    # (the default builtin plan's 64 KiB groups run k2_kernel_rich; for the smaller tables of
    # the other two plans the device's occupancy query decides)
    st, nref, ntri = run_records(sc, cb.batch, want, chunk, ext_cap=ext_cap,
                                 rich=None if name == ("builtin", None) else "either", dev_out=dev)
    assert st["overflow"] == 0 and dev["count"] == len(dev["records"])
    tri = sc.expand_candidates(cb.batch, dev["records"])
    n = CC.cover(sc, cb, tri, dev["flags"], chunk, ext_cap or S.DEFAULT_EXT_CAP)
    print("%s chunk %d ext_cap %d: %d records, %s" % (name, chunk, ext_cap, nref, n))
    assert n["ends"] >= sum(1 for t in cb.truth if t) > 0   # every kept file has a match
    assert n["bounded_explicit"] * 10 >= n["bounded"] * 9, n
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
