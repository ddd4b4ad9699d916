"""The automaton K1 (k1_kernel) in its legacy LDS layout, and with wide keyword rows.

k1_kernel runs whenever K1F does not (k1f_build declines the rule set, the batch reaches 4 GiB,
or the knob k1_automaton), and has two inner loops.  The builtin rules' automaton (515 x 43) is
packed, and so is everything the other device tests put on the automaton.  A table over 64 KiB
runs the legacy loop: class words with the run masks folded into their upper bits, rows as
entry indices, a saturating pair of run counters (run_step / run_max), a 156 KiB LDS image with
the class words replicated per lane.  About 30 to 90 user rules beside the builtin ones give
such a table with no unusual knob.  The rule sets (tests/k1_legacy_common.py; tests/
test_k1_layout.py pins their layouts on the CPU):

  L30  user30: legacy, just past packed (68,992 bytes)
  L70  user70: legacy, 1,152 bytes under the plan's cap: the largest image
  LX   user1000 under x_step 4: legacy + K1X, keyword rows of 28 words
  PW   user1000: packed + K1X, 28 words -- the control that tells wide rows from legacy

Every test sets k1_automaton and asserts from GpuContext.k1_layout() and the batch's stats which
kernel body ran.  Every comparison is exact."""
import functools

import numpy as np
import pytest

from tests import gpu_common as GC
from tests import grid_rounds_common as R
from tests import helpers as H
from tests import k1_adapted_common as AC
from tests import k1_legacy_common as KL
from tests import lane_reuse_common as LR
from trivy_amd import configs
from trivy_amd import corpus
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

NEVER = 0xFFFFFFFF
LEGACY = (KL.L30, KL.L70, KL.LX)


@pytest.fixture(autouse=True)
def automaton(knob):
    knob("k1_automaton", 1)


def _ran(ctx, name):
    """The context's K1 is the automaton in the layout `name` is run for, and the last batch
    went through it."""
    lay = ctx.k1_layout()
    assert lay["k1_filter"] == 0, lay
    if name in LEGACY:
        assert KL.is_legacy(lay) and lay["row_unit"] == lay["stride"], lay
    else:
        assert KL.is_packed(lay) and lay["row_unit"] == 2 * lay["stride"], lay
    info = ctx.scanner.info()
    assert (lay["states"], lay["classes"], lay["kw_words"]) == (
        info["kw_states"], info["kw_classes"], (info["n_keywords"] + 31) // 32), lay
    assert ctx.stats()["k1_filter"] == 0
    return lay


def _context(name, chunk, **kw):
    kw.setdefault("adapt_mib", NEVER)
    return S.GpuContext(KL.scanner(name), 0, chunk_bytes=chunk, **kw)


# ---------------------------------------------------------------- 1. bits and events
@functools.lru_cache(maxsize=None)
def _mixed(name, nbytes, seed):
    return S.Batch.from_args(configs.mixed_batch(KL.doc(name), nbytes, seed, plants_per_file=0.9))


def _k1_batches(name, chunk):
    sc = KL.scanner(name)
    return [H.small_files_batch(chunk), corpus.k1_edge_batch(sc.k1_literals(), 7 + chunk % 5),
            _mixed(name, 256 << 10, 31 + chunk)]


@pytest.mark.parametrize("name,chunk", [(n, c) for n in (KL.L30, KL.L70) for c in (16, 48, 256, 1024)] +
                         [(n, c) for n in (KL.LX, KL.PW) for c in (16, 256)])
def test_bits_and_events(name, chunk):
    """Keyword bits and chunk events == k1_reference on many small files, the K1 edge batch of
    the rule set's own literals and a corpus with the rule set's secrets planted.  Over the
    three batches every kind of event and keyword bits occur, and for the 1,000-rule sets bits
    in keyword words past the builtin rules' four and K1X hit words."""
    sc = KL.scanner(name)
    seen = {"run-U": 0, "run-D": 0, "literal": 0, "kw words": 0, "wide words": 0, "k1x": 0, "files": 0, "bytes": 0}
    ctx = _context(name, chunk)
    try:
        for b in _k1_batches(name, chunk):
            ref = sc.k1_reference(b, chunk)
            kw, ev, st = GC.k1_on(sc, ctx, b, ref)
            _ran(ctx, name)
            rkw, rev = ref
            seen["run-U"] += int(((rev & 1) != 0).sum())
            seen["run-D"] += int(((rev & 2) != 0).sum())
            seen["literal"] += int(((rev >> 2) != 0).sum())
            seen["kw words"] += int(np.count_nonzero(rkw))
            seen["wide words"] += int(np.count_nonzero(rkw[:, 4:]))
            seen["k1x"] += st["k1x_records"] + st["k1x_inline"]
            seen["files"] += b.nfiles
            seen["bytes"] += int(b.offsets[-1])
    finally:
        ctx.close()
    print("%s chunk %d: %s" % (name, chunk, seen))
    assert seen["run-U"] and seen["run-D"] and seen["literal"] and seen["kw words"]
    if name in (KL.LX, KL.PW):
        assert seen["wide words"] and seen["k1x"]
    else:
        assert seen["k1x"] == 0


# ---------------------------------------------------------------- 2. run counters
@functools.lru_cache(maxsize=None)
def _saturation_case(name, chunk):
    b = H.run_saturation_batch()
    return b, KL.scanner(name).k1_reference(b, chunk)


@pytest.mark.parametrize("chunk", [16, 256])
@pytest.mark.parametrize("k1", ["legacy", "packed", "k1f"])
def test_run_counters_at_and_past_saturation(knob, k1, chunk):
    """helpers.run_saturation_batch (runs of 11 to 70,000 bytes of each run class at five
    offsets, one split over two files, one ending the batch) through the legacy loop's
    run_step (L70), the packed loop's pk_mad_sat (builtin rules) and K1F's run flags (builtin,
    knob reset): a counter that wraps at 256 or 65,536 instead of saturating loses the events
    of the chunks inside a run behind the wrap, and the comparison with k1_reference."""
    name = KL.L70 if k1 == "legacy" else KL.BUILTIN
    if k1 == "k1f":
        knob("k1_automaton", 0)
    sc = KL.scanner(name)
    b, ref = _saturation_case(name, chunk)
    ctx = _context(name, chunk)
    try:
        GC.k1_on(sc, ctx, b, ref)
        if k1 == "k1f":
            assert ctx.k1_layout()["k1_filter"] == 1 and ctx.stats()["k1_filter"] == 1
        else:
            _ran(ctx, name)
    finally:
        ctx.close()
    nu, nd = int(((ref[1] & 1) != 0).sum()), int(((ref[1] & 2) != 0).sum())
    print("%s chunk %d: %d files, %d bytes, run-U chunks %d, run-D chunks %d" % (
        k1, chunk, b.nfiles, int(b.offsets[-1]), nu, nd))
    assert nu > 2 * 65536 // chunk and nd > 65536 // chunk


# ---------------------------------------------------------------- 3. many rounds per block
@pytest.fixture(params=R.CAPS, ids=["cap1", "cap3"])
def cap(request, knob):
    knob("grid_cap", request.param)
    return request.param


@functools.lru_cache(maxsize=None)
def _corpus_5m():
    """5 MiB, 368 files (also the used-lane test's predecessor)."""
    return corpus.make_corpus(5 << 20, seed=41, plants_per_mib=100)[0]


@pytest.mark.parametrize("chunk", [16, 256])
@pytest.mark.parametrize("name", [KL.L70, KL.LX])
def test_many_rounds_per_block(cap, name, chunk):
    """One block and three: the persistent loop (it0 += stride) over several rounds of one staged
    156 KiB image, the last round partial, with ghost lanes.  A lane walks an item of 16 chunks,
    so `small files` (1 MiB) is 4,099 items at chunk 16 (four rounds of 1,024 lanes and a fifth
    of three items; 1.33 rounds of 3,072) but a quarter of a round at chunk 256, where the 5 MiB
    corpus (1,280 items) follows it on the same context: 1.25 rounds of one block.  Three blocks
    at chunk 256 stay under one round (0.42: ghost lanes and idle threads only), and the
    several-rounds condition is not asserted there."""
    sc = KL.scanner(name)
    batches = [H.small_files_batch(chunk)] + ([_corpus_5m()] if chunk == 256 else [])
    ctx = _context(name, chunk)
    try:
        for b in batches:
            kw, ev, st = GC.k1_on(sc, ctx, b)
            lay = _ran(ctx, name)
            assert (ev & 1).any() and (ev >> 2).any() and kw.any()
    finally:
        ctx.close()
    items = -(-int(batches[-1].offsets[-1]) // (16 * chunk))   # an item: 2 chains x 8 chunks
    lanes = cap * lay["threads"]   # (grid_cap caps the blocks of the launch)
    print("%s chunk %d cap %d: %d items, %.2f rounds" % (name, chunk, cap, items, items / lanes))
    assert items % lanes, "a full last round"
    if (chunk, cap) != (256, 3):
        assert items > lanes, "one round per block"


# ---------------------------------------------------------------- 4. adaptation
@pytest.mark.parametrize("chunk", [16, 256])
def test_adaptation_on_a_legacy_table(chunk):
    """adapt_k1 on the largest legacy table: the sampling launch (A.hits), k1_tables with the
    hot states, the re-upload and acc_row in entry-index units.  The adapting batch, then the
    K1 edge batch and a folding-rune batch on the same context."""
    sc = KL.scanner(KL.L70)
    batch = AC.case(False, sc)[0]
    nkw = sc.info()["n_keywords"]
    ctx = AC.adapted_context(sc, batch, chunk)
    try:
        a = ctx.adaptation()
        assert a["adapted"] == 1 and a["k1_filter"] == 0 and a["hot_states"] > 0
        assert a["hits"] is None and a["quiet"] is None
        assert not a["kw_unknown"][nkw - 3:].any()          # the folding-rune keywords stay exact
        assert 0 < int(a["kw_unknown"].sum()) < nkw
        _ran(ctx, KL.L70)
        AC.check_bits(sc, ctx, batch, chunk, a, scanned=True)
        AC.check_bits(sc, ctx, corpus.k1_edge_batch(sc.k1_literals(), 7 + chunk % 5), chunk, a)
        AC.check_bits(sc, ctx, corpus.fold_runes_batch(11, nbytes=512 << 10, plants=300, frac=0.3), chunk, a)
        b = ctx.adaptation()
        assert b["hot_states"] == a["hot_states"] and np.array_equal(b["kw_unknown"], a["kw_unknown"])
        _ran(ctx, KL.L70)                                    # still legacy after the rebuild
        print("L70 chunk %d: %d hot states, %d unknown keywords, ev_hot %#x, sample %d bytes" % (
            chunk, a["hot_states"], int(a["kw_unknown"].sum()), a["ev_hot"], a["sample_bytes"]))
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. downstream of a legacy K1
@pytest.mark.parametrize("chunk", [16, 256])
@pytest.mark.parametrize("name", [KL.L70, KL.LX])
def test_everything_downstream(name, chunk):
    """gpu_common.check_batch: K1, the work lists, K2's records, flags and rows against the
    references, then scan() against the exact path.  Both rule sets have more than 64 groups
    (asserted from info()), so the gate rows are at least two words wide."""
    sc = KL.scanner(name)
    batch = _mixed(name, 192 << 10, 77)
    want = sc.ScanBatch(batch, nthreads=16)
    ctx = _context(name, chunk)
    try:
        rb, tot = GC.check_batch(sc, ctx, batch)
        _ran(ctx, name)
        got = ctx.scan()
        _ran(ctx, name)
    finally:
        ctx.close()
    assert got == want
    nfind = sum(len(x["Findings"] or []) for x in want)
    print("%s chunk %d: %d files, %d bytes, %d records, %d findings, layout %s" % (
        name, chunk, batch.nfiles, int(batch.offsets[-1]), rb["cand"]["count"], nfind, tot))
    assert nfind > 10 and sc.info()["n_groups"] > 64


# ---------------------------------------------------------------- 6. a used lane
def test_used_lane():
    """`small files` on the lane a batch four times larger has just used: no buffer is allocated
    again (lane_buffers), and the bits and events are the reference's."""
    sc = KL.scanner(KL.L70)
    big = _corpus_5m()
    small = H.small_files_batch(256)
    assert int(big.offsets[-1]) >= 4 * int(small.offsets[-1]) and big.nfiles >= small.nfiles
    with LR.Lanes(sc, 256) as L:
        L.run(0, "big", lambda c: GC.k1_on(sc, c, big)[2])
        _ran(L.ctx, KL.L70)
        L.run(0, "small files", lambda c: GC.k1_on(sc, c, small)[2], reuse="all")
        assert "filler" in L.log[-2]
        _ran(L.ctx, KL.L70)
