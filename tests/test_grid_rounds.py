"""The inputs of tests/test_gpu_grid_rounds.py meet their conditions, proved without a device.

Under the knob grid_cap a kernel runs with 1 or 3 blocks, so a small batch takes each block
through its loop many times.  A capped test that silently ran one round would prove nothing:
here every input's claim is asserted from the references and the kernels' block shapes
(trivy_amd.secret) alone -- each block of the capped grid runs its loop three times or more and
the last round is partial -- and K2's persistent loop gets the entry sequences it needs."""
import numpy as np
import pytest

from tests import cover_common as CC
from tests import device_layer_common as XL
from tests import device_spans_common as XS
from tests import grid_rounds_common as R
from tests import helpers as H
from tests.device_input_common import big_file_batch, want_segments
from tests.gpu_common import k2_input
from trivy_amd import _native as N
from trivy_amd import corpus
from trivy_amd import secret as S

CAPS = R.CAPS


@pytest.fixture(scope="module")
def builtin():
    return S.NewScanner(None)


@pytest.fixture(scope="module")
def user():
    return S.NewScanner(S.config_from_dict(R.user_doc()))


def test_grid_cap_knob(builtin, knob):
    """grid_cap rejects a negative value, accepts 0 and a cap, and an emulated context (which
    launches nothing) scans the same under it."""
    with pytest.raises(N.NativeError):
        N.knob("grid_cap", -1)
    batch = corpus.make_corpus(64 << 10, seed=3, plants_per_mib=300)[0]
    want = builtin.ScanBatch(batch, nthreads=4)
    for cap in (0, 1, 3):
        knob("grid_cap", cap)
        ctx = S.GpuContext(builtin, 0, emulate=True)
        ctx.upload(batch)
        assert ctx.scan() == want
        assert ctx.stats()["k1x_img_bytes"] == 0
        ctx.close()


def test_rounds_arithmetic():
    assert R.rounds(65555, 8192, 1) == (9, 9, 19) and R.rounds(65555, 8192, 3) == (3, 3, 16403)
    assert R.many_rounds(65555, 8192, 3) and not R.many_rounds(65536, 8192, 3)  # (block 2: two rounds)
    assert not R.many_rounds(3 * 768, 256, 3) and R.many_rounds(3 * 768 + 1, 256, 3)  # (a full last round)
    assert R.many_rounds(2049, 256, 3) and not R.many_rounds(2048, 256, 3)
    assert R.many_rounds(3, 1, 1) and not R.many_rounds(2, 1, 1)


@pytest.mark.parametrize("cap", CAPS)
def test_k1x_totals(cap):
    """k1x_kernel: a round is cap x 64 KiB, one word per lane cap x 16 KiB.  The four totals end
    exactly on the third round, one byte into a fourth, on the third round's first word per
    lane, and 87 bytes into its third word; the batches have exactly these bytes."""
    Rb, U = cap * R.K1X_ROUND_BYTES, cap * R.K1X_LANE_BYTES
    assert (Rb, U) == (cap * (64 << 10), cap * (16 << 10))
    shapes = []
    for total in R.k1x_totals(cap):
        n, last_block, tail = R.rounds(total, R.K1X_ROUND_BYTES, cap)
        assert n >= 3 and total < 600 << 10
        shapes.append((n, tail))
        b = R.k1x_batch(total)
        assert int(b.offsets[-1]) == total and b.nfiles > 10
    assert shapes == [(3, Rb), (4, 1), (3, U), (3, 2 * U + 87)]
    assert (2 * U + 87) % 16 and 2 * U < 2 * U + 87 < 3 * U  # ends mid-word, inside u = 2
    # at a grid of one, the overflow batch of test_k1x_list_overflow_inline_verify still
    # overflows the single slice: 131,072 hit words against total / 256 + 65,536 records
    total = 64 * ((32 << 10) + 5)
    assert 64 * (32 << 10) // 16 == 131072 > total // 256 + 65536


def test_user_rule_set_has_k1x(user):
    assert user.info()["k1x_literals"] > 800 and user.info()["n_groups"] > 900


@pytest.mark.parametrize("cap", CAPS)
def test_rounds_corpus_conditions(builtin, cap):
    """The corpus of (1 << 20) + 301 bytes at chunk 16: ev_compact_block (8,192 chunks per block
    and round), both item passes (nev + F units, 256 per block and round), and K2's list pass
    (a change of group and a run of entries of one group)."""
    b = R.rounds_corpus()
    chunk = R.ROUNDS_CHUNK
    n = H.nchunks_of(b, chunk)
    assert int(b.offsets[-1]) == (1 << 20) + 301 and n == 65555
    assert R.COMPACT_CHUNKS == 8192 and R.many_rounds(n, R.COMPACT_CHUNKS, cap)
    ng, nb, tail = R.rounds(n, R.COMPACT_CHUNKS, cap)
    assert (ng, nb, tail) == ((9, 9, 19) if cap == 1 else (3, 3, 16403))
    # (cap 3: block 2's third round starts at chunk 65,536 and holds 19 chunks: whole waves empty)
    assert n - 2 * cap * R.COMPACT_CHUNKS - (cap - 1) * R.COMPACT_CHUNKS == 19 or cap == 1
    # ... and a lost last round would show: those 19 chunks hold events and items
    _, ev = builtin.k1_reference(b, chunk)
    tri, _ = builtin.emulate_items(b, chunk, 16)
    assert np.count_nonzero(ev[65536:] & 0x7FFFFFFF) >= 2 and (tri[:, 2] >= 65536).sum() > 10
    units = R.event_chunks(builtin, b, chunk) + b.nfiles
    assert R.many_rounds(units, S.BLOCK_THREADS, cap), units
    _, counts = builtin.emulate_items(b, chunk, 16)
    kind, tot = S.layout_reference(counts, n, S.default_items_cap(n))
    assert tot["skipped"] == 0 and tot["entries"] > 3 * cap and (kind == S.GROUP_LIST).sum() > 10
    assert len(builtin.emulate_candidates(b, chunk)) < S.DEFAULT_CAND_CAPACITY


def _staging(seq):
    """(changes of group, entries behind one of their own group, returns to an earlier group)."""
    change = sum(1 for a, b in zip(seq, seq[1:]) if a != b)
    reuse = sum(1 for a, b in zip(seq, seq[1:]) if a == b)
    back = sum(1 for i in range(1, len(seq)) if seq[i] != seq[i - 1] and seq[i] in seq[:i - 1])
    return change, reuse, back


def test_k2_entry_sequences(builtin, user):
    """At a grid of one the single block runs the entries 0 .. E-1 in order, so the entry
    groups of the reference work lists are the order in which k2_run stages DFAs.  Of the K2
    inputs, the list pass gets changes of group (a restage) and runs of one group (the staged
    tables are reused) in one input (the rounds corpus) and each alone in others; the dense
    pass gets two groups of three entries each.

    A return to a group staged earlier cannot occur in one launch: layout_block, like
    layout_reference, gives the groups their entries in id order, so the sequence never
    decreases (asserted here).  A stale `staged` would still show: after a change of group the
    new group's entries would run on the old tables."""
    k2 = H.k2_scanner()
    inputs = {
        "rounds corpus": (builtin, R.rounds_corpus(), R.ROUNDS_CHUNK),
        "many groups, user rules": (user, k2_input(user, ("corpus", 128 << 10, 9)), 256),
        "many groups, builtin rules": (builtin, k2_input(builtin, ("corpus", 256 << 10, 7)), 256),
        "entry shapes": (k2, H.entry_shape_batch(*R.ENTRY_SHAPE)[0], R.ENTRY_SHAPE[0]),
        "dense": (builtin, H.dense_batch(*H.DENSE_SHAPES[0])[0], H.DENSE_SHAPES[0][0]),
        "user items": (user, R.user_items_batch(), R.ROUNDS_CHUNK),
        "assertion contexts": (CC.rule_set("assert")[0], CC.fixture_batch("assert").batch, 256),
    }
    seen = {}
    for name, (sc, batch, chunk) in inputs.items():
        lst, dns = R.entry_groups(sc, batch, chunk)
        assert lst == sorted(lst) and dns == sorted(dns), name
        assert len(lst) >= 3, name  # the block's claim loop runs three times or more
        seen[name] = (_staging(lst), _staging(dns))
        assert len(sc.emulate_candidates(batch, chunk)) < S.DEFAULT_CAND_CAPACITY, name
    assert all(s[0][2] == 0 and s[1][2] == 0 for s in seen.values())
    c, r, _ = seen["rounds corpus"][0]
    assert c >= 10 and r >= 10
    assert seen["many groups, user rules"][0][0] > 50 and seen["many groups, builtin rules"][0][0] > 30
    assert seen["entry shapes"][0] == (0, 2, 0)
    lst, dns = R.entry_groups(builtin, H.dense_batch(*H.DENSE_SHAPES[0])[0], H.DENSE_SHAPES[0][0])
    assert len(set(dns)) == 2 and all(dns.count(g) >= 2 for g in set(dns)) and seen["dense"][1][:2] == (1, 4)
    # one block lays out the entries of hundreds of list groups (g % gridDim.x)
    lst, _ = R.entry_groups(user, R.user_items_batch(), R.ROUNDS_CHUNK)
    assert len(set(lst)) >= 200 and user.info()["n_groups"] > 900
    # the overflow input exceeds its own capacity
    assert len(builtin.emulate_candidates(k2_input(builtin, ("corpus", 256 << 10, 7)), 256)) > 63


@pytest.mark.parametrize("cap", CAPS)
def test_outputs_batch_conditions(builtin, cap):
    """outputs_kernel: files and 16-B words of candidate records against 256 threads per block;
    the record bytes leave a tail under 16 for copy_range's byte loop."""
    b = R.outputs_batch()
    ref = builtin.emulate_candidates(b, 256)
    assert b.nfiles > 3 * 3 * 256 and len(ref) > 3072 and len(ref) % 4
    assert len(ref) < S.DEFAULT_CAND_CAPACITY
    assert R.many_rounds(b.nfiles, S.BLOCK_THREADS, cap)
    assert R.many_rounds(len(ref) * 12 // 16, S.BLOCK_THREADS, cap) and (len(ref) * 12) % 16
    sizes = np.diff(b.offsets.astype(np.int64))
    assert (sizes == 0).sum() > 300
    out = H.reference_output(builtin, b, 256, ref)
    assert 0 < int((out["flags"] & 4 != 0).sum()) < b.nfiles  # sparse rows: some files, not all
    assert S.OUT_BLOCKS > max(CAPS)


@pytest.mark.parametrize("cap", CAPS)
def test_k1_and_prep_conditions(cap):
    """k1_kernel (the automaton): a thread takes an item of 16 chunks, a block has 512 or 1,024
    threads; small_files_batch at chunk 16 gives a grid of one at least three rounds at either
    block size (chunk 256: a single partial round, run for the partial block alone).
    prep_kernel: the 4 MiB batches of the grow-shrink-grow sequence zero nchunks / 4 16-B words
    of event bits with 256 threads per block."""
    items = H.nchunks_of(H.small_files_batch(16), 16) // 16
    assert R.rounds(items, 1024, 1)[1] >= 3 and R.rounds(items, 512, cap)[1] >= 2
    assert R.rounds((4 << 20) // 256 // 4, S.BLOCK_THREADS, cap)[1] >= 3  # (16 rounds and 5)


@pytest.mark.parametrize("cap", CAPS)
def test_device_input_conditions(builtin, cap):
    """The device-resident inputs: stage_kernel's 16-B words, the gather / fetch segments (a
    block per segment), the gate's spans and tar_mark_kernel's bitmap words (a wave each)."""
    # gather into the lane buffer: one segment per kept, non-empty file that touches no other
    for kind in ("shuffled", "big file"):
        lay = XS.order_layout("shuffled") if kind == "shuffled" else XS.big_layout()
        kept = ~lay.binary()
        b = lay.batch(kept)
        files = [f for f in range(b.nfiles) if b.offsets[f + 1] > b.offsets[f]]
        segs = want_segments(b.offsets.astype(np.int64), files, lay.starts[kept])
        assert len(segs) >= 10 and R.many_rounds(len(segs), 1, cap), (kind, len(segs))
    # the fetch of the files with findings alone (the resolver reads more: never fewer segments)
    b = big_file_batch(48)
    want = builtin.ScanBatch(b, nthreads=4)
    segs = want_segments(b.offsets.astype(np.int64), [f for f, r in enumerate(want) if r["Findings"]])
    assert len(segs) >= 10 and R.many_rounds(len(segs), 1, cap)
    nspans = len(XS.gate_layout().contents)
    assert nspans >= 40 and R.many_rounds(nspans, R.WAVES, cap)
    words = -(-4097 // 64)
    assert words == 65 and R.many_rounds(words, R.WAVES, cap)
    # 17 rounds of four waves, the last with one; 6 rounds of twelve, the last with five
    assert R.rounds(words, R.WAVES, cap)[::2] == ((17, 1) if cap == 1 else (6, 5))
    assert len(XL.mixed_blocks(130, 9)) == 130 * 512
