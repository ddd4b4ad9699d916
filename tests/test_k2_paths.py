"""The item passes' reference and K2's dense, skip and overflow rules, without a device.

tsg_emulate_items is the predicate the emulation itself runs (its per-group bytes equal
tsg_emulate_candidate_stats'); layout_reference restates the device's layout decision; an
emulated context applies both and the candidate capacity, so the resolver's group_skipped
and overflow paths run here.  The inputs of tests/test_gpu_k2_paths.py and
tests/test_gpu_k2_records.py are checked for the edges they were built for, from the
reference alone: an input that stops covering its edge fails here, before it reaches a GPU.
tsg_emulate_candidates (what K2 should write, record by record) is checked against itself
(word and transition records expand to the same triples; without a dense group the unique
triples equal those of emulate_kernels' per-item form, tsg_emulate_item_candidates), and
check_candidates against outputs built from the reference."""
import numpy as np
import pytest

from tests import helpers as H
from trivy_amd import _native as N
from trivy_amd import corpus
from trivy_amd import secret as S

INF = 0xFFFFFFFF


@pytest.fixture(scope="module")
def builtin():
    return S.NewScanner(None)


@pytest.fixture(scope="module")
def corpus256k():
    return corpus.make_corpus(256 << 10, seed=7, plants_per_mib=300)[0]


def _item_bytes(batch, tri, chunk, G):
    offs = batch.offsets.astype(np.int64)
    f, c = tri[:, 1].astype(np.int64), tri[:, 2].astype(np.int64)
    n = np.minimum(offs[f + 1], (c + 1) * chunk) - np.maximum(offs[f], c * chunk)
    assert (n > 0).all()
    return np.bincount(tri[:, 0], weights=n, minlength=G).astype(np.uint64)


@pytest.mark.parametrize("chunk", [16, 256])
def test_emulate_items_is_the_emulations_item_set(builtin, corpus256k, chunk):
    """The triples are sorted, unique, inside their files, and their bytes per group are the
    bytes the emulated K2 scanned; the device's every-chunk rule only matters for groups
    whose window is longer than 16 chunks (none of the builtin ones at these sizes)."""
    G = builtin.info()["n_groups"]
    for batch in (corpus256k, H.back_window_batch(chunk)):
        tri, counts = builtin.emulate_items(batch, chunk, INF)
        _, per_group = builtin.candidate_stats(batch, chunk)
        assert len(tri) and np.array_equal(_item_bytes(batch, tri, chunk, G), per_group)
        assert np.array_equal(np.bincount(tri[:, 0], minlength=G), counts)
        key = (tri[:, 0].astype(np.int64) << 44) | (tri[:, 1].astype(np.int64) << 24) | tri[:, 2]
        assert (np.diff(key) > 0).all()
        dev, dcounts = builtin.emulate_items(batch, chunk, 16)
        assert max(b for _, b in H.group_table(builtin, chunk)) <= 16
        assert np.array_equal(dev, tri) and np.array_equal(dcounts, counts)


def test_emulate_items_every_chunk_rule(builtin):
    """max_back below a group's window turns it into an every-chunk group: with max_back 0
    every finite-back group with a window lists all chunks of its gated files, a superset
    of its items, and exactly the chunks of the files it had items in or is gated for."""
    chunk = 16
    batch = H.back_window_batch(chunk)
    tri, counts = builtin.emulate_items(batch, chunk, INF)
    all_, acounts = builtin.emulate_items(batch, chunk, 0)
    assert (acounts >= counts).all() and acounts.sum() > counts.sum()
    have = set(map(tuple, all_.tolist()))
    assert set(map(tuple, tri.tolist())) <= have
    offs = [int(x) for x in batch.offsets]
    table = H.group_table(builtin, chunk)
    for g, f in {(g, f) for g, f, _ in tri.tolist()}:
        if table[g][1] > 0:
            assert all((g, f, c) in have for c in range(offs[f] // chunk, (offs[f + 1] - 1) // chunk + 1))


def test_layout_reference_hand_made():
    L, D, K, Z = S.GROUP_LIST, S.GROUP_DENSE, S.GROUP_SKIP, S.GROUP_NONE
    # exactly at capacity; one item more does not fit
    kind, tot = S.layout_reference([10, 0, 20], 100, 30)
    assert kind.tolist() == [L, Z, L] and tot == {"items": 30, "entries": 2, "dense_entries": 0, "skipped": 0}
    kind, tot = S.layout_reference([10, 0, 21], 100, 30)
    assert kind.tolist() == [L, Z, K] and tot["skipped"] == 1 and tot["items"] == 31
    # entries of 512 items; a dense group takes ceil(nchunks / 1,024) dense entries
    kind, tot = S.layout_reference([512, 513, 3000], 4000, 1 << 16)
    assert kind.tolist() == [L, L, D] and tot["entries"] == 3 and tot["dense_entries"] == 4
    # the 2nd dense group under max_dense = 1 is skipped; the list group behind it fits (a
    # dense-wanting group has no region)
    kind, tot = S.layout_reference([60, 70, 5], 100, 1 << 16, max_dense=1)
    assert kind.tolist() == [D, K, L] and tot == {"items": 5, "entries": 1, "dense_entries": 1, "skipped": 1}
    # a list group over the capacity keeps its region: the group behind it does not fit
    # either, although its own items would; a dense group behind them is not affected
    kind, tot = S.layout_reference([10, 40, 5, 90], 100, 30)
    assert kind.tolist() == [L, K, K, D] and tot["items"] == 55 and tot["skipped"] == 2
    # half of the chunks is not dense, one more is
    assert S.layout_reference([50], 100, 1 << 16)[0].tolist() == [L]
    assert S.layout_reference([51], 101, 1 << 16)[0].tolist() == [D]
    assert S.layout_reference([], 0, 0)[1]["skipped"] == 0


def test_knob_ranges():
    for name, bad in (("k2_max_dense", 17), ("k2_max_dense", -1), ("k2_items_cap", -1), ("k2_items_cap", 1 << 31)):
        with pytest.raises(N.NativeError):
            N.knob(name, bad)
    for name in ("k2_max_dense", "k2_items_cap", "k2_no_word_recs"):
        N.knob(name, 1)
        N.knob(name, None)


def test_work_list_checker(builtin):
    """check_work_lists accepts lists built from the reference and rejects a lost item, a
    duplicated item, an overlong entry and a wrong skip flag."""
    chunk = 16
    batch = H.back_window_batch(chunk)
    n = H.nchunks_of(batch, chunk)
    tri, counts = builtin.emulate_items(batch, chunk, 16)
    for cap in (S.default_items_cap(n), H.middle_items_cap(counts, n)):
        good = H.reference_work_lists(tri, counts, n, cap)
        kind, tot = H.check_work_lists(good, tri, counts, n, cap)
        assert tot["entries"] > 0
        ent, dent, items, gskip = good
        bad_items = items.copy()
        bad_items[0] = bad_items[1]  # one item lost, one twice
        flags = gskip.copy()
        flags[int(ent[0, 0])] ^= 1
        long_ent = ent.copy()
        long_ent[0, 2] += 1
        for bad in ((ent, dent, bad_items, gskip), (ent, dent, items, flags), (long_ent, dent, items, gskip),
                    (ent[1:], dent, items, gskip)):
            with pytest.raises(AssertionError):
                H.check_work_lists(bad, tri, counts, n, cap)
    assert (kind == S.GROUP_SKIP).any() and (kind == S.GROUP_LIST).any()


def _emulated(sc, batch, chunk, **kw):
    ctx = S.GpuContext(sc, 0, chunk_bytes=chunk, emulate=True, **kw)
    ctx.upload(batch)
    got = ctx.scan()
    st = ctx.stats()
    with pytest.raises(N.NativeError):
        ctx.batch_items()  # no device, no work lists
    with pytest.raises(N.NativeError):
        ctx.batch_candidates()  # ... and no output block
    ctx.close()
    return got, st


def test_emulated_context_skip_dense_and_overflow(builtin, corpus256k, knob):
    """An emulated context under a small item capacity, one dense group, a small candidate
    capacity and transition records: groups are skipped, the candidate buffer overflows,
    and the findings are the exact CPU path's (the resolver's group_skipped and overflow
    paths on the CPU)."""
    chunk = 64
    want = builtin.ScanBatch(corpus256k, nthreads=8)
    n = H.nchunks_of(corpus256k, chunk)
    _, counts = builtin.emulate_items(corpus256k, chunk, 16)
    _, st0 = _emulated(builtin, corpus256k, chunk)
    _, tot0 = S.layout_reference(counts, n, S.default_items_cap(n))
    assert st0["groups_skipped"] == 0 and st0["overflow"] == 0 and st0["candidates"] > 63
    assert (st0["k2_items"], st0["k2_launches"], st0["k2_dense_entries"]) == (
        tot0["items"], tot0["entries"], tot0["dense_entries"])
    cap = H.middle_items_cap(counts, n)
    knob("k2_items_cap", cap)
    knob("k2_max_dense", 1)
    knob("k2_no_word_recs", 1)
    knob("emu_wordrec", 1)  # (overridden by k2_no_word_recs)
    kind, tot = S.layout_reference(counts, n, cap, 1)
    assert tot["skipped"] > 0
    for cc in (1, 63, 0):
        got, st = _emulated(builtin, corpus256k, chunk, cand_capacity=cc)
        assert got == want, cc
        assert st["groups_skipped"] == tot["skipped"], cc
        assert st["overflow"] == (1 if cc else 0) and st["candidates"] > 63, cc
        assert (st["k2_items"], st["k2_launches"]) == (tot["items"], tot["entries"])


def test_emulated_context_two_dense_groups(builtin, knob):
    """The dense batch on an emulated context: with k2_max_dense = 1 the second
    dense-wanting group (aws-access-key-id's) is skipped, and its findings still come out,
    from the host."""
    chunk, total = H.DENSE_SHAPES[0]
    batch, plants = H.dense_batch(chunk, total)
    want = builtin.ScanBatch(batch, nthreads=8)
    knob("k2_max_dense", 1)
    got, st = _emulated(builtin, batch, chunk)
    assert got == want and st["groups_skipped"] == 1 and st["k2_dense_entries"] == 3
    assert sum(f["RuleID"] == H.AKIA_GROUP_RULE for r in got for f in r["Findings"] or []) == len(plants)


def test_cand_capacity_stat_follows_the_capacity_used(builtin, corpus256k):
    """overflow compares with the capacity the kernels had: exactly the candidate count
    fits, one less overflows."""
    _, st0 = _emulated(builtin, corpus256k, 256)
    r0 = st0["candidates"]
    want = builtin.ScanBatch(corpus256k, nthreads=8)
    for cc, ovf in ((r0, 0), (r0 - 1, 1)):
        got, st = _emulated(builtin, corpus256k, 256, cand_capacity=cc)
        assert got == want and st["overflow"] == ovf and st["candidates"] == r0


# ---- the GPU tests' inputs cover their edges

@pytest.mark.parametrize("chunk", H.ITEM_CHUNKS)
def test_back_window_batch_covers_its_edges(builtin, chunk):
    batch = H.back_window_batch(chunk)
    assert int(batch.offsets[-1]) <= 1 << 20 and int(batch.offsets[-1]) % chunk
    cov = H.back_window_coverage(builtin, batch, chunk)
    if max(b for _, b in H.group_table(builtin, chunk)) < 2:
        assert chunk == 256 and not cov.pop("clamped, chunks in between")
    assert all(cov.values()), [k for k, v in cov.items() if not v]


@pytest.mark.parametrize("chunk", H.ITEM_CHUNKS)
def test_item_inputs_fit_the_default_layout_and_a_middle_cap_skips(builtin, chunk):
    """Every item-pass input is at most 1 MiB, lists several groups over more than one
    entry's worth of items, has empty files, and under middle_items_cap has listed groups
    before skipped ones."""
    for name, batch in H.item_inputs(builtin, chunk).items():
        n = H.nchunks_of(batch, chunk)
        assert int(batch.offsets[-1]) <= (1 << 20) + (64 << 10), name
        assert name == "k1 edges" or (np.diff(batch.offsets.astype(np.int64)) == 0).any(), name
        _, counts = builtin.emulate_items(batch, chunk, 16)
        kind, tot = S.layout_reference(counts, n, S.default_items_cap(n))
        assert tot["skipped"] == 0 and (kind == S.GROUP_LIST).sum() >= 3, name
        kind, tot = S.layout_reference(counts, n, H.middle_items_cap(counts, n))
        ks = kind[kind != S.GROUP_NONE].tolist()
        assert S.GROUP_LIST in ks and S.GROUP_SKIP in ks, name
        assert ks.index(S.GROUP_SKIP) > ks.index(S.GROUP_LIST), name
    _, counts = builtin.emulate_items(H.item_inputs(builtin, chunk)["small files"], chunk, 16)
    if chunk < 256:  # (1 MiB in 256-byte chunks gives no group more than one entry's items)
        assert counts.max() > S.ENTRY_ITEMS  # a group of several entries, the last one partial
        assert counts.max() % S.ENTRY_ITEMS


@pytest.mark.parametrize("chunk,total", H.DENSE_SHAPES)
def test_dense_batch_covers_its_edges(builtin, chunk, total):
    batch, plants = H.dense_batch(chunk, total)
    offs = [int(x) for x in batch.offsets]
    n = H.nchunks_of(batch, chunk)
    R, E = 4 * chunk, S.ENTRY_CHUNKS * chunk
    assert offs[-1] == total and total <= (1 << 20)
    assert n == (2 * 1024 + 300 if chunk == 16 else 1025) and (total - 1) % E < (chunk if chunk == 256 else E)
    # the group is every-chunk and gated, and the reference gives it more than half the chunks
    g = builtin.rule_group([r.ID for r in builtin.Rules].index(H.AKIA_GROUP_RULE))
    assert H.group_table(builtin, chunk)[g][0] >> 31
    tri, counts = builtin.emulate_items(batch, chunk, 16)
    kind, tot = S.layout_reference(counts, n, S.default_items_cap(n))
    assert counts[g] * 2 > n and kind[g] == S.GROUP_DENSE
    dense = np.flatnonzero(kind == S.GROUP_DENSE).tolist()
    assert len(dense) == 2 and dense[1] == g and tot["dense_entries"] == 2 * -(-n // S.ENTRY_CHUNKS)
    assert S.layout_reference(counts, n, S.default_items_cap(n), 1)[0][g] == S.GROUP_SKIP
    # list groups beside them: under middle_items_cap some are listed, later ones skipped,
    # and the dense group behind the skipped ones still runs
    ks = S.layout_reference(counts, n, H.middle_items_cap(counts, n))[0]
    ks = ks[ks != S.GROUP_NONE].tolist()
    assert ks[0] == S.GROUP_DENSE and ks[-1] == S.GROUP_DENSE and S.GROUP_LIST in ks[:ks.index(S.GROUP_SKIP)]
    gated = sorted({f for gg, f, _ in tri.tolist() if gg == g})
    sizes = np.diff(np.array(offs))
    ungated = [f for f in range(batch.nfiles) if sizes[f] and f not in gated]
    # files: empty, 1-15 bytes, a boundary inside a lane's range and one exactly on it,
    # gated and ungated alternating
    assert (sizes == 0).any() and ((sizes > 0) & (sizes < 16)).any()
    inner = [o for o in offs[1:-1]]
    assert any(o % R for o in inner) and any(o % R == 0 for o in inner)
    assert len(ungated) >= 3 and all(f - 1 in gated or sizes[f - 1] == 0 for f in ungated)
    # matches: every plant is a finding of the group's rule, and they lie where they should
    want = builtin.ScanBatch(batch, nthreads=8)
    found = sum(f["RuleID"] == H.AKIA_GROUP_RULE for r in want for f in r["Findings"] or [])
    assert found == len(plants)
    spans = [(p, p + len(H.AKIA)) for p in plants]  # [start, end)
    assert any(a // R != (b - 1) // R for a, b in spans)                     # a lane range
    assert all(any(a < e < b or (b == e + 1 == total and a < e) for a, b in spans) for e in range(E, total, E))
    assert spans[-1][1] == total                                            # the last byte
    ends = {b for _, b in spans}
    assert any(offs[f] in ends for f in ungated)                              # ungated behind it


# ---- K2's candidate records: the reference, the checker, and the inputs' edges

@pytest.fixture(scope="module")
def k2sc():
    return H.k2_scanner()


def _reference(sc, batch, chunk, ext_cap=S.DEFAULT_EXT_CAP, **kw):
    """(raw records, (file, rule id, end) triples) of the reference in both record forms; the
    forms expand to the same multiset."""
    ref = sc.emulate_candidates(batch, chunk, ext_cap, **kw)
    named = H.named_triples(sc, sc.expand_candidates(batch, ref))
    trans = sc.emulate_candidates(batch, chunk, ext_cap, word_recs=False, **kw)
    assert H.named_triples(sc, sc.expand_candidates(batch, trans)) == named
    assert not (trans[:, 1] & S.CAND_WORD & np.where(trans[:, 1] & S.CAND_TRANS, 0xFFFFFFFF, 0)).any()
    assert len(trans) >= len(ref) and len(ref) < S.DEFAULT_CAND_CAPACITY
    return ref, named


def _equals_item_form(sc, batch, chunk, named, ext_cap=S.DEFAULT_EXT_CAP):
    """The reference's unique triples are those of emulate_kernels' per-item form (run_segment
    over every item): holds where no group is dense, a list item being one segment in both."""
    item = H.named_triples(sc, sc.emulate_item_candidates(batch, chunk, ext_cap))
    assert sorted(set(named)) == sorted(set(item))


def _list_only(sc, batch, chunk):
    n = H.nchunks_of(batch, chunk)
    _, counts = sc.emulate_items(batch, chunk, 16)
    kind, tot = S.layout_reference(counts, n, S.default_items_cap(n))
    assert tot["skipped"] == 0 and tot["dense_entries"] == 0 and (kind == S.GROUP_LIST).any()
    return counts


@pytest.mark.parametrize("chunk", H.K2_CHUNKS)
def test_word_mask_batch_covers_its_edges(k2sc, chunk):
    """The reference's triples are exactly the planted ones (no record for a split secret,
    none from a neighbouring file's bytes), and the files lie where the edges need them."""
    batch, want, notes = H.word_mask_batch(chunk)
    offs = [int(x) for x in batch.offsets]
    assert offs[-1] <= 128 << 10 and offs[-1] % chunk
    _list_only(k2sc, batch, chunk)
    ref, named = _reference(k2sc, batch, chunk)
    assert named == want
    data = bytes(batch.data)
    # base == 0 and a file on the chunk's first byte
    assert offs[notes["first"]] == 0 and (notes["first"], "short", 6) in want
    for r, f in notes["starts"].items():  # a file starting at offset r of a word, a \b behind a letter
        assert offs[f] % chunk and offs[f] % 16 == r and data[offs[f] - 1:offs[f] + 3] == b"qwbk"
        end = offs[f] + 7
        assert (end // 16 == offs[f] // 16) == (r != 15)  # the accept inside the first, partial word
    for r, (f, g) in notes["ends"].items():  # an accept on the last byte, digits behind it in the word
        fe = offs[f + 1]
        assert fe % 16 == r and g == f + 1 and (f, "short", fe - offs[f] - 1) in want
        assert data[fe - 7:fe + 3] == b"shk123456 " and not [t for t in want if t[0] == g]
    for name, (f, g, cut) in notes["splits"].items():
        fe = offs[f + 1]
        assert g == f + 1 and fe - offs[f] == cut and not [t for t in want if t[0] in (f, g)]
        assert b"bdk=abcdefghijklmnopqrst;" in data[offs[f]:offs[g + 1]]
        start = fe - 12
        # the cut inside a word / on a word boundary, both inside the secret's chunk; behind the
        # chunk's end, inside a word of the next chunk
        assert {"word": fe % 16 and start // chunk == fe // chunk,
                "boundary": fe % 16 == 0 and fe % chunk and start // chunk == fe // chunk,
                "chunk": start // chunk < (fe - 1) // chunk and fe % 16}[name], (name, start, fe)
    f, ends = notes["body"]  # every position of a word: secret and accept in one chunk ...
    assert {(offs[f] + e) % 16 for e in ends} == set(range(16))
    assert all((offs[f] + e - 6) // chunk == (offs[f] + e) // chunk for e in ends)
    f, ends = notes["tail"]  # ... and the accept in the chunk behind the secret's literal
    assert {(offs[f] + e) % 16 for e in ends} == set(range(16)) and offs[f] % chunk == 0
    assert all(data[(offs[f] + e) // chunk * chunk - 4:][:4] == b"bdk=" for e in ends)
    f, starts = notes["ctx"]  # an item that starts mid-file: the byte before the chunk decides
    assert offs[f] % chunk == 0 and [data[offs[f] + s - 1:offs[f] + s] for s in starts] == [b"a", b" ", b"\n"]
    assert [(f, "wb", s + 7) in want for s in starts] == [False, True, True]
    last = notes["last"]
    assert last == batch.nfiles - 1 and offs[last] // chunk == (offs[-1] - 1) // chunk and offs[last] % chunk == 0
    assert len(set(named)) == len(named)
    _equals_item_form(k2sc, batch, chunk, named)


@pytest.mark.parametrize("ext_cap", [S.DEFAULT_EXT_CAP, 64, 40])
@pytest.mark.parametrize("chunk", H.K2_CHUNKS)
def test_tail_batch_covers_its_edges(k2sc, chunk, ext_cap):
    batch, want, notes = H.tail_batch(chunk, ext_cap)
    offs = [int(x) for x in batch.offsets]
    assert offs[-1] <= 128 << 10
    _list_only(k2sc, batch, chunk)
    ref, named = _reference(k2sc, batch, chunk, ext_cap)
    assert named == H.with_group_mates(k2sc, want)
    _equals_item_form(k2sc, batch, chunk, named, ext_cap)
    cut = (ext_cap + 15) // 16 * 16
    size = lambda name: offs[notes[name] + 1] - offs[notes[name]]
    assert all(offs[f] % chunk == 0 for f in notes.values())
    assert size("fe on chunk end") == chunk and size("fe mid-word in a tail") % 16
    assert (notes["alive at fe, accepts at eot"], "bounded", size("alive at fe, accepts at eot")) in want
    assert (notes["eot rule at fe in a tail"], "eot", size("eot rule at fe in a tail")) in want
    whole = {f for f, _, e in want if e == H.WHOLE}
    assert notes["immortal"] in whole
    if ext_cap == S.DEFAULT_EXT_CAP:
        assert whole == {notes["immortal"]}
        assert (notes["crosses a whole chunk"], "bounded", 2 * chunk + 31) in want
    else:
        assert cut == (64 if ext_cap == 64 else 48)
        assert (notes["ends on the last followed byte"], "bounded", chunk + cut - 1) in want
        assert notes["ends on the last followed byte"] not in whole and notes["alive at the cut"] in whole
        # every rule of the group, once
        g = k2sc.rule_group(H.rule_index(k2sc, "bounded"))
        mates = sorted(r.ID for i, r in enumerate(k2sc.Rules) if k2sc.rule_group(i) == g)
        assert sorted(r for f, r, e in named if f == notes["alive at the cut"]) == mates and len(mates) > 1


@pytest.mark.parametrize("chunk", H.K2_CHUNKS)
def test_entry_shape_batches_have_their_item_counts(k2sc, chunk):
    g = k2sc.rule_group(H.rule_index(k2sc, "short"))
    for n in H.ENTRY_COUNTS:
        batch, want = H.entry_shape_batch(chunk, n)
        assert int(batch.offsets[-1]) <= 1 << 20
        counts = _list_only(k2sc, batch, chunk)
        assert counts[g] == n and counts.sum() == n
        ref, named = _reference(k2sc, batch, chunk)
        assert named == want and len(ref) == n
        _equals_item_form(k2sc, batch, chunk, named)


@pytest.mark.parametrize("chunk,total", H.DENSE_SHAPES)
def test_dense_reference_and_whole_file_records(builtin, chunk, total):
    """The dense groups' reference follows the lane ranges, not the items: with ext_cap 64
    the long tokens give the run-U group kCandWhole records from a range inside one file
    (four chunk segments, a tail behind each) and from a range shared by files (one segment
    and one tail per file), counted here from the geometry alone.  At the default ext_cap
    the batch has none."""
    n = H.nchunks_of(H.dense_batch(chunk, total)[0], chunk)
    for long_tokens in (False, True):
        batch, _ = H.dense_batch(chunk, total, long_tokens)
        ref, named = _reference(builtin, batch, chunk)
        assert not [t for t in named if t[2] == H.WHOLE]
        if not long_tokens:  # the batch as it is has no tail of 64 bytes: ext_cap 64 changes nothing
            assert _reference(builtin, batch, chunk, 64)[1] == named
    ref, named = _reference(builtin, batch, chunk, 64)
    _, counts = builtin.emulate_items(batch, chunk, 16)
    kind, _ = S.layout_reference(counts, n, S.default_items_cap(n))
    g = int(np.flatnonzero(kind == S.GROUP_DENSE)[0])
    rules = [r.ID for i, r in enumerate(builtin.Rules) if builtin.rule_group(i) == g]
    offs = [int(x) for x in batch.offsets]
    data = bytes(batch.data)
    R = 4 * chunk
    token = b"key=" + b"Zz9" * 45 + b"\n"
    at = [i for i in range(len(data)) if data.startswith(token, i)]
    assert len(at) == 2 and at[0] < offs[1] and offs[1] % R == 0  # file 0: one-file ranges only
    f = max(k for k in range(batch.nfiles) if offs[k] <= at[1])
    assert f > 0 and offs[f] % R and at[1] >= offs[f] and offs[f] // R == (at[1] + 20) // R - 1  # the range f starts in
    whole = {}
    for ff, r, e in named:
        if e == H.WHOLE:
            whole[(ff, r)] = whole.get((ff, r), 0) + 1
    assert {k[0] for k in whole} == {0, f} and {k[1] for k in whole} == set(rules)
    # a tail is alive 64 bytes behind a segment's end e when the token's run covers
    # [e - 1, e + 64): chunk ends in a one-file range, the range's end alone in a shared one
    for ff, s0 in ((0, at[0]), (f, at[1])):
        ends = [e for e in range(0, total, chunk) if s0 + 4 <= e and e + 64 <= s0 + len(token) - 1]
        if ff == f:
            ends = [e for e in ends if not offs[f] // R * R < e < (offs[f] // R + 1) * R]
        assert ends and all(whole[(ff, r)] == len(ends) for r in rules), (ff, ends, whole)


@pytest.mark.parametrize("chunk,total", H.DENSE_SHAPES)
def test_hex_lines_batch_sends_a_look_ahead_table_through_the_dense_pass(chunk, total):
    """The file of 32-hex-digit lines under the "assert" rules of tests/cover_common.py: the
    group of (?m)^[a-f0-9]{32}$ (anchor: a class-U run, which every chunk holds) has an item in
    more than half of the chunks and gets the dense pass, its device table is look-ahead (the
    trailing (?m)$), every whole line is a finding and nothing else is, the reference stays
    under the default candidate capacity and both record forms expand alike."""
    from oracle import goregex
    from tests import cover_common as CC
    sc, _ = CC.rule_set("assert")
    batch = H.hex_lines_batch(total)
    n = H.nchunks_of(batch, chunk)
    assert batch.nfiles == 1 and int(batch.offsets[-1]) == total and total % 33
    r = [x.ID for x in sc.Rules].index("hex32")
    g = sc.rule_group(r)
    assert sc.group_table(g) == {"rules": [r], "per_state": False}
    assert CC.plan_of(sc, r)["kind"] == "run U"
    _, counts = sc.emulate_items(batch, chunk, 16)
    kind, tot = S.layout_reference(counts, n, S.default_items_cap(n))
    assert counts[g] * 2 > n and kind[g] == S.GROUP_DENSE and tot["skipped"] == 0
    ref, named = _reference(sc, batch, chunk)
    lines = [(0, "hex32", 33 * i + 32) for i in range(total // 33)]
    assert [t for t in named if t[1] == "hex32"] == lines
    want = sc.ScanBatch(batch, nthreads=8)
    assert sum(f["RuleID"] == "hex32" for f in want[0]["Findings"]) == len(lines)
    if chunk == 16:   # (the oracle on the smaller shape: the lines are what it finds)
        body = bytes(batch.data[:total])
        assert [e for _, e in goregex.MustCompile(sc.Rules[r].Regex).FindAllIndex(body)] == [t[2] for t in lines]
    assert sc.ScanBatch(batch, emulate_chunk=chunk) == want


def test_many_group_inputs_fit_the_default_capacity(builtin, corpus256k):
    """The seeded corpora of the record tests: under the default capacity, word and
    transition forms agree, and on the 256 KiB corpus the word form is the shorter one and
    the triples are those of emulate_kernels' per-item form (no dense group, no tail at the
    cap)."""
    from trivy_amd import configs
    ref, named = _reference(builtin, corpus256k, 256)
    assert 64 < len(ref) < len(builtin.emulate_candidates(corpus256k, 256, word_recs=False))
    _list_only(builtin, corpus256k, 256)
    _equals_item_form(builtin, corpus256k, 256, named)
    assert not [t for t in named if t[2] == H.WHOLE]
    user = S.NewScanner(S.config_from_dict(configs.user_rules_doc(1000, 4)))
    batch, _ = corpus.make_corpus(128 << 10, seed=9, plants_per_mib=300)
    ref, named = _reference(user, batch, 256)
    assert len(ref) > 64 and user.info()["n_groups"] > builtin.info()["n_groups"]
    _list_only(user, batch, 256)
    _equals_item_form(user, batch, 256, named)


def test_item_pass_inputs_fit_the_default_capacity(builtin):
    """The item-pass inputs of the record tests at chunk 256: under the default capacity, both
    record forms agree, and the list-only ones equal the per-item form."""
    for name, batch in H.item_inputs(builtin, 256).items():
        ref, named = _reference(builtin, batch, 256)
        _list_only(builtin, batch, 256)
        _equals_item_form(builtin, batch, 256, named)


def test_candidate_checker(k2sc, builtin, corpus256k):
    """check_candidates accepts the reference against itself (records in another order) and
    rejects a lost record, a duplicated record, an end shifted by one, a kCandWhole swapped
    for an end, a wrong flag and a wrong keyword row; under a capacity it accepts the
    reference's own overflow and rejects an unflagged file and a flag without a record; with
    a host-only rule or a skipped group it wants every file's row, and only then."""
    chunk = 128
    batch, want, notes = H.tail_batch(chunk, 64)
    ref = k2sc.emulate_candidates(batch, chunk, 64, word_recs=False)  # (an end is a transition's)
    good = H.reference_output(k2sc, batch, chunk, ref)
    assert H.check_candidates(good, ref, batch, k2sc, chunk) == (len(ref), len(H.with_group_mates(k2sc, want)))
    rec = good["records"]
    whole = int(np.flatnonzero(rec[:, 2] == H.WHOLE)[0])
    plain = int(np.flatnonzero((rec[:, 2] != H.WHOLE) & (rec[:, 1] & S.CAND_TRANS != 0))[0])

    def bad(**kw):
        out = dict(good)
        out.update(kw)
        with pytest.raises(AssertionError) as e:
            H.check_candidates(out, ref, batch, k2sc, chunk)
        return str(e.value)
    msg = bad(records=np.delete(rec, plain, axis=0), count=len(rec) - 1)
    assert "missing" in msg and "chunk" in msg and "group" in msg and "offset" in msg
    assert "extra" in bad(records=np.vstack([rec, rec[plain:plain + 1]]), count=len(rec) + 1)
    bad(records=np.vstack([rec, rec[plain:plain + 1]]))   # the count alone
    shifted = rec.copy()
    shifted[plain, 2] += 1
    bad(records=shifted)
    swapped = rec.copy()
    swapped[whole, 2] = 5
    bad(records=swapped)
    swapped = rec.copy()
    swapped[plain] = (rec[plain, 0], H.rule_index(k2sc, "short"), H.WHOLE)
    bad(records=swapped)
    f = int(rec[plain, 0])
    for bit in (1, 2, 4):
        flags = good["flags"].copy()
        flags[f] ^= bit
        bad(flags=flags)
    flags = good["flags"].copy()
    flags[0] |= 4  # a filler file: no record, no row
    assert not (good["flags"][0] & 4)
    bad(flags=flags)
    kw = good["kw"].copy()
    kw[f, 0] ^= 1
    bad(kw=kw)
    # every row: a rule set with a host-only rule, and a batch with a skipped group
    host = H.hostonly_scanner()
    href = host.emulate_candidates(batch, chunk, 64)
    every = H.reference_output(host, batch, chunk, href)
    assert (every["flags"] & 4).all() and not (good["flags"] & 4).all()
    H.check_candidates(every, href, batch, host, chunk)
    sref = k2sc.emulate_candidates(batch, chunk, 64, items_cap=0)  # nothing fits: every group skipped
    assert len(sref) == 0
    every = H.reference_output(k2sc, batch, chunk, sref, skipped=True)
    H.check_candidates(every, sref, batch, k2sc, chunk, skipped=True)
    sparse = H.reference_output(k2sc, batch, chunk, sref)
    for out, sc_, r_, kw_ in ((sparse, k2sc, sref, {"skipped": True}), (every, k2sc, sref, {}),
                              (dict(every, flags=good["flags"], kw=good["kw"]), host, href, {})):
        with pytest.raises(AssertionError):
            H.check_candidates(out, r_, batch, sc_, chunk, **kw_)
    # the 256 KiB corpus under a capacity
    ref = builtin.emulate_candidates(corpus256k, 256)
    for cap in (len(ref) - 1, 63, 1):
        out = H.reference_output(builtin, corpus256k, 256, ref, cand_cap=cap)
        H.check_candidates(out, ref, corpus256k, builtin, 256)
        flagged = np.flatnonzero(out["flags"] & 1)
        assert len(flagged)
        flags = out["flags"].copy()
        flags[flagged[0]] &= ~np.uint8(1)
        with pytest.raises(AssertionError):
            H.check_candidates(dict(out, flags=flags), ref, corpus256k, builtin, 256)
        clean = np.flatnonzero(np.bincount(ref[:, 0], minlength=corpus256k.nfiles) == 0)
        flags = out["flags"].copy()
        flags[clean[0]] |= 5
        with pytest.raises(AssertionError):
            H.check_candidates(dict(out, flags=flags), ref, corpus256k, builtin, 256)
        with pytest.raises(AssertionError):  # a record of its own making
            extra = out["records"].copy()
            extra[0, 1:] = (0, 0x7FFFFFF0)
            H.check_candidates(dict(out, records=extra), ref, corpus256k, builtin, 256)
