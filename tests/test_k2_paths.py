"""The item passes' reference and K2's dense, skip and overflow rules, without a device.

tsg_emulate_items is the predicate the emulation itself runs (its per-group bytes equal
tsg_emulate_candidate_stats'); layout_reference restates the device's layout decision; an
emulated context applies both and the candidate capacity, so the resolver's group_skipped
and overflow paths run here.  The inputs of tests/test_gpu_k2_paths.py are checked for the
edges they were built for, from the reference alone: an input that stops covering its edge
fails here, before it reaches a GPU."""
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
