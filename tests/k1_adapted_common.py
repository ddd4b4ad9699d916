"""The adapted K1's device comparisons, shared by tests/test_gpu_k1_adapted.py (fresh contexts)
and tests/test_gpu_lane_reuse.py (an adapted context that has run other batches since): the
adapting batches and their unadapted references, computed once, K1's bits and events against
k1_reference / k1f_emulate, and the item lists and K2's records against the unadapted
emulation (equal where the adaptation touched nothing, supersets elsewhere)."""
import functools

import numpy as np

from tests import helpers as H
from trivy_amd import secret as S


@functools.lru_cache(maxsize=None)
def scanner():
    return S.NewScanner(None)


@functools.lru_cache(maxsize=None)
def case(fold_hot, sc=None):
    """(batch, picks, plain counts per literal, predicted quiet set) of an adapting batch for
    the scanner sc (default: the builtin rules')."""
    sc = scanner() if sc is None else sc
    batch, picks = H.adapted_batch(sc, fold_hot=fold_hot)
    counts = H.literal_counts(sc, batch)
    nkw = sc.info()["n_keywords"]
    quiet, tied = H.predict_quiet(counts, int(batch.offsets[-1]), set(range(nkw - 3, nkw)))
    assert not tied
    return batch, picks, counts, quiet


@functools.lru_cache(maxsize=None)
def big_case():
    return H.adapted_batch(scanner(), H.ADAPT_BIG_TOTAL)[0]


def item_refs(sc, batch, chunk):
    """The unadapted references of a batch: item triples and counts, the per-item candidate
    triples, the exact findings."""
    tri, counts = sc.emulate_items(batch, chunk, 16)
    return tri, counts, sc.emulate_item_candidates(batch, chunk), sc.ScanBatch(batch, nthreads=16)


@functools.lru_cache(maxsize=None)
def item_case(fold_hot, chunk):
    """item_refs of an adapting batch."""
    return item_refs(scanner(), case(fold_hot)[0], chunk)


def adapted_context(sc, batch, chunk=0):
    """A context with adapt_mib = 1 after kernels() of the adapting batch."""
    ctx = S.GpuContext(sc, 0, chunk_bytes=chunk, adapt_mib=1)
    ctx.upload(batch)
    ctx.kernels()
    return ctx


def kw_mask(nkw, W, ids):
    m = np.zeros(W, dtype=np.uint32)
    for k in ids:
        if k < nkw:
            m[k // 32] |= np.uint32(1 << (k % 32))
    return m


def check_bits(sc, ctx, batch, chunk, a, scanned=False):
    """K1's output for `batch` on the adapted context against the references: outside the
    unknown keywords and the hot event classes it equals k1_reference, inside it is a subset;
    K1F's equals k1f_emulate without the quiet literals exactly, its quiet columns are zero."""
    if not scanned:
        ctx.upload(batch)
        ctx.kernels()
    kw, ev = ctx.k1_output(chunk)
    rkw, rev = sc.k1_reference(batch, chunk)
    nkw = sc.info()["n_keywords"]
    unknown = kw_mask(nkw, kw.shape[1], np.flatnonzero(a["kw_unknown"]).tolist())
    hot = np.uint32(a["ev_hot"])
    assert np.array_equal(kw & ~unknown, rkw & ~unknown)
    assert np.array_equal(ev & ~hot, rev & ~hot)
    assert not (kw & ~rkw).any() and not (ev & ~rev).any()
    if a["k1_filter"]:
        assert not (kw & unknown).any()
        if not sc.info()["k1x_literals"]:  # (the emulation is K1F's alone: no K1X bits)
            fk, fe, _ = sc.k1f_emulate(batch, chunk, np.flatnonzero(a["quiet"]).tolist())
            assert np.array_equal(kw, fk)
            assert np.array_equal(ev, fe)


def rows(a):
    return set(map(tuple, np.asarray(a, dtype=np.int64).reshape(-1, 2).tolist()))


def check_lists_and_records(sc, batch, chunk, a, st, kw_dev, lists, dev, tri, counts, cand_ref, mixed=False,
                            dense_full=True):
    """gates_kernel, the item passes and K2 with opened gates (galways, d_galw) and
    everywhere-events (kEvAlways, gofbit row 31), for the last kernels() call of an adapted
    context: a = its adaptation(), st, kw_dev, lists and dev what stats(), k1_output(),
    batch_items() and batch_candidates() gave for `batch`; tri, counts, cand_ref the batch's
    unadapted references (item_refs).  The groups the adaptation touched hold supersets of the
    reference's items (every chunk of every non-empty file where gate and events are both
    open), the others exactly the reference's; the records of untouched groups' rules equal
    the reference's, and none of the reference's is missing.  mixed: the reference has
    records of touched and of untouched rules.  dense_full: every touched group in the dense
    pass has gate and events both open, as on the adapting batches (False: a touched group
    with one of them open may also reach the dense pass; its count is not known then, only
    that it is over half of the chunks, which is all the layout reads of it)."""
    ent, dent, items, gskip = lists
    G, F = sc.info()["n_groups"], batch.nfiles
    n = H.nchunks_of(batch, chunk)
    offs = batch.offsets.astype(np.int64)
    nonempty = offs[1:] > offs[:-1]
    first, last = offs[:-1] // chunk, (offs[1:] - 1) // chunk
    every = {(f, c) for f in np.flatnonzero(nonempty).tolist() for c in range(int(first[f]), int(last[f]) + 1)}
    gate0, evw0 = H.gates_after_adaptation(sc, np.zeros(len(a["kw_unknown"]), np.uint8), 0)
    touched = (a["gate_open"] != gate0) | (a["event_everywhere"] != evw0)
    assert touched.any() and not gskip.any()
    # the device's items per group, gathered through its list entries
    dev_items = {g: np.concatenate([items[int(s):int(s) + int(m)] for _, s, m, _ in ent[ent[:, 0] == g]])
                 for g in set(ent[:, 0].tolist())}
    dense = set(dent[:, 0].tolist())
    dev_counts = np.zeros(G, dtype=np.uint64)
    dev_tri = [tri[~touched[tri[:, 0]]]]
    opened = 0
    for g in range(G):
        ref = rows(tri[tri[:, 0] == g][:, 1:])
        if not touched[g]:
            dev_counts[g] = counts[g]      # (check_work_lists compares its items with the reference's)
            continue
        full = bool(a["gate_open"][g] and a["event_everywhere"][g])
        opened += full
        if g in dense:
            # a touched group takes the dense pass over every chunk: its count is known only
            # where it must hold every chunk of every non-empty file
            assert (full or not dense_full) and g not in dev_items, g
            dev_counts[g] = len(every)
            continue
        arr = dev_items.get(g, np.zeros((0, 2), dtype=np.uint32)).astype(np.int64)
        got = rows(arr)
        assert len(got) == len(arr), "group %d: an item twice" % g
        f, c = arr[:, 0], arr[:, 1]
        assert (f < F).all() and nonempty[f].all() and (first[f] <= c).all() and (c <= last[f]).all(), g
        assert ref <= got, (g, sorted(ref - got)[:4])
        if full:
            assert got == every, g
        dev_counts[g] = len(arr)
        dev_tri.append(np.column_stack([np.full(len(arr), g), arr]).astype(tri.dtype))
    assert opened > 0
    # layout and tiling of the device's lists from its own counts; untouched groups' items exact
    kind, tot = H.check_work_lists(lists, np.concatenate(dev_tri), dev_counts, n, S.default_items_cap(n))
    assert (st["k2_items"], st["k2_launches"], st["k2_dense_entries"], st["groups_skipped"]) == (
        tot["items"], tot["entries"], tot["dense_entries"], tot["skipped"])
    for g in dense:
        assert kind[g] == S.GROUP_DENSE
    # K2's records
    assert dev["count"] <= dev["cand_cap"]
    got_tri = sc.expand_candidates(batch, dev["records"])
    group = np.array([sc.rule_group(r) for r in range(len(sc.Rules))])
    assert (group >= 0).all()
    as_set = lambda t: set(map(tuple, np.asarray(t, dtype=np.int64).reshape(-1, 3).tolist()))
    untouched_rule = ~touched[group]
    assert as_set(got_tri[untouched_rule[got_tri[:, 1]]]) == as_set(cand_ref[untouched_rule[cand_ref[:, 1]]])
    missing = as_set(cand_ref) - as_set(got_tri)
    assert not missing, sorted(missing)[:4]
    if mixed:
        assert untouched_rule[cand_ref[:, 1]].any() and (~untouched_rule[cand_ref[:, 1]]).any()
    wrote = (dev["flags"] & 4) != 0
    assert wrote.any() and np.array_equal(dev["kw"][wrote], kw_dev[wrote])
