"""Harnesses shared by the device tests: one batch on a fresh context, compared exactly with
the CPU references.  They were the private helpers of tests/test_gpu_configs.py,
tests/test_gpu_k2_paths.py and tests/test_gpu_k2_records.py, which import them from here, as
does tests/test_gpu_grid_rounds.py (the same comparisons under the knob grid_cap)."""
import functools

import pytest

from tests import helpers as H
from trivy_amd import _native as N
from trivy_amd import configs
from trivy_amd import corpus
from trivy_amd import secret as S

NEVER = 0xFFFFFFFF


# ---- K1 (+ K1X) bits and events
def k1_vs_reference(sc, b, chunks=(64, 256)):
    """K1 (+ K1X) keyword bits and chunk events of batch b == k1_reference, on a fresh context
    per chunk size.  Returns the stats of the last one."""
    import numpy as np
    for chunk in chunks:
        ctx = S.GpuContext(sc, 0, chunk_bytes=chunk, adapt_mib=0xFFFFFFFF)
        ctx.upload(b)
        ctx.kernels()
        kw, ev = ctx.k1_output(chunk)
        st = ctx.stats()
        ctx.close()
        rkw, rev = sc.k1_reference(b, chunk)
        assert np.array_equal(kw, rkw)
        assert np.array_equal(ev, rev)
    return st


# ---- the item passes' work lists
@functools.lru_cache(maxsize=None)
def builtin_scanner():
    return S.NewScanner(None)


@functools.lru_cache(maxsize=None)
def item_case(chunk, name):
    """(batch, reference triples, counts, chunks, exact findings) of one item-pass input,
    computed once and shared by the tests that need it."""
    sc = builtin_scanner()
    batch = H.item_inputs(sc, chunk)[name]
    tri, counts = sc.emulate_items(batch, chunk, 16)
    return batch, tri, counts, H.nchunks_of(batch, chunk), sc.ScanBatch(batch, nthreads=16)


@functools.lru_cache(maxsize=None)
def dense_case(chunk, total):
    sc = builtin_scanner()
    batch, plants = H.dense_batch(chunk, total)
    tri, counts = sc.emulate_items(batch, chunk, 16)
    return batch, plants, tri, counts, H.nchunks_of(batch, chunk), sc.ScanBatch(batch, nthreads=16)


def run_lists(sc, batch, chunk, **kw):
    """kernels() + work lists + stats + findings of one batch on a fresh context."""
    ctx = S.GpuContext(sc, 0, chunk_bytes=chunk, adapt_mib=NEVER, **kw)
    ctx.upload(batch)
    ctx.kernels()
    st = ctx.stats()
    lists = ctx.batch_items()
    got = ctx.scan()
    st2 = ctx.stats()
    ctx.close()
    return lists, st, got, st2


def check_stats(st, tot):
    got = (st["k2_items"], st["k2_launches"], st["k2_dense_entries"], st["groups_skipped"])
    assert got == (tot["items"], tot["entries"], tot["dense_entries"], tot["skipped"]), (got, tot)


# ---- K2's candidate records
@functools.lru_cache(maxsize=None)
def k2_scanner_for(rules, kernel):
    """A scanner per rule set and list kernel: group_table_kib = 32 at compile time gives
    smaller DFAs, for which the occupancy API picks k2_kernel instead of k2_kernel_rich."""
    if kernel == "small tables":
        N.knob("group_table_kib", 32)
    try:
        if rules == "k2":
            return H.k2_scanner()
        if rules == "user":
            return S.NewScanner(S.config_from_dict(configs.user_rules_doc(1000, 4)))
        if rules in ("assert", "group64"):   # the rule sets of tests/cover_common.py
            from tests import cover_common as CC
            return S.NewScanner(S.config_from_dict(CC.assert_doc() if rules == "assert" else CC.group64_doc()))
        return S.NewScanner(None)
    finally:
        N.knob("group_table_kib", None)


def k2_input(sc, key):
    """The batch of a named input of the record tests."""
    name, args = key[0], key[1:]
    if name == "mask":
        return H.word_mask_batch(*args)[0]
    if name == "tail":
        return H.tail_batch(*args)[0]
    if name == "entry":
        return H.entry_shape_batch(*args)[0]
    if name == "dense":
        return H.dense_batch(*args)[0]
    if name == "items":
        return H.item_inputs(sc, args[0])[args[1]]
    if name == "cover":   # a committed batch of tests/golden/candidate_cover/
        from tests import cover_common as CC
        return CC.fixture_batch(args[0]).batch
    if name == "hex lines":
        return H.hex_lines_batch(*args)
    return corpus.make_corpus(*args[:1], seed=args[1], plants_per_mib=300)[0]


@functools.lru_cache(maxsize=None)
def k2_exact(rules, key):
    """(batch, exact CPU findings) of a named input, computed once.  The findings do not
    depend on the plan, so both list kernels share them."""
    sc = k2_scanner_for(rules, "default")
    batch = k2_input(sc, key)
    return batch, sc.ScanBatch(batch, nthreads=16)


def run_records(sc, batch, want, chunk, kernel="default", words=True, ext_cap=0, cand_capacity=0, rich=None,
                items_cap=None, dev_out=None):
    """kernels() -> batch_candidates() -> check_candidates against emulate_candidates with the
    context's settings, then scan() against the exact path.  rich: the list kernel that must
    have run (default: k2_kernel_rich unless the scanner was compiled with small tables;
    "either": a plan whose table sizes leave the choice to the device's occupancy query);
    items_cap: the k2_items_cap knob the caller has set (groups may then be skipped);
    dev_out: a dict that receives what batch_candidates() read back.
    Returns (stats of kernels(), reference records, reference triples)."""
    ctx = S.GpuContext(sc, 0, chunk_bytes=chunk, ext_cap=ext_cap, cand_capacity=cand_capacity, adapt_mib=NEVER)
    try:
        ctx.upload(batch)
        ctx.kernels()
        st = ctx.stats()
        dev = ctx.batch_candidates()
        n = H.nchunks_of(batch, chunk)
        items_cap = S.default_items_cap(n) if items_cap is None else items_cap
        ref = sc.emulate_candidates(batch, chunk, ext_cap or S.DEFAULT_EXT_CAP, word_recs=words, items_cap=items_cap)
        _, counts = sc.emulate_items(batch, chunk, 16)
        skipped = S.layout_reference(counts, n, items_cap)[1]["skipped"]
        assert dev["cand_cap"] == (cand_capacity or S.DEFAULT_CAND_CAPACITY)
        nref, ntri = H.check_candidates(dev, ref, batch, sc, chunk, skipped=skipped > 0)
        assert st["candidates"] == nref and st["groups_skipped"] == skipped
        assert st["overflow"] == (1 if nref > dev["cand_cap"] else 0)
        if rich != "either":
            assert st["k2_rich"] == ((0 if kernel == "small tables" else 1) if rich is None else rich), st["k2_rich"]
        if dev_out is not None:
            dev_out.update(dev)
        got = ctx.scan()
        with pytest.raises(N.NativeError):  # something was submitted since kernels()
            ctx.batch_candidates()
    finally:
        ctx.close()
    assert got == want
    return st, nref, ntri
