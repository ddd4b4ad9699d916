"""Device-resident input (tsg_device_submit / tsg_scan_device) on an emulated context.

Under TSG_CTX_EMULATE d_data is an ordinary host pointer and the fetch is a memcpy of the
segment list, so the mirror, the shared need predicate (plan.hpp file_needs_scan), the
segment builder and the stats run here exactly as on a device.  Every scan runs with the
knob device_poison on: the slot's data area is filled with a line the builtin rules match
before the fetch, so a resolver read of a byte that was not fetched is a wrong finding."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from trivy_amd import _native as N
from trivy_amd import corpus
from trivy_amd import secret as S
from tests.device_input_common import (big_file_batch, check_mirror, files_with_findings, hostonly_case,
                                       raw_scan_batch, raw_scan_device, result_bytes)


@pytest.fixture(scope="module")
def builtin():
    return S.NewScanner(None)


@pytest.fixture(scope="module")
def seeded():
    """768 KiB of the seeded corpus, seed 1: 73 files, 30 of them with findings."""
    return corpus.make_corpus(768 << 10, seed=1)[0]


@pytest.fixture(scope="module")
def hostonly():
    return hostonly_case()


@pytest.fixture
def poisoned(knob):
    knob("device_poison", 1)


def _batches(seeded):
    return {"seeded": seeded,
            "small files": H.small_files_batch(3),
            "fold runes": corpus.fold_runes_batch(11, nbytes=256 << 10, plants=150, frac=0.2),
            "big file": big_file_batch()}


@pytest.mark.parametrize("name", ["seeded", "small files", "fold runes", "big file"])
def test_scan_device_equals_scan_batch(builtin, seeded, poisoned, name):
    """Result bytes of tsg_scan_device == tsg_scan_batch's on the same context; the fetch
    wrote whole needed files and nothing else; every file with findings was fetched."""
    b = _batches(seeded)[name]
    ctx = S.GpuContext(builtin, 0, emulate=True)
    try:
        want = raw_scan_batch(ctx, b)
        got = raw_scan_device(ctx, b)
        assert got == want
        st = ctx.device_input_stats()
        assert st["whole_batch_copy"] == 0 and st["batches"] == 1 and st["sum_bytes"] == int(b.offsets[-1])
        full = check_mirror(ctx, b, st)
        found = files_with_findings(want, builtin, b)
        assert found > 0 and st["fetched_files"] >= found
        res = S.decode_results(want, [b.path(i) for i in range(b.nfiles)], builtin.Rules)
        sizes = np.diff(b.offsets.astype(np.int64))
        assert all(f in full for f in range(b.nfiles) if res[f]["Findings"] and sizes[f])
    finally:
        ctx.close()


def test_clean_corpus_fetches_a_part(builtin, seeded, poisoned):
    """On the seeded corpus (768 KiB, seed 1, 73 files) the emulation fetches 44 files: the
    30 with findings and 14 whose candidates the resolver rejects; 29 never cross."""
    ctx = S.GpuContext(builtin, 0, emulate=True)
    try:
        want = raw_scan_batch(ctx, seeded)
        assert raw_scan_device(ctx, seeded) == want
        st = ctx.device_input_stats()
        found = files_with_findings(want, builtin, seeded)
        assert seeded.nfiles == 73 and found == 30
        assert found <= st["fetched_files"] == 44 < seeded.nfiles
        assert st["fetched_bytes"] < int(seeded.offsets[-1])
    finally:
        ctx.close()


def test_hostonly_rules_copy_the_whole_batch(hostonly, poisoned):
    sc, b = hostonly
    ctx = S.GpuContext(sc, 0, emulate=True)
    try:
        want = raw_scan_batch(ctx, b)
        assert raw_scan_device(ctx, b) == want
        st = ctx.device_input_stats()
        assert st["whole_batch_copy"] == 1
        assert st["fetched_files"] == b.nfiles and st["fetched_bytes"] == int(b.offsets[-1])
        mirror, segs = ctx.device_mirror()
        assert segs.tolist() == [[0, int(b.offsets[-1])]]
        assert np.array_equal(mirror, b.data[:int(b.offsets[-1])])
        res = S.decode_results(want, [b.path(i) for i in range(b.nfiles)], sc.Rules)
        assert sum(1 for x in res if any(f["RuleID"] == "many-words" for f in x["Findings"] or [])) >= 10
    finally:
        ctx.close()


@pytest.mark.parametrize("cc", [1, 63])
def test_candidate_overflow_fetches_flagged_files(builtin, seeded, poisoned, cc):
    """A candidate capacity the batch overflows (as tests/test_k2_paths.py): the files whose
    records were dropped are flagged, fetched whole and resolved whole."""
    base = S.GpuContext(builtin, 0, emulate=True)
    ctx = S.GpuContext(builtin, 0, emulate=True, cand_capacity=cc)
    try:
        want = raw_scan_batch(base, seeded)
        assert raw_scan_batch(ctx, seeded) == want
        assert raw_scan_device(ctx, seeded) == want
        assert ctx.stats()["overflow"] == 1
        st = ctx.device_input_stats()
        assert st["whole_batch_copy"] == 0
        full = check_mirror(ctx, seeded, st)
        assert raw_scan_device(base, seeded) == want
        assert len(full) >= len(check_mirror(base, seeded, base.device_input_stats()))
    finally:
        base.close()
        ctx.close()


def test_tickets_collected_in_reverse(builtin, seeded, poisoned):
    """Three device submissions from three buffers, collected last first."""
    batches = [seeded, big_file_batch(), H.small_files_batch(3)]
    ctx = S.GpuContext(builtin, 0, emulate=True)
    try:
        want = [raw_scan_batch(ctx, b) for b in batches]
        datas = [np.array(b.data[:int(b.offsets[-1])]) for b in batches]
        tickets = []
        for b, d in zip(batches, datas):
            _, offs, nfiles, paths, poffs = b.ptrs()
            t = C.c_uint64()
            N.check(N.lib().tsg_device_submit(ctx.handle, C.c_void_p(d.ctypes.data), offs, nfiles, paths, poffs,
                                              C.byref(t)))
            tickets.append(t.value)
        assert ctx.pending() == 3
        for k in (2, 1, 0):
            out = C.c_void_p()
            N.check(N.lib().tsg_batch_collect(ctx.handle, tickets[k], C.byref(out)))
            assert result_bytes(out) == want[k], k
        st = ctx.device_input_stats()
        assert st["batches"] == 3 and st["sum_bytes"] == sum(int(b.offsets[-1]) for b in batches)
        assert ctx.stats()["h2d_ms"] == st["stage_ms"] == 0  # nothing is staged in the emulation
    finally:
        ctx.close()


def test_empty_batches(builtin, poisoned):
    ctx = S.GpuContext(builtin, 0, emulate=True)
    try:
        for args in ([], [S.ScanArgs("a", b""), S.ScanArgs("b", b"")]):
            b = S.Batch.from_args(args)
            _, offs, nfiles, paths, poffs = b.ptrs()
            out = C.c_void_p()
            N.check(N.lib().tsg_scan_device(ctx.handle, None, offs, nfiles, paths, poffs, C.byref(out)))
            assert result_bytes(out) == raw_scan_batch(ctx, b)
            assert ctx.device_input_stats()["fetched_bytes"] == 0
    finally:
        ctx.close()


def test_argument_errors(builtin, seeded):
    L = N.lib()
    _, offs, nfiles, paths, poffs = seeded.ptrs()
    data = C.c_void_p(seeded.data.ctypes.data)
    out, t = C.c_void_p(), C.c_uint64()
    assert L.tsg_scan_device(None, data, offs, nfiles, paths, poffs, C.byref(out)) == N.TSG_ERR_ARG
    assert L.tsg_device_submit(None, data, offs, nfiles, paths, poffs, C.byref(t)) == N.TSG_ERR_ARG
    assert L.tsg_ctx_get_device_input_stats(None, None) == N.TSG_ERR_ARG
    ctx = S.GpuContext(builtin, 0, emulate=True)
    try:
        h = ctx.handle
        assert L.tsg_scan_device(h, None, offs, nfiles, paths, poffs, C.byref(out)) == N.TSG_ERR_ARG
        assert L.tsg_device_submit(h, None, offs, nfiles, paths, poffs, C.byref(t)) == N.TSG_ERR_ARG
        assert L.tsg_scan_device(h, data, offs, nfiles, paths, poffs, None) == N.TSG_ERR_ARG
        assert L.tsg_device_submit(h, data, offs, nfiles, paths, poffs, None) == N.TSG_ERR_ARG
        bad = seeded.offsets.copy()
        bad[3], bad[4] = bad[4], bad[3]
        assert bad[4] < bad[3]
        badp = bad.ctypes.data_as(C.POINTER(C.c_uint64))
        assert L.tsg_scan_device(h, data, badp, nfiles, paths, poffs, C.byref(out)) == N.TSG_ERR_ARG
        assert L.tsg_device_submit(h, data, badp, nfiles, paths, poffs, C.byref(t)) == N.TSG_ERR_ARG
        assert ctx.pending() == 0
        with pytest.raises(N.NativeError):
            ctx.device_mirror()  # no device-resident batch yet
        # the context still works
        assert raw_scan_device(ctx, seeded) == raw_scan_batch(ctx, seeded)
    finally:
        ctx.close()


def test_stats_binding_follows_header():
    import os
    import re
    from tests.conftest import ROOT
    src = open(os.path.join(ROOT, "include", "trivy_secret.h")).read()
    body = re.search(r"typedef struct tsg_device_input_stats \{(.*?)\} tsg_device_input_stats;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"double": C.c_double, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        fields += [(name, ctype[words[0]]) for name in words[1:]]
    assert fields == list(N.DeviceInputStats._fields_)
    assert {"stage_ms", "fetch_ms", "fetched_files", "fetched_bytes", "whole_batch_copy", "batches", "sum_stage_ms",
            "sum_fetch_ms", "sum_fetched_bytes", "sum_bytes"} == {n for n, _ in fields}


def test_scan_tensor_wrapper(builtin, seeded, poisoned):
    """scan_tensor / submit_tensor on an emulated context take host tensors: findings equal
    scan_batch's, a slice with a storage offset works, the tensor lives until collect, and a
    wrong dtype, layout or device raises before any native call."""
    import torch
    paths = [seeded.path(i) for i in range(seeded.nfiles)]
    total = int(seeded.offsets[-1])
    ctx = S.GpuContext(builtin, 0, emulate=True)
    try:
        want = ctx.scan_batch(seeded)
        whole = torch.zeros(total + 23, dtype=torch.uint8)
        whole[7:7 + total] = torch.from_numpy(np.array(seeded.data[:total]))
        t = whole[7:7 + total]
        assert t.storage_offset() == 7
        assert ctx.scan_tensor(t, seeded.offsets, paths) == want
        ticket = ctx.submit_tensor(t, seeded.offsets, paths)
        assert ctx._tensors[ticket] is t
        del t, whole
        assert ctx.collect(ticket) == want and not ctx._tensors
        t = torch.from_numpy(np.array(seeded.data[:total]))
        n0 = ctx.device_input_stats()["batches"]
        for bad, exc in ((t.to(torch.int8), TypeError), (np.array(seeded.data[:total]), TypeError),
                         (t.to(torch.float32), TypeError), (t[::2], ValueError), (t.reshape(2, -1), ValueError),
                         (t[:10], ValueError)):
            with pytest.raises(exc):
                ctx.scan_tensor(bad, seeded.offsets, paths)
            with pytest.raises(exc):
                ctx.submit_tensor(bad, seeded.offsets, paths)
        with pytest.raises(ValueError):
            ctx.scan_tensor(t, seeded.offsets, paths[:-1])
        with pytest.raises(ValueError):
            ctx.scan_tensor(t, seeded.offsets[::-1].copy(), paths)
        assert ctx.device_input_stats()["batches"] == n0 and ctx.pending() == 0
    finally:
        ctx.close()
