"""Files as spans of a device buffer (tsg_device_spans_submit / tsg_scan_device_spans,
GpuContext.scan_spans, SecretAnalyzer.AnalyzeTensor) on an emulated context.

Under TSG_CTX_EMULATE the base is a host pointer, the gate is the C++ IsBinary of the other
ingest paths and both gathers are memcpy of the same segment lists the kernels take, so the
argument checks, the kept list, the compacted offsets and paths, the segment builder, the
fetch and the stats run here exactly as on a device.  Every scan but the argument test runs
with the knob device_poison on, and the gaps between the spans hold the same line: a copied
gap byte, or a resolver read of an unfetched byte, is a wrong finding."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.conftest import ROOT
from tests.device_input_common import SEG, raw_scan_batch, raw_scan_device
from tests import device_spans_common as X
from trivy_amd import _native as N
from trivy_amd import secret as S

GPU = False


@pytest.fixture(scope="module")
def builtin():
    return S.NewScanner(None)


@pytest.fixture
def poisoned(knob):
    knob("device_poison", 1)


@pytest.fixture
def ctx(builtin):
    c = S.GpuContext(builtin, 0, emulate=True)
    yield c
    c.close()


def test_gate_edges(ctx, poisoned):
    lay = X.gate_layout()
    dev = X.Dev(lay.buf, GPU, skew=7)
    kept, _, st, _, _ = X.check_scan(ctx, lay, dev)
    assert 0 < st["files_dropped"] < st["files_in"]
    assert not kept[1] and kept[2]  # the control byte at index 299 / at index 300


@pytest.mark.parametrize("kind", ["descending", "shuffled", "adjacent", "big file", "alignments"])
def test_gather_edges(ctx, poisoned, kind):
    lay = {"descending": lambda: X.order_layout("descending"), "shuffled": lambda: X.order_layout("shuffled"),
           "adjacent": X.adjacency_layout, "big file": X.big_layout, "alignments": X.alignment_layout}[kind]()
    dev = X.Dev(lay.buf, GPU, skew=3, fill=X.POISON)
    kept, b, st, di, _ = X.check_scan(ctx, lay, dev)
    assert di["fetched_files"] > 0
    if kind == "big file":
        _, segs = ctx.device_mirror()
        assert len(segs) >= 6 and st["bytes_kept"] > 4 * SEG
    if kind == "alignments":
        assert kept.all() and di["fetched_files"] == 256


def test_every_file_needed_is_fetched_as_segments(poisoned):
    sc, lay = X.hostonly_layout()
    c = S.GpuContext(sc, 0, emulate=True)
    try:
        kept, b, st, di, res = X.check_scan(c, lay, X.Dev(lay.buf, GPU), wrapper=False)
        assert di["whole_batch_copy"] == 0
        assert di["fetched_files"] == int(kept.sum()) and di["fetched_bytes"] == st["bytes_kept"]
        assert sum(1 for x in res if any(f["RuleID"] == "many-words" for f in x["Findings"] or [])) >= 10
    finally:
        c.close()


def test_gate_off_equals_scan_tensor(ctx, poisoned):
    lay = X.order_layout("shuffled")
    assert lay.binary().any()
    dev = X.Dev(lay.buf, GPU)
    kept, b, st, _, _ = X.check_scan(ctx, lay, dev, gate=False)
    assert kept.all() and st["gate_ms"] == 0 and st["wait_ms"] == 0 and st["files_dropped"] == 0
    res, _ = ctx.scan_spans(dev.tensor, lay.starts, lay.lengths, lay.paths, binary_gate=False)
    compact = X.Dev(np.array(b.data[:int(b.offsets[-1])]), GPU)
    assert res == ctx.scan_tensor(compact.tensor, b.offsets, lay.paths)
    got, _ = X.raw_scan_spans(ctx, dev, lay.starts, lay.lengths, lay.paths, 0)
    assert got == raw_scan_device(ctx, b)


def test_degenerate_batches(ctx, poisoned):
    files = [b"\x7fELF" + X.text(100, k) for k in range(5)] + [b"\x00" * 20]
    lay = X.Layout(files)
    dev = X.Dev(lay.buf, GPU)
    kept, b, st, di, _ = X.check_scan(ctx, lay, dev)
    assert not kept.any() and b.nfiles == 0 and st["bytes_kept"] == 0 and di["fetched_bytes"] == 0
    assert ctx.scan_spans(dev.tensor, lay.starts, lay.lengths, lay.paths)[0] == []
    none = X.Layout([], tail=16)
    res, kept = ctx.scan_spans(X.Dev(none.buf, GPU).tensor, [], [], [])
    assert res == [] and len(kept) == 0
    out = C.c_void_p()
    N.check(N.lib().tsg_scan_device_spans(ctx.handle, None, 0, None, None, 0, None, None, X.GATE, None, C.byref(out)))
    assert X.result_bytes(out) == raw_scan_batch(ctx, S.Batch.from_args([]))
    lay = X.Layout([b"", b""])  # only empty files: nothing to gate, gather or fetch
    X.check_scan(ctx, lay, X.Dev(lay.buf, GPU))
    lay = X.order_layout("descending")  # the context still scans
    X.check_scan(ctx, lay, X.Dev(lay.buf, GPU))


def test_tar_shape(ctx, poisoned):
    X.case_tar(ctx, GPU)


def test_argument_errors(ctx):
    L = N.lib()
    lay = X.order_layout("descending")
    dev = X.Dev(lay.buf, GPU)
    blob, poffs = X.path_arrays(lay.paths)
    n = len(lay.paths)
    out, t = C.c_void_p(), C.c_uint64()
    kept = np.zeros(n, dtype=np.uint8)
    kp = kept.ctypes.data_as(C.POINTER(C.c_uint8))

    def both(h, base, nbytes, starts, lengths, flags=X.GATE, outp=True):
        a = (h, C.c_void_p(base), nbytes, X.u64p(starts), X.u64p(lengths), n, C.c_void_p(blob.ctypes.data),
             X.u64p(poffs), flags, kp)
        return (L.tsg_scan_device_spans(*a, C.byref(out) if outp else None),
                L.tsg_device_spans_submit(*a, C.byref(t) if outp else None))
    ok = (lay.starts, lay.lengths)
    assert both(None, dev.ptr, dev.n, *ok) == (N.TSG_ERR_ARG,) * 2           # NULL context
    assert L.tsg_ctx_get_device_spans_stats(None, None) == N.TSG_ERR_ARG
    assert L.tsg_ctx_get_device_spans_stats(ctx.handle, None) == N.TSG_ERR_ARG
    h = ctx.handle
    assert both(h, dev.ptr, dev.n, *ok, outp=False) == (N.TSG_ERR_ARG,) * 2  # NULL out pointer
    assert both(h, None, dev.n, *ok) == (N.TSG_ERR_ARG,) * 2                 # NULL base, non-empty spans
    for flags in (2, 3, 0x80000000):
        assert both(h, dev.ptr, dev.n, *ok, flags=flags) == (N.TSG_ERR_ARG,) * 2
    last = int(np.argmax(lay.starts))
    for k, start, length in ((last, int(lay.starts[last]), int(dev.n - lay.starts[last]) + 1),  # one byte past the end
                             (0, dev.n + 1, 0),                                              # starts past the end
                             (1, dev.n, 1),
                             (2, 2 ** 64 - 8, 16),                                           # start + length overflows
                             (3, 16, 2 ** 64 - 8)):
        st, ln = lay.starts.copy(), lay.lengths.copy()
        st[k], ln[k] = start, length
        assert both(h, dev.ptr, dev.n, st, ln) == (N.TSG_ERR_ARG,) * 2, (k, start, length)
    assert both(h, dev.ptr, int(lay.starts[last]), *ok) == (N.TSG_ERR_ARG,) * 2  # base_bytes cuts the last span
    assert ctx.pending() == 0 and ctx.device_spans_stats()["batches"] == 0
    # Python raises before any native call
    paths = lay.paths
    for bad, exc in ((dev.tensor.to(torch.int8), TypeError), (lay.buf, TypeError), (dev.tensor.to(torch.float32), TypeError),
                     (dev.tensor[::2], ValueError), (dev.tensor.reshape(1, -1), ValueError)):
        with pytest.raises(exc):
            ctx.scan_spans(bad, lay.starts, lay.lengths, paths)
        with pytest.raises(exc):
            ctx.submit_spans(bad, lay.starts, lay.lengths, paths)
    st = lay.starts.copy()
    st[0] = dev.n
    for a in ((st, lay.lengths, paths), (lay.starts[:-1], lay.lengths, paths), (lay.starts, lay.lengths, paths[:-1]),
              (lay.starts.astype(np.int64) * -1, lay.lengths, paths), (lay.starts.astype(np.float64), lay.lengths, paths),
              (lay.starts, lay.lengths.reshape(1, -1), paths)):
        with pytest.raises(ValueError):
            ctx.scan_spans(dev.tensor, *a)
        with pytest.raises(ValueError):
            ctx.submit_spans(dev.tensor, *a)
    with pytest.raises(ValueError):
        ctx.scan_spans(dev.tensor[:int(lay.starts[last])], lay.starts, lay.lengths, paths)
    assert ctx.pending() == 0 and ctx.device_spans_stats()["batches"] == 0 and not ctx._tensors
    X.check_scan(ctx, lay, dev, mirror=False)  # the context still scans


def test_stats_binding_follows_header():
    src = open(os.path.join(ROOT, "include", "trivy_secret.h")).read()
    body = re.search(r"typedef struct tsg_device_spans_stats \{(.*?)\} tsg_device_spans_stats;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"double": C.c_double, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        fields += [(name, ctype[words[0]]) for name in words[1:]]
    assert fields == list(N.DeviceSpansStats._fields_)
    assert {"gate_ms", "gather_ms", "wait_ms", "files_in", "files_kept", "files_dropped", "bytes_in",
            "bytes_kept"} <= {n for n, _ in fields}
    assert re.search(r"#define\s+TSG_SPANS_BINARY_GATE\s+1u", src) and N.TSG_SPANS_BINARY_GATE == 1


def test_stats_sum_over_batches(ctx, poisoned):
    lays = [X.order_layout("shuffled"), X.adjacency_layout()]
    for lay in lays:
        X.check_scan(ctx, lay, X.Dev(lay.buf, GPU))
    st = ctx.device_spans_stats()
    assert st["batches"] == 4  # (check_scan scans twice: the raw call and the wrapper)
    assert st["sum_files_in"] == 2 * sum(len(l.contents) for l in lays)
    assert st["sum_files_kept"] + st["sum_files_dropped"] == st["sum_files_in"]
    assert st["sum_bytes_kept"] == 2 * sum(int(l.lengths[~l.binary()].sum()) for l in lays)
    assert st["sum_gate_ms"] >= st["gate_ms"] >= 0 and st["sum_wait_ms"] >= st["wait_ms"] >= st["gate_ms"]
    assert st["gather_ms"] == 0  # nothing is staged by a kernel in the emulation
    assert ctx.device_input_stats()["batches"] == 4


def test_two_submitters(ctx, poisoned):
    X.case_two_submitters(ctx, GPU)
