"""Files as spans of a device buffer on the device: binary_gate_kernel (utils.IsBinary per
span, any alignment, nothing outside the buffer read), gather_kernel (the kept spans into
the lane buffer in the stage's place; the needed files into the pinned mirror at their
compacted offsets) and the pipeline around them, through the raw ABI and
GpuContext.scan_spans / submit_spans / SecretAnalyzer.AnalyzeTensor.

The cases and references are those of tests/test_device_spans.py
(tests/device_spans_common.py): the kept mask against trivy_amd.analyzer.IsBinary over the
host bytes, the result bytes against tsg_scan_batch's for a Batch of the kept files.  Every
scan runs with the knob device_poison on and with the matching line in the gaps between the
spans.  Each test runs one context and small inputs."""
import numpy as np
import pytest

from tests.device_input_common import SEG
from tests import device_spans_common as X
from trivy_amd import secret as S

pytestmark = pytest.mark.gpu

GPU = True


@pytest.fixture(scope="module")
def builtin():
    return S.NewScanner(None)


@pytest.fixture
def poisoned(knob):
    knob("device_poison", 1)


@pytest.fixture
def ctx(builtin):
    c = S.GpuContext(builtin, 0, adapt_mib=0xFFFFFFFF)
    yield c
    c.close()


def test_gate_edges(ctx, poisoned):
    """The tensor is a slice with storage offset 7 of a zero-filled allocation; every gap is
    zero too, so a gate that reads a byte outside a span drops a text file."""
    lay = X.gate_layout()
    dev = X.Dev(lay.buf, GPU, skew=7)
    assert dev.tensor.data_ptr() % 16 == 7
    kept, _, st, _, _ = X.check_scan(ctx, lay, dev)
    assert 0 < st["files_dropped"] < st["files_in"]
    assert not kept[1] and kept[2]  # the control byte at index 299 / at index 300
    assert st["gate_ms"] > 0 and st["wait_ms"] >= st["gate_ms"]


@pytest.mark.parametrize("kind", ["descending", "shuffled", "adjacent", "big file", "alignments"])
def test_gather_edges(ctx, poisoned, kind):
    lay = {"descending": lambda: X.order_layout("descending"), "shuffled": lambda: X.order_layout("shuffled"),
           "adjacent": X.adjacency_layout, "big file": X.big_layout, "alignments": X.alignment_layout}[kind]()
    dev = X.Dev(lay.buf, GPU, skew=3, fill=X.POISON)
    kept, b, st, di, _ = X.check_scan(ctx, lay, dev)
    assert di["fetched_files"] > 0 and st["gather_ms"] > 0 and ctx.stats()["h2d_ms"] > 0
    if kind == "big file":
        _, segs = ctx.device_mirror()
        assert len(segs) >= 6 and st["bytes_kept"] > 4 * SEG
    if kind == "alignments":
        assert kept.all() and di["fetched_files"] == 256


def test_every_file_needed_is_fetched_as_segments(poisoned):
    sc, lay = X.hostonly_layout()
    c = S.GpuContext(sc, 0, adapt_mib=0xFFFFFFFF)
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


def test_degenerate_batches(ctx, poisoned):
    files = [b"\x7fELF" + X.text(100, k) for k in range(5)] + [b"\x00" * 20]
    lay = X.Layout(files)
    dev = X.Dev(lay.buf, GPU)
    kept, b, st, di, _ = X.check_scan(ctx, lay, dev)
    assert not kept.any() and b.nfiles == 0 and st["bytes_kept"] == 0 and di["fetched_bytes"] == 0
    assert st["gather_ms"] == 0  # no launch over zero bytes
    none = X.Layout([], tail=16)
    res, kept = ctx.scan_spans(X.Dev(none.buf, GPU).tensor, [], [], [])
    assert res == [] and len(kept) == 0
    lay = X.Layout([b"", b""])  # only empty files: nothing to gather or fetch
    X.check_scan(ctx, lay, X.Dev(lay.buf, GPU))
    lay = X.order_layout("descending")  # the context still scans
    X.check_scan(ctx, lay, X.Dev(lay.buf, GPU))


def test_tar_shape(ctx, poisoned):
    st = X.case_tar(ctx, GPU)
    assert st["gate_ms"] > 0 and st["gather_ms"] > 0


def test_stats_sum_over_batches(ctx, poisoned):
    lays = [X.order_layout("shuffled"), X.adjacency_layout()]
    for lay in lays:
        X.check_scan(ctx, lay, X.Dev(lay.buf, GPU))
    st = ctx.device_spans_stats()
    assert st["batches"] == 4  # (check_scan scans twice: the raw call and the wrapper)
    assert st["sum_files_in"] == 2 * sum(len(l.contents) for l in lays)
    assert st["sum_files_kept"] + st["sum_files_dropped"] == st["sum_files_in"]
    assert st["sum_bytes_kept"] == 2 * sum(int(l.lengths[~l.binary()].sum()) for l in lays)
    assert st["gate_ms"] > 0 and st["gather_ms"] > 0 and st["wait_ms"] >= st["gate_ms"]
    assert st["sum_gate_ms"] > st["gate_ms"] and st["sum_gather_ms"] > st["gather_ms"]
    assert ctx.device_input_stats()["batches"] == 4
    assert ctx.device_input_stats()["sum_stage_ms"] == pytest.approx(st["sum_gather_ms"])


def test_two_submitters(ctx, poisoned):
    X.case_two_submitters(ctx, GPU)


def test_device_tensor_checks(ctx):
    """A host tensor on a device context, and a bad span, raise before any native call."""
    lay = X.order_layout("descending")
    host = X.Dev(lay.buf, False).tensor
    with pytest.raises(ValueError):
        ctx.scan_spans(host, lay.starts, lay.lengths, lay.paths)
    dev = X.Dev(lay.buf, GPU)
    st = lay.starts.copy()
    st[0] = dev.n
    with pytest.raises(ValueError):
        ctx.submit_spans(dev.tensor, st, lay.lengths, lay.paths)
    assert ctx.pending() == 0 and ctx.device_spans_stats()["batches"] == 0
