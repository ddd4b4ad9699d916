"""A layer tar in the context's memory (tsg_device_layer_scan, walker.scan_layer_tensor,
GpuContext.tar_marks) on an emulated context.

Under TSG_CTX_EMULATE the tar is a host pointer, the marks are a CPU loop over layer.cpp's
checksum_ok / zero_block and the gathers are memcpy of the same range lists the kernels take,
so the sparse view, the walk over it, the payload rounds, the batch cutting, the assembled
layer and result and the stats run here exactly as on a device.  The cases and references are
tests/device_layer_common.py's."""
import io
import tarfile

import pytest

from tests import device_layer_common as X
from trivy_amd import analyzer as A
from trivy_amd import secret as S
from trivy_amd import walker as W

GPU = False


@pytest.fixture(scope="module")
def builtin():
    return S.NewScanner(None)


@pytest.fixture
def ctx(builtin):
    c = S.GpuContext(builtin, 0, emulate=True)
    yield c
    c.close()


def test_reference_marks_on_a_real_tar():
    """The restated rule agrees with tarfile on what is a header."""
    tar = X.layer_bytes(tarfile.GNU_FORMAT)
    hdr, zero = X.ref_marks(tar)
    with tarfile.open(fileobj=io.BytesIO(tar)) as tf:
        offs = [m.offset // 512 for m in tf.getmembers()]
    assert all(hdr[o] for o in offs) and zero[-1] and not (hdr & zero).any()


def test_marks_edge_blocks(ctx):
    blocks, want = X.edge_blocks()
    tar = X.member(b"first.env", X.body()) + b"".join(blocks) + X.member(b"last.env", X.body())
    hdr, zero = X.check_marks(ctx, tar, GPU)
    assert hdr[2:2 + len(blocks)].tolist() == want
    assert zero[2:2 + len(blocks)].tolist() == [b == X.ZERO_BLOCK for b in blocks]


@pytest.mark.parametrize("nblocks", [0, 1, 63, 64, 65, 4097])
def test_marks_block_counts(ctx, nblocks):
    hdr, zero = X.check_marks(ctx, X.mixed_blocks(nblocks, nblocks), GPU)
    assert len(hdr) == len(zero) == nblocks
    if nblocks > 60:
        assert hdr.any() and zero.any() and not (hdr | zero).all()


def test_marks_tails(ctx):
    """tar_len 0, 511, 512 and 512 k + 1 .. + 511: the tail under 512 bytes is no block, also
    where it holds the start of a header."""
    whole = X.mixed_blocks(3, 5) + X.header(b"tail.env")
    for n in [0, 1, 511, 512, 513, 1023, 1024] + list(range(3 * 512 + 1, 4 * 512)) + [4 * 512]:
        hdr, _ = X.check_marks(ctx, whole[:n], GPU)
        assert len(hdr) == n // 512
    assert hdr[3]


@pytest.mark.parametrize("skew", [0, 1, 7, 15])
def test_marks_alignment_and_guards(ctx, skew):
    tar = X.mixed_blocks(130, 9)
    a, _ = X.check_marks(ctx, tar, GPU, skew=skew, fill=b"\xff")
    b, _ = X.check_marks(ctx, tar, GPU, skew=skew, fill=b"\0")
    assert a.tolist() == b.tolist()


@pytest.mark.parametrize("fmt", [tarfile.PAX_FORMAT, tarfile.GNU_FORMAT])
@pytest.mark.parametrize("skips", [False, True])
def test_layer_equals_host_call(ctx, fmt, skips):
    tar = X.layer_bytes(fmt)
    kw = {"skip_files": ["/app/skipme.txt"], "skip_dirs": ["etc"]} if skips else {}
    (paths, res, opq, wh, walked), st = X.check_layer(ctx, tar, GPU, skew=3, **kw)
    assert ("/app/skipme.txt" in paths) != skips and ("/etc/app.env" in paths) != skips
    assert "/app/" + "d" * 120 + "/long.env" in paths and "/app/bin.dat" not in paths
    assert opq == ["var/"] and wh == ["app/removed.txt"]
    # the long name's extended header: its payload came in a round, and nothing else did
    sizes = X.ext_payload_sizes(tar)
    assert sizes and st["payload_rounds"] >= 1
    assert st["payloads"] == len(sizes) and st["payload_bytes"] == sum(sizes)
    assert st["chain_entries"] + len(sizes) == st["marked_blocks"] and st["span_batches"] == 1


def test_nested_tar(ctx):
    (paths, res, _, _, _), st = X.check_layer(ctx, X.nested_layer(), GPU)
    assert st["chain_entries"] == 3 and st["marked_blocks"] == 3 + 5
    assert paths == ["/a/first.env", "/a/last.env"] and not any("inner" in p for p in paths)
    assert st["payload_rounds"] == 0 and st["payload_bytes"] == 0


def test_pax_size_override(ctx):
    tar = X.pax_size_layer()
    (paths, res, _, _, _), st = X.check_layer(ctx, tar, GPU)
    assert paths == ["/grow.env", "/renamed/short.env", "/after.env"]
    assert st["chain_entries"] == 3 and st["payloads"] >= 2 and st["payload_rounds"] >= 1
    assert all(r["Findings"] for r in res)


@pytest.mark.parametrize("name", sorted(X.malformed_tars()))
def test_malformed(ctx, name):
    assert X.case_malformed(ctx, GPU, name) is not None  # (every one of them is an error)


def test_malformed_errors_are_the_walkers():
    """The inputs fail as their names say (on the host call, which the device call must equal)."""
    c = S.GpuContext(S.NewScanner(None), 0, emulate=True)
    try:
        errs = {k: X.native_error(W.scan_layer_pipelined, c, v) for k, v in X.malformed_tars().items()}
    finally:
        c.close()
    text = {k: (e[1] if e else None) for k, e in errs.items()}
    assert "unexpected EOF" in text["truncated in a header"]
    assert "unexpected EOF" in text["truncated in a member's data"]
    assert "unexpected EOF" in text["truncated in a PAX payload"]
    assert "unexpected EOF" in text["PAX payload past the end"]
    assert "invalid header" in text["a chain block with a broken checksum"]
    assert "invalid header" in text["a zero block, then a non-zero block"]
    assert "invalid PAX record" in text["a malformed PAX record"]
    assert "invalid size" in text["an invalid size field"]
    assert "invalid PAX size" in text["an invalid PAX size"]


@pytest.mark.parametrize("name", sorted(X.empty_tars()))
def test_empty_archives(ctx, name):
    tar = X.empty_tars()[name]
    want = X.native_error(W.scan_layer_pipelined, ctx, tar)
    if want is not None:  # (under one block: unexpected EOF on both sides)
        assert X.native_error(W.scan_layer_tensor, ctx, X.tensor_of(tar, GPU)) == want
        return
    (paths, _, _, _, _), st = X.check_layer(ctx, tar, GPU)
    assert len(paths) == (1 if b"one.env" in tar else 0)


def test_pieces(ctx, knob):
    X.case_pieces(ctx, GPU, knob)


def test_poisoned_mirror_gives_the_same(ctx, knob):
    knob("device_poison", 1)
    X.check_layer(ctx, X.layer_bytes(), GPU)
    X.check_layer(ctx, X.pax_size_layer(), GPU, skew=5)


def test_two_threads(ctx):
    X.case_two_threads(ctx, GPU)


def test_arguments(ctx):
    X.case_arguments(ctx, GPU)
    with pytest.raises(ValueError):
        W.scan_layer_tensor(ctx, X.tensor_of(X.good_layer(), GPU).reshape(-1, 512)[:2])


def test_stats_sum_over_calls(ctx):
    sts = [X.check_layer(ctx, t, GPU)[1] for t in (X.layer_bytes(), X.nested_layer(), X.pax_size_layer())]
    last = ctx.device_layer_stats()
    assert last["calls"] == 3
    for k in ("tar_bytes", "blocks", "marked_blocks", "chain_entries", "header_bytes", "payloads", "payload_bytes",
              "payload_rounds", "span_batches", "files_scanned", "fetched_bytes", "pcie_bytes"):
        assert last["sum_" + k] == sum(s[k] for s in sts), k
    assert last["sum_mark_ms"] == pytest.approx(sum(s["mark_ms"] for s in sts)) and last["mark_ms"] > 0
    assert 0 < last["pcie_bytes"] and sts[0]["fetched_bytes"] > 0


def test_analyze_layer_tensor(ctx, builtin):
    an = A.SecretAnalyzer(builtin, "")
    tar = X.layer_bytes()
    want = W.analyze_layer_native(an, tar, ctx=ctx, skip_files=["app/skipme.txt"])
    got = W.analyze_layer_tensor(an, X.tensor_of(tar, GPU), ctx, skip_files=["app/skipme.txt"])
    assert got == want and [s["FilePath"] for s in got[0]][:1] == ["/abs/slack.txt"]
