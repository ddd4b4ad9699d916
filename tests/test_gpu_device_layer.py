"""A layer tar in GPU memory on the device: tar_mark_kernel (the header-checksum and
all-zero bit of every 512-byte block, any alignment of the tar, nothing outside it read),
gather_kernel over the marked blocks and the extended-header payloads, and the pipeline
around them, through GpuContext.tar_marks and walker.scan_layer_tensor.

The cases and references are those of tests/test_device_layer.py
(tests/device_layer_common.py): the marks against the checksum rule restated in Python, every
scan against tsg_layer_scan of the same bytes from host memory on the same context.  Each
test runs one context and inputs of a few KiB to a few MiB."""
import tarfile

import pytest

from tests import device_layer_common as X
from trivy_amd import analyzer as A
from trivy_amd import secret as S
from trivy_amd import walker as W

pytestmark = pytest.mark.gpu

GPU = True


@pytest.fixture(scope="module")
def builtin():
    return S.NewScanner(None)


@pytest.fixture
def ctx(builtin):
    c = S.GpuContext(builtin, 0, adapt_mib=0xFFFFFFFF)
    yield c
    c.close()


def test_marks_edge_blocks(ctx):
    blocks, want = X.edge_blocks()
    tar = X.member(b"first.env", X.body()) + b"".join(blocks) + X.member(b"last.env", X.body())
    for skew in (0, 5):
        hdr, zero = X.check_marks(ctx, tar, GPU, skew=skew)
        assert hdr[2:2 + len(blocks)].tolist() == want
        assert zero[2:2 + len(blocks)].tolist() == [b == X.ZERO_BLOCK for b in blocks]


@pytest.mark.parametrize("nblocks", [0, 1, 63, 64, 65, 4097])
def test_marks_block_counts(ctx, nblocks):
    hdr, zero = X.check_marks(ctx, X.mixed_blocks(nblocks, nblocks), GPU, skew=nblocks % 16)
    assert len(hdr) == len(zero) == nblocks
    if nblocks > 60:
        assert hdr.any() and zero.any() and not (hdr | zero).all()


def test_marks_tails(ctx):
    """tar_len 0, 511, 512 and 512 k + 1 .. + 511: the tail under 512 bytes is no block, also
    where it holds the start of a header.  Every length is a slice of one device tensor."""
    whole = X.mixed_blocks(3, 5) + X.header(b"tail.env")
    t = X.tensor_of(whole, GPU, skew=9)
    for n in [0, 1, 511, 512, 513, 1023, 1024] + list(range(3 * 512 + 1, 4 * 512)) + [4 * 512]:
        hdr, zero = ctx.tar_marks(t[:n])
        rh, rz = X.ref_marks(whole[:n])
        assert hdr.tolist() == rh.tolist() and zero.tolist() == rz.tolist(), n
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
    sizes = X.ext_payload_sizes(tar)
    assert sizes and st["payload_rounds"] >= 1
    assert st["payloads"] == len(sizes) and st["payload_bytes"] == sum(sizes)
    assert st["chain_entries"] + len(sizes) == st["marked_blocks"] and st["span_batches"] == 1
    assert st["mark_ms"] > 0


def test_nested_tar(ctx):
    (paths, res, _, _, _), st = X.check_layer(ctx, X.nested_layer(), GPU, skew=1)
    assert st["chain_entries"] == 3 and st["marked_blocks"] == 3 + 5
    assert paths == ["/a/first.env", "/a/last.env"] and not any("inner" in p for p in paths)
    assert st["payload_rounds"] == 0 and st["payload_bytes"] == 0


def test_pax_size_override(ctx):
    (paths, res, _, _, _), st = X.check_layer(ctx, X.pax_size_layer(), GPU, skew=15)
    assert paths == ["/grow.env", "/renamed/short.env", "/after.env"]
    assert st["chain_entries"] == 3 and st["payloads"] >= 2 and st["payload_rounds"] >= 1
    assert all(r["Findings"] for r in res)


@pytest.mark.parametrize("name", sorted(X.malformed_tars()))
def test_malformed(ctx, name):
    assert X.case_malformed(ctx, GPU, name) is not None


@pytest.mark.parametrize("name", sorted(X.empty_tars()))
def test_empty_archives(ctx, name):
    tar = X.empty_tars()[name]
    want = X.native_error(W.scan_layer_pipelined, ctx, tar)
    if want is not None:
        assert X.native_error(W.scan_layer_tensor, ctx, X.tensor_of(tar, GPU)) == want
        return
    (paths, _, _, _, _), st = X.check_layer(ctx, tar, GPU)
    assert len(paths) == (1 if b"one.env" in tar else 0)


def test_pieces(ctx, knob):
    st = X.case_pieces(ctx, GPU, knob)
    assert st["mark_ms"] > 0


def test_poisoned_mirror_gives_the_same(ctx, knob):
    knob("device_poison", 1)
    X.check_layer(ctx, X.layer_bytes(), GPU)
    X.check_layer(ctx, X.pax_size_layer(), GPU, skew=5)


def test_two_threads(ctx):
    X.case_two_threads(ctx, GPU)


def test_arguments(ctx):
    X.case_arguments(ctx, GPU)
    with pytest.raises(ValueError):  # a host tensor on a device context
        W.scan_layer_tensor(ctx, X.tensor_of(X.good_layer(), False))
    with pytest.raises(ValueError):
        ctx.tar_marks(X.tensor_of(X.good_layer(), False))


def test_analyze_layer_tensor(ctx, builtin):
    an = A.SecretAnalyzer(builtin, "")
    tar = X.layer_bytes()
    want = W.analyze_layer_native(an, tar, ctx=ctx, skip_files=["app/skipme.txt"])
    got = W.analyze_layer_tensor(an, X.tensor_of(tar, GPU), ctx, skip_files=["app/skipme.txt"])
    assert got == want and [s["FilePath"] for s in got[0]][:1] == ["/abs/slack.txt"]
