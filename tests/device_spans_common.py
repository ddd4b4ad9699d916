"""Shared by tests/test_device_spans.py (emulated context, host tensors) and
tests/test_gpu_device_spans.py (device): files laid out as spans of one buffer, the raw ABI
call, the references and the cases both files run.

The references do not come from the code under test: the kept mask is
trivy_amd.analyzer.IsBinary over the host bytes, and the findings are tsg_scan_batch's result
bytes (raw_scan_batch) for a Batch built from the kept files."""
import ctypes as C
import io
import tarfile
import threading

import numpy as np
import torch

from tests import helpers as H
from tests.device_input_common import (POISON, big_file_batch, check_mirror, hostonly_case, raw_scan_batch,
                                       result_bytes)
from trivy_amd import _native as N
from trivy_amd import analyzer as A
from trivy_amd import configs
from trivy_amd import secret as S

GATE = N.TSG_SPANS_BINARY_GATE
ZERO = b"\0"


class Layout:
    """Files placed in one buffer.  `contents[i]` is input file i; `order` is the order in
    which the files lie in the buffer (default: input order); `gaps[k]` is the number of fill
    bytes before the k-th placed file (an int for all), raised to the next value that gives
    the file the start offset `align[i]` mod 16 where one is asked for; `tail` fill bytes
    follow the last file.  The buffer is the fill pattern repeated, and the pattern starts
    again right behind every file, so a copy that runs one byte past a span copies the
    pattern's first byte."""

    def __init__(self, contents, fill=POISON, order=None, gaps=512, align=None, tail=64, paths=None):
        n = len(contents)
        order = list(range(n)) if order is None else list(order)
        assert sorted(order) == list(range(n))
        gaps = [gaps] * n if isinstance(gaps, int) else list(gaps)
        starts = [0] * n
        at = 0
        for k, i in enumerate(order):
            at += gaps[k]
            if align is not None and align[i] is not None:
                at += (align[i] - at) % 16
            starts[i] = at
            at += len(contents[i])
        total = at + tail
        buf = np.frombuffer((fill * (total // len(fill) + 1))[:total], dtype=np.uint8).copy()
        for i in order:  # the pattern from its start behind every file ...
            e = starts[i] + len(contents[i])
            m = min(len(fill), total - e)
            buf[e:e + m] = np.frombuffer(fill[:m], dtype=np.uint8)
        for i in order:  # ... and the files over it
            buf[starts[i]:starts[i] + len(contents[i])] = np.frombuffer(contents[i], dtype=np.uint8)
        self.contents = [bytes(c) for c in contents]
        self.buf = buf
        self.starts = np.array(starts, dtype=np.uint64)
        self.lengths = np.array([len(c) for c in contents], dtype=np.uint64)
        self.paths = list(paths) if paths is not None else ["s/%d.txt" % i for i in range(n)]

    def binary(self):
        return np.array([A.IsBinary(c, len(c)) for c in self.contents], dtype=bool)

    def batch(self, kept):
        """The Batch of the kept files, in input order."""
        return S.Batch.from_args([S.ScanArgs(p, c) for p, c, k in zip(self.paths, self.contents, kept) if k])


class Dev:
    """The buffer where the context reads it: a host tensor (emulated) or a tensor on cuda:0,
    optionally as a slice with storage offset `skew` of an allocation of the same fill."""

    def __init__(self, buf, gpu, skew=0, fill=ZERO):
        host = np.concatenate([np.frombuffer(fill * skew, dtype=np.uint8)[:skew], buf,
                               np.frombuffer(fill * 32, dtype=np.uint8)[:32]]) if skew else buf
        t = torch.from_numpy(np.ascontiguousarray(host).copy())
        if gpu:
            t = t.to("cuda:0")
            torch.cuda.synchronize()
        self.whole = t
        self.tensor = t[skew:skew + len(buf)] if skew else t
        assert self.tensor.storage_offset() == skew and self.tensor.numel() == len(buf)
        self.ptr = self.tensor.data_ptr() if len(buf) else None
        self.n = len(buf)


def u64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def path_arrays(paths):
    pb = [p.encode() for p in paths]
    poffs = np.zeros(len(pb) + 1, dtype=np.uint64)
    np.cumsum(np.array([len(p) for p in pb], dtype=np.uint64), out=poffs[1:])
    return np.frombuffer(b"".join(pb) or b"\0", dtype=np.uint8), poffs


def raw_scan_spans(ctx, dev, starts, lengths, paths, flags=GATE):
    """tsg_scan_device_spans: (result bytes, kept mask)."""
    blob, poffs = path_arrays(paths)
    kept = np.full(max(len(paths), 1), 7, dtype=np.uint8)
    out = C.c_void_p()
    N.check(N.lib().tsg_scan_device_spans(ctx.handle, C.c_void_p(dev.ptr), dev.n, u64p(starts), u64p(lengths),
                                          len(paths), C.c_void_p(blob.ctypes.data), u64p(poffs), flags,
                                          kept.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(out)))
    kept = kept[:len(paths)]
    assert set(kept.tolist()) <= {0, 1}
    return result_bytes(out), kept.astype(bool)


def check_scan(ctx, lay, dev, gate=True, mirror=True, wrapper=True):
    """One spans scan against the references: kept == !IsBinary (all files with the gate
    off), result bytes == tsg_scan_batch's for the kept files, the stats add up, and (with
    the knob device_poison on) the mirror holds whole needed files of the compacted batch and
    the poison elsewhere.  The Python wrapper returns the same.  Returns (kept, batch of the
    kept files, spans stats, device-input stats, decoded findings of the kept files)."""
    want_kept = ~lay.binary() if gate else np.ones(len(lay.contents), dtype=bool)
    b = lay.batch(want_kept)
    want = raw_scan_batch(ctx, b)
    before = ctx.device_spans_stats()
    got, kept = raw_scan_spans(ctx, dev, lay.starts, lay.lengths, lay.paths, GATE if gate else 0)
    assert kept.tolist() == want_kept.tolist()
    assert got == want
    st, di = ctx.device_spans_stats(), ctx.device_input_stats()
    assert st["files_in"] == len(lay.contents) and st["files_kept"] == int(kept.sum())
    assert st["files_kept"] + st["files_dropped"] == st["files_in"]
    assert st["bytes_in"] == int(lay.lengths.sum()) and st["bytes_kept"] == int(lay.lengths[kept].sum())
    assert st["batches"] == before["batches"] + 1
    assert st["sum_files_kept"] == before["sum_files_kept"] + st["files_kept"]
    assert st["sum_bytes_in"] == before["sum_bytes_in"] + st["bytes_in"]
    assert di["whole_batch_copy"] == 0 and di["stage_ms"] == st["gather_ms"]
    if mirror:
        check_mirror(ctx, b, di, src=lay.starts[want_kept])
    found = S.decode_results(want, [b.path(i) for i in range(b.nfiles)], ctx.scanner.Rules)
    if wrapper:
        res, kept2 = ctx.scan_spans(dev.tensor, lay.starts, lay.lengths, lay.paths, binary_gate=gate)
        assert kept2.tolist() == want_kept.tolist()
        assert res == found
    return kept, b, st, di, found


# ---------------------------------------------------------------- inputs
def text(n, seed=0):
    return H.quiet(np.random.default_rng(1000 + seed), n)


def gate_layout():
    """The gate's edges in one zero-filled buffer (an over-read flags a text file): the
    control byte at index 299 / 300, lengths 0, 1, 299, 300, 301, every boundary value of the
    predicate once in a clean file, a span at every alignment 0..15, one at byte 0 of the
    buffer and one ending at its last byte."""
    files, align = [], []

    def add(c, a=None):
        files.append(bytes(c))
        align.append(a)
    add(text(37, 1), 0)                                  # at byte 0 of the buffer
    for at in (299, 300):
        c = bytearray(text(400, at))
        c[at] = 1
        add(c)
    for n in (0, 1, 299, 300, 301):
        add(text(n, n))
    for v in (6, 7, 10, 11, 12, 13, 14, 26, 27, 28, 31, 32, 0x7e, 0x7f, 0x80, 0xff):
        c = bytearray(text(40, v))
        c[17] = v
        add(c)
    c = bytearray(text(300, 5))                          # binary by its last looked-at byte only
    c[299] = 0x7f
    add(c)
    for k in range(16):
        add(text(33 + k, 50 + k), k)
        c = bytearray(text(33, 70 + k))
        c[32] = 3                                        # the last byte decides
        add(c, k)
    add(text(21, 2))                                     # ends at the buffer's last byte
    lay = Layout(files, fill=ZERO, gaps=[0] + [19] * (len(files) - 1), align=align, tail=0)
    assert lay.starts[0] == 0 and int(lay.starts[-1] + lay.lengths[-1]) == len(lay.buf)
    want = [False, True, False] + [False] * 5 + [v in (6, 11, 14, 26, 28, 31, 0x7f) for v in
                                                 (6, 7, 10, 11, 12, 13, 14, 26, 27, 28, 31, 32, 0x7e, 0x7f, 0x80, 0xff)]
    assert lay.binary().tolist()[:len(want)] == want     # (the reference agrees with the issue's table)
    return lay


def small_files(seed, n=14):
    """Short files, some with a secret at the start, in the middle or as their last bytes,
    some empty, some binary."""
    rng = np.random.default_rng(seed)
    files = []
    for i in range(n):
        body = H.quiet(rng, int(rng.integers(30, 900)))
        if i % 4 == 0:
            body = b"k = " + H.AKIA + b"\n" + body
        elif i % 4 == 1:
            body = body + b"\n" + H.AKIA               # the secret ends at the span's last byte
        elif i % 7 == 3:
            body = b""
        elif i % 7 == 6:
            body = b"\x7fELF\x02\x01\x01" + body + b"\nk = " + H.AKIA + b"\n"
        files.append(body)
    return files


def order_layout(kind):
    files = small_files(21)
    n = len(files)
    order = list(range(n))[::-1] if kind == "descending" else list(np.random.default_rng(3).permutation(n))
    return Layout(files, order=order, gaps=[int(g) for g in np.random.default_rng(4).integers(1, 700, n)])


def adjacency_layout():
    """Files 0 and 1 touch in the source (gap 0: one staging segment), files 2 and 3 are
    adjacent in the destination only (3 lies before 2 in the buffer), 4 and 5 touch in the
    source in the wrong order, and an empty file sits between two touching ones (6, 7, 8)."""
    f = small_files(33, 9)
    f[7] = b""
    order = [0, 1, 3, 2, 5, 4, 6, 7, 8]
    return Layout(f, order=order, gaps=[40, 0, 100, 77, 9, 0, 300, 0, 0])


def big_layout():
    b = big_file_batch()
    files = [bytes(b.data[int(b.offsets[i]):int(b.offsets[i + 1])]) for i in range(b.nfiles)]
    assert max(len(c) for c in files) == 300 << 10 and any(len(c) == 0 for c in files)
    return Layout(files, gaps=[int(g) for g in np.random.default_rng(8).integers(1, 600, len(files))],
                  paths=[b.path(i) for i in range(b.nfiles)])


def alignment_layout():
    """256 files of 49 bytes with a secret each: file 16 s + d starts at s mod 16 in the
    buffer and (every length being 1 mod 16) at d mod 16 in the batch."""
    files = [b"k = " + H.AKIA + b"\n" + text(24, k) for k in range(256)]
    lay = Layout(files, gaps=17, align=[k // 16 for k in range(256)])
    dst = np.concatenate([[0], np.cumsum(lay.lengths)[:-1]]).astype(np.int64)
    assert {(int(s) % 16, int(d) % 16) for s, d in zip(lay.starts, dst)} == {(s, d) for s in range(16) for d in range(16)}
    return lay


def hostonly_layout():
    sc, b = hostonly_case(8 << 10)
    files = [bytes(b.data[int(b.offsets[i]):int(b.offsets[i + 1])]) for i in range(b.nfiles)]
    return sc, Layout(files, gaps=512, paths=[b.path(i) for i in range(b.nfiles)])


def tar_members():
    """(tar bytes, [(offset_data, size, name)] of the regular files) of the layer tar of
    configs[2] with 30 % binary blobs."""
    tar = configs.layer_tar(256 << 10, binary_frac=0.3)
    with tarfile.open(fileobj=io.BytesIO(tar)) as tf:
        members = [(m.offset_data, m.size, m.name) for m in tf.getmembers() if m.isreg()]
    return tar, members


# ---------------------------------------------------------------- cases both files run
def case_tar(ctx, gpu):
    """AnalyzeTensor over the whole tar == AnalyzeBatch over the same members read on the
    host; the input holds both kept and dropped files (by IsBinary alone)."""
    tar, members = tar_members()
    an = A.SecretAnalyzer(ctx.scanner)
    req = [(o, n, name) for o, n, name in members if an.Required(name, n)]
    binary = [A.IsBinary(tar[o:o + n], n) for o, n, _ in req]
    assert any(binary) and not all(binary) and len(req) < len(members)
    inputs = [A.AnalysisInput("", name, tar[o:o + n]) for o, n, name in members if an.Required(name, n)]
    want = an.AnalyzeBatch(inputs, ctx=ctx)
    assert want and all(s["FilePath"].startswith("/") for s in want)
    dev = Dev(np.frombuffer(tar, dtype=np.uint8), gpu)
    got = an.AnalyzeTensor(dev.tensor, [o for o, _, _ in members], [n for _, n, _ in members],
                           [name for _, _, name in members], dir="", ctx=ctx)
    assert got == want
    st = ctx.device_spans_stats()
    assert st["files_in"] == len(req) and st["files_dropped"] == sum(binary) and st["files_kept"] == len(req) - sum(binary)
    return st


def case_two_submitters(ctx, gpu):
    """Two threads submit and collect spans batches on one context while the main thread
    scans another tensor with scan_tensor; everyone gets its own results."""
    lays = [order_layout("descending"), adjacency_layout()]
    devs = [Dev(l.buf, gpu) for l in lays]
    keeps = [~l.binary() for l in lays]
    batches = [l.batch(k) for l, k in zip(lays, keeps)]
    want = [ctx.scan_batch(b) for b in batches]
    other = big_file_batch()
    other_want = ctx.scan_batch(other)
    other_t = Dev(np.array(other.data[:int(other.offsets[-1])]), gpu).tensor
    errors = []

    def worker(k):
        try:
            for _ in range(3):
                t = ctx.submit_spans(devs[k].tensor, lays[k].starts, lays[k].lengths, lays[k].paths)
                assert ctx.spans_kept(t).tolist() == keeps[k].tolist()
                t2 = ctx.submit_spans(devs[k].tensor, lays[k].starts, lays[k].lengths, lays[k].paths)
                assert ctx.collect(t2) == want[k]
                assert ctx.collect(t) == want[k]
        except BaseException as e:  # noqa: B902 (reported by the main thread)
            errors.append((k, repr(e)))
    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for _ in range(3):
        assert ctx.scan_tensor(other_t, other.offsets, [other.path(i) for i in range(other.nfiles)]) == other_want
    for t in threads:
        t.join()
    assert not errors, errors
    assert ctx.pending() == 0 and not ctx._tensors and not ctx._kept
    assert ctx.device_spans_stats()["batches"] == 12
