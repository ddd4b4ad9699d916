#!/usr/bin/env python
"""Device-resident input against the PCIe path, same bytes, same context.

    python tools/device_bench.py [--gb 4] [--steps 20] [--rounds 3] [--warmup 1] [--depth 4]
    python tools/device_bench.py --spans [--gb 1] [--batch-mib 256] ...
    python tools/device_bench.py --layer [--gb 1] [--steps 5] [--rounds 3] ...

The configs[1] workload of bench.py (builtin rules over the seeded corpus, seed 2, in
batches of --batch-mib) is scanned two ways on one GpuContext:

  pcie      the batches sit in pinned slots and are submitted with tsg_slot_submit, --depth
            in flight: bench.py's headline path (content crosses PCIe once per scan)
  resident  the same bytes were uploaded once as torch tensors and are submitted with
            tsg_device_submit (GpuContext.submit_tensor), --depth in flight: staged HBM ->
            HBM, and only the files the resolver reads come back

Every batch's result bytes of the two paths are compared (they must be equal).  Prints one
JSON line: GB/s of both paths, the per-batch stage / fetch / resolve / K1 times of the
resident path, and the share of the bytes that was fetched.  The two paths are timed in
alternation, --rounds windows of --steps passes each after --warmup passes, with the host
clock over whole windows (every result collected); the line carries every window's GB/s
and the medians.  The per-stage figures are the library's HIP-event times of the last
window (tsg_stats, tsg_device_input_stats); resident_windows_ms has the stage's and the
fetch's mean of every window.

--spans measures tsg_device_spans_submit instead (GpuContext.scan_spans' entry point).  The
seeded corpus is laid out as a decompressed layer would be: the files in order with 512
bytes between them, 30 % of them binary blobs (random bytes from the first byte on, which
utils.IsBinary drops), uploaded once as one tensor.  Two paths run in alternation on one
context, over the same kept bytes:

  spans     the files as (start, length) spans of that tensor, the binary gate on: gate
            kernel, the submit-side wait for it, the gather into the lane buffer
  compact   the parent path: the kept files packed back to back on the host beforehand
            (the pre-compaction is not timed), uploaded once, tsg_device_submit

Every batch's result bytes of the two paths are compared, and the kept mask is compared
with IsBinary on the host.  The JSON line carries GB/s of kept bytes of both paths per
window, and per batch the gate, the submit wait and the gather beside the compact path's
stage_ms, each as the mean of every window (so the spread between windows shows).

--layer measures tsg_device_layer_scan (walker.scan_layer_tensor).  One configs.layer_tar
layer of --gb GiB is scanned two ways on one context, in alternating windows:

  host      the tar in host memory through tsg_layer_scan (walker.scan_layer_pipelined): the
            only way to scan these bytes without the new call; the kept files cross PCIe
  device    the same bytes uploaded once as one tensor, through tsg_device_layer_scan: the
            marks kernel over the whole tar, the header blocks and extended-header payloads
            fetched, the walk on the host, the kept files as spans batches

Both are timed as raw native calls (nothing is decoded in Python inside a window), and the
result bytes, paths, opaque dirs, whiteouts and walked count of the two calls are compared.  The JSON line carries GB/s of tar of both
per window, mark_ms per window beside the staging copy of the same number of bytes
(stage_ms of a scan_tensor over as many zero bytes as one file, a single read + write
pass), the header and payload bytes fetched, and the share of the tar that crossed PCIe."""
import argparse
import collections
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=4.0, help="GiB of corpus")
    ap.add_argument("--batch-mib", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20, help="passes over the corpus per timed window")
    ap.add_argument("--rounds", type=int, default=3, help="timed windows per path, alternating")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--depth", type=int, default=4, help="batches in flight")
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--emulate", action="store_true",
                    help="dry run of this script without a GPU (emulated context, host tensors)")
    ap.add_argument("--spans", action="store_true",
                    help="files as spans of one buffer with 30 %% binary blobs against scan_tensor "
                         "over the pre-compacted kept bytes")
    ap.add_argument("--layer", action="store_true",
                    help="one layer tar from host memory (tsg_layer_scan) against the same tar in a tensor "
                         "(tsg_device_layer_scan)")
    args = ap.parse_args()
    if args.spans:
        return main_spans(args)
    if args.layer:
        return main_layer(args)

    import numpy as np
    import torch
    from bench import fill_slots
    from trivy_amd import _native as N
    from trivy_amd import corpus
    from trivy_amd import secret as S

    def log(msg):
        print(msg, file=sys.stderr, flush=True)

    L = N.lib()
    sc = S.NewScanner(None)
    t0 = time.perf_counter()
    batch, info = corpus.make_corpus(int(args.gb * (1 << 30)), seed=args.seed, plants_per_mib=1.0)
    log("corpus %.2f GiB, %d files, generated in %.1fs" % (info["bytes"] / (1 << 30), info["files"],
                                                          time.perf_counter() - t0))
    nb = -(-int(batch.offsets[-1]) // (args.batch_mib << 20))
    # pinned slots: the PCIe path's own, and one mirror per resident batch in flight
    ctx = S.GpuContext(sc, args.device, max_slots=nb + args.depth + 4, emulate=args.emulate)
    slots = fill_slots(ctx, batch, args.batch_mib << 20)
    dev = "cpu" if args.emulate else "cuda:%d" % args.device
    pieces, f0 = [], 0
    for sid, nf, nbytes in slots:  # the same cuts, as tensors in HBM (uploaded once)
        base = int(batch.offsets[f0])
        offs = (batch.offsets[f0:f0 + nf + 1] - np.uint64(base)).copy()
        t = torch.from_numpy(batch.data[base:base + nbytes]).to(dev)
        # checked and packed once (submit_tensor would encode the paths again on every call)
        pieces.append((t, ctx._tensor_args(t, offs, [batch.path(i) for i in range(f0, f0 + nf)])))
        f0 += nf
    if not args.emulate:
        torch.cuda.synchronize()
    total = sum(nbytes for _, _, nbytes in slots)
    log("%d batches packed: pinned slots and device tensors" % len(slots))

    def raw(out):
        n = C.c_size_t()
        p = L.tsg_result_data(out, C.byref(n))
        buf = C.string_at(p, n.value)
        L.tsg_result_free(out)
        return buf

    def run(submit, steps, keep):
        """`steps` passes over the batches, --depth in flight; the last pass's result bytes
        per batch when keep."""
        q, kept = collections.deque(), {}

        def collect():
            t, k, i = q.popleft()
            out = C.c_void_p()
            N.check(L.tsg_batch_collect(ctx.handle, t, C.byref(out)))
            if keep and k == steps - 1:
                kept[i] = raw(out)
            else:
                L.tsg_result_free(out)

        for k in range(steps):
            for i in range(len(slots)):
                q.append((submit(i), k, i))
                while len(q) >= args.depth:
                    collect()
        while q:
            collect()
        return kept

    def submit_pcie(i):
        t = C.c_uint64()
        N.check(L.tsg_slot_submit(ctx.handle, slots[i][0], slots[i][1], C.byref(t)))
        return t.value

    def submit_resident(i):
        tk = C.c_uint64()
        N.check(L.tsg_device_submit(ctx.handle, *pieces[i][1][0], C.byref(tk)))
        return tk.value

    def timed(submit):
        run(submit, args.warmup, False)
        s0, d0 = ctx.stats(), ctx.device_input_stats()
        t0 = time.perf_counter()
        kept = run(submit, args.steps, True)
        dt = time.perf_counter() - t0
        s1, d1 = ctx.stats(), ctx.device_input_stats()
        ds = {k: s1[k] - s0[k] for k in s1 if k.startswith("sum_") or k == "batches"}
        dd = {k: d1[k] - d0[k] for k in d1 if k.startswith("sum_") or k == "batches"}
        return kept, dt, ds, dd

    pgbs, rgbs, equal = [], [], True
    win = {"stage": [], "fetch": []}  # HIP-event means per batch of each resident window
    for _ in range(max(1, args.rounds)):
        pk, pdt, ps, _ = timed(submit_pcie)
        rk, rdt, rs, rd = timed(submit_resident)
        equal = equal and all(pk[i] == rk[i] for i in range(len(slots)))
        pgbs.append(round(total * args.steps / pdt / 1e9, 3))
        rgbs.append(round(total * args.steps / rdt / 1e9, 3))
        win["stage"].append(round(rs["sum_h2d_ms"] / max(1, rs["batches"]), 4))
        win["fetch"].append(round(rd["sum_fetch_ms"] / max(1, rs["batches"]), 4))
    nbat = max(1, rs["batches"])
    pbat = max(1, ps["batches"])
    line = {
        "metric": "secret-scan GB/s (builtin rules), device-resident input vs the PCIe path, 1 MI355X",
        "resident_gbs": round(float(np.median(rgbs)), 3),
        "pcie_gbs": round(float(np.median(pgbs)), 3),
        "unit": "GB/s",
        "resident_gbs_windows": rgbs, "pcie_gbs_windows": pgbs,
        "findings_equal": equal,
        "gib": round(total / (1 << 30), 3), "batches": len(slots), "batch_mib": args.batch_mib,
        "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup, "depth": args.depth,
        "resident_per_batch_ms": {
            "stage": round(rs["sum_h2d_ms"] / nbat, 3), "fetch": round(rd["sum_fetch_ms"] / nbat, 3),
            "k1": round(rs["sum_k1_ms"] / nbat, 3), "gates": round(rs["sum_gate_ms"] / nbat, 3),
            "k2": round(rs["sum_k2_ms"] / nbat, 3), "resolve": round(rs["sum_resolve_ms"] / nbat, 3),
            "wall": round(rdt / args.steps / len(slots) * 1e3, 3)},
        "resident_windows_ms": win,
        "pcie_per_batch_ms": {
            "h2d": round(ps["sum_h2d_ms"] / pbat, 3), "k1": round(ps["sum_k1_ms"] / pbat, 3),
            "resolve": round(ps["sum_resolve_ms"] / pbat, 3),
            "wall": round(pdt / args.steps / len(slots) * 1e3, 3)},
        "fetched_share": round(rd["sum_fetched_bytes"] / max(1, rd["sum_bytes"]), 5),
        "fetched_mib_per_batch": round(rd["sum_fetched_bytes"] / nbat / (1 << 20), 3),
        "whole_batch_copy": ctx.device_input_stats()["whole_batch_copy"],
    }
    for sid, _, _ in slots:
        ctx.release_slot(sid)
    ctx.close()
    print(json.dumps(line))
    return 0 if equal else 1


def main_spans(args):
    import numpy as np
    import torch
    from trivy_amd import _native as N
    from trivy_amd import corpus
    from trivy_amd import secret as S

    def log(msg):
        print(msg, file=sys.stderr, flush=True)

    GAP = 512
    L = N.lib()
    sc = S.NewScanner(None)
    t0 = time.perf_counter()
    batch, info = corpus.make_corpus(int(args.gb * (1 << 30)), seed=args.seed, plants_per_mib=1.0)
    offs = batch.offsets.astype(np.int64)
    sizes = np.diff(offs)
    F = len(sizes)
    rng = np.random.default_rng(args.seed + 1000)
    blob = rng.random(F) < 0.3
    starts = np.cumsum(sizes + GAP) - sizes  # 512 bytes before every file
    buf = np.zeros(int(starts[-1] + sizes[-1]) + GAP, dtype=np.uint8)
    for f in range(F):
        a, n = int(starts[f]), int(sizes[f])
        if blob[f]:
            buf[a:a + n] = rng.integers(0, 256, size=n, dtype=np.uint8)
        else:
            buf[a:a + n] = batch.data[offs[f]:offs[f] + n]
    # utils.IsBinary on the host: the reference of the kept mask
    ctl = np.zeros(256, dtype=bool)
    for b in range(256):
        ctl[b] = b < 7 or b == 11 or 13 < b < 27 or 27 < b < 0x20 or b == 0x7F
    binary = np.array([ctl[buf[int(starts[f]):int(starts[f]) + min(int(sizes[f]), 300)]].any() for f in range(F)])
    keep = ~binary
    log("corpus %.2f GiB, %d files (%d binary), laid out in %.2f GiB, in %.1fs" % (
        sizes.sum() / (1 << 30), F, int(binary.sum()), len(buf) / (1 << 30), time.perf_counter() - t0))
    dev = "cpu" if args.emulate else "cuda:%d" % args.device
    whole = torch.from_numpy(buf).to(dev)
    # batches: runs of files holding about --batch-mib of kept bytes
    cuts, acc = [0], 0
    for f in range(F):
        acc += int(sizes[f]) if keep[f] else 0
        if acc >= (args.batch_mib << 20):
            cuts.append(f + 1)
            acc = 0
    if cuts[-1] != F:
        cuts.append(F)
    ctx = S.GpuContext(sc, args.device, max_slots=2 * args.depth + 4, emulate=args.emulate)
    paths = [batch.path(i) for i in range(F)]
    span_args, compact_args, tensors, kept_bytes = [], [], [], 0
    for a, e in zip(cuts[:-1], cuts[1:]):
        k = np.flatnonzero(keep[a:e]) + a
        span_args.append(ctx._spans_args(whole, starts[a:e], sizes[a:e], paths[a:e], True))
        packed = np.concatenate([buf[int(starts[f]):int(starts[f] + sizes[f])] for f in k] or [np.zeros(0, np.uint8)])
        o = np.zeros(len(k) + 1, dtype=np.uint64)
        np.cumsum(sizes[k], out=o[1:])
        t = torch.from_numpy(packed).to(dev)
        tensors.append(t)
        compact_args.append(ctx._tensor_args(t, o, [paths[f] for f in k]))
        kept_bytes += int(sizes[k].sum())
    if not args.emulate:
        torch.cuda.synchronize()
    nb = len(span_args)
    log("%d batches, %.3f GiB kept of %.3f GiB listed" % (nb, kept_bytes / (1 << 30), sizes.sum() / (1 << 30)))

    def raw(out):
        n = C.c_size_t()
        p = L.tsg_result_data(out, C.byref(n))
        data = C.string_at(p, n.value)
        L.tsg_result_free(out)
        return data

    def submit_spans(i):
        tk = C.c_uint64()
        N.check(L.tsg_device_spans_submit(ctx.handle, *span_args[i][0], C.byref(tk)))
        return tk.value

    def submit_compact(i):
        tk = C.c_uint64()
        N.check(L.tsg_device_submit(ctx.handle, *compact_args[i][0], C.byref(tk)))
        return tk.value

    def run(submit, steps, keep_last):
        q, got = collections.deque(), {}

        def collect():
            t, k, i = q.popleft()
            out = C.c_void_p()
            N.check(L.tsg_batch_collect(ctx.handle, t, C.byref(out)))
            if keep_last and k == steps - 1:
                got[i] = raw(out)
            else:
                L.tsg_result_free(out)
        for k in range(steps):
            for i in range(nb):
                q.append((submit(i), k, i))
                while len(q) >= args.depth:
                    collect()
        while q:
            collect()
        return got

    def sums(d):
        return {k: v for k, v in d.items() if k.startswith("sum_") or k == "batches"}

    def timed(submit):
        run(submit, args.warmup, False)
        s0, d0, p0 = sums(ctx.stats()), sums(ctx.device_input_stats()), sums(ctx.device_spans_stats())
        t0 = time.perf_counter()
        got = run(submit, args.steps, True)
        dt = time.perf_counter() - t0
        s1, d1, p1 = sums(ctx.stats()), sums(ctx.device_input_stats()), sums(ctx.device_spans_stats())
        return got, dt, {k: s1[k] - s0[k] for k in s1}, {k: d1[k] - d0[k] for k in d1}, {k: p1[k] - p0[k] for k in p1}

    sg, cg, equal, kept_equal = [], [], True, True
    win = {"gate": [], "wait": [], "gather": [], "stage": [], "spans_fetch": [], "compact_fetch": [], "spans_k1": [],
           "compact_k1": []}
    for _ in range(max(1, args.rounds)):
        sk, sdt, ss, sd, sp = timed(submit_spans)
        for (a, e), sa in zip(zip(cuts[:-1], cuts[1:]), span_args):
            kept_equal = kept_equal and bool((sa[3].astype(bool) == keep[a:e]).all())
        ck, cdt, cs, cd, _ = timed(submit_compact)
        equal = equal and all(sk[i] == ck[i] for i in range(nb))
        sg.append(round(kept_bytes * args.steps / sdt / 1e9, 3))
        cg.append(round(kept_bytes * args.steps / cdt / 1e9, 3))
        n = max(1, sp["batches"])
        m = max(1, cd["batches"])
        win["gate"].append(round(sp["sum_gate_ms"] / n, 4))
        win["wait"].append(round(sp["sum_wait_ms"] / n, 4))
        win["gather"].append(round(sp["sum_gather_ms"] / n, 4))
        win["stage"].append(round(cd["sum_stage_ms"] / m, 4))
        win["spans_fetch"].append(round(sd["sum_fetch_ms"] / n, 4))
        win["compact_fetch"].append(round(cd["sum_fetch_ms"] / m, 4))
        win["spans_k1"].append(round(ss["sum_k1_ms"] / n, 4))
        win["compact_k1"].append(round(cs["sum_k1_ms"] / m, 4))
    st = ctx.device_spans_stats()
    line = {
        "metric": "secret-scan GB/s of kept bytes (builtin rules), spans of a device buffer with the binary gate "
                  "vs scan_tensor over pre-compacted bytes, 1 MI355X",
        "spans_gbs": round(float(np.median(sg)), 3), "compact_gbs": round(float(np.median(cg)), 3), "unit": "GB/s",
        "spans_gbs_windows": sg, "compact_gbs_windows": cg,
        "findings_equal": equal, "kept_equals_isbinary": kept_equal,
        "files": F, "files_kept": int(keep.sum()), "files_dropped": int(binary.sum()),
        "listed_gib": round(float(sizes.sum()) / (1 << 30), 3), "kept_gib": round(kept_bytes / (1 << 30), 3),
        "buffer_gib": round(len(buf) / (1 << 30), 3), "gap_bytes": GAP,
        "batches": nb, "batch_mib": args.batch_mib, "steps": args.steps, "rounds": args.rounds,
        "warmup": args.warmup, "depth": args.depth,
        "per_batch_ms_windows": win,
        "per_batch_ms": {k: round(float(np.median(v)), 4) for k, v in win.items()},
        "last_batch": {k: st[k] for k in ("files_in", "files_kept", "files_dropped", "bytes_in", "bytes_kept")},
    }
    ctx.close()
    print(json.dumps(line))
    return 0 if equal and kept_equal else 1


def main_layer(args):
    import numpy as np
    import torch
    from trivy_amd import configs
    from trivy_amd import secret as S

    def log(msg):
        print(msg, file=sys.stderr, flush=True)

    sc = S.NewScanner(None)
    t0 = time.perf_counter()
    tar = configs.layer_tar(int(args.gb * (1 << 30)), seed=args.seed)
    log("layer tar %.3f GiB, built in %.1fs" % (len(tar) / (1 << 30), time.perf_counter() - t0))
    dev = "cpu" if args.emulate else "cuda:%d" % args.device
    whole = torch.from_numpy(np.frombuffer(tar, dtype=np.uint8).copy()).to(dev)
    if not args.emulate:
        torch.cuda.synchronize()
    ctx = S.GpuContext(sc, args.device, emulate=args.emulate)

    def sums(d):
        return {k: v for k, v in d.items() if k.startswith("sum_") or k in ("batches", "calls")}

    def timed(scan):
        for _ in range(args.warmup):
            scan()
        l0, d0 = sums(ctx.device_layer_stats()), sums(ctx.device_input_stats())
        t0 = time.perf_counter()
        for _ in range(args.steps):
            got = scan()
        dt = time.perf_counter() - t0
        l1, d1 = sums(ctx.device_layer_stats()), sums(ctx.device_input_stats())
        return got, dt, {k: l1[k] - l0[k] for k in l1}, {k: d1[k] - d0[k] for k in d1}

    from trivy_amd import _native as N
    L = N.lib()
    host = np.frombuffer(tar, dtype=np.uint8)
    ctx._check_tensor(whole)

    def raw(call, ptr):
        """One native call; (result bytes, path bytes, path offsets, opq, wh, walked): nothing is
        decoded in Python inside the timed windows."""
        h, out = C.c_void_p(), C.c_void_p()
        N.check(call(ctx.handle, C.c_void_p(ptr), len(tar), None, 0, None, 0, b"", C.byref(h), C.byref(out)))
        v = N.LayerView()
        N.check(L.tsg_layer_get(h, C.byref(v)))
        n = C.c_size_t()
        p = L.tsg_result_data(out, C.byref(n))
        poffs = np.ctypeslib.as_array(v.path_offsets, shape=(v.nfiles + 1,)).copy()
        got = (C.string_at(p, n.value), C.string_at(v.paths, int(poffs[-1])), poffs.tobytes(),
               C.string_at(v.opq, v.opq_len), C.string_at(v.wh, v.wh_len), v.walked)
        L.tsg_result_free(out)
        L.tsg_layer_free(h)
        return got

    hg, dg, marks, equal = [], [], [], True
    for _ in range(max(1, args.rounds)):
        want, hdt, _, _ = timed(lambda: raw(L.tsg_layer_scan, host.ctypes.data))
        got, ddt, dl, dd = timed(lambda: raw(L.tsg_device_layer_scan, whole.data_ptr()))
        equal = equal and got == want
        hg.append(round(len(tar) * args.steps / hdt / 1e9, 3))
        dg.append(round(len(tar) * args.steps / ddt / 1e9, 3))
        marks.append(round(dl["sum_mark_ms"] / max(1, dl["calls"]), 4))
    st = ctx.device_layer_stats()
    # a plain copy pass over as many bytes: the staging kernel of scan_tensor, the tar as one file
    # (a batch addresses 4 GiB at most: a longer tar is cut to that, and the time scaled)
    n1 = min(len(tar), (1 << 32) - (1 << 20))
    blank = torch.zeros(n1, dtype=torch.uint8, device=dev)  # (zero bytes: nothing to resolve or fetch)
    for _ in range(2):
        ctx.scan_tensor(blank, np.array([0, n1], dtype=np.uint64), ["/whole.bin"])
    stage_ms = ctx.device_input_stats()["stage_ms"] * len(tar) / n1
    line = {
        "metric": "secret-scan GB/s of tar (builtin rules), a layer tar in GPU memory (tsg_device_layer_scan) vs the "
                  "same tar from host memory (tsg_layer_scan), 1 MI355X",
        "device_gbs": round(float(np.median(dg)), 3), "host_gbs": round(float(np.median(hg)), 3), "unit": "GB/s",
        "device_gbs_windows": dg, "host_gbs_windows": hg, "outputs_equal": equal,
        "tar_gib": round(len(tar) / (1 << 30), 3), "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup,
        "mark_ms_windows": marks, "mark_ms": round(float(np.median(marks)), 4),
        "mark_read_gbs": round(len(tar) / max(float(np.median(marks)), 1e-9) / 1e6, 1),
        "stage_ms_same_bytes": round(stage_ms, 4),
        "last_call": {k: st[k] for k in ("blocks", "marked_blocks", "chain_entries", "header_bytes", "payloads",
                                         "payload_bytes", "payload_rounds", "span_batches", "files_scanned",
                                         "fetched_bytes", "pcie_bytes")},
        "pcie_share": round(st["pcie_bytes"] / max(1, len(tar)), 5),
        "files_walked": want[5],
    }
    ctx.close()
    print(json.dumps(line))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
