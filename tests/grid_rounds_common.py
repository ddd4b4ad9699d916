"""Inputs of tests/test_gpu_grid_rounds.py (the kernel-level comparisons under the knob
grid_cap) and the arithmetic of a capped grid's rounds.  tests/test_grid_rounds.py proves from
the references and the kernels' block shapes alone that each input takes every block of a
capped grid through its loop several times, with a partial last round.

Every kernel whose grid the knob caps walks `units` of work with gridDim.x blocks of
`block_units` each: thread or wave (b, t) takes unit r * cap * block_units + b * block_units + t
in round r."""
import functools

import numpy as np

from tests import helpers as H
from trivy_amd import configs
from trivy_amd import corpus
from trivy_amd import secret as S

CAPS = (1, 3)  # 3: no power of two, the blocks' ranges align with nothing

K1X_LANE_BYTES = 16 * S.K1X_BLOCK               # one 16-B word per lane of a block
K1X_ROUND_BYTES = S.K1X_WORDS * K1X_LANE_BYTES  # ... and kXWords of them per round
COMPACT_CHUNKS = S.EV_PER * S.BLOCK_THREADS     # chunks of one compaction block and round
WAVES = S.BLOCK_THREADS // 64                   # units of a wave-per-unit block and round


def rounds(units, block_units, cap):
    """(rounds of the grid, rounds of its last block, units in the grid's last round)."""
    per = cap * block_units
    n = -(-units // per)
    last_block = -(-max(units - (cap - 1) * block_units, 0) // per)
    return n, last_block, units - (n - 1) * per


def many_rounds(units, block_units, cap, least=3):
    """Every block of the capped grid runs its loop `least` times or more, and the grid's last
    round is partial (where a round holds more than one unit)."""
    n, last_block, tail = rounds(units, block_units, cap)
    return last_block >= least and (tail < cap * block_units or cap * block_units == 1)


# ---- K1X: user1000 rules, batch totals around the rounds of k1x_kernel's pipelined loop
@functools.lru_cache(maxsize=None)
def user_doc():
    return configs.user_rules_doc(1000, seed=4)


def k1x_totals(cap):
    """3 rounds exactly; 3 rounds + 1 byte; 2 rounds + one word per lane exactly; 2 rounds + 2
    words per lane + 87 bytes (ends inside u = 2, mid-word)."""
    R, U = cap * K1X_ROUND_BYTES, cap * K1X_LANE_BYTES
    return (3 * R, 3 * R + 1, 2 * R + U, 2 * R + 2 * U + 87)


def trimmed(args, total):
    """The files of `args` cut to exactly `total` bytes (the last kept file is cut short)."""
    out, at = [], 0
    for a in args:
        n = min(len(a.Content), total - at)
        out.append(S.ScanArgs(a.FilePath, a.Content[:n]))
        at += n
        if at == total:
            break
    assert at == total, (at, total)
    return S.Batch.from_args(out)


@functools.lru_cache(maxsize=None)
def k1x_batch(total):
    args = configs.mixed_batch(user_doc(), total + (128 << 10), seed=65, plants_per_file=0.8)
    return trimmed(args, total)


@functools.lru_cache(maxsize=None)
def k1x_overflow_case():
    """(scanner, batch) of tests/test_gpu_configs.py's test_k1x_list_overflow_inline_verify: the
    1,000 user rules and a periodic literal, and a 2 MiB batch every 16-byte word of which holds
    that literal, so that the blocks' list slices overflow and k1x_kernel verifies inline."""
    doc = configs.user_rules_doc(1000, seed=4)
    doc["rules"].append({"id": "periodic", "category": "user", "title": "periodic", "severity": "LOW",
                         "regex": r"qzqzqzqzqz(?P<secret>[0-9]{4})", "keywords": ["qzqzqzqzqz"]})
    sc = S.NewScanner(S.config_from_dict(doc))
    files = [S.ScanArgs("p/%d.txt" % i, b"qz" * (16 << 10) + b"0123\n") for i in range(64)]
    return sc, S.Batch.from_args(files)


# ---- compaction, item passes and K2: a corpus of 65,555 chunks of 16 bytes, dense with events
ROUNDS_CHUNK = 16


@functools.lru_cache(maxsize=None)
def rounds_corpus():
    return corpus.make_corpus((1 << 20) + 301, seed=5, plants_per_mib=1500)[0]


@functools.lru_cache(maxsize=None)
def user_items_batch():
    return S.Batch.from_args(configs.mixed_batch(user_doc(), 256 << 10, seed=67, plants_per_file=0.8))


def event_chunks(sc, batch, chunk):
    """Chunks with an event bit in k1_reference's events: the length of the device's event list."""
    _, ev = sc.k1_reference(batch, chunk)
    return int(np.count_nonzero(ev & 0x7FFFFFFF))


def entry_groups(sc, batch, chunk):
    """(groups of the list entries, groups of the dense entries) in list order, from the
    reference alone: the order in which one block of a grid of one stages the DFAs."""
    n = H.nchunks_of(batch, chunk)
    tri, counts = sc.emulate_items(batch, chunk, 16)
    ent, dent, _, _ = H.reference_work_lists(tri, counts, n, S.default_items_cap(n))
    return ent[:, 0].tolist(), dent[:, 0].tolist()


ENTRY_SHAPE = (128, 1100)  # entry_shape_batch: one group, three entries (512, 512, 76 items)


# ---- outputs_kernel: files and candidate records for three rounds of its 256-thread blocks
@functools.lru_cache(maxsize=None)
def outputs_batch():
    """2,500 files in small_files_batch's style: one to three lines with an AWS access key id
    each (a record or two per line), every 7th file empty, every 5th without a secret."""
    rng = np.random.default_rng(12)
    args = []
    for i in range(2500):
        if i % 7 == 3:
            body = b""
        elif i % 5 == 2:
            body = H.quiet(rng, int(rng.integers(1, 60)))
        else:
            body = b"".join(H.quiet(rng, int(rng.integers(0, 24))) + b"\nk = " + H.AKIA + b"\n"
                            for _ in range(1 + i % 3))
        args.append(S.ScanArgs("o/%d.txt" % i, body))
    return S.Batch.from_args(args)
