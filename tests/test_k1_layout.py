"""Which body of the automaton K1 (k1_kernel) a keyword automaton gets, without a GPU.

k1_kernel has two inner loops: the packed layout (rows as 16-bit byte offsets, states x stride
x 2 <= 65,536) and the legacy one (rows as entry indices, class words with the run masks folded
in, a saturating pair of run counters) for every larger table up to the plan's cap of 96 KiB.
The hook tsg_test_k1_layout_of restates nothing: it calls the library's own k1_stride,
k1_packed_fits and k1_lds_class.  Here its answers are swept over every automaton the plan can
produce -- only two layouts are reachable, which is why only two kernels are built -- and
pinned for the rule sets tests/test_gpu_k1_legacy.py runs on the device, so that a planner
change that moves one of them out of its layout fails here, not silently there."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers as H
from tests import k1_legacy_common as KL
from trivy_amd import _native as N
from trivy_amd import secret as S

REP_BYTES = 256 * 32 * 4   # the legacy image's replicated class words (kK1RepBytes)


def test_only_two_layouts_are_reachable():
    """Every (states, classes) with 2 <= classes <= 128 and states x classes x 2 <= 98,304
    (217,846 automata; the full sweep, about a second): the layout is packed or the legacy
    one of LDS class 2 with replicated class words, and the call succeeds, i.e. a kernel is
    built for it.  Beside that, what the kernels rely on to stay inside their LDS images and
    16-bit rows: a packed table fits the 64 KiB behind the class entries, a legacy table and
    the 32 KiB of class words fit the 156 KiB image, the last state's row fits 16 bits, and
    the stride is the class count padded to 2 mod 4 wherever that padding neither changes
    the layout nor overflows the rows (restated here from the rule, not from k1_stride)."""
    f = N.lib().tsg_test_k1_layout_of
    v = N.K1Layout()
    ref = C.byref(v)
    seen = {"packed": 0, "legacy": 0, "padded": 0, "unpadded": 0}
    for nc in range(2, 129):
        rs = nc + (2 - nc) % 4
        for ns in range(1, KL.KW_TABLE_CAP // 2 // nc + 1):
            rc = f(ns, nc, ref)
            got = (v.packed, v.lds_class, v.rep, v.lds_kib, v.threads, v.blocks_per_cu)
            assert rc == N.TSG_OK, "states %d classes %d: %s, layout %s" % (ns, nc, N.lib().tsg_last_error(), got)
            assert (v.states, v.classes) == (ns, nc)
            entries = ns * v.stride
            assert v.table_bytes == (entries + (entries & 1)) * 2
            if v.packed:
                assert got == (1, v.lds_class, v.rep, 128, 1024, 1), (ns, nc, got)
                assert v.table_bytes <= 65536 and v.row_unit == 2 * v.stride
                assert ns * nc * 2 <= 65536
                want = rs if ns * rs * 2 <= 65536 else nc
            else:
                assert got == (0, 2, 1, 156, 1024, 1), (ns, nc, got)
                assert v.table_bytes + REP_BYTES <= 156 * 1024 and v.row_unit == v.stride
                assert ns * nc * 2 > 65536
                padded = (ns * rs + (ns * rs & 1)) * 2
                want = rs if (ns - 1) * rs <= 0xFFFF and padded + REP_BYTES <= 156 * 1024 else nc
            assert v.stride == want, (ns, nc, v.stride, want)
            assert (ns - 1) * v.row_unit <= 0xFFFF
            seen["packed" if v.packed else "legacy"] += 1
            seen["padded" if v.stride % 4 == 2 else "unpadded"] += 1
    print("K1 layouts of %d automata: %s" % (seen["packed"] + seen["legacy"], seen))
    assert min(seen.values()) > 0


def test_layout_of_rejects_what_device_tables_cannot_hold():
    """TSG_ERR_ARG where make_device_k1 / k1_tables fail: no state or class, more than 128
    classes, rows past 16 bits, a table past LDS."""
    for ns, nc in ((0, 8), (8, 0), (8, 129), (40000, 2), (1300, 128), (3000, 44)):
        with pytest.raises(N.NativeError) as e:
            S.k1_layout_of(ns, nc)
        assert e.value.code == N.TSG_ERR_ARG, (ns, nc)
    assert S.k1_layout_of(8, 128)["packed"] == 1


@pytest.mark.parametrize("name", sorted(KL.SETS))
def test_rule_sets_keep_their_layout(name):
    """The builtin rules and the user rule sets of the device tests: states, classes, layout
    and K1X literal count are those the tests were chosen for."""
    n, step, states, classes, packed, k1x = KL.SETS[name]
    info = KL.scanner(name).info()
    lay = KL.layout(name)
    print(name, info, lay)
    moved = ("%s no longer compiles to the keyword automaton tests/test_gpu_k1_legacy.py runs it for "
             "(%d x %d, %s, %d K1X literals): it is now %d x %d, %s, %d K1X literals.  Choose a new n for the "
             "device tests (tests/k1_legacy_common.py)." % (
                 name, states, classes, "packed" if packed else "legacy", k1x, info["kw_states"], info["kw_classes"],
                 "packed" if lay["packed"] else "legacy", info["k1x_literals"]))
    assert (info["kw_states"], info["kw_classes"], lay["packed"], info["k1x_literals"]) == (states, classes, packed, k1x), moved
    assert (KL.is_packed(lay) if packed else KL.is_legacy(lay)), moved
    assert info["kw_states"] * info["kw_classes"] * 2 <= KL.KW_TABLE_CAP
    if name in (KL.L30, KL.L70):
        assert info["k1x_literals"] == 0, moved
    if name in (KL.LX, KL.PW):   # wide keyword rows: 28 words
        assert (info["n_keywords"] + 31) // 32 == 28, moved


def test_emulated_context_has_no_layout():
    ctx = S.GpuContext(KL.scanner(KL.BUILTIN), 0, emulate=True)
    try:
        with pytest.raises(N.NativeError) as e:
            ctx.k1_layout()
        assert e.value.code == N.TSG_ERR_ARG
    finally:
        ctx.close()


@pytest.mark.parametrize("name", [KL.BUILTIN, "user60"])
def test_run_saturation_batch_covers_its_edges(name):
    """The batch of the device's saturation test, from the references alone: 153 files, runs of
    both classes, and k1_reference == tsg_emulate_k1f (two independent restatements of the run
    counters) at chunks 16 and 256; at chunk 16 tens of thousands of chunks lie wholly inside a
    run behind byte 256 and behind byte 65,536 of it."""
    sc = KL.scanner(name)
    b = H.run_saturation_batch()
    total = int(b.offsets[-1])
    assert b.nfiles == 153 and 3_300_000 < total < 3_500_000
    assert bytes(b.data[total - 66000:total]).translate(None, H.RUN_U) == b""   # the last run ends the batch
    for chunk in (16, 256):
        rkw, rev = sc.k1_reference(b, chunk)
        fkw, fev, _ = sc.k1f_emulate(b, chunk)
        assert np.array_equal(rkw, fkw) and np.array_equal(rev, fev)
        nu, nd = int(((rev & 1) != 0).sum()), int(((rev & 2) != 0).sum())
        print("%s chunk %d: %d files, %d bytes, run-U chunks %d, run-D chunks %d" % (name, chunk, b.nfiles, total, nu, nd))
        assert nu > 65536 * 2 // chunk and nd > 65536 // chunk
