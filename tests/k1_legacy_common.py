"""The rule sets that put the automaton K1 (k1_kernel) into each of its two LDS layouts, shared
by tests/test_k1_layout.py (which proves on the CPU that each still compiles to the layout it is
run for) and tests/test_gpu_k1_legacy.py (which runs them on the device).  A set is the builtin
rules plus configs.user_rules_doc(n, seed=4); scanners are compiled once per process."""
import functools

from trivy_amd import _native as N
from trivy_amd import configs
from trivy_amd import secret as S

# name -> (user rules, x_step knob or None, states, classes, packed, K1X literals)
# (states x classes x 2 bytes: packed up to 65,536, legacy up to the plan's 98,304)
SETS = {
    "builtin": (0, None, 515, 43, 1, 0),
    "user20": (20, None, 704, 44, 1, 0),
    "user30": (30, None, 784, 44, 0, 0),       # 68,992 bytes: just past packed
    "user60": (60, None, 1018, 44, 0, 0),
    "user70": (70, None, 1104, 44, 0, 0),      # 97,152 bytes: 1,152 under the cap
    "user100": (100, None, 697, 44, 1, 71),
    "user1000": (1000, None, 697, 44, 1, 979),
    "user1000 x_step 4": (1000, "4", 1114, 38, 0, 833),
}
# the device tests' names
L30, L70, LX, PW, BUILTIN = "user30", "user70", "user1000 x_step 4", "user1000", "builtin"
KW_TABLE_CAP = 96 * 1024   # PlanOptions::max_kw_table_bytes


def doc(name):
    n = SETS[name][0]
    return configs.user_rules_doc(n, seed=4) if n else None


@functools.lru_cache(maxsize=None)
def scanner(name):
    n, step = SETS[name][:2]
    if (n, step) == (1000, None):   # the scanner the K2 record tests already compile
        from tests import gpu_common as GC
        return GC.k2_scanner_for("user", "default")
    # x_step is read when the plan is built, so it is set around the compile alone and not held
    # through the knob fixture (as gpu_common.k2_scanner_for does with its knob).  The reset to
    # None would undo a value a caller holds through the fixture: no test holds x_step while it
    # asks for a scanner here.
    if step is not None:
        N.knob("x_step", step)
    try:
        return S.NewScanner(S.config_from_dict(doc(name)) if n else None)
    finally:
        if step is not None:
            N.knob("x_step", None)


def layout(name):
    """k1_layout_of the set's keyword automaton."""
    i = scanner(name).info()
    return S.k1_layout_of(i["kw_states"], i["kw_classes"])


def is_legacy(lay):
    """The one legacy kernel that is built: the 156 KiB image with replicated class words."""
    return (lay["packed"], lay["lds_class"], lay["rep"], lay["lds_kib"], lay["threads"]) == (0, 2, 1, 156, 1024)


def is_packed(lay):
    return (lay["packed"], lay["lds_kib"], lay["threads"]) == (1, 128, 1024)
