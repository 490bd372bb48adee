"""KZG per-point openings (plk_kzg_points_count, plk_kzg_points_workspace, plk_kzg_open_points_batch*) without
a GPU: the exports, the host-only calls, the argument checks that come before any device query, and no CPU
fallback (an opening needs a resident SRS, and without a device there is none: PLK_ERR_NODEV)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import kzg_points_model as PM
from conftest import ROOT

NEW = ("plk_kzg_points_count", "plk_kzg_points_workspace", "plk_kzg_open_points_batch", "plk_kzg_open_points_batch_dev")
FULL = PM.FULL


def test_exports_and_signatures():
    import plonkhip as h
    lib = h.lib()
    for name in NEW:
        assert name in h.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("kzg_points_count", "kzg_points_workspace", "kzg_open_points", "kzg_open_points_dev"):
        assert hasattr(h, name), name
    assert len(h.SIGNATURES["plk_kzg_open_points_batch"][1]) == 8
    assert len(h.SIGNATURES["plk_kzg_open_points_batch_dev"][1]) == 11
    with open(os.path.join(ROOT, "include", "plonkhip.h")) as f:
        txt = f.read()
    assert "#define PLK_KZG_POINTS_LAUNCH_POLYS %d " % h.PLK_KZG_POINTS_LAUNCH_POLYS in txt
    assert h.PLK_KZG_POINTS_LAUNCH_POLYS >= 1


def test_points_count():
    import plonkhip as h
    lib = h.lib()
    assert h.kzg_points_count([1]) == 1 and h.kzg_points_count([1 << 16]) == 1
    assert h.kzg_points_count([FULL]) == 17                       # all 17 bits is a set here
    assert h.kzg_points_count([FULL] * 5) == 85
    assert h.kzg_points_count([0b11, 0b101000, FULL & ~1]) == 2 + 2 + 16
    sets = [1, 2, 0b110, FULL, 0x10001, 0x0F0F0]
    assert h.kzg_points_count(sets) == PM.count(sets) == sum(bin(m).count("1") for m in sets)
    assert PM.expand([0b101, 0b10])[:3] == [(0, 0), (0, 2), (1, 1)]
    for bad in (0, 1 << 17, FULL | 1 << 17, 0xFFFFFFFF, 1 << 31):
        assert h.kzg_points_count([3, bad, 5]) == 0 == PM.count([3, bad, 5]), bad
    assert h.kzg_points_count([]) == 0
    assert lib.plk_kzg_points_count(None, 3) == 0
    assert lib.plk_kzg_points_count((C.c_uint32 * 2)(1, 1), -1) == 0


def test_workspace_is_host_only_and_grows_with_popcount_times_chunks():
    import plonkhip as h
    lib = h.lib()
    ws = h.kzg_points_workspace
    assert ws([], []) == 0
    assert lib.plk_kzg_points_workspace(None, (C.c_uint32 * 1)(1), 1) == 0
    assert lib.plk_kzg_points_workspace((C.c_size_t * 1)(5), None, 1) == 0
    assert lib.plk_kzg_points_workspace((C.c_size_t * 1)(5), (C.c_uint32 * 1)(1), 0) == 0
    assert ws([5, 0], [1, 1]) == 0
    for bad in (0, 1 << 17, 0xFFFFFFFF):
        assert ws([9000, 9000], [1, bad]) == 0, bad
    # nothing is needed when every polynomial fits one chunk, whatever the sets
    assert ws([1, 17, 4095, 4096], [1, FULL, 0b110, FULL]) == 0
    one = ws([4097], [1])
    assert one > 0 and one % 256 == 0
    assert ws([4097, 4096, 5], [1, FULL, FULL]) == one             # one-chunk neighbours add nothing
    # exact up to the rounding: 4 bytes per (point + non-zero point, chunk)
    for lens, sets in (([1 << 20], [FULL]), ([1 << 22], [1]), ([1 << 22], [2]), ([1 << 22, 4097, 100], [0b1011, FULL, 7]),
                       ([8193] * 9, [FULL] * 9)):
        words = PM.workspace_words(lens, sets)
        assert 4 * words <= ws(lens, sets) < 4 * words + 256, (lens, sets)
    by_points = [ws([1 << 22], [(1 << t) - 1]) for t in range(1, 18)]
    assert by_points == sorted(by_points) and len(set(by_points)) == 17
    # (33 words a chunk here, rounded to 256 bytes: two chunks more are always visible)
    by_chunks = [ws([n], [FULL]) for n in (4097, 3 * 4096 + 1, 1 << 16, 1 << 20, (1 << 20) + 8192, 1 << 22)]
    assert by_chunks == sorted(by_chunks) and len(set(by_chunks)) == 6
    assert ws([1 << 22], [FULL]) >= 4 * 33 * 1024
    assert ws([1 << 22] * 2, [FULL] * 2) > ws([1 << 22], [FULL])


# ------------------------------------------------------------------ argument checks, no device
def _opaque_handle():
    """a non-NULL handle the calls under test must never look into: their argument checks return first"""
    return (C.c_uint8 * 256)()


class OpenArgs:
    """ctypes blocks of three polynomials that a failing call never reads"""

    def __init__(self, n=3, length=4):
        self.bufs = [(C.c_uint8 * length)() for _ in range(n)]
        self.ptrs = (C.POINTER(C.c_uint8) * n)(*[C.cast(b, C.POINTER(C.c_uint8)) for b in self.bufs])
        self.vptrs = (C.c_void_p * n)(*[C.addressof(b) for b in self.bufs])
        self.lens = (C.c_size_t * n)(*[length] * n)
        self.sets = (C.c_uint32 * n)(*[0b101] * n)
        self.n = n
        self.zs = (C.c_uint8 * (17 * n))()
        self.ys = (C.c_uint8 * (17 * n))()
        self.out = (C.c_uint8 * (51 * n))()
        self.status = (C.c_uint8 * (17 * n))()

    def call(self, h, s, dev, drop=None, n=None):
        a = {k: (None if drop == k else getattr(self, k)) for k in ("lens", "sets", "zs", "ys", "out", "status")}
        n = self.n if n is None else n
        if dev:
            polys = None if drop == "polys" else self.vptrs
            adr = {k: (None if a[k] is None else C.addressof(a[k])) for k in ("zs", "ys", "out", "status")}
            return h.lib().plk_kzg_open_points_batch_dev(s, polys, a["lens"], a["sets"], n, adr["zs"], adr["ys"], adr["out"],
                                                         adr["status"], None, None)
        polys = None if drop == "polys" else self.ptrs
        return h.lib().plk_kzg_open_points_batch(s, polys, a["lens"], a["sets"], n, a["zs"], a["ys"], a["out"])


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_null_handle_is_arg_error(dev):
    import plonkhip as h
    assert OpenArgs().call(h, None, dev) == h.PLK_ERR_ARG
    assert "plk_kzg_open_points_batch" in h.last_error()


CASES = ["n0", "n_negative", "null_polys", "null_lens", "null_sets", "null_ys", "null_out", "len0", "mask0",
         "mask_bit17", "mask_bit31", "mask_all_and_bit17"]


@pytest.mark.parametrize("case,dev", [(c, d) for c in CASES for d in (False, True)] + [("null_status", True)])
def test_arg_errors_come_before_any_device_query(case, dev):
    import plonkhip as h
    fake = _opaque_handle()
    s = C.addressof(fake)
    a = OpenArgs()
    drop, n = None, None
    if case == "n0":
        n = 0
    elif case == "n_negative":
        n = -2
    elif case.startswith("null_"):
        drop = case[5:]
    elif case == "len0":
        a.lens[1] = 0
    elif case == "mask0":
        a.sets[2] = 0
    elif case == "mask_bit17":
        a.sets[1] = 1 << 17 | 1
    elif case == "mask_bit31":
        a.sets[0] = 1 << 31
    elif case == "mask_all_and_bit17":
        a.sets[2] = FULL | 1 << 17
    assert a.call(h, s, dev, drop, n) == h.PLK_ERR_ARG, case
    assert "plk_kzg_open_points_batch" in h.last_error()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_range_errors_of_a_zeroed_handle(dev):
    """zs may be NULL and all 17 bits is a set: such a call passes the argument checks and reaches the range
    check, which a handle of zero bytes (an SRS of no points) fails with the reference's text"""
    import plonkhip as h
    fake = _opaque_handle()
    a = OpenArgs()
    a.sets[0] = FULL
    assert a.call(h, C.addressof(fake), dev, drop="zs") == h.PLK_ERR_RANGE
    assert "degree exceeds SRS size" in h.last_error()


_NODEV_CHILD = r"""
import sys
sys.path[:0] = %r
import test_kzg_points_cpu as t
import plonkhip as h
assert h.device_count() == 0, "the device is still visible"
print("code", t.open_without_device(h))
"""


def open_without_device(h):
    try:
        with h.Srs([1, 2, 0] * 4) as s:
            h.kzg_open_points(s, [[1, 2, 3]], [0b111])
    except h.PlonkHipError as e:
        return e.code
    return h.PLK_OK


def test_no_cpu_fallback():
    """in this process when it has no device; otherwise in one child process that hides it"""
    import plonkhip as h
    if h.device_count() == 0:
        code = open_without_device(h)
    else:
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        paths = [os.path.dirname(os.path.abspath(__file__))] + [p for p in sys.path if p.startswith(ROOT)]
        out = subprocess.run([sys.executable, "-c", _NODEV_CHILD % (paths,)], env=env, capture_output=True, text=True,
                             timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        code = int(out.stdout.split("code", 1)[1].split()[0])
    assert code == h.PLK_ERR_NODEV
