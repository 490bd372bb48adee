"""Batched small-circuit prover (plk_prover_prove_batch / plk_prover_rounds_batch and their _dev forms)
without a GPU: the exports, the argument checks that come before any device query, the exit messages
(check_status's strings, prove.hip) and the wrapper's length checks."""
import ctypes as C

import numpy as np
import pytest

NEW = ("plk_prove_exit_message", "plk_prover_batch_path", "plk_prover_prove_batch", "plk_prover_rounds_batch",
       "plk_prover_prove_batch_dev", "plk_prover_rounds_batch_dev")

# the exits by number with the text check_status sets and the code it returns
ARG, RANGE = 2, 3
EXITS = {1: ("Constraint %u not satisfied.", ARG),
         2: ("Invalid copy_of type", ARG),
         3: ("SRS length is less than polynomial length", RANGE),
         4: ("assertion acc_x(omega^n) == 1 failed", ARG),
         5: ("Non-zero remainder in t(x) division", ARG),
         6: ("Invalid slice indices in poly_slice", RANGE),
         7: ("assertion poly_is_zero(&rem1) failed", ARG),
         8: ("assertion poly_is_zero(&rem2) failed", ARG)}


def test_exports_and_signatures():
    import plonkhip as h
    lib = h.lib()
    for name in NEW:
        assert name in h.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("prove_batch", "rounds_batch", "prove_batch_dev", "rounds_batch_dev", "batch_path"):
        assert hasattr(h.Prover, name), name
    assert hasattr(h, "prove_exit_message")
    with open(h.LIB_PATH, "rb") as f:
        assert b"prove_batch_kernel" in f.read()       # the fused kernel is in the library


def _bufs(batch=2, n=4):
    u8 = lambda k: (C.c_uint8 * max(k, 1))()
    return dict(in_=u8(14 * n * batch), chals=u8(5 * batch), rands=u8(9 * batch), proofs=u8(34 * batch),
                status=(C.c_uint32 * max(batch, 1))())


def _call(lib, name, p, b, batch, flags=0):
    f = getattr(lib, name)
    if name.endswith("_dev"):
        args = [C.cast(x, C.c_void_p) if x is not None else None
                for x in (b["in_"], b["chals"], b["rands"], b["proofs"], b["status"])]
        if "rounds" in name:
            return f(p, args[0], args[1], args[2], flags, batch, args[3], args[4], None)
        return f(p, args[0], args[1], args[2], batch, args[3], args[4], None)
    if "rounds" in name:
        return f(p, b["in_"], b["chals"], b["rands"], flags, batch, b["proofs"], b["status"])
    return f(p, b["in_"], b["chals"], b["rands"], batch, b["proofs"], b["status"])


CALLS = NEW[2:]


@pytest.mark.parametrize("name", CALLS)
def test_null_prover_is_arg_error(name):
    import plonkhip as h
    assert _call(h.lib(), name, None, _bufs(), 2) == h.PLK_ERR_ARG
    assert name in h.last_error()


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("case", ["in_", "chals", "rands", "proofs", "status", "batch0", "batch_negative"])
def test_arg_errors_come_before_any_device_query(name, case):
    """a non-NULL handle the calls must never look into: their argument checks return first"""
    import plonkhip as h
    fake = (C.c_uint8 * 4096)()
    b = _bufs()
    batch = {"batch0": 0, "batch_negative": -5}.get(case, 2)
    if case in b:
        b[case] = None
    assert _call(h.lib(), name, C.addressof(fake), b, batch) == h.PLK_ERR_ARG


@pytest.mark.parametrize("name", CALLS)
def test_batch_above_2_24_is_range_error(name):
    import plonkhip as h
    fake = (C.c_uint8 * 4096)()
    assert _call(h.lib(), name, C.addressof(fake), _bufs(), (1 << 24) + 1) == h.PLK_ERR_RANGE


def test_rounds_batch_refuses_the_preprocessed_flag():
    import plonkhip as h
    fake = (C.c_uint8 * 4096)()
    for name in ("plk_prover_rounds_batch", "plk_prover_rounds_batch_dev"):
        assert _call(h.lib(), name, C.addressof(fake), _bufs(), 2, flags=h.PLK_PROVE_PREPROCESSED) == h.PLK_ERR_ARG


def test_batch_path_null_prover():
    import plonkhip as h
    assert h.lib().plk_prover_batch_path(None, 1) == -h.PLK_ERR_ARG
    assert h.lib().plk_prover_batch_path(None, 0) == -h.PLK_ERR_ARG


@pytest.mark.parametrize("kind", sorted(EXITS))
def test_exit_messages_are_check_status_strings(kind):
    import plonkhip as h
    text, code = EXITS[kind]
    for gate in ((0, 3, 15) if kind == 1 else (0,)):
        want = text % gate if kind == 1 else text
        word = code | (kind << 8) | (gate << 16)
        assert h.prove_exit_message(word) == want
        buf = C.create_string_buffer(b"\xff" * 64, 64)
        assert h.lib().plk_prove_exit_message(word, buf, 64) == len(want)
        assert buf.value.decode() == want
        # a short cap: truncated, NUL-terminated, nothing written past cap, the full length returned
        short = C.create_string_buffer(b"\xff" * 16, 16)
        assert h.lib().plk_prove_exit_message(word, short, 8) == len(want)
        assert short.raw[:8] == want.encode()[:7] + b"\0" and short.raw[8:] == b"\xff" * 8
        assert h.lib().plk_prove_exit_message(word, None, 0) == len(want)


def test_exit_message_edges():
    import plonkhip as h
    assert h.prove_exit_message(0) == ""
    assert h.prove_exit_message(ARG | (9 << 8)) != ""            # INPUT: the batch's own exit
    for bad in (ARG, ARG | (10 << 8), ARG | (255 << 8)):
        assert h.lib().plk_prove_exit_message(bad, None, 0) == -h.PLK_ERR_ARG
        with pytest.raises(ValueError):
            h.prove_exit_message(bad)


def _shell(n=4):
    """a Prover object without a handle: the wrapper's checks raise before the library is called"""
    import plonkhip as h
    p = h.Prover.__new__(h.Prover)
    p._h = C.c_void_p()
    p.n = n
    return p


def test_wrapper_length_checks():
    p = _shell(4)
    ok = dict(c=np.zeros(2 * 56, np.uint8), ch=np.zeros(10, np.uint8), rd=np.zeros(18, np.uint8))
    for c, ch, rd in ((ok["c"][:-1], ok["ch"], ok["rd"]), (ok["c"], ok["ch"][:-1], ok["rd"]),
                      (ok["c"], ok["ch"], ok["rd"][:-1]), (ok["c"], np.zeros(0, np.uint8), ok["rd"]),
                      (np.zeros(3 * 56, np.uint8), ok["ch"], ok["rd"])):
        with pytest.raises(ValueError):
            p.prove_batch(c, ch, rd)
    polys = np.zeros(2 * 52, np.uint8)
    for pl, ch, rd in ((polys[:-1], ok["ch"], ok["rd"]), (polys, ok["ch"][:5], ok["rd"]), (polys, ok["ch"], ok["rd"][:9])):
        with pytest.raises(ValueError):
            p.rounds_batch(pl, ch, rd)
    with pytest.raises(ValueError):
        p.prove_batch_dev(0, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError):
        p.rounds_batch_dev(0, 0, 0, -1, 0, 0)
