"""KZG over a resident SRS (plk_srs_* / plk_kzg_*) without a GPU: the exports, the argument checks that
come before any device query, the host-only workspace size, and no CPU fallback."""
import ctypes as C

import pytest

NEW = ("plk_srs_create", "plk_srs_destroy", "plk_srs_len", "plk_srs_irregular", "plk_kzg_commit_batch",
       "plk_kzg_open_batch", "plk_kzg_workspace", "plk_kzg_commit_batch_dev", "plk_kzg_open_batch_dev")


def test_exports_and_signatures():
    import plonkhip as h
    lib = h.lib()
    for name in NEW:
        assert name in h.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in ("Srs", "kzg_commit", "kzg_open", "kzg_workspace", "kzg_commit_dev", "kzg_open_dev"):
        assert hasattr(h, name), name


def _args(n, length=4, z=1):
    """ctypes blocks of n jobs (host buffers that are never read when the call fails its checks)"""
    bufs = [(C.c_uint8 * max(length, 1))() for _ in range(max(n, 1))]
    ptrs = (C.POINTER(C.c_uint8) * max(n, 1))(*[C.cast(b, C.POINTER(C.c_uint8)) for b in bufs])
    vptrs = (C.c_void_p * max(n, 1))(*[C.addressof(b) for b in bufs])
    lens = (C.c_size_t * max(n, 1))(*[length] * max(n, 1))
    zs = (C.c_uint8 * max(n, 1))(*[z] * max(n, 1))
    return bufs, ptrs, vptrs, lens, zs


def test_null_handle_is_arg_error_without_device():
    import plonkhip as h
    lib = h.lib()
    bufs, ptrs, vptrs, lens, zs = _args(2)
    out = (C.c_uint8 * 6)()
    ys = (C.c_uint8 * 2)()
    assert lib.plk_kzg_commit_batch(None, ptrs, lens, 2, out) == h.PLK_ERR_ARG
    assert "plk_kzg_commit_batch" in h.last_error()
    assert lib.plk_kzg_open_batch(None, ptrs, lens, zs, 2, ys, out) == h.PLK_ERR_ARG
    assert lib.plk_kzg_commit_batch_dev(None, vptrs, lens, 2, None, None) == h.PLK_ERR_ARG
    assert lib.plk_kzg_open_batch_dev(None, vptrs, lens, zs, 2, None, None, None, None, None) == h.PLK_ERR_ARG


def _opaque_handle():
    """a non-NULL handle the calls under test must never look into: their argument checks return first"""
    return (C.c_uint8 * 256)()


@pytest.mark.parametrize("case", ["n0", "n_negative", "len0", "z17", "null_lens", "null_polys", "null_zs"])
def test_arg_errors_come_before_any_device_query(case):
    import plonkhip as h
    lib = h.lib()
    fake = _opaque_handle()
    s = C.addressof(fake)
    n = {"n0": 0, "n_negative": -3}.get(case, 3)
    bufs, ptrs, vptrs, lens, zs = _args(3)
    if case == "len0":
        lens[1] = 0
    if case == "z17":
        zs[2] = 17
    out = (C.c_uint8 * 9)()
    ys = (C.c_uint8 * 3)()
    a_lens = None if case == "null_lens" else lens
    a_ptrs = None if case == "null_polys" else ptrs
    a_vptrs = None if case == "null_polys" else vptrs
    a_zs = None if case == "null_zs" else zs
    assert lib.plk_kzg_open_batch(s, a_ptrs, a_lens, a_zs, n, ys, out) == h.PLK_ERR_ARG
    assert lib.plk_kzg_open_batch_dev(s, a_vptrs, a_lens, a_zs, n, None, None, None, None, None) == h.PLK_ERR_ARG
    if case not in ("z17", "null_zs"):
        assert lib.plk_kzg_commit_batch(s, a_ptrs, a_lens, n, out) == h.PLK_ERR_ARG
        assert lib.plk_kzg_commit_batch_dev(s, a_vptrs, a_lens, n, None, None) == h.PLK_ERR_ARG


def test_workspace_is_host_only_and_grows_with_the_chunk_count():
    import plonkhip as h
    assert h.kzg_workspace([]) == 0
    assert h.lib().plk_kzg_workspace(None, 3) == 0
    one = h.kzg_workspace([4096])
    assert one > 0 and one % 256 == 0
    assert h.kzg_workspace([1]) == one                         # one chunk either way
    sizes = [h.kzg_workspace([n]) for n in (4096, 4097, 1 << 20, (1 << 20) + 1, 1 << 22)]
    assert sizes == sorted(sizes)
    assert sizes[2] >= 4 * ((1 << 20) // 4096) and sizes[4] >= 4 * ((1 << 22) // 4096)
    assert sizes[3] > sizes[2] or sizes[3] >= 4 * 257            # (rounded to 256 bytes)
    assert h.kzg_workspace([1 << 20] * 9) >= 9 * 4 * 256
    assert h.kzg_workspace([1 << 22] * 2) > h.kzg_workspace([1 << 22])


def test_srs_handle_edges_without_device():
    import plonkhip as h
    lib = h.lib()
    assert lib.plk_srs_len(None) == 0
    assert lib.plk_srs_irregular(None) == 0
    lib.plk_srs_destroy(None)                                  # no-op
    hnd = C.c_void_p()
    pts = (C.c_uint8 * 3)(1, 2, 0)
    assert lib.plk_srs_create(None, 1, C.byref(hnd)) == h.PLK_ERR_ARG
    assert lib.plk_srs_create(pts, 0, C.byref(hnd)) == h.PLK_ERR_ARG
    assert lib.plk_srs_create(pts, 1, None) == h.PLK_ERR_ARG
    with pytest.raises(ValueError):
        h.Srs([1, 2, 0, 1])


def test_srs_create_without_gpu_is_nodev():
    import plonkhip as h
    if h.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(h.PlonkHipError) as e:
        h.Srs([1, 2, 0])
    assert e.value.code == h.PLK_ERR_NODEV
