"""Pairings and KZG verification (plk_pairing_batch*, plk_kzg_verify_batch*) on the GPU.

Expected values are the reference's own outputs recorded in tests/golden/pairing.json, and the Python
model of tests/pairing_model.py (pinned to that file by tests/test_pairing_cpu.py) where a test needs
a shape the file does not hold.  Everything is exact: bytes are compared for equality."""
import numpy as np
import pytest

import gen
import pairing_model as M
from conftest import load_golden

pytestmark = pytest.mark.gpu

GUARD = 32
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, (1 << 20) + 1]
POSITIONS = {"first": 0, "block_edge": 255, "last": 256}     # of a 257-job batch, 256 lanes per block


class Gold:
    def __init__(self):
        g = load_golden("pairing.json")
        self.g2m = {int(k): tuple(bytes.fromhex(v)) for k, v in g["g2_multiples"].items()}
        pts = gen.all_points()
        h = np.array([self.g2m[k] for k in range(1, 17)], np.uint8)
        self.table_in = np.concatenate([np.repeat(pts, 16, 0), np.tile(h, (len(pts), 1))], 1)
        self.table_out = np.frombuffer(bytes.fromhex(g["table"]), np.uint8).reshape(-1, 2)
        self.raw_in = np.frombuffer(bytes.fromhex(g["raw"]["inputs"]), np.uint8).reshape(-1, 5)
        self.raw_out = np.frombuffer(bytes.fromhex(g["raw"]["out"]), np.uint8).reshape(-1, 2)
        self.ex_vk = bytes.fromhex(g["verify_exhaustive"]["vk"])
        self.ex_bits = np.unpackbits(np.frombuffer(bytes.fromhex(g["verify_exhaustive"]["bits"]), np.uint8),
                                     bitorder="little")[:17 ** 4]
        self.vr_jobs = np.frombuffer(bytes.fromhex(g["verify_raw"]["jobs"]), np.uint8).reshape(-1, 15)
        self.vr_bits = np.array([int(c) for c in g["verify_raw"]["bits"]], np.uint8)


@pytest.fixture(scope="module")
def gold():
    return Gold()


def vk_of(hip, b):
    b = bytes(b)
    return hip.KzgVk(b[0:3], b[3:5], b[5:7])


def on_device(a, offset=0, fill=None, guard=0):
    """a byte array on the device starting `offset` bytes past a 16-byte boundary (fill: an output
    block of that many 0xEE bytes instead, with `guard` more behind it)"""
    import torch
    n = a if fill else a.size
    t = torch.full((offset + n + guard + 16,), 0xEE, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    if not fill:
        t[offset:offset + n] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    return t[offset:]


def taken(t, n):
    """the n output bytes of block t, after checking that the guard behind them is untouched"""
    h = t.cpu().numpy()
    assert (h[n:n + GUARD] == 0xEE).all(), "wrote past the output"
    return h[:n].copy()


def pairing_dev(hip, g1, g2, offset=0, stream=None):
    import torch
    n = g1.size // 3
    d1, d2 = on_device(g1, offset), on_device(g2, offset)
    out = on_device(2 * n, offset, fill=True, guard=GUARD)
    torch.cuda.synchronize()
    hip.pairing_dev(d1, d2, n, out, stream=stream)
    torch.cuda.synchronize()
    return taken(out, 2 * n).reshape(n, 2)


def verify_dev(hip, vk, c, z, y, w, offset=0, stream=None):
    import torch
    n = z.size
    d = [on_device(np.asarray(a, np.uint8), offset) for a in (c, z, y, w)]
    ok = on_device(n, offset, fill=True, guard=GUARD)
    torch.cuda.synchronize()
    hip.kzg_verify_dev(vk, d[0], d[1], d[2], d[3], n, ok, stream=stream)
    torch.cuda.synchronize()
    return taken(ok, n)


def pairing_both(hip, jobs, form):
    g1, g2 = np.ascontiguousarray(jobs[:, :3]), np.ascontiguousarray(jobs[:, 3:])
    return hip.pairing(g1, g2) if form == "host" else pairing_dev(hip, g1, g2)


def verify_both(hip, vk, jobs, form, offset=0):
    """jobs: n x 8 bytes {C 3, W 3, z, y}"""
    c, w = np.ascontiguousarray(jobs[:, 0:3]), np.ascontiguousarray(jobs[:, 3:6])
    z, y = np.ascontiguousarray(jobs[:, 6]), np.ascontiguousarray(jobs[:, 7])
    return hip.kzg_verify(vk, c, z, y, w) if form == "host" else verify_dev(hip, vk, c, z, y, w, offset)


# ------------------------------------------------------------------ pairing against the goldens
@pytest.mark.parametrize("form", ["host", "dev"])
def test_pairing_table(hip, gold, form):
    got = pairing_both(hip, gold.table_in, form)
    assert np.array_equal(got, gold.table_out)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_pairing_raw(hip, gold, form):
    got = pairing_both(hip, gold.raw_in, form)
    bad = np.flatnonzero((got != gold.raw_out).any(1))
    assert bad.size == 0, (bad[:8], gold.raw_in[bad[:8]], got[bad[:8]], gold.raw_out[bad[:8]])


@pytest.mark.parametrize("n", SIZES)
def test_pairing_batch_sizes(hip, gold, n):
    reps = -(-n // len(gold.raw_in))
    jobs = np.tile(gold.raw_in, (reps, 1))[:n]
    exp = np.tile(gold.raw_out, (reps, 1))[:n]
    assert np.array_equal(pairing_both(hip, jobs, "dev"), exp)
    assert np.array_equal(pairing_both(hip, jobs, "host"), exp)


def ex_jobs(gold):
    kg = np.array(gen.KG, np.uint8)
    c, w, z, y = (v.reshape(-1) for v in np.meshgrid(*[np.arange(17)] * 4, indexing="ij"))
    return np.concatenate([kg[c], kg[w], z[:, None].astype(np.uint8), y[:, None].astype(np.uint8)], 1)


@pytest.mark.parametrize("n", SIZES)
def test_verify_batch_sizes(hip, gold, n):
    """the exhaustive cases from a start where accepts and rejects mix, tiled"""
    base = ex_jobs(gold)
    reps = -(-n // len(base))
    jobs = np.tile(base, (reps, 1))[:n]
    exp = np.tile(gold.ex_bits, reps)[:n]
    assert np.array_equal(verify_both(hip, vk_of(hip, gold.ex_vk), jobs, "dev"), exp)


# ------------------------------------------------------------------ device-buffer edges
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_unaligned_device_buffers_and_guards(hip, gold, offset):
    jobs = gold.raw_in[:257]
    got = pairing_dev(hip, np.ascontiguousarray(jobs[:, :3]), np.ascontiguousarray(jobs[:, 3:]), offset)
    assert np.array_equal(got, gold.raw_out[:257])
    base = ex_jobs(gold)[4000:4257]
    assert np.array_equal(verify_both(hip, vk_of(hip, gold.ex_vk), base, "dev", offset), gold.ex_bits[4000:4257])


# ------------------------------------------------------------------ invalid encodings
PAIRING_INVALID = {"g1_x_101": (0, 101), "g1_y_101": (1, 101), "g1_x_255": (0, 255), "g1_y_255": (1, 255),
                   "g1_flag_2": (2, 2), "g2_x_101": (3, 101), "g2_y_101": (4, 101), "g2_x_255": (3, 255),
                   "g2_y_255": (4, 255)}


@pytest.mark.parametrize("where", sorted(POSITIONS))
@pytest.mark.parametrize("kind", sorted(PAIRING_INVALID))
def test_pairing_invalid_encoding(hip, gold, kind, where):
    col, val = PAIRING_INVALID[kind]
    pos = POSITIONS[where]
    jobs = gold.raw_in[:257].copy()
    jobs[pos, col] = val
    exp = gold.raw_out[:257].copy()
    exp[pos] = 0xFF
    assert M.pairing_bytes(jobs[pos, :3].tolist(), jobs[pos, 3:].tolist()) == (0xFF, 0xFF)
    for form in ("host", "dev"):
        assert np.array_equal(pairing_both(hip, jobs, form), exp), form


VERIFY_INVALID = {"c_x_101": (0, 101), "c_y_255": (1, 255), "c_flag_2": (2, 2), "w_x_255": (3, 255),
                  "w_y_101": (4, 101), "w_flag_2": (5, 2), "z_17": (6, 17), "y_17": (7, 17), "z_255": (6, 255)}


@pytest.mark.parametrize("where", sorted(POSITIONS))
@pytest.mark.parametrize("kind", sorted(VERIFY_INVALID))
def test_verify_invalid_encoding(hip, gold, kind, where):
    col, val = VERIFY_INVALID[kind]
    pos = POSITIONS[where]
    jobs = ex_jobs(gold)[4000:4257].copy()
    jobs[pos, col] = val
    exp = gold.ex_bits[4000:4257].copy()
    assert 0 < exp.sum() < exp.size
    exp[pos] = 2
    for form in ("host", "dev"):
        assert np.array_equal(verify_both(hip, vk_of(hip, gold.ex_vk), jobs, form), exp), form


# ------------------------------------------------------------------ verify against the goldens
@pytest.mark.parametrize("form", ["host", "dev"])
def test_verify_exhaustive_in_one_launch(hip, gold, form):
    got = verify_both(hip, vk_of(hip, gold.ex_vk), ex_jobs(gold), form)
    bad = np.flatnonzero(got != gold.ex_bits)
    assert bad.size == 0, (bad[:8], got[bad[:8]])
    assert int(got.sum()) == 17 ** 3


def test_verify_raw_dev(hip, gold):
    """every job has its own key, so one launch per job: all queued, one wait"""
    import torch
    jobs = gold.vr_jobs
    n = len(jobs)
    d = {k: on_device(np.ascontiguousarray(jobs[:, a:b])) for k, (a, b) in
         {"c": (7, 10), "w": (10, 13), "z": (13, 14), "y": (14, 15)}.items()}
    ok = on_device(n, fill=True, guard=GUARD)
    torch.cuda.synchronize()
    for i in range(n):
        hip.kzg_verify_dev(vk_of(hip, jobs[i, :7]), d["c"][3 * i:], d["z"][i:], d["y"][i:], d["w"][3 * i:], 1, ok[i:])
    torch.cuda.synchronize()
    got = taken(ok, n)
    bad = np.flatnonzero(got != gold.vr_bits)
    assert bad.size == 0, (bad[:8], jobs[bad[:8]], got[bad[:8]])


def test_verify_raw_host(hip, gold):
    """all 2048 jobs, one synchronous call each (every job has its own key)"""
    jobs = gold.vr_jobs
    got = [int(hip.kzg_verify(vk_of(hip, j[:7]), j[7:10], j[13:14], j[14:15], j[10:13])[0]) for j in jobs]
    assert got == gold.vr_bits.tolist()


def test_host_forms_select_the_library_device(hip, gold):
    """called from a thread whose current device is another GPU, the host forms run on the library's
    device as the other host-buffer entry points do; the _dev forms refuse (PLK_ERR_ARG)"""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU")
    jobs = gold.raw_in[:65]
    base = ex_jobs(gold)[4000:4065]
    d = [on_device(np.ascontiguousarray(jobs[:, :3])), on_device(np.ascontiguousarray(jobs[:, 3:])),
         on_device(130, fill=True, guard=GUARD)]
    torch.cuda.synchronize()
    try:
        torch.cuda.set_device(1)
        with pytest.raises(hip.PlonkHipError) as e:
            hip.pairing_dev(d[0], d[1], 65, d[2])
        assert e.value.code == hip.PLK_ERR_ARG
        assert np.array_equal(pairing_both(hip, jobs, "host"), gold.raw_out[:65])
        torch.cuda.set_device(1)
        assert np.array_equal(verify_both(hip, vk_of(hip, gold.ex_vk), base, "host"), gold.ex_bits[4000:4065])
    finally:
        torch.cuda.set_device(0)


# ------------------------------------------------------------------ end to end with commit and open
E2E_LENGTHS = [1, 2, 3, 17, 4097]
E2E_ZS = [0, 1, 2, 5, 16]


@pytest.fixture(scope="module")
def e2e(hip, gold):
    """a well-formed SRS for s = 2, srs[i] = (2^i mod 17) G, and the library's own commitments and
    openings of every (polynomial, z)"""
    g1 = load_golden("g1.json")["kG_k0_17"]
    srs_pts = np.array([list(bytes.fromhex(g1[pow(2, i, 17)])) for i in range(max(E2E_LENGTHS))], np.uint8)
    polys = [gen.poly_inputs(0xE2E + n, n, 0)[0] for n in E2E_LENGTHS]
    with hip.Srs(srs_pts) as srs:
        assert not srs.irregular
        commits = hip.kzg_commit(srs, polys)
        jobs = [(i, z) for i in range(len(polys)) for z in E2E_ZS]
        ys, proofs = hip.kzg_open(srs, [polys[i] for i, _ in jobs], [z for _, z in jobs])
    vk = hip.KzgVk((1, 2, 0), gold.g2m[1], gold.g2m[2])
    return {"vk": vk, "key": ((1, 2, 0), gold.g2m[1], gold.g2m[2]), "polys": polys, "commits": commits, "jobs": jobs,
            "ys": ys, "proofs": proofs}


def e2e_rows(e, ys=None, proofs=None):
    ys = e["ys"] if ys is None else ys
    proofs = e["proofs"] if proofs is None else proofs
    return np.array([list(e["commits"][i]) + list(proofs[k]) + [z, ys[k]] for k, (i, z) in enumerate(e["jobs"])],
                    np.uint8)


def model_bits(e, rows):
    return np.array([M.kzg_verify(e["key"], tuple(r[0:3]), tuple(r[3:6]), r[6], r[7]) for r in rows.tolist()], np.uint8)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_every_opening_of_the_library_verifies(hip, e2e, form):
    rows = e2e_rows(e2e)
    assert model_bits(e2e, rows).tolist() == [1] * len(rows)
    assert verify_both(hip, e2e["vk"], rows, form).tolist() == [1] * len(rows)
    # a constant polynomial's proof is the identity
    assert all(bytes(p) == bytes([0, 0, 1]) for p, (i, _) in zip(e2e["proofs"], e2e["jobs"]) if i == 0)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_wrong_value_is_rejected(hip, e2e, form):
    rows = e2e_rows(e2e, ys=[(y + 1) % 17 for y in e2e["ys"]])
    assert model_bits(e2e, rows).tolist() == [0] * len(rows)
    assert verify_both(hip, e2e["vk"], rows, form).tolist() == [0] * len(rows)


@pytest.mark.parametrize("form", ["host", "dev"])
def test_another_polynomials_proof(hip, e2e, form):
    """the proof of the next polynomial at the same z: rejected except where the model accepts too"""
    nz = len(E2E_ZS)
    k = len(e2e["jobs"])
    rows = e2e_rows(e2e, proofs=[e2e["proofs"][(j + nz) % k] for j in range(k)])
    exp = model_bits(e2e, rows)
    assert (exp == 0).sum() >= k // 2
    assert np.array_equal(verify_both(hip, e2e["vk"], rows, form), exp)


# ------------------------------------------------------------------ streams and determinism
def test_non_default_stream(hip, gold):
    import torch
    s = torch.cuda.Stream()
    jobs = gold.raw_in[:1000]
    got = pairing_dev(hip, np.ascontiguousarray(jobs[:, :3]), np.ascontiguousarray(jobs[:, 3:]), stream=s)
    assert np.array_equal(got, gold.raw_out[:1000])
    base = ex_jobs(gold)[:5000]
    c, w = np.ascontiguousarray(base[:, 0:3]), np.ascontiguousarray(base[:, 3:6])
    got = verify_dev(hip, vk_of(hip, gold.ex_vk), c, np.ascontiguousarray(base[:, 6]), np.ascontiguousarray(base[:, 7]), w,
                     stream=s)
    assert np.array_equal(got, gold.ex_bits[:5000])


def test_two_streams_two_outputs(hip, gold):
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, b = gold.raw_in[:512], gold.raw_in[512:]
    da = [on_device(np.ascontiguousarray(a[:, :3])), on_device(np.ascontiguousarray(a[:, 3:]))]
    db = [on_device(np.ascontiguousarray(b[:, :3])), on_device(np.ascontiguousarray(b[:, 3:]))]
    oa, ob = on_device(1024, fill=True, guard=GUARD), on_device(1024, fill=True, guard=GUARD)
    torch.cuda.synchronize()
    hip.pairing_dev(da[0], da[1], 512, oa, stream=s1)
    hip.pairing_dev(db[0], db[1], 512, ob, stream=s2)
    s1.synchronize()
    s2.synchronize()
    assert np.array_equal(taken(oa, 1024).reshape(-1, 2), gold.raw_out[:512])
    assert np.array_equal(taken(ob, 1024).reshape(-1, 2), gold.raw_out[512:])


def test_repeated_call_gives_identical_bytes(hip, gold):
    first = pairing_both(hip, gold.raw_in, "dev")
    assert np.array_equal(pairing_both(hip, gold.raw_in, "dev"), first)
    vk = vk_of(hip, gold.ex_vk)
    base = ex_jobs(gold)[:4096]
    v1 = verify_both(hip, vk, base, "dev")
    assert np.array_equal(verify_both(hip, vk, base, "dev"), v1)
    assert np.array_equal(verify_both(hip, vk, base, "host"), v1)
