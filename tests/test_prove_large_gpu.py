"""Device prover (plk_prover_rounds_dev) at the gate counts where its round-3 plan switches, past
the 2^16 / 2^20 the rest of the suite proves at: tile width, which products share an inverse
transform, the transforms' field, and the largest n one transform holds exactly (the switch table
in tests/prove_large_cases.py).  The answers are the CPU oracle's, recorded in
tests/golden/prove_large.json (2 .. 80 s of oracle time a case); that each size really took the
plan the table names is read from the NTT launch log (PLK_OPT_NTT_LAUNCH_LOG), whose expected
records follow from the plan rules (tests/test_prove_large_cpu.py), not from a device run.
Most of a test's time is the host generating the instance (0.3 - 2 s); a proof takes milliseconds."""
import pytest
import torch

import gen
import prove_large_cases as PL
from conftest import load_golden
from prove_ref import Prover as RefProver, ProveError
from test_prove_gpu import _SWEEP, _odd_qm

pytestmark = pytest.mark.gpu

_GOLD = {(c["n"], c["seed"]): c for c in load_golden("prove_large.json")["cases"]}
_PRE = sorted(PL.QM_TRANSFORM_USED)     # preprocessed = plain = golden: 524288, 1223337, 1835007, 2097152


def _instance(n, seed):
    polys, chal, rnd, zh, pts = gen.prove_instance(n, seed, 2 * n + 8)
    return [torch.from_numpy(p).to("cuda") for p in polys], chal, rnd, zh, pts


def _centres(hip, run):
    """run() with the launch log on: its result and the centre launches in launch order as
    (k, tile bits, field, products, products with inverse passes, lo = 0 pass units)"""
    hip.ntt_launch_log()
    with hip.options(NTT_LAUNCH_LOG=1):
        try:
            got = run()
        finally:
            log = hip.ntt_launch_log()
    out = []
    for r in log:
        if r["kind"] == 2:
            out.append([r["k"], r["tb"], r["field"], r["n"], set(), r["units"]])
        elif r["kind"] == 1:
            # inverse passes follow their centre launch; same size, tiles and field
            assert out and (r["k"], r["tb"], r["field"]) == tuple(out[-1][:3]), (r, out)
            out[-1][4].add(r["n"])
        else:
            assert r["kind"] in (0, 3), r
    for c in out:
        assert len(c[4]) == 1, (c, "every inverse pass of a launch runs the same products")
    return got, [(k, tb, f, nj, inv.pop(), units) for k, tb, f, nj, inv, units in out]


@pytest.mark.parametrize("n,seed", sorted(_GOLD))
def test_golden_and_plan(hip, n, seed):
    """Every golden entry: the oracle's 34 bytes twice over (or PlonkHipError where the reference
    exits: t(x) too short for its slices), and the centre launches PL.LAUNCHES names -- their
    transform sizes, tile widths, fields, and how many products kept inverse passes of their own
    (sum-group members have none).  At 524288, 1223337, 1835007 and 2097152 also preprocessed:
    the same bytes twice, in the same launches, with one lo = 0 pass fewer in (a b) q_m's launch
    exactly where q_m's recorded transform is of that launch's field -- at 1835007 and 2097152 it
    was recorded for F29, the launch runs in BabyBear, and the call transforms q_m itself."""
    g = _GOLD[(n, seed)]
    dev, chal, rnd, zh, pts = _instance(n, seed)
    pr = hip.Prover(n, zh, pts)
    if g["proof"] is None:
        def refused():
            with pytest.raises(hip.PlonkHipError, match=g["exit"]):
                pr.rounds_dev(dev, chal, rnd)
        # (the slices are cut after round 3: the launches are those of the proof beside it)
        _, plan = _centres(hip, refused)
        assert [c[:5] for c in plan] == PL.LAUNCHES[n], plan
        refused()
        pr.close()
        return
    got, plan = _centres(hip, lambda: pr.rounds_dev(dev, chal, rnd))
    assert got.hex() == g["proof"]
    assert pr.rounds_dev(dev, chal, rnd) == got
    assert [c[:5] for c in plan] == PL.LAUNCHES[n], plan
    if n in _PRE:
        pr.preprocess(dev)
        pre, plan_pre = _centres(hip, lambda: pr.rounds_dev(dev, chal, rnd, preprocessed=True))
        assert pre.hex() == g["proof"]
        assert pr.rounds_dev(dev, chal, rnd, preprocessed=True) == pre
        assert [c[:5] for c in plan_pre] == PL.LAUNCHES[n], plan_pre
        qk = PL.product_plan(2 * n + 3, n)[0]
        i = max(j for j, c in enumerate(plan) if c[0] == qk)         # (a b) q_m's launch: the last of its size
        assert plan_pre[i][5] == plan[i][5] - (1 if PL.QM_TRANSFORM_USED[n] else 0), (plan, plan_pre)
        pr.preprocess(None)
        assert pr.rounds_dev(dev, chal, rnd, preprocessed=True).hex() == g["proof"]
    pr.close()


@pytest.mark.parametrize("n", [524288, 2097152])
def test_option_sweep_vs_golden(hip, n):
    """Each switch of test_prove_gpu._SWEEP off its default, plain and preprocessed, where one proof
    runs both tile widths (524288) and where its 4n products run in BabyBear beside F29 ones
    (2097152): the golden bytes every time.  Round 5's generic form (lincomb_batch, then the
    two-launch scan) is no option: q_m as a view one byte into a larger buffer reaches it."""
    assert {("NTT_F29", 0), ("NTT_CENTER_SUM", 0), ("NTT_SHARED_FIX", 0), ("NTT_SHARED_FIX", 2), ("NTT_SHARE", 0),
            ("PROVE_DERIVE_T2A", 0), ("PROVE_DERIVE_T2A", 1)} <= set(_SWEEP)
    want = _GOLD[(n, 51)]["proof"]
    dev, chal, rnd, zh, pts = _instance(n, 51)
    pr = hip.Prover(n, zh, pts)
    for opt, val in _SWEEP:
        with hip.options(**{opt: val}):
            assert pr.rounds_dev(dev, chal, rnd).hex() == want, (opt, val)
    odd = _odd_qm(dev, off=1)
    assert pr.rounds_dev(odd, chal, rnd).hex() == want, "q_m at an odd address"
    pr.preprocess(dev)
    for opt, val in _SWEEP:
        with hip.options(**{opt: val}):
            assert pr.rounds_dev(dev, chal, rnd, preprocessed=True).hex() == want, (opt, val, "pre")
    pr.preprocess(odd)
    assert pr.rounds_dev(odd, chal, rnd, preprocessed=True).hex() == want, "q_m at an odd address, pre"
    pr.close()


def test_helper_2_21_vs_golden(hip):
    """2097152 gates with t_3's chain on a helper prover (the device list repeating device 0, as
    tests/test_prove_helpers_gpu.py rehearses it): the golden bytes"""
    n = 2097152
    hip.init_devices([0, 0])
    try:
        dev, chal, rnd, zh, pts = _instance(n, 51)
        pr = hip.Prover(n, zh, pts)
        pr.attach_helpers(1)
        assert pr.helpers() == 1
        assert pr.rounds_dev(dev, chal, rnd).hex() == _GOLD[(n, 51)]["proof"]
        pr.close()
    finally:
        hip.init_devices([0])


def test_upper_limit(hip, oracle):
    """n = 3,932,159: t_2's operand A2 B2 has 2n + 3 = 7,864,321 coefficients, 256 times that is
    past BabyBear's prime, the product batch has no blocked path, and rounds_dev returns
    PLK_ERR_RANGE from the batch's checks, before any of its transforms is launched (n = 3,932,158
    gives the golden: test_golden_and_plan).  The prover can be destroyed after the error and the
    library proves on."""
    n = PL.N_MAX + 1
    dev, chal, rnd, zh, pts = _instance(n, 51)
    pr = hip.Prover(n, zh, pts)
    with pytest.raises(hip.PlonkHipError, match="outside the exact range") as e:
        pr.rounds_dev(dev, chal, rnd)
    assert e.value.code == hip.PLK_ERR_RANGE
    pr.close()
    del dev
    n = 4096
    polys, chal, rnd, zh, pts = gen.prove_instance(n, 63, 2 * n + 8)
    want = RefProver(oracle, pts.tobytes(), n, z_h=zh.tobytes()).rounds(polys, chal, rnd, strict=False)
    pr = hip.Prover(n, zh, pts)
    assert pr.rounds_dev([torch.from_numpy(p).to("cuda") for p in polys], chal, rnd).hex() == want.hex()
    pr.close()


# 2n + 1 .. 2n + 4 and 4n + 6 around 2^m + 16, the most a wrapped product carries over:
#   n = 2^m + 2: 4n + 6 wrapped by 14        + 3: 4n + 6 = 2^(m+2) + 18, not wrapped
#   n = 2^m + 6: 2n + 4 wrapped by 16        + 7: 2n + 1, 2n + 2 wrapped by 15, 16; 2n + 3, 2n + 4 not
# (seed 81: the reference exits at none of them)
@pytest.mark.parametrize("n", [4098, 4099, 4102, 4103, 65538, 65539, 65542, 65543])
def test_wrap_range_vs_oracle(hip, oracle, n):
    """Wrapped products at the top of the wrap range next to unwrapped ones in one batch, plain and
    preprocessed, against the oracle computed here (under 1 s a case)"""
    m = 1 << (n.bit_length() - 1)
    e2 = [PL.product_plan(n + 2, n)[1], PL.product_plan(n + 3, n)[1], PL.product_plan(n + 2, n + 2)[1],
          PL.product_plan(n + 2, n + 3)[1]]
    e4 = PL.product_plan(2 * n + 3, 2 * n + 4)[1]
    assert (e2, e4) == {2: ([5, 6, 7, 8], 14), 3: ([7, 8, 9, 10], 0), 6: ([13, 14, 15, 16], 0),
                        7: ([15, 16, 0, 0], 0)}[n - m]
    polys, chal, rnd, zh, pts = gen.prove_instance(n, 81, 2 * n + 8)
    try:
        want = RefProver(oracle, pts.tobytes(), n, z_h=zh.tobytes()).rounds(polys, chal, rnd, strict=False)
    except ProveError:
        pytest.fail("seed 81 was chosen so that the reference does not exit")
    dev = [torch.from_numpy(p).to("cuda") for p in polys]
    pr = hip.Prover(n, zh, pts)
    got, plan = _centres(hip, lambda: pr.rounds_dev(dev, chal, rnd))
    assert got.hex() == want.hex()
    assert [c[:5] for c in plan] == PL.prover_launches(n), plan
    pr.preprocess(dev)
    for _ in range(2):
        assert pr.rounds_dev(dev, chal, rnd, preprocessed=True).hex() == want.hex()
    pr.preprocess(None)
    assert pr.rounds_dev(dev, chal, rnd).hex() == want.hex()
    pr.close()
