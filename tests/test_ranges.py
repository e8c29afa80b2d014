"""The fixtures of tests/ranges_ref.py meet their own conditions (CPU): the kernel tests of tests/test_ranges_gpu.py rely on them."""
import pytest
import torch

import ranges_ref as rr


def _finite(d):
    return all(bool(torch.isfinite(v).all()) for v in d.values() if torch.is_tensor(v) and v.is_floating_point())


@pytest.mark.parametrize("Tq,Tk,causal", rr.ATT_SHAPES)
@pytest.mark.parametrize("regime", rr.ATT_REGIMES)
def test_attention_fixtures(regime, Tq, Tk, causal):
    case = rr.attention_case(regime, Tq, Tk, causal)
    assert bool((case["key_valid"][:, 0] == 1).all()) and int((case["key_valid"] == 0).sum()) > 0 or Tk < 10
    for bf in (False, True):
        want, plain32 = rr.attention_math(case, torch.float64, bf), rr.attention_math(case, torch.float32, bf)
        assert _finite(want) and _finite(plain32)
    want, plain32 = rr.attention_math(case, torch.float64), rr.attention_math(case, torch.float32)
    if regime == "planted":                      # every other probability underflows to exactly 0 in fp32
        p = plain32["p"]
        assert bool(((p != 0).sum(-1) == 1).all()) and bool((p.max(-1).values == 1).all())
        s_gap = want["p"].topk(2, dim=-1).values
        assert float((s_gap[..., 1] / s_gap[..., 0]).max()) < 1e-52          # e^-120
    if regime == "sharp":
        assert float(want["p"].max(-1).values.median()) > 0.9
    if regime == "flat":
        n = want["mask"].expand_as(want["p"]).sum(-1).double()
        assert float((want["p"].max(-1).values * n - 1).abs().max()) < 1e-3
    fl = rr.attention_floors(case)
    assert all(f > 0 for f in fl.values())


@pytest.mark.parametrize("M", [37, 530])
def test_gate_fixture(M):
    case = rr.gate_case(M)
    want, plain32 = rr.gate_ref(case, torch.float64), rr.gate_ref(case, torch.float32)
    assert _finite(want) and _finite(plain32)
    d = want["a_minus_b"]
    assert float(d.max()) > 200 and float(d.min()) < -200
    assert bool((d[::5] == 0).all())                                         # q = 0 rows: a = b exactly


@pytest.mark.parametrize("kind", ["cancel", "unit", "saturated", "mixed"])
def test_copy_fixture(kind):
    case = rr.copy_case(kind)
    for masked in (False, True):
        want, plain32 = rr.copy_ref(case, torch.float64, masked), rr.copy_ref(case, torch.float32, masked)
        assert _finite(want) and _finite(plain32)
    if kind == "saturated":                      # 1 - th^2 is exactly 0 in fp32 for most elements
        x = (case["src"][:, None] + case["tgt"][:, :, None])
        assert float((1 - torch.tanh(x) ** 2 == 0).float().mean()) > 0.7
    x = rr.tanh_sweep()
    assert float(x.min()) == -100 and float(x.max()) == 100 and bool(((x.abs() > 8.6e-3) & (x.abs() < 1e-2)).any())


@pytest.mark.parametrize("V", [1000, 1001])
def test_head_loss_fixture_keeps_the_clamp_decision_unambiguous(V):
    case = rr.head_loss_case(V)
    want, plain32 = rr.head_loss_ref(case, torch.float64), rr.head_loss_ref(case, torch.float32)
    assert _finite(want) and _finite(plain32)
    p = want["p_label"][want["labelled"]]
    assert not bool(((p >= rr.BAND[0]) & (p <= rr.BAND[1])).any())           # the stated condition of the fixture
    assert bool(torch.equal(want["clamped"], plain32["clamped"]))
    gen = (case["label"] < V)[want["labelled"]]
    for part in (gen, ~gen):                                                 # both parts, both sides of the clamp
        assert int(((p < rr.CLAMP) & part).sum()) >= 2 and int(((p > rr.CLAMP) & part).sum()) >= 2
    near = lambda t: bool(((p > t / 3) & (p < t * 3)).any())
    assert near(1e-12) and near(1e-8) and bool((p > 0.999999).any())
    for t in (1e-12, 1e-8):
        assert bool(((p > t / 3) & (p < t * 3) & gen).any()) and bool(((p > t / 3) & (p < t * 3) & ~gen).any())
    assert bool((p == 0).any())                                              # the copy label on a masked slot
    assert want["ntok"] == int(want["labelled"].sum()) > 20


@pytest.mark.parametrize("c", [1e2, 1e3])
@pytest.mark.parametrize("M", [33, 530])
def test_layernorm_fixture(M, c):
    case = rr.ln_case(M, c)
    s = case["x"] + case["res"]
    want, plain32 = (rr.ln_ref(s, case["gamma"], case["beta"], case["dy"], dt) for dt in (torch.float64, torch.float32))
    assert _finite(want) and _finite(plain32)
    groups = rr.ln_groups(M)
    assert sorted(r for v in groups.values() for r in v) == list(range(M))
    for r in groups["constant"]:                                             # variance exactly 0, in fp32 too
        assert float(s[r].var(unbiased=False)) == 0.0 and float(want["rstd"][r]) == pytest.approx(1e5 ** 0.5, rel=1e-12)
    sd = s.double().std(1)
    assert float((sd[list(groups["std1e-3"])] / 1e-3 - 1).abs().max()) < 0.2
    assert float((sd[list(groups["std1e3"])] / 1e3 - 1).abs().max()) < 0.2
    reg = list(groups["regular"])
    assert float((s.double().mean(1)[reg] / c - 1).abs().max()) < 0.01 and float((sd[reg] / 2 ** 0.5 - 1).abs().max()) < 0.3
    w = rr.zero_mean_rows(rr.randn(64, 256, seed=9))
    assert float((w.double() @ torch.ones(256, dtype=torch.float64)).abs().max()) < 1e-5


def test_row_err_reports_a_single_corrupted_row():
    want = rr.randn(3000, 256, seed=1)
    got = want.clone()
    got[1234] = 0.0                                                         # a row that was never written
    assert rr.row_err(got, want, 1e-6) > 0.5 and rr.rel_err(got, want) < 0.02
    assert rr.row_err(want, want, 1e-6) == 0.0
    z = torch.zeros(4, 8)
    assert rr.row_err(z + 1e-9, z, 1e-6) == pytest.approx(8 ** 0.5 * 1e-3)    # below the floor: compared absolutely
