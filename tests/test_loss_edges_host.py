"""The float64 references and the inputs of tests/test_gpu_loss_edges.py, checked on the CPU (tests/lossutil.py):
  guard / branches  every case's threshold decisions are settled (guard >= 1e-4) and every branch the case is there for is populated;
  anchor            at the golden shapes the float64 references reproduce what the REFERENCE project recorded (loss_dsph, loss_dchmt,
                    dnph + dnph_grads, qmi, spl under tests/golden/), inputs from `recipe` and the *util.py helpers, tolerances those
                    of the existing golden tests - this ties the references to the reference project, not to our kernels;
  float32 spread    e32 = max |float32 - float64| / max |float64| of the same formula evaluated in float32 on the CPU, printed per case
                    and output (run with -s); the GPU module's docstring quotes them next to the kernels' measured errors."""
import numpy as np
import pytest
import torch

import lossutil as L
import recipe


def _fmt(es):
    return " ".join(f"{e:.1e}" for e in es)


# ------------------------------------------------------------------------------------------------------------ guard and branches
@pytest.mark.parametrize("case", L.HYP_CASES)
def test_hyp_case_is_settled_and_populated(case):
    c, fn, tensors, _ = L.problem("hyp", case)
    lab = c["lab"]
    guard = L.hyp_guard(c["x"], c["y"], c["prox"], lab, c["thr"], c["alpha"])
    print(f"hyp {case}: guard {guard:.2e}  e32 (loss, dx, dy, dproxies) {_fmt(L.spread(fn, tensors, L.UPSTREAM['hyp']))}")
    assert guard >= L.GUARD
    assert (lab == 1).any() and (lab == 0).any() and not lab[0].any() and lab[1].sum() >= 3
    prox, pair = L.hyp_decisions(c["x"], c["y"], c["prox"], lab, c["thr"], c["alpha"])
    assert (prox > c["thr"]).any() and (prox < c["thr"]).any()                   # proxy hinge active and inactive
    multi = lab.sum(1) > 1
    assert multi[-1] and ((lab[multi] @ lab[-1]) == 0).any()                      # the last row (a window / tile of its own) pairs
    if c["alpha"] > 0:
        assert pair is not None                                                   # Z > 0: multi-label pairs with disjoint labels
        assert (pair > c["thr"]).any() and (pair < c["thr"]).any()
    else:
        assert pair is None


@pytest.mark.parametrize("case", L.DCHMT_CASES)
def test_dchmt_case_is_settled_and_populated(case):
    c, fn, tensors, _ = L.problem("dchmt", case)
    output_dim, similarity, loss_type, vartheta, thr = c["cfg"]
    guard = L.dchmt_guard(c["img"], c["txt"], c["lab"], *c["cfg"])
    print(f"dchmt {case}: guard {guard:.2e}  e32 (loss, dimg, dtxt) {_fmt(L.spread(fn, tensors, L.UPSTREAM['dchmt']))}")
    assert guard >= L.GUARD
    maxv2 = 2 * output_dim * vartheta
    if similarity == "euclidean":
        assert maxv2 == int(maxv2) and int(maxv2) % 4 != 0                        # distances^2 are multiples of 4
        assert float(c["img"].abs().max()) == 1.0 == float(c["img"].abs().min())
    if loss_type == "l1" and similarity == "cosine":
        assert case[1] % 2 == 1                                                   # 1 - cos is never exactly 1
    assert torch.unique(torch.cat((c["img"], c["txt"])), dim=0).shape[0] == 2 * case[0]     # distinct rows: only (a, a) is at distance 0
    dec = L.dchmt_decisions(c["img"], c["txt"], c["lab"], output_dim, similarity, vartheta, thr)
    pos = torch.cat([v - t for v, t in dec[0::2]])
    neg = torch.cat([v - t for v, t in dec[1::2]])
    assert pos.numel() and neg.numel()                                            # similar and dissimilar pairs
    assert (pos > 0).any() and (neg > 0).any() and (neg < 0).any()                # clamp(max) passing and cutting
    if similarity == "cosine":
        assert (pos < 0).any()                                                    # clamp(min=thr) cutting: a row with itself
    else:
        same = (c["lab"] @ c["lab"].T) > 0
        assert same.diagonal().any()                                              # zero distances among the similar pairs


@pytest.mark.parametrize("case", L.DNPH_CASES)
def test_dnph_case_is_populated(case):
    c, fn, tensors, _ = L.problem("dnph", case)
    lab = c["lab"]
    print(f"dnph {case}: e32 (loss, dhash_img, dhash_txt, dpre_img, dpre_txt, dproxies) {_fmt(L.spread(fn, tensors, L.UPSTREAM['dnph']))}")
    assert (lab == 1).any() and (lab == 0).any() and not lab[0].any() and lab[1].sum() >= 3
    assert (c["noise_i"] is not None) == case[3]
    assert int(lab[1].argmax()) == 0 and (lab.sum(1) > 1).any()                   # argmax of a multi-hot row: the first maximum
    assert len(set(lab.argmax(-1).tolist())) > 1


@pytest.mark.parametrize("family,case,variant", [("qmi", c, None) for c in L.QMI_CASES] +
                         [("spl", c, v) for c in L.SPL_CASES for v in ("same", "cross")])
def test_qmi_and_spl_cases_are_populated(family, case, variant):
    c, fn, tensors, names = L.problem(family, case, variant)
    print(f"{family} {case} {variant or ''}: e32 (loss, {', '.join(names)}) {_fmt(L.spread(fn, tensors, L.UPSTREAM[family]))}")
    lab = c["lab"]
    same = (lab @ lab.T) > 0
    assert (lab.sum(1) > 0).all()                                                 # P_i > 0
    assert same.any(1).all() and (~same).any(1).all() if family == "spl" else (~same).any()     # both sums of every row are populated
    assert (lab.sum(1) > 1).any()


@pytest.mark.parametrize("M,N,K", L.LINEAR_SHAPES)
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("use_mask", [False, True])
def test_linear_case_spread(M, N, K, act, use_mask):
    c = L.linear_case(M, N, K, act, use_mask)
    fn = lambda x, w, b: (L.linear_act(x, w, b, act, c["mask"], L.LINEAR_DROP) * c["dy"].to(x.dtype)).sum()
    y64 = L.linear_act(c["x"].double(), c["w"].double(), c["b"].double(), act, c["mask"], L.LINEAR_DROP)
    y32 = L.linear_act(c["x"], c["w"], c["b"], act, c["mask"], L.LINEAR_DROP)
    ey = float((y32.double() - y64).abs().max() / y64.abs().max())
    print(f"linear {(M, N, K)} act {act} mask {use_mask}: e32 (y, dx, dW, db) {_fmt([ey] + L.spread(fn, [c['x'], c['w'], c['b']])[1:])}")
    if act == 2:                                                                  # relu's own threshold: no unmasked pre-activation near 0
        z = c["x"].double() @ c["w"].double().T + c["b"].double()
        assert float(z.abs()[c["mask"] != 0].min() if use_mask else z.abs().min()) >= L.GUARD
        assert (y64 > 0).any() and (y64 == 0).any()
    if use_mask:
        assert (c["mask"] == 0).any() and (c["mask"] == 1).any()


@pytest.mark.parametrize("B,d", L.BATCHNORM_SHAPES)
def test_batchnorm_case_spread(B, d):
    c = L.batchnorm_case(B, d)
    fn = lambda x, w, b: (L.batchnorm_train(x, w, b, L.BATCHNORM_EPS) * c["dy"].to(x.dtype)).sum()
    y64 = L.batchnorm_train(c["x"].double(), c["w"].double(), c["b"].double(), L.BATCHNORM_EPS)
    y32 = L.batchnorm_train(c["x"], c["w"], c["b"], L.BATCHNORM_EPS)
    ey = float((y32.double() - y64).abs().max() / y64.abs().max())
    r64 = L.batchnorm_running(c["x"].double(), c["rm"].double(), c["rv"].double(), L.BATCHNORM_MOMENTUM)
    r32 = L.batchnorm_running(c["x"], c["rm"], c["rv"], L.BATCHNORM_MOMENTUM)
    er = [float((a.double() - b).abs().max() / b.abs().max()) for a, b in zip(r32, r64)]
    print(f"batchnorm {(B, d)}: e32 (y, running_mean, running_var, dx, dw, db) {_fmt([ey] + er + L.spread(fn, [c['x'], c['w'], c['b']])[1:])}")
    # the module itself states the same thing
    bn = torch.nn.BatchNorm1d(d, eps=L.BATCHNORM_EPS, momentum=L.BATCHNORM_MOMENTUM).double()
    with torch.no_grad():
        bn.weight.copy_(c["w"]), bn.bias.copy_(c["b"]), bn.running_mean.copy_(c["rm"]), bn.running_var.copy_(c["rv"])
    torch.testing.assert_close(bn(c["x"].double()), y64, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(bn.running_mean, r64[0], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(bn.running_var, r64[1], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ anchor: the goldens
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


@pytest.mark.parametrize("B,K,C", [(32, 64, 24), (48, 16, 80), (16, 128, 21), (8, 32, 24)])
def test_hyp_reference_reproduces_the_golden(golden, B, K, C):
    g = golden("loss_dsph.npz")
    tag, seed = f"B{B}_K{K}_C{C}", 21
    x = torch.tanh(_t(recipe.features(B, K, seed, f"dsph_x_{tag}")))
    y = torch.tanh(_t(recipe.features(B, K, seed, f"dsph_y_{tag}")))
    prox = _t(recipe.features(C, K, seed, f"dsph_prox_{tag}"))
    lab = _t(recipe.labels(B, C, seed, p=float(g[f"{tag}_p"]), tag=f"dsph_lab_{tag}"))
    thr, alpha = float(g[f"{tag}_threshold"]), float(g[f"{tag}_alpha"])
    (loss,), grads = L.evaluate(lambda a, b, p: L.hyp_loss(a, b, p, lab, thr, alpha), [x, y, prox])
    assert abs(loss - float(g[f"{tag}_loss"])) < 1e-4
    for got, name in zip(grads, ("gx", "gy", "gprox")):
        np.testing.assert_allclose(got.numpy(), g[f"{tag}_{name}"], rtol=1e-4, atol=1e-6, err_msg=name)


@pytest.mark.parametrize("B,K,C,fn,lt", [(32, 16, 24, "euclidean", "l2"), (32, 16, 24, "cosine", "l2"), (24, 64, 24, "euclidean", "l1"),
                                         (24, 64, 80, "cosine", "l1")])
def test_dchmt_reference_reproduces_the_golden(golden, B, K, C, fn, lt):
    g = golden("loss_dchmt.npz")
    tag, seed = f"B{B}_K{K}_C{C}_{fn}_{lt}", 31
    pairs = lambda z: torch.softmax((2 * _t(z)).view(B, K, 2), -1).reshape(B, 2 * K)       # the select head's pair probabilities
    hi, ht = pairs(recipe.features(B, 2 * K, seed, f"dchmt_zi_{tag}")), pairs(recipe.features(B, 2 * K, seed, f"dchmt_zt_{tag}"))
    lab = _t(recipe.labels(B, C, seed, tag=f"dchmt_lab_{tag}"))
    (loss,), grads = L.evaluate(lambda a, b: L.dchmt_loss(a, b, lab, K, fn, lt, 0.5, 0.1), [hi, ht])
    ref = float(g[f"{tag}_loss"])
    assert abs(loss - ref) < 1e-4 * max(1.0, abs(ref))
    np.testing.assert_allclose(grads[0].numpy(), g[f"{tag}_gi"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(grads[1].numpy(), g[f"{tag}_gt"], rtol=1e-4, atol=1e-7)


def test_dnph_reference_reproduces_the_goldens(golden):
    from heads2util import DNPH_CASES, dnph_case
    g, gn = golden("dnph_grads.npz"), golden("dnph.npz")
    for B, K, C in DNPH_CASES:
        c = dnph_case(B, K, C)
        tag = c["tag"]
        lab, ni, nt = _t(c["lab"]), _t(gn[f"{tag}_noise_i"]), _t(gn[f"{tag}_noise_t"])
        (total, loss1, _), grads = L.evaluate(lambda hi, ht, pi, pt, prox: L.dnph_loss(hi, ht, pi, pt, prox, lab, ni, nt, 1.0, 0.1),
                                              [_t(c[k]) for k in ("hi", "ht", "pi", "pt", "prox")])
        assert abs(loss1 - float(gn[f"{tag}_loss1"])) < 1e-4 * max(1.0, abs(loss1))
        assert abs(total - float(gn[f"{tag}_step_loss"])) < 1e-4 * max(1.0, abs(total))
        assert abs(total - float(g[f"{tag}_step_loss"])) < 1e-4 * max(1.0, abs(total))
        for got, name in zip(grads, ("ghi", "ght", "gpi", "gpt", "gprox")):
            np.testing.assert_allclose(got.numpy(), g[f"{tag}_{name}"], rtol=2e-4, atol=2e-6, err_msg=name)


def test_qmi_reference_reproduces_the_golden(golden):
    from qmiutil import CASES, qmi_case
    g = golden("qmi.npz")
    for B, K, C, p in CASES:
        c = qmi_case(B, K, C, p)
        tag, lab = c["tag"], _t(c["lab"])
        (loss,), grads = L.evaluate(lambda x, t: L.qmi_loss(x, t, lab), [_t(c["x"]), _t(c["y"])])
        want = float(g[f"{tag}_loss"])
        assert abs(loss - want) < 1e-4 * max(1.0, abs(want))
        for got, name in zip(grads, ("gx", "gy")):
            ref = g[f"{tag}_{name}"]
            np.testing.assert_allclose(got.numpy(), ref, rtol=2e-4, atol=2e-5 * np.abs(ref).max(), err_msg=name)


def test_spl_reference_reproduces_the_golden(golden):
    from mslutil import SPL_CASES, spl_case
    g = golden("spl.npz")
    for B, K, C, p, epoch, total in SPL_CASES:
        c = spl_case(B, K, C, p, epoch, total)
        tag, lab = c["tag"], _t(c["lab"])
        third = int(total / 3)
        delta = epoch / third if epoch <= third else 1.0
        three = lambda x, y: tuple(L.spl_loss(a, b, lab, 0.3, delta) for a, b in ((x, x), (y, y), (x, y)))
        fn = lambda x, y: (sum(three(x, y)),) + three(x, y)          # the trainer's sum first: gradients of all three calls
        (_, ii, tt, it), grads = L.evaluate(fn, [_t(c["x"]), _t(c["y"])])
        plain = float(L.spl_loss(_t(c["x"]).double(), _t(c["y"]).double(), lab, 0.3, 0.0))
        for got, name in ((ii, "ii"), (tt, "tt"), (it, "it"), (plain, "it_plain")):
            want = float(g[f"{tag}_loss_{name}"])
            assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (name, got, want)
        for got, name in zip(grads, ("gx", "gy")):
            ref = g[f"{tag}_{name}"]
            np.testing.assert_allclose(got.numpy(), ref, rtol=2e-4, atol=2e-5 * np.abs(ref).max(), err_msg=name)
