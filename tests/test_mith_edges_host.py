"""The float64 references and the inputs of tests/test_gpu_mith_edges.py, checked on the CPU (tests/mithedgeutil.py):
  guard / branches  every case's decisions are settled (guard >= 1e-4; the Bayesian products 1 away from the clamp) and every branch
                    the case is there for is populated;
  anchor            the references reproduce what the REFERENCE project recorded: LocalizedTokenAggregation and BitwiseHashing with
                    their autograd gradients (tests/golden/mith_edges.npz, make_golden19.py), the multi-similarity loss at the golden
                    shapes of msl.npz with the tolerances of tests/test_gpu_msl.py;
  float32 spread    e32 = max |float32 - float64| / max |float64| of the same formula evaluated in float32 on the CPU, printed per case
                    and output (run with -s); the GPU module's docstring quotes them next to the kernels' measured errors;
  sensitivity       for every edge a case is there for, the float64 reference is perturbed the way a kernel would get that edge wrong
                    (the last row / column / candidate of the last trip, slice, quarter or chunk dropped, the top_k-th value without
                    multiplicity, > for >=, l0 ignored, NaN kept, the clamp skipped, one role's gradient instead of two) and a
                    compared output must move by more than 10 x the bound of the GPU test: each case CAN fail."""
import numpy as np
import pytest
import torch

import mithedgeutil as U

TEN_LOSS, TEN_TENSOR = 10 * U.LOSS_BOUND, 10 * U.TENSOR_BOUND


def _fmt(es):
    return " ".join(f"{e:.1e}" for e in es)


def _e32(a32, a64):
    return U.of_max(a32.double(), a64)


def _moves(what, edge, tensors=(), losses=(), rows=False):
    """tensors: (perturbed, reference) pairs, losses likewise: at least one of them moves by more than 10 x its bound"""
    measure = U.per_row if rows else U.of_max
    moved = [measure(p, r) / TEN_TENSOR for p, r in tensors] + [U.loss_err(p, r) / TEN_LOSS for p, r in losses]
    print(f"  sensitivity {what} [{edge}]: {max(moved):.1e} x (10 x bound)")
    assert max(moved) > 1.0, (what, edge, moved)


# ------------------------------------------------------------------------------------------------------------------ LTA
def _lta(c, dtype=torch.float64, **how):
    l0, L, top_k = c["geom"]
    tokens = c["tokens"].detach().clone().to(dtype).requires_grad_(True)
    out = U.lta_forward(tokens, c["sim"], c["kpm"], l0, L, top_k, **how)
    if not bool(torch.isnan(out).any()):
        (U.UPSTREAM["lta"] * (out * c["dmerge"].to(dtype)).sum()).backward()
    return out.detach(), tokens.grad


@pytest.mark.parametrize("case", U.LTA_CASES)
def test_lta_case_is_populated_and_can_fail(case):
    B, Ltot, l0, L, K, D, top_k, with_kpm = case
    c = U.lta_case(*case)
    out, dtok = _lta(c)
    out32, dtok32 = _lta(c, torch.float32)
    _, info = U.lta_weights(c["sim"], c["kpm"], l0, L, top_k)
    print(f"lta {case}: e32 (merge, dtokens) {_fmt([_e32(out32, out), _e32(dtok32, dtok)])}  kept per token {int(info['kept'].min())}.."
          f"{int(info['kept'].max())}  dead columns {int(info['dead'].sum())}")
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dtok).all())
    # the slice: gradients outside it are exact zeros
    assert not dtok[:, :l0].any() and not dtok[:, l0 + L:].any()
    # every case: the last token, the last concept and the last feature column take part
    cut = dict(c, kpm=None if c["kpm"] is None else c["kpm"][:, :L - 1], geom=(l0, L - 1, top_k))
    _moves(f"lta {case}", "last token dropped", [(_lta(cut)[0], out)])
    z = out.clone()
    z[:, K - 1] = 0
    _moves(f"lta {case}", "last concept dropped", [(z, out)])
    z = dtok.clone()
    z[..., D - 1] = 0
    _moves(f"lta {case}", "last feature column dropped", [(z, dtok)])
    if with_kpm and case != U.LTA_HAND:
        assert c["kpm"][1].all() and not out[1].any() and not dtok[1].any()            # the fully masked sample
        assert c["kpm"][B - 1].sum() == 1
        _moves(f"lta {case}", "mask ignored", [(_lta(dict(c, kpm=None))[0], out)])
    if l0 > 0 or L < Ltot:
        _moves(f"lta {case}", "l0 ignored", [(_lta(c, use_l0=False)[0], out)])
    if bool(info["dead"].any()):
        _moves(f"lta {case}", "NaN kept", [(_lta(c, nan_to_zero=False)[0], out)])
    if top_k < 8:
        assert int(info["kept"].max()) < 8                                                # a kernel that always kept 8 would differ
    if case == U.LTA_CASES[0]:
        assert (L, K) == (80, 128) and D % 256 == 4 and bool(info["dead"][1].all())
    if case == U.LTA_CASES[2]:
        assert bool((info["positives"] == 0).any()) and int(info["kept"].max()) == 1
    if case == U.LTA_HAND:
        assert info["kept"][0].tolist() == [4, 5, 2, 0, 3, 0] and info["positives"][0].tolist() == [5, 5, 2, 0, 4, 0]
        assert bool(info["dead"][0, 4]) and bool(info["dead"][0, 11]) and bool((c["sim"][0, l0:l0 + L - 1, 4] > 0).any())
        assert l0 + L < Ltot
        _moves(f"lta {case}", "> for >=", [(_lta(c, tie="gt")[0], out)])
        _moves(f"lta {case}", "top_k-th distinct value", [(_lta(c, tie="distinct")[0], out)])


def test_lta_and_bitwise_hashing_references_reproduce_the_golden(golden):
    g = golden("mith_edges.npz")
    for i, (B, L, K, D, top_k, with_kpm, ties) in enumerate(U.ANCHOR_LTA):
        c = U.anchor_lta_case(i)
        out, dtok = _lta(c)
        _, info = U.lta_weights(c["sim"], c["kpm"], 0, L, top_k)
        np.testing.assert_allclose(out.numpy(), g[f"lta{i}_merge"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(dtok.numpy() / U.UPSTREAM["lta"], g[f"lta{i}_dtokens"], rtol=1e-5, atol=1e-6)
        assert np.array_equal(info["mask"].numpy(), g[f"lta{i}_pseudo"] != 0)
        if ties:
            assert int(info["kept"].max()) > top_k
            assert U.of_max(_lta(c, tie="gt")[0], out) > TEN_TENSOR and U.of_max(_lta(c, tie="distinct")[0], out) > TEN_TENSOR
        if with_kpm:
            assert bool(info["dead"][0, 3]) and not np.any(g[f"lta{i}_merge"][0, 3])
    c = U.anchor_bithash_case()
    leaves = [c[k].double().requires_grad_(True) for k in ("x", "w", "b")]
    y = U.bithash(*leaves)
    y.backward(c["dy"].double())
    for got, name in zip([y.detach()] + [l.grad for l in leaves], ("bh_y", "bh_dx", "bh_dw", "bh_db")):
        np.testing.assert_allclose(got.numpy(), g[name], rtol=1e-5, atol=1e-6, err_msg=name)


# ------------------------------------------------------------------------------------------------------------------ heads
def _bithash(c, dtype=torch.float64, keep=None):
    """keep: (samples, columns) slices a short trip would still read"""
    leaves = [c[k].detach().clone().to(dtype).requires_grad_(True) for k in ("x", "w", "b")]
    x, w, b = leaves
    if keep is not None:
        x, w = x[:, :, :keep], w[:, :keep]
    y = U.bithash(x, w, b)
    (U.UPSTREAM["bithash"] * (y * c["dy"].to(dtype)).sum()).backward()
    return [y.detach()] + [l.grad for l in leaves]


@pytest.mark.parametrize("case", U.BITHASH_CASES)
def test_bithash_case_can_fail(case):
    B, K, D = case
    c = U.bithash_case(*case)
    ref, r32 = _bithash(c), _bithash(c, torch.float32)
    print(f"bithash {case}: e32 (y, dx, dw, db) {_fmt([_e32(a, b) for a, b in zip(r32, ref)])}")
    if D > 4:
        _moves(f"bithash {case}", "last float4 of a row dropped", [(_bithash(c, keep=D - 4)[0], ref[0])])
    z = ref[2].clone()
    z[:, D - 1] = 0
    _moves(f"bithash {case}", "last dw column dropped", [(z, ref[2])])
    last = dict(c, dy=c["dy"].clone())
    last["dy"][B - 1] = 0                                                              # the last sample left out of the sums over samples
    if B > 1:
        pert = _bithash(last)
        _moves(f"bithash {case}", "last sample dropped from dw, db", [(pert[2], ref[2]), (pert[3], ref[3])])
    if case == (5, 16, 512):
        per = (B + 3) // 4
        assert [max(0, min(B, (q + 1) * per) - q * per) for q in range(4)] == [2, 2, 1, 0]
    if case == (261, 4, 68):
        per = (B + 3) // 4
        assert per == 66 and per % 4 == 2 and per > 64


@pytest.mark.parametrize("case", U.L2NORM_CASES)
def test_l2norm_case_can_fail(case):
    R, D = case
    c = U.l2norm_case(*case)
    x, dy = c["x"].double(), c["dy"].double()
    y, dx = U.l2norm(x), U.UPSTREAM["l2norm"] * U.l2norm_dx(x, dy)
    y32, dx32 = U.l2norm(c["x"]), U.UPSTREAM["l2norm"] * U.l2norm_dx(c["x"], c["dy"])
    print(f"l2norm {case}: e32 per row (y, dx) {_fmt([U.per_row(y32, y), U.per_row(dx32, dx)])}")
    leaf = x.clone().requires_grad_(True)
    clamped = torch.linalg.vector_norm(x, dim=-1) <= U.L2_EPS
    U.l2norm(leaf)[~clamped].backward(U.UPSTREAM["l2norm"] * dy[~clamped])               # above the clamp autograd states the same
    assert U.per_row(dx[~clamped], leaf.grad[~clamped]) < 1e-12
    short = torch.cat((U.l2norm(x[:, :D - 1]), torch.zeros(R, 1, dtype=torch.float64)), 1)
    _moves(f"l2norm {case}", "last column dropped", [(short, y)], rows=True)
    if case == (4, 128):
        assert clamped.tolist() == [False, True, True, False] and not x[1].any() and bool(x[2].any())
        assert U.of_max(y[2], x[2] / U.L2_EPS) < 1e-15 and U.of_max(dx[1:3], U.UPSTREAM["l2norm"] * dy[1:3] / U.L2_EPS) < 1e-15
        _moves(f"l2norm {case}", "clamp skipped", [(U.l2norm(x, clamp=False), y)], rows=True)
        proj = (dy - y * (y * dy).sum(-1, keepdim=True)) / U.L2_EPS * U.UPSTREAM["l2norm"]   # the projection kept under the clamp
        assert U.per_row(proj, dx) > 0 and float(dx[2].abs().max()) > 1e10


def test_elementwise_cases_are_settled():
    c = U.mix_case()
    v, Bc, Hi, Ht = U.mith_mix(*(c[k].double() for k in ("ic", "it", "tc", "tt")), U.MIX_LAMBDA)
    v32, _, Hi32, Ht32 = U.mith_mix(c["ic"], c["it"], c["tc"], c["tt"], U.MIX_LAMBDA)
    guard = float(v.abs()[v != 0].min())
    print(f"mith_mix: guard {guard:.2e}  zeros {int((v == 0).sum())}  +1 {int((Bc > 0).sum())}  -1 {int((Bc < 0).sum())}"
          f"  e32 (H_i, H_t) {_fmt([_e32(Hi32, Hi), _e32(Ht32, Ht)])}")
    assert guard >= U.GUARD and bool(((v32 == 0) == (v == 0)).all())                      # the exact zeros are exact in float32 too
    assert int((v == 0).sum()) >= 30 and v[256] == 0 and bool((Bc > 0).any()) and bool((Bc < 0).any())
    both = (v == 0) & (c["ic"] != 0)
    assert bool(both.any()) and bool(((v == 0) & (c["ic"] == 0)).any())
    _moves("mith_mix", "sign(0) = 1", [(torch.where(v >= 0, 1.0, -1.0).double(), Bc)])
    g = U.gelu_case()
    x = g["x"].double().requires_grad_(True)
    y = torch.nn.functional.gelu(x)
    y.backward(g["dy"].double())
    x32 = g["x"].clone().requires_grad_(True)
    y32 = torch.nn.functional.gelu(x32)
    y32.backward(g["dy"])
    print(f"gelu: e32 (y, dx) {_fmt([_e32(y32.detach(), y.detach()), _e32(x32.grad, x.grad)])}")
    assert g["x"][0] == 0 and g["x"][1] == 6 and g["x"][2] == -6 and y[0] == 0
    z = x.grad.clone()
    z[256] = 0
    _moves("gelu", "the element of the second block dropped", [(z, x.grad)])
    for n in U.SQDIFF_SIZES:
        s = U.sqdiff_case(n)
        ref = ((s["a"].double() - s["b"].double()) ** 2).sum()
        e = abs(float(((s["a"] - s["b"]) ** 2).sum()) - float(ref)) / float(ref)
        print(f"sq_diff n = {n}: e32 {e:.1e}")
        if n > U.SQ_GRID:
            first_trip = ((s["a"].double() - s["b"].double())[:U.SQ_GRID] ** 2).sum()
            _moves(f"sq_diff {n}", "second grid-stride trip dropped", losses=[(first_trip, ref)])


# ------------------------------------------------------------------------------------------------------------------ Bayesian loss
def _bayes(c, dtype=torch.float64, **how):
    fn = lambda batch: U.bayes_loss(batch, c["bank"], c["bank_label"], c["label"], **how)
    (v,), (g,) = U.evaluate(fn, [c["batch"]], dtype, U.UPSTREAM["bayes"])
    return v, g


def _bayes_without(c, rows=None, k_last=False, c_last=False):
    """the loss a kernel computes that misses the bank rows `rows` (it still divides by Mb B), the last bit, or the last class"""
    Mb = c["bank"].shape[0]
    keep = torch.ones(Mb, dtype=torch.bool)
    if rows is not None:
        keep[rows] = False
    d = dict(c, bank=c["bank"][keep], bank_label=c["bank_label"][keep])
    if k_last:
        d["bank"] = d["bank"].clone()
        d["bank"][:, -1] = 0
    if c_last:
        d["bank_label"] = d["bank_label"].clone()
        d["bank_label"][:, -1] = 0
    v, g = _bayes(d)
    scale = float(keep.sum()) / Mb
    return v * scale, g * scale


@pytest.mark.parametrize("case", U.BAYES_CASES)
def test_bayes_case_is_settled_and_can_fail(case):
    Mb, B, K, C = case
    c = U.bayes_case(*case)
    guard, far = U.bayes_guard(c["bank"], c["batch"])
    v, g = _bayes(c)
    v32, g32 = _bayes(c, torch.float32)
    print(f"bayes {case}: guard {guard:.2f}  largest product {far:.0f}  e32 (loss, dbatch) {_fmt([U.loss_err(v32, v), _e32(g32, g)])}")
    assert guard >= 1.0 and far >= 65.0
    assert bool(((c["bank_label"] == 0) | (c["bank_label"] == 1)).all()) and bool(((c["label"] == 0) | (c["label"] == 1)).all())
    ls = (c["bank_label"] @ c["label"].T) > 0
    assert bool(ls.any()) and bool((~ls).any())
    vu, gu = _bayes(c, clamp=False)
    _moves(f"bayes {case}", "clamp skipped", [(gu, g)], [(vu, v)])
    vp, gp = _bayes_without(c, rows=[Mb - 1])
    _moves(f"bayes {case}", "last bank row dropped", [(gp, g)], [(vp, v)])
    z = g.clone()
    z[B - 1] = 0
    _moves(f"bayes {case}", "last batch row dropped", [(z, g)])
    per = (Mb + U.BAYES_SLICES - 1) // U.BAYES_SLICES
    if Mb in (1023, 1025):
        assert B % 16 == 1 and (Mb < 1024 or Mb - 15 * per == 50)                         # one slice / sixteen, the last of 50 rows
    if Mb == 5:
        assert per == 1 and Mb < U.BAYES_SLICES                                            # slices 5 .. 15 are empty
    if Mb == 10257:
        assert per == U.BAYES_CHUNK + 2
        vp, gp = _bayes_without(c, rows=[s * per + U.BAYES_CHUNK + i for s in range(15) for i in (0, 1)])
        _moves(f"bayes {case}", "second LDS chunk dropped", [(gp, g)])
    if K % 16:
        vp, gp = _bayes_without(c, k_last=True)
        _moves(f"bayes {case}", "last bit dropped", [(gp, g)], [(vp, v)])
    if C > 128:
        vp, gp = _bayes_without(c, c_last=True)
        _moves(f"bayes {case}", "last class dropped", [(gp, g)], [(vp, v)])


# ------------------------------------------------------------------------------------------------------------------ InfoNCE
@pytest.mark.parametrize("case", U.NCE_CASES)
def test_nce_case_can_fail(case):
    R, G, D = case
    c = U.nce_case(*case)
    fn = lambda a, b: U.info_nce(a, b, G)
    (v,), grads = U.evaluate(fn, [c["a"], c["b"]], upstream=U.UPSTREAM["nce"])
    print(f"nce {case}: e32 (loss, da, db) {_fmt(U.spread(fn, [c['a'], c['b']], U.UPSTREAM['nce'])) if G > 1 else 'exact zeros'}")
    if G == 1:
        assert v == 0.0 and not grads[0].any() and not grads[1].any()
        return
    (vp,), gp = U.evaluate(lambda a, b: U.info_nce(a, b, G, drop_last=True), [c["a"], c["b"]], upstream=U.UPSTREAM["nce"])
    _moves(f"nce {case}", "last candidate of a group dropped", list(zip(gp, grads)), [(vp, v)])
    z = grads[0].clone()
    z[:, D - 1] = 0
    _moves(f"nce {case}", "last feature column dropped", [(z, grads[0])])
    assert (D % 64 == 0) == (case in U.NCE_CASES[:2])                                     # which path the shape selects
    if G == 5:
        per = (G + 3) // 4
        assert 3 * per >= G                                                                # the fourth row quarter is empty


# ------------------------------------------------------------------------------------------------------------------ multi-similarity loss
@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("case", U.MSL_CASES)
def test_msl_case_is_settled_and_can_fail(case, cross):
    B, K, Kl = case[:3]
    c, fn, tensors, names = U.msl_problem(case, cross)
    y = c["x"] if c["y"] is None else c["y"]
    guard = U.msl_guard(c["x"], y, c["code"])
    p = U.msl_parts(c["x"].double(), y.double(), c["code"])
    has = p["has"][:, None]
    cut_pos, cut_neg = int((p["pos_"] & ~p["pos"] & has).sum()), int((p["neg_"] & ~p["neg"] & has).sum())
    zero_row = (B, K, Kl) == U.MSL_ZERO_ROW
    measure = U.per_row if zero_row else U.of_max
    (v,), grads = U.evaluate(fn, tensors, upstream=U.UPSTREAM["msl"])
    (v32,), g32 = U.evaluate(fn, tensors, torch.float32, U.UPSTREAM["msl"])
    print(f"msl {case[:3]} {'cross' if cross else 'self'}: guard {guard:.2e}  valid rows {int(p['valid'].sum())}/{B}  positives cut {cut_pos}"
          f"  negatives cut {cut_neg} kept {int((p['neg'] & p['valid'][:, None]).sum())}  e32 (loss, {', '.join(names)}) "
          f"{_fmt([U.loss_err(v32, v)] + [measure(a, b) for a, b in zip(g32, grads)])}")
    assert guard >= U.GUARD
    assert Kl % 2 == 1 and bool((c["x"].abs() <= 1).all()) and bool((c["code"].abs() == 1).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads) and int(p["valid"].sum()) >= 3 and cut_pos > 0
    if (B, K, Kl) == (7, 1024, 1023):
        assert int(p["valid"].sum()) < B                                                   # a skipped row
    if (B, K, Kl) == (65, 16, 3):
        assert cut_pos >= 10 and cut_neg >= 10
    if zero_row:
        assert not c["x"][0].any() and float(p["norm"][0]) < 1e-12 and bool(p["valid"][0]) and float(grads[0][0].abs().max()) > 1e8
        (vu,), gu = U.evaluate(lambda *t: fn(*t, clamp=False), tensors, upstream=U.UPSTREAM["msl"])
        _moves(f"msl {case[:3]}", "clamp skipped", [(gu[0], grads[0])], rows=True)
    (vp,), gp = U.evaluate(lambda *t: fn(*t, drop_col=B - 1), tensors, upstream=U.UPSTREAM["msl"])
    _moves(f"msl {case[:3]}", "last column j dropped", list(zip(gp, grads)), [(vp, v)], rows=zero_row)
    short = [t.clone() for t in tensors]
    short[-1][:, K - 1] = 0                                                                # the last k of the products S
    (vp,), gp = U.evaluate(fn, short, upstream=U.UPSTREAM["msl"])
    _moves(f"msl {case[:3]}", "last feature k dropped", list(zip(gp, grads)), [(vp, v)], rows=zero_row)
    z = grads[-1].clone()
    z[B - 1] = 0
    _moves(f"msl {case[:3]}", "last row of the column kernel dropped", [(z, grads[-1])], rows=zero_row)
    if not cross:
        fixed = tensors[0].double()
        (_,), once = U.evaluate(lambda x: U.msl_loss(x, fixed, c["code"]), tensors, upstream=U.UPSTREAM["msl"])
        _moves(f"msl {case[:3]}", "one role's gradient instead of two", [(once[0], grads[0])], rows=zero_row)


def test_msl_both_log_terms_weigh_in_the_gradient():
    """in at least one case each of the two log terms alone reaches 1e-2 of max |gradient| (the negative term carries scale 40, the
    positive one scale 2: in most cases the negative term dominates)"""
    best = {"pos": 0.0, "neg": 0.0}
    for case in U.MSL_CASES[:4]:
        for cross in (False, True):
            c, fn, tensors, _ = U.msl_problem(case, cross)
            _, grads = U.evaluate(fn, tensors)
            top = max(float(g.abs().max()) for g in grads)
            for term in ("pos", "neg"):
                _, gt = U.evaluate(lambda *t: fn(*t, term=term), tensors)
                share = max(float(g.abs().max()) for g in gt) / top
                best[term] = max(best[term], share)
                print(f"msl {case[:3]} {'cross' if cross else 'self'}: the {term} term alone reaches {share:.2e} of max |gradient|")
    assert best["pos"] >= 1e-2 and best["neg"] >= 1e-2


def test_msl_reference_reproduces_the_golden(golden):
    from mslutil import CASES, msl_case
    g = golden("msl.npz")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    for B, K, C, p, epoch in CASES:
        c = msl_case(B, K, C, p, epoch)
        tag, code = c["tag"], t(g[f"{c['tag']}_ln_code"])
        three = lambda x, y: (U.msl_loss(x, x, code), U.msl_loss(y, y, code), U.msl_loss(x, y, code))
        fn = lambda x, y: (sum(three(x, y)),) + three(x, y)          # the trainer's sum first: gradients of all three calls
        (_, ii, tt, it), grads = U.evaluate(fn, [t(c["x"]), t(c["y"])])
        for got, name in ((ii, "ii"), (tt, "tt"), (it, "it")):
            want = float(g[f"{tag}_loss_{name}"])
            assert abs(got - want) < 1e-4 * max(1.0, abs(want)), (tag, name, got, want)
        for got, name in zip(grads, ("gx", "gy")):
            ref = g[f"{tag}_{name}"]
            np.testing.assert_allclose(got.numpy(), ref, rtol=2e-4, atol=2e-5 * max(np.abs(ref).max(), 1e-30), err_msg=name)
